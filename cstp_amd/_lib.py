"""ctypes binding of libcstp_hip.so (the C ABI declared in include/cstp_hip.h).

The product path has no CPU fallback: if the HIP library is missing or fails to load this
module raises, loudly, at first use.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_uint32, c_uint64, POINTER, c_char_p, c_double, c_float, c_int32, c_int64, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# CSTP_LIB_PATH: developer override for A/B-ing kernel builds (tools/ab_*.sh); unset in production
LIB_PATH = os.environ.get("CSTP_LIB_PATH") or os.path.join(_HERE, "lib", "libcstp_hip.so")
ABI_VERSION = 18


class ConvDesc(ctypes.Structure):
    """struct cstp_conv_desc (include/cstp_hip.h)."""
    _fields_ = [(n, c_int32) for n in
                ("n", "c", "d", "h", "w", "k", "kt", "kh", "kw", "st", "sh", "sw", "pt", "ph", "pw")]


class InAffine(ctypes.Structure):
    """struct cstp_in_affine: BN(+ReLU) folded into a convolution's gather."""
    _fields_ = [("scale_shift", c_void_p), ("groups", c_int32), ("relu", c_int32)]


class PackRec(ctypes.Structure):
    """struct cstp_pack_rec: one recorded weight-pack launch (cstp_pack_mode / cstp_pack_recorded / cstp_pack_replay)."""
    _fields_ = [("kind", c_int32), ("nblocks", c_int32), ("w", c_void_p), ("dst", c_void_p), ("inv_a", c_void_p),
                ("cells", c_void_p), ("a", c_int32 * 10)]


class GateBranch(ctypes.Structure):
    """struct cstp_gate_branch: one branch of a fused S3D-G self-gating + concat call (cstp_gate_concat_*)."""
    _fields_ = [("x", c_void_p), ("w", c_void_p), ("b", c_void_p), ("dx", c_void_p), ("dw", c_void_p), ("db", c_void_p),
                ("c", c_int32), ("reserved", c_int32)]


class BncBranch(ctypes.Structure):
    """struct cstp_bnc_branch: one branch of a fused I3D BatchNorm + ReLU + concat call (cstp_bnrelu_concat_*)."""
    _fields_ = [("x", c_void_p), ("gamma", c_void_p), ("beta", c_void_p), ("running_mean", c_void_p), ("running_var", c_void_p),
                ("part", c_void_p), ("dx", c_void_p), ("dgamma", c_void_p), ("dbeta", c_void_p), ("dx_absmax", c_void_p),
                ("c", c_int32), ("nsplit", c_int32)]


class ClipMixEntry(ctypes.Structure):
    """struct cstp_clip_mix_entry: one sample of a mixup / CutMix launch (cstp_clip_mix)."""
    _fields_ = [("partner", c_int32), ("mode", c_int32), ("lam", c_float), ("y0", c_int32), ("y1", c_int32), ("x0", c_int32),
                ("x1", c_int32), ("reserved", c_int32)]


class CstpError(RuntimeError):
    pass


_P = c_void_p  # device pointers travel as integers (tensor.data_ptr())

# name -> (restype, argtypes).  Must list EVERY symbol include/cstp_hip.h declares
# (tests/test_abi.py parses the header and checks this table and the .so against it).
SIGNATURES = {
    "cstp_abi_version": (c_int32, []),
    "cstp_last_error": (c_char_p, []),
    "cstp_conv3d_workspace_bytes": (c_size_t, [POINTER(ConvDesc)]),
    "cstp_conv3d_forward": (c_int32, [_P, POINTER(ConvDesc), _P, _P, _P, POINTER(InAffine), _P, _P, c_size_t]),
    "cstp_conv3d_backward_data": (c_int32, [_P, POINTER(ConvDesc), _P, _P, _P, _P, c_size_t]),
    "cstp_conv3d_backward_weight": (c_int32, [_P, POINTER(ConvDesc), _P, POINTER(InAffine), _P, _P, _P, c_size_t]),
    "cstp_conv3d_forward_am": (c_int32, [_P, POINTER(ConvDesc), _P, _P, _P, POINTER(InAffine), _P, _P, c_size_t, _P]),
    "cstp_conv3d_backward_data_am": (c_int32, [_P, POINTER(ConvDesc), _P, _P, _P, _P, c_size_t, _P]),
    "cstp_conv3d_backward_data_acc": (c_int32, [_P, POINTER(ConvDesc), _P, _P, _P, _P, c_size_t, _P, c_int32]),
    "cstp_conv3d_backward_weight_am": (c_int32, [_P, POINTER(ConvDesc), _P, POINTER(InAffine), _P, _P, _P, c_size_t, _P, _P]),
    "cstp_conv3d_backward_weight_acc": (c_int32, [_P, POINTER(ConvDesc), _P, POINTER(InAffine), _P, _P, _P, c_size_t, _P, _P,
                                                 c_int32]),
    "cstp_pack_mode": (c_int32, [c_int32]),
    "cstp_pack_recorded": (c_int32, [POINTER(PackRec), c_int32]),
    "cstp_pack_replay": (c_int32, [_P, _P, _P, c_int32, c_int32]),
    "cstp_pack_register": (c_int32, [POINTER(c_void_p), c_int32, c_int32]),
    "cstp_set_deterministic": (c_int32, [c_int32]),
    "cstp_get_deterministic": (c_int32, []),
    "cstp_gemm_set_split_terms": (c_int32, [c_int32]),
    "cstp_gemm_get_split_terms": (c_int32, []),
    "cstp_conv3d_query_tile": (c_int32, [POINTER(ConvDesc), c_int32, POINTER(c_int32)]),
    "cstp_conv3d_set_tile": (c_int32, [POINTER(ConvDesc), c_int32, POINTER(c_int32)]),
    "cstp_conv3d_get_tile": (c_int32, [POINTER(ConvDesc), c_int32, POINTER(c_int32)]),
    "cstp_conv3d_autotune": (c_int32, [_P, POINTER(ConvDesc), c_int32, _P, _P, _P, _P, c_size_t, c_int32]),
    "cstp_bn_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "cstp_bn_forward_train": (c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32,
                                        c_float, c_float, c_int32, _P, c_size_t]),
    "cstp_bn_forward_train_am": (c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32,
                                           c_float, c_float, c_int32, _P, c_size_t, _P]),
    "cstp_bn_forward_train_pre": (c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32,
                                            c_float, c_float, c_int32, _P, c_size_t, _P, _P, c_int32]),
    "cstp_conv3d_bnstats_nsplit": (c_int32, [POINTER(ConvDesc), c_int32]),
    "cstp_conv3d_bnstats_nsplit_aff": (c_int32, [POINTER(ConvDesc), c_int32]),
    "cstp_conv3d_forward_bnstats": (c_int32, [_P, POINTER(ConvDesc), _P, _P, _P, _P, c_size_t, _P, c_int32, _P, _P, c_size_t,
                                              POINTER(c_int32), _P, _P]),
    "cstp_conv3d_in_affine_fused": (c_int32, [POINTER(ConvDesc), c_int32]),
    "cstp_bn_finalize_pre": (c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_float, c_float,
                                       c_int32, _P, c_int32, _P]),
    "cstp_bn_backward_am": (c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32,
                                      c_int32, _P, c_size_t, _P, c_int32]),
    "cstp_bn1d_backward": (c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_float, c_int32, c_int32]),
    "cstp_bn_stats_train": (c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_float,
                                      c_float, _P, c_size_t]),
    "cstp_bn_backward": (c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32,
                                   c_int32, _P, c_size_t]),
    "cstp_bn_eval_workspace_bytes": (c_size_t, [c_int32]),
    "cstp_bn_forward_eval": (c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_float, c_int32, _P,
                                       c_size_t]),
    "cstp_bn_forward_eval_am": (c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_float, c_int32, _P,
                                          c_size_t, _P]),
    "cstp_avgpool_forward": (c_int32, [_P, _P, _P, c_int32, c_int32]),
    "cstp_avgpool_backward": (c_int32, [_P, _P, _P, c_int32, c_int32]),
    "cstp_maxpool3d_forward": (c_int32, [_P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32),
                                         POINTER(c_int32)]),
    "cstp_maxpool3d_backward": (c_int32, [_P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32),
                                          POINTER(c_int32)]),
    "cstp_channel_sum": (c_int32, [_P, _P, _P, c_int32, c_int32, c_int32, _P, c_size_t]),
    "cstp_byol_loss_forward": (c_int32, [_P, _P, _P, _P, c_int32, c_int32]),
    "cstp_byol_loss_backward": (c_int32, [_P, _P, _P, _P, _P, c_int32, c_int32]),
    "cstp_l2_normalize_forward": (c_int32, [_P, _P, _P, _P, c_int32, c_int32, c_float]),
    "cstp_l2_normalize_backward": (c_int32, [_P, _P, _P, _P, _P, c_int32, c_int32, c_float]),
    "cstp_cross_entropy_forward": (c_int32, [_P, _P, _P, _P, c_int32, c_int32]),
    "cstp_cross_entropy_backward": (c_int32, [_P, _P, _P, _P, _P, c_int32, c_int32]),
    "cstp_soft_cross_entropy_forward": (c_int32, [_P, _P, _P, _P, _P, c_float, _P, c_int32, c_int32]),
    "cstp_soft_cross_entropy_backward": (c_int32, [_P, _P, _P, _P, _P, c_float, _P, _P, c_int32, c_int32]),
    "cstp_ntxent_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "cstp_ntxent_forward": (c_int32, [_P, _P, _P, c_int32, c_int32, c_float, _P, c_size_t]),
    "cstp_ntxent_backward": (c_int32, [_P, _P, _P, _P, c_int32, c_int32, c_float, _P, c_size_t]),
    "cstp_clip_assemble": (c_int32, [_P, _P, c_int32, c_int32, c_int32, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P,
                                     c_int32, _P, _P, c_int32, c_int32, c_int32, _P, _P]),
    "cstp_clip_assemble_u8": (c_int32, [_P, _P, c_int32, c_int32, c_int32, _P, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P,
                                        c_int32, _P, _P, c_int32, c_int32, c_int32, _P, _P]),
    "cstp_clip_rotate": (c_int32, [_P, _P, _P, c_int32, c_int32, c_int32, _P]),
    "cstp_clip_blend": (c_int32, [_P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_float, _P]),
    "cstp_clip_hue": (c_int32, [_P, _P, _P, c_size_t, c_int32, c_int32]),
    "cstp_clip_gray": (c_int32, [_P, _P, _P, c_int32, c_int32, c_int32, _P]),
    "cstp_clip_box_blur": (c_int32, [_P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_uint32, c_uint32, c_int32]),
    "cstp_clip_finish": (c_int32, [_P, _P, _P, c_int32, c_int32, c_int32, c_int32]),
    "cstp_clip_batch_desc_bytes": (c_size_t, []),
    "cstp_clip_batch_forward": (c_int32, [_P, _P, _P, c_int32, c_int32, c_int32, _P, c_int32, _P, c_int64, _P, c_int32, _P,
                                          c_int32]),
    "cstp_clip_mix": (c_int32, [_P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32]),
    # RandAugment layers and the erasing finish of a batch of 8-bit clips (csrc/randaug.h)
    "cstp_randaug_entry_bytes": (c_size_t, []),
    "cstp_randaug_layer": (c_int32, [_P, _P, _P, _P, _P, c_int32, c_int32, c_int32, _P, _P]),
    "cstp_randaug_finish": (c_int32, [_P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32]),
    "cstp_ema_update": (c_int32, [_P, _P, _P, c_size_t, c_double]),
    "cstp_sumsq": (c_int32, [_P, _P, c_size_t, _P, _P, c_size_t]),
    "cstp_clip_coef": (c_int32, [_P, _P, c_float, _P, _P]),
    "cstp_sgd_step": (c_int32, [_P, _P, _P, _P, c_size_t, _P, c_float, c_float, _P, c_int32, c_int32]),
    "cstp_adam_step": (c_int32, [_P, _P, _P, _P, _P, c_size_t, _P, c_float, c_float, c_float, c_float, c_int32, c_int32]),
    "cstp_lars_chunk": (c_int32, []),
    "cstp_lars_workspace_bytes": (c_size_t, [c_int32]),
    "cstp_lars_ratio": (c_int32, [_P, _P, _P, c_size_t, _P, c_int32, _P, c_int32, c_float, c_float, _P, _P, _P, c_size_t]),
    "cstp_lars_step": (c_int32, [_P, _P, _P, _P, c_size_t, _P, c_int32, _P, c_int32, _P, _P, c_float, c_float, _P, c_int32]),
    "cstp_tab_sgd_step": (c_int32, [_P, _P, _P, _P, _P, c_size_t, _P, c_int32, _P, c_int32, _P, c_float, _P, c_int32, c_int32, c_float]),
    "cstp_tab_adam_step": (c_int32, [_P, _P, _P, _P, _P, _P, c_size_t, _P, c_int32, _P, c_int32, _P, c_float, c_float, c_float, c_int32,
                                     c_int32, c_float]),
    # the bf16-storage path (csrc/b16.hip)
    "cstp_b16_cast": (c_int32, [_P, _P, _P, c_size_t]),
    "cstp_b16_conv3d_workspace_bytes": (c_size_t, [POINTER(ConvDesc)]),
    "cstp_b16_conv3d_forward": (c_int32, [_P, POINTER(ConvDesc), _P, _P, _P, _P, c_size_t]),
    "cstp_b16_conv3d_backward_data": (c_int32, [_P, POINTER(ConvDesc), _P, _P, _P, _P, c_size_t]),
    "cstp_b16_conv3d_backward_data_acc": (c_int32, [_P, POINTER(ConvDesc), _P, _P, _P, _P, c_size_t, c_int32]),
    "cstp_b16_conv3d_backward_weight": (c_int32, [_P, POINTER(ConvDesc), _P, _P, _P, _P, c_size_t, c_int32]),
    "cstp_b16_bn_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "cstp_b16_bn_forward_train": (c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32,
                                            c_float, c_float, c_int32, _P, c_size_t]),
    "cstp_b16_bn_backward": (c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32,
                                       c_int32, _P, c_size_t, c_int32]),
    "cstp_b16_bn_forward_eval": (c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_float, c_int32]),
    "cstp_b16_maxpool3d_forward": (c_int32, [_P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32),
                                             POINTER(c_int32), POINTER(c_int32)]),
    "cstp_b16_maxpool3d_backward": (c_int32, [_P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32),
                                              POINTER(c_int32), POINTER(c_int32)]),
    "cstp_b16_avgpool_forward": (c_int32, [_P, _P, _P, c_int32, c_int32]),
    "cstp_b16_avgpool_backward": (c_int32, [_P, _P, _P, c_int32, c_int32]),
    # S3D-G self-gating + inception concat (csrc/gate.hip)
    "cstp_gate_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "cstp_gate_concat_forward": (c_int32, [_P, POINTER(GateBranch), c_int32, c_int32, c_int32, _P, _P, _P, _P]),
    "cstp_gate_concat_backward": (c_int32, [_P, POINTER(GateBranch), c_int32, c_int32, c_int32, _P, _P, _P, _P, c_size_t,
                                            c_int32]),
    # I3D: SAME max-pool, windowed average pool, BatchNorm + ReLU into the inception concat (csrc/mixed.hip)
    "cstp_maxpool3d_same_out": (c_int32, [c_int32, c_int32, c_int32]),
    "cstp_maxpool3d_same_forward": (c_int32, [_P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32),
                                              POINTER(c_int32)]),
    "cstp_maxpool3d_same_backward": (c_int32, [_P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32),
                                               POINTER(c_int32)]),
    "cstp_avgpool3d_window_forward": (c_int32, [_P, _P, _P, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32)]),
    "cstp_avgpool3d_window_backward": (c_int32, [_P, _P, _P, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32)]),
    "cstp_bnrelu_concat_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "cstp_bnrelu_concat_forward": (c_int32, [_P, POINTER(BncBranch), c_int32, c_int32, c_int32, c_int32, c_float, c_float, _P, _P,
                                             _P, _P, _P, c_size_t, _P]),
    "cstp_bnrelu_concat_eval": (c_int32, [_P, POINTER(BncBranch), c_int32, c_int32, c_int32, c_float, _P, _P, _P]),
    "cstp_bnrelu_concat_backward": (c_int32, [_P, POINTER(BncBranch), c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P,
                                              c_size_t, c_int32]),
    # retrieval: streaming similarity top-k (csrc/retrieve.hip)
    "cstp_simtopk_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "cstp_simtopk": (c_int32, [_P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P, _P, c_size_t]),
    # k-NN classification: the weighted vote on a top-k list (csrc/retrieve.hip)
    "cstp_knn_vote": (c_int32, [_P, _P, _P, _P, c_int32, c_int32, c_int32, c_float, c_int32, _P, _P]),
    # fine-tuning regularisers: dropout and the stochastic-depth residual join (csrc/reg.h)
    "cstp_philox4x32_10": (c_int32, [POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32)]),
    "cstp_dropout": (c_int32, [_P, _P, _P, c_int64, c_float, c_uint64, c_uint64]),
    "cstp_droppath_add_relu_forward": (c_int32, [_P, _P, _P, _P, _P, c_int64, c_int64, c_int32, _P]),
    "cstp_droppath_add_relu_backward": (c_int32, [_P, _P, _P, _P, _P, _P, c_int64, c_int64, c_int32]),
    # linear probe on cached features: classifier step and ranking (csrc/probe.h)
    "cstp_probe_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "cstp_probe_step": (c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P,
                                  c_size_t]),
    "cstp_probe_predict": (c_int32, [_P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    # the same for up to 32 classifiers side by side: head = grid dimension (csrc/probe.h)
    "cstp_probe_sweep_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "cstp_probe_sweep_step": (c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P,
                                        _P, _P, _P, c_size_t]),
    "cstp_probe_sweep_score": (c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P,
                                         _P, c_size_t]),
    # NT-Xent with a queue of extra negatives (csrc/ntxq.h)
    "cstp_ntxq_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "cstp_ntxq_forward": (c_int32, [_P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_float, _P, c_size_t]),
    "cstp_ntxq_backward": (c_int32, [_P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_float, _P, c_size_t]),
    "cstp_ntxq_push": (c_int32, [_P, _P, _P, c_int32, c_int32, c_int32, c_int32]),
    # spherical k-means on cached features: assignment and centroid update of all restarts (csrc/kmeans.h)
    "cstp_kmeans_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "cstp_kmeans_assign": (c_int32, [_P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, c_size_t]),
    "cstp_kmeans_update": (c_int32, [_P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    # label-free collapse metrics on cached features: feature Gram matrix and pairwise Gaussian potential (csrc/health.h)
    "cstp_feat_gram_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "cstp_feat_gram": (c_int32, [_P, _P, c_int32, c_int32, _P, _P, _P, c_size_t]),
    "cstp_pair_potential_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "cstp_pair_potential": (c_int32, [_P, _P, c_int32, c_int32, c_float, _P, _P, c_size_t]),
    # few-shot episodic evaluation on cached features: N-way K-shot cosine nearest-centroid episodes (csrc/fewshot.h)
    "cstp_fewshot_episodes": (c_int32, [_P, _P, c_int32, _P, c_int32, c_int32, _P, _P, c_int32, c_int32, c_int32, POINTER(c_int32),
                                        c_int32, _P, _P, _P]),
}

_lib = None


def load() -> ctypes.CDLL:
    """Load libcstp_hip.so (once).  Raises CstpError when it is absent -- there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise CstpError(
            "libcstp_hip.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  cstp_amd has no CPU fallback." % LIB_PATH)
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # missing ROCm runtime etc.
        raise CstpError("failed to load %s: %s" % (LIB_PATH, e)) from e
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise CstpError("libcstp_hip.so lacks symbol %s (stale build?)" % name) from e
        fn.restype = res
        fn.argtypes = args
    ver = lib.cstp_abi_version()
    if ver != ABI_VERSION:
        raise CstpError("libcstp_hip.so ABI version %d != binding %d (rebuild)" % (ver, ABI_VERSION))
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().cstp_last_error()
        raise CstpError("%s failed: %s" % (what, msg.decode() if msg else "unknown error"))

"""I3D-BYOL for MI355X -- host-side mirror of /root/reference/models/BE/i3d_byol.py as models/model.py:66-71 builds it for
``--model_name i3d_byol``: ``I3DBYOL(pretrain=True, opts=opts)`` / ``I3DBYOL(pretrain=False, opts=opts)``.

Mirrors (same class names, attribute names, state-dict keys in the same order, argument meaning and initialisation RNG stream):
  get_fine_tuning_parameters :17-38, get_padding_shape :70-87, Unit3Dpy :99-167 (``conv3d``, ``batch3d``; bias-free everywhere it
  is instantiated), MaxPool3dTFPadding :170-183, Mixed :186-220 (``branch_0``, ``branch_1`` / ``branch_2`` / ``branch_3`` as
  Sequentials), I3D :223-415 (with_classifier False: ``id_head`` = global average pool, flatten, x / ||x||_2; True: ``avg_pool``
  (2, 7, 7) stride 1, ``dropout`` p = 0, ``conv3d_0c_1x1_custom`` = a bare 1024 -> n_classes (7, 1, 1) convolution, squeeze, mean
  over time), Predictor :602-613, I3DBYOL :616-799 (o_type 'loss_com' :748-772, 'ft_fc' / 'ft_all' / 'test' :787-795).
Kept from the reference: target_net is a deepcopy of online_net made BEFORE the Glorot pass (both are re-drawn independently by
the modules() loop, :632-640); the encoder has no projector (the predictor and the target comparison act on the 1024-d
normalised features); the pretext heads are plain Linear layers, overlap 2048 -> 5, playback / rotation 1024 -> 4, the last one
called ``rot_cls``; the fine-tune wrapper has no ``classify`` / ``cls_bn``: its classifier is the encoder's last convolution.
Out of scope: load_tf_weights and the TensorFlow checkpoint helpers (:428-585), the 'flow' modality, the projection id_head.

TensorFlow "SAME" padding (:70-87): per dimension pad = max(k - s, 0), front pad // 2, the rest behind.  The 7x7x7 / stride 2 stem
pads (2, 3): the 3-channel clip is padded with ATen (it needs no gradient and is tiny next to the 64-channel output) and the
convolution runs with padding 0 -- symmetric padding 3 would sample other positions.  1x1x1 and 3x3x3 / stride 1 convolutions are
symmetric (0 / 1) and run on the implicit-GEMM dispatch as they are.  Every max-pooling is one kernel (ops.max_pool3d_same) that
treats the one-sided zero padding as candidates of value 0 instead of copying the activation into a padded tensor.

A Mixed block ends in four train-mode BatchNorm3d + ReLU and a torch.cat: here the four raw convolution outputs go through ONE
fused op (ops.bn_relu_concat) that writes the normalised branches straight into the block's output tensor -- three launches
forward (two where every branch's convolution left its BatchNorm sums, which no I3D layer does today), two backward, no concat copy and no channel-slice copies of the gradient.  ``CSTP_I3D_FUSED=0`` builds the same model
from F.pad + ATen max_pool3d(ceil_mode=True), per-branch ops.batch_norm_act and torch.cat, for same-box comparison.
fp32 activations only: ``--act_dtype bf16`` is refused.
"""
from __future__ import annotations

import copy
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .r21d_byol import BatchNorm1d, BatchNorm3d, ByolBase, Conv3d, Linear, Predictor

# A/B switch (read at import): 0 = SAME pooling and the Mixed tail composed from ATen + the per-branch ops
FUSED = os.environ.get("CSTP_I3D_FUSED", "1") != "0"


def get_fine_tuning_parameters(model, ft_begin_index):
    """The fine-tune plan of i3d_byol.py:17-38, restated.  Index 0 trains everything and hands back ``model.parameters()``.
    Any other index keeps a parameter trainable only if its NAME contains 'layer<i>' for some i in ft_begin_index..4, or 'fc';
    all the others are frozen and enter the optimizer with lr 0.0.  One param group per tensor, in named_parameters() order.
    No I3D parameter name contains either substring, so every non-zero index freezes the whole model (generate_model refuses
    ``--task ft_fc`` for that reason)."""
    if ft_begin_index == 0:
        return model.parameters()
    wanted = ["layer%d" % i for i in range(ft_begin_index, 5)] + ["fc"]
    print("i3d_byol fine-tune plan: parameters named like", wanted, "stay trainable")
    groups = []
    for name, param in model.named_parameters():
        if any(tag in name for tag in wanted):
            groups.append({"params": param})
            continue
        param.requires_grad = False
        groups.append({"params": param, "lr": 0.0})
    return groups


def get_padding_shape(filter_shape, stride):
    """i3d_byol.py:70-87: (front, back) per dimension, returned in ConstantPad3d order with the depth pair moved last."""
    pads = []
    for k, s in zip(filter_shape, stride):
        front, back, _ = ops.same_pool_geometry(max(k, 1), k, s)
        pads += [front, back]
    return tuple(pads[2:] + pads[:2])


def _same_pads(kernel, stride):
    """((front, back) for d, h, w)."""
    return tuple(ops.same_pool_geometry(max(k, 1), k, s)[:2] for k, s in zip(kernel, stride))


def _bump(bn, groups):
    if not getattr(bn, "_nbt_in_arena", False):
        bn.num_batches_tracked += groups      # else: one add per net per forward (ByolBase.flatten_parameters)


class Unit3Dpy(nn.Module):
    """Convolution (SAME or VALID) -> BatchNorm3d -> ReLU (:99-167); ``use_bn`` / ``activation`` None drop the last two."""

    def __init__(self, in_channels, out_channels, kernel_size=(1, 1, 1), stride=(1, 1, 1), activation="relu", padding="SAME",
                 use_bias=False, use_bn=True):
        super().__init__()
        if padding not in ("SAME", "VALID"):
            raise ValueError("Unit3Dpy padding %r: 'SAME' | 'VALID'" % (padding,))
        if activation not in ("relu", None):
            raise ValueError("activation %r: relu | None" % (activation,))
        if use_bn != (activation == "relu"):
            raise NotImplementedError("Unit3Dpy is served as conv -> BatchNorm3d -> ReLU or as a bare convolution (the two forms "
                                      "I3D instantiates)")
        self.padding = padding
        self.use_bn = use_bn
        kernel_size, stride = tuple(kernel_size), tuple(stride)
        pads = _same_pads(kernel_size, stride) if padding == "SAME" else ((0, 0),) * 3
        # a pad that is not symmetric is applied to the input ahead of a pad-0 convolution (the reference's ConstantPad3d, :124-132)
        self.simplify_pad = all(f == b for f, b in pads)
        self._pre_pad = None if self.simplify_pad else (pads[2] + pads[1] + pads[0])
        self.conv3d = Conv3d(in_channels, out_channels, kernel_size, stride=stride,
                             padding=tuple(f for f, _ in pads) if self.simplify_pad else 0, bias=use_bias)
        if use_bn:
            self.batch3d = BatchNorm3d(out_channels)

    def conv(self, x, groups=1):
        """The convolution alone; in train mode it leaves the BatchNorm's partial sums beside its output where its kernel can."""
        if self._pre_pad is not None:
            x = F.pad(x, self._pre_pad)
        if self.use_bn and self.batch3d.training:
            return self.conv3d(x, groups, self.batch3d.running_mean)
        return self.conv3d(x)

    def forward(self, x, groups=1):
        x = self.conv(x, groups)
        if self.use_bn:
            x = self.batch3d(x, relu=True, groups=groups)
        return x


class MaxPool3dTFPadding(nn.Module):
    """ConstantPad3d(SAME pads, 0) -> MaxPool3d(kernel, stride, ceil_mode=True) (:170-183); no state."""

    def __init__(self, kernel_size, stride=None, padding="SAME"):
        super().__init__()
        if padding != "SAME":
            raise NotImplementedError("MaxPool3dTFPadding is served with padding='SAME' (what I3D instantiates)")
        self.kernel_size, self.stride = tuple(kernel_size), tuple(stride)
        self.padding_shape = get_padding_shape(self.kernel_size, self.stride)

    def out_size(self, dhw):
        return tuple(ops.same_pool_geometry(n, k, s)[2] for n, k, s in zip(dhw, self.kernel_size, self.stride))

    def forward(self, x):
        if FUSED:
            return ops.max_pool3d_same(x, self.kernel_size, self.stride)
        return F.max_pool3d(F.pad(x, self.padding_shape), self.kernel_size, self.stride, ceil_mode=True)


class _Branch(nn.Sequential):
    """Sequential(Unit3Dpy | MaxPool3dTFPadding, Unit3Dpy): keys ``branch_1.0.conv3d.weight`` ..."""

    def raw(self, x, groups):
        """Everything but the last unit's BatchNorm + ReLU."""
        first = self[0]
        x = first(x) if isinstance(first, MaxPool3dTFPadding) else first(x, groups)
        return self[1].conv(x, groups)

    def forward(self, x, groups=1):
        return self[1].batch3d(self.raw(x, groups), relu=True, groups=groups)


class Mixed(nn.Module):
    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.branch_0 = Unit3Dpy(in_channels, out_channels[0], kernel_size=(1, 1, 1))
        self.branch_1 = _Branch(Unit3Dpy(in_channels, out_channels[1], kernel_size=(1, 1, 1)),
                                Unit3Dpy(out_channels[1], out_channels[2], kernel_size=(3, 3, 3)))
        self.branch_2 = _Branch(Unit3Dpy(in_channels, out_channels[3], kernel_size=(1, 1, 1)),
                                Unit3Dpy(out_channels[3], out_channels[4], kernel_size=(3, 3, 3)))
        self.branch_3 = _Branch(MaxPool3dTFPadding(kernel_size=(3, 3, 3), stride=(1, 1, 1), padding="SAME"),
                                Unit3Dpy(in_channels, out_channels[5], kernel_size=(1, 1, 1)))
        self.out_channels = out_channels[0] + out_channels[2] + out_channels[4] + out_channels[5]

    def forward(self, x, groups=1):
        xs = [self.branch_0.conv(x, groups), self.branch_1.raw(x, groups), self.branch_2.raw(x, groups),
              self.branch_3.raw(x, groups)]
        bns = [self.branch_0.batch3d, self.branch_1[1].batch3d, self.branch_2[1].batch3d, self.branch_3[1].batch3d]
        if not FUSED:
            return torch.cat([bn(xi, relu=True, groups=groups) for bn, xi in zip(bns, xs)], 1)
        tables = [(bn.weight, bn.bias, bn.running_mean, bn.running_var) for bn in bns]
        if not self.training:
            return ops.bn_relu_concat_eval(xs, tables, bns[0].eps)
        if xs[0].numel() // xs[0].shape[1] // groups <= 1:
            # same failure the reference hits in nn.BatchNorm3d (train mode)
            raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(xs[0].shape),))
        y = ops.bn_relu_concat(xs, tables, groups, bns[0].eps, bns[0].momentum)
        for bn in bns:
            _bump(bn, groups)
        return y


class _IdHead(nn.Module):
    """nn.Sequential(AdaptiveAvgPool3d((1, 1, 1)), Flatten(), Normalize(2)) (:328-341; no state).  Normalize(2) divides by the
    plain L2 norm; ops.l2_normalize clamps the norm at 1e-12, which only matters for an all-zero feature row (NaN in the
    reference)."""

    def forward(self, x):
        return ops.l2_normalize(ops.global_avg_pool(x))


class AvgPool3d(nn.Module):
    """nn.AvgPool3d(kernel_size, stride (1, 1, 1)) stand-in (no state)."""

    def __init__(self, kernel_size, stride=(1, 1, 1)):
        super().__init__()
        if tuple(stride) != (1, 1, 1):
            raise NotImplementedError("AvgPool3d is served with stride 1 (i3d_byol.py:297)")
        self.kernel_size, self.stride = tuple(kernel_size), tuple(stride)

    def forward(self, x):
        return ops.avg_pool3d_window(x, self.kernel_size)


class Dropout(nn.Module):
    """nn.Dropout(p) stand-in (no state); I3DBYOL builds it with p = 0, the identity.  --dropout sets ``p`` and the step's mask
    ``key`` for one training forward (I3DBYOL.regularized): the mask is the counter-based one of ops.dropout, not torch's."""

    def __init__(self, p=0.0):
        super().__init__()
        if p != 0:
            raise NotImplementedError("I3D's classifier dropout is built with p = 0 (i3d_byol.py:227,630); a positive p comes "
                                      "from --dropout per training step, not from the constructor (got %r)" % (p,))
        self.p, self.key = p, None

    def forward(self, x):
        if self.training and self.p > 0 and self.key is not None:
            return ops.dropout(x, self.p, self.key, 0)
        return x


class I3D(nn.Module):
    def __init__(self, num_classes=0, modality="rgb", dropout_prob=0, name="inception", with_classifier=False, projection=False):
        super().__init__()
        self.name = name
        self.num_classes = num_classes
        if modality != "rgb":
            if modality == "flow":
                raise NotImplementedError("the 'flow' modality of I3D is out of scope")
            raise ValueError("I3D modality %r: only 'rgb' is served" % (modality,))
        if projection:
            raise NotImplementedError("I3DBYOL builds I3D(projection=False) (i3d_byol.py:621,630)")
        self.modality = modality
        self.conv3d_1a_7x7 = Unit3Dpy(out_channels=64, in_channels=3, kernel_size=(7, 7, 7), stride=(2, 2, 2), padding="SAME")
        self.maxPool3d_2a_3x3 = MaxPool3dTFPadding(kernel_size=(1, 3, 3), stride=(1, 2, 2), padding="SAME")
        self.conv3d_2b_1x1 = Unit3Dpy(out_channels=64, in_channels=64, kernel_size=(1, 1, 1), padding="SAME")
        self.conv3d_2c_3x3 = Unit3Dpy(out_channels=192, in_channels=64, kernel_size=(3, 3, 3), padding="SAME")
        self.maxPool3d_3a_3x3 = MaxPool3dTFPadding(kernel_size=(1, 3, 3), stride=(1, 2, 2), padding="SAME")
        self.mixed_3b = Mixed(192, [64, 96, 128, 16, 32, 32])
        self.mixed_3c = Mixed(256, [128, 128, 192, 32, 96, 64])
        self.maxPool3d_4a_3x3 = MaxPool3dTFPadding(kernel_size=(3, 3, 3), stride=(2, 2, 2), padding="SAME")
        self.mixed_4b = Mixed(480, [192, 96, 208, 16, 48, 64])
        self.mixed_4c = Mixed(512, [160, 112, 224, 24, 64, 64])
        self.mixed_4d = Mixed(512, [128, 128, 256, 24, 64, 64])
        self.mixed_4e = Mixed(512, [112, 144, 288, 32, 64, 64])
        self.mixed_4f = Mixed(528, [256, 160, 320, 32, 128, 128])
        self.maxPool3d_5a_2x2 = MaxPool3dTFPadding(kernel_size=(2, 2, 2), stride=(2, 2, 2), padding="SAME")
        self.mixed_5b = Mixed(832, [256, 160, 320, 32, 128, 128])
        self.mixed_5c = Mixed(832, [384, 192, 384, 48, 128, 128])
        self.with_classifier = with_classifier
        if with_classifier:
            self.avg_pool = AvgPool3d((2, 7, 7), (1, 1, 1))
            self.dropout = Dropout(dropout_prob)
            self.conv3d_0c_1x1_custom = Unit3Dpy(in_channels=1024, out_channels=self.num_classes, kernel_size=(7, 1, 1),
                                                 activation=None, use_bias=False, use_bn=False)
        else:
            self.projection = projection
            print("No classifier, No projection")
            self.id_head = _IdHead()

    def final_map(self, dhw):
        """(D, H, W) of the mixed_5c output for a clip of ``dhw``: the stem (SAME, stride 2) and the four poolings."""
        dhw = tuple((n + 5 - 7) // 2 + 1 for n in dhw)
        for pool in (self.maxPool3d_2a_3x3, self.maxPool3d_3a_3x3, self.maxPool3d_4a_3x3, self.maxPool3d_5a_2x2):
            dhw = pool.out_size(dhw) if min(dhw) >= 1 else dhw
        return dhw

    def check_clip(self, shape):
        """Raise a clear error instead of a kernel failure for clips the network (or its classifier) cannot take."""
        if len(shape) != 5 or shape[1] != 3:
            raise ValueError("I3D expects clips [B, 3, D, H, W], got %s" % (tuple(shape),))
        fm = self.final_map(tuple(shape[2:]))
        if min(fm) < 1:
            raise ValueError("clip %s is too small for I3D: its stem reduces it to nothing (needs at least 2 frames of 2x2 "
                             "pixels)" % (tuple(shape[1:]),))
        if self.with_classifier:
            if fm[0] < 2 or fm[1] < 7 or fm[2] < 7:
                raise ValueError("clip %s is too small for the I3D classifier: the final map %s is below the (2, 7, 7) average "
                                 "pool (needs at least 10 frames of 194x194 pixels)" % (tuple(shape[1:]), fm))
            if fm[1] != 7 or fm[2] != 7:
                raise ValueError("clip %s: the I3D classifier squeezes a 1x1 spatial map, i.e. a final map of exactly 7x7 "
                                 "(194..225 pixels); got %s" % (tuple(shape[1:]), fm))

    def forward(self, x, groups=1, after_early_stage=None):
        """``groups`` > 1: x holds that many independent forward calls back to back along the batch axis (per-call BN
        statistics).  ``after_early_stage``: called once conv3d_2c_3x3 is enqueued (I3DBYOL starts the target network's stream there)."""
        self.check_clip(x.shape)
        x = self.conv3d_1a_7x7(x, groups)
        x = self.maxPool3d_2a_3x3(x)
        x = self.conv3d_2c_3x3(self.conv3d_2b_1x1(x, groups), groups)
        if after_early_stage is not None:
            after_early_stage()
        x = self.maxPool3d_3a_3x3(x)
        x = self.mixed_3c(self.mixed_3b(x, groups), groups)
        x = self.maxPool3d_4a_3x3(x)
        for m in (self.mixed_4b, self.mixed_4c, self.mixed_4d, self.mixed_4e, self.mixed_4f):
            x = m(x, groups)
        x = self.maxPool3d_5a_2x2(x)
        x = self.mixed_5c(self.mixed_5b(x, groups), groups)
        if self.with_classifier:
            x = self.conv3d_0c_1x1_custom(self.dropout(self.avg_pool(x)))      # [B, n_classes, T, 1, 1]
            return ops.global_avg_pool(x)                                      # squeeze(3), squeeze(3), mean(2)  (:409-411)
        return self.id_head(x)


class I3DBYOL(ByolBase):
    """forward(x1, x2, o_type='loss_com') -> (loss_byol, (pred_spa, pred_tem, pred_pb_1, pred_pb_2, pred_rot_1, pred_rot_2))
    with [B,5], [B,5], [B,4] x4 logits (i3d_byol.py:748-772)."""
    ROT_HEAD = "rot_cls"      # the rotation head's attribute name in this wrapper

    def __init__(self, momentum=0.996, pretrain=True, opts=None):
        super().__init__()
        self.pretrain = bool(pretrain)
        act = getattr(opts, "act_dtype", "fp32") or "fp32"
        if act != "fp32":
            raise ValueError("--act_dtype %r: i3d_byol runs fp32 activations only (bf16 storage is served for r21d_byol / r3d_byol)"
                             % (act,))
        if pretrain:
            self.momentum = momentum
            self.online_net = I3D(with_classifier=False, projection=False)
            self.target_net = copy.deepcopy(self.online_net)       # copied BEFORE the Glorot pass (:622)
            self.predictor = Predictor(dim=1024, prediction_size=1024, prediction_hidden_size=4096)
            self._set_grad(self.target_net, False)
            self.overlap_spa = Linear(2048, 5)
            self.overlap_tem = Linear(2048, 5)
            self.pb_cls = Linear(1024, 4)
            self.rot_cls = Linear(1024, 4)
        else:
            self.online_net = I3D(num_classes=opts.n_classes, with_classifier=True, projection=False)
        self._glorot_all((Linear, Conv3d, BatchNorm1d, BatchNorm3d))   # :632-640 (the deep-copied target is re-drawn too)
        self._arenas = None

    def _head_bn_calls(self):
        return [(self.predictor, 2)]

    def regularized(self, dropout=None, drop_scales=None):
        """--dropout sets the probability (and this step's key) of the encoder's own ``dropout`` module, which sits in front of
        conv3d_0c_1x1_custom; I3D has no residual blocks to drop."""
        if drop_scales:
            raise ValueError("--drop_path: i3d_byol has no residual branch to drop")
        return _I3DDropout(self.online_net.dropout if not self.pretrain else None, dropout)

    def forward(self, x1, x2=None, o_type="r_byol"):
        if o_type == "loss_com":
            return self._two_view_step(x1, x2)
        if o_type == "r_byol":
            raise NotImplementedError("o_type='r_byol' reads an attribute the reference never sets (self.shuffle_bn, "
                                      "i3d_byol.py:777); use o_type='loss_com'")
        if o_type in ["ft_fc", "ft_all", "test"]:
            if self.pretrain:
                raise AttributeError("I3DBYOL(pretrain=True) has no classifier: o_type=%r needs pretrain=False" % o_type)
            out = self.online_net(x1)                              # :787-795: the encoder's own classifier, [B, n_classes]
            if self.training and self._arenas is not None:
                self._arenas["nbt"]["all"] += 1
            return out
        if o_type == "scratch":
            raise AttributeError("I3DBYOL has no `classify`: o_type='scratch' fails in the reference too (i3d_byol.py:796-799); "
                                 "use o_type='ft_all'")
        return None     # the reference falls off the end of forward for any other o_type


class _I3DDropout:
    """I3DBYOL.regularized: (p, key) on the classifier's Dropout module for one forward, p = 0 again afterwards."""

    def __init__(self, module, dropout):
        self.module, self.dropout = module, dropout

    def __enter__(self):
        if self.module is not None and self.dropout is not None:
            self.module.p, self.module.key = self.dropout
        return self.module

    def __exit__(self, *exc):
        if self.module is not None:
            self.module.p, self.module.key = 0, None
        return False

"""Command-line surface of the pre-training driver: the same flat flag namespace as
/root/reference/opts.py:4-245 (same flag names, defaults and types, so the reference's launch
scripts -- README.md:41-50, script/r2p1d/kin400/*.sh -- run unchanged), expressed as a table.

Additions (all optional, defaults reproduce the reference):
  --ntxent_weight   weight of the NT-Xent term on all-gathered projector embeddings (default 0:
                    the reference builds the criterion but never adds it, main_byol.py:71-73,191-197)
  --ntxent_queue    K rows of extra negatives for that term (default 0 = off, today's loss): a FIFO queue of past ONLINE projections,
                    L2-normalised, the all-gathered rows of every step in push order -- identical on every rank without any
                    communication -- read by the streaming kernels of csrc/ntxq.h (no [2N, K] matrix is built).  K must be a
                    multiple of 2 * batch_size; needs --ntxent_weight != 0.  The queue is NOT checkpointed: a resumed run refills
                    it in K / (2 * batch_size) steps (cstp_amd/ntxent.py; every driver but main_byol.py ignores the flag)
  --synthetic_len   samples per epoch of the built-in synthetic dataset (--dataset synthetic)
  --max_steps       stop an epoch after this many iterations (0 = full epoch)
  --bucket_cap_mb   DDP gradient bucket size (xGMI ring all-reduce is per-link bound)
  --act_dtype       fp32 (default) | bf16: storage type of the 5-D activations and their gradients (BASELINE configs[4]:
                    3D-ResNet-50, bf16; both backbones -- cstp_amd/r3d_byol.py, cstp_amd/r21d_byol.py)
  --retrieval_k     the k of R@k for the retrieval driver (retrieval.py), each in 1..64 (default 1 5 10 20 50)
  --retrieval_gallery_len   gallery videos of --dataset synthetic_video in the retrieval driver (queries: --synthetic_len / 4)
  --lars_eta        trust coefficient of --optimizer lars (default 1e-3): each weight tensor's step is scaled by
                    eta * ||w|| / ||g + weight_decay * w||; biases and BatchNorm parameters are neither decayed nor adapted
  --label_smoothing  fine-tuning (main_ft_mp.py): weight eps of the uniform part of the training target, in [0, 1) (default 0)
  --mixup_alpha      fine-tuning: mixup with lam ~ Beta(alpha, alpha), one draw per batch (default 0 = off)
  --cutmix_alpha     fine-tuning: CutMix with lam ~ Beta(alpha, alpha), the box spanning all frames of the clip (default 0 = off)
  --mix_prob         fine-tuning: probability that a batch is mixed at all (default 1)
  --mix_switch_prob  fine-tuning: probability of CutMix when both alphas are positive (default 0.5)
                     (cstp_amd/mix.py; validation keeps the plain cross-entropy; main_byol.py, test.py and retrieval.py
                     ignore all five)
  --dropout          fine-tuning: dropout probability on the classifier's input in train mode, in [0, 1) (default 0 = off); every
                     backbone, ft_fc and ft_all (i3d_byol: the probability of its own dropout module)
  --drop_path        fine-tuning: stochastic depth on the residual blocks of r21d_byol / r3d_byol, in [0, 1) (default 0 = off):
                     block l of L is dropped per sample with P * l / (L - 1); refused for s3d_byol, i3d_byol and --task ft_fc
                     (cstp_amd/regularize.py; validation, main_byol.py, test.py, retrieval.py and knn.py never regularise)
  --randaug_n        fine-tuning: RandAugment operations per TRAINING clip, 0..4 (default 0 = off), drawn uniformly from the 14 of
                     the paper; each equals its Pillow call bit for bit on every frame, fill colour (128, 128, 128)
  --randaug_m        its magnitude m, a float in [0, 30] (default 9)
  --randaug_mstd     each operation's magnitude is min(30, max(0, gauss(m, mstd))), >= 0 (default 0)
  --random_erase     fine-tuning: probability in [0, 1] that a training clip gets one box, through all its frames, erased to
                     uniform noise on [-1, 1) (default 0 = off)
                     (cstp_amd/randaug.py, csrc/randaug.h: one operation table per layer for the whole batch; --dataset
                     synthetic_video | UcfFineTune with --transform_mode img only, refused otherwise; validation and test clips
                     are never augmented; every driver but main_ft_mp.py ignores all four)
  --layer_decay      fine-tuning: layer-wise learning-rate decay D in (0, 1] (default 1 = off): a tensor of layer l of L trains at
                     lr * D ** (L - l) -- the stem is layer 0, residual block b is layer b, the classifier head is layer L;
                     r21d_byol / r3d_byol with --task ft_all | scratch | resume, refused for s3d_byol, i3d_byol and ft_fc
  --wd_skip_1d       fine-tuning: 1 = no weight decay on tensors with dim() <= 1 (biases, BatchNorm gamma / beta) (default 0)
  --model_ema        fine-tuning: momentum M in [0, 1) of an exponential moving average of the weights and BatchNorm statistics
                     (default 0 = off), m = min(M, (1 + t) / (10 + t)) at update t; validation, the plateau metric and the best
                     checkpoint then use the EMA weights, and the checkpoint gains ``state_dict_ema``; every backbone and task
  --lr_schedule      fine-tuning: plateau (default: ReduceLROnPlateau per epoch) | cosine (linear warm-up over --warmup_epochs, then
                     a half cosine to --min_lr, stepped per iteration)
  --warmup_epochs    epochs of linear warm-up of --lr_schedule cosine, >= 0 and fewer than --n_epochs (default 0)
  --min_lr           the rate --lr_schedule cosine ends at, >= 0 (default 0)
  --test_ema         test.py: 1 = test the checkpoint's ``state_dict_ema`` (default 0: ``state_dict``)
                     (cstp_amd/recipe.py, csrc/optim_table.h: one optimiser launch per step whatever the grouping, the EMA in the
                     same pass; --optimizer lars takes --model_ema and refuses --layer_decay / --wd_skip_1d; every driver but
                     main_ft_mp.py and test.py ignores all seven)
  --knn_k           weighted k-NN classification (knn.py, the --knn_every monitor): neighbours per query, 1..64 (default 20)
  --knn_t           its temperature: neighbour j weighs exp((sim_j - sim_0) / T), must be > 0 (default 0.07)
  --knn_every       main_byol.py: after every E-th epoch and after the last, rank 0 classifies the labelled test videos by k-NN
                    on the online encoder and logs top-1 in the ``acc`` column (default 0 = off); --dataset synthetic_video and
                    UcfRepreBYOLSpPre, --sample_size 112 | 224 (main_ft_mp.py, test.py and retrieval.py ignore all three)
  --probe_epochs    linear probe on cached features (linear_probe.py): passes over the gallery features (default 100)
  --probe_batch     its batch size in videos, 0 = one full batch per epoch (default 1024)
  --probe_lr        its peak learning rate, a cosine to 0 over all steps, must be finite and > 0 (default 1e-3)
  --probe_wd        its weight decay on the weight matrix, >= 0 (default 0; decoupled with adam, coupled with sgd)
  --probe_optimizer adam | sgd (momentum 0.9) (default adam); the number of classes is --n_finetune_classes; the defaults are
                    conventional choices, not tuned on real data (every other driver ignores all five)
  --probe_lrs       linear_probe.py: one or more peak learning rates, each finite and > 0, no duplicates (default: not given =
                    no sweep).  Given, the grid --probe_lrs x --probe_wds (lr-major, at most 32 points) is trained side by side
                    on a stratified part of the TRAIN list and scored on the rest of it; the best point (validation top-1, then
                    validation loss, then grid order) is refitted on the whole train list and scored on the test list
  --probe_wds       the grid's weight decays, each finite and >= 0, no duplicates (default: not given = [--probe_wd])
  --probe_val_fraction  the share of every class's train videos held out for the selection, in (0, 0.5] (default 0.2).
                    --probe_wds and --probe_val_fraction are refused without --probe_lrs.  The three are absent from the parsed
                    namespace when not given (opts.probe_grid reads them), so no driver's options dump changes.  The defaults of
                    all eight probe flags remain conventional, untuned choices: no linear-probe accuracy of a trained encoder
                    on real data has been measured with this code
  --cluster_k       k-means clustering evaluation (cluster.py): the number of clusters, >= 0; 0 = --n_finetune_classes (default 0)
  --cluster_iters   its Lloyd iterations per restart, exactly that many (no early stop: nothing is read back), >= 1 (default 50)
  --cluster_restarts  its k-means++ restarts, run side by side in one launch, 1..32; the best final score wins (default 10); the
                    seed is --manual_seed; the defaults are conventional choices, not tuned on real data (every other driver
                    ignores all three)
  --health_every    main_byol.py: after every E-th epoch and after the last, rank 0 computes the label-free collapse metrics of
                    the online encoder on the test-list videos (cstp_amd/health.py: std_ratio, erank, rankme, top1_share,
                    uniformity, nn_sim), prints ``Health epoch N: ...`` and appends a JSON line to health.jsonl in the run's
                    result folder (default 0 = off); the data sets and sizes of --knn_every; it extracts its own features even
                    where --knn_every fires in the same epoch; the epoch log is unchanged
  --health_t        the t of the uniformity term exp(-t |x_i - x_j|^2) (health.py, --health_every), finite and > 0 (default 2).
                    Both are absent from the parsed namespace when not given (opts.health_opts reads them), so no driver's
                    options dump changes; every driver but main_byol.py and health.py ignores them
  --fewshot_way     few-shot episodic evaluation (fewshot.py): classes per episode, 2..20 (default 5)
  --fewshot_shot    its shot counts, one to four values in 1..16, strictly ascending (default 1 5); the counts are nested -- the
                    K-shot prototype is the sum of the first K support videos of the same episode -- so they are paired
  --fewshot_query   query videos per class and episode, 1..32, with way x query <= 320 (default 15)
  --fewshot_episodes  random episodes, 1..2^20 (default 10000); accuracy is the mean over them, +- 1.96 std / sqrt(episodes)
  --fewshot_seed    seed of the episode sampler's private generator, >= 0 (default 0): equal flags give equal episodes.
                    Support videos come from the train list, queries from the test list (cstp_amd/fewshot.py, csrc/fewshot.h:
                    one launch for all episodes).  All five are absent from the parsed namespace when not given
                    (opts.fewshot_opts reads them), so no driver's options dump changes; every driver but fewshot.py ignores
                    them.  The defaults are the literature's conventions, not tuned: no few-shot accuracy of a trained encoder
                    on real data has been measured with this code
torchrun passes LOCAL_RANK through the environment instead of --local_rank; both are honoured.
"""
from __future__ import annotations

import argparse
import os

# (flag, default, type, help) -- type None means store_true
_FLAGS = [
    # datasets
    ("frame_dir", "dataset/HMDB51/", str, "root of the frame folders: <frame_dir>/<Class>/<v_name>/%05d.jpg, 1-based"),
    ("annotation_path", "dataset/HMDB51_labels", str, "folder of trainlist0{split}_nframe.txt / testlist0{split}_nframe.txt "
     "(lines 'Class/v_name.avi <label> <n_frames>')"),
    ("dataset", "HMDB51", str, "UcfRepreBYOLSpPre (main_byol.py) | UcfFineTune (main_ft_mp.py, test.py): UCF-style frame folders, JPEGs "
     "decoded on --n_workers CPU threads, clips assembled on the GPU | synthetic | synthetic_video (HBM-resident videos, clips "
     "assembled on the GPU: pre-training, fine-tuning with --transform_mode img, video test with --transform_mode img_test); "
     "the LMDB / Kinetics names are refused"),
    ("split", 1, str, "split id (HMDB51 / UCF101): picks trainlist0{split}_nframe.txt / testlist0{split}_nframe.txt"),
    ("modality", "RGB", str, "RGB | Flow"),
    ("input_channels", 3, int, "3 | 2"),
    ("n_classes", 400, int, "number of classes"),
    ("n_finetune_classes", 51, int, "number of classes when fine-tuning"),
    # model
    ("model_name", "resnext", str, "backbone (this package: r21d_byol | r3d_byol | s3d_byol | i3d_byol)"),
    ("model_depth", 101, int, "r21d_byol: 1 -> (1,1,1,1), 18 -> (2,2,2,2), 34 -> (3,4,6,3); r3d_byol: 10..152; "
                                        "s3d_byol / i3d_byol: ignored (only names the checkpoint arch)"),
    ("resnet_shortcut", "B", str, "shortcut type of resnet (A | B)"),
    ("resnext_cardinality", 32, int, "ResNeXt cardinality"),
    ("ft_begin_index", 0, int, "first block to fine-tune"),
    ("sample_size", 112, int, "clip height and width"),
    ("sample_duration", 16, int, "clip length in frames"),
    ("batch_size", 32, int, "GLOBAL batch size (split over ranks)"),
    ("n_workers", 4, int, "dataloader workers; for the frame-folder data sets the JPEG decode threads (at least 1, at most 16)"),
    ("pretrained_path", "", str, "pretrained checkpoint"),
    ("test_md_path", "", str, "checkpoint to test"),
    ("resume_md_path", "", str, "checkpoint to resume"),
    # optimiser
    ("learning_rate", 3e-4, float, "peak learning rate"),
    ("momentum", 0.9, float, "SGD momentum"),
    ("dampening", 0.9, float, "accepted for compatibility; the reference never passes it to SGD"),
    ("weight_decay", 1e-4, float, "weight decay"),
    ("nesterov", False, None, "accepted for compatibility; unused by the reference driver"),
    ("optimizer", "sgd", str, "sgd | adamw | adam | lars (flat-arena HIP kernels; lars: SGD with momentum and per-tensor trust "
     "ratios, see --lars_eta)"),
    ("lr_patience", 10, int, "ReduceLROnPlateau patience (fine-tune only)"),
    ("n_epochs", 400, int, "epochs"),
    # logging / misc
    ("result_path", "", str, "output directory"),
    ("log", True, None, "kept for compatibility"),
    ("manual_seed", 1, int, "random seed"),
    ("random_seed", 1, bool, "kept for compatibility"),
    ("cuda", False, None, "set by the driver"),
    ("device", None, str, "set by the driver"),
    ("tau", 8, int, "slow-path stride (other backbones)"),
    ("alpha", 4, int, "fast/slow frame-rate ratio (other backbones)"),
    ("input_h", 128, int, "input height before crop"),
    ("input_w", 171, int, "input width before crop"),
    ("temperature", 0.5, float, "NT-Xent temperature"),
    ("task", "r_ctr", str, "loss_com | r_byol | ..."),
    ("temp_transform", "speed/random/periodic/warp", str, "temporal transforms"),
    ("lr_decay", 1e-4, float, "learning rate decay"),
    ("local_rank", -1, int, "GPU rank (torch.distributed.launch); env LOCAL_RANK also honoured"),
    ("rank", -1, int, "process rank"),
    ("dist_url", "env://", str, "rendezvous url"),
    ("dist_backend", "nccl", str, "nccl (= RCCL on ROCm) | gloo"),
    ("world_size", -1, int, "set by the driver from WORLD_SIZE"),
    ("nprocs", -1, int, "set by the driver"),
    ("distributed", False, None, "set by the driver"),
    ("sync_bn", 1, int, "kept: the reference's SyncBN spans a one-rank group, i.e. per-GPU BN either way"),
    ("clip_grad_norm", 1, int, "1 = clip_grad_norm_(., 18)"),
    ("split_path", "", str, "training list path"),
    ("pb_rate", 4, int, "playback rate of a clip 1,2,4,8"),
    ("transform_mode", "numpy", str, "transform mode; --dataset synthetic_video and UcfFineTune serve img (validation: img_val) and img_test"),
    ("input_size", 320, int, "input size"),
    ("output_feat", 128, int, "output feature size"),
    ("norm_method", "tf_norm", str, "input normalisation"),
    ("max_iter", 80000, int, "maximum iterations"),
    ("t_ft_task", "", str, "fine-tune task for test"),
    ("sc_type", "B", str, "resnet shortcut type"),
    ("lmdb_path", "", str, "LMDB path"),
    # additions
    ("ntxent_weight", 0.0, float, "weight of the NT-Xent term on all-gathered embeddings (0 = reference)"),
    ("ntxent_queue", 0, int, "main_byol.py: rows of the NT-Xent term's queue of past online projections used as extra negatives "
     "(0 = off; a multiple of 2 * batch_size; needs --ntxent_weight; not checkpointed)"),
    ("synthetic_len", 256, int, "samples per epoch for --dataset synthetic"),
    ("max_steps", 0, int, "stop each epoch after this many iterations (0 = all)"),
    ("bucket_cap_mb", 25, int, "DDP gradient bucket size in MB"),
    ("act_dtype", "fp32", str, "fp32 | bf16: activation storage type (r21d_byol and r3d_byol; s3d_byol and i3d_byol are fp32 only)"),
    ("retrieval_gallery_len", 64, int, "retrieval.py with --dataset synthetic_video: number of gallery videos"),
    ("lars_eta", 1e-3, float, "--optimizer lars: trust coefficient eta of the per-tensor ratio eta * |w| / |g + weight_decay * w|"),
    ("label_smoothing", 0.0, float, "main_ft_mp.py: label smoothing eps of the training loss, in [0, 1) (0 = hard labels)"),
    ("mixup_alpha", 0.0, float, "main_ft_mp.py: mixup, lam ~ Beta(alpha, alpha) once per batch (0 = off)"),
    ("cutmix_alpha", 0.0, float, "main_ft_mp.py: CutMix, lam ~ Beta(alpha, alpha) once per batch, one box through all frames (0 = off)"),
    ("mix_prob", 1.0, float, "main_ft_mp.py: probability that a batch is mixed (with --mixup_alpha / --cutmix_alpha)"),
    ("mix_switch_prob", 0.5, float, "main_ft_mp.py: probability of CutMix instead of mixup when both alphas are positive"),
    ("dropout", 0.0, float, "main_ft_mp.py: dropout probability in front of the classifier, in [0, 1) (0 = off)"),
    ("drop_path", 0.0, float, "main_ft_mp.py: stochastic depth on the residual blocks of r21d_byol / r3d_byol, linear rule, in [0, 1) (0 = off)"),
    ("randaug_n", 0, int, "main_ft_mp.py: RandAugment operations per training clip, 0..4 (0 = off)"),
    ("randaug_m", 9.0, float, "main_ft_mp.py: RandAugment magnitude, in [0, 30]"),
    ("randaug_mstd", 0.0, float, "main_ft_mp.py: standard deviation of the per-operation magnitude gauss(m, mstd) clipped to [0, 30], >= 0"),
    ("random_erase", 0.0, float, "main_ft_mp.py: probability in [0, 1] that a training clip gets a box erased to noise (0 = off)"),
    ("layer_decay", 1.0, float, "main_ft_mp.py: layer-wise learning-rate decay in (0, 1] for r21d_byol / r3d_byol (1 = off)"),
    ("wd_skip_1d", 0, int, "main_ft_mp.py: 1 = no weight decay on biases and BatchNorm parameters (tensors with dim() <= 1)"),
    ("model_ema", 0.0, float, "main_ft_mp.py: momentum in [0, 1) of the weight EMA that is validated and checkpointed (0 = off)"),
    ("lr_schedule", "plateau", str, "main_ft_mp.py: plateau (ReduceLROnPlateau per epoch) | cosine (warm-up + cosine per iteration)"),
    ("warmup_epochs", 0, int, "main_ft_mp.py: warm-up epochs of --lr_schedule cosine, >= 0 and fewer than --n_epochs"),
    ("min_lr", 0.0, float, "main_ft_mp.py: final learning rate of --lr_schedule cosine, >= 0"),
    ("test_ema", 0, int, "test.py: 1 = load the checkpoint's state_dict_ema (written under --model_ema)"),
    ("knn_every", 0, int, "main_byol.py: k-NN top-1 of the online encoder after every E-th epoch and after the last (0 = off)"),
]
RETRIEVAL_MAX_K = 64      # ops.SIM_TOPK_MAX_K: one lane per list slot


def _retrieval_k(text):
    k = int(text)
    if not 1 <= k <= RETRIEVAL_MAX_K:
        raise argparse.ArgumentTypeError("--retrieval_k takes values in 1..%d, got %d" % (RETRIEVAL_MAX_K, k))
    return k


def _knn_k(text):
    k = int(text)
    if not 1 <= k <= RETRIEVAL_MAX_K:
        raise argparse.ArgumentTypeError("--knn_k takes values in 1..%d, got %d" % (RETRIEVAL_MAX_K, k))
    return k


def _knn_t(text):
    t = float(text)
    if not (t > 0.0 and t < float("inf")):
        raise argparse.ArgumentTypeError("--knn_t must be finite and > 0, got %r" % (text,))
    return t


def _probe_epochs(text):
    e = int(text)
    if e < 1:
        raise argparse.ArgumentTypeError("--probe_epochs must be >= 1, got %d" % e)
    return e


def _probe_batch(text):
    b = int(text)
    if b < 0:
        raise argparse.ArgumentTypeError("--probe_batch must be >= 0 (0 = full batch), got %d" % b)
    return b


def _probe_lr(text):
    v = float(text)
    if not (v > 0.0 and v < float("inf")):
        raise argparse.ArgumentTypeError("--probe_lr must be finite and > 0, got %r" % (text,))
    return v


def _probe_wd(text):
    v = float(text)
    if not (v >= 0.0 and v < float("inf")):
        raise argparse.ArgumentTypeError("--probe_wd must be finite and >= 0, got %r" % (text,))
    return v


PROBE_MAX_GRID = 32          # ops.PROBE_MAX_HEADS: the grid point is a grid dimension of the kernels
PROBE_VAL_FRACTION = 0.2


def _probe_val_fraction(text):
    v = float(text)
    if not (v > 0.0 and v <= 0.5):
        raise argparse.ArgumentTypeError("--probe_val_fraction must be in (0, 0.5], got %r" % (text,))
    return v


def probe_grid(args):
    """-> None without --probe_lrs, else (lrs, wds, val_fraction) with the defaults filled in: [--probe_wd] and 0.2."""
    lrs = getattr(args, "probe_lrs", None)
    if lrs is None:
        return None
    return list(lrs), list(getattr(args, "probe_wds", [args.probe_wd])), getattr(args, "probe_val_fraction", PROBE_VAL_FRACTION)


def _check_probe_grid(parser, args):
    lrs, wds = getattr(args, "probe_lrs", None), getattr(args, "probe_wds", None)
    if lrs is None:
        for flag in ("probe_wds", "probe_val_fraction"):
            if hasattr(args, flag):
                parser.error("--%s selects nothing without --probe_lrs" % flag)
        return
    for flag, vals in (("probe_lrs", lrs), ("probe_wds", wds or [])):
        if len(set(vals)) != len(vals):
            parser.error("--%s: duplicate values in %r" % (flag, vals))
    if len(lrs) * len(wds or [0.0]) > PROBE_MAX_GRID:
        parser.error("--probe_lrs x --probe_wds: %d grid points, at most %d train side by side"
                     % (len(lrs) * len(wds or [0.0]), PROBE_MAX_GRID))


HEALTH_T = 2.0               # cstp_amd.health.DEFAULT_T: Wang & Isola's choice


def _health_every(text):
    return int(text)          # main_byol.check_health_opts refuses a negative value with the monitor's own message


def _health_t(text):
    t = float(text)
    if not (t > 0.0 and t < float("inf")):
        raise argparse.ArgumentTypeError("--health_t must be finite and > 0, got %r" % (text,))
    return t


def health_opts(args):
    """-> (health_every, health_t) with the defaults filled in: 0 (off) and 2.0."""
    return getattr(args, "health_every", 0), getattr(args, "health_t", HEALTH_T)


# ops.FEWSHOT_*: the limits of cstp_fewshot_episodes
FEWSHOT_MAX_WAY, FEWSHOT_MAX_QUERY, FEWSHOT_MAX_SLOTS, FEWSHOT_MAX_SHOTS, FEWSHOT_MAX_SHOT, FEWSHOT_MAX_EPISODES = 20, 32, 320, 4, 16, 1 << 20
FEWSHOT_DEFAULTS = (5, (1, 5), 15, 10000, 0)      # way, shots, queries per class, episodes, seed: the literature's conventions


def _int_in(flag, lo, hi):
    def parse(text):
        v = int(text)
        if not lo <= v <= hi:
            raise argparse.ArgumentTypeError("--%s takes values in %d..%d, got %d" % (flag, lo, hi, v))
        return v
    return parse


def fewshot_opts(args):
    """-> (way, shots, queries per class, episodes, seed) with the defaults filled in: 5, (1, 5), 15, 10000, 0."""
    way, shots, query, episodes, seed = FEWSHOT_DEFAULTS
    return (getattr(args, "fewshot_way", way), tuple(getattr(args, "fewshot_shot", shots)), getattr(args, "fewshot_query", query),
            getattr(args, "fewshot_episodes", episodes), getattr(args, "fewshot_seed", seed))


def _check_fewshot(parser, args):
    way, shots, query, _, _ = fewshot_opts(args)
    if len(shots) > FEWSHOT_MAX_SHOTS:
        parser.error("--fewshot_shot: at most %d shot counts, got %r" % (FEWSHOT_MAX_SHOTS, list(shots)))
    if any(b <= a for a, b in zip(shots, shots[1:])):
        parser.error("--fewshot_shot: the shot counts must be strictly ascending, got %r" % (list(shots),))
    if way * query > FEWSHOT_MAX_SLOTS:
        parser.error("--fewshot_way x --fewshot_query: %d query slots per episode, at most %d" % (way * query, FEWSHOT_MAX_SLOTS))


CLUSTER_MAX_RESTARTS = 32    # ops.KMEANS_MAX_RESTARTS: the restart is a grid dimension of the kernels


def _cluster_k(text):
    k = int(text)
    if k < 0:
        raise argparse.ArgumentTypeError("--cluster_k must be >= 0 (0 = --n_finetune_classes), got %d" % k)
    return k


def _cluster_iters(text):
    v = int(text)
    if v < 1:
        raise argparse.ArgumentTypeError("--cluster_iters must be >= 1, got %d" % v)
    return v


def _cluster_restarts(text):
    v = int(text)
    if not 1 <= v <= CLUSTER_MAX_RESTARTS:
        raise argparse.ArgumentTypeError("--cluster_restarts takes values in 1..%d, got %d" % (CLUSTER_MAX_RESTARTS, v))
    return v


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="CSTP pre-training on MI355X")
    for name, default, typ, text in _FLAGS:
        if typ is None:
            parser.add_argument("--" + name, action="store_true", help=text)
            parser.set_defaults(**{name: default})
        else:
            parser.add_argument("--" + name, default=default, type=typ, help=text)
    parser.add_argument("--highest_val", default={"name": 0}, type=dict, help="best validation score store")
    parser.add_argument("--loss_weight", default=1.0, nargs="+", type=float,
                        help="weights of (byol, spatial overlap, temporal overlap, playback rate, rotation)")
    parser.add_argument("--retrieval_k", default=[1, 5, 10, 20, 50], nargs="+", type=_retrieval_k,
                        help="retrieval.py: the k of R@k, each in 1..%d" % RETRIEVAL_MAX_K)
    parser.add_argument("--knn_k", default=20, type=_knn_k,
                        help="knn.py / --knn_every: neighbours per query, 1..%d" % RETRIEVAL_MAX_K)
    parser.add_argument("--knn_t", default=0.07, type=_knn_t, help="knn.py / --knn_every: temperature of the vote, > 0")
    parser.add_argument("--probe_epochs", default=100, type=_probe_epochs, help="linear_probe.py: epochs over the gallery features")
    parser.add_argument("--probe_batch", default=1024, type=_probe_batch, help="linear_probe.py: batch size, 0 = full batch")
    parser.add_argument("--probe_lr", default=1e-3, type=_probe_lr, help="linear_probe.py: peak learning rate (cosine to 0), > 0")
    parser.add_argument("--probe_wd", default=0.0, type=_probe_wd, help="linear_probe.py: weight decay on the weight matrix, >= 0")
    parser.add_argument("--probe_optimizer", default="adam", choices=("adam", "sgd"), help="linear_probe.py: the update rule")
    # absent from the namespace unless given: the options dump of every driver stays as it is (probe_grid reads them)
    parser.add_argument("--probe_lrs", default=argparse.SUPPRESS, nargs="+", type=_probe_lr,
                        help="linear_probe.py: sweep these peak learning rates (x --probe_wds, at most %d points) on a hold-out "
                             "of the train list and refit the best" % PROBE_MAX_GRID)
    parser.add_argument("--probe_wds", default=argparse.SUPPRESS, nargs="+", type=_probe_wd,
                        help="linear_probe.py: the sweep's weight decays (default: --probe_wd); needs --probe_lrs")
    parser.add_argument("--probe_val_fraction", default=argparse.SUPPRESS, type=_probe_val_fraction,
                        help="linear_probe.py: share of each class's train videos held out for the selection, in (0, 0.5] "
                             "(default %g); needs --probe_lrs" % PROBE_VAL_FRACTION)
    parser.add_argument("--cluster_k", default=0, type=_cluster_k,
                        help="cluster.py: number of k-means clusters, 0 = --n_finetune_classes")
    parser.add_argument("--cluster_iters", default=50, type=_cluster_iters,
                        help="cluster.py: Lloyd iterations per restart, >= 1 (a conventional choice, not tuned on real data)")
    parser.add_argument("--cluster_restarts", default=10, type=_cluster_restarts,
                        help="cluster.py: k-means++ restarts, 1..%d, the best final score wins (a conventional choice, not tuned "
                             "on real data)" % CLUSTER_MAX_RESTARTS)
    # absent from the namespace unless given, like the probe grid: the options dump stays as it is (health_opts reads them)
    parser.add_argument("--health_every", default=argparse.SUPPRESS, type=_health_every,
                        help="main_byol.py: label-free collapse metrics of the online encoder on the test-list videos after every "
                             "E-th epoch and after the last (0 = off, the default); runs its own feature extraction even when "
                             "--knn_every fires in the same epoch")
    parser.add_argument("--health_t", default=argparse.SUPPRESS, type=_health_t,
                        help="health.py / --health_every: t of the uniformity term, finite and > 0 (default %g)" % HEALTH_T)
    # absent from the namespace unless given, like the health flags (fewshot_opts reads them)
    parser.add_argument("--fewshot_way", default=argparse.SUPPRESS, type=_int_in("fewshot_way", 2, FEWSHOT_MAX_WAY),
                        help="fewshot.py: classes per episode, 2..%d (default %d)" % (FEWSHOT_MAX_WAY, FEWSHOT_DEFAULTS[0]))
    parser.add_argument("--fewshot_shot", default=argparse.SUPPRESS, nargs="+", type=_int_in("fewshot_shot", 1, FEWSHOT_MAX_SHOT),
                        help="fewshot.py: one to %d shot counts in 1..%d, strictly ascending, nested within an episode (default 1 5)"
                             % (FEWSHOT_MAX_SHOTS, FEWSHOT_MAX_SHOT))
    parser.add_argument("--fewshot_query", default=argparse.SUPPRESS, type=_int_in("fewshot_query", 1, FEWSHOT_MAX_QUERY),
                        help="fewshot.py: query videos per class and episode, 1..%d, way x query <= %d (default %d)"
                             % (FEWSHOT_MAX_QUERY, FEWSHOT_MAX_SLOTS, FEWSHOT_DEFAULTS[2]))
    parser.add_argument("--fewshot_episodes", default=argparse.SUPPRESS, type=_int_in("fewshot_episodes", 1, FEWSHOT_MAX_EPISODES),
                        help="fewshot.py: random episodes, 1..2^20 (default %d; a convention of the literature, not tuned)"
                             % FEWSHOT_DEFAULTS[3])
    parser.add_argument("--fewshot_seed", default=argparse.SUPPRESS, type=_int_in("fewshot_seed", 0, (1 << 63) - 1),
                        help="fewshot.py: seed of the episode sampler, >= 0 (default %d)" % FEWSHOT_DEFAULTS[4])
    return parser


def parse_opts(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    _check_probe_grid(parser, args)
    _check_fewshot(parser, args)
    if args.local_rank == -1 and "LOCAL_RANK" in os.environ:   # torchrun / torch.distributed.run
        args.local_rank = int(os.environ["LOCAL_RANK"])
    return args

"""Host side of the GPU clip assembly (libcstp_hip.so: cstp_clip_assemble): coefficient tables of Pillow's bicubic resize,
the launch, and a clip-pair builder / dataset that turns decoded uint8 videos resident in HBM into the reference's training
sample ``([clip_1, clip_2], [spa_label, tem_label, pb_label, [rot_label_1, rot_label_2]])`` (datasets.py:855-857) with the
decisions of cstp_amd.sampler.

Replaces the reference's per-worker PIL pipeline, both its `null_transform` path and its `base_transform` path (small-angle
rotation, colour jitter, channel gray, Gaussian blur on the resized 8-bit frames: preprocess_data.py:1110-1121) -- (Image.open -> transpose -> crop -> resize ->
flip -> ToTensor -> normalise on the CPU, 6 DataLoader workers per GPU, preprocess_data.py:1103-1130): the frames are uploaded
once as uint8 and every clip is produced where it is consumed.  There is no CPU implementation here.

The fine-tune / validation / video-test side (UcfFineTune, datasets.py:952-1097, under the 'img' / 'img_val' / 'img_test' transforms)
is the second half of this file: ``assemble_batch`` (cstp_clip_batch_forward: a whole batch or test video in two launches),
``GpuLabelledVideos`` and ``GpuLabelledLoader``.
"""
from __future__ import annotations

import ctypes
import math
import random
from functools import lru_cache
from typing import List

import numpy as np
import torch

from . import _lib, randaug, sampler
from ._lib import check

PRECISION_BITS = 32 - 8 - 2        # Pillow: libImaging/Resample.c


def _bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@lru_cache(maxsize=4096)
def resize_tables(in_size: int, out_size: int):
    """(ksize, bounds int32 [out][2], coefficients int32 [out][ksize]) of Image.resize(..., BICUBIC) along one axis of length
    in_size -> out_size: Resample.c precompute_coeffs (double arithmetic, same operation order) + normalize_coeffs_8bpc."""
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in k:
            ww += w
        for x in range(xmax):
            v = k[x] / ww if ww != 0.0 else k[x]
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return ksize, bounds, kk


_dev_tables = {}


def _device_tables(in_size: int, out_size: int, device: torch.device):
    key = (in_size, out_size, device.index)
    t = _dev_tables.get(key)
    if t is None:
        if len(_dev_tables) > 8192:
            _dev_tables.clear()
        ks, b, k = resize_tables(in_size, out_size)
        t = (ks, torch.from_numpy(b).to(device), torch.from_numpy(k).to(device), int(b[0, 0]), int(b[-1, 0] + b[-1, 1]))
        _dev_tables[key] = t
    return t


# ---- the base_transform branch: host-side constants of the Pillow algorithms the kernels reproduce --------------------------
def rotate_coeffs(w: int, h: int, angle: float):
    """Image.rotate(angle)'s reverse affine matrix about (w / 2, h / 2) (PIL/Image.py) as Geometry.c affine_fixed's six 16.16
    fixed-point coefficients; None for the angles Image.rotate serves by a transpose or a copy."""
    a = angle % 360.0
    if a == 0 or a == 180 or (a in (90, 270) and w == h):
        return None
    r = -math.radians(a)
    m = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0, round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]
    cx, cy = w / 2, h / 2
    m[2] = m[0] * (-cx) + m[1] * (-cy) + m[2] + cx
    m[5] = m[3] * (-cx) + m[4] * (-cy) + m[5] + cy

    def fix(v):
        return int(math.floor(v * 65536.0 + 0.5))
    return [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def gaussian_box_weights(sigma: float, passes: int = 3):
    """ImageFilter.GaussianBlur(sigma) -> (integer box radius, ww, fw) of BoxBlur.c: _gaussian_blur_radius in its float / double
    mix, then the two 24-bit fixed-point weights of ImagingLineBoxBlur8 (a float division)."""
    f32, f64 = np.float32, np.float64
    sigma2 = f32(f32(sigma) * f32(sigma) / f32(passes))
    big_l = f32(math.sqrt(12.0 * f64(sigma2) + 1.0))
    small_l = f32(math.floor((f64(big_l) - 1.0) / 2.0))
    a = f32(f64(f32(2) * small_l + f32(1)) * (f64(small_l * (small_l + f32(1))) - 3.0 * f64(sigma2)))
    a = f32(a / f32(f32(6) * f32(sigma2 - (small_l + f32(1)) * (small_l + f32(1)))))
    radius = f32(small_l + a)
    r_int = int(radius)
    ww = int(f32(1 << 24) / f32(radius * f32(2) + f32(1)))
    fw = ((1 << 24) - (r_int * 2 + 1) * ww) // 2
    return r_int, ww, fw


def _u8_clip(t):
    if not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3:
        raise _lib.CstpError("expected a uint8 [T, H, W, 3] clip on a HIP device (cstp_amd has no CPU path)")
    return t.contiguous()


def clip_rotate(clip: torch.Tensor, angle: float) -> torch.Tensor:
    """Every frame of the clip through Image.rotate(angle) (RandomRotation, preprocess_data.py:1091-1094)."""
    clip = _u8_clip(clip)
    t, h, w, _ = clip.shape
    a = angle % 360.0
    coef = rotate_coeffs(w, h, angle)
    if coef is None:      # Image.rotate's fast paths: copy / transpose
        return clip.clone() if a == 0 else torch.rot90(clip, {90: 1, 180: 2, 270: 3}[int(a)], dims=(1, 2)).contiguous()
    out = torch.empty_like(clip)
    check(_lib.load().cstp_clip_rotate(torch.cuda.current_stream().cuda_stream, clip.data_ptr(), out.data_ptr(), t, h, w,
                                       (ctypes.c_int32 * 6)(*coef)), "cstp_clip_rotate")
    return out


_BLEND_MODE = {"brightness": 0, "contrast": 1, "saturation": 2}


def clip_colour(clip: torch.Tensor, op: str, factor: float) -> torch.Tensor:
    """torchvision adjust_brightness / adjust_contrast / adjust_saturation / adjust_hue on every frame (ClipColorJitter)."""
    clip = _u8_clip(clip)
    t, h, w, _ = clip.shape
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    out = torch.empty_like(clip)
    if op == "hue":
        if not -0.5 <= factor <= 0.5:
            raise ValueError("hue_factor is not in [-0.5, 0.5]")
        shift = int(np.array(factor * 255).astype(np.uint8))
        check(lib.cstp_clip_hue(st, clip.data_ptr(), out.data_ptr(), t * h * w, shift, 0), "cstp_clip_hue")
        return out
    if op not in _BLEND_MODE:
        raise ValueError("colour operation %r" % (op,))
    if factor == 1.0:      # Image.blend returns a copy of the image
        return clip.clone()
    means = torch.empty(t, dtype=torch.int32, device=clip.device) if op == "contrast" else None
    check(lib.cstp_clip_blend(st, clip.data_ptr(), out.data_ptr(), t, h, w, _BLEND_MODE[op], float(factor),
                              None if means is None else means.data_ptr()), "cstp_clip_blend")
    return out


def clip_gray(clip: torch.Tensor, channels) -> torch.Tensor:
    """ClipRandomGray.grayscale: frame i keeps channels[i] in all three channels."""
    clip = _u8_clip(clip)
    t, h, w, _ = clip.shape
    if len(channels) != t:
        raise ValueError("%d channel choices for %d frames" % (len(channels), t))
    ch = torch.tensor([int(c) for c in channels], dtype=torch.int32, device=clip.device)
    out = torch.empty_like(clip)
    check(_lib.load().cstp_clip_gray(torch.cuda.current_stream().cuda_stream, clip.data_ptr(), out.data_ptr(), t, h, w,
                                     ch.data_ptr()), "cstp_clip_gray")
    return out


def clip_gaussian_blur(clip: torch.Tensor, sigma: float) -> torch.Tensor:
    """Every frame through ImageFilter.GaussianBlur(radius=sigma) (ClipGaussianBlur)."""
    clip = _u8_clip(clip)
    if sigma == 0:
        return clip.clone()
    t, h, w, _ = clip.shape
    r_int, ww, fw = gaussian_box_weights(sigma)
    out, tmp = clip.clone(), torch.empty_like(clip)
    check(_lib.load().cstp_clip_box_blur(torch.cuda.current_stream().cuda_stream, out.data_ptr(), tmp.data_ptr(), t, h, w, r_int,
                                         ww, fw, 3), "cstp_clip_box_blur")
    return out


def clip_finish(clip: torch.Tensor, flip: bool, out: torch.Tensor = None) -> torch.Tensor:
    """[flip] -> ToTensor -> 'tf' normalise: uint8 [T][S][S][3] -> fp32 [3][T][S][S] (into ``out``, if given)."""
    clip = _u8_clip(clip)
    t, h, w, _ = clip.shape
    if out is None:
        out = torch.empty((3, t, h, w), dtype=torch.float32, device=clip.device)
    elif out.shape != (3, t, h, w) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != clip.device:
        raise ValueError("out must be a contiguous fp32 [3, %d, %d, %d] tensor on %s" % (t, h, w, clip.device))
    check(_lib.load().cstp_clip_finish(torch.cuda.current_stream().cuda_stream, clip.data_ptr(), out.data_ptr(), t, h, w,
                                       1 if flip else 0), "cstp_clip_finish")
    return out


def apply_base_transform(clip: torch.Tensor, base: "sampler.BasePlan", flip: bool, out: torch.Tensor = None) -> torch.Tensor:
    """base_transform (preprocess_data.py:1110-1121) on the resized 8-bit clip, in Compose order (into ``out``, if given)."""
    clip = clip_rotate(clip, base.angle)
    for op, factor in (base.jitter or ()):
        clip = clip_colour(clip, op, factor)
    if base.gray is not None:
        clip = clip_gray(clip, base.gray)
    if base.blur_sigma is not None:
        clip = clip_gaussian_blur(clip, base.blur_sigma)
    return clip_finish(clip, flip, out)


def assemble_clip(frames: torch.Tensor, plan: "sampler.ClipPlan", size: int) -> torch.Tensor:
    """frames: uint8 [F][H][W][3] on a HIP device -> fp32 [3][T][size][size] (torch.stack(clip).transpose(0, 1)).
    A plan that carries base_transform draws (plan.base) is resized to 8-bit frames first and taken through that branch."""
    lib = _lib.load()
    if not frames.is_cuda or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise _lib.CstpError("frames must be a uint8 [F, H, W, 3] tensor on a HIP device (cstp_amd has no CPU path)")
    frames = frames.contiguous()
    f, h, w, _ = frames.shape
    x0, y0, x1, y1 = plan.box
    if not (x0 < x1 and y0 < y1):
        raise _lib.CstpError("empty crop box %s" % (plan.box,))
    dev = frames.device
    ksh, bh, kh, _, _ = _device_tables(x1 - x0, size, dev)
    ksv, bv, kv, first, last = _device_tables(y1 - y0, size, dev)
    t = len(plan.frames)
    idx = torch.tensor(plan.frames, dtype=torch.int32, device=dev)
    tmp = torch.empty((t, last - first, size, 3), dtype=torch.uint8, device=dev)
    if getattr(plan, "base", None) is not None:
        u8 = torch.empty((t, size, size, 3), dtype=torch.uint8, device=dev)
        check(lib.cstp_clip_assemble_u8(torch.cuda.current_stream().cuda_stream, frames.data_ptr(), f, h, w, idx.data_ptr(), t,
                                        int(plan.rotate), int(x0), int(y0), int(size), kh.data_ptr(), bh.data_ptr(), ksh,
                                        kv.data_ptr(), bv.data_ptr(), ksv, first, last - first, tmp.data_ptr(), u8.data_ptr()),
              "cstp_clip_assemble_u8")
        return apply_base_transform(u8, plan.base, plan.flip)
    out = torch.empty((3, t, size, size), dtype=torch.float32, device=dev)
    check(lib.cstp_clip_assemble(torch.cuda.current_stream().cuda_stream, frames.data_ptr(), f, h, w, idx.data_ptr(), t,
                                 int(plan.rotate), int(x0), int(y0), int(size), 1 if plan.flip else 0, kh.data_ptr(), bh.data_ptr(),
                                 ksh, kv.data_ptr(), bv.data_ptr(), ksv, first, last - first, tmp.data_ptr(), out.data_ptr()),
          "cstp_clip_assemble")
    return out


def assemble_pair(frames: torch.Tensor, plan: "sampler.PairPlan", size: int):
    """-> ([clip_1, clip_2], [spa_label, tem_label, pb_label, [rot_label_1, rot_label_2]])  (datasets.py:855-857)."""
    return ([assemble_clip(frames, plan.clip_1, size), assemble_clip(frames, plan.clip_2, size)],
            [plan.spa_label, plan.tem_label, plan.pb_label, list(plan.rot_labels)])


class GpuVideoClips:
    """Stands in for UcfRepre / Kin400RepreLMDB on synthetic data: ``n_videos`` decoded videos (uint8 frames, smooth moving
    patterns) live in HBM; batch(i) draws clip pairs with cstp_amd.sampler and assembles them on the device.  Selected by the
    pre-training driver with ``--dataset synthetic_video``."""

    def __init__(self, device, n_videos=4, frames=96, height=128, width=171, sample_duration=16, sample_size=112, length=256,
                 seed=1):
        self.device, self.t, self.size, self.length, self.seed = torch.device(device), sample_duration, sample_size, length, seed
        g = torch.Generator(device=self.device).manual_seed(seed)
        ys = torch.linspace(0, 1, height, device=self.device).view(1, height, 1, 1)
        xs = torch.linspace(0, 1, width, device=self.device).view(1, 1, width, 1)
        ts = torch.linspace(0, 1, frames, device=self.device).view(frames, 1, 1, 1)
        self.videos = []
        for v in range(n_videos):
            ph = torch.rand(3, generator=g, device=self.device).view(1, 1, 1, 3) * 6.28
            fr = 2 + 3 * torch.rand(3, generator=g, device=self.device).view(1, 1, 1, 3)
            img = 0.5 + 0.35 * torch.sin(6.28 * (fr * xs + (v + 1) * ys) + ph + 6.28 * ts) \
                + 0.15 * torch.rand((frames, height, width, 3), generator=g, device=self.device)
            self.videos.append((img.clamp(0, 1) * 255).to(torch.uint8).contiguous())

    def __len__(self):
        return self.length

    def sample(self, index: int):
        rng = random.Random(self.seed * 1000003 + index)
        np_rng = np.random.RandomState((self.seed * 1000003 + index) & 0x7fffffff)      # ClipRandomGray's np.random.choice
        video = self.videos[index % len(self.videos)]
        f, h, w, _ = video.shape
        return assemble_pair(video, sampler.sample_pair(f, w, h, self.t, rng, np_rng=np_rng), self.size)

    def batch(self, indices: List[int]):
        """-> (clip_1 [B,3,T,S,S], clip_2, spa, tem, pb, rot_1, rot_2) on the device, labels int64."""
        samples = [self.sample(i) for i in indices]
        c1 = torch.stack([s[0][0] for s in samples])
        c2 = torch.stack([s[0][1] for s in samples])
        lab = lambda f: torch.tensor([f(s[1]) for s in samples], dtype=torch.int64, device=self.device)  # noqa: E731
        return (c1, c2, lab(lambda l: l[0]), lab(lambda l: l[1]), lab(lambda l: l[2]), lab(lambda l: l[3][0]),
                lab(lambda l: l[3][1]))


class GpuClipLoader:
    """DataLoader + DistributedSampler for GpuVideoClips in one object: per epoch an epoch-seeded permutation of the sample
    indices, this rank's stride of it (utils.py:109-113 semantics: shuffle, drop_last, per-rank batch), batches assembled on the
    device in the reference's collated layout ``([clip_1, clip_2], [spa, tem, pb, [rot_1, rot_2]])``.  No worker processes and
    no host->device copy: the training loop's ``.to(device)`` calls are no-ops on these tensors."""

    def __init__(self, dataset: GpuVideoClips, batch_size: int, rank: int = 0, world_size: int = 1, seed: int = 0):
        self.dataset, self.batch_size, self.rank, self.world_size, self.seed, self.epoch = dataset, batch_size, rank, world_size, \
            seed, 0
        if batch_size < 1 or not 0 <= rank < world_size:
            raise ValueError("batch_size %r, rank %r of %r" % (batch_size, rank, world_size))

    def set_epoch(self, epoch: int):
        self.epoch = epoch

    def indices(self) -> List[int]:
        order = list(range(len(self.dataset)))
        random.Random(self.seed * 7919 + self.epoch).shuffle(order)
        per_rank = len(order) // self.world_size                  # every rank the same count (no padding duplicates)
        return order[self.rank:per_rank * self.world_size:self.world_size]

    def __len__(self):
        return (len(self.dataset) // self.world_size) // self.batch_size

    def __iter__(self):
        idx = self.indices()
        for b in range(len(self)):
            c1, c2, spa, tem, pb, r1, r2 = self.dataset.batch(idx[b * self.batch_size:(b + 1) * self.batch_size])
            yield [c1, c2], [spa, tem, pb, [r1, r2]]


# ---- batched assembly (libcstp_hip.so: cstp_clip_batch_forward) and the fine-tune / validation / video-test data path ----------
# struct cstp_clip_batch_desc (include/cstp_hip.h), packed by hand into the pinned upload buffer
_BATCH_DESC = np.dtype([(n, "<u8") for n in ("frames", "kh", "bh", "kv", "bv")] + [("tmp_off", "<i8")]
                       + [(n, "<i4") for n in ("f", "h", "w", "idx_off", "box_x0", "box_y0", "ksh", "ksv", "rw", "rh", "win_x",
                                               "win_y", "row_first", "rows", "flip", "out_slot", "out8_slot", "rot")])


def window_rows(in_size: int, out_size: int, origin: int, size: int):
    """(first, count) of the input rows that the vertical taps of output rows [origin, origin + size) read."""
    _, b, _ = resize_tables(in_size, out_size)
    first = int(b[origin, 0])
    return first, int(b[origin + size - 1, 0] + b[origin + size - 1, 1]) - first


def assemble_batch(videos, plans, size: int, out: torch.Tensor = None) -> torch.Tensor:
    """A whole batch of clips in two launches: plans[i] (``sampler.FtClipPlan``, or any plan with ``frames`` and ``box``; optional
    ``resized`` (w, h), ``window`` (x, y), ``jitter``, ``flip``) cut from videos[i] (uint8 [F][H][W][3] on one HIP device; a single
    tensor serves every plan) -> fp32 [B][3][T][size][size], written straight into the batch tensor (``out``, if given).  Clips
    may come from videos of different frame sizes.  Descriptors and frame indices travel in ONE pinned upload; nothing is
    allocated per clip.  Clips with colour jitter leave the resize as 8-bit frames and go on through cstp_clip_blend / _hue /
    _finish, one transform per clip (ClipColorJitter)."""
    plans = list(plans)
    if len(plans) == 0:
        raise ValueError("assemble_batch needs at least one plan")
    for p in plans:
        if getattr(p, "rotate", 0) or getattr(p, "base", None) is not None:
            raise ValueError("assemble_batch serves crop / scale / window / jitter plans; rotated and base_transform clips go "
                             "through assemble_clip")
    jittered = [i for i, p in enumerate(plans) if getattr(p, "jitter", None)]
    if any(getattr(p, "randaug", None) or getattr(p, "erase", None) is not None for p in plans):
        return _assemble_augmented(videos, plans, size, out, jittered)
    out, u8 = _batch_forward(videos, plans, size, out, jittered)
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    t = len(plans[0].frames)
    for j, i in enumerate(jittered):
        clip = u8[j]
        for op, factor in plans[i].jitter:
            clip = clip_colour(clip, op, factor)
        check(lib.cstp_clip_finish(st, clip.data_ptr(), out[i].data_ptr(), t, size, size, 1 if getattr(plans[i], "flip", False) else 0),
              "cstp_clip_finish")
    return out


def _assemble_augmented(videos, plans, size: int, out, jittered):
    """assemble_batch when some plan carries ``randaug`` or ``erase``: EVERY clip leaves the resize as 8-bit frames in slot i of one
    buffer, jittered clips take today's per-clip colour calls on their slot first (the jitter precedes RandAugment in the
    transform), then ``augment_batch`` serves the whole buffer.  The operation tables ride in the descriptor upload."""
    flips = [bool(getattr(p, "flip", False)) for p in plans]
    packed = randaug.tables(plans, flips, size)
    out, u8, tables = _batch_forward_with(videos, plans, size, out, list(range(len(plans))), packed)
    for i in jittered:
        clip = u8[i]
        for op, factor in plans[i].jitter:
            clip = clip_colour(clip, op, factor)
        u8[i].copy_(clip)
    augment_batch(u8, plans, out, flips, tables=tables)
    return out


def augment_batch(u8: torch.Tensor, plans, out: torch.Tensor, flips, tables=None):
    """RandAugment layers and the erasing finish over a batch of 8-bit clips: u8 [n][t][s][s][3] (uint8, one HIP device), clip i
    under ``plans[i].randaug`` ([(operation, value)], cstp_amd.randaug) -> [flip if flips[i]] -> tensor -> ``plans[i].erase``
    -> out[i] (fp32 [n][3][t][s][s]).  Per layer one cstp_randaug_layer (a statistics launch only when some clip's operation is
    AutoContrast, Equalize or Contrast, and the apply launch), then one cstp_randaug_finish: at most 2 L + 1 launches for L layers,
    whatever n is.  The twin buffer, the look-up tables and the means are allocated once per call; ``u8`` is the other half of the
    ping-pong and is overwritten from the second layer on.  ``tables``: (pinned host bytes, their device copy) of
    ``randaug.tables(plans, flips, s)`` when the caller has uploaded them already.
    -> (out, the 8-bit clips after the last layer: ``u8`` or its twin)."""
    lib = _lib.load()
    plans = list(plans)
    if not u8.is_cuda or u8.dtype != torch.uint8 or u8.dim() != 5 or u8.shape[4] != 3 or u8.shape[2] != u8.shape[3] \
            or not u8.is_contiguous():
        raise _lib.CstpError("expected contiguous uint8 [N, T, S, S, 3] clips on a HIP device (cstp_amd has no CPU path)")
    n, t, s = int(u8.shape[0]), int(u8.shape[1]), int(u8.shape[2])
    if len(plans) != n or len(flips) != n:
        raise ValueError("%d plans and %d flips for %d clips" % (len(plans), len(flips), n))
    if out.shape != (n, 3, t, s, s) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != u8.device:
        raise ValueError("out must be a contiguous fp32 [%d, 3, %d, %d, %d] tensor on %s" % (n, t, s, s, u8.device))
    if lib.cstp_randaug_entry_bytes() != randaug.ENTRY.itemsize or randaug.FINISH_ENTRY.itemsize != randaug.ENTRY.itemsize:
        raise _lib.CstpError("cstp_randaug_entry is %d bytes in the library, %d here"
                             % (lib.cstp_randaug_entry_bytes(), randaug.ENTRY.itemsize))
    layers = randaug.n_layers(plans)
    if tables is None:
        packed = randaug.tables(plans, flips, s)
        host = torch.empty(packed.size, dtype=torch.uint8, pin_memory=True)
        host.numpy()[:] = packed
        dev = torch.empty(packed.size, dtype=torch.uint8, device=u8.device)
        dev.copy_(host, non_blocking=True)
    else:
        host, dev = tables
    step = n * randaug.ENTRY.itemsize
    if host.numel() != (layers + 1) * step or dev.numel() != host.numel():
        raise ValueError("operation tables of %d bytes for %d layers of %d clips" % (host.numel(), layers, n))
    ops = host.numpy()[:layers * step].view(randaug.ENTRY)["op"]
    stats = bool(np.isin(ops, (randaug.RA_AUTOCONTRAST, randaug.RA_EQUALIZE, randaug.RA_CONTRAST)).any())
    lut = torch.empty((n, t, 3, 256), dtype=torch.uint8, device=u8.device) if stats else None
    mean = torch.empty((n, t), dtype=torch.int32, device=u8.device) if stats else None
    st = torch.cuda.current_stream().cuda_stream
    src, dst = u8, (torch.empty_like(u8) if layers else None)
    for l in range(layers):
        check(lib.cstp_randaug_layer(st, src.data_ptr(), dst.data_ptr(), dev.data_ptr() + l * step, host.data_ptr() + l * step, n, t, s,
                                     None if lut is None else lut.data_ptr(), None if mean is None else mean.data_ptr()),
              "cstp_randaug_layer")
        src, dst = dst, src
    check(lib.cstp_randaug_finish(st, src.data_ptr(), out.data_ptr(), dev.data_ptr() + layers * step, host.data_ptr() + layers * step,
                                  n, t, s, n), "cstp_randaug_finish")
    return out, src


def _batch_forward(videos, plans, size: int, out, eight_bit):
    """``_batch_forward_with`` without a payload -> (out, u8)."""
    return _batch_forward_with(videos, plans, size, out, eight_bit, None)[:2]


def _batch_forward_with(videos, plans, size: int, out, eight_bit, extra):
    """The descriptor table, its one pinned upload and the two launches of cstp_clip_batch_forward for ``plans`` (any mix of
    FtClipPlan / ClipPlan: ``rotate`` is honoured here).  The clips listed in ``eight_bit`` stop after the resize as uint8
    [t][size][size][3] (no flip, no normalisation) for the caller's 8-bit operations; every other clip i is finished into
    out[i].  ``extra`` (uint8 numpy bytes) rides behind the table in the same upload, on a 16-byte boundary.
    -> (out fp32 [n][3][t][size][size], u8 [len(eight_bit)][t][size][size][3] or None,
        (pinned host view, device view) of ``extra`` or None)."""
    lib = _lib.load()
    n = len(plans)
    if torch.is_tensor(videos):
        videos = [videos] * n
    if len(videos) != n:
        raise ValueError("%d videos for %d plans" % (len(videos), n))
    if lib.cstp_clip_batch_desc_bytes() != _BATCH_DESC.itemsize:
        raise _lib.CstpError("cstp_clip_batch_desc is %d bytes in the library, %d here"
                             % (lib.cstp_clip_batch_desc_bytes(), _BATCH_DESC.itemsize))
    dev = videos[0].device
    t = len(plans[0].frames)
    slot8 = {i: j for j, i in enumerate(eight_bit)}
    nbytes = n * _BATCH_DESC.itemsize + 4 * n * t
    extra_off = (nbytes + 15) // 16 * 16
    if extra is not None:
        nbytes = extra_off + extra.size
    host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    view = host.numpy()
    desc = view[:n * _BATCH_DESC.itemsize].view(_BATCH_DESC)
    idx = view[n * _BATCH_DESC.itemsize:n * _BATCH_DESC.itemsize + 4 * n * t].view(np.int32)
    if extra is not None:
        view[extra_off:] = extra
    tmp_pixels = 0
    for i, (v, p) in enumerate(zip(videos, plans)):
        if not v.is_cuda or v.dtype != torch.uint8 or v.dim() != 4 or v.shape[3] != 3 or not v.is_contiguous() or v.device != dev:
            raise _lib.CstpError("videos must be contiguous uint8 [F, H, W, 3] tensors on one HIP device (cstp_amd has no CPU path)")
        if len(p.frames) != t:
            raise ValueError("clips of %d and %d frames in one batch" % (t, len(p.frames)))
        rot = int(getattr(p, "rotate", 0))
        if rot not in (0, 90, 180, 270):
            raise ValueError("rotation %r: a clip is rotated by 0 / 90 / 180 / 270 degrees" % (rot,))
        x0, y0, x1, y1 = p.box
        if not (x0 < x1 and y0 < y1):
            raise _lib.CstpError("empty crop box %s" % (p.box,))
        rw, rh = getattr(p, "resized", (size, size))
        wx, wy = getattr(p, "window", (0, 0))
        if wx < 0 or wy < 0 or wx + size > rw or wy + size > rh:
            raise ValueError("window (%d, %d) + %d leaves the %d x %d resized image" % (wx, wy, size, rw, rh))
        ksh, bh, kh, _, _ = _device_tables(x1 - x0, rw, dev)
        ksv, bv, kv, _, _ = _device_tables(y1 - y0, rh, dev)
        first, rows = window_rows(y1 - y0, rh, wy, size)
        f, h, w, _ = v.shape
        desc[i] = (v.data_ptr(), kh.data_ptr(), bh.data_ptr(), kv.data_ptr(), bv.data_ptr(), tmp_pixels, f, h, w, i * t, x0, y0,
                   ksh, ksv, rw, rh, wx, wy, first, rows, 1 if getattr(p, "flip", False) else 0,
                   -1 if i in slot8 else i, slot8.get(i, -1), rot)
        idx[i * t:(i + 1) * t] = p.frames
        tmp_pixels += t * rows * size
    if out is None:
        out = torch.empty((n, 3, t, size, size), dtype=torch.float32, device=dev)
    elif out.shape != (n, 3, t, size, size) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a contiguous fp32 [%d, 3, %d, %d, %d] tensor on %s" % (n, t, size, size, dev))
    table = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    table.copy_(host, non_blocking=True)
    tmp = torch.empty(tmp_pixels * 3, dtype=torch.uint8, device=dev)
    u8 = torch.empty((len(slot8), t, size, size, 3), dtype=torch.uint8, device=dev) if slot8 else None
    st = torch.cuda.current_stream().cuda_stream
    check(lib.cstp_clip_batch_forward(st, table.data_ptr(), host.data_ptr(), n, t, size,
                                      table.data_ptr() + n * _BATCH_DESC.itemsize, n * t, tmp.data_ptr(), tmp_pixels,
                                      out.data_ptr(), n, None if u8 is None else u8.data_ptr(), len(slot8)),
          "cstp_clip_batch_forward")
    return out, u8, (None if extra is None else (host[extra_off:], table[extra_off:]))


def assemble_pairs(videos, pair_plans, size: int, out: torch.Tensor = None):
    """A whole batch of pre-training pairs: pair_plans[i] (``sampler.PairPlan``) cut from videos[i] (uint8 [F][H][W][3]; a single
    tensor serves every pair) -> (clip_1 [B][3][T][size][size], clip_2 likewise), the two halves of one fp32 [2][B][3][T][size][size]
    tensor (``out``, if given).  2B descriptors -- rotation codes, boxes that may reach past the rotated frame, flips -- travel in
    ONE pinned upload and are served by the two launches of cstp_clip_batch_forward.  ``null_transform`` clips are written straight
    into their slot; ``base_transform`` clips leave the resize as 8-bit frames and go on through ``apply_base_transform`` into
    theirs.  Bit-identical to ``assemble_clip`` on every clip."""
    pair_plans = list(pair_plans)
    b = len(pair_plans)
    if b == 0:
        raise ValueError("assemble_pairs needs at least one pair")
    if torch.is_tensor(videos):
        videos = [videos] * b
    if len(videos) != b:
        raise ValueError("%d videos for %d pairs" % (len(videos), b))
    plans = [p.clip_1 for p in pair_plans] + [p.clip_2 for p in pair_plans]
    t = len(plans[0].frames)
    if out is not None:
        if out.shape != (2, b, 3, t, size, size):
            raise ValueError("out must be a contiguous fp32 [2, %d, 3, %d, %d, %d] tensor" % (b, t, size, size))
        out = out.view(2 * b, 3, t, size, size)
    based = [i for i, p in enumerate(plans) if p.base is not None]
    flat, u8 = _batch_forward(list(videos) * 2, plans, size, out, based)
    for j, i in enumerate(based):
        apply_base_transform(u8[j], plans[i].base, plans[i].flip, out=flat[i])
    return flat[:b], flat[b:]


def augment_settings(randaug_nmstd, random_erase: float, data_type: str, mode: str):
    """The ``randaug.Settings`` of a labelled data set's ``randaug=(n, m, mstd)`` (or None) and ``random_erase=P`` arguments, None
    when both are off.  Only training clips under 'img' are augmented: anything else is refused."""
    n, m, mstd = (0, 9.0, 0.0) if randaug_nmstd is None else randaug_nmstd
    settings = randaug.Settings(n, float(m), float(mstd), float(random_erase))
    if not settings.on:
        return None
    if data_type != "train" or mode != "img":
        raise ValueError("randaug / random_erase augment training clips under 'img'; data_type %r with mode %r is never augmented"
                         % (data_type, mode))
    return settings


def _labelled_video(label: int, n_classes: int, frames: int, height: int, width: int, gen, device) -> torch.Tensor:
    """uint8 [F][H][W][3]: a moving grating whose orientation, frequency, drift and colour phase are functions of the label,
    plus uniform noise -- separable by a classifier, and smooth enough that a resize is not all aliasing."""
    ang = math.pi * label / max(n_classes, 1)
    freq = 2.0 + (label % 4)
    drift = 0.5 * (1 + (label // 4) % 3)
    ys = torch.linspace(-1, 1, height, device=device).view(1, height, 1, 1)
    xs = torch.linspace(-1, 1, width, device=device).view(1, 1, width, 1)
    ts = torch.arange(frames, device=device, dtype=torch.float32).view(frames, 1, 1, 1) / 32.0
    ch = torch.tensor([0.0, 2.1, 4.2], device=device).view(1, 1, 1, 3) * (1 + label % 3) / 3.0
    phase = freq * math.pi * (math.cos(ang) * xs + math.sin(ang) * ys) + 2 * math.pi * drift * ts + ch
    img = 0.5 + 0.35 * torch.sin(phase) + 0.15 * (torch.rand((frames, height, width, 3), generator=gen, device=device) - 0.5)
    return (img.clamp(0, 1) * 255).to(torch.uint8).contiguous()


class GpuLabelledVideos:
    """Stands in for UcfFineTune (datasets.py:952-1097) on synthetic data: ``n_videos`` labelled, decoded videos (uint8 frames,
    class-dependent patterns, 240 x 320 by default so ClipScale really resizes) live in HBM, with mixed lengths -- the first is
    shorter than clip_range + 1 and takes the wrap-around branch, the second is exactly clip_range + 1.  'train' / 'val' items
    are one clip under ``mode`` ('img' / 'img_val'); a 'test' item is every clip of a video under 'img_test'.  Each sample's RNG
    is seeded from (seed, epoch, index), so the augmentation of a video changes from epoch to epoch.  ``randaug=(n, m, mstd)`` and
    ``random_erase=P`` add RandAugment and random erasing to 'train' clips (cstp_amd.randaug: drawn from a second generator
    seeded from the same three, so the plan's other fields do not move).  Selected by the fine-tune and test drivers with
    ``--dataset synthetic_video``."""

    _SALT = {"train": 11, "val": 23, "test": 37}
    augment = None                     # randaug.Settings of the ``randaug`` / ``random_erase`` arguments; None = off

    def __init__(self, device, data_type="train", mode="img", n_videos=8, n_classes=101, height=240, width=320, sample_duration=16,
                 sample_size=112, pb_rate=4, length=None, seed=1, lengths=None, randaug=None, random_erase=0.0):
        if data_type not in self._SALT:
            raise ValueError("data_type %r" % (data_type,))
        self.augment = augment_settings(randaug, random_erase, data_type, mode)
        sampler._check_ft_mode(mode)
        if (data_type == "test") != (mode == "img_test"):
            raise ValueError("data_type %r with transform mode %r: the video test takes 'img_test', train / val take 'img' / "
                             "'img_val'" % (data_type, mode))
        if mode != "img":
            sampler.short_side(sample_size)
        self.device, self.data_type, self.mode = torch.device(device), data_type, mode
        self.t, self.size, self.pb_rate, self.seed, self.n_classes = sample_duration, sample_size, pb_rate, seed, n_classes
        clip_range = (sample_duration - 1) * pb_rate
        if lengths is None:
            cycle = [max(clip_range - 3, 2), clip_range + 1, 2 * clip_range + 7, clip_range + clip_range // 2, 3 * clip_range + 5]
            lengths = [cycle[v % len(cycle)] for v in range(n_videos)]
        salt = self._SALT[data_type]
        g = torch.Generator(device=self.device).manual_seed(seed * 101 + salt)
        self.labels = [(v * 7 + salt) % n_classes for v in range(len(lengths))]
        self.videos = [_labelled_video(lab, n_classes, int(f), height, width, g, self.device)
                       for lab, f in zip(self.labels, lengths)]
        self.length = len(self.videos) if length is None else length

    def __len__(self):
        return self.length

    def plan(self, index: int, epoch: int = 0):
        """-> (video number, FtClipPlan) for 'train' / 'val', (video number, [FtClipPlan]) for 'test'."""
        v = index % len(self.videos)
        f, h, w, _ = self.videos[v].shape
        if self.data_type == "test":
            return v, sampler.plan_test_video(f, w, h, self.t, self.size, self.pb_rate, self.mode)
        s = ((self.seed * 1000003 + epoch) * 1000003 + index) * 101 + self._SALT[self.data_type]
        plan = sampler.sample_ft_clip(f, w, h, self.t, self.size, self.pb_rate, self.mode, random.Random(s))
        if self.augment is not None:      # a generator of its own: the draws above keep their values
            plan.randaug, plan.erase = randaug.draw(self.augment, self.size, randaug.clip_rng(s))
        return v, plan

    def _labels(self, vs):
        return torch.tensor([self.labels[v] for v in vs], dtype=torch.int64).pin_memory().to(self.device, non_blocking=True)

    def batch(self, indices: List[int], epoch: int = 0):
        """-> (clips [B,3,T,S,S] fp32, labels [B] int64) on the device."""
        picked = [self.plan(i, epoch) for i in indices]
        clips = assemble_batch([self.videos[v] for v, _ in picked], [p for _, p in picked], self.size)
        return clips, self._labels([v for v, _ in picked])

    def video(self, index: int):
        """A 'test' item: (clips [n_clips,3,T,S,S] fp32, label [1] int64) on the device (datasets.py:999-1001)."""
        if self.data_type != "test":
            raise ValueError("video() serves data_type 'test'")
        v, plans = self.plan(index)
        return assemble_batch(self.videos[v], plans, self.size), self._labels([v])


class GpuLabelledLoader(GpuClipLoader):
    """GpuClipLoader's sharding for GpuLabelledVideos.  'train': epoch-seeded shuffle, this rank's stride, full batches only;
    'val': in order, the last partial batch kept (utils.py:91-163); 'test': one video per item, ``(clips [1,n_clips,3,T,S,S],
    label [1])`` as DataLoader(batch_size=1) collates it (test.py:58-60).  Batches are born on the device."""

    def __init__(self, dataset: GpuLabelledVideos, batch_size: int = 1, rank: int = 0, world_size: int = 1, seed: int = 0):
        super().__init__(dataset, batch_size, rank, world_size, seed)
        self.data_type = dataset.data_type

    def indices(self) -> List[int]:
        if self.data_type == "train":
            return super().indices()
        return list(range(len(self.dataset)))[self.rank::self.world_size]

    def __len__(self):
        if self.data_type == "train":
            return super().__len__()
        n = len(self.indices())
        return n if self.data_type == "test" else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        idx = self.indices()
        if self.data_type == "test":
            for i in idx:
                clips, label = self.dataset.video(i)
                yield clips.unsqueeze(0), label
            return
        for b in range(len(self)):
            yield self.dataset.batch(idx[b * self.batch_size:(b + 1) * self.batch_size], self.epoch)

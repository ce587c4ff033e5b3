"""Clip-pair sampler and pretext-label generator of the CSTP pre-training data path -- the host-side decisions of
/root/reference/data_process/datasets.py:859-948 (``repre_train_clip``: playback rate, rotations, temporal overlap) and
/root/reference/data_process/preprocess_data.py:479-565,568-581,713-741 (``ClipRandomSizedCropOverlap`` spatial-overlap crop
geometry, ``ClipRandomHorizontalFlip``, ``TwoClipTransform``'s base-vs-null choice), with every draw taken from one
``random.Random`` in the ORDER the reference takes it from the global ``random`` module, so that a plan is a pure function of
(video length, frame size, options, seed).

What a plan says and what executes it: frame indices, 90-degree rotation codes, crop boxes, flips and the five labels are
decided here on the host (a few dozen integers per pair); the pixels never touch the host -- ``cstp_amd.clip_ops.assemble_pair``
runs rotate -> crop -> bicubic resize -> flip -> tensor -> 'tf' normalise on the decoded uint8 frames resident in HBM.

The reference applies its ``base_transform`` (preprocess_data.py:1110-1121: RandomRotation(10), ClipColorJitter(0.4, 0.4, 0.4,
0.1) with p = 0.8, ClipRandomGray(p = 0.2), ClipGaussianBlur([0.1, 2]) with p = 0.5, then flip / tensor / normalise) to a clip
with probability 0.3 and the ``null_transform`` (flip, tensor, normalise) otherwise (TwoClipTransform :713-741).  The plan
records that choice and, for a base clip, every parameter the branch draws (``BasePlan``), in the reference's draw order --
``transforms.RandomApply`` as the torchvision of the reference's era implements it (``if self.p < random.random(): skip``;
current torchvision draws from torch's generator instead), ``random.shuffle`` of the four colour operations, the channel of
ClipRandomGray per frame from a NumPy ``RandomState`` (the reference calls ``np.random.choice(3)``).  The executor
(cstp_amd.clip_ops) runs both branches on the GPU.  The reference bug that reads clip 2 of the LMDB dataset from
``start_frame`` instead of ``start_frame_2`` (datasets.py:1397) is not replicated.
"""
from __future__ import annotations

import math
import random
from dataclasses import dataclass
from typing import List, Optional, Tuple

PACE = [1, 2, 4, 8]                               # datasets.py:17
OVERLAP_TEM_RATE = [1.0, 0.8, 0.6, 0.4, 0.2]      # datasets.py:18
ROTATE = [0, 90, 180, 270]                        # datasets.py:19 (Image.ROTATE_90 / 180 / 270, counter-clockwise)
OVERLAP_SPA_RATE = [1.0, 0.8, 0.6, 0.4, 0.2]      # preprocess_data.py:18


@dataclass
class BasePlan:
    """The draws of one pass through base_transform (preprocess_data.py:1110-1121), applied to the resized 8-bit frames."""
    angle: float                               # RandomRotation(10): Image.rotate(angle)
    jitter: Optional[List[Tuple[str, float]]]  # ClipColorJitter: ("brightness" | "contrast" | "saturation" | "hue", factor) in
                                               #   the shuffled order, or None (RandomApply p = 0.8 skipped it)
    gray: Optional[List[int]]                  # ClipRandomGray: the channel kept per frame, or None
    blur_sigma: Optional[float]                # ClipGaussianBlur: one sigma per clip, or None (RandomApply p = 0.5)


@dataclass
class ClipPlan:
    frames: List[int]            # 0-based frame indices, in clip order
    rotate: int                  # 0 / 90 / 180 / 270, applied to the whole frame before cropping
    box: Tuple[int, int, int, int]   # (x0, y0, x1, y1) in the ROTATED frame
    flip: bool
    use_base: bool               # TwoClipTransform chose base_transform for this clip (p = 0.3)
    base: Optional[BasePlan] = None   # its draws (None: null_transform)


@dataclass
class PairPlan:
    clip_1: ClipPlan
    clip_2: ClipPlan
    spa_label: int               # spatial-overlap class 0..4  (preprocess_data.py:520)
    tem_label: int               # temporal-overlap class 0..4 (datasets.py:915)
    pb_label: int                # playback-rate class 0..3    (datasets.py:872-873)
    rot_labels: Tuple[int, int]  # rotation classes 0..3       (datasets.py:878-881)


def sample_frames(total_frames: int, sample_duration: int, rng: random.Random):
    """datasets.py:859-948 without the image I/O: -> (idx_1, idx_2, tem_label, pb_label, (rot_label_1, rot_label_2)),
    0-based frame indices (the reference's file names are 1-based: '%05d.jpg' % (start_frame + i))."""
    max_pb = int(math.log2(total_frames / (sample_duration - 1)))
    pb_label = rng.randint(0, min(3, max_pb))
    sample_rate = PACE[pb_label]
    clip_range = (sample_duration - 1) * sample_rate
    rot_label_1 = rng.randint(0, 3)
    rot_label_2 = rng.randint(0, 3)
    if total_frames - clip_range <= 0:
        # short video: wrap around, both clips read the same frames, temporal label 0 (:884-909)
        index_clip, idx_frame = [], 0
        while len(index_clip) < sample_duration:
            index_clip.append(idx_frame)
            idx_frame += sample_rate
            if idx_frame >= total_frames:
                idx_frame = 0
        return list(index_clip), list(index_clip), 0, pb_label, (rot_label_1, rot_label_2)
    start_frame = rng.randint(1, total_frames - clip_range)
    while True:
        tem_label = rng.randint(0, 4)
        tem_rate = OVERLAP_TEM_RATE[tem_label]
        front_behind = rng.randint(0, 1)
        if front_behind == 0:
            start_frame_2 = start_frame - int((1 - tem_rate) * clip_range)
            if start_frame_2 < 1:
                continue
        else:
            start_frame_2 = start_frame + int((1 - tem_rate) * clip_range)
            if start_frame_2 > total_frames - clip_range:
                continue
        offs = list(range(0, clip_range + 1, sample_rate))
        return ([start_frame - 1 + i for i in offs], [start_frame_2 - 1 + i for i in offs], tem_label, pb_label,
                (rot_label_1, rot_label_2))


class OverlapCrop:
    """ClipRandomSizedCropOverlap (preprocess_data.py:479-565): the first call (flag 0) picks a random-sized crop, the second
    (flag 1) a crop of the same size whose overlap with the first is one of OVERLAP_SPA_RATE, anchored at a random corner."""

    def __init__(self, rng: random.Random, p: float = 1.0, bottom_area: float = 0.2):
        self.rng, self.threshold, self.bottom_area = rng, p, bottom_area
        self.pick_size = None
        self.pick_loc = None

    def first(self, img_w: int, img_h: int) -> Tuple[int, int, int, int]:
        rng = self.rng
        if not rng.random() < self.threshold:
            raise NotImplementedError("p < 1 (center crop) is not on the pre-training path (get_transforms builds p = 1.0)")
        while True:
            area = img_w * img_h
            target_area = rng.uniform(self.bottom_area, 1) * area
            aspect_ratio = rng.uniform(3. / 4, 4. / 3)
            w = int(round(math.sqrt(target_area * aspect_ratio)))
            h = int(round(math.sqrt(target_area / aspect_ratio)))
            if rng.random() < 0.5:
                w, h = h, w
            if w <= img_w and h <= img_h:
                x1 = rng.randint(0, img_w - w)
                y1 = rng.randint(0, img_h - h)
                self.pick_size = [w, h]
                self.pick_loc = [x1, y1]
                return (x1, y1, x1 + w, y1 + h)

    def second(self, img_w: int, img_h: int):
        rng = self.rng
        if not rng.random() < self.threshold:
            raise NotImplementedError("p < 1 (center crop) is not on the pre-training path")
        p_w, p_h = self.pick_size
        p_x, p_y = self.pick_loc
        while True:
            rng.uniform(self.bottom_area, 1)          # the reference draws (and ignores) these two on every attempt (:496-497)
            rng.uniform(3. / 4, 4. / 3)
            spa_label = rng.randint(0, 4)
            spa_rate = OVERLAP_SPA_RATE[spa_label]
            corner = rng.randint(0, 3)
            s_w = rng.randint(int(spa_rate * p_w), p_w)
            s_h = int(spa_rate * p_w * p_h / s_w)
            if corner == 0:
                e_w, e_h = p_x + s_w, p_y + s_h
                ok = e_w - p_w >= 0 and e_h - p_h >= 0
            elif corner == 1:
                e_w, e_h = p_x + p_w - s_w + p_w, p_y + s_h
                ok = e_w <= img_w and e_h - p_h >= 0
            elif corner == 2:
                e_w, e_h = p_x + s_w, p_y + p_h - s_h + p_h
                ok = e_w - p_w >= 0 and e_h <= img_h
            else:
                e_w, e_h = p_x + p_w - s_w + p_w, p_y + p_h - s_h + p_h
                ok = e_w <= img_w and e_h <= img_h
            if ok:
                return (e_w - p_w, e_h - p_h, e_w, e_h), spa_label


def _rotated_size(w: int, h: int, rot: int) -> Tuple[int, int]:
    return (h, w) if rot in (90, 270) else (w, h)


def base_draws(rng: random.Random, np_rng, n_frames: int, sample_duration: int) -> BasePlan:
    """base_transform's random draws up to (not including) the flip, in Compose order (preprocess_data.py:1110-1119)."""
    angle = rng.uniform(-10, 10)                               # RandomRotation(10) :1091
    jitter = None
    if not 0.8 < rng.random():                                 # transforms.RandomApply(p = 0.8)
        rng.random()                                           # ClipColorJitter.__call__: random.random() < p (= 1.0) :658
        ops = [("brightness", rng.uniform(0.6, 1.4)), ("contrast", rng.uniform(0.6, 1.4)),
               ("saturation", rng.uniform(0.6, 1.4)), ("hue", rng.uniform(-0.1, 0.1))]       # get_params :632-648
        rng.shuffle(ops)                                       # random.shuffle(transforms) :650
        jitter = ops
    gray = None
    if rng.random() < 0.2:                                     # ClipRandomGray(p = 0.2) :699
        if np_rng is None:
            raise ValueError("the ClipRandomGray channel draws need a numpy RandomState (np.random.choice(3), :705)")
        gray = [int(np_rng.choice(3)) for _ in range(n_frames)]
    sigma = None
    if not 0.5 < rng.random():                                 # transforms.RandomApply(p = 0.5)
        for idx in range(n_frames):                            # ClipGaussianBlur :682-686: a new sigma every sample_duration frames
            if idx % sample_duration == 0:
                sigma = rng.uniform(0.1, 2.0)
    return BasePlan(angle, jitter, gray, sigma)


def sample_pair(total_frames: int, frame_w: int, frame_h: int, sample_duration: int, rng: random.Random,
                p_base: float = 0.3, np_rng=None) -> PairPlan:
    """One training sample of the 'pre_train' pipeline: repre_train_clip (frames, rotations, temporal / playback labels), then
    TwoClipTransform (preprocess_data.py:713-741): base-or-null draw for each clip, overlap crop of clip 1, its flip, overlap
    crop of clip 2, its flip -- with the base_transform draws of a clip (``base_draws``) between its crop and its flip.  Both clips of a pair are cropped in the coordinates of THEIR OWN rotated frames; the reference
    takes the image size from the first frame of each clip list, which is what this does."""
    idx_1, idx_2, tem_label, pb_label, (r1, r2) = sample_frames(total_frames, sample_duration, rng)
    rng.choices(range(2), weights=[1, 0])                     # TransformController picks TwoClipTransform (:779, weights [1, 0])
    use_base_1 = rng.random() < p_base
    use_base_2 = rng.random() < p_base
    crop = OverlapCrop(rng)
    w1, h1 = _rotated_size(frame_w, frame_h, ROTATE[r1])
    box_1 = crop.first(w1, h1)
    base_1 = base_draws(rng, np_rng, len(idx_1), sample_duration) if use_base_1 else None     # q = tr1(q) :736
    flip_1 = rng.random() < 0.5
    w2, h2 = _rotated_size(frame_w, frame_h, ROTATE[r2])
    box_2, spa_label = crop.second(w2, h2)
    base_2 = base_draws(rng, np_rng, len(idx_2), sample_duration) if use_base_2 else None     # k = tr2(k) :738
    flip_2 = rng.random() < 0.5
    return PairPlan(ClipPlan(idx_1, ROTATE[r1], box_1, flip_1, use_base_1, base_1),
                    ClipPlan(idx_2, ROTATE[r2], box_2, flip_2, use_base_2, base_2), spa_label, tem_label, pb_label, (r1, r2))


# ---- the fine-tune / validation / video-test data path (UcfFineTune, datasets.py:952-1097; transform modes 'img', 'img_val',
#      'img_test', preprocess_data.py:1131-1149) ------------------------------------------------------------------------------
FT_MODES = ("img", "img_val", "img_test")


@dataclass
class FtClipPlan:
    """One fine-tune / validation / test clip: crop ``box`` of the frame -> BICUBIC resize to ``resized`` -> the size x size
    window at ``window`` of the resized image -> [colour jitter] -> tensor.  'img' crops resize straight to (size, size) with the
    window at (0, 0); ClipScale -> ClipCenterCrop resizes the whole frame and keeps the centre window."""
    frames: List[int]                          # 0-based frame indices, in clip order
    box: Tuple[int, int, int, int]             # (x0, y0, x1, y1) in the frame
    resized: Tuple[int, int]                   # (width, height) the box is resized to (== the box's size: no resize, ClipScale :853)
    window: Tuple[int, int]                    # (x, y) origin of the size x size output window in the resized image
    jitter: Optional[List[Tuple[str, float]]] = None   # ClipColorJitter's operations in shuffled order, or None
    flip: bool = False                         # 'img' has no flip (preprocess_data.py:1135 is commented out)
    randaug: Optional[List[Tuple[str, float]]] = None   # RandAugment: (operation, parameter of its Pillow call) per layer, or None
    erase: Optional[Tuple[int, int, int, int, int]] = None   # random erasing: (x0, y0, w, h, 64-bit fill key) or None (cstp_amd.randaug)


def _wrap_indices(total_frames: int, sample_duration: int, pb_rate: int, first: int) -> List[int]:
    index_clip, idx_frame = [], first
    while len(index_clip) < sample_duration:
        index_clip.append(idx_frame)
        idx_frame += pb_rate
        if idx_frame >= total_frames:
            idx_frame = first
    return index_clip


def ft_clip_frames(total_frames: int, sample_duration: int, pb_rate: int, rng: random.Random) -> List[int]:
    """UcfFineTune._get_train_clip / _get_val_clip (datasets.py:1003-1060; validation draws a random start too, :1047): a video
    longer than clip_range takes ``randint(1, total - clip_range)`` as its 1-based start, a shorter one wraps around from index 0
    with start_frame = 1 and draws nothing.  0-based indices."""
    clip_range = (sample_duration - 1) * pb_rate
    if total_frames - clip_range <= 0:
        return _wrap_indices(total_frames, sample_duration, pb_rate, 0)          # '%05d.jpg' % (1 + i) -> 0-based i
    start_frame = rng.randint(1, total_frames - clip_range)
    return [start_frame - 1 + i for i in range(0, clip_range + 1, pb_rate)]


def ft_test_frames(total_frames: int, sample_duration: int, pb_rate: int) -> List[List[int]]:
    """UcfFineTune._get_test_clip (datasets.py:1062-1097): windows that start at ``arange(1, total - clip_range + 1, clip_range)``
    plus one extra last window ``arange(total - clip_range, total + 1, pb_rate)``; a short video is sampled once with the
    1-based wrap-around that never reads frame ``total`` (:1068-1073).  No random draw.  0-based indices per clip."""
    clip_range = (sample_duration - 1) * pb_rate
    if total_frames - clip_range <= 0:
        return [[i - 1 for i in _wrap_indices(total_frames, sample_duration, pb_rate, 1)]]
    clips = [[s - 1 + j * pb_rate for j in range(sample_duration)] for s in range(1, total_frames - clip_range + 1, clip_range)]
    clips.append([i - 1 for i in range(total_frames - clip_range, total_frames + 1, pb_rate)])
    return clips


def clip_scale_size(frame_w: int, frame_h: int, size: int) -> Tuple[int, int]:
    """ClipScale(size) (preprocess_data.py:843-864) -> (width, height): unchanged when the short side already equals ``size``,
    otherwise the short side becomes ``size`` and the other ``int(size * long / short)``."""
    if (frame_w <= frame_h and frame_w == size) or (frame_h <= frame_w and frame_h == size):
        return frame_w, frame_h
    if frame_w < frame_h:
        return size, int(size * frame_h / frame_w)
    return int(size * frame_w / frame_h), size


def center_crop_origin(w: int, h: int, size: int) -> Tuple[int, int]:
    """ClipCenterCrop(size) (preprocess_data.py:815-840): Python's round (half to even): (171 - 112) / 2. -> 30."""
    return int(round((w - size) / 2.)), int(round((h - size) / 2.))


def _scale_center(frames, frame_w, frame_h, short_size, size, jitter=None) -> FtClipPlan:
    rw, rh = clip_scale_size(frame_w, frame_h, short_size)
    wx, wy = center_crop_origin(rw, rh, size)
    if wx < 0 or wy < 0 or wx + size > rw or wy + size > rh:
        raise ValueError("centre crop %d of the %d x %d scaled frame reaches past it" % (size, rw, rh))
    return FtClipPlan(frames, (0, 0, frame_w, frame_h), (rw, rh), (wx, wy), jitter)


def random_sized_crop(frame_w: int, frame_h: int, rng: random.Random, bottom_area: float = 0.2):
    """ClipRandomSizedCrop's draws (preprocess_data.py:440-476): the p = 1.0 draw (consumed), then up to 10 attempts of uniform
    area, uniform aspect, swap draw and -- on success -- randint x, randint y.  -> the box, or None after 10 failures (the caller
    falls back to ClipScale -> ClipCenterCrop)."""
    if not rng.random() < 1.0:
        raise NotImplementedError("p < 1 (plain centre crop) is not on the 'img' path (get_transforms builds p = 1.0)")
    for _ in range(10):
        target_area = rng.uniform(bottom_area, 1) * (frame_w * frame_h)
        aspect_ratio = rng.uniform(3. / 4, 4. / 3)
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if rng.random() < 0.5:
            w, h = h, w
        if w <= frame_w and h <= frame_h:
            x1 = rng.randint(0, frame_w - w)
            y1 = rng.randint(0, frame_h - h)
            return (x1, y1, x1 + w, y1 + h)
    return None


def colour_jitter_draws(rng: random.Random, p: float, brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1):
    """ClipColorJitter.__call__ (preprocess_data.py:659-664): one ``random()`` against p, then get_params' four uniforms and the
    shuffle (:636-654); one transform for the whole clip.  -> [(op, factor)] in applied order, or None."""
    if not rng.random() < p:
        return None
    ops = [("brightness", rng.uniform(max(0, 1 - brightness), 1 + brightness)),
           ("contrast", rng.uniform(max(0, 1 - contrast), 1 + contrast)),
           ("saturation", rng.uniform(max(0, 1 - saturation), 1 + saturation)), ("hue", rng.uniform(-hue, hue))]
    rng.shuffle(ops)
    return ops


def _check_ft_mode(mode: str):
    if mode in ("numpy", "numpy_val"):
        raise ValueError("transform mode %r resizes with cv2.resize (preprocess_data.py:867-890); cv2 is not available to pin a "
                         "bit-exact kernel against, so only the PIL modes %s are served" % (mode, "/".join(FT_MODES)))
    if mode not in FT_MODES:
        raise ValueError("transform mode %r: the fine-tune clip path serves %s" % (mode, "/".join(FT_MODES)))


def short_side(sample_size: int) -> int:
    """get_transforms 'img_val' / 'img_test' (preprocess_data.py:1140-1143): 112 -> 128, 224 -> 256."""
    if sample_size == 112:
        return 128
    if sample_size == 224:
        return 256
    raise ValueError("sample_size %r: the reference binds short_size only for 112 and 224 (preprocess_data.py:1140-1143) and "
                     "fails with an unbound name for any other" % (sample_size,))


def spatial_plan(mode: str, frames: List[int], frame_w: int, frame_h: int, sample_size: int, rng: Optional[random.Random]):
    """The transform of one clip, get_transforms(mode) (preprocess_data.py:1131-1149).  'img' draws from ``rng`` (crop, then
    jitter); 'img_val' / 'img_test' draw nothing."""
    _check_ft_mode(mode)
    if mode == "img":
        box = random_sized_crop(frame_w, frame_h, rng)
        if box is None:
            plan = _scale_center(frames, frame_w, frame_h, sample_size, sample_size)       # the fallback :470-473
        else:
            plan = FtClipPlan(frames, box, (sample_size, sample_size), (0, 0))
        plan.jitter = colour_jitter_draws(rng, 0.3)
        return plan
    return _scale_center(frames, frame_w, frame_h, short_side(sample_size), sample_size)


def sample_ft_clip(total_frames: int, frame_w: int, frame_h: int, sample_duration: int, sample_size: int, pb_rate: int,
                   mode: str, rng: random.Random) -> FtClipPlan:
    """One train ('img') or validation ('img_val') sample of UcfFineTune.__getitem__ (datasets.py:993-998): frame indices, then
    the spatial transform, every draw from ``rng`` in the reference's order."""
    _check_ft_mode(mode)
    if mode == "img_test":
        raise ValueError("'img_test' plans a whole video: use plan_test_video")
    if mode != "img":
        short_side(sample_size)                     # refuse before any draw
    frames = ft_clip_frames(total_frames, sample_duration, pb_rate, rng)
    return spatial_plan(mode, frames, frame_w, frame_h, sample_size, rng)


def plan_test_video(total_frames: int, frame_w: int, frame_h: int, sample_duration: int, sample_size: int, pb_rate: int,
                    mode: str = "img_test") -> List[FtClipPlan]:
    """Every clip of one test video (datasets.py:999-1001, 1062-1097) under 'img_test' (or 'img_val'): deterministic."""
    _check_ft_mode(mode)
    if mode == "img":
        raise ValueError("the video test takes 'img_test' (test.py); 'img' is the training augmentation")
    return [spatial_plan(mode, f, frame_w, frame_h, sample_size, None)
            for f in ft_test_frames(total_frames, sample_duration, pb_rate)]

"""RandAugment and random erasing for fine-tuning: the settings behind --randaug_n / --randaug_m / --randaug_mstd /
--random_erase, the per-clip draws, and the operation tables of cstp_randaug_layer / cstp_randaug_finish (csrc/randaug.h;
DESIGN.md section 23).  The kernels run from ``clip_ops.augment_batch``; nothing here touches the device.

The 14 operations (Cubuk et al., "RandAugment", 2020), each the Pillow call it must equal bit for bit on every frame of the clip,
with r = m / 30, s = +-1, S = clip size, F = (128, 128, 128):

    Identity                      copy
    ShearX / ShearY               im.transform(im.size, AFFINE, (1, v, 0, 0, 1, 0) / (1, 0, 0, v, 1, 0), NEAREST, fillcolor=F), v = s 0.3 r
    TranslateX / TranslateY       the same call with (1, 0, d, 0, 1, 0) / (1, 0, 0, 0, 1, d), d = s int(0.45 S r)
    Rotate                        im.rotate(s 30 r, fillcolor=F)
    Brightness / Color / Contrast / Sharpness     ImageEnhance.X(im).enhance(1 + s 0.9 r)
    Posterize                     ImageOps.posterize(im, 8 - int(round(4 r)))
    Solarize                      ImageOps.solarize(im, int(round(255 (1 - r))))
    AutoContrast / Equalize       ImageOps.autocontrast(im) / ImageOps.equalize(im)

A plan carries ``randaug = [(name, value)]`` with ``value`` the one parameter of that call (v, d, the angle, the factor, the bits,
the threshold; 0.0 where there is none) and ``erase = (x0, y0, w, h, key)``: a box in the finished clip, through all frames and
channels, and the 64-bit Philox key of its fill.

Draw order, per clip, from a generator of the clip's own (``clip_rng``: the plan's seed plus a salt, so the frames, crop and
jitter of ``sampler.sample_ft_clip`` keep their values whatever these settings are):  n times {operation: randrange(14);
magnitude: gauss(m, mstd) clipped to [0, 30]; sign: random() < 0.5 -> -1} -- all three are drawn for every operation, used or not,
so the stream has a fixed shape -- then the erase draw: random() against P, up to 10 attempts of {area: uniform(0.02, 1 / 3) S^2;
aspect: exp(uniform(log 0.3, log(1 / 0.3))); h = round(sqrt(area aspect)), w = round(sqrt(area / aspect)); accepted when
1 <= w < S and 1 <= h < S: y0 = randint(0, S - h), x0 = randint(0, S - w)}, then getrandbits(64) for the key.
Degenerate draws (v = 0, d = 0, angle 0, factor exactly 1.0) become Identity: Pillow returns copies there."""
from __future__ import annotations

import math
import random
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness",
       "Posterize", "Solarize", "AutoContrast", "Equalize")
MAX_N, MAX_M = 4, 30.0
GPU_CLIP_DATASETS = ("synthetic_video", "UcfFineTune")

# operation codes of cstp_randaug_entry.op (include/cstp_hip.h)
RA_COPY, RA_AUTOCONTRAST, RA_EQUALIZE, RA_POSTERIZE, RA_SOLARIZE, RA_BRIGHTNESS, RA_CONTRAST, RA_COLOR, RA_SHARPNESS, RA_AFFINE, \
    RA_SHIFT = range(11)
_BLEND = {"Brightness": RA_BRIGHTNESS, "Contrast": RA_CONTRAST, "Color": RA_COLOR, "Sharpness": RA_SHARPNESS}

ENTRY = np.dtype([("op", "<i4"), ("a", "<i4", (6,)), ("factor", "<f4")])                  # struct cstp_randaug_entry
FINISH_ENTRY = np.dtype([(n, "<i4") for n in ("out_slot", "flip", "x0", "y0", "w", "h")]
                        + [("key_lo", "<u4"), ("key_hi", "<u4")])                           # struct cstp_randaug_finish_entry


@dataclass(frozen=True)
class Settings:
    """--randaug_n, --randaug_m, --randaug_mstd, --random_erase; out-of-range values are refused with the flag's name."""
    n: int = 0
    m: float = 9.0
    mstd: float = 0.0
    erase: float = 0.0

    def __post_init__(self):
        if isinstance(self.n, bool) or int(self.n) != self.n or not 0 <= self.n <= MAX_N:
            raise ValueError("--randaug_n takes 0..%d operations per clip, got %r" % (MAX_N, self.n))
        if not 0.0 <= self.m <= MAX_M:                          # (a NaN fails both comparisons)
            raise ValueError("--randaug_m takes a magnitude in [0, %g], got %r" % (MAX_M, self.m))
        if not (0.0 <= self.mstd < float("inf")):
            raise ValueError("--randaug_mstd must be finite and >= 0, got %r" % (self.mstd,))
        if not 0.0 <= self.erase <= 1.0:
            raise ValueError("--random_erase takes a probability in [0, 1], got %r" % (self.erase,))

    @property
    def on(self) -> bool:
        return self.n > 0 or self.erase > 0.0


def from_opts(opts) -> Optional[Settings]:
    """The Settings of the four flags, or None when both features are off (the data path is then today's, bit for bit).
    Refused: out-of-range values; either feature with a data set that has no GPU clip path or a transform mode other than 'img'."""
    s = Settings(opts.randaug_n, float(opts.randaug_m), float(opts.randaug_mstd), float(opts.random_erase))
    if not s.on:
        return None
    flag = "--randaug_n" if s.n > 0 else "--random_erase"
    if opts.dataset not in GPU_CLIP_DATASETS:
        raise ValueError("%s needs a data set whose clips are assembled on the GPU (--dataset %s), got --dataset %s"
                         % (flag, " | ".join(GPU_CLIP_DATASETS), opts.dataset))
    if opts.transform_mode != "img":
        raise ValueError("%s augments the training transform 'img', got --transform_mode %s" % (flag, opts.transform_mode))
    return s


def clip_rng(plan_seed: int) -> random.Random:
    """The private generator of one clip's RandAugment / erase draws: the integer its plan is seeded from, salted."""
    return random.Random(plan_seed * 1000003 + 0x5A17)


def op_value(name: str, magnitude: float, sign: int, size: int) -> Tuple[str, float]:
    """(operation, the parameter of its Pillow call) at ``magnitude`` in [0, 30]; degenerate parameters give Identity."""
    r = magnitude / 30.0
    if name in ("ShearX", "ShearY"):
        v = sign * 0.3 * r
        return (name, v) if v != 0 else ("Identity", 0.0)
    if name in ("TranslateX", "TranslateY"):
        d = sign * int(0.45 * size * r)
        return (name, float(d)) if d != 0 else ("Identity", 0.0)
    if name == "Rotate":
        a = sign * 30.0 * r
        return (name, a) if a != 0 else ("Identity", 0.0)
    if name in _BLEND:
        f = 1 + sign * 0.9 * r
        return (name, f) if f != 1.0 else ("Identity", 0.0)
    if name == "Posterize":
        return name, float(8 - int(round(4 * r)))
    if name == "Solarize":
        return name, float(int(round(255 * (1 - r))))
    if name not in OPS:
        raise ValueError("RandAugment operation %r" % (name,))
    return name, 0.0


def draw_ops(s: Settings, size: int, rng: random.Random) -> Optional[List[Tuple[str, float]]]:
    if s.n == 0:
        return None
    ops = []
    for _ in range(s.n):
        name = OPS[rng.randrange(len(OPS))]
        magnitude = min(MAX_M, max(0.0, rng.gauss(s.m, s.mstd)))
        sign = -1 if rng.random() < 0.5 else 1
        ops.append(op_value(name, magnitude, sign, size))
    return ops


def draw_erase(s: Settings, size: int, rng: random.Random) -> Optional[Tuple[int, int, int, int, int]]:
    if not rng.random() < s.erase:
        return None
    for _ in range(10):
        area = rng.uniform(0.02, 1.0 / 3.0) * size * size
        aspect = math.exp(rng.uniform(math.log(0.3), math.log(1.0 / 0.3)))
        h = int(round(math.sqrt(area * aspect)))
        w = int(round(math.sqrt(area / aspect)))
        if 1 <= w < size and 1 <= h < size:
            y0 = rng.randint(0, size - h)
            x0 = rng.randint(0, size - w)
            return x0, y0, w, h, rng.getrandbits(64)
    return None


def draw(s: Settings, size: int, rng: random.Random):
    """-> (randaug, erase) of one clip, both possibly None, in the module docstring's draw order."""
    ops = draw_ops(s, size, rng)
    return ops, draw_erase(s, size, rng)


def _fix(v: float) -> int:
    return int(math.floor(v * 65536.0 + 0.5))


def affine_coeffs(m) -> List[int]:
    """Geometry.c affine_fixed: the matrix (a, b, c, d, e, f) of Image.transform(AFFINE) in 16.16 fixed point, the half-pixel
    centre folded into the offsets."""
    return [_fix(m[0]), _fix(m[1]), _fix(m[2] + m[0] * 0.5 + m[1] * 0.5), _fix(m[3]), _fix(m[4]), _fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def entry(name: str, value: float, size: int):
    """(op code, six int32, factor) of struct cstp_randaug_entry for one operation of a plan."""
    zero = [0] * 6
    if name == "Identity":
        return RA_COPY, zero, 1.0
    if name == "ShearX":
        return RA_AFFINE, affine_coeffs((1.0, value, 0.0, 0.0, 1.0, 0.0)), 1.0
    if name == "ShearY":
        return RA_AFFINE, affine_coeffs((1.0, 0.0, 0.0, value, 1.0, 0.0)), 1.0
    if name in ("TranslateX", "TranslateY"):
        d = int(value)
        if d != value or abs(d) > size:
            raise ValueError("%s by %r pixels in a clip of size %d" % (name, value, size))
        return RA_SHIFT, ([d, 0] if name == "TranslateX" else [0, d]) + [0] * 4, 1.0
    if name == "Rotate":
        from .clip_ops import rotate_coeffs
        coef = rotate_coeffs(size, size, value)
        if coef is None:                                    # 0 / 90 / 180 / 270: Image.rotate copies or transposes
            if value % 360.0 == 0:
                return RA_COPY, zero, 1.0
            raise ValueError("Rotate by %r degrees: RandAugment rotates by at most 30" % (value,))
        return RA_AFFINE, coef, 1.0
    if name in _BLEND:
        if not 0.0 <= value <= 2.0:
            raise ValueError("%s factor %r outside [0, 2]" % (name, value))
        return (RA_COPY, zero, 1.0) if value == 1.0 else (_BLEND[name], zero, float(value))
    if name == "Posterize":
        bits = int(value)
        if bits != value or not 1 <= bits <= 8:
            raise ValueError("Posterize to %r bits" % (value,))
        return RA_POSTERIZE, [~(2 ** (8 - bits) - 1) & 255] + [0] * 5, 1.0
    if name == "Solarize":
        t = int(value)
        if t != value or not 0 <= t <= 256:
            raise ValueError("Solarize threshold %r" % (value,))
        return RA_SOLARIZE, [t] + [0] * 5, 1.0
    if name == "AutoContrast":
        return RA_AUTOCONTRAST, zero, 1.0
    if name == "Equalize":
        return RA_EQUALIZE, zero, 1.0
    raise ValueError("RandAugment operation %r" % (name,))


def n_layers(plans) -> int:
    return max(len(getattr(p, "randaug", None) or ()) for p in plans)


def tables(plans, flips, size: int) -> np.ndarray:
    """The tables of one batch as bytes: ``n_layers(plans)`` layer tables of len(plans) ENTRY each (a clip with fewer operations
    is copied through the remaining layers), then the FINISH_ENTRY table; clip i finishes into out[i]."""
    n, layers = len(plans), n_layers(plans)
    lay = np.zeros((layers, n), dtype=ENTRY)
    lay["factor"] = 1.0
    fin = np.zeros(n, dtype=FINISH_ENTRY)
    for i, p in enumerate(plans):
        for l, (name, value) in enumerate(getattr(p, "randaug", None) or ()):
            lay[l, i] = entry(name, value, size)
        fin[i]["out_slot"], fin[i]["flip"] = i, 1 if flips[i] else 0
        er = getattr(p, "erase", None)
        if er is not None:
            x0, y0, w, h, key = er
            if not (w >= 1 and h >= 1 and x0 >= 0 and y0 >= 0 and x0 + w <= size and y0 + h <= size):
                raise ValueError("erase box %r leaves the %d x %d clip" % (er[:4], size, size))
            fin[i]["x0"], fin[i]["y0"], fin[i]["w"], fin[i]["h"] = x0, y0, w, h
            fin[i]["key_lo"], fin[i]["key_hi"] = key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF
    return np.concatenate([lay.reshape(-1).view(np.uint8), fin.view(np.uint8)])

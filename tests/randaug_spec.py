"""TEST INFRASTRUCTURE ONLY -- numpy restatement of RandAugment and random erasing: the 14 operations on one
8-bit RGB frame [H][W][3], the erased box of the finished fp32 clip (on top of tests/reg_spec.philox4x32_10), and the draws.
tests/test_randaug_host.py pins every operation here bit for bit against the Pillow call it stands for; the GPU tests then
compare the kernels with Pillow AND with this file.  Nothing in cstp_amd imports it."""
import math

import numpy as np

import reg_spec
from oracle import pil_ops

FILL = 128
OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness",
       "Posterize", "Solarize", "AutoContrast", "Equalize")
SIGNED = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness")


# ---- the parameter of each Pillow call ------------------------------------------------------------------------------------------
def op_value(name, magnitude, sign, size):
    """-> (operation, parameter); degenerate parameters (v = 0, d = 0, angle 0, factor exactly 1.0) give Identity."""
    r = magnitude / 30.0
    if name in ("ShearX", "ShearY"):
        v = sign * 0.3 * r
    elif name in ("TranslateX", "TranslateY"):
        v = float(sign * int(0.45 * size * r))
    elif name == "Rotate":
        v = sign * 30.0 * r
    elif name in ("Brightness", "Color", "Contrast", "Sharpness"):
        v = 1 + sign * 0.9 * r
        return (name, v) if v != 1.0 else ("Identity", 0.0)
    elif name == "Posterize":
        return name, float(8 - int(round(4 * r)))
    elif name == "Solarize":
        return name, float(int(round(255 * (1 - r))))
    else:
        assert name in OPS, name
        return name, 0.0
    return (name, v) if v != 0 else ("Identity", 0.0)


# ---- geometry: Geometry.c affine_fixed with a fill colour, and the integer shift ---------------------------------------------------
def affine_fill(img, m):
    """Image.transform(size, AFFINE, m, NEAREST, fillcolor=(128,) * 3) for a matrix that takes the fixed-point path."""
    h, w = img.shape[:2]
    a0, a1, a2, a3, a4, a5 = pil_ops.affine_fixed_coeffs(m)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.int64)
    xin = (a2 + a1 * ys + a0 * xs) >> 16
    yin = (a5 + a4 * ys + a3 * xs) >> 16
    ok = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
    out = np.full_like(img, FILL)
    out[ok] = img[yin[ok], xin[ok]]
    return out


def shift_fill(img, dx, dy):
    """out(x, y) = img(x + dx, y + dy), the fill colour outside: what Pillow's scale path makes of an integer translation."""
    h, w = img.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    xin, yin = xs + dx, ys + dy
    ok = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
    out = np.full_like(img, FILL)
    out[ok] = img[yin[ok], xin[ok]]
    return out


def rotate_fill(img, angle):
    h, w = img.shape[:2]
    if angle % 360.0 == 0:
        return img.copy()
    return affine_fill(img, pil_ops.rotate_matrix(w, h, angle))


# ---- look-up tables --------------------------------------------------------------------------------------------------------------
def autocontrast_table(hist):
    """ImageOps.autocontrast(im)'s table of one channel from its 256-bin histogram."""
    filled = np.nonzero(hist)[0]
    lo, hi = int(filled[0]), int(filled[-1])
    if hi <= lo:
        return np.arange(256, dtype=np.uint8)
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.array([min(255, max(0, int(ix * scale + offset))) for ix in range(256)], dtype=np.uint8)


def equalize_table_raw(hist):
    """ImageOps.equalize(im)'s table of one channel as its loop leaves it: entries may exceed 255."""
    hist = [int(v) for v in hist]
    filled = [v for v in hist if v]
    if len(filled) <= 1:
        return list(range(256))
    step = (sum(filled) - filled[-1]) // 255
    if not step:
        return list(range(256))
    lut, n = [], step // 2
    for i in range(256):
        lut.append(n // step)
        n += hist[i]
    return lut


def equalize_table(hist):
    """... as Image.point applies it: entries above 255 are clipped, not wrapped."""
    return np.array([min(v, 255) for v in equalize_table_raw(hist)], dtype=np.uint8)


def equalize_peak(channel):
    """The largest unclipped table entry that a pixel of this channel (uint8 [H][W]) actually reads."""
    hist = np.bincount(channel.reshape(-1), minlength=256)
    return equalize_table_raw(hist)[int(np.nonzero(hist)[0][-1])]


def _per_channel(img, table_of):
    out = np.empty_like(img)
    for c in range(3):
        out[..., c] = table_of(np.bincount(img[..., c].reshape(-1), minlength=256))[img[..., c]]
    return out


# ---- the 3 x 3 smooth filter -----------------------------------------------------------------------------------------------------------
def smooth(img):
    """ImageFilter.SMOOTH: border rows and columns copied, inner pixels (2 * sum + 13) // 26, weights (1 1 1 / 1 5 1 / 1 1 1)."""
    out = img.copy()
    h, w = img.shape[:2]
    if h < 3 or w < 3:
        return out
    a = img.astype(np.int64)
    s = 4 * a[1:-1, 1:-1]
    for dy in range(3):
        for dx in range(3):
            s = s + a[dy:h - 2 + dy, dx:w - 2 + dx]
    out[1:-1, 1:-1] = ((2 * s + 13) // 26).astype(np.uint8)
    return out


# ---- one operation on one frame ------------------------------------------------------------------------------------------------------
def apply_op(img, name, value):
    if name == "Identity":
        return img.copy()
    if name == "ShearX":
        return affine_fill(img, (1.0, value, 0.0, 0.0, 1.0, 0.0))
    if name == "ShearY":
        return affine_fill(img, (1.0, 0.0, 0.0, value, 1.0, 0.0))
    if name == "TranslateX":
        return shift_fill(img, int(value), 0)
    if name == "TranslateY":
        return shift_fill(img, 0, int(value))
    if name == "Rotate":
        return rotate_fill(img, value)
    if name == "Brightness":
        return pil_ops.adjust_brightness(img, value)
    if name == "Color":
        return pil_ops.adjust_saturation(img, value)
    if name == "Contrast":
        return pil_ops.adjust_contrast(img, value)
    if name == "Sharpness":
        return pil_ops.blend(smooth(img), img, value)
    if name == "Posterize":
        return img & np.uint8(~(2 ** (8 - int(value)) - 1) & 255)
    if name == "Solarize":
        return np.where(img.astype(np.int32) < int(value), img, 255 - img).astype(np.uint8)
    if name == "AutoContrast":
        return _per_channel(img, autocontrast_table)
    if name == "Equalize":
        return _per_channel(img, equalize_table)
    raise ValueError(name)


def apply_chain(frames, ops):
    """frames uint8 [T][S][S][3] under [(operation, value)], frame by frame -> uint8 [T][S][S][3]."""
    out = []
    for im in frames:
        for name, value in (ops or ()):
            im = apply_op(im, name, value)
        out.append(im)
    return np.stack(out)


# ---- the finish: flip, tensor, erased box ---------------------------------------------------------------------------------------------
def erase_fill(n_elements, key):
    """fp32 [n]: what element e of a clip's tensor becomes INSIDE the box: (w >> 8) * 2^-23 - 1, w = Philox((e >> 2, 0), key)[e & 3]."""
    q = np.arange((n_elements + 3) // 4, dtype=np.uint64)
    w = reg_spec.philox4x32_10((q & reg_spec.M32, q >> np.uint64(32), 0, 0), (key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF)).reshape(-1)
    return ((w[:n_elements] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)).astype(np.float32)


def finish(frames, flip, erase=None):
    """uint8 [T][S][S][3] -> fp32 [3][T][S][S]: [flip] -> ToTensor -> 'tf' -> the box (x0, y0, w, h, key) of the OUTPUT erased."""
    out = np.stack([pil_ops.to_tensor_tf(pil_ops.transpose(im, "flip") if flip else im) for im in frames], axis=1)
    if erase is not None:
        x0, y0, w, h, key = erase
        fill = erase_fill(out.size, key).reshape(out.shape)
        out[:, :, y0:y0 + h, x0:x0 + w] = fill[:, :, y0:y0 + h, x0:x0 + w]
    return out


# ---- the draws -----------------------------------------------------------------------------------------------------------------------
def draw(n, m, mstd, p_erase, size, rng):
    """One clip's draws from ``rng`` (a random.Random), in order -> (ops or None, erase or None)."""
    ops = None
    if n > 0:
        ops = []
        for _ in range(n):
            name = OPS[rng.randrange(14)]
            magnitude = min(30.0, max(0.0, rng.gauss(m, mstd)))
            sign = -1 if rng.random() < 0.5 else 1
            ops.append(op_value(name, magnitude, sign, size))
    erase = None
    if rng.random() < p_erase:
        for _ in range(10):
            area = rng.uniform(0.02, 1.0 / 3.0) * size * size
            aspect = math.exp(rng.uniform(math.log(0.3), math.log(1.0 / 0.3)))
            h, w = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
            if 1 <= w < size and 1 <= h < size:
                y0 = rng.randint(0, size - h)
                x0 = rng.randint(0, size - w)
                erase = (x0, y0, w, h, rng.getrandbits(64))
                break
    return ops, erase

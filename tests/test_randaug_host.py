"""RandAugment and random erasing, host side (no GPU): tests/randaug_spec.py against Pillow itself, operation by operation and bit for
bit; the draws of cstp_amd.randaug; the flags and every refusal; the new symbols of the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
from PIL import Image, ImageEnhance, ImageOps

import randaug_spec as spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = (spec.FILL,) * 3
MAGNITUDES = (0.0, 9.0, 30.0, 13.7)


# ---- the Pillow calls the issue defines the operations by ---------------------------------------------------------------------------
def pil_apply(img, name, value):
    im = Image.fromarray(img)
    if name == "Identity":
        out = im.copy()
    elif name == "ShearX":
        out = im.transform(im.size, Image.AFFINE, (1, value, 0, 0, 1, 0), Image.NEAREST, fillcolor=F)
    elif name == "ShearY":
        out = im.transform(im.size, Image.AFFINE, (1, 0, 0, value, 1, 0), Image.NEAREST, fillcolor=F)
    elif name == "TranslateX":
        out = im.transform(im.size, Image.AFFINE, (1, 0, int(value), 0, 1, 0), Image.NEAREST, fillcolor=F)
    elif name == "TranslateY":
        out = im.transform(im.size, Image.AFFINE, (1, 0, 0, 0, 1, int(value)), Image.NEAREST, fillcolor=F)
    elif name == "Rotate":
        out = im.rotate(value, fillcolor=F)
    elif name == "Brightness":
        out = ImageEnhance.Brightness(im).enhance(value)
    elif name == "Color":
        out = ImageEnhance.Color(im).enhance(value)
    elif name == "Contrast":
        out = ImageEnhance.Contrast(im).enhance(value)
    elif name == "Sharpness":
        out = ImageEnhance.Sharpness(im).enhance(value)
    elif name == "Posterize":
        out = ImageOps.posterize(im, int(value))
    elif name == "Solarize":
        out = ImageOps.solarize(im, int(value))
    elif name == "AutoContrast":
        out = ImageOps.autocontrast(im)
    elif name == "Equalize":
        out = ImageOps.equalize(im)
    else:
        raise ValueError(name)
    return np.array(out)


def pil_chain(frames, ops):
    """uint8 [T][S][S][3] through the Pillow calls of [(operation, value)], frame by frame."""
    out = []
    for im in frames:
        for name, value in (ops or ()):
            im = pil_apply(im, name, value)
        out.append(im)
    return np.stack(out)


# ---- frames -------------------------------------------------------------------------------------------------------------------------
def textured(size, seed):
    """Random frame with a dark quadrant and a saturated column."""
    rs = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:size, 0:size]
    img = np.clip(120 + 70 * np.sin(xs / 3.0 + ys / 5.0)[:, :, None] + rs.randint(-60, 60, size=(size, size, 3)), 0, 255).astype(np.uint8)
    img[:size // 2, :size // 2] //= 6
    img[:, size - 2] = 255
    return img


def constant_channel(size, seed):
    img = textured(size, seed)
    img[..., 1] = 77
    return img


def two_valued_channel(size, seed):
    img = textured(size, seed)
    img[..., 2] = np.where(np.random.RandomState(seed + 1).rand(size, size) < 0.3, 40, 200).astype(np.uint8)
    return img


def over_255(size, seed):
    """A frame whose Equalize table holds an entry above 255 that a pixel reads (most textured frames do; this one is checked)."""
    img = textured(size, seed)
    img[..., 0] = np.minimum(img[..., 0], 250)
    img[0, 0, 0] = 251                                  # the last non-empty bin holds one pixel
    assert spec.equalize_peak(img[..., 0]) > 255
    return img


def edge_frames(size):
    frames = [textured(size, 1), textured(size, 2), constant_channel(size, 3), two_valued_channel(size, 4)]
    if size * size >= 510:                              # below that Equalize's step is 0 and every table is the identity
        frames.append(over_255(size, 5))
    return frames


def all_op_values(size):
    """Every (operation, value) at the magnitudes 0, 9, 30 and a non-integer one, both signs, without duplicates."""
    seen, out = set(), []
    for name in spec.OPS:
        for m in MAGNITUDES:
            for sign in ((-1, 1) if name in spec.SIGNED else (1,)):
                ov = spec.op_value(name, m, sign, size)
                if ov not in seen:
                    seen.add(ov)
                    out.append(ov)
    return out


# ---- spec == Pillow -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [33, 8])
def test_every_operation_of_the_spec_equals_its_pillow_call(size):
    cases = all_op_values(size)
    assert {n for n, _ in cases} == set(spec.OPS)
    for k, img in enumerate(edge_frames(size)):
        for name, value in cases:
            got, want = spec.apply_op(img, name, value), pil_apply(img, name, value)
            assert np.array_equal(got, want), (size, k, name, value, int((got != want).sum()))


def test_non_square_and_tiny_frames():
    rs = np.random.RandomState(7)
    for h, w in ((40, 56), (7, 9)):
        img = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        for name, value in [("ShearX", 0.21), ("ShearY", -0.3), ("Rotate", 17.5), ("Rotate", -30.0), ("TranslateX", 3.0), ("TranslateY", -2.0),
                            ("Sharpness", 1.9), ("Sharpness", 0.1), ("Equalize", 0.0), ("AutoContrast", 0.0), ("Posterize", 4.0),
                            ("Solarize", 128.0)]:
            assert np.array_equal(spec.apply_op(img, name, value), pil_apply(img, name, value)), (h, w, name, value)


def test_equalize_edge_frames():
    small = textured(8, 1)                              # 64 pixels: step = (64 - last) // 255 = 0 -> identity
    assert np.array_equal(spec.apply_op(small, "Equalize", 0.0), small) and np.array_equal(pil_apply(small, "Equalize", 0.0), small)
    big = over_255(33, 5)
    got = spec.apply_op(big, "Equalize", 0.0)
    assert np.array_equal(got, pil_apply(big, "Equalize", 0.0))
    assert got[0, 0, 0] == 255                          # clipped, not wrapped
    const = constant_channel(33, 3)
    assert np.array_equal(spec.apply_op(const, "Equalize", 0.0)[..., 1], const[..., 1])
    assert np.array_equal(spec.apply_op(const, "AutoContrast", 0.0)[..., 1], const[..., 1])


def test_degenerate_parameters_become_identity():
    for name in spec.SIGNED:
        assert spec.op_value(name, 0.0, 1, 112) == ("Identity", 0.0) and spec.op_value(name, 0.0, -1, 112) == ("Identity", 0.0)
    assert spec.op_value("TranslateX", 0.5, 1, 8) == ("Identity", 0.0)           # int(0.45 * 8 * 0.5 / 30) = 0
    assert spec.op_value("Posterize", 0.0, 1, 112) == ("Posterize", 8.0) and spec.op_value("Posterize", 30.0, 1, 112) == ("Posterize", 4.0)
    assert spec.op_value("Solarize", 30.0, 1, 112) == ("Solarize", 0.0) and spec.op_value("Solarize", 0.0, 1, 112) == ("Solarize", 255.0)
    from cstp_amd import randaug
    for name in spec.OPS:
        for m in MAGNITUDES + (0.4,):
            for sign in (-1, 1):
                for size in (8, 33, 112):
                    assert randaug.op_value(name, m, sign, size) == spec.op_value(name, m, sign, size)


def test_erase_fill_is_uniform_on_the_normalised_range():
    a = spec.erase_fill(4099, 0x0123456789ABCDEF)
    assert a.dtype == np.float32 and a.min() >= -1.0 and a.max() < 1.0 and abs(float(a.mean())) < 0.05
    assert np.array_equal(a[:64], spec.erase_fill(64, 0x0123456789ABCDEF)) and not np.array_equal(a[:64], spec.erase_fill(64, 1))
    frames = np.stack([textured(8, 1), textured(8, 2)])
    plain = spec.finish(frames, True)
    boxed = spec.finish(frames, True, (2, 1, 3, 5, 99))
    inside = np.zeros(plain.shape, dtype=bool)
    inside[:, :, 1:6, 2:5] = True
    assert np.array_equal(boxed[~inside], plain[~inside]) and not np.any(boxed[inside] == plain[inside])


# ---- the draws -------------------------------------------------------------------------------------------------------------------------
def test_draws_follow_the_spec_and_depend_on_the_seed_alone():
    from cstp_amd import randaug
    s = randaug.Settings(3, 11.0, 2.5, 0.6)
    seen_erase = 0
    for seed in range(200):
        got = randaug.draw(s, 33, randaug.clip_rng(seed))
        assert got == randaug.draw(s, 33, randaug.clip_rng(seed))
        assert got == spec.draw(3, 11.0, 2.5, 0.6, 33, randaug.clip_rng(seed))
        seen_erase += got[1] is not None
    assert 80 < seen_erase < 160
    assert randaug.draw(s, 33, randaug.clip_rng(1)) != randaug.draw(s, 33, randaug.clip_rng(2))
    assert randaug.draw(randaug.Settings(0, 9.0, 0.0, 0.0), 33, randaug.clip_rng(1)) == (None, None)


def test_every_operation_occurs_and_boxes_stay_inside():
    from cstp_amd import randaug
    s = randaug.Settings(2, 9.0, 0.0, 1.0)
    names, keys = set(), set()
    for seed in range(2000):
        for size in (8, 112):
            ops, erase = randaug.draw(s, size, randaug.clip_rng(seed))
            names.update(n for n, _ in ops)
            if erase is not None:
                x0, y0, w, h, key = erase
                assert 1 <= w < size and 1 <= h < size and 0 <= x0 and x0 + w <= size and 0 <= y0 and y0 + h <= size
                assert 0 <= key < 2 ** 64
                if size == 112:
                    keys.add(key)
    assert names == set(spec.OPS) and len(keys) > 1990             # one key per clip: ten rejected attempts in a row are rare
    with_std = randaug.Settings(4, 29.0, 5.0, 0.0)
    for seed in range(300):
        for name, value in randaug.draw(with_std, 112, randaug.clip_rng(seed))[0]:
            if name == "Rotate":
                assert abs(value) <= 30.0
            if name in ("TranslateX", "TranslateY"):
                assert abs(value) <= int(0.45 * 112) and value == int(value)


def test_plan_fields_are_untouched_by_the_flags():
    """The data set's draws with the flags on: frames, box, resized, window, jitter and flip equal those with the flags off, and
    the new fields are a function of (seed, epoch, index)."""
    import dataclasses
    from cstp_amd import clip_ops, randaug, sampler
    assert [f.name for f in dataclasses.fields(sampler.FtClipPlan)] == ["frames", "box", "resized", "window", "jitter", "flip", "randaug",
                                                                        "erase"]
    assert sampler.FtClipPlan([0], (0, 0, 1, 1), (1, 1), (0, 0)).randaug is None
    s = randaug.Settings(2, 9.0, 0.5, 0.5)

    class Stub(clip_ops.GpuLabelledVideos):                # plan() needs shapes only: no device, no videos
        def __init__(self, augment):
            self.videos = [np.zeros((70, 24, 32, 3), dtype=np.uint8), np.zeros((40, 24, 32, 3), dtype=np.uint8)]
            self.data_type, self.mode, self.t, self.size, self.pb_rate, self.seed, self.augment = "train", "img", 4, 16, 2, 5, augment

    on, off = Stub(s), Stub(None)
    some = False
    for epoch in (0, 3):
        for index in range(40):
            (va, a), (vb, b) = on.plan(index, epoch), off.plan(index, epoch)
            assert va == vb and b.randaug is None and b.erase is None
            assert dataclasses.replace(a, randaug=None, erase=None) == b
            assert len(a.randaug) == 2
            assert on.plan(index, epoch)[1] == a
            some = some or a.erase is not None
    assert some
    assert on.plan(1, 0)[1].randaug != on.plan(1, 1)[1].randaug or on.plan(1, 0)[1].erase != on.plan(1, 1)[1].erase


def test_frame_folder_plans_take_the_same_draws(tmp_path):
    """FrameLabelledFolder with the settings on: the same generator and salt as GpuLabelledVideos, the plan's other fields
    untouched, the new fields carried into the staged request; build_finetune hands the settings to 'train' only."""
    import argparse
    import dataclasses
    from cstp_amd import randaug
    from cstp_amd.frame_folder import FrameLabelledFolder, build_finetune
    from test_frame_folder_host import PB, SEED, SIZE, T, write_tree
    frame_dir, ann = write_tree(tmp_path)
    s = randaug.Settings(2, 9.0, 1.0, 0.5)
    on = FrameLabelledFolder("cuda:0", frame_dir, ann, 1, "train", "img", T, SIZE, PB, seed=SEED, randaug=(2, 9.0, 1.0), random_erase=0.5)
    off = FrameLabelledFolder("cuda:0", frame_dir, ann, 1, "train", "img", T, SIZE, PB, seed=SEED)
    assert on.augment == s and off.augment is None
    for index, epoch in ((0, 0), (3, 2), (5, 1), (1, 4)):
        a, b = on.plan(index, epoch), off.plan(index, epoch)
        seed = ((SEED * 1000003 + epoch) * 1000003 + index) * 101 + 11
        assert (a.randaug, a.erase) == randaug.draw(s, SIZE, randaug.clip_rng(seed))
        assert dataclasses.replace(a, randaug=None, erase=None) == b and b.randaug is None and b.erase is None
    plans, _, _ = on._request(((0, 3, 5), 2))
    assert [(p.randaug, p.erase) for p in plans] == [(on.plan(i, 2).randaug, on.plan(i, 2).erase) for i in (0, 3, 5)]
    opts = argparse.Namespace(frame_dir=frame_dir, annotation_path=ann, split=1, sample_duration=T, sample_size=112, pb_rate=PB,
                              manual_seed=SEED, n_workers=2)
    assert build_finetune(opts, "cuda:0", "train", "img", augment=s).augment == s
    assert build_finetune(opts, "cuda:0", "val", "img_val", augment=s).augment is None
    with pytest.raises(ValueError):
        FrameLabelledFolder("cuda:0", frame_dir, ann, 1, "val", "img_val", T, 112, PB, random_erase=0.5)


# ---- the operation tables ---------------------------------------------------------------------------------------------------------------
def test_tables_pack_every_operation():
    from cstp_amd import randaug, sampler
    assert randaug.ENTRY.itemsize == 32 and randaug.FINISH_ENTRY.itemsize == 32

    def plan(ops, erase=None):
        return sampler.FtClipPlan([0, 1], (0, 0, 8, 8), (8, 8), (0, 0), randaug=ops, erase=erase)
    plans = [plan([("Posterize", 5.0), ("Rotate", -12.0)], (1, 2, 3, 4, (7 << 32) | 9)), plan(None), plan([("TranslateY", -3.0)]),
             plan([("Color", 1.0), ("Solarize", 200.0), ("Equalize", 0.0)])]
    raw = randaug.tables(plans, [False, True, False, False], 33)
    assert randaug.n_layers(plans) == 3 and raw.dtype == np.uint8 and raw.size == (3 + 1) * 4 * 32
    lay = raw[:3 * 4 * 32].view(randaug.ENTRY).reshape(3, 4)
    fin = raw[3 * 4 * 32:].view(randaug.FINISH_ENTRY)
    assert lay["op"].tolist() == [[randaug.RA_POSTERIZE, 0, randaug.RA_SHIFT, 0], [randaug.RA_AFFINE, 0, 0, randaug.RA_SOLARIZE],
                                  [0, 0, 0, randaug.RA_EQUALIZE]]
    assert lay[0, 0]["a"][0] == 0xF8 and lay[0, 2]["a"].tolist() == [0, -3, 0, 0, 0, 0] and lay[1, 3]["a"][0] == 200
    from oracle import pil_ops
    assert lay[1, 0]["a"].tolist() == list(pil_ops.affine_fixed_coeffs(pil_ops.rotate_matrix(33, 33, -12.0)))
    assert randaug.entry("ShearX", 0.25, 33)[1] == list(pil_ops.affine_fixed_coeffs((1.0, 0.25, 0.0, 0.0, 1.0, 0.0)))
    assert randaug.entry("ShearY", -0.1, 33)[1] == list(pil_ops.affine_fixed_coeffs((1.0, 0.0, 0.0, -0.1, 1.0, 0.0)))
    assert fin["out_slot"].tolist() == [0, 1, 2, 3] and fin["flip"].tolist() == [0, 1, 0, 0]
    assert [fin[0][k] for k in ("x0", "y0", "w", "h", "key_lo", "key_hi")] == [1, 2, 3, 4, 9, 7] and fin[1]["w"] == 0
    with pytest.raises(ValueError):
        randaug.tables([plan(None, (30, 0, 4, 4, 1))], [False], 33)
    with pytest.raises(ValueError):
        randaug.entry("Blur", 1.0, 33)


# ---- flags ----------------------------------------------------------------------------------------------------------------------------------
def _opts(*argv):
    from cstp_amd.opts import parse_opts
    return parse_opts(list(argv))


def test_flags_parse_and_default_to_off():
    from cstp_amd import randaug
    o = _opts()
    assert (o.randaug_n, o.randaug_m, o.randaug_mstd, o.random_erase) == (0, 9.0, 0.0, 0.0)
    assert randaug.from_opts(o) is None
    assert randaug.from_opts(_opts("--dataset", "synthetic", "--randaug_m", "12")) is None       # off: nothing to refuse
    o = _opts("--dataset", "synthetic_video", "--transform_mode", "img", "--randaug_n", "2", "--randaug_m", "7.5", "--randaug_mstd",
              "0.5", "--random_erase", "0.25")
    assert randaug.from_opts(o) == randaug.Settings(2, 7.5, 0.5, 0.25)
    o = _opts("--dataset", "UcfFineTune", "--transform_mode", "img", "--random_erase", "1")
    assert randaug.from_opts(o) == randaug.Settings(0, 9.0, 0.0, 1.0)
    import cstp_amd.opts as opts_mod
    for flag in ("--randaug_n", "--randaug_m", "--randaug_mstd", "--random_erase"):
        assert flag in opts_mod.__doc__


@pytest.mark.parametrize("argv,flag", [
    (["--randaug_n", "5"], "--randaug_n"), (["--randaug_n", "-1"], "--randaug_n"),
    (["--randaug_n", "1", "--randaug_m", "30.5"], "--randaug_m"), (["--randaug_m", "-0.1"], "--randaug_m"),
    (["--randaug_m", "nan"], "--randaug_m"), (["--randaug_mstd", "-1"], "--randaug_mstd"), (["--randaug_mstd", "inf"], "--randaug_mstd"),
    (["--random_erase", "1.5"], "--random_erase"), (["--random_erase", "-0.5"], "--random_erase"),
    (["--dataset", "synthetic", "--transform_mode", "img", "--randaug_n", "1"], "--randaug_n"),
    (["--dataset", "synthetic", "--transform_mode", "img", "--random_erase", "0.5"], "--random_erase"),
    (["--dataset", "synthetic_video", "--transform_mode", "img_val", "--randaug_n", "1"], "--randaug_n"),
    (["--dataset", "synthetic_video", "--transform_mode", "numpy", "--random_erase", "0.5"], "--random_erase"),
    (["--dataset", "UcfFineTune", "--randaug_n", "2"], "--randaug_n"),                    # --transform_mode defaults to numpy
])
def test_refusals_name_the_flag(argv, flag):
    from cstp_amd import randaug
    with pytest.raises(ValueError) as e:
        randaug.from_opts(_opts(*argv))
    assert flag in str(e.value)


def test_only_training_clips_under_img_are_augmented():
    from cstp_amd import clip_ops
    assert clip_ops.augment_settings(None, 0.0, "val", "img_val") is None
    assert clip_ops.augment_settings((0, 9.0, 0.0), 0.0, "test", "img_test") is None
    assert clip_ops.augment_settings((2, 9.0, 0.0), 0.0, "train", "img").n == 2
    for data_type, mode in (("val", "img_val"), ("test", "img_test"), ("train", "img_val")):
        with pytest.raises(ValueError):
            clip_ops.augment_settings((1, 9.0, 0.0), 0.0, data_type, mode)
        with pytest.raises(ValueError):
            clip_ops.augment_settings(None, 0.5, data_type, mode)
    with pytest.raises(ValueError):
        clip_ops.augment_settings((9, 9.0, 0.0), 0.0, "train", "img")
    src = open(os.path.join(ROOT, "main_ft_mp.py")).read()
    assert "randaug.from_opts(opts)" in src and "--randaug_n" in src and "--random_erase" in src


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    from cstp_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cstp_hip.h")).read(), flags=re.S)
    assert "#define CSTP_ABI_VERSION 18" in header and _lib.ABI_VERSION == 18
    lib = _lib.load()
    for name in ("cstp_randaug_layer", "cstp_randaug_finish", "cstp_randaug_entry_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.cstp_abi_version() == 18 and lib.cstp_randaug_entry_bytes() == 32
    assert os.path.isfile(os.path.join(ROOT, "cstp_amd", "csrc", "randaug.h"))
    import __graft_entry__ as entry
    assert entry.SOURCES == ["igemm.hip", "bn.hip", "misc.hip", "clip.hip", "b16.hip", "gate.hip", "mixed.hip", "retrieve.hip"]


def test_entry_points_refuse_bad_tables_before_any_launch():
    from cstp_amd import _lib, randaug
    lib = _lib.load()
    one = ctypes.c_void_p(64)                           # never dereferenced: the checks fail first
    two = ctypes.c_void_p(128)

    def layer(entries, b=None, t=2, s=8, src=one, dst=two, lut=None, mean=None):
        tab = np.zeros(len(entries), dtype=randaug.ENTRY)
        tab["factor"] = 1.0
        for i, e in enumerate(entries):
            tab[i] = e
        return lib.cstp_randaug_layer(None, src, dst, one, tab.ctypes.data, len(entries) if b is None else b, t, s, lut, mean)

    zero = [0] * 6
    for call, needle in [
        (lambda: layer([(0, zero, 1.0)], dst=one), b"aliased"),
        (lambda: layer([(0, zero, 1.0)], s=5000), b"bad shape"),
        (lambda: layer([(0, zero, 1.0)], b=0), b"bad shape"),
        (lambda: layer([(11, zero, 1.0)]), b"unknown operation"),
        (lambda: layer([(-1, zero, 1.0)]), b"unknown operation"),
        (lambda: layer([(randaug.RA_BRIGHTNESS, zero, float("nan"))]), b"blend factor"),
        (lambda: layer([(randaug.RA_POSTERIZE, [256] + [0] * 5, 1.0)]), b"posterize"),
        (lambda: layer([(randaug.RA_SOLARIZE, [-1] + [0] * 5, 1.0)]), b"solarize"),
        (lambda: layer([(randaug.RA_SHIFT, [1 << 20] + [0] * 5, 1.0)]), b"shift"),
        (lambda: layer([(randaug.RA_AFFINE, [1 << 20] + [0] * 5, 1.0)]), b"affine"),
        (lambda: layer([(0, zero, 1.0), (randaug.RA_EQUALIZE, zero, 1.0)]), b"need the lut"),
        (lambda: layer([(randaug.RA_CONTRAST, zero, 0.5)], lut=one), b"need the lut"),
    ]:
        rc = call()
        msg = lib.cstp_last_error()
        assert rc != 0 and needle in msg, (rc, msg, needle)

    def finish(entries, s=8, out_slots=2):
        tab = np.zeros(len(entries), dtype=randaug.FINISH_ENTRY)
        for i, e in enumerate(entries):
            tab[i] = e
        return lib.cstp_randaug_finish(None, one, two, one, tab.ctypes.data, len(entries), 2, s, out_slots)

    for entries, needle in [([(2, 0, 0, 0, 0, 0, 0, 0)], b"output slot"), ([(-1, 0, 0, 0, 0, 0, 0, 0)], b"output slot"),
                            ([(0, 0, 6, 0, 3, 1, 0, 0)], b"erased box"), ([(0, 0, 0, 7, 1, 2, 0, 0)], b"erased box"),
                            ([(0, 0, 0, 0, 0, 2, 0, 0)], b"erased box"), ([(0, 0, -1, 0, 1, 1, 0, 0)], b"erased box"),
                            ([(0, 0, 0, 0, -1, 0, 0, 0)], b"negative box")]:
        rc = finish(entries)
        msg = lib.cstp_last_error()
        assert rc != 0 and needle in msg, (entries, rc, msg)

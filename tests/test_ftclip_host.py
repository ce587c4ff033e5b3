"""Host decisions of the fine-tune / validation / video-test clip path (cstp_amd.sampler: UcfFineTune's frame selection,
datasets.py:1003-1097, and the 'img' / 'img_val' / 'img_test' transforms, preprocess_data.py:440-476, 584-664, 815-864,
1131-1149), checked without a GPU: the draw order against the reference's sequence restated by hand, frame lists against lists
written out here, the ClipScale / ClipCenterCrop geometry, the forced fallback of ClipRandomSizedCrop, and the numpy chain
through oracle/pil_ops against the PIL calls the reference makes.  ``reference_clip`` below restates the reference's data path
(frame selection + transform) on its own, from one random.Random; tests/test_ftclip_gpu.py holds the GPU path against it."""
import math
import random

import numpy as np
import pytest
from PIL import Image

from oracle import pil_ops

COLOUR = {"brightness": pil_ops.adjust_brightness, "contrast": pil_ops.adjust_contrast,
          "saturation": pil_ops.adjust_saturation, "hue": pil_ops.adjust_hue}


# ---- the reference's data path, restated with PIL (crop / resize) and oracle/pil_ops (colour jitter, tensor) -------------------
def _resize(im, w, h, backend):
    if backend == "pil":
        return np.asarray(Image.fromarray(im).resize((w, h), Image.BICUBIC))
    return pil_ops.resize_bicubic(im, w, h)


def _crop(im, box, backend):
    if backend == "pil":
        return np.asarray(Image.fromarray(im).crop(box))
    return pil_ops.crop(im, box)


def clip_scale(clip, size, backend):
    """ClipScale(size) (preprocess_data.py:843-864)."""
    h, w = clip[0].shape[:2]
    if (w <= h and w == size) or (h <= w and h == size):
        return clip
    if w < h:
        ow, oh = size, int(size * h / w)
    else:
        ow, oh = int(size * w / h), size
    return [_resize(im, ow, oh, backend) for im in clip]


def clip_center_crop(clip, size, backend):
    """ClipCenterCrop(size) (preprocess_data.py:815-840)."""
    h, w = clip[0].shape[:2]
    x1 = int(round((w - size) / 2.))
    y1 = int(round((h - size) / 2.))
    return [_crop(im, (x1, y1, x1 + size, y1 + size), backend) for im in clip]


def reference_transform(clip, mode, size, r, backend="pil"):
    """get_transforms(mode) (preprocess_data.py:1131-1149) up to ClipToTensor: list of uint8 [H][W][3] -> list of uint8
    [size][size][3], every draw from ``r`` in the reference's order."""
    if mode == "img":
        h, w = clip[0].shape[:2]
        done = None
        if r.random() < 1.0:                                    # ClipRandomSizedCrop :449
            for _ in range(10):
                target_area = r.uniform(0.2, 1) * (w * h)
                aspect_ratio = r.uniform(3. / 4, 4. / 3)
                cw = int(round(math.sqrt(target_area * aspect_ratio)))
                chh = int(round(math.sqrt(target_area / aspect_ratio)))
                if r.random() < 0.5:
                    cw, chh = chh, cw
                if cw <= w and chh <= h:
                    x1 = r.randint(0, w - cw)
                    y1 = r.randint(0, h - chh)
                    done = [_resize(_crop(im, (x1, y1, x1 + cw, y1 + chh), backend), size, size, backend) for im in clip]
                    break
            if done is None:                                    # the fallback :470-473
                done = clip_center_crop(clip_scale(clip, size, backend), size, backend)
        clip = done
        if r.random() < 0.3:                                    # ClipColorJitter(0.4, 0.4, 0.4, 0.1, p = 0.3) :659-664
            ops = [("brightness", r.uniform(0.6, 1.4)), ("contrast", r.uniform(0.6, 1.4)), ("saturation", r.uniform(0.6, 1.4)),
                   ("hue", r.uniform(-0.1, 0.1))]
            r.shuffle(ops)
            for op, factor in ops:
                clip = [COLOUR[op](im, factor) for im in clip]
        return clip
    assert mode in ("img_val", "img_test")
    short = {112: 128, 224: 256}[size]
    return clip_center_crop(clip_scale(clip, short, backend), size, backend)


def reference_train_frames(total, t, pb, r):
    """_get_train_clip / _get_val_clip (datasets.py:1003-1060), 0-based."""
    clip_range = (t - 1) * pb
    if total - clip_range <= 0:
        index_clip, idx_frame = [], 0
        while len(index_clip) < t:
            index_clip.append(idx_frame)
            idx_frame += pb
            if idx_frame >= total:
                idx_frame = 0
        start_frame = 1
    else:
        start_frame = r.randint(1, total - clip_range)
        index_clip = list(np.arange(0, clip_range + 1, pb))
    return [int(start_frame + i) - 1 for i in index_clip]


def reference_test_frames(total, t, pb):
    """_get_test_clip (datasets.py:1062-1081), 0-based, with the reference's numpy calls."""
    clip_range = (t - 1) * pb
    if total - clip_range <= 0:
        seq_idx, idx_frame = [], 1
        while len(seq_idx) < t:
            seq_idx.append(idx_frame)
            idx_frame += pb
            if idx_frame >= total:
                idx_frame = 1
        seq_idx = np.expand_dims(seq_idx, 0)
    else:
        start = np.expand_dims(np.arange(1, total - clip_range + 1, clip_range), 1)
        seq_idx = np.expand_dims(np.arange(t) * pb, 0) + start
        last = np.expand_dims(np.arange(total - clip_range, total + 1, pb), 0)
        seq_idx = np.append(seq_idx, last, 0)
    return [[int(i) - 1 for i in idx] for idx in seq_idx]


def to_tensor(clip):
    """ClipToTensor + ClipNormalize('tf') + torch.stack(clip).transpose(0, 1): fp32 [3][T][S][S]."""
    return np.stack([pil_ops.to_tensor_tf(im) for im in clip], axis=1)


def reference_clip(video, t, size, pb, mode, r, backend="pil"):
    """One train / val item of UcfFineTune.__getitem__ from video uint8 [F][H][W][3]: fp32 [3][T][S][S]."""
    frames = reference_train_frames(video.shape[0], t, pb, r)
    return to_tensor(reference_transform([video[f] for f in frames], mode, size, r, backend))


def reference_video(video, t, size, pb, backend="pil"):
    """One test item: fp32 [n_clips][3][T][S][S] (np.stack(clip_batch).transpose(0, 2, 1, 3, 4), datasets.py:1001)."""
    return np.stack([to_tensor(reference_transform([video[f] for f in idx], "img_test", size, None, backend))
                     for idx in reference_test_frames(video.shape[0], t, pb)])


def plan_clip_u8(video, plan, size):
    """What a sampler.FtClipPlan SAYS, executed with oracle/pil_ops: crop(box) -> resize(resized) -> window -> jitter."""
    out = []
    for f in plan.frames:
        im = pil_ops.crop(video[f], plan.box)
        rw, rh = plan.resized
        if (rw, rh) != (im.shape[1], im.shape[0]):
            im = pil_ops.resize_bicubic(im, rw, rh)
        wx, wy = plan.window
        im = pil_ops.crop(im, (wx, wy, wx + size, wy + size))
        for op, factor in (plan.jitter or ()):
            im = COLOUR[op](im, factor)
        out.append(im)
    return out


def noise_video(frames, h, w, seed):
    rs = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    base = 127 + 90 * np.sin(xs / 9.0 + ys / 13.0)[None, :, :, None] * np.ones((frames, 1, 1, 3))
    return np.clip(base + rs.randint(-40, 40, size=(frames, h, w, 3)), 0, 255).astype(np.uint8)


# ---- draw order -----------------------------------------------------------------------------------------------------------------
def test_ft_draw_order_matches_the_reference_sequence():
    """The reference consumes the global `random` stream as: train start (datasets.py:1017), ClipRandomSizedCrop's p draw and
    attempts (preprocess_data.py:449-462), ClipColorJitter's p draw, four uniforms and shuffle (:660, 639-654)."""
    from cstp_amd import sampler
    total, t, pb, w, h = 200, 16, 4, 320, 240
    seen_jitter = seen_plain = seen_retry = False
    for seed in range(60):
        plan = sampler.sample_ft_clip(total, w, h, t, 112, pb, "img", random.Random(seed))
        r = random.Random(seed)
        start = r.randint(1, total - 15 * 4)
        assert plan.frames == [start - 1 + 4 * i for i in range(16)]
        r.random()                                              # the p = 1.0 draw, consumed
        attempts = 0
        while True:
            attempts += 1
            area = r.uniform(0.2, 1) * (w * h)
            aspect = r.uniform(3. / 4, 4. / 3)
            cw, ch = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
            if r.random() < 0.5:
                cw, ch = ch, cw
            if cw <= w and ch <= h:
                x1 = r.randint(0, w - cw)
                y1 = r.randint(0, h - ch)
                break
        seen_retry |= attempts > 1
        assert plan.box == (x1, y1, x1 + cw, y1 + ch) and plan.resized == (112, 112) and plan.window == (0, 0)
        if r.random() < 0.3:
            ops = [("brightness", r.uniform(0.6, 1.4)), ("contrast", r.uniform(0.6, 1.4)), ("saturation", r.uniform(0.6, 1.4)),
                   ("hue", r.uniform(-0.1, 0.1))]
            r.shuffle(ops)
            assert plan.jitter == ops
            seen_jitter = True
        else:
            assert plan.jitter is None
            seen_plain = True
        assert plan.flip is False
        # nothing else was drawn: the next value of both streams agrees
        r2 = random.Random(seed)
        sampler.sample_ft_clip(total, w, h, t, 112, pb, "img", r2)
        assert r2.random() == r.random()
    assert seen_jitter and seen_plain and seen_retry


def test_val_draws_a_random_start_and_nothing_else():
    """_get_val_clip draws its start like the train clip (datasets.py:1047); 'img_val' draws nothing."""
    from cstp_amd import sampler
    for seed in range(20):
        r2 = random.Random(seed)
        plan = sampler.sample_ft_clip(200, 320, 240, 16, 112, 4, "img_val", r2)
        r = random.Random(seed)
        start = r.randint(1, 200 - 60)
        assert plan.frames == [start - 1 + 4 * i for i in range(16)] and plan.jitter is None
        assert r2.random() == r.random()
    # a short video draws nothing at all
    r2 = random.Random(3)
    sampler.sample_ft_clip(40, 320, 240, 16, 112, 4, "img_val", r2)
    assert r2.random() == random.Random(3).random()


# ---- frame lists ----------------------------------------------------------------------------------------------------------------
def test_frame_lists_written_out():
    from cstp_amd import sampler
    t, pb = 8, 4                                                # clip_range 28
    # long video: start drawn in 1..(100 - 28), 0-based list from start - 1
    r = random.Random(5)
    start = random.Random(5).randint(1, 72)
    assert sampler.ft_clip_frames(100, t, pb, r) == [start - 1 + d for d in (0, 4, 8, 12, 16, 20, 24, 28)]
    # short video (total 10 <= 28): wrap-around from index 0, start_frame 1 -> 0-based 0, 4, 8, then 12 >= 10 wraps
    assert sampler.ft_clip_frames(10, t, pb, random.Random(0)) == [0, 4, 8, 0, 4, 8, 0, 4]
    # total == clip_range is still short: 28 >= 28 wraps
    assert sampler.ft_clip_frames(28, t, pb, random.Random(0)) == [0, 4, 8, 12, 16, 20, 24, 0]
    # total == clip_range + 1: randint(1, 1), the one possible window; the draw is consumed
    r = random.Random(9)
    assert sampler.ft_clip_frames(29, t, pb, r) == [0, 4, 8, 12, 16, 20, 24, 28]
    r9 = random.Random(9)
    r9.randint(1, 1)
    assert r.random() == r9.random()
    # test windows of a 100-frame video: starts 1, 29, 57 (1-based), the extra last one from 72 to 100
    assert sampler.ft_test_frames(100, t, pb) == [
        [0, 4, 8, 12, 16, 20, 24, 28], [28, 32, 36, 40, 44, 48, 52, 56], [56, 60, 64, 68, 72, 76, 80, 84],
        [71, 75, 79, 83, 87, 91, 95, 99]]
    # total == clip_range + 1: one regular window and the last one, identical
    assert sampler.ft_test_frames(29, t, pb) == [[0, 4, 8, 12, 16, 20, 24, 28]] * 2
    # short test video: the 1-based wrap 1, 5, 9 then 13 >= 10 -> 1; frame `total` (1-based 10, 0-based 9) is never read
    assert sampler.ft_test_frames(10, t, pb) == [[0, 4, 8, 0, 4, 8, 0, 4]]
    assert sampler.ft_test_frames(9, t, pb) == [[0, 4, 0, 4, 0, 4, 0, 4]]          # 1, 5, then 9 >= 9 wraps: frame 9 unread
    # ... and all of them against the reference's own numpy statements
    for total in (9, 10, 28, 29, 30, 57, 100, 300):
        assert sampler.ft_test_frames(total, t, pb) == reference_test_frames(total, t, pb)
        assert sampler.ft_clip_frames(total, t, pb, random.Random(total)) == reference_train_frames(total, t, pb, random.Random(total))
    assert sampler.ft_test_frames(300, 16, 4) == reference_test_frames(300, 16, 4) and len(sampler.ft_test_frames(300, 16, 4)) == 5


# ---- geometry -------------------------------------------------------------------------------------------------------------------
def test_scale_and_center_crop_geometry():
    from cstp_amd import sampler
    assert sampler.clip_scale_size(320, 240, 128) == (170, 128)
    assert sampler.center_crop_origin(170, 128, 112) == (29, 8)
    plan = sampler.spatial_plan("img_val", [0], 320, 240, 112, None)
    assert (plan.box, plan.resized, plan.window, plan.jitter) == ((0, 0, 320, 240), (170, 128), (29, 8), None)
    # 128 x 171 frames: ClipScale returns the clip unchanged; round(29.5) is 30 (half to even), not 29
    assert sampler.clip_scale_size(171, 128, 128) == (171, 128)
    plan = sampler.spatial_plan("img_test", [0], 171, 128, 112, None)
    assert (plan.resized, plan.window) == ((171, 128), (30, 8))
    # portrait frames scale the width; 224 takes short side 256
    assert sampler.clip_scale_size(240, 320, 128) == (128, 170)
    assert sampler.clip_scale_size(320, 240, 256) == (341, 256)
    plan = sampler.spatial_plan("img_val", [0], 320, 240, 224, None)
    assert (plan.resized, plan.window) == ((341, 256), (58, 16))
    plans = sampler.plan_test_video(300, 320, 240, 16, 112, 4)
    assert len(plans) == 5 and all(p.window == (29, 8) for p in plans)


def test_forced_fallback_on_frames_no_crop_fits():
    """320 x 32 frames reject every ClipRandomSizedCrop attempt (the smallest candidate side is sqrt(0.2 * 10240 * 3 / 4) = 39
    > 32 whichever way it is swapped): after 10 attempts the fallback ClipScale(size) -> ClipCenterCrop(size)."""
    from cstp_amd import sampler
    for seed in range(50):
        r = random.Random(seed)
        plan = sampler.spatial_plan("img", [0], 320, 32, 112, r)
        assert (plan.box, plan.resized, plan.window) == ((0, 0, 320, 32), (1120, 112), (504, 0))
        # exactly 1 + 10 * 3 draws, then the jitter's
        q = random.Random(seed)
        for _ in range(31):
            q.random()
        jit = q.random() < 0.3
        assert (plan.jitter is not None) == jit
    # 320 x 240 never falls back in practice
    for seed in range(300):
        assert sampler.spatial_plan("img", [0], 320, 240, 112, random.Random(seed)).resized == (112, 112)


# ---- Pillow equality --------------------------------------------------------------------------------------------------------------
def test_numpy_chain_equals_the_pil_chain():
    from cstp_amd import sampler
    video = noise_video(3, 240, 320, 0)
    clip = [video[0], video[2]]
    for mode, size in (("img_val", 112), ("img_test", 224)):    # 240 x 320 -> 128 x 170 / 256 x 341
        a = reference_transform(clip, mode, size, None, "pil")
        b = reference_transform(clip, mode, size, None, "numpy")
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[0].shape == (size, size, 3)
    for seed in range(6):                                        # random-sized crops
        a = reference_transform(clip, "img", 112, random.Random(seed), "pil")
        b = reference_transform(clip, "img", 112, random.Random(seed), "numpy")
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    thin = noise_video(2, 32, 320, 1)                            # the upscaling fallback 32 x 320 -> 112 x 1120
    a = reference_transform(list(thin), "img", 112, random.Random(1), "pil")
    b = reference_transform(list(thin), "img", 112, random.Random(1), "numpy")
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # ... and what the PLAN says (box -> resize -> window), executed in numpy, is that same clip
    for vid, mode, seed in ((video, "img", 2), (video, "img_val", 0), (thin, "img", 1)):
        plan = sampler.spatial_plan(mode, [0, 1], vid.shape[2], vid.shape[1], 112, random.Random(seed))
        want = reference_transform([vid[0], vid[1]], mode, 112, random.Random(seed), "pil")
        assert all(np.array_equal(x, y) for x, y in zip(plan_clip_u8(vid, plan, 112), want))
    unchanged = noise_video(2, 128, 171, 2)                      # ClipScale returns 128 x 171 frames as they are
    plan = sampler.spatial_plan("img_val", [0, 1], 171, 128, 112, None)
    want = reference_transform(list(unchanged), "img_val", 112, None, "pil")
    assert np.array_equal(want[0], unchanged[0][8:120, 30:142])
    assert all(np.array_equal(x, y) for x, y in zip(plan_clip_u8(unchanged, plan, 112), want))


def test_equal_size_tables_are_the_identity():
    """The executor serves 'unchanged' (ClipScale :853) as a resize n -> n: Pillow's bicubic coefficients at integer offsets are
    exactly (0, 1 << 22, 0), so the pass copies."""
    from cstp_amd.clip_ops import resize_tables, window_rows
    for n in (112, 128, 171):
        ks, b, k = resize_tables(n, n)
        for xx in range(n):
            x0, cnt = b[xx]
            row = np.zeros(n, dtype=np.int64)
            row[x0:x0 + cnt] = k[xx, :cnt]
            assert row[xx] == 1 << 22 and row.sum() == 1 << 22
    # rows 8..119 with Pillow's tap span int(c - 2 + 0.5) .. int(c + 2 + 0.5) - 1 around c = yy + 0.5: rows 7..121
    assert window_rows(128, 128, 8, 112) == (7, 115)
    first, rows = window_rows(240, 128, 8, 112)
    assert 0 < first and first + rows < 240                      # the window skips the rows above and below it


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from cstp_amd import sampler
    for mode in ("numpy", "numpy_val"):
        with pytest.raises(ValueError, match="cv2"):
            sampler.sample_ft_clip(100, 320, 240, 16, 112, 4, mode, random.Random(0))
        with pytest.raises(ValueError, match="cv2"):
            sampler.plan_test_video(100, 320, 240, 16, 112, 4, mode)
    with pytest.raises(ValueError):
        sampler.sample_ft_clip(100, 320, 240, 16, 112, 4, "pre_train", random.Random(0))
    for size in (96, 128, 160):
        with pytest.raises(ValueError, match="short_size"):
            sampler.sample_ft_clip(100, 320, 240, 16, size, 4, "img_val", random.Random(0))
        with pytest.raises(ValueError, match="short_size"):
            sampler.plan_test_video(100, 320, 240, 16, size, 4)
    # 'img' itself takes any size (ClipRandomSizedCrop(size))
    assert sampler.sample_ft_clip(100, 320, 240, 16, 96, 4, "img", random.Random(0)).resized == (96, 96)


def test_loader_shards_and_epoch_seeding_without_a_gpu():
    """GpuLabelledLoader's index plans and GpuLabelledVideos.plan are host logic (no frame is touched)."""
    from cstp_amd.clip_ops import GpuLabelledLoader, GpuLabelledVideos

    class Stub:
        data_type = "train"

        def __len__(self):
            return 37

    stub = Stub()
    a, b = GpuLabelledLoader(stub, 4, 0, 2, seed=3), GpuLabelledLoader(stub, 4, 1, 2, seed=3)
    assert len(a) == len(b) == 4 and not set(a.indices()) & set(b.indices()) and len(a.indices()) == 18
    a.set_epoch(1)
    assert a.indices() != GpuLabelledLoader(stub, 4, 0, 2, seed=3).indices()
    stub.data_type = "val"
    v = GpuLabelledLoader(stub, 4, 1, 2)
    assert v.indices() == list(range(1, 37, 2)) and len(v) == 5                  # in order, the partial batch kept
    stub.data_type = "test"
    assert len(GpuLabelledLoader(stub)) == 37
    # plans: a pure function of (seed, epoch, index); another epoch is another augmentation
    ds = GpuLabelledVideos.__new__(GpuLabelledVideos)
    ds.data_type, ds.mode, ds.t, ds.size, ds.pb_rate, ds.seed = "train", "img", 16, 112, 4, 1

    class V:
        shape = (200, 240, 320, 3)

    ds.videos = [V()]
    assert ds.plan(5, 0) == ds.plan(5, 0) and ds.plan(5, 0) != ds.plan(5, 1) and ds.plan(5, 0) != ds.plan(6, 0)


def test_batch_entry_point_checks_every_descriptor_before_any_launch():
    """cstp_clip_batch_forward reads the host copy of the descriptor table and refuses any offset, window or slot that leaves the
    buffer sizes it is given -- pure host code, nothing is enqueued (the device pointers here are never dereferenced)."""
    from cstp_amd import _lib, clip_ops
    lib = _lib.load()
    assert lib.cstp_clip_batch_desc_bytes() == clip_ops._BATCH_DESC.itemsize == 120
    desc = np.zeros(1, dtype=clip_ops._BATCH_DESC)
    one = 64
    desc[0] = (one, one, one, one, one, 0, 4, 8, 8, 0, 0, 0, 5, 5, 8, 8, 0, 0, 0, 8, 0, 0, -1, 0)

    def args(d, tmp_pixels=1 << 20):
        return (None, one, d.ctypes.data, 1, 2, 8, one, 2, one, tmp_pixels, one, 1, None, 0)
    for change, needle in ((dict(idx_off=1), b"index array"), (dict(win_x=1), b"output window"), (dict(tmp_off=1 << 20), b"tmp of"),
                           (dict(out_slot=1), b"output slot"), (dict(out8_slot=0), b"exactly one"), (dict(frames=0), b"null pointer"),
                           (dict(rows=0), b"bad tmp rows"), (dict(w=0), b"bad frame shape")):
        d = desc.copy()
        for k, v in change.items():
            d[k] = v
        assert lib.cstp_clip_batch_forward(*args(d)) != 0 and needle in lib.cstp_last_error(), change
    assert lib.cstp_clip_batch_forward(*args(desc, tmp_pixels=2 * 8 * 8 - 1)) != 0 and b"tmp of" in lib.cstp_last_error()
    assert lib.cstp_clip_batch_forward(None, None, desc.ctypes.data, 1, 2, 8, one, 2, one, 128, one, 1, None, 0) != 0
    assert b"null argument" in lib.cstp_last_error()


def _windowed_clip_u8(video, plan, size):
    """The two passes of cstp_clip_batch_forward as the kernels index them, in numpy, from the executor's own tables
    (clip_ops.resize_tables / window_rows): only the window's columns, only the tmp rows its vertical taps read."""
    from cstp_amd.clip_ops import resize_tables, window_rows
    x0b, y0b, x1b, y1b = plan.box
    (rw, rh), (wx, wy) = plan.resized, plan.window
    _, bh, kh = resize_tables(x1b - x0b, rw)
    _, bv, kv = resize_tables(y1b - y0b, rh)
    first, rows = window_rows(y1b - y0b, rh, wy, size)
    out = []
    for f in plan.frames:
        src = pil_ops.crop(video[f], plan.box).astype(np.int64)
        tmp = np.zeros((rows, size, 3), dtype=np.int64)
        for xx in range(size):
            x0, n = bh[wx + xx]
            acc = (1 << 21) + (src[first:first + rows, x0:x0 + n] * kh[wx + xx, :n].astype(np.int64)[None, :, None]).sum(axis=1)
            tmp[:, xx] = np.clip(acc >> 22, 0, 255)
        img = np.zeros((size, size, 3), dtype=np.uint8)
        for yy in range(size):
            y0, n = bv[wy + yy]
            y0 -= first
            assert 0 <= y0 and y0 + n <= rows                    # the window's taps stay inside the rows kept
            acc = (1 << 21) + (tmp[y0:y0 + n] * kv[wy + yy, :n].astype(np.int64)[:, None, None]).sum(axis=0)
            img[yy] = np.clip(acc >> 22, 0, 255)
        out.append(img)
    return out


def test_windowed_passes_equal_resize_then_crop():
    """Scale -> centre-crop computed as a window of the resize (what the batched kernels do) equals Pillow's resize followed by
    its crop bit for bit, for the downscale, the identity ('unchanged' frames), the upscaling fallback, 224 and random crops."""
    from cstp_amd import sampler
    cases = [(noise_video(2, 240, 320, 0), "img_val", 112), (noise_video(2, 128, 171, 1), "img_test", 112),
             (noise_video(2, 32, 320, 2), "img", 112), (noise_video(2, 240, 320, 3), "img_val", 224),
             (noise_video(2, 320, 240, 4), "img_val", 112), (noise_video(2, 240, 320, 5), "img", 112)]
    for video, mode, size in cases:
        plan = sampler.spatial_plan(mode, [0, 1], video.shape[2], video.shape[1], size, random.Random(11))
        plan.jitter = None
        r = random.Random(11)
        want = reference_transform([video[0], video[1]], mode, size, r, "pil") if mode != "img" else None
        if want is None:                                         # 'img': the reference without its jitter = the plan in pil_ops
            want = plan_clip_u8(video, plan, size)
        got = _windowed_clip_u8(video, plan, size)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), (video.shape, mode, size)

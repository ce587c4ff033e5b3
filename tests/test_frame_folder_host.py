"""Host side of the frame-folder data sources (cstp_amd.frame_folder: UcfRepreBYOLSpPre / UcfFineTune from JPEG frame folders),
checked without a GPU: list parsing and paths, the union of a sample's frames and the remap of its plan, plans as a pure
function of (seed, epoch, index), the coverage of the plans the GPU tests use, the rotation check of the batched entry point and
the refusals.  The JPEG trees are written under tmp_path with Pillow (smooth patterns plus noise, quality 90);
``pil_clip`` below is the reference's chain on PIL images written out, and tests/test_frame_folder_gpu.py holds the GPU path
against it."""
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance, ImageFilter

PIL_ROT = {90: Image.ROTATE_90, 180: Image.ROTATE_180, 270: Image.ROTATE_270}
T, SIZE, PB = 4, 16, 2
# (list entry, label, frames, height, width, grayscale JPEG): non-square frames of different sizes; the 3- and 5-frame videos
# take the wrap-around branch of the fine-tune sampling (clip_range 6), the 3-frame one that of the pre-training too
VIDEOS = [("Archery/v_Archery_g01_c01.avi", 3, 40, 37, 53, False), ("Archery/v_Archery_g02_c03.avi", 3, 3, 48, 36, False),
          ("Bowling/v_Bowling_g01_c02.avi", 7, 17, 60, 44, True), ("Bowling/v_Bowling_g05_c01.avi", 7, 25, 37, 53, False),
          ("YoYo/v_YoYo_g03_c04.avi", 11, 5, 48, 36, False), ("YoYo/v_YoYo_g04_c01.avi", 11, 31, 41, 59, False)]
MISSING = "YoYo/v_YoYo_g09_c09.avi 11 12"
SEED, EPOCHS = 50, (0, 1, 2, 3)                         # what the GPU end-to-end tests draw their pairs from


def frame_image(video: int, frame: int, h: int, w: int, gray: bool) -> Image.Image:
    rs = np.random.RandomState(video * 1000 + frame)
    ys, xs = np.mgrid[0:h, 0:w]
    base = 127 + 80 * np.sin(xs / (5.0 + video) + ys / 7.0 + frame / 3.0)[:, :, None] * np.array([1.0, 0.7, -0.8])
    img = np.clip(base + rs.randint(-25, 25, size=(h, w, 3)), 0, 255).astype(np.uint8)
    return Image.fromarray(img, "RGB").convert("L") if gray else Image.fromarray(img, "RGB")


def write_tree(root, videos=VIDEOS, split=1, missing=True):
    """-> (frame_dir, annotation_path): <frame_dir>/<Class>/<v_name>/%05d.jpg and the two *_nframe.txt lists (the train list
    names every video, the test list every second one; both name one folder that does not exist)."""
    frame_dir, ann = os.path.join(str(root), "frames"), os.path.join(str(root), "labels")
    os.makedirs(ann, exist_ok=True)
    lines = []
    for v, (entry, label, n, h, w, gray) in enumerate(videos):
        folder = os.path.join(frame_dir, entry.split(".")[0])
        os.makedirs(folder, exist_ok=True)
        for f in range(n):
            frame_image(v, f, h, w, gray).save(os.path.join(folder, "%05d.jpg" % (f + 1)), quality=90)
        lines.append("%s %d %d" % (entry, label, n))
    extra = [MISSING] if missing else []
    with open(os.path.join(ann, "trainlist0%s_nframe.txt" % split), "w") as f:
        f.write("\n".join(lines[:2] + extra + lines[2:]) + "\n")
    with open(os.path.join(ann, "testlist0%s_nframe.txt" % split), "w") as f:
        f.write("\n".join(lines[::2] + extra) + "\n")
    return frame_dir, ann


def open_frames(folder, indices):
    """Image.open of the 0-based frames, as the reference opens them (non-RGB JPEGs converted)."""
    out = []
    for i in indices:
        im = Image.open(os.path.join(folder, "%05d.jpg" % (i + 1)))
        out.append(im if im.mode == "RGB" else im.convert("RGB"))
    return out


def tf_tensor(im) -> np.ndarray:
    """ToTensor -> x * 2 - 1: fp32 [3][H][W]."""
    t = torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1).float().div(255)
    return torch.clamp(t * 2 - 1, -1, 1).numpy()


def pil_clip(images, cp, size) -> np.ndarray:
    """One pre-training clip with Pillow, chained as the reference chains it: transpose -> crop -> resize(BICUBIC) ->
    [base_transform: rotate -> colour jitter in the drawn order -> channel gray -> Gaussian blur] -> [flip] -> ToTensor ->
    x * 2 - 1; ``images`` are the clip's frames in clip order.  fp32 [3][T][size][size]."""
    enh = {"brightness": ImageEnhance.Brightness, "contrast": ImageEnhance.Contrast, "saturation": ImageEnhance.Color}
    out = []
    for i, im in enumerate(images):
        if cp.rotate:
            im = im.transpose(PIL_ROT[cp.rotate])
        im = im.crop(cp.box).resize((size, size), Image.BICUBIC)
        if cp.base is not None:
            im = im.rotate(cp.base.angle)
            for op, fac in (cp.base.jitter or ()):
                if op == "hue":
                    h, s, v = im.convert("HSV").split()
                    nh = np.array(h, dtype=np.uint8)
                    with np.errstate(over="ignore"):
                        nh += np.array(fac * 255).astype(np.uint8)
                    im = Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB")
                else:
                    im = enh[op](im).enhance(fac)
            if cp.base.gray is not None:
                c = np.array(im)[:, :, cp.base.gray[i]]
                im = Image.fromarray(np.dstack([c, c, c]), "RGB")
            if cp.base.blur_sigma is not None:
                im = im.filter(ImageFilter.GaussianBlur(radius=cp.base.blur_sigma))
        if cp.flip:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        out.append(tf_tensor(im))
    return np.stack(out, axis=1)


def pair_source(root, **kw):
    from cstp_amd.frame_folder import FramePairFolder
    frame_dir, ann = write_tree(root)
    return FramePairFolder("cuda:0", frame_dir, ann, 1, "train", T, SIZE, seed=SEED, n_workers=4, **kw)


# ---- list parsing and paths ------------------------------------------------------------------------------------------------
def test_lists_folders_and_frame_names(tmp_path, capsys):
    from cstp_amd import frame_folder as ff
    frame_dir, ann = write_tree(tmp_path, split=2)
    assert ff.list_name("train", 2) == "trainlist02_nframe.txt"
    assert ff.list_name("val", 2) == ff.list_name("test", 2) == "testlist02_nframe.txt"
    with pytest.raises(ValueError):
        ff.list_name("training", 1)
    train = ff.read_list(ann, frame_dir, "train", 2)
    out = capsys.readouterr().out
    gone = os.path.join(frame_dir, "YoYo/v_YoYo_g09_c09")
    assert out.strip() == "%s does not exist" % gone                      # listed, absent: reported and skipped
    assert [(os.path.relpath(p, frame_dir), lab, n) for p, lab, n in train] == \
        [(e.split(".")[0], lab, n) for e, lab, n, _, _, _ in VIDEOS]
    test = ff.read_list(ann, frame_dir, "test", 2)
    assert test == ff.read_list(ann, frame_dir, "val", 2) == train[::2]
    # the folder name stops at the FIRST '.', the frame count is the list's (not the folder's), frames are 1-based %05d.jpg
    os.makedirs(os.path.join(frame_dir, "A", "v_x"))
    with open(os.path.join(ann, "trainlist07_nframe.txt"), "w") as f:
        f.write("A/v_x.part2.avi 4 99\n")
    assert ff.read_list(ann, frame_dir, "train", 7) == [(os.path.join(frame_dir, "A", "v_x"), 4, 99)]
    assert ff.frame_path("/d/A/v_x", 0) == "/d/A/v_x/00001.jpg" and ff.frame_path("/d/A/v_x", 122) == "/d/A/v_x/00123.jpg"
    assert all(os.path.exists(ff.frame_path(train[0][0], i)) for i in (0, 39)) and not os.path.exists(ff.frame_path(train[0][0], 40))
    assert ff.frame_size(ff.frame_path(train[0][0], 0)) == (53, 37) and ff.frame_size(ff.frame_path(train[2][0], 3)) == (44, 60)
    with pytest.raises(ff.FrameError, match="00041.jpg"):
        ff.frame_size(ff.frame_path(train[0][0], 40))


def test_decode_reports_the_file(tmp_path):
    from cstp_amd import frame_folder as ff
    frame_dir, ann = write_tree(tmp_path)
    data = ff.read_list(ann, frame_dir, "train", 1)
    dst = np.zeros((37, 53, 3), dtype=np.uint8)
    ff.decode_into(ff.frame_path(data[0][0], 4), dst)
    assert np.array_equal(dst, np.asarray(Image.open(ff.frame_path(data[0][0], 4))))
    gray = np.zeros((60, 44, 3), dtype=np.uint8)
    ff.decode_into(ff.frame_path(data[2][0], 1), gray)                     # a grayscale JPEG: .convert('RGB')
    assert Image.open(ff.frame_path(data[2][0], 1)).mode == "L"
    assert np.array_equal(gray, np.asarray(Image.open(ff.frame_path(data[2][0], 1)).convert("RGB")))
    with pytest.raises(ff.FrameError, match="00041.jpg"):
        ff.decode_into(ff.frame_path(data[0][0], 40), dst)                 # missing
    with pytest.raises(ff.FrameError, match="v_Archery_g02_c03.00001.jpg is 36 x 48"):
        ff.decode_into(ff.frame_path(data[1][0], 0), dst)                  # another size than planned
    broken = ff.frame_path(data[0][0], 2)
    with open(broken, "r+b") as f:
        f.truncate(200)
    with pytest.raises(ff.FrameError, match="00003.jpg"):
        ff.decode_into(broken, dst)
    assert ff.decode_threads(0) == 1 and ff.decode_threads(6) == 6 and ff.decode_threads(64) == 16


# ---- union and remap -------------------------------------------------------------------------------------------------------
def test_union_and_remap():
    from cstp_amd import frame_folder as ff, sampler
    overlapping = disjoint = wrapped = 0
    for seed in range(200):
        for total in (200, 24, 7, 5):
            idx_1, idx_2, tem, pb, _ = sampler.sample_frames(total, 8, random.Random(seed))
            unique, (r1, r2) = ff.union_remap([idx_1, idx_2])
            assert unique == sorted(set(idx_1) | set(idx_2))
            assert [unique[k] for k in r1] == idx_1 and [unique[k] for k in r2] == idx_2      # the same files
            if set(idx_1) & set(idx_2):
                overlapping += 1
                assert len(unique) < 2 * 8
            else:
                disjoint += 1
                assert len(unique) == 2 * 8
            if total - 7 * sampler.PACE[pb] <= 0:                  # the wrap-around branch: one frame list, twice
                wrapped += 1
                assert idx_1 == idx_2 and len(unique) <= 8 and max(unique) < total and tem == 0
                if len(set(idx_1)) < 8:
                    assert len(unique) < 8 and r1 == r2
    assert overlapping > 50 and disjoint > 50 and wrapped > 20


def test_requests_name_the_planned_files(tmp_path):
    """A staged request: per sample the union's files in frame order, the plan's indices remapped to positions in it."""
    from cstp_amd import frame_folder as ff
    ds = pair_source(tmp_path)
    assert len(ds) == 6 and ds.threads == 4
    indices = [0, 1, 2, 5]
    plans, samples = ds._request((tuple(indices), 1))
    for i, plan, (paths, h, w) in zip(indices, plans, samples):
        orig = ds.plan(i, 1)
        folder = ds.data[i][0]
        assert (h, w) == VIDEOS[i][3:5] and paths == sorted(paths) and len(set(paths)) == len(paths)
        assert len(paths) == len(set(orig.clip_1.frames) | set(orig.clip_2.frames))
        for got, want in ((plan.clip_1, orig.clip_1), (plan.clip_2, orig.clip_2)):
            assert [paths[k] for k in got.frames] == [ff.frame_path(folder, f) for f in want.frames]
            assert (got.rotate, got.box, got.flip, got.base) == (want.rotate, want.box, want.flip, want.base)
        assert (plan.spa_label, plan.tem_label, plan.pb_label, plan.rot_labels) == \
            (orig.spa_label, orig.tem_label, orig.pb_label, orig.rot_labels)
    # video 1 has 3 frames: the wrap-around branch, both clips read the same (repeated) frames
    assert len(samples[1][0]) <= 3 and plans[1].clip_1.frames == plans[1].clip_2.frames and plans[1].tem_label == 0
    ds.close()


# ---- plans -----------------------------------------------------------------------------------------------------------------
def test_plans_are_a_function_of_seed_epoch_and_index(tmp_path):
    from cstp_amd import sampler
    from cstp_amd.frame_folder import FrameLabelledFolder
    ds = pair_source(tmp_path)
    assert ds.plan(3, 0) == ds.plan(3, 0) and ds.plan(3, 0) != ds.plan(3, 1) and ds.plan(3, 0) != ds.plan(0, 0)
    for index, epoch in ((0, 0), (3, 2), (5, 1), (1, 4)):
        s = ((SEED * 1000003 + epoch) * 1000003 + index) * 101 + 11
        _, _, n, h, w, _ = VIDEOS[index]
        want = sampler.sample_pair(n, w, h, T, random.Random(s), np_rng=np.random.RandomState(s & 0x7fffffff))
        assert ds.plan(index, epoch) == want
    frame_dir, ann = ds.frame_dir, ds.annotation_path
    ft = FrameLabelledFolder("cuda:0", frame_dir, ann, 1, "train", "img", T, SIZE, PB, seed=SEED)
    assert ft.plan(0, 0) == ft.plan(0, 0) and ft.plan(0, 0) != ft.plan(0, 1)
    s = ((SEED * 1000003 + 2) * 1000003 + 3) * 101 + 11
    assert ft.plan(3, 2) == sampler.sample_ft_clip(25, 53, 37, T, SIZE, PB, "img", random.Random(s))
    assert ft.labels == [3, 3, 7, 7, 11, 11]
    test = FrameLabelledFolder("cuda:0", frame_dir, ann, 1, "test", "img_test", T, 112, PB)
    assert len(test) == 3 and test.plan(0) == sampler.plan_test_video(40, 53, 37, T, 112, PB)
    assert [len(test.plan(i)) for i in range(3)] == [len(sampler.ft_test_frames(n, T, PB)) for n in (40, 17, 5)]


def covered_plans(ds):
    return [cp for e in EPOCHS for i in range(len(ds)) for p in [ds.plan(i, e)] for cp in (p.clip_1, p.clip_2)]


def test_the_gpu_tests_plans_cover_every_branch(tmp_path):
    """The pairs the GPU end-to-end tests draw (SEED, EPOCHS, every video of the tree) take every rotation code, both flips, both
    transform branches and, within base_transform, each of jitter, gray and blur present and absent."""
    clips = covered_plans(pair_source(tmp_path))
    assert {c.rotate for c in clips} == {0, 90, 180, 270}
    assert {c.flip for c in clips} == {False, True}
    base = [c.base for c in clips if c.base is not None]
    assert base and len(base) < len(clips)
    assert {b.jitter is None for b in base} == {False, True}
    assert {b.gray is None for b in base} == {False, True}
    assert {b.blur_sigma is None for b in base} == {False, True}
    assert {c.rotate for c in clips if c.base is not None} >= {0, 90}          # rotated frames through the 8-bit branch too


# ---- the batched entry point ------------------------------------------------------------------------------------------------
def test_batch_entry_point_refuses_a_bad_rotation_before_any_launch():
    """cstp_clip_batch_forward checks desc.rot on the host copy of the table: pure host code, nothing is enqueued (the device
    pointers here are never dereferenced)."""
    from cstp_amd import _lib, clip_ops
    lib = _lib.load()
    assert lib.cstp_clip_batch_desc_bytes() == clip_ops._BATCH_DESC.itemsize == 120
    assert clip_ops._BATCH_DESC.names[-1] == "rot" and clip_ops._BATCH_DESC.fields["rot"][1] == 116
    assert _lib.ABI_VERSION == 18
    desc = np.zeros(1, dtype=clip_ops._BATCH_DESC)
    one = 64
    desc[0] = (one, one, one, one, one, 0, 4, 8, 8, 0, 0, 0, 5, 5, 8, 8, 0, 0, 0, 8, 0, 0, -1, 0)
    for rot in (45, -90, 360, 1):
        d = desc.copy()
        d["rot"] = rot
        assert lib.cstp_clip_batch_forward(None, one, d.ctypes.data, 1, 2, 8, one, 2, one, 1 << 20, one, 1, None, 0) != 0
        assert b"rotation" in lib.cstp_last_error(), rot
    for rot in (90, 180, 270):                   # a legal code passes the rotation check: the next refusal is another one
        d = desc.copy()
        d["rot"], d["win_x"] = rot, 1
        assert lib.cstp_clip_batch_forward(None, one, d.ctypes.data, 1, 2, 8, one, 2, one, 1 << 20, one, 1, None, 0) != 0
        assert b"output window" in lib.cstp_last_error()


def _rotated_passes_u8(frame, rot, box, size):
    """The two passes of cstp_clip_batch_forward for one frame as the kernels index them with desc.rot, in numpy, from the
    executor's own tables: every horizontal tap is mapped from the rotated frame to the stored one, taps beyond it read zero."""
    from cstp_amd.clip_ops import resize_tables
    h, w = frame.shape[:2]
    x0b, y0b, x1b, y1b = box
    _, bh, kh = resize_tables(x1b - x0b, size)
    _, bv, kv = resize_tables(y1b - y0b, size)
    first, rows = int(bv[0, 0]), int(bv[-1, 0] + bv[-1, 1] - bv[0, 0])
    tmp = np.zeros((rows, size, 3), dtype=np.int64)
    for y in range(rows):
        oy = y0b + first + y
        for xx in range(size):
            acc = np.full(3, 1 << 21, dtype=np.int64)
            for j in range(int(bh[xx, 1])):
                rx = x0b + int(bh[xx, 0]) + j
                if rot == 90:
                    sx, sy = w - 1 - oy, rx
                elif rot == 180:
                    sx, sy = w - 1 - rx, h - 1 - oy
                elif rot == 270:
                    sx, sy = oy, h - 1 - rx
                else:
                    sx, sy = rx, oy
                if 0 <= sx < w and 0 <= sy < h:
                    acc += frame[sy, sx].astype(np.int64) * int(kh[xx, j])
            tmp[y, xx] = np.clip(acc >> 22, 0, 255)
    out = np.zeros((size, size, 3), dtype=np.uint8)
    for yy in range(size):
        y0, n = int(bv[yy, 0]) - first, int(bv[yy, 1])
        acc = (1 << 21) + (tmp[y0:y0 + n] * kv[yy, :n].astype(np.int64)[:, None, None]).sum(axis=0)
        out[yy] = np.clip(acc >> 22, 0, 255)
    return out


def test_rotated_taps_as_the_kernel_maps_them_equal_pillow():
    """transpose -> crop -> resize(BICUBIC) with Pillow against the kernel's source indexing under every rotation code, on
    non-square frames with boxes on each border of the rotated frame and one reaching past it."""
    rs = np.random.RandomState(3)
    for h, w in ((37, 53), (48, 36)):
        frame = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        for rot in (0, 90, 180, 270):
            rw, rh = (h, w) if rot in (90, 270) else (w, h)
            for box in ((0, 0, rw - 9, rh - 7), (9, 6, rw, rh), (0, 0, rw, rh), (rw - 20, rh - 18, rw + 6, rh + 5)):
                im = Image.fromarray(frame, "RGB")
                if rot:
                    im = im.transpose(PIL_ROT[rot])
                want = np.asarray(im.crop(box).resize((12, 12), Image.BICUBIC))
                assert np.array_equal(_rotated_passes_u8(frame, rot, box, 12), want), (h, w, rot, box)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(tmp_path):
    import importlib.util
    from cstp_amd.frame_folder import FrameLabelledFolder
    from cstp_amd.opts import parse_opts
    frame_dir, ann = write_tree(tmp_path)
    for mode in ("numpy", "numpy_val"):
        with pytest.raises(ValueError, match="cv2"):
            FrameLabelledFolder("cuda:0", frame_dir, ann, 1, "train", mode, T, SIZE, PB)
    for data_type, mode in (("test", "img"), ("test", "img_val"), ("train", "img_test")):
        with pytest.raises(ValueError, match="img_test"):
            FrameLabelledFolder("cuda:0", frame_dir, ann, 1, data_type, mode, T, 112, PB)
    with pytest.raises(ValueError):
        FrameLabelledFolder("cuda:0", frame_dir, ann, 1, "val", "img_val", T, 96, PB)       # no short side bound for 96
    with pytest.raises(FileNotFoundError):
        FrameLabelledFolder("cuda:0", frame_dir, ann, 3, "train", "img", T, SIZE, PB)       # no list for that split
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def driver(name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    for name, build in (("main_byol", lambda m, o: m.build_dataset(o)), ("main_ft_mp", lambda m, o: m.build_dataset(o, "train")),
                        ("test", lambda m, o: m.build_dataset(o))):
        mod = driver(name)
        for dataset in ("Kin400RepreLMDB", "UCF101", "HMDB51"):
            opts = parse_opts(["--dataset", dataset, "--frame_dir", frame_dir, "--annotation_path", ann])
            opts.local_rank, opts.device = 0, "cuda:0"
            with pytest.raises(NotImplementedError):
                build(mod, opts)
    # the new names are built from the reference's flags, without touching a device
    opts = parse_opts(["--dataset", "UcfRepreBYOLSpPre", "--frame_dir", frame_dir, "--annotation_path", ann, "--split", "1",
                       "--n_workers", "6", "--sample_duration", "4", "--sample_size", "16"])
    opts.local_rank = 0
    ds = driver("main_byol").build_dataset(opts)
    assert len(ds) == 6 and ds.threads == 6 and (ds.t, ds.size) == (4, 16)
    opts = parse_opts(["--dataset", "UcfFineTune", "--frame_dir", frame_dir, "--annotation_path", ann, "--transform_mode", "img",
                       "--sample_duration", "4", "--pb_rate", "2"])
    opts.device = 0
    ft = driver("main_ft_mp")
    assert len(ft.build_dataset(opts, "train")) == 6
    val = ft.build_dataset(opts, "val")
    assert len(val) == 3 and val.mode == "img_val" and val.data_type == "val"
    opts.transform_mode, opts.device = "img_test", "cuda:0"
    assert driver("test").build_dataset(opts).data_type == "test"
    opts.transform_mode, opts.device = "numpy", 0
    with pytest.raises(ValueError, match="cv2"):
        ft.build_dataset(opts, "train")

"""The frame-folder data path on a real MI355X: rotation in the batched assembly kernels (cstp_clip_batch_forward through
cstp_amd.clip_ops.assemble_pairs), the base_transform branch of a batch, and FramePairFolder / FrameLabelledFolder end to end
from JPEG files under tmp_path -- np.array_equal / torch.equal against the per-clip executor and against the Pillow chain written
out in tests/test_frame_folder_host.py, no tolerance.  Then the prefetch against the same batches prepared one at a time, the
launch budget, and the three drivers on the new dataset names."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from test_frame_folder_host import (EPOCHS, PB, SEED, SIZE, T, VIDEOS, covered_plans, open_frames, pair_source, pil_clip, tf_tensor,
                                    write_tree)
from test_ftclip_host import noise_video

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(video):
    return torch.from_numpy(video).cuda().contiguous()


def _boxes(h, w, rot):
    """Boxes in the ROTATED frame: touching its left / top, top / right, left / bottom and right / bottom borders, the whole frame,
    one reaching past the right and bottom edges (zero fill) and a one-pixel column."""
    rw, rh = (h, w) if rot in (90, 270) else (w, h)
    return [(0, 0, rw - 9, rh - 7), (9, 0, rw, rh - 5), (0, 6, rw - 11, rh), (5, 7, rw, rh), (0, 0, rw, rh),
            (rw - 20, rh - 18, rw + 6, rh + 5), (3, 2, 4, rh - 1)]


def _edge_plans(h, w, t=T):
    """Pairs over every rotation code x every box of ``_boxes`` x both flips; the second clip of a pair takes another rotation."""
    from cstp_amd import sampler
    rots, pairs = (0, 90, 180, 270), []
    for k, rot in enumerate(rots):
        for j, box in enumerate(_boxes(h, w, rot)):
            frames = [(3 * j + i * (k + 1)) % 6 for i in range(t)]
            rot_2 = rots[(k + j) % 4]
            boxes_2 = _boxes(h, w, rot_2)
            a = sampler.ClipPlan(frames, rot, box, j % 2 == 0, False)
            b = sampler.ClipPlan(frames[::-1], rot_2, boxes_2[(j + 3) % len(boxes_2)], (j // 2) % 2 == 0, False)
            pairs.append(sampler.PairPlan(a, b, 0, 0, 0, (k, (k + j) % 4)))
    return pairs


@pytest.mark.parametrize("h,w,size", [(37, 53, 16), (48, 36, 32), (53, 37, 21)])
def test_rotated_pairs_equal_the_per_clip_executor_and_pillow(h, w, size):
    from cstp_amd import clip_ops
    video = noise_video(6, h, w, h)
    dev = _dev(video)
    pairs = _edge_plans(h, w)
    c1, c2 = clip_ops.assemble_pairs(dev, pairs, size)
    assert c1.shape == c2.shape == (len(pairs), 3, T, size, size) and c1.dtype == torch.float32
    single_1 = torch.stack([clip_ops.assemble_clip(dev, p.clip_1, size) for p in pairs])
    single_2 = torch.stack([clip_ops.assemble_clip(dev, p.clip_2, size) for p in pairs])
    assert torch.equal(c1, single_1) and torch.equal(c2, single_2)
    seen = set()
    got_1, got_2 = c1.cpu().numpy(), c2.cpu().numpy()
    for i, p in enumerate(pairs):                              # every pair against the Pillow chain: all rotations x both flips
        for got, cp in ((got_1[i], p.clip_1), (got_2[i], p.clip_2)):
            want = pil_clip([Image.fromarray(video[f], "RGB") for f in cp.frames], cp, size)
            assert np.array_equal(got, want), (i, cp)
            seen.add((cp.rotate, cp.flip))
    assert seen == {(r, f) for r in (0, 90, 180, 270) for f in (False, True)}
    # a given ``out`` is written in place, and a second call repeats the first
    out = torch.full((2, len(pairs), 3, T, size, size), 7.0, device="cuda")
    d1, d2 = clip_ops.assemble_pairs(dev, pairs, size, out=out)
    assert d1.data_ptr() == out.data_ptr() and d2.data_ptr() == out[1].data_ptr()
    assert torch.equal(out[0], c1) and torch.equal(out[1], c2)


def test_rotated_clips_with_an_eight_bit_output():
    """out8_slot under every rotation code: the 8-bit resize of a rotated clip, before any base operation, equals Pillow's."""
    from cstp_amd import clip_ops, sampler
    video = noise_video(5, 37, 53, 2)
    dev = _dev(video)
    plans, rots = [], (0, 90, 180, 270)
    for rot in rots:
        rw, rh = (37, 53) if rot in (90, 270) else (53, 37)
        plans.append(sampler.ClipPlan([0, 4, 2, 2], rot, (2, 0, rw, rh - 3), rot == 90, False))
    out, u8 = clip_ops._batch_forward(dev, plans, 24, None, [0, 1, 2, 3])
    assert u8.shape == (4, T, 24, 24, 3) and u8.dtype == torch.uint8
    got = u8.cpu().numpy()
    for k, cp in enumerate(plans):
        for j, f in enumerate(cp.frames):
            im = Image.fromarray(video[f], "RGB")
            if cp.rotate:
                im = im.transpose({90: Image.ROTATE_90, 180: Image.ROTATE_180, 270: Image.ROTATE_270}[cp.rotate])
            assert np.array_equal(got[k, j], np.asarray(im.crop(cp.box).resize((24, 24), Image.BICUBIC))), (cp.rotate, j)


def test_assemble_batch_keeps_refusing_rotated_and_base_plans():
    from cstp_amd import clip_ops, sampler
    video = _dev(noise_video(4, 32, 32, 1))
    with pytest.raises(ValueError, match="assemble_clip"):
        clip_ops.assemble_batch(video, [sampler.ClipPlan([0, 1], 180, (0, 0, 32, 32), False, False)], 16)
    with pytest.raises(ValueError, match="assemble_clip"):
        clip_ops.assemble_batch(video, [sampler.ClipPlan([0, 1], 0, (0, 0, 32, 32), False, True,
                                                         sampler.BasePlan(3.0, None, None, None))], 16)
    with pytest.raises(ValueError, match="rotation"):
        clip_ops.assemble_pairs(video, [sampler.PairPlan(sampler.ClipPlan([0, 1], 45, (0, 0, 32, 32), False, False),
                                                         sampler.ClipPlan([0, 1], 0, (0, 0, 32, 32), False, False), 0, 0, 0, (0, 0))], 16)


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_two_launches_for_a_batch_of_mixed_sizes_and_rotations():
    from cstp_amd import clip_ops, sampler
    shapes = [(20, 37, 53), (20, 48, 36), (20, 60, 44), (20, 41, 59)]
    videos = [_dev(noise_video(f, h, w, 20 + i)) for i, (f, h, w) in enumerate(shapes)]
    pairs, seed = [], 0
    while len(pairs) < 8:                                      # null_transform pairs only: no 8-bit branch in this batch
        f, h, w = shapes[len(pairs) % 4]
        p = sampler.sample_pair(f, w, h, T, random.Random(seed), np_rng=np.random.RandomState(seed))
        seed += 1
        if p.clip_1.base is None and p.clip_2.base is None:
            pairs.append(p)
    assert {c.rotate for p in pairs for c in (p.clip_1, p.clip_2)} == {0, 90, 180, 270}
    vids = [videos[i % 4] for i in range(8)]
    clip_ops.assemble_pairs(vids, pairs, SIZE)                 # warm-up: library load, coefficient tables
    names = _kernel_names(lambda: clip_ops.assemble_pairs(vids, pairs, SIZE))
    kernels = [n for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()]
    print(names)
    assert len(kernels) == 2 and "clip_batch_h" in kernels[0] and "clip_batch_v" in kernels[1]
    assert len(names) - len(kernels) <= 1                      # the one packed upload
    c1, c2 = clip_ops.assemble_pairs(vids, pairs, SIZE)
    for i, p in enumerate(pairs):
        assert torch.equal(c1[i], clip_ops.assemble_clip(vids[i], p.clip_1, SIZE))
        assert torch.equal(c2[i], clip_ops.assemble_clip(vids[i], p.clip_2, SIZE))


def test_base_transform_pairs_equal_the_per_clip_executor():
    from cstp_amd import clip_ops, sampler
    video = noise_video(30, 48, 36, 9)
    dev = _dev(video)
    pairs = [sampler.sample_pair(30, 36, 48, T, random.Random(s), p_base=0.7, np_rng=np.random.RandomState(s)) for s in range(10)]
    base = [c.base for p in pairs for c in (p.clip_1, p.clip_2) if c.base is not None]
    assert 6 <= len(base) < 20 and any(b.gray for b in base) and any(b.jitter for b in base) and any(b.blur_sigma for b in base)
    c1, c2 = clip_ops.assemble_pairs(dev, pairs, 32)
    for i, p in enumerate(pairs):
        (s1, s2), _ = clip_ops.assemble_pair(dev, p, 32)
        assert torch.equal(c1[i], s1) and torch.equal(c2[i], s2), (i, p)
    i = next(i for i, p in enumerate(pairs) if p.clip_1.base is not None)
    cp = pairs[i].clip_1
    assert np.array_equal(c1[i].cpu().numpy(), pil_clip([Image.fromarray(video[f], "RGB") for f in cp.frames], cp, 32))


# ---- end to end from files --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    ds = pair_source(tmp_path_factory.mktemp("pairs"))
    yield ds
    ds.close()


def test_pair_folder_batches_equal_the_pillow_chain(pairs):
    """Every video of the tree (among them the 3-frame one on the wrap-around branch and the grayscale JPEGs) over the epochs
    whose plans tests/test_frame_folder_host.py shows to cover every branch."""
    ds = pairs
    assert len(covered_plans(ds)) == 2 * len(VIDEOS) * len(EPOCHS)
    indices = list(range(len(ds)))
    for epoch in EPOCHS:
        c1, c2, spa, tem, pb, r1, r2 = ds.batch(indices, epoch)
        assert c1.shape == c2.shape == (len(indices), 3, T, SIZE, SIZE) and c1.is_cuda and spa.dtype == torch.int64
        got_1, got_2 = c1.cpu().numpy(), c2.cpu().numpy()
        for k, i in enumerate(indices):
            plan = ds.plan(i, epoch)
            folder = ds.data[i][0]
            assert np.array_equal(got_1[k], pil_clip(open_frames(folder, plan.clip_1.frames), plan.clip_1, SIZE)), (epoch, i)
            assert np.array_equal(got_2[k], pil_clip(open_frames(folder, plan.clip_2.frames), plan.clip_2, SIZE)), (epoch, i)
            assert (int(spa[k]), int(tem[k]), int(pb[k]), int(r1[k]), int(r2[k])) == \
                (plan.spa_label, plan.tem_label, plan.pb_label, plan.rot_labels[0], plan.rot_labels[1])
    assert Image.open(os.path.join(ds.data[2][0], "00001.jpg")).mode == "L"
    wrapped = ds.plan(1, 0)
    assert wrapped.clip_1.frames == wrapped.clip_2.frames and max(wrapped.clip_1.frames) < 3
    assert not torch.equal(ds.batch([0, 3], 0)[0], ds.batch([0, 3], 1)[0])      # another epoch, another augmentation


def test_prefetched_batches_equal_the_same_batches_prepared_one_at_a_time(tmp_path):
    """Four consecutive batches of different total sizes through the prefetch (the arenas grow and are reused, batch k + 1 is
    decoded while batch k is assembled) against a second source that prepares each batch when it is asked for."""
    from cstp_amd.frame_folder import FramePairFolder
    ds = pair_source(tmp_path)
    fresh = FramePairFolder("cuda:0", ds.frame_dir, ds.annotation_path, 1, "train", T, SIZE, seed=SEED, n_workers=2)
    batches = [[1, 4], [2], [0, 5, 3, 2, 1], [5, 0, 3]]
    totals = [sum(len(p) * h * w * 3 for p, h, w in ds._request((tuple(b), 2))[1]) for b in batches]
    # each arena serves every second batch; the later batch of each outgrows the 64 KiB that held the earlier one
    assert len(set(totals)) == 4 and totals[2] > (1 << 16) >= totals[0] and totals[3] > (1 << 16) >= totals[1]
    got, capacity = [], []
    for k, b in enumerate(batches):
        got.append(ds.batch(b, 2, prefetch=batches[k + 1] if k + 1 < len(batches) else None))
        if k + 1 < len(batches):
            assert ds._pending is not None and ds._pending[0] == (tuple(batches[k + 1]), 2)
        capacity.append([None if a is None else a.numel() for a in ds.stager().dev + ds.stager().pinned])
    assert capacity[0][1] is None and capacity[1][1] is not None                 # two arenas of each kind, used in turn
    assert capacity[2][0] > capacity[0][0] and capacity[3][1] > capacity[1][1] and capacity[2][2] > capacity[0][2]   # they grow
    assert all(b is None or a is None or b >= a for x, y in zip(capacity, capacity[1:]) for a, b in zip(x, y))
    torch.cuda.synchronize()
    for b, have in zip(batches, got):
        want = fresh.batch(b, 2)
        assert all(torch.equal(a, w) for a, w in zip(have, want)), b
    # a prefetch that names another batch than the one asked for next is dropped, not served
    ds.batch(batches[0], 2, prefetch=batches[1])
    other = ds.batch(batches[3], 2)
    assert all(torch.equal(a, w) for a, w in zip(other, got[3])) and ds._pending is None
    ds.close()
    fresh.close()


def test_loader_shards_like_the_synthetic_one(pairs):
    from cstp_amd.clip_ops import GpuClipLoader
    from cstp_amd.frame_folder import FramePairLoader
    a, b = FramePairLoader(pairs, 2, 0, 2, seed=3), GpuClipLoader(pairs, 2, 0, 2, seed=3)
    a.set_epoch(4)
    b.set_epoch(4)
    assert a.indices() == b.indices() and len(a) == len(b) == 1
    (clips, labels), = list(a)
    want = pairs.batch(a.indices()[:2], 4)
    assert torch.equal(clips[0], want[0]) and torch.equal(clips[1], want[1]) and torch.equal(labels[3][1], want[6])


def _pil_ft_clip(folder, plan, size):
    out = []
    for im in open_frames(folder, plan.frames):
        im = im.crop(plan.box)
        if plan.resized != im.size:
            im = im.resize(plan.resized, Image.BICUBIC)
        wx, wy = plan.window
        out.append(tf_tensor(im.crop((wx, wy, wx + size, wy + size))))
    return np.stack(out, axis=1)


def test_labelled_folder_modes_and_loaders(tmp_path):
    """'img' (unjittered plans against the Pillow chain, every plan against the executor on the decoded frames), 'img_val' and a
    whole 'img_test' video bit for bit; 'val' / 'test' loaders in order with the partial batch kept."""
    from cstp_amd import clip_ops
    from cstp_amd.frame_folder import FrameLabelledFolder, FrameLabelledLoader
    videos = [(e, lab, n, 140, 150 + 10 * k, g) for k, (e, lab, n, _, _, g) in enumerate(VIDEOS)]      # short side > 128
    frame_dir, ann = write_tree(tmp_path, videos)
    train = FrameLabelledFolder("cuda:0", frame_dir, ann, 1, "train", "img", T, 112, PB, seed=3, n_workers=4)
    clips, labels = train.batch([0, 1, 2, 3, 4, 5], 1)
    assert clips.shape == (6, 3, T, 112, 112) and labels.tolist() == [3, 3, 7, 7, 11, 11]
    plain = 0
    for k in range(6):
        plan = train.plan(k, 1)
        folder = train.data[k][0]
        frames = _dev(np.stack([np.asarray(im) for im in open_frames(folder, range(videos[k][2]))]))
        assert torch.equal(clips[k], clip_ops.assemble_batch(frames, [plan], 112)[0])
        if plan.jitter is None:
            plain += 1
            assert np.array_equal(clips[k].cpu().numpy(), _pil_ft_clip(folder, plan, 112)), k
    assert plain >= 2
    assert train.plan(1, 1).frames == [0, 2, 0, 2] and train.plan(4, 1).frames == [0, 2, 4, 0]       # the wrap-around branch
    assert len(list(FrameLabelledLoader(train, 4, seed=3))) == 1                                      # full batches only
    val = FrameLabelledFolder("cuda:0", frame_dir, ann, 1, "val", "img_val", T, 112, PB, seed=3, n_workers=4)
    seen = list(FrameLabelledLoader(val, 2))
    assert [c.shape[0] for c, _ in seen] == [2, 1] and [l.tolist() for _, l in seen] == [[3, 7], [11]]
    for k, c in enumerate([seen[0][0][0], seen[0][0][1], seen[1][0][0]]):
        assert np.array_equal(c.cpu().numpy(), _pil_ft_clip(val.data[k][0], val.plan(k, 0), 112)), k
    test = FrameLabelledFolder("cuda:0", frame_dir, ann, 1, "test", "img_test", T, 112, PB, n_workers=4)
    items = list(FrameLabelledLoader(test))
    assert [int(l) for _, l in items] == [3, 7, 11] and [c.shape[1] for c, _ in items] == [7, 3, 1]
    for k, (c, label) in enumerate(items):
        want = np.stack([_pil_ft_clip(test.data[k][0], p, 112) for p in test.plan(k)])
        assert c.shape == (1,) + want.shape and label.shape == (1,)
        assert np.array_equal(torch.squeeze(c, 0).cpu().numpy(), want), k
    with pytest.raises(ValueError):
        test.batch([0])
    with pytest.raises(ValueError):
        val.video(0)
    for ds in (train, val, test):
        ds.close()


def test_a_missing_frame_raises_with_its_path(tmp_path):
    from cstp_amd.frame_folder import FrameError
    ds = pair_source(tmp_path)
    plan = ds.plan(0, 0)
    gone = os.path.join(ds.data[0][0], "%05d.jpg" % (plan.clip_2.frames[-1] + 1))
    os.remove(gone)
    with pytest.raises(FrameError, match=os.path.basename(gone)):
        ds.batch([3, 0], 0)
    c1 = ds.batch([3], 0)[0]                                     # the source goes on serving
    assert c1.shape == (1, 3, T, SIZE, SIZE)
    ds.close()


# ---- drivers ------------------------------------------------------------------------------------------------------------------
def _run(args, timeout):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args[0], r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_pretrain_driver_on_a_frame_folder(tmp_path):
    frame_dir, ann = write_tree(tmp_path / "data")
    res = str(tmp_path / "res")
    out = _run(["main_byol.py", "--dataset", "UcfRepreBYOLSpPre", "--frame_dir", frame_dir, "--annotation_path", ann, "--split", "1",
                "--sample_duration", "4", "--sample_size", "32", "--model_name", "r21d_byol", "--model_depth", "1", "--n_workers",
                "4", "--batch_size", "2", "--result_path", res, "--task", "loss_com", "--loss_weight", "0.1", "1", "1", "1", "1",
                "--n_epochs", "1", "--max_steps", "2", "--learning_rate", "0.01"], 300)
    assert "Length of training data =  6" in out and "does not exist" in out
    log = os.path.join(res, "UcfRepreBYOLSpPre", "loss_com", "UcfRepreBYOLSpPre_train_clip4modelr21d_byol1.log")
    rows = open(log).read().strip().split("\n")
    assert len(rows) == 2 and all(np.isfinite(float(x)) for x in rows[1].split("\t") if x not in ("None", ""))
    assert out.count("Epoch: [1][") == 2


def test_finetune_and_test_drivers_on_a_frame_folder(tmp_path):
    videos = [(e, 1, n, 130, 150, g) for e, lab, n, _, _, g in VIDEOS]      # one class: the first validation is right, so
    # main_ft_mp.py writes the best-accuracy checkpoint that test.py picks up
    frame_dir, ann = write_tree(tmp_path / "data", videos)
    res = str(tmp_path / "res")
    common = ["--dataset", "UcfFineTune", "--frame_dir", frame_dir, "--annotation_path", ann, "--split", "1", "--sample_duration", "4",
              "--sample_size", "112", "--model_name", "r21d_byol", "--model_depth", "1", "--n_workers", "4", "--n_classes", "2",
              "--batch_size", "2", "--pb_rate", "2", "--result_path", res, "--weight_decay", "1e-4"]
    _run(["main_ft_mp.py"] + common + ["--transform_mode", "img", "--task", "scratch", "--learning_rate", "0.05", "--n_epochs", "3"],
         300)
    d = os.path.join(res, "UcfFineTune", "scratch")
    assert len([f for f in os.listdir(d) if f.endswith("_max.pth") or f.endswith(".log")]) >= 2
    out = _run(["test.py"] + common + ["--transform_mode", "img_test", "--task", "test", "--t_ft_task", "scratch"], 300)
    result = os.path.join(res, "UcfFineTune", "test_r21d_byol1_UcfFineTune_1_RGB_4_plusone.txt")
    text = open(result).read()
    assert text.count("Video[") == 3 and "Video accuracy" in text
    assert [int(ln.split("clips = ")[1]) for ln in out.split("\n") if "clips = " in ln] == [7, 3, 1]

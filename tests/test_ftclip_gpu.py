"""The batched GPU clip path of fine-tuning, validation and the video test (cstp_clip_batch_forward through
cstp_amd.clip_ops.assemble_batch / GpuLabelledVideos) on a real MI355X, bit for bit against the reference's data path restated
with PIL in tests/test_ftclip_host.py (frame selection + transform from one random.Random): np.array_equal / torch.equal
everywhere, no tolerance.  Then the launch budget, and the drivers end to end on --dataset synthetic_video."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_ftclip_host import noise_video, plan_clip_u8, reference_clip, reference_video, to_tensor

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, PB = 8, 4


def _dev(video):
    return torch.from_numpy(video).cuda().contiguous()


def _batch(video, mode, seeds, size=112, t=T):
    from cstp_amd import clip_ops, sampler
    f, h, w, _ = video.shape
    plans = [sampler.sample_ft_clip(f, w, h, t, size, PB, mode, random.Random(s)) for s in seeds]
    return plans, clip_ops.assemble_batch(_dev(video), plans, size).cpu().numpy()


def test_img_clips_equal_the_pil_chain_over_many_seeds():
    video = noise_video(100, 240, 320, 0)
    seeds = list(range(40))
    plans, got = _batch(video, "img", seeds)
    assert got.shape == (40, 3, T, 112, 112) and got.dtype == np.float32
    jittered = 0
    for i, s in enumerate(seeds):
        want = reference_clip(video, T, 112, PB, "img", random.Random(s))
        assert np.array_equal(got[i], want), "seed %d (jitter %s)" % (s, plans[i].jitter)
        jittered += plans[i].jitter is not None
    assert 3 <= jittered < 40                                   # both branches of ClipColorJitter(p = 0.3) were compared


def test_jittered_clips_equal_the_pil_ops_chain():
    """Every clip of this batch takes the colour jitter: resize kept 8-bit, the four operations in their shuffled order, one
    transform for the whole clip."""
    from cstp_amd import sampler
    video = noise_video(60, 240, 320, 4)
    seeds = [s for s in range(200)
             if sampler.sample_ft_clip(60, 320, 240, T, 112, PB, "img", random.Random(s)).jitter is not None][:6]
    assert len(seeds) == 6
    plans, got = _batch(video, "img", seeds)
    for i, s in enumerate(seeds):
        assert {op for op, _ in plans[i].jitter} == {"brightness", "contrast", "saturation", "hue"}
        assert np.array_equal(got[i], to_tensor(plan_clip_u8(video, plans[i], 112)))
        assert np.array_equal(got[i], reference_clip(video, T, 112, PB, "img", random.Random(s)))


def test_forced_fallback_equals_the_pil_chain():
    """320 x 32 frames: no crop attempt fits, ClipScale(112) upscales to 1120 x 112 and the centre 112 x 112 is kept -- the
    kernel computes only that window."""
    video = noise_video(40, 32, 320, 1)
    plans, got = _batch(video, "img", range(5))
    assert all(p.resized == (1120, 112) and p.window == (504, 0) for p in plans)
    for s in range(5):
        assert np.array_equal(got[s], reference_clip(video, T, 112, PB, "img", random.Random(s)))


@pytest.mark.parametrize("h,w,size", [(240, 320, 112), (128, 171, 112), (240, 320, 224), (320, 240, 112)])
def test_img_val_equals_the_pil_chain(h, w, size):
    """240 x 320 -> 128 x 170 -> window (29, 8); 128 x 171 unchanged -> window (30, 8); 224 from short side 240 -> 256; portrait."""
    video = noise_video(70, h, w, 2)
    plans, got = _batch(video, "img_val", range(4), size=size)
    for s in range(4):
        assert np.array_equal(got[s], reference_clip(video, T, size, PB, "img_val", random.Random(s)))
    if (h, w) == (128, 171):
        assert plans[0].resized == (171, 128) and plans[0].window == (30, 8)
        f0 = plans[0].frames[0]                                  # unchanged frames: the window is a plain copy
        assert np.array_equal(got[0][:, 0], to_tensor([video[f0][8:120, 30:142]])[:, 0])


@pytest.mark.parametrize("total", [300, 61, 40])
def test_whole_img_test_video(total):
    """Every clip of a test video in one call: [n, 3, T, S, S]; 300 frames at T = 16, pb = 4 give 4 windows + the last one, 61
    (= clip_range + 1) two identical ones, 40 the single wrap-around clip."""
    from cstp_amd import clip_ops, sampler
    video = noise_video(total, 240, 320, 3)
    plans = sampler.plan_test_video(total, 320, 240, 16, 112, PB)
    got = clip_ops.assemble_batch(_dev(video), plans, 112).cpu().numpy()
    want = reference_video(video, 16, 112, PB)
    assert got.shape == want.shape == ({300: 5, 61: 2, 40: 1}[total], 3, 16, 112, 112)
    assert np.array_equal(got, want)


def test_one_batch_mixes_videos_of_different_frame_sizes():
    from cstp_amd import clip_ops, sampler
    shapes = [(50, 240, 320), (40, 128, 171), (33, 32, 320), (90, 320, 240), (20, 112, 112)]
    videos = [noise_video(f, h, w, 10 + i) for i, (f, h, w) in enumerate(shapes)]
    dev = [_dev(v) for v in videos]
    picks, plans = [], []
    for k in range(15):
        v = k % len(videos)
        f, h, w, _ = videos[v].shape
        mode = "img" if k % 2 == 0 else "img_val"
        picks.append((v, mode, k))
        plans.append(sampler.sample_ft_clip(f, w, h, T, 112, PB, mode, random.Random(k)))
    got = clip_ops.assemble_batch([dev[v] for v, _, _ in picks], plans, 112).cpu().numpy()
    for i, (v, mode, k) in enumerate(picks):
        assert np.array_equal(got[i], reference_clip(videos[v], T, 112, PB, mode, random.Random(k))), (i, shapes[v], mode)


def test_batched_equals_the_per_clip_executor_and_is_repeatable():
    """The same 'img' crops through the per-clip assemble_clip (two launches, an upload and an allocation per clip) and through
    one assemble_batch call: torch.equal; two identical calls give identical batches; a given ``out`` is written in place."""
    from cstp_amd import clip_ops, sampler
    video = _dev(noise_video(100, 240, 320, 5))
    plans = [sampler.sample_ft_clip(100, 320, 240, 16, 112, PB, "img", random.Random(s)) for s in range(12)]
    for p in plans:
        p.jitter = None
    single = torch.stack([clip_ops.assemble_clip(video, sampler.ClipPlan(p.frames, 0, p.box, False, False), 112) for p in plans])
    a = clip_ops.assemble_batch(video, plans, 112)
    out = torch.full((12, 3, 16, 112, 112), 7.0, device="cuda")
    b = clip_ops.assemble_batch(video, plans, 112, out=out)
    assert b.data_ptr() == out.data_ptr()
    assert torch.equal(a, single) and torch.equal(a, b)
    # flips (not on the 'img' path, served for other callers) against the per-clip executor too
    for p in plans[::2]:
        p.flip = True
    single = torch.stack([clip_ops.assemble_clip(video, sampler.ClipPlan(p.frames, 0, p.box, p.flip, False), 112) for p in plans])
    assert torch.equal(clip_ops.assemble_batch(video, plans, 112), single)


def test_bad_plans_are_refused_before_any_launch():
    from cstp_amd import _lib, clip_ops, sampler
    video = _dev(noise_video(20, 64, 64, 6))
    good = sampler.FtClipPlan([0, 1], (0, 0, 64, 64), (64, 64), (0, 0))
    with pytest.raises(ValueError, match="leaves"):
        clip_ops.assemble_batch(video, [sampler.FtClipPlan([0, 1], (0, 0, 64, 64), (64, 64), (8, 0))], 60)
    with pytest.raises(ValueError, match="frames in one batch"):
        clip_ops.assemble_batch(video, [good, sampler.FtClipPlan([0], (0, 0, 64, 64), (64, 64), (0, 0))], 32)
    with pytest.raises(ValueError, match="assemble_clip"):
        clip_ops.assemble_batch(video, [sampler.ClipPlan([0, 1], 90, (0, 0, 64, 64), False, False)], 32)
    with pytest.raises(_lib.CstpError):
        clip_ops.assemble_batch(video.cpu(), [good], 32)


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_two_launches_per_unjittered_batch_and_per_test_video():
    from cstp_amd import clip_ops, sampler
    video = _dev(noise_video(300, 240, 320, 7))
    batch = [sampler.sample_ft_clip(300, 320, 240, 16, 112, PB, "img", random.Random(s)) for s in range(32)]
    for p in batch:
        p.jitter = None
    test_video = sampler.plan_test_video(300, 320, 240, 16, 112, PB)
    for plans in (batch, test_video):
        clip_ops.assemble_batch(video, plans, 112)              # warm-up: library load, coefficient tables
        names = _kernel_names(lambda: clip_ops.assemble_batch(video, plans, 112))
        kernels = [n for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()]
        print("%d clips:" % len(plans), names)
        assert len(kernels) == 2 and "clip_batch_h" in kernels[0] and "clip_batch_v" in kernels[1]
        assert len(names) - len(kernels) <= 1                   # the one packed upload


def test_labelled_videos_and_loaders():
    from cstp_amd.clip_ops import GpuLabelledLoader, GpuLabelledVideos
    from cstp_amd.device_batches import DeviceBatches
    train = GpuLabelledVideos("cuda:0", "train", "img", n_videos=5, n_classes=4, sample_duration=T, pb_rate=PB, length=12, seed=3)
    clip_range = (T - 1) * PB
    lens = [v.shape[0] for v in train.videos]
    assert all(v.shape[1:] == (240, 320, 3) and v.dtype == torch.uint8 for v in train.videos)
    assert min(lens) < clip_range + 1 and clip_range + 1 in lens and len(set(lens)) >= 4
    assert all(0 <= lab < 4 for lab in train.labels) and len(set(train.labels)) > 1
    loader = GpuLabelledLoader(train, 4, seed=3)
    first = list(loader)
    assert len(first) == 3
    for clips, labels in first:
        assert clips.shape == (4, 3, T, 112, 112) and clips.is_cuda and labels.shape == (4,) and labels.dtype == torch.int64
        assert float(clips.abs().max()) <= 1.0
    again = list(loader)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(first, again))
    # another epoch augments the same video differently
    idx = loader.indices()[:4]
    assert not torch.equal(train.batch(idx, 0)[0], train.batch(idx, 1)[0])
    # a batch equals the reference's data path, sample by sample, from the sample's own seed
    clips, labels = train.batch([0, 1, 7], 2)
    for j, i in enumerate([0, 1, 7]):
        v = i % 5
        rng = random.Random(((3 * 1000003 + 2) * 1000003 + i) * 101 + 11)
        assert np.array_equal(clips[j].cpu().numpy(), reference_clip(train.videos[v].cpu().numpy(), T, 112, PB, "img", rng))
        assert int(labels[j]) == train.labels[v]
    # validation: in order, partial batch kept; DeviceBatches hands device tensors through untouched
    val = GpuLabelledVideos("cuda:0", "val", "img_val", n_videos=5, n_classes=4, sample_duration=T, pb_rate=PB, length=6, seed=3)
    direct = list(GpuLabelledLoader(val, 4))
    assert [c.shape[0] for c, _ in direct] == [4, 2]
    seen = []
    loader = GpuLabelledLoader(val, 4)
    handed = []

    def spy():
        for c, l in loader:
            handed.append((c.data_ptr(), l.data_ptr()))
            yield c, l
    for c, l in DeviceBatches(spy(), 0):
        seen.append((c.data_ptr(), l.data_ptr()))
        assert torch.equal(c, direct[len(seen) - 1][0])
    assert seen == handed and len(seen) == 2
    # test: one video per item with DataLoader's batch dimension of one
    test = GpuLabelledVideos("cuda:0", "test", "img_test", n_videos=5, n_classes=4, sample_duration=T, pb_rate=PB, seed=3)
    items = list(GpuLabelledLoader(test))
    assert len(items) == 5
    for (clips, label), video in zip(items, test.videos):
        want = reference_video(video.cpu().numpy(), T, 112, PB)
        assert clips.shape == (1,) + want.shape and label.shape == (1,)
        assert np.array_equal(torch.squeeze(clips, 0).cpu().numpy(), want)
    with pytest.raises(ValueError):
        GpuLabelledVideos("cuda:0", "train", "numpy")
    with pytest.raises(ValueError):
        GpuLabelledVideos("cuda:0", "val", "img_val", sample_size=96)
    with pytest.raises(ValueError):
        GpuLabelledVideos("cuda:0", "test", "img")


def _run(args, timeout):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args[0], r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def _check_ft_and_test(res, out_ft, out_test, t, task="ft_all"):
    from cstp_amd import sampler
    d = os.path.join(res, "synthetic_video", task)
    for split in ("train", "val"):
        log = [f for f in os.listdir(d) if f.startswith("synthetic_video_%s_" % split)]
        assert len(log) == 1
        rows = open(os.path.join(d, log[0])).read().strip().split("\n")
        assert len(rows) >= 2 and all(np.isfinite(float(x)) for r in rows[1:] for x in r.split("\t"))
    assert len([f for f in os.listdir(d) if f.endswith("_max.pth")]) == 1
    lines = [ln for ln in out_test.split("\n") if ln.startswith("Video[") and "top1" in ln]
    counts = [int(ln.split("clips = ")[1]) for ln in out_test.split("\n") if ln.startswith("Video[") and "clips = " in ln]
    # the driver's test set: max(synthetic_len // 4, 1) = 4 items over GpuLabelledVideos' default lengths
    clip_range = (t - 1) * PB
    lens = [max(clip_range - 3, 2), clip_range + 1, 2 * clip_range + 7, clip_range + clip_range // 2]
    assert len(lines) == 4 and counts == [len(sampler.ft_test_frames(n, t, PB)) for n in lens]
    assert counts[0] == 1 and counts[1] == 2 and counts[2] == 3
    assert "Video accuracy" in out_test
    print(out_ft[-600:], out_test[-900:])                         # the accuracies are reported, not asserted


def test_driver_chain_pretrain_finetune_test_on_synthetic_video(tmp_path):
    """main_byol.py (100 one-step epochs: the driver checkpoints every 100) -> main_ft_mp.py --dataset synthetic_video
    --transform_mode img --task ft_all (validation on 'img_val') -> test.py --transform_mode img_test, depth-1 R(2+1)D at
    T = 8, 112 x 112, each a child process with a time limit: finite logs, one result line and the planned clip count per video."""
    res = str(tmp_path)
    common = ["--dataset", "synthetic_video", "--sample_duration", "8", "--sample_size", "112", "--model_name", "r21d_byol",
              "--model_depth", "1", "--n_workers", "0", "--result_path", res]
    _run(["main_byol.py"] + common + ["--batch_size", "4", "--synthetic_len", "4", "--task", "loss_com", "--loss_weight", "0.1", "1",
                                      "1", "1", "1", "--n_epochs", "100", "--max_steps", "1", "--learning_rate", "0.005",
                                      "--weight_decay", "5e-4"], 900)
    ckpt = os.path.join(res, "synthetic_video", "loss_com", "save_100.pth")
    ft = common + ["--n_classes", "4", "--batch_size", "8", "--synthetic_len", "16", "--weight_decay", "1e-4", "--pb_rate", "4"]
    out_ft = _run(["main_ft_mp.py"] + ft + ["--transform_mode", "img", "--task", "ft_all", "--pretrained_path", ckpt,
                                            "--learning_rate", "0.02", "--n_epochs", "3"], 600)
    out_test = _run(["test.py"] + ft + ["--transform_mode", "img_test", "--task", "test", "--t_ft_task", "ft_all"], 600)
    _check_ft_and_test(res, out_ft, out_test, 8)
    # the other data sets and modes are refused as before / with a reason
    r = subprocess.run([sys.executable, "main_ft_mp.py"] + ft + ["--transform_mode", "numpy", "--task", "scratch"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "cv2" in r.stderr


@pytest.mark.parametrize("model,depth,t,size", [("r3d_byol", "10", 8, 112), ("s3d_byol", "1", 8, 112), ("i3d_byol", "1", 16, 224)])
def test_other_backbones_run_through_both_drivers(tmp_path, model, depth, t, size):
    """The same two drivers on --dataset synthetic_video with the other three backbones (ft_all from a checkpoint that carries no
    weights, so every layer keeps its initialisation: the pre-training of each is covered by its own suite)."""
    res = str(tmp_path)
    ckpt = os.path.join(res, "empty.pth")
    torch.save({"epoch": 0, "arch": "%s-%s" % (model, depth), "state_dict": {}}, ckpt)
    ft = ["--dataset", "synthetic_video", "--sample_duration", str(t), "--sample_size", str(size), "--model_name", model,
          "--model_depth", depth, "--n_workers", "0", "--result_path", res, "--n_classes", "4", "--batch_size", "4",
          "--synthetic_len", "16", "--weight_decay", "1e-4", "--pb_rate", "4"]
    out_ft = _run(["main_ft_mp.py"] + ft + ["--transform_mode", "img", "--task", "ft_all", "--pretrained_path", ckpt,
                                            "--learning_rate", "0.01", "--n_epochs", "1", "--max_steps", "2"], 900)
    out_test = _run(["test.py"] + ft + ["--transform_mode", "img_test", "--task", "test", "--t_ft_task", "ft_all"], 900)
    _check_ft_and_test(res, out_ft, out_test, t)

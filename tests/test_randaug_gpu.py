"""RandAugment and random erasing on the HIP kernels (csrc/randaug.h through clip_ops.augment_batch / assemble_batch /
GpuLabelledVideos and main_ft_mp.py).  Every comparison is bit equality: the 8-bit clips after the last layer against the Pillow
calls themselves (tests/test_randaug_host.pil_apply), the fp32 clips against tests/randaug_spec.finish.  Shapes: (B, T, S) =
(16, 3, 33) -- 1089 pixels a frame, no multiple of 16, the one-pixel-per-thread path, several blocks per clip -- and (3, 2, 8) --
128 pixels a clip, the 48-byte path, one block -- with one case at the training size (4, 16, 112)."""
import dataclasses
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import randaug_spec as spec
from test_ftclip_host import plan_clip_u8
from test_randaug_host import all_op_values, constant_channel, over_255, pil_chain, textured, two_valued_channel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


class P:
    """The two fields augment_batch reads from a plan."""

    def __init__(self, randaug=None, erase=None):
        self.randaug, self.erase = randaug, erase


@functools.lru_cache(maxsize=None)
def _clips(b, t, s):
    """uint8 [b][t][s][s][3]: textured frames, with a constant-channel, a two-valued-channel and (where Equalize is not the
    identity anyway) a table-above-255 frame in every clip's rotation."""
    makers = [textured, constant_channel, two_valued_channel] + ([over_255] if s * s >= 510 else []) + [textured]
    out = np.stack([np.stack([makers[(i + k) % len(makers)](s, 10 * i + k) for k in range(t)]) for i in range(b)])
    out.setflags(write=False)
    return out


def _run(clips, plans, flips):
    """-> (8-bit clips after the last layer, fp32 batch) as numpy."""
    from cstp_amd import clip_ops
    u8 = torch.from_numpy(np.array(clips)).to(DEV)            # (a copy: the cached clips are read-only)
    out = torch.full((len(plans), 3) + clips.shape[1:4], 7.0, dtype=torch.float32, device=DEV)
    got, last = clip_ops.augment_batch(u8, plans, out, flips)
    assert got is out
    return last.cpu().numpy(), out.cpu().numpy()


def _check(clips, plans, flips):
    last, out = _run(clips, plans, flips)
    for i, p in enumerate(plans):
        want8 = pil_chain(clips[i], p.randaug)
        assert np.array_equal(last[i], want8), (i, p.randaug, int((last[i] != want8).sum()))
        assert np.array_equal(out[i], spec.finish(want8, flips[i], p.erase)), (i, p.randaug, p.erase)


# ---- every operation, two layers a run ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,t,s", [(16, 3, 33), (3, 2, 8)])
def test_every_operation_equals_pillow(b, t, s):
    cases = all_op_values(s)                      # magnitudes 0, 9, 30 and 13.7, both signs
    assert {n for n, _ in cases} == set(spec.OPS)
    groups = [[c for c in cases if c[0] == name] for name in spec.OPS]        # round robin: the first 14 cases are the 14 operations
    cases = [g[k] for k in range(max(len(g) for g in groups)) for g in groups if k < len(g)]
    clips = _clips(b, t, s)
    per_run = 2 * b
    for r in range(0, len(cases), per_run):
        chunk = cases[r:r + per_run]
        chunk = chunk + cases[:per_run - len(chunk)]
        if b == 16:
            assert r > 0 or {n for n, _ in chunk} == set(spec.OPS)          # two layers of 16 clips: every operation in ONE run
        plans = [P([chunk[i], chunk[b + i]]) for i in range(b)]
        _check(clips, plans, [i % 2 == 1 for i in range(b)])


def test_training_size():
    b, t, s = 4, 16, 112
    clips = _clips(b, t, s)
    plans = [P([("Equalize", 0.0), ("Rotate", -17.5)], (100, 0, 12, 111, 5)), P([("Contrast", 1.63), ("ShearX", 0.21)]),
             P([("Sharpness", 1.9), ("AutoContrast", 0.0)], (0, 40, 111, 9, 1 << 63)), P([("TranslateY", -23.0), ("Color", 0.37)])]
    _check(clips, plans, [False, True, True, False])


# ---- chains ----------------------------------------------------------------------------------------------------------------------------
def test_three_layers_equal_the_three_pillow_calls_in_order():
    from cstp_amd import randaug
    b, t, s = 16, 3, 33
    settings = randaug.Settings(3, 12.0, 4.0, 0.5)
    plans = [P(*randaug.draw(settings, s, randaug.clip_rng(100 + i))) for i in range(b)]
    plans[3].randaug = plans[3].randaug[:1]                               # clips with fewer operations are copied through
    plans[7].randaug = None
    assert any(p.erase for p in plans) and len({n for p in plans for n, _ in (p.randaug or ())}) >= 8
    _check(_clips(b, t, s), plans, [i % 3 == 0 for i in range(b)])


def test_same_call_twice_gives_equal_bits():
    from cstp_amd import randaug
    b, t, s = 16, 3, 33
    settings = randaug.Settings(2, 20.0, 5.0, 1.0)
    plans = [P(*randaug.draw(settings, s, randaug.clip_rng(7 + i))) for i in range(b)]
    plans[0].randaug, plans[1].randaug, plans[2].randaug = [("Equalize", 0.0)] * 2, [("AutoContrast", 0.0), ("Contrast", 0.4)], \
        [("Sharpness", 0.2), ("Equalize", 0.0)]
    flips = [False] * b
    a8, a = _run(_clips(b, t, s), plans, flips)
    b8, bb = _run(_clips(b, t, s), plans, flips)
    assert np.array_equal(a8, b8) and np.array_equal(a, bb)


# ---- erasing -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,t,s", [(16, 3, 33), (3, 2, 8)])
def test_erase_equals_the_spec(b, t, s):
    boxes = [(0, 0, 5, 3), (s - 4, 0, 4, 6), (0, s - 2, 7, 2), (s - 1, s - 1, 1, 1), (3, 2, 1, 1), (0, 0, s - 1, s - 1), (1, 1, s - 1, s - 1),
             (s // 2, 0, 2, s - 1)]
    clips = _clips(b, t, s)
    plans = [P(None, boxes[i % len(boxes)] + ((0x9E3779B97F4A7C15 * (i + 1)) & (2 ** 64 - 1),)) for i in range(b)]
    plans[-1].erase = None
    for flips in ([False] * b, [True] * b):
        last, out = _run(clips, plans, flips)
        assert np.array_equal(last, clips)                                # no layer: the 8-bit clips are untouched
        _, plain = _run(clips, [P() for _ in range(b)], flips)
        for i, p in enumerate(plans):
            assert np.array_equal(out[i], spec.finish(clips[i], flips[i], p.erase)), (i, p.erase, flips[i])
            inside = np.zeros(out[i].shape, dtype=bool)
            if p.erase is not None:
                x0, y0, w, h, _ = p.erase
                inside[:, :, y0:y0 + h, x0:x0 + w] = True
                assert out[i][inside].min() >= -1.0 and out[i][inside].max() < 1.0
            assert np.array_equal(out[i][~inside], plain[i][~inside])        # elements outside the box are untouched


def test_finish_without_layers_equals_clip_finish():
    from cstp_amd import clip_ops
    clips = _clips(3, 2, 8)
    _, out = _run(clips, [P(), P(), P()], [False, True, False])
    for i in range(3):
        ref = clip_ops.clip_finish(torch.from_numpy(np.array(clips[i])).to(DEV), i == 1)
        assert np.array_equal(out[i], ref.cpu().numpy())


def test_refusals():
    from cstp_amd import _lib, clip_ops
    u8 = torch.zeros((2, 2, 8, 8, 3), dtype=torch.uint8, device=DEV)
    out = torch.zeros((2, 3, 2, 8, 8), device=DEV)
    with pytest.raises(_lib.CstpError):
        clip_ops.augment_batch(u8.cpu(), [P(), P()], out, [False, False])
    with pytest.raises(ValueError):
        clip_ops.augment_batch(u8, [P()], out, [False, False])
    with pytest.raises(ValueError):
        clip_ops.augment_batch(u8, [P(), P()], out[:1], [False, False])
    with pytest.raises(ValueError):
        clip_ops.augment_batch(u8, [P(), P(None, (6, 0, 3, 1, 0))], out, [False, False])
    with pytest.raises(ValueError):
        clip_ops.augment_batch(u8, [P([("Blur", 1.0)]), P()], out, [False, False])


# ---- the whole path ----------------------------------------------------------------------------------------------------------------------
T, S, PB = 3, 33, 2


@functools.lru_cache(maxsize=None)
def _dataset(on):
    from cstp_amd.clip_ops import GpuLabelledVideos
    kw = dict(randaug=(2, 14.0, 3.0), random_erase=0.5) if on else {}
    return GpuLabelledVideos(DEV, "train", "img", n_videos=5, n_classes=4, height=48, width=64, sample_duration=T, sample_size=S,
                             pb_rate=PB, length=64, seed=3, **kw)


def _reference(ds, indices, epoch):
    want = []
    for i in indices:
        v, plan = ds.plan(i, epoch)
        u8 = np.stack(plan_clip_u8(ds.videos[v].cpu().numpy(), plan, S))          # crop -> resize -> window -> jitter
        want.append(spec.finish(pil_chain(u8, plan.randaug), plan.flip, plan.erase))
    return np.stack(want)


def test_whole_path_equals_crop_resize_pillow_chain_normalise_erase():
    ds = _dataset(True)
    indices = list(range(16))
    plans = [ds.plan(i, 2)[1] for i in indices]
    both = [p for p in plans if p.jitter and p.randaug and any(n != "Identity" for n, _ in p.randaug)]
    assert both and any(p.erase for p in plans) and any(p.erase is None for p in plans)      # jitter, then RandAugment, in one clip
    clips, labels = ds.batch(indices, 2)
    assert clips.shape == (16, 3, T, S, S) and labels.shape == (16,)
    assert np.array_equal(clips.cpu().numpy(), _reference(ds, indices, 2))
    again, _ = ds.batch(indices, 2)
    assert torch.equal(clips, again)


def test_flags_off_is_todays_batch():
    from cstp_amd import clip_ops
    on, off = _dataset(True), _dataset(False)
    assert off.augment is None
    indices = list(range(20, 36))
    picked = [off.plan(i, 1) for i in indices]
    assert all(p.randaug is None and p.erase is None for _, p in picked) and any(p.jitter for _, p in picked)
    assert [dataclasses.replace(on.plan(i, 1)[1], randaug=None, erase=None) for i in indices] == [p for _, p in picked]
    clips, _ = off.batch(indices, 1)
    today = clip_ops.assemble_batch([off.videos[v] for v, _ in picked], [p for _, p in picked], S)
    assert torch.equal(clips, today)
    assert np.array_equal(clips.cpu().numpy(), _reference(off, indices, 1))
    # and the 8-bit road with nothing to do on it arrives at the same bits as the direct one
    idle = [dataclasses.replace(p, randaug=[("Identity", 0.0)]) for _, p in picked]
    assert torch.equal(clip_ops.assemble_batch([off.videos[v] for v, _ in picked], idle, S), today)


def test_validation_and_test_clips_are_never_augmented():
    from cstp_amd.clip_ops import GpuLabelledVideos
    for data_type, mode in (("val", "img_val"), ("test", "img_test")):
        with pytest.raises(ValueError):
            GpuLabelledVideos(DEV, data_type, mode, n_videos=1, randaug=(2, 9.0, 0.0))
        with pytest.raises(ValueError):
            GpuLabelledVideos(DEV, data_type, mode, n_videos=1, random_erase=0.5)


# ---- the driver, in a fresh process --------------------------------------------------------------------------------------------------------
def test_finetune_driver_with_the_flags(tmp_path):
    res = str(tmp_path)
    args = ["main_ft_mp.py", "--dataset", "synthetic_video", "--transform_mode", "img", "--randaug_n", "2", "--random_erase", "0.25",
            "--task", "scratch", "--model_name", "r21d_byol", "--model_depth", "1", "--n_classes", "4", "--batch_size", "4",
            "--synthetic_len", "16", "--sample_duration", "8", "--sample_size", "112", "--pb_rate", "4", "--n_workers", "0",
            "--learning_rate", "0.01", "--n_epochs", "1", "--max_steps", "4", "--result_path", res]
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "randaug_n=2" in r.stdout and "random_erase=0.25" in r.stdout
    d = os.path.join(res, "synthetic_video", "scratch")
    rows = open(os.path.join(d, "synthetic_video_train_clip8modelr21d_byol1.log")).read().strip().split("\n")
    assert len(rows) == 2 and np.isfinite(float(rows[1].split("\t")[1])), rows
    assert len([f for f in os.listdir(d) if f.endswith("_max.pth")]) == 1
    bad = subprocess.run([sys.executable, "main_ft_mp.py", "--dataset", "synthetic", "--transform_mode", "img", "--randaug_n", "2",
                          "--task", "scratch", "--model_name", "r21d_byol", "--model_depth", "1", "--result_path", res],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "--randaug_n" in bad.stderr, bad.stderr[-2000:]

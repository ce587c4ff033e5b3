#!/usr/bin/env python3
"""The batched fine-tune clip path (cstp_clip_batch_forward) against the per-clip executor (cstp_clip_assemble, one clip at a
time + torch.stack) on the SAME plans, alternating in one process: a batch of 32 'img' clips (16 x 112 x 112) from 240x320
frames, and one 300-frame 'img_test' video.  Wall time per batch (host clock around work that ends in a synchronise) and device
time (events), median and range over the repeats; the outputs of the two paths are compared before anything is timed.
--step adds the R(2+1)D-18 ft_all step the clips feed (B = 32), for the share.  One JSON line per case."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cstp_amd import clip_ops, sampler  # noqa: E402


def timed(fn, inner):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev0.record()
    for _ in range(inner):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner, ev0.elapsed_time(ev1) / inner


def summary(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def ft_step_ms(batch, steps):
    from cstp_amd.optim import FlatSGD
    from cstp_amd.r21d_byol import R21DBYOL, layer_sizes_for_depth
    from cstp_amd.train import FineTuneStep
    model = R21DBYOL(pretrain=False, num_classes=101, cls_bn=True, layer_sizes=layer_sizes_for_depth(18)).cuda()
    arenas = model.flatten_parameters()
    model.train()
    opt = FlatSGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=5e-4, arenas=arenas)
    step = FineTuneStep(model, opt, "ft_all")
    x = torch.rand((batch, 3, 16, 112, 112), device="cuda") * 2 - 1
    y = torch.randint(0, 101, (batch,), device="cuda")
    for _ in range(4):
        step(x, y)
    return summary([timed(lambda: step(x, y), steps)[0] for _ in range(3)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--step", action="store_true", help="also time the R(2+1)D-18 ft_all step at B = 32")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ftclip.py needs a HIP device")
    ds = clip_ops.GpuLabelledVideos("cuda:0", "train", "img", n_videos=4, lengths=[300, 200, 120, 61], seed=1)
    picked = [ds.plan(i, 0) for i in range(32)]
    for _, p in picked:
        p.jitter = None                      # the per-clip executor has no jitter branch of its own: same work on both sides
    videos, plans = [ds.videos[v] for v, _ in picked], [p for _, p in picked]
    old_plans = [sampler.ClipPlan(p.frames, 0, p.box, False, False) for p in plans]

    def batched():
        return clip_ops.assemble_batch(videos, plans, 112)

    def per_clip():
        return torch.stack([clip_ops.assemble_clip(v, p, 112) for v, p in zip(videos, old_plans)])

    assert torch.equal(batched(), per_clip())
    tplans = sampler.plan_test_video(300, 320, 240, 16, 112, 4)

    def test_video():
        return clip_ops.assemble_batch(ds.videos[0], tplans, 112)

    for fn in (batched, per_clip, test_video):
        for _ in range(3):
            fn()
    res = {k: ([], []) for k in ("batched", "per_clip", "test_video")}
    for _ in range(args.repeats):            # alternating: every repeat times all three back to back
        for name, fn in (("batched", batched), ("per_clip", per_clip), ("test_video", test_video)):
            wall, dev = timed(fn, args.inner)
            res[name][0].append(wall)
            res[name][1].append(dev)
    out = {"case": "32 img clips 16x112x112 from 240x320", "repeats": args.repeats, "inner": args.inner}
    for name in ("batched", "per_clip"):
        out[name + "_wall_ms"], out[name + "_gpu_ms"] = summary(res[name][0]), summary(res[name][1])
    out["speedup_wall_median"] = round(out["per_clip_wall_ms"]["median"] / out["batched_wall_ms"]["median"], 2)
    print(json.dumps(out))
    print(json.dumps({"case": "one 300-frame img_test video (%d clips, 240x320 -> 128x170 -> 112x112 window)" % len(tplans),
                      "wall_ms": summary(res["test_video"][0]), "gpu_ms": summary(res["test_video"][1])}))
    if args.step:
        st = ft_step_ms(32, 5)
        print(json.dumps({"case": "R(2+1)D-18 ft_all step, B = 32, fp32", "wall_ms": st,
                          "batched_share": round(out["batched_wall_ms"]["median"] / st["median"], 4),
                          "per_clip_share": round(out["per_clip_wall_ms"]["median"] / st["median"], 4)}))


if __name__ == "__main__":
    main()

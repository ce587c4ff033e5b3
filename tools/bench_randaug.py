#!/usr/bin/env python3
"""RandAugment + random erasing on the fine-tune clip path (csrc/randaug.h), timed three ways on the SAME plans, alternating in one
process (as tools/bench_ftclip.py does): batch assembly with the flags off; with the flags on through the batched path
(clip_ops.assemble_batch -> augment_batch: one operation table per layer for the whole batch); and the same plans applied one clip
at a time -- the new entry points called with a batch of one, the per-clip composition the batched path replaces.  'img' clips of
16 x 112 x 112 from 240x320 frames at B = 16 and B = 64, --randaug_n 2 --randaug_m 9 --random_erase 0.25.  Wall time per batch (host
clock around work that ends in a synchronise) and device time (events), median and range over the repeats; the two augmented paths
are compared bit for bit before anything is timed.  --step adds the R(2+1)D-18 ft_all step fed by the assembly, with and without
the flags.  One JSON line per case."""
import argparse
import dataclasses
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cstp_amd import clip_ops  # noqa: E402
from tools.bench_ftclip import summary, timed  # noqa: E402

T, S = 16, 112


def build(batch):
    """-> (assembly with the flags off, batched with the flags on, one clip at a time with the flags on, what the plans hold)."""
    ds = clip_ops.GpuLabelledVideos("cuda:0", "train", "img", n_videos=4, lengths=[300, 200, 120, 61], seed=1, sample_duration=T,
                                    sample_size=S, randaug=(2, 9.0, 0.0), random_erase=0.25)
    picked = [ds.plan(i, 0) for i in range(batch)]
    videos, plans = [ds.videos[v] for v, _ in picked], [p for _, p in picked]
    plain = [dataclasses.replace(p, randaug=None, erase=None) for p in plans]
    jittered = [i for i, p in enumerate(plans) if p.jitter]

    def off():
        return clip_ops.assemble_batch(videos, plain, S)

    def batched():
        return clip_ops.assemble_batch(videos, plans, S)

    def per_clip():
        out, u8 = clip_ops._batch_forward(videos, plans, S, None, list(range(batch)))
        for i in jittered:
            clip = u8[i]
            for op, factor in plans[i].jitter:
                clip = clip_ops.clip_colour(clip, op, factor)
            u8[i].copy_(clip)
        for i, p in enumerate(plans):
            clip_ops.augment_batch(u8[i:i + 1], [p], out[i:i + 1], [p.flip])
        return out

    ops = [n for p in plans for n, _ in p.randaug]
    info = {"clips": batch, "jittered": len(jittered), "erased": sum(p.erase is not None for p in plans),
            "operations": {n: ops.count(n) for n in sorted(set(ops))}}
    return off, batched, per_clip, info


def ft_step(batch):
    from cstp_amd.optim import FlatSGD
    from cstp_amd.r21d_byol import R21DBYOL, layer_sizes_for_depth
    from cstp_amd.train import FineTuneStep
    model = R21DBYOL(pretrain=False, num_classes=101, cls_bn=True, layer_sizes=layer_sizes_for_depth(18)).cuda()
    arenas = model.flatten_parameters()
    model.train()
    opt = FlatSGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=5e-4, arenas=arenas)
    step = FineTuneStep(model, opt, "ft_all")
    y = torch.randint(0, 101, (batch,), device="cuda")
    return lambda x: step(x, y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--step", action="store_true", help="also time assembly + the R(2+1)D-18 ft_all step, flags off and on")
    ap.add_argument("--step_batch", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_randaug.py needs a HIP device")
    for batch in args.batches:
        off, batched, per_clip, info = build(batch)
        assert torch.equal(batched(), per_clip())
        names = (("off", off), ("batched", batched), ("per_clip", per_clip))
        for _, fn in names:
            for _ in range(3):
                fn()
        res = {k: ([], []) for k, _ in names}
        for _ in range(args.repeats):            # alternating: every repeat times all three back to back
            for name, fn in names:
                wall, dev = timed(fn, args.inner)
                res[name][0].append(wall)
                res[name][1].append(dev)
        out = {"case": "%d img clips %dx%dx%d from 240x320, randaug n=2 m=9, erase 0.25" % (batch, T, S, S), "repeats": args.repeats,
               "inner": args.inner}
        out.update(info)
        for name, _ in names:
            out[name + "_wall_ms"], out[name + "_gpu_ms"] = summary(res[name][0]), summary(res[name][1])
        out["per_clip_over_batched_wall"] = round(out["per_clip_wall_ms"]["median"] / out["batched_wall_ms"]["median"], 2)
        out["batched_minus_off_wall_ms"] = round(out["batched_wall_ms"]["median"] - out["off_wall_ms"]["median"], 3)
        print(json.dumps(out), flush=True)
    if args.step:
        off, batched, _, _ = build(args.step_batch)
        step = ft_step(args.step_batch)
        names = (("off", lambda: step(off())), ("batched", lambda: step(batched())))
        for _, fn in names:
            for _ in range(4):
                fn()
        res = {k: [] for k, _ in names}
        for _ in range(3):
            for name, fn in names:
                res[name].append(timed(fn, args.inner)[0])
        print(json.dumps({"case": "assembly + R(2+1)D-18 ft_all step, B = %d, fp32" % args.step_batch,
                          "flags_off_wall_ms": summary(res["off"]), "flags_on_wall_ms": summary(res["batched"])}), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the fine-tuning recipe's optimiser side costs, on the R(2+1)D-18 ``ft_all`` arena, in one process on one box, alternating
repeats.  One JSON line per case.

Optimizer step alone, for SGD and for AdamW (``"optimizer"`` in the line):
  a  flat          FlatSGD / FlatAdam on model.parameters(): one run, the flags off -- the floor
  b  flat_groups   the same class on one group per tensor with --layer_decay / --wd_skip_1d hyper-parameters, through the runs of
                   _plan(): what layer decay costs without the table kernel
  c  table         TableSGD / TableAdam on those groups: one launch
  d  table_ema     the same with the EMA shadow updated in that launch
  e  table_ema_sep the same step without the shadow, then one ops.ema_update_ pass over the arena
``launches`` is counted from a profiled step, ``bytes`` is what the passes have to move, computed from the arena layout.
Then the whole ``ft_all`` step (FineTuneStep, B = --batch) with the flags off (FlatSGD) and on (TableSGD with layer decay, the 1-D
weight-decay skip and the EMA): ``"case": "step_off"`` / ``"step_on"``.
Times are host clocks around --inner steps that end in a device synchronise, after --warmup steps of each side; the median of
--repeats alternating windows is reported with its minimum and maximum, per step."""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("CSTP_TUNE_TABLE_RO", "1")          # read the committed tile table, never write this run's into it

import torch  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cstp_amd import ops, recipe  # noqa: E402
from cstp_amd.optim import FlatAdam, FlatSGD, TableAdam, TableSGD  # noqa: E402
from cstp_amd.r21d_byol import R21DBYOL, layer_sizes_for_depth  # noqa: E402
from cstp_amd.train import FineTuneStep  # noqa: E402

MOMENTUM, WD, LAYER_DECAY, EMA = 0.9, 5e-4, 0.75, 0.999
LRS = {"sgd": 0.01, "adamw": 1e-6}       # AdamW moves every weight by about lr per step whatever the gradient: kept tiny over the repeats


def window(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    # (torch wraps Optimizer.step in a profiler range of its own, reported on the device side too: not a launch)
    return sum(e.device_type == torch.autograd.DeviceType.CUDA and not e.name.startswith("Optimizer.step#") for e in prof.events())


def alternate(sides, args, inner):
    for fn in sides.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in sides}
    for _ in range(args.repeats):
        for k, fn in sides.items():
            times[k].append(window(fn, inner))
    return times


def optimizer_cases(kind, model, arenas, args):
    lr = LRS[kind]
    groups = lambda: recipe.param_groups(model, model.parameters(), LAYER_DECAY, WD, True)
    if kind == "sgd":
        make = lambda cls, plist: cls(plist, lr=lr, momentum=MOMENTUM, weight_decay=WD, arenas=arenas)
        flat, table = FlatSGD, TableSGD
    else:
        make = lambda cls, plist: cls(plist, lr=lr, betas=(0.9, 0.99), weight_decay=WD, decoupled=True, arenas=arenas)
        flat, table = FlatAdam, TableAdam
    opts = {"flat": make(flat, model.parameters()), "flat_groups": make(flat, groups()), "table": make(table, groups()),
            "table_ema": make(table, groups()), "table_ema_sep": make(table, groups())}
    opts["table_ema"].enable_ema(EMA)
    shadow = arenas["param"].clone()

    def separate():
        opts["table_ema_sep"].step()
        ops.ema_update_(shadow, arenas["param"], EMA)
    sides = {k: o.step for k, o in opts.items()}
    sides["table_ema_sep"] = separate
    times = alternate(sides, args, args.inner)
    if not bool(torch.isfinite(arenas["param"]).all()):
        raise RuntimeError("the parameters left the finite range during the timed steps")
    n = arenas["param"].numel()
    streams = {"sgd": 6, "adamw": 7}[kind]                 # SGD reads and writes p, g, buf; AdamW reads g and reads and writes p, m, v
    nbytes = {"flat": streams, "flat_groups": streams, "table": streams, "table_ema": streams + 2, "table_ema_sep": streams + 3}
    med = {k: statistics.median(v) for k, v in times.items()}
    for k in sides:
        row = {"optimizer": kind, "case": k, "arena": "r21d_byol depth %d ft_all" % args.depth, "arena_floats": n,
               "tensors": len(list(model.parameters())), "runs": len(opts[k]._plan()), "launches": launches(sides[k]),
               "bytes": nbytes[k] * 4 * n, "gb_per_s": round(nbytes[k] * 4 * n / med[k] / 1e6, 1),
               "over_flat": round(med[k] / med["flat"], 3), "repeats": args.repeats, "inner_steps": args.inner,
               "warmup_steps": args.warmup}
        row.update(stats(times[k]))
        print(json.dumps(row), flush=True)


def step_cases(model, arenas, args):
    gen = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(args.batch, 3, args.frames, args.size, args.size, device="cuda", generator=gen)
    y = torch.arange(args.batch, device="cuda") % 101
    off = FlatSGD(model.parameters(), lr=1e-4, momentum=MOMENTUM, weight_decay=WD, arenas=arenas)
    on = TableSGD(recipe.param_groups(model, model.parameters(), LAYER_DECAY, WD, True), lr=1e-4, momentum=MOMENTUM, weight_decay=WD,
                  arenas=arenas)
    on.enable_ema(EMA)
    steps = {"step_off": FineTuneStep(model, off, "ft_all"), "step_on": FineTuneStep(model, on, "ft_all")}
    sides = {k: (lambda s=s: s(x, y)) for k, s in steps.items()}
    times = alternate(sides, args, args.step_inner)
    med = {k: statistics.median(v) for k, v in times.items()}
    for k in sides:
        row = {"case": k, "arena": "r21d_byol depth %d ft_all" % args.depth, "batch": args.batch,
               "clip": [3, args.frames, args.size, args.size], "optimizer": type(steps[k].optimizer).__name__,
               "over_off": round(med[k] / med["step_off"], 4), "repeats": args.repeats, "inner_steps": args.step_inner,
               "warmup_steps": args.warmup}
        row.update(stats(times[k]))
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--depth", type=int, default=18, choices=(1, 18, 34))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--step_inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=112)
    ap.add_argument("--skip_step", action="store_true", help="time the optimizer cases only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_recipe.py needs a HIP device: there is nothing to time without one")
    torch.manual_seed(1)
    model = R21DBYOL(pretrain=False, num_classes=101, cls_bn=True, layer_sizes=layer_sizes_for_depth(args.depth)).cuda().train()
    arenas = model.flatten_parameters()
    gen = torch.Generator(device="cuda").manual_seed(2)
    for p in model.parameters():                          # per tensor: the padding between tensors stays zero
        p.grad.copy_(torch.randn(p.shape, device="cuda", generator=gen) * 1e-4)
    for kind in ("sgd", "adamw"):
        optimizer_cases(kind, model, arenas, args)
    if not args.skip_step:
        step_cases(model, arenas, args)


if __name__ == "__main__":
    main()

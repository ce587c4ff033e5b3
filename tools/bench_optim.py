#!/usr/bin/env python3
"""One optimizer step over the R(2+1)D-18 pre-training arena, three ways, in one process on one box, alternating repeats.
One JSON line:
  * flat_sgd   FlatSGD.step: one pass over the same bytes (reads p, g, buf; writes p, g, buf) -- the floor;
  * flat_lars  FlatLARS.step: the norm pass (reads p and g of the adapted tensors), the per-tensor fold, the update pass;
  * aten_lars  the same LARS spec as a per-tensor loop of ATen calls on the same device tensors, no host read.
Every side steps with a clip coefficient pending, as main_byol.py does (clip_grad_norm_(., 18) before every step); the gradient is
seeded noise small enough for the coefficient to be exactly 1, so the written-back gradient does not decay over the repeats.
Times are host clocks around --inner steps that end in a device synchronise, after --warmup steps of each side; the median of
--repeats alternating windows is reported with its minimum and maximum, per step.  The byte counts are what each pass has to move,
computed from the arena layout, not a measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cstp_amd import ops  # noqa: E402
from cstp_amd.optim import FlatLARS, FlatSGD  # noqa: E402
from cstp_amd.r21d_byol import R21DBYOL  # noqa: E402

LR, MOMENTUM, WD, ETA, CLIP = 0.05, 0.9, 5e-4, 1e-3, 18.0


@torch.no_grad()
def aten_lars_step(params, bufs, coef):
    """The spec of FlatLARS composed from ATen, tensor by tensor (include/cstp_hip.h, cstp_lars_ratio)."""
    one = coef.new_ones(())
    for p, buf in zip(params, bufs):
        g = p.grad
        g.mul_(coef)
        if p.dim() > 1:
            d = g.add(p, alpha=WD)
            wn, dn = torch.linalg.vector_norm(p), torch.linalg.vector_norm(d)
            d.mul_(torch.where((wn > 0) & (dn > 0), ETA * wn / dn, one))
        else:
            d = g
        buf.mul_(MOMENTUM).add_(d)
        p.add_(buf, alpha=-LR)


def window(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--depth", type=int, default=18, choices=(1, 18, 34))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_optim.py needs a HIP device: there is nothing to time without one")
    torch.manual_seed(1)
    model = R21DBYOL(pretrain=True, layer_sizes={1: (1, 1, 1, 1), 18: (2, 2, 2, 2), 34: (3, 4, 6, 3)}[args.depth]).cuda()
    arenas = model.flatten_parameters()
    params = [p for p in model.trainable_parameters() if p.requires_grad]
    gen = torch.Generator(device="cuda").manual_seed(2)
    for p in params:                                      # per tensor: the padding between tensors stays zero
        p.grad.copy_(torch.randn(p.shape, device="cuda", generator=gen) * 1e-4)
    sgd = FlatSGD(model.parameters(), lr=LR, momentum=MOMENTUM, weight_decay=WD, arenas=arenas)
    lars = FlatLARS(model.parameters(), lr=LR, momentum=MOMENTUM, weight_decay=WD, eta=ETA, arenas=arenas)
    aten_buf = torch.zeros_like(arenas["param"])
    base = arenas["param"].data_ptr()
    bufs = [aten_buf[(p.data_ptr() - base) // 4:(p.data_ptr() - base) // 4 + p.numel()].view_as(p) for p in params]
    lars.clip_grad_norm_(CLIP)
    coef = lars._coef.clone()
    if float(coef) != 1.0:
        raise RuntimeError("the seeded gradient was meant to stay under the clip norm (coefficient %r)" % float(coef))

    def with_clip(opt):
        def fn():
            opt._coef.copy_(coef)
            opt._clip_pending = True
            opt.step()
        return fn
    sides = {"flat_sgd": with_clip(sgd), "flat_lars": with_clip(lars), "aten_lars": lambda: aten_lars_step(params, bufs, coef)}
    for fn in sides.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in sides}
    for _ in range(args.repeats):
        for k, fn in sides.items():
            times[k].append(window(fn, args.inner))
    if not bool(torch.isfinite(arenas["param"]).all()):
        raise RuntimeError("the parameters left the finite range during the timed steps")

    n = arenas["param"].numel()
    adapted = sum((p.numel() + 3) // 4 * 4 for p in params if p.dim() > 1)
    tables = lars._run_tables()
    med = {k: statistics.median(v) for k, v in times.items()}
    row = {"arena": "r21d_byol depth %d pre-training" % args.depth, "arena_floats": n, "tensors": len(params),
           "adapted_tensors": sum(p.dim() > 1 for p in params), "adapted_floats": adapted, "lars_chunk": ops.LARS_CHUNK,
           "lars_chunks": sum(int(t[1].shape[0]) for t in tables), "lars_runs": len(tables),
           "repeats": args.repeats, "inner_steps": args.inner, "warmup_steps": args.warmup,
           "flat_sgd": dict(stats(times["flat_sgd"]), launches=len(sgd._plan()), bytes=6 * 4 * n),
           "flat_lars": dict(stats(times["flat_lars"]), launches=3 * len(tables), norm_pass_bytes=2 * 4 * adapted,
                             update_pass_bytes=6 * 4 * n, bytes=2 * 4 * adapted + 6 * 4 * n),
           "aten_lars": stats(times["aten_lars"]),
           "lars_over_sgd": round(med["flat_lars"] / med["flat_sgd"], 3),
           "aten_over_lars": round(med["aten_lars"] / med["flat_lars"], 3),
           "flat_lars_gb_per_s": round((2 * 4 * adapted + 6 * 4 * n) / med["flat_lars"] / 1e6, 1),
           "flat_sgd_gb_per_s": round(6 * 4 * n / med["flat_sgd"] / 1e6, 1)}
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Pre-training throughput of the S3D-G-BYOL wrapper (cstp_amd/s3dg_byol.py) on one MI355X, synthetic clips resident in HBM.

    python tools/bench_s3dg.py --batch 16 --frames 16 --size 112 --steps 10
    CSTP_S3D_GATE=0 python tools/bench_s3dg.py ...      # self-gating + concat composed from ops.linear + ATen (A/B)

Prints one JSON line: ms/step, clips/s, kernel launches per step (torch.profiler device events of one step, both streams), the
launches of the gating + concat themselves, and a per-kernel-class table (every spanned C-ABI call of two extra steps under a
HIP-event pair on its launch stream, stream overlaps off; classes as tools/bench_r3d.py plus the fused gate op).  Not the
headline metric (bench.py is)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cstp_amd import ops, r21d_byol as _rb, s3dg_byol  # noqa: E402
from cstp_amd.optim import FlatSGD  # noqa: E402
from cstp_amd.s3dg_byol import S3DGBYOL  # noqa: E402
from cstp_amd.synthetic import device_batch  # noqa: E402
from cstp_amd.train import PretrainStep  # noqa: E402
from tools.bench_r3d import AllTimers, classify  # noqa: E402


def kernel_class(what, key):
    if what.startswith("gate_"):
        return "gate+concat " + ("fwd" if what == "gate_forward" else "bwd")
    return classify(what, key)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=112)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    torch.manual_seed(1)
    dev = torch.device("cuda", 0)
    model = S3DGBYOL(pretrain=True, gating=True, slow=False, num_classes=400).cuda()
    arenas = model.flatten_parameters()
    model.train()
    opt = FlatSGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=5e-4, arenas=arenas)
    step = PretrainStep(model, opt, (0.1, 1.0, 1.0, 1.0, 1.0), clip_grad_norm=True)
    x1, x2, lab = device_batch(a.batch, a.frames, a.size, dev, seed=1)

    def run(n):
        for _ in range(n):
            step(x1, x2, lab["spa"], lab["tem"], lab["pb"], lab["rot1"], lab["rot2"]).to_host()

    run(1 + a.warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(a.steps)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / a.steps * 1e3

    # ---- launches of one step (device kernel events)
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        run(1)
        torch.cuda.synchronize()
    kern = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    gate_kern = [k for k in kern if "gate_" in k]

    # ---- per-class table: two more steps, stream overlaps off, every spanned call under a HIP-event pair
    tm = AllTimers()
    ops.kernel_timer = tm
    saved = (ops.OVERLAP_WGRAD, _rb.OVERLAP_TARGET_FORWARD)
    ops.OVERLAP_WGRAD = False
    _rb.OVERLAP_TARGET_FORWARD = False
    tm.enabled = True
    nrep = 2
    run(nrep)
    torch.cuda.synchronize()
    tm.enabled = False
    ops.kernel_timer = None
    ops.OVERLAP_WGRAD, _rb.OVERLAP_TARGET_FORWARD = saved
    classes = {}
    for (what, key), pairs in tm.pairs.items():
        c = classes.setdefault(kernel_class(what, key), {"calls": 0, "ms": 0.0})
        c["calls"] += len(pairs)
        c["ms"] += sum(x.elapsed_time(y) for x, y in pairs)
    rows = [{"class": name, "calls_per_step": c["calls"] / nrep, "ms_per_step": round(c["ms"] / nrep, 3)}
            for name, c in sorted(classes.items(), key=lambda kv: -kv[1]["ms"])]
    print(json.dumps({"config": {"workload": "s3d_byol S3D-G, B=%d clip pairs 3x%dx%dx%d, full loss_com, clip 18, SGD; fp32"
                                             % (a.batch, a.frames, a.size, a.size),
                                 "gate": "fused" if s3dg_byol.FUSED_GATE else "composed (CSTP_S3D_GATE=0)"},
                      "ms_per_step": round(ms, 2), "clips_per_s": round(a.batch / ms * 1e3, 2),
                      "launches_per_step": len(kern), "gate_launches_per_step": len(gate_kern),
                      "max_mem_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
                      "classes": rows,
                      "classes_note": "HIP events around each C-ABI call on its launch stream, %d steps after the timed region with "
                                      "the stream overlaps off; ATen kernels (the composed gate's mean / sigmoid / mul / cat) are "
                                      "not spanned" % nrep}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Pre-training throughput of the I3D-BYOL wrapper (cstp_amd/i3d_byol.py) on one MI355X, synthetic clips resident in HBM.

    python tools/bench_i3d.py --batch 16 --frames 16 --size 112 --steps 10
    CSTP_I3D_FUSED=0 python tools/bench_i3d.py ...      # SAME pooling and the Mixed tail composed from ATen + per-branch ops (A/B)

Prints one JSON line: ms/step, clips/s, peak GiB, kernel launches per step (torch.profiler device events of one step, both
streams) and how many of them are the SAME-pool and BatchNorm + ReLU + concat kernels of csrc/mixed.hip.  Not the headline metric
(bench.py is)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cstp_amd import i3d_byol  # noqa: E402
from cstp_amd.i3d_byol import I3DBYOL  # noqa: E402
from cstp_amd.optim import FlatSGD  # noqa: E402
from cstp_amd.synthetic import device_batch  # noqa: E402
from cstp_amd.train import PretrainStep  # noqa: E402


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
    model = I3DBYOL(pretrain=True, opts=None).cuda()
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

    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        run(1)
        torch.cuda.synchronize()
    kern = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    print(json.dumps({"config": {"workload": "i3d_byol, B=%d clip pairs 3x%dx%dx%d, full loss_com, clip 18, SGD; fp32"
                                             % (a.batch, a.frames, a.size, a.size),
                                 "path": "fused" if i3d_byol.FUSED else "composed (CSTP_I3D_FUSED=0)"},
                      "ms_per_step": round(ms, 2), "clips_per_s": round(a.batch / ms * 1e3, 2),
                      "max_mem_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
                      "launches_per_step": len(kern),
                      "pool_same_launches_per_step": len([k for k in kern if "pool_same" in k]),
                      "bnc_launches_per_step": len([k for k in kern if "bnc_" in k])}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""R(2+1)D pre-training step with fp32 vs bf16 activation storage, same box, same run: ms/step, clips/s and peak memory of each
(one fresh child process per storage type, so that each peak is its own), then the per-call-site table of the bf16 step (every
spanned C-ABI call under a HIP-event pair, stream overlaps off, summed per (operation, shape)).
The step: R(2+1)D-18, 16 clip pairs of 3x16x112x112 (cfg2), BYOL + the four pretext heads, gradient clipping, SGD (PretrainStep).
usage: python tools/r21d_b16_timing.py [--depth 18] [--batch 16] [--frames 16] [--size 112] [--steps 10] [--warmup 6]"""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one(a):
    from cstp_amd.optim import FlatSGD
    from cstp_amd.r21d_byol import R21DBYOL, layer_sizes_for_depth
    from cstp_amd.synthetic import device_batch
    from cstp_amd.train import PretrainStep
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    model = R21DBYOL(pretrain=True, layer_sizes=layer_sizes_for_depth(a.depth), act_dtype=a.one).cuda()
    arenas = model.flatten_parameters()
    model.train()
    opt = FlatSGD(model.parameters(), lr=0.09, momentum=0.9, weight_decay=5e-4, arenas=arenas)
    step = PretrainStep(model, opt, (0.1, 1.0, 1.0, 1.0, 1.0), clip_grad_norm=True)
    x1, x2, lab = device_batch(a.batch, a.frames, a.size, dev, seed=1)

    def run(n):
        out = None
        for _ in range(n):
            out = step(x1, x2, lab["spa"], lab["tem"], lab["pb"], lab["rot1"], lab["rot2"]).to_host()
        return out
    run(a.warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run(a.steps)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / a.steps * 1e3
    res = {"act_dtype": a.one, "depth": a.depth, "batch": a.batch, "frames": a.frames, "size": a.size, "ms_per_step": round(ms, 2),
           "clips_per_s": round(a.batch / ms * 1e3, 1), "peak_gib": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2),
           "loss_total": round(out["loss"], 5)}
    print("RESULT " + json.dumps(res), flush=True)
    if not a.table:
        return
    from cstp_amd import ops, r21d_byol as rb
    from tools.bench_r3d import AllTimers, classify
    tm = AllTimers()
    ops.kernel_timer = tm
    ops.OVERLAP_WGRAD = False
    rb.OVERLAP_TARGET_FORWARD = False
    run(1)
    tm.enabled = True
    nrep = 2
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run(nrep)
    e1.record()
    torch.cuda.synchronize()
    tm.enabled = False
    rows, by = [], {}
    for (what, key), pairs in tm.pairs.items():
        t = sum(x.elapsed_time(y) for x, y in pairs) / nrep
        cls, flop, nbytes = classify(what, key)
        k = tuple(v for v in key if v != "bf16")
        if what.startswith("conv3d"):
            n, c, d, h, w, ko, kt, kh, kw, st, sh, sw = k[:12]
            name = "%s %dx%d->%d k%d%d%d s%d%d%d @%dx%dx%d" % (what[7:].replace("backward_", "d"), n, c, ko, kt, kh, kw, st, sh, sw, d, h, w)
        else:
            name = "%s %dx%dx%d g%d res%d relu%d" % (what, k[0], k[1], k[2], k[3], int(bool(k[4])), int(bool(k[5])))
        rows.append((t, len(pairs) / nrep, name, flop, nbytes))
        by[cls] = by.get(cls, 0.0) + t
    rows.sort(key=lambda r: -r[0])
    print("%s step under the timers: %.2f ms (overlaps off); spanned calls sum to %.2f ms"
          % (a.one, e0.elapsed_time(e1) / nrep, sum(r[0] for r in rows)))
    print("%-60s %5s %8s %8s %7s %6s" % ("call site", "n/st", "ms/step", "avg_ms", "TF/s", "TB/s"))
    for t, n, name, flop, nbytes in rows:
        avg = t / n
        print("%-60s %5.1f %8.3f %8.4f %7.1f %6.2f" % (name, n, t, avg, flop / avg / 1e9, nbytes / avg / 1e9))
    print({k: round(v, 2) for k, v in sorted(by.items(), key=lambda kv: -kv[1])})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=18)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=112)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--one", choices=("fp32", "bf16"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--table", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a)
    base = [sys.executable, os.path.abspath(__file__), "--depth", str(a.depth), "--batch", str(a.batch), "--frames", str(a.frames),
            "--size", str(a.size), "--steps", str(a.steps), "--warmup", str(a.warmup)]
    for act in ("fp32", "bf16"):
        r = subprocess.run(base + ["--one", act] + (["--table"] if act == "bf16" else []), cwd=ROOT)
        if r.returncode != 0:
            sys.exit(r.returncode)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""ops.ntxent_queue + ops.ntxent_queue_push (csrc/ntxq.h) timed against the ATen composition they replace, in one process on one
box, alternating repeats.  One JSON line per case:
  * part "op":   forward + backward + push at (R, f, K) -- the queue full (n_valid = K), temperature 0.07 -- against
                 F.normalize, cat, matmul, logsumexp and autograd on the same operands, followed by the same push written as
                 a slice assignment of the normalised rows.  The composition builds the [R, R + K] logits (and autograd keeps
                 them); the kernels never do.  Before timing, the two losses and gradients are compared.
  * part "step": the cfg2 pre-training step of bench.py (R(2+1)D-18, B = 16, 3x16x112x112, loss_weight (0.1, 1, 1, 0, 0) +
                 1 x NT-Xent) with --ntxent_queue 0 and with --ntxent_queue K, the queue filled before timing.
Times are host clocks around --inner calls that end in one device synchronise, after a warm-up of each side; the medians of
--repeats alternating runs are reported per call with their minimum and maximum.  Peak memory is the growth of
torch.cuda.max_memory_allocated over the operands."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cstp_amd import ops  # noqa: E402

CASES = [(32, 512, 4096), (32, 512, 65536), (512, 512, 65536), (32, 1024, 65536)]      # (R, f, K)
T = 0.07


def hip_side(reps, queue, k, ptr):
    r = reps.detach().requires_grad_(True)
    loss = ops.ntxent_queue(r, queue, k, T)
    loss.backward()
    ops.ntxent_queue_push(reps, queue, ptr)
    return loss.detach(), r.grad


def aten_side(reps, queue, k, ptr):
    r = reps.detach().requires_grad_(True)
    R = r.shape[0]
    z = torch.nn.functional.normalize(r, dim=1, eps=1e-8)
    logits = (z @ torch.cat([z, queue[:k]], 0).t()) / T
    idx = torch.arange(R, device=r.device)
    pos = logits[idx, (idx + R // 2) % R]
    logits = logits.masked_fill(torch.eye(R, logits.shape[1], dtype=torch.bool, device=r.device), float("-inf"))
    loss = (torch.logsumexp(logits, dim=1) - pos).mean()
    loss.backward()
    with torch.no_grad():
        queue[ptr:ptr + R] = torch.nn.functional.normalize(reps, dim=1, eps=1e-8)
    return loss.detach(), r.grad


def timed(fn, inner):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    for _ in range(inner):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner, torch.cuda.max_memory_allocated() - base, out


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def alternate(a, b, repeats, inner):
    ta, tb, ma, mb = [], [], 0, 0
    for _ in range(repeats):
        ms, mem, _ = timed(a, inner)
        ta.append(ms)
        ma = max(ma, mem)
        ms, mem, _ = timed(b, inner)
        tb.append(ms)
        mb = max(mb, mem)
    return dict(stats(ta), peak_bytes=ma), dict(stats(tb), peak_bytes=mb), round(statistics.median(tb) / statistics.median(ta), 3)


def bench_op(R, f, K, repeats, inner):
    gen = torch.Generator(device="cuda").manual_seed(1)
    reps = torch.randn((R, f), device="cuda", generator=gen)
    queue = torch.nn.functional.normalize(torch.randn((K, f), device="cuda", generator=gen), dim=1)
    q2 = queue.clone()
    ours = lambda: hip_side(reps, queue, K, 0)         # noqa: E731
    theirs = lambda: aten_side(reps, q2, K, 0)         # noqa: E731
    _, _, (l1, g1) = timed(ours, 1)                    # warm-up of both sides, and the comparison
    _, _, (l2, g2) = timed(theirs, 1)
    dl = abs(float(l1) - float(l2)) / abs(float(l2))
    dg = float((g1 - g2).abs().max() / g2.abs().max())
    a, b, speed = alternate(ours, theirs, repeats, inner)
    return dict(part="op", R=R, f=f, K=K, temperature=T, repeats=repeats, inner=inner, splits=ops.ntxent_queue_splits(R, f, K),
                ntxent_queue=a, aten_matmul_logsumexp=b, logits_bytes=R * (R + K) * 4, rel_loss_diff=dl, rel_grad_diff=dg,
                speedup_vs_aten=speed)


def build_step(K, batch):
    from cstp_amd.ntxent import NTXentLoss
    from cstp_amd.optim import FlatSGD
    from cstp_amd.r21d_byol import R21DBYOL, layer_sizes_for_depth
    from cstp_amd.synthetic import device_batch
    from cstp_amd.train import PretrainStep
    torch.manual_seed(1)
    dev = torch.device("cuda", 0)
    model = R21DBYOL(pretrain=True, layer_sizes=layer_sizes_for_depth(18))
    model.cuda(0)
    arenas = model.flatten_parameters()
    model.train()
    opt = FlatSGD(model.parameters(), lr=0.09, momentum=0.9, weight_decay=5e-4, arenas=arenas)
    ntx = NTXentLoss(device=dev, batch_size=batch, temperature=0.5, use_cosine_similarity=True, queue_size=K)
    step = PretrainStep(model, opt, (0.1, 1.0, 1.0, 0.0, 0.0), clip_grad_norm=True, ntxent=ntx, ntxent_weight=1.0)
    x1, x2, lab = device_batch(batch, 16, 112, dev, seed=1)
    return ntx, lambda: step(x1, x2, lab["spa"], lab["tem"], lab["pb"], lab["rot1"], lab["rot2"])


def bench_step(K, repeats, inner, batch):
    ntx0, plain = build_step(0, batch)
    ntxk, queued = build_step(K, batch)
    for _ in range(3):
        plain()
        queued()
    # a full queue without K / (2 B) steps: random unit rows (the timing does not depend on what the rows hold)
    ntxk.queue.copy_(torch.nn.functional.normalize(torch.randn_like(ntxk.queue), dim=1))
    ntxk.n_valid = K
    a, b, ratio = alternate(plain, queued, repeats, inner)
    return dict(part="step", model="r21d_byol-18", batch=batch, clip="3x16x112x112", K=K, repeats=repeats, inner=inner,
                step_queue_0=a, step_queue_K=b, queued_over_plain=ratio)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--parts", nargs="+", default=["op", "step"], choices=["op", "step"])
    ap.add_argument("--step_k", type=int, default=65536)
    ap.add_argument("--step_batch", type=int, default=16)
    ap.add_argument("--step_inner", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_ntxent_queue.py needs a HIP device: there is nothing to time without one")
    if "op" in args.parts:
        for R, f, K in CASES:
            print(json.dumps(bench_op(R, f, K, args.repeats, args.inner)), flush=True)
            torch.cuda.empty_cache()
    if "step" in args.parts:
        print(json.dumps(bench_step(args.step_k, args.repeats, args.step_inner, args.step_batch)), flush=True)


if __name__ == "__main__":
    main()

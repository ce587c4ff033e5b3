#!/usr/bin/env python3
"""The collapse-metric kernels (csrc/health.h) timed against the ATen composition they stand in for, in one process on one box,
alternating repeats on the same inputs.  One JSON line per (part, case), the cases being (n, d) = rows, features:
  * part "gram":    ops.feat_gram (G = x^T x and the column sums in fp64, two launches) against ``x.T @ x`` and ``x.sum(0)`` -- the
                    vendor GEMM, fp32 results;
  * part "pair":    ops.pair_potential (two launches, at most 32 doubles of scratch per row) against ``x @ x.T`` -> ``exp`` ->
                    diagonal zeroed -> fp64 row sums, which builds the [n, n] matrix;
  * part "metrics": the whole of health.metrics (normalise, the two kernels, sim_topk, the copies to the host and the fp64 host
                    arithmetic with two eigvalsh) against the same figures from the ATen composition through the same host
                    arithmetic; ``eigvalsh_ms`` is the host arithmetic alone, timed on the copied sums, so its share of both
                    sides is stated.
A timed window is --inner calls (one for "metrics"), a host clock around work that ends in a device synchronise, after a warm-up
of each side; the medians of --repeats alternating windows are reported with their minimum and maximum.  Before timing the two
answers are compared against fp64 on the device and the errors are part of the line; so is the peak device memory each side
allocates on top of its operands (torch.cuda.max_memory_allocated around one call)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cstp_amd import health, ops  # noqa: E402

CASES = [(9537, 512), (9537, 2048), (3783, 512), (65536, 512)]
T = 2.0


def window(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner, out


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def alternate(ours, theirs, inner, repeats):
    window(ours, max(1, inner // 10))
    window(theirs, max(1, inner // 10))
    t_ours, t_aten = [], []
    for _ in range(repeats):
        t_ours.append(window(ours, inner)[0])
        t_aten.append(window(theirs, inner)[0])
    return stats(t_ours), stats(t_aten), round(statistics.median(t_aten) / statistics.median(t_ours), 3)


def peak_bytes(fn):
    """The most device memory ``fn`` holds on top of what is allocated when it starts."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def operands(n, d, seed):
    """Features as an encoder's pooled output looks: low rank plus noise plus an offset, all on the device; raw and unit rows."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    rank = max(1, d // 16)
    feat = (torch.randn((n, rank), device="cuda", generator=gen) @ torch.randn((rank, d), device="cuda", generator=gen)
            + 0.2 * torch.randn((n, d), device="cuda", generator=gen) + 0.5).contiguous()
    return feat, torch.nn.functional.normalize(feat, dim=1).contiguous()


def rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max())


def aten_gram(x):
    return x.T @ x, x.sum(dim=0)


def aten_pair(x, t=T):
    e = torch.exp((2.0 * t) * (x @ x.T - 1.0))
    e.fill_diagonal_(0.0)
    return e.sum(dim=1, dtype=torch.float64)


def pair_ref(x, t=T, rows=2048):
    """fp64 row sums, a block of rows at a time."""
    xd = x.double()
    out = []
    for i0 in range(0, x.shape[0], rows):
        e = torch.exp((2.0 * t) * (xd[i0:i0 + rows] @ xd.T - 1.0))
        idx = torch.arange(i0, min(i0 + rows, x.shape[0]), device=x.device)
        e[idx - i0, idx] = 0.0
        out.append(e.sum(dim=1))
        del e
    return torch.cat(out)


def aten_metrics(feat, t=T):
    n, d = feat.shape
    x = torch.nn.functional.normalize(feat, dim=1)
    gram, colsum = aten_gram(x)
    s = x @ x.T
    e = torch.exp((2.0 * t) * (s - 1.0))
    e.fill_diagonal_(0.0)
    rowsum = e.sum(dim=1, dtype=torch.float64)
    s.fill_diagonal_(float("-inf"))
    return health.metrics_from_parts(gram, colsum, rowsum, s.max(dim=1).values, n, d, t)


def bench(args):
    for n, d in [CASES[i] for i in args.cases]:
        feat, x = operands(n, d, 1)
        line = dict(n=n, d=d, inner=args.inner, repeats=args.repeats)
        if "gram" in args.parts:
            xd = x.double()
            g_ref, s_ref = xd.T @ xd, xd.sum(dim=0)
            del xd
            g1, s1 = ops.feat_gram(x)
            g2, s2 = aten_gram(x)
            err = {"gram_rel_err_hip": rel(g1, g_ref), "gram_rel_err_aten": rel(g2, g_ref), "colsum_rel_err_hip": rel(s1, s_ref),
                   "colsum_rel_err_aten": rel(s2, s_ref)}
            del g1, g2, g_ref
            t_ours, t_aten, speed = alternate(lambda: ops.feat_gram(x), lambda: aten_gram(x), args.inner, args.repeats)
            print(json.dumps(dict(part="gram", **line, feat_gram=t_ours, aten_xtx_sum=t_aten, speedup_vs_aten=speed,
                                  workspace_bytes=int(ops._lib.load().cstp_feat_gram_workspace_bytes(n, d)),
                                  peak_bytes_ours=peak_bytes(lambda: ops.feat_gram(x)), peak_bytes_aten=peak_bytes(lambda: aten_gram(x)),
                                  **err)), flush=True)
        if "pair" in args.parts:
            ref = pair_ref(x)
            row_rel = lambda a: float(((a.double() - ref).abs() / ref.abs()).max())      # noqa: E731
            err = {"rowsum_rel_err_hip": row_rel(ops.pair_potential(x, T)), "rowsum_rel_err_aten": row_rel(aten_pair(x))}
            del ref
            inner = max(1, args.inner // 5)
            t_ours, t_aten, speed = alternate(lambda: ops.pair_potential(x, T), lambda: aten_pair(x), inner, args.repeats)
            print(json.dumps(dict(part="pair", **dict(line, inner=inner), pair_potential=t_ours, aten_xxt_exp_sum=t_aten,
                                  speedup_vs_aten=speed,
                                  workspace_bytes=int(ops._lib.load().cstp_pair_potential_workspace_bytes(n, d)),
                                  peak_bytes_ours=peak_bytes(lambda: ops.pair_potential(x, T)),
                                  peak_bytes_aten=peak_bytes(lambda: aten_pair(x)), **err)), flush=True)
        if "metrics" in args.parts:
            r1, r2 = health.metrics(feat, T), aten_metrics(feat, T)
            diff = {k: [r1[k], r2[k]] for k in health.KEYS}
            xn = ops.l2_normalize(feat)
            gram, colsum = ops.feat_gram(xn)
            parts = (gram.cpu(), colsum.cpu(), ops.pair_potential(xn, T).cpu(), ops.sim_topk(xn, xn, 1, True)[0][:, 0].cpu())
            del xn, gram, colsum
            host = stats([window(lambda: health.metrics_from_parts(*parts, n, d, T), 1)[0] for _ in range(args.repeats)])
            t_ours, t_aten, speed = alternate(lambda: health.metrics(feat, T), lambda: aten_metrics(feat, T), 1, args.repeats)
            print(json.dumps(dict(part="metrics", **dict(line, inner=1), health_metrics=t_ours, aten_metrics=t_aten,
                                  speedup_vs_aten=speed, eigvalsh_ms=host,
                                  eigvalsh_share_of_ours=round(host["median_ms"] / t_ours["median_ms"], 3),
                                  peak_bytes_ours=peak_bytes(lambda: health.metrics(feat, T)),
                                  peak_bytes_aten=peak_bytes(lambda: aten_metrics(feat, T)), ours_vs_aten=diff)), flush=True)
        del feat, x
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parts", nargs="+", default=["gram", "pair", "metrics"], choices=["gram", "pair", "metrics"])
    ap.add_argument("--inner", type=int, default=20, help="calls per timed window (gram; a fifth of it for pair; 1 for metrics)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cases", nargs="+", type=int, default=list(range(len(CASES))), choices=range(len(CASES)),
                    help="which of the (n, d) cases, by position")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_health.py needs a HIP device: there is nothing to time without one")
    bench(args)


if __name__ == "__main__":
    main()

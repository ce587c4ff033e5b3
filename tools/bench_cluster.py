#!/usr/bin/env python3
"""The k-means kernels (csrc/kmeans.h) timed against the ATen composition they replace, in one process on one box, alternating
repeats.  One JSON line per (part, case), the cases being (n, d, c, r) = rows, features, clusters, restarts:
  * part "iter": one Lloyd iteration of all r restarts -- ops.kmeans_assign + ops.kmeans_update into preallocated buffers
                 (three launches) against, per restart, ``x @ cent.T`` -> ``max`` (values summed in fp64 for the score, indices the
                 assignment) -> ``index_add_`` of the rows into a zeroed [c, d] -> ``F.normalize`` (the [n, c] similarity table
                 exists, index_add_ adds with atomics);
  * part "fit":  cluster.fit (k-means++ seeding, --iters iterations, the final scoring, one host read) against the same loop
                 composed from ATen, from the same seeding, with the same number of iterations and one host read at its end.
A timed window is --inner iterations or one whole fit, a host clock around work that ends in a device synchronise, after a warm-up
of each side; the medians of --repeats alternating windows are reported per call with their minimum and maximum.  Before timing,
the two answers are compared and the differences are part of the line; so is the peak device memory each side allocates on top of
its operands (torch.cuda.max_memory_allocated around one call)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cstp_amd import cluster, ops  # noqa: E402

CASES = [(9537, 512, 101, 10), (9537, 2048, 101, 10), (3783, 512, 101, 1), (65536, 512, 400, 4)]


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


def operands(n, d, c, r, seed):
    """Unit rows around c class directions (so that clusters exist) and r sets of centroids drawn from the rows."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    centres = torch.randn((c, d), device="cuda", generator=gen)
    labels = torch.randint(0, c, (n,), device="cuda", generator=gen)
    x = torch.nn.functional.normalize(centres[labels] + 2.0 * torch.randn((n, d), device="cuda", generator=gen), dim=1).contiguous()
    pick = torch.stack([torch.randperm(n, device="cuda", generator=gen)[:c] for _ in range(r)])
    return x, x[pick].contiguous()


def aten_iteration(x, cent):
    """-> (cent_new [r, c, d], assign [r, n], score [r] fp64): the composition, restart by restart -- one product and one ``max``
    (values for the score, indices for the assignment) per restart."""
    new, assigns, scores = [], [], []
    for s in range(cent.shape[0]):
        best = (x @ cent[s].T).max(dim=1)
        a = best.indices
        total = torch.zeros_like(cent[s]).index_add_(0, a, x)
        empty = (total * total).sum(dim=1, keepdim=True) == 0
        new.append(torch.where(empty, cent[s], torch.nn.functional.normalize(total, dim=1)))
        assigns.append(a)
        scores.append(best.values.double().sum())
    return torch.stack(new), torch.stack(assigns), torch.stack(scores)


def bench_iter(args):
    for n, d, c, r in [CASES[i] for i in args.cases]:
        x, cent = operands(n, d, c, r, 1)
        out_a = (torch.empty((r, n), dtype=torch.int32, device="cuda"), torch.empty((r, n), device="cuda"),
                 torch.empty(r, dtype=torch.int32, device="cuda"), torch.empty(r, dtype=torch.float64, device="cuda"))
        out_u = (torch.empty_like(cent), torch.empty((r, c), dtype=torch.int32, device="cuda"))

        def ours():
            ops.kmeans_assign(x, cent, None, out=out_a)
            return ops.kmeans_update(x, out_a[0], cent, out=out_u)

        theirs = lambda: aten_iteration(x, cent)
        new1 = ours()[0].clone()
        new2, a2, _ = theirs()
        diff = {"assign_agree": float((out_a[0].to(torch.int64) == a2).double().mean()),
                "cent_max_abs_diff": float((new1 - new2).abs().max())}
        t_assign = stats([window(lambda: ops.kmeans_assign(x, cent, None, out=out_a), args.inner)[0] for _ in range(args.repeats)])
        t_update = stats([window(lambda: ops.kmeans_update(x, out_a[0], cent, out=out_u), args.inner)[0] for _ in range(args.repeats)])
        t_ours, t_aten, speed = alternate(ours, theirs, args.inner, args.repeats)
        mem = {"peak_bytes_ours": peak_bytes(lambda: (ops.kmeans_assign(x, cent), ops.kmeans_update(x, out_a[0], cent))),
               "peak_bytes_aten": peak_bytes(theirs)}
        print(json.dumps(dict(part="iter", n=n, d=d, c=c, r=r, inner=args.inner, repeats=args.repeats, kmeans_assign_update=t_ours,
                              aten_mm_max_index_add=t_aten, speedup_vs_aten=speed, kmeans_assign_alone=t_assign,
                              kmeans_update_alone=t_update,
                              workspace_bytes=int(ops._lib.load().cstp_kmeans_workspace_bytes(n, d, c, r)), **diff, **mem)), flush=True)
        del x, cent, out_a, out_u, new1, new2, a2
        torch.cuda.empty_cache()


def aten_fit(x, init, iters):
    """The loop of cluster.fit composed from ATen on unit rows x from the centroids init [r, c, d], one product per restart and
    iteration: -> (final scores [r] CPU, assign [r, n])."""
    cent = init
    r = cent.shape[0]
    log = torch.zeros((iters + 1, r), dtype=torch.float64, device="cuda")
    for t in range(iters):
        cent, _, log[t] = aten_iteration(x, cent)
    best = [(x @ cent[s].T).max(dim=1) for s in range(r)]
    log[iters] = torch.stack([b.values.double().sum() for b in best])
    return log.cpu()[iters], torch.stack([b.indices for b in best])


def bench_fit(args):
    for n, d, c, r in [CASES[i] for i in args.cases]:
        x, _ = operands(n, d, c, r, 2)
        ours = lambda: cluster.fit(x, c, args.iters, r, 0)
        theirs = lambda: aten_fit(x, cluster.init_pp(x, cluster.plan(n, c, r, 0)), args.iters)      # the same seeding on both sides
        r1, r2 = ours(), theirs()
        diff = {"final_score": [r1.score, float(r2[0].max())], "winner": [r1.restart, int(r2[0].argmax())],
                "converged_at": r1.converged_at.tolist()}
        seed_ms = stats([window(lambda: cluster.init_pp(x, cluster.plan(n, c, r, 0)), 1)[0] for _ in range(args.repeats)])
        t_ours, t_aten, speed = alternate(ours, theirs, 1, args.repeats)
        mem = {"peak_bytes_ours": peak_bytes(ours), "peak_bytes_aten": peak_bytes(theirs)}
        print(json.dumps(dict(part="fit", n=n, d=d, c=c, r=r, iters=args.iters, repeats=args.repeats, cluster_fit=t_ours,
                              aten_loop=t_aten, speedup_vs_aten=speed, seeding_alone=seed_ms,
                              ms_per_iteration=round((t_ours["median_ms"] - seed_ms["median_ms"]) / args.iters, 4), **diff, **mem)),
              flush=True)
        del x, r1, r2
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parts", nargs="+", default=["iter", "fit"], choices=["iter", "fit"])
    ap.add_argument("--inner", type=int, default=50, help="iterations per timed window (part iter)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=cluster.DEFAULT_ITERS, help="Lloyd iterations of a fit (part fit)")
    ap.add_argument("--cases", nargs="+", type=int, default=list(range(len(CASES))), choices=range(len(CASES)),
                    help="which of the (n, d, c, r) cases, by position")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_cluster.py needs a HIP device: there is nothing to time without one")
    for part in args.parts:
        {"iter": bench_iter, "fit": bench_fit}[part](args)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""ops.sim_topk (csrc/retrieve.hip) timed against the ATen composition it replaces, ``(q @ g.T).topk(k)``, in one process on one
box, alternating repeats.  One JSON line per case:
  * ucf       3 783 queries x 9 537 gallery rows x 512 features (UCF-101 split 1, R(2+1)D / R3D features);
  * kinetics  20 000 x 240 000 x 512 (a Kinetics-400-like size: the fp32 similarity matrix would be 17.9 GiB);
  * d2048     3 783 x 9 537 x 2 048 (the 3D-ResNet-50 feature width).
The composition is chunked over queries so that one chunk's similarity matrix stays under --chunk_gib; its peak memory is that
chunk.  Times are host clocks around work that ends in a device synchronise, after one warm-up of each side; the medians of
--repeats alternating runs are reported with their minimum and maximum.  Peak memory is the growth of
torch.cuda.max_memory_allocated over the operands.  Before timing, the two answers are compared: the share of queries whose top-k
index SETS agree (they may differ where similarities lie within rounding of the k-th: the two sides sum in different orders)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cstp_amd import _lib, ops  # noqa: E402

CASES = {"ucf": (3783, 9537, 512), "kinetics": (20000, 240000, 512), "d2048": (3783, 9537, 2048)}


def unit(n, d, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return ops.l2_normalize(torch.randn((n, d), device="cuda", generator=g))


def aten_topk(q, g, k, chunk):
    vals, idxs = [], []
    for a in range(0, q.shape[0], chunk):
        v, i = (q[a:a + chunk] @ g.T).topk(k, dim=1)
        vals.append(v)
        idxs.append(i)
    return torch.cat(vals), torch.cat(idxs)


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    return ms, torch.cuda.max_memory_allocated() - base, out


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", nargs="+", default=list(CASES), choices=list(CASES))
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunk_gib", type=float, default=2.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_retrieval.py needs a HIP device: there is nothing to time without one")
    lib = _lib.load()
    for name in args.cases:
        nq, ng, d = CASES[name]
        q, g = unit(nq, d, 1), unit(ng, d, 2)
        chunk = max(1, min(nq, int(args.chunk_gib * 2 ** 30 // (ng * 4))))
        ours, theirs = (lambda: ops.sim_topk(q, g, args.k)), (lambda: aten_topk(q, g, args.k, chunk))
        _, _, (v1, i1) = timed(ours)                   # warm-up of both sides, and the comparison
        _, _, (v2, i2) = timed(theirs)
        same = (torch.sort(i1.to(torch.int64), dim=1).values == torch.sort(i2, dim=1).values).all(dim=1)
        agree = float(same.to(torch.float64).mean())
        vdiff = float((v1 - v2).abs().max())
        del v1, i1, v2, i2, same
        t_ours, t_aten, m_ours, m_aten = [], [], 0, 0
        for _ in range(args.repeats):
            ms, mem, _ = timed(ours)
            t_ours.append(ms)
            m_ours = max(m_ours, mem)
            ms, mem, _ = timed(theirs)
            t_aten.append(ms)
            m_aten = max(m_aten, mem)
        flop = 2.0 * nq * ng * d
        row = {"case": name, "nq": nq, "ng": ng, "d": d, "k": args.k, "repeats": args.repeats,
               "sim_topk": dict(stats(t_ours), peak_bytes=m_ours, workspace_bytes=lib.cstp_simtopk_workspace_bytes(nq, ng, d, args.k),
                                tflops=round(flop / statistics.median(t_ours) / 1e9, 2)),
               "aten_matmul_topk": dict(stats(t_aten), peak_bytes=m_aten, query_chunk=chunk),
               "matrix_bytes": nq * ng * 4, "topk_sets_agree": round(agree, 6), "max_abs_val_diff": vdiff,
               "speedup_vs_aten": round(statistics.median(t_aten) / statistics.median(t_ours), 3)}
        print(json.dumps(row), flush=True)
        del q, g
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""ops.knn_vote (csrc/retrieve.hip) and knn.classify timed against the ATen compositions they replace, in one process on one box,
alternating repeats.  One JSON line per (case, part):
  * part "vote":     ops.knn_vote on a sim_topk answer against label gather + exp + scatter_add_ into a [nq, classes] table +
                     topk (the table is what the kernel never builds);
  * part "classify": knn.classify (l2_normalize x 2, sim_topk, knn_vote) against F.normalize x 2, ``(q @ g.T).topk(k)`` and that
                     composition.
Cases:
  * ucf       3 783 queries x 9 537 gallery rows x 512 features, 101 classes (UCF-101 split 1);
  * kinetics  19 761 x 240 436 x 512, 400 classes (a Kinetics-400-like size; the composition's similarity matrix is chunked over
              queries to stay under --chunk_gib).
Times are host clocks around work that ends in a device synchronise, after one warm-up of each side; the medians of --repeats
alternating runs are reported with their minimum and maximum.  Peak memory is the growth of torch.cuda.max_memory_allocated over
the operands.  Before timing, the two answers are compared: the share of queries with the same top-1 class and the largest
relative difference of the top-1 score among those."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cstp_amd import knn, ops  # noqa: E402

CASES = {"ucf": (3783, 9537, 512, 101), "kinetics": (19761, 240436, 512, 400)}


def aten_vote(val, idx, g_labels, temperature, n_top, classes):
    live = idx >= 0
    lab = g_labels[idx.clamp(min=0).to(torch.int64)]
    w = torch.where(live, torch.exp((val - val[:, :1]) / temperature), torch.zeros_like(val))
    table = torch.zeros((val.shape[0], classes), dtype=torch.float32, device=val.device)
    table.scatter_add_(1, lab, w)
    score, pred = table.topk(n_top, dim=1)
    return pred, score


def aten_classify(q, g, g_labels, k, temperature, n_top, classes, chunk):
    qn, gn = torch.nn.functional.normalize(q, dim=1), torch.nn.functional.normalize(g, dim=1)
    preds, scores = [], []
    for a in range(0, q.shape[0], chunk):
        val, idx = (qn[a:a + chunk] @ gn.T).topk(k, dim=1)
        p, s = aten_vote(val, idx, g_labels, temperature, n_top, classes)
        preds.append(p)
        scores.append(s)
    return torch.cat(preds), torch.cat(scores)


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


def compare(ours, theirs, repeats):
    """-> (row fields of the two sides, agreement of the two answers)"""
    _, _, (p1, s1) = timed(ours)                       # warm-up of both sides, and the comparison
    _, _, (p2, s2) = timed(theirs)
    same = p1[:, 0].to(torch.int64) == p2[:, 0].to(torch.int64)
    rel = ((s1[:, 0] - s2[:, 0]).abs() / s2[:, 0].abs().clamp_min(1e-30))[same]
    agree, sdiff = float(same.to(torch.float64).mean()), float(rel.max()) if rel.numel() else 0.0
    del p1, s1, p2, s2, same, rel
    t_ours, t_aten, m_ours, m_aten = [], [], 0, 0
    for _ in range(repeats):
        ms, mem, _ = timed(ours)
        t_ours.append(ms)
        m_ours = max(m_ours, mem)
        ms, mem, _ = timed(theirs)
        t_aten.append(ms)
        m_aten = max(m_aten, mem)
    return (dict(stats(t_ours), peak_bytes=m_ours), dict(stats(t_aten), peak_bytes=m_aten), agree, sdiff,
            round(statistics.median(t_aten) / statistics.median(t_ours), 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", nargs="+", default=["ucf"], choices=list(CASES))
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--temperature", type=float, default=0.07)
    ap.add_argument("--n_top", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunk_gib", type=float, default=2.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_knn.py needs a HIP device: there is nothing to time without one")
    k, t, n_top = args.k, args.temperature, args.n_top
    for name in args.cases:
        nq, ng, d, classes = CASES[name]
        gen = torch.Generator(device="cuda").manual_seed(1)
        q = torch.randn((nq, d), device="cuda", generator=gen)
        g = torch.randn((ng, d), device="cuda", generator=gen)
        g_labels = torch.randint(0, classes, (ng,), device="cuda", generator=gen)
        labels32 = g_labels.to(torch.int32)
        val, idx = ops.sim_topk(ops.l2_normalize(q), ops.l2_normalize(g), k)
        base = {"case": name, "nq": nq, "ng": ng, "d": d, "classes": classes, "k": k, "temperature": t, "n_top": n_top,
                "repeats": args.repeats}
        ours, theirs, agree, sdiff, speed = compare(lambda: ops.knn_vote(val, idx, labels32, t, n_top),
                                                    lambda: aten_vote(val, idx, g_labels, t, n_top, classes), args.repeats)
        print(json.dumps(dict(base, part="vote", knn_vote=ours, aten_scatter_topk=theirs, table_bytes=nq * classes * 4,
                              top1_agree=round(agree, 6), max_rel_score_diff=sdiff, speedup_vs_aten=speed)), flush=True)
        chunk = max(1, min(nq, int(args.chunk_gib * 2 ** 30 // (ng * 4))))
        ours, theirs, agree, sdiff, speed = compare(
            lambda: knn.classify(q, g, g_labels, k, t, n_top)[:2],
            lambda: aten_classify(q, g, g_labels, k, t, n_top, classes, chunk), args.repeats)
        print(json.dumps(dict(base, part="classify", classify=ours, aten_matmul_topk_scatter=dict(theirs, query_chunk=chunk),
                              matrix_bytes=nq * ng * 4, top1_agree=round(agree, 6), max_rel_score_diff=sdiff,
                              speedup_vs_aten=speed)), flush=True)
        del q, g, val, idx
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The few-shot episode kernel (csrc/fewshot.h) timed against the ATen composition it stands in for, in one process on one box,
alternating repeats on the same tables.  One JSON line per (part, case), the cases being (ns, nq, d, N, shots, Q, E) = support
rows, query rows, features, ways, shot counts, queries per class, episodes:
  * part "op":    ops.fewshot_episodes with device tables (one launch, S * E integers stored) against gather -> prefix sums over
                  the support columns -> normalise -> ``bmm`` -> ``argmax`` -> count, in chunks of episodes whose gathered rows
                  fill at most --chunk_mb;
  * part "eval":  the whole of fewshot.evaluate_features (normalise, the host sampler, the upload of the tables, the launch, the
                  copy of hits to the host, the fp64 statistics) against the same with the ATen composition in place of the op;
                  ``sampler_ms`` is the host sampler alone, so its share of both sides is stated.
A timed window is --inner calls (one for "eval"), a host clock around work that ends in a device synchronise, after a warm-up of
each side; the medians of --repeats alternating windows are reported with their minimum and maximum.  Before timing the two
answers are compared (the share of (shot count, episode) cells whose hit counts differ: fp32 sums in another order may flip a
decision that lies within rounding of a tie) and the line carries the peak device memory each side allocates on top of its
operands (torch.cuda.max_memory_allocated around one call)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cstp_amd import fewshot, ops  # noqa: E402

# UCF-101 split 1 (9537 / 3783 videos, 101 classes) at d = 512 and 2048, HMDB-51 split 1 (3570 / 1530, 51 classes), and the
# largest episode the kernel serves with three shot counts
CASES = [(9537, 3783, 512, 5, (1, 5), 15, 10000, 101), (9537, 3783, 2048, 5, (1, 5), 15, 10000, 101),
         (3570, 1530, 512, 5, (1, 5), 15, 10000, 51), (9537, 3783, 512, 20, (1, 5, 16), 15, 2000, 101)]


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


def operands(ns, nq, d, n_classes, seed):
    """Class-structured features on the device (a direction per class plus noise) and their labels on the host."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    means = torch.randn((n_classes, d), device="cuda", generator=gen)
    out = []
    for n in (ns, nq):
        labels = torch.arange(n) % n_classes
        feat = (0.25 * torch.nn.functional.normalize(means, dim=1)[labels.cuda()]
                + torch.randn((n, d), device="cuda", generator=gen) / d ** 0.5 + 0.05).contiguous()
        out += [feat, labels]
    return out


def aten_episodes(xs, xq, sup_idx, qry_idx, n_query, shots, chunk_mb):
    """hits [S, E] int32 from plain tensor ops, in chunks of episodes."""
    e, n, kmax = sup_idx.shape
    d = xs.shape[1]
    chunk = max(1, int(chunk_mb * 1e6) // (n * (kmax + n_query) * d * 4))
    own = (torch.arange(n * n_query, device=xs.device) // n_query).reshape(1, -1)
    hits = torch.empty((len(shots), e), dtype=torch.int32, device=xs.device)
    for e0 in range(0, e, chunk):
        prefix = xs[sup_idx[e0:e0 + chunk].long()].cumsum(dim=2)                               # [c, N, Kmax, d]
        queries = xq[qry_idx[e0:e0 + chunk].reshape(-1, n * n_query).long()]                   # [c, N Q, d]
        for s, k in enumerate(shots):
            proto = torch.nn.functional.normalize(prefix[:, :, k - 1], dim=2)
            pred = torch.bmm(queries, proto.transpose(1, 2)).argmax(dim=2)
            hits[s, e0:e0 + chunk] = (pred == own).sum(dim=1)
    return hits


def aten_evaluate(s_feat, s_labels, q_feat, q_labels, n_way, shots, n_query, episodes, seed, chunk_mb):
    sup_idx, qry_idx, _ = fewshot.sample_episodes(s_labels, q_labels, n_way, shots[-1], n_query, episodes, seed)
    xs, xq = torch.nn.functional.normalize(s_feat, dim=1), torch.nn.functional.normalize(q_feat, dim=1)
    hits = aten_episodes(xs, xq, sup_idx.to(xs.device), qry_idx.to(xs.device), n_query, shots, chunk_mb)
    return fewshot.accuracy_from_hits(hits.cpu(), n_way * n_query)


def bench(args):
    for ns, nq, d, n_way, shots, n_query, episodes, n_classes in [CASES[i] for i in args.cases]:
        s_feat, s_labels, q_feat, q_labels = operands(ns, nq, d, n_classes, 1)
        line = dict(ns=ns, nq=nq, d=d, n_way=n_way, shots=list(shots), n_query=n_query, episodes=episodes, inner=args.inner,
                    repeats=args.repeats, chunk_mb=args.chunk_mb)
        ev = lambda: fewshot.evaluate_features(s_feat, s_labels, q_feat, q_labels, n_way, shots, n_query, episodes, 0)     # noqa: E731
        ev_aten = lambda: aten_evaluate(s_feat, s_labels, q_feat, q_labels, n_way, shots, n_query, episodes, 0, args.chunk_mb)  # noqa: E731
        if "op" in args.parts:
            sup_idx, qry_idx, _ = fewshot.sample_episodes(s_labels, q_labels, n_way, shots[-1], n_query, episodes, 0)
            sup_idx, qry_idx = sup_idx.cuda(), qry_idx.cuda()
            xs, xq = ops.l2_normalize(s_feat), ops.l2_normalize(q_feat)
            ours = lambda: ops.fewshot_episodes(xs, xq, sup_idx, qry_idx, n_query, shots)                                   # noqa: E731
            theirs = lambda: aten_episodes(xs, xq, sup_idx, qry_idx, n_query, shots, args.chunk_mb)                         # noqa: E731
            h1, h2 = ours(), theirs()
            differ = float((h1 != h2).double().mean())
            acc = [float(v) for v in (h1.double() / (n_way * n_query)).mean(dim=1)]
            t_ours, t_aten, speed = alternate(ours, theirs, args.inner, args.repeats)
            print(json.dumps(dict(part="op", **line, fewshot_episodes=t_ours, aten_gather_bmm=t_aten, speedup_vs_aten=speed,
                                  peak_bytes_ours=peak_bytes(ours), peak_bytes_aten=peak_bytes(theirs),
                                  gather_bytes_unchunked=episodes * n_way * (shots[-1] + n_query) * d * 4,
                                  cells_that_differ=differ, accuracy=acc)), flush=True)
            del sup_idx, qry_idx, xs, xq, h1, h2
        if "eval" in args.parts:
            r1, r2 = ev(), ev_aten()
            sampler = stats([window(lambda: fewshot.sample_episodes(s_labels, q_labels, n_way, shots[-1], n_query, episodes, 0), 1)[0]
                             for _ in range(args.repeats)])
            t_ours, t_aten, speed = alternate(ev, ev_aten, 1, args.repeats)
            print(json.dumps(dict(part="eval", **dict(line, inner=1), evaluate_features=t_ours, aten_evaluate=t_aten,
                                  speedup_vs_aten=speed, sampler_ms=sampler,
                                  sampler_share_of_ours=round(sampler["median_ms"] / t_ours["median_ms"], 3),
                                  peak_bytes_ours=peak_bytes(ev), peak_bytes_aten=peak_bytes(ev_aten),
                                  acc_ours=[r1["acc"][k] for k in shots], ci95_ours=[r1["ci95"][k] for k in shots],
                                  acc_aten=r2[0])), flush=True)
        del s_feat, q_feat
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parts", nargs="+", default=["op", "eval"], choices=["op", "eval"])
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window (op; 1 for eval)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunk_mb", type=float, default=256.0, help="gathered rows per chunk of the ATen composition, in MB")
    ap.add_argument("--cases", nargs="+", type=int, default=list(range(len(CASES))), choices=range(len(CASES)),
                    help="which of the cases, by position")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_fewshot.py needs a HIP device: there is nothing to time without one")
    bench(args)


if __name__ == "__main__":
    main()

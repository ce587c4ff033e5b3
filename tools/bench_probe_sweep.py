#!/usr/bin/env python3
"""The linear-probe sweep (cstp_amd.probe.sweep: G classifiers side by side, four launches per step whatever G is) timed against
the two ways of getting the same G classifiers without it, in one process on one box, alternating repeats.  One JSON line per
case, G in {4, 16} at (n, d, c) = (9537, 512, 101), (9537, 2048, 101), (9537, 1024, 400), default probe flags (100 epochs, batch
1024, Adam, cosine), val_fraction 0.2:
  * "sweep":       probe.sweep, whole: the split, the tables, every step, the validation score and its host read;
  * "sequential":  G probe.fit calls on the train part, one per grid point -- the single-classifier path, five launches per step
                   per grid point, which the sweep leaves untouched;
  * "aten":        the same G heads composed from ATen on a standardised copy of the train part: baddbmm for the logits,
                   log_softmax, hand-written gradients (two bmm-shaped products), a batched AdamW with one learning rate and
                   one weight decay per head, the same permutations and schedules, no host read in the loop either.
A timed window is one whole run of a side, a host clock around work that ends in a device synchronise, after a warm-up of each
side; the medians of --repeats alternating windows are reported with their minimum and maximum, and the peak device memory of one
run of each side (torch.cuda.max_memory_allocated above what was allocated before it).  Before timing, the answers are compared:
every head of the sweep against its probe.fit (bit equality is the contract) and against the ATen heads.
--epochs shortens every side alike (a trace of a few steps shows the launch count as well as a hundred epochs do)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cstp_amd import ops, probe  # noqa: E402

CASES = [(9537, 512, 101), (9537, 2048, 101), (9537, 1024, 400)]
GRIDS = {4: ([3e-4, 3e-3], [0.0, 1e-2]), 16: ([1e-4, 3e-4, 1e-3, 3e-3], [0.0, 1e-3, 1e-2, 1e-1])}
VAL_FRACTION = 0.2


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1), out


def features(n, d, c, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((n, d), device="cuda", generator=gen) * (0.5 + 1.5 * torch.rand(d, device="cuda", generator=gen)) \
        + torch.randn(d, device="cuda", generator=gen)
    labels = torch.randint(0, c, (n,), device="cuda", generator=gen)
    x += 2.0 * torch.nn.functional.one_hot(labels, d).float()                     # something to learn: a class-dependent offset
    return x, labels


def aten_sweep(x_train, y_train, x_val, y_val, c, grid, epochs, batch, seed):
    """-> (W [G, c, d], b [G, c], val hits [G]) of the G heads trained side by side with ATen operations only."""
    n, d = x_train.shape
    G = len(grid)
    perm, _, bounds = probe.plan(n, epochs, batch, grid[0][0], seed)
    steps = epochs * len(bounds)
    lrs = torch.stack([probe.schedule(lr, steps) for lr, _ in grid], dim=1).to("cuda")          # [steps, G]
    wds = torch.tensor([wd for _, wd in grid], dtype=torch.float32, device="cuda").view(G, 1, 1)
    mean, inv_std = probe.standardize(x_train)
    xs = (x_train - mean) * inv_std
    w = torch.zeros((G, c, d), device="cuda")
    b = torch.zeros((G, 1, c), device="cuda")
    state = [torch.zeros_like(t) for t in (w, w, b, b)]
    perm_dev = perm.to("cuda").to(torch.int64)
    loss_log = torch.zeros((steps, G), device="cuda")
    b1, b2 = probe.ADAM_BETAS
    t = 0
    for e in range(epochs):
        for lo, hi in bounds:
            idx = perm_dev[e, lo:hi]
            xb, y = xs.index_select(0, idx), y_train.index_select(0, idx)
            m = xb.shape[0]
            logp = torch.log_softmax(torch.baddbmm(b, xb.expand(G, m, d), w.transpose(1, 2)), dim=2)
            loss_log[t] = -logp[:, torch.arange(m, device="cuda"), y].mean(dim=1)
            g = logp.exp()
            g[:, torch.arange(m, device="cuda"), y] -= 1.0
            g /= m
            dw, db = torch.matmul(g.transpose(1, 2), xb), g.sum(dim=1, keepdim=True)
            lr = lrs[t].view(G, 1, 1)
            c1, c2 = 1.0 - b1 ** (t + 1), 1.0 - b2 ** (t + 1)
            for p, grad, m1, m2, wd in ((w, dw, state[0], state[1], wds), (b, db, state[2], state[3], None)):
                if wd is not None:
                    p.mul_(1.0 - lr * wd)
                m1.mul_(b1).add_(grad, alpha=1.0 - b1)
                m2.mul_(b2).addcmul_(grad, grad, value=1.0 - b2)
                p.sub_(lr / c1 * m1 / (m2.sqrt() / c2 ** 0.5 + probe.ADAM_EPS))
            t += 1
    logits = torch.baddbmm(b, ((x_val - mean) * inv_std).expand(G, -1, d), w.transpose(1, 2))
    hits = (logits.argmax(dim=2) == y_val).sum(dim=1)
    return w, b.view(G, c), hits.cpu(), loss_log


def bench_case(n, d, c, G, args):
    x, labels = features(n, d, c, 4)
    lrs, wds = GRIDS[G]
    grid = probe.grid_points(lrs, wds)
    kw = dict(epochs=args.epochs, batch=probe.DEFAULT_BATCH, seed=0)
    train_idx, val_idx = probe.holdout_split(labels, VAL_FRACTION, kw["seed"])
    tr, va = torch.from_numpy(train_idx).to("cuda").long(), torch.from_numpy(val_idx).to("cuda").long()
    x_train, y_train, x_val, y_val = x[tr], labels[tr], x[va], labels[va]
    ours = lambda: probe.sweep(x, labels, c, lrs, wds, VAL_FRACTION, optimizer="adam", **kw)
    seq = lambda: [probe.fit(x_train, y_train, c, lr=lr, weight_decay=wd, optimizer="adam", **kw) for lr, wd in grid]
    aten = lambda: aten_sweep(x_train, y_train, x_val, y_val, c, grid, kw["epochs"], kw["batch"], kw["seed"])
    mem_sweep, r1 = peak_mib(ours)                                # (these three runs are the warm-up as well)
    mem_seq, r2 = peak_mib(seq)
    mem_aten, r3 = peak_mib(aten)
    steps = int(r1.loss_log.shape[0])
    same = all(torch.equal(r1.w[g], r2[g].w) and torch.equal(r1.b[g], r2[g].b) for g in range(G))
    w_diff = max(float((r1.w[g] - r3[0][g]).abs().max() / r3[0][g].abs().max()) for g in range(G))
    check = {"steps": steps, "n_train": int(train_idx.size), "n_val": int(val_idx.size), "heads_bit_equal_to_fit": same,
             "w_diff_vs_aten_of_maxabs": w_diff, "val_hits": r1.val_hits.tolist(), "val_hits_aten": r3[2].tolist(),
             "selected": list(grid[probe.select(r1)])}
    del r1, r2, r3
    t = {"sweep": [], "sequential": [], "aten": []}
    for _ in range(args.repeats):
        t["sweep"].append(timed(ours)[0])
        t["sequential"].append(timed(seq)[0])
        t["aten"].append(timed(aten)[0])
    med = {k: statistics.median(v) for k, v in t.items()}
    lib = ops._lib.load()
    print(json.dumps(dict(part="sweep", n=n, d=d, c=c, heads=G, lrs=lrs, wds=wds, val_fraction=VAL_FRACTION, repeats=args.repeats, **kw,
                          sweep=stats(t["sweep"]), sequential_fits=stats(t["sequential"]), aten_batched=stats(t["aten"]),
                          speedup_vs_sequential=round(med["sequential"] / med["sweep"], 3),
                          speedup_vs_aten=round(med["aten"] / med["sweep"], 3), ms_per_step=round(med["sweep"] / steps, 4),
                          peak_mib={"sweep": mem_sweep, "sequential": mem_seq, "aten": mem_aten},
                          workspace_bytes=int(lib.cstp_probe_sweep_workspace_bytes(G, min(kw["batch"], int(train_idx.size)), d, c)),
                          **check)), flush=True)
    del x, labels, x_train, x_val
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--heads", nargs="+", type=int, default=[4, 16], choices=sorted(GRIDS))
    ap.add_argument("--cases", nargs="+", type=int, default=list(range(len(CASES))), choices=range(len(CASES)),
                    help="which of the (n, d, c) cases, by position")
    ap.add_argument("--epochs", type=int, default=probe.DEFAULT_EPOCHS)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_probe_sweep.py needs a HIP device: there is nothing to time without one")
    for i in args.cases:
        for G in args.heads:
            bench_case(*CASES[i], G, args)


if __name__ == "__main__":
    main()

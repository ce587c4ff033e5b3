#!/usr/bin/env python3
"""The linear-probe kernels (csrc/probe.h) timed against the ATen compositions they replace, in one process on one box,
alternating repeats.  One JSON line per (part, case):
  * part "step":    ops.probe_step (rows gathered and standardised on load, loss, hits, dW, db: three launches) against
                    index_select + standardise + addmm -> log_softmax -> nll_loss -> autograd for dW, db, at
                    (m, d, c) = (1024, 512, 101), (1024, 2048, 101), (9537, 512, 101), (1024, 1024, 400); the feature matrix has
                    9 537 rows and the batch is a permutation prefix (the full matrix in order where m = 9 537);
  * part "fit":     probe.fit at n = 9 537, d = 512, c = 101 with the default flags (100 epochs, batch 1024, Adam, cosine from
                    1e-3) against the same loop composed from ATen (a standardised copy of the features made once, index_select,
                    F.cross_entropy, backward, torch.optim.AdamW, the same permutations and learning rates, no host read in the
                    loop either);
  * part "predict": ops.probe_predict at n = 3 783 (the UCF-101 test list), d = 512, c = 101 against
                    ``(xs @ W.T + b).topk(5)`` on a standardised copy.
A timed window is --inner calls (step, predict) or one whole fit, a host clock around work that ends in a device synchronise,
after a warm-up of each side; the medians of --repeats alternating windows are reported per call with their minimum and maximum.
Before timing, the two answers are compared and the differences are part of the line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cstp_amd import ops, probe  # noqa: E402

N_GALLERY, N_QUERY = 9537, 3783
STEP_CASES = [(1024, 512, 101), (1024, 2048, 101), (9537, 512, 101), (1024, 1024, 400)]


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


def operands(n, d, c, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((n, d), device="cuda", generator=gen) * (0.5 + 1.5 * torch.rand(d, device="cuda", generator=gen)) \
        + torch.randn(d, device="cuda", generator=gen)
    labels = torch.randint(0, c, (n,), device="cuda", generator=gen)
    w = torch.randn((c, d), device="cuda", generator=gen) / d ** 0.5
    b = 0.1 * torch.randn(c, device="cuda", generator=gen)
    mean, inv_std = probe.standardize(x)
    return x, labels, w, b, mean, inv_std


def aten_step(x, labels, w, b, rows, mean, inv_std):
    xb, y = (x, labels) if rows is None else (x.index_select(0, rows), labels.index_select(0, rows))
    xs = (xb - mean) * inv_std
    w = w.detach().requires_grad_()
    b = b.detach().requires_grad_()
    logits = torch.addmm(b, xs, w.T)
    loss = torch.nn.functional.nll_loss(torch.log_softmax(logits, dim=1), y)
    dw, db = torch.autograd.grad(loss, (w, b))
    hits = (logits.argmax(dim=1) == y).sum()
    return loss.detach(), hits, dw, db


def bench_step(args):
    for m, d, c in [STEP_CASES[i] for i in args.step_cases]:
        x, labels, w, b, mean, inv_std = operands(N_GALLERY, d, c, 1)
        rows = None if m == N_GALLERY else torch.randperm(N_GALLERY, device="cuda")[:m].to(torch.int32)
        rows64 = None if rows is None else rows.to(torch.int64)
        out = (torch.empty(1, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"), torch.empty_like(w), torch.empty_like(b))
        ours = lambda: ops.probe_step(x, labels, w, b, rows, mean, inv_std, out=out)
        theirs = lambda: aten_step(x, labels, w, b, rows64, mean, inv_std)
        l1, h1, dw1, db1 = [t.clone() for t in ours()]
        l2, h2, dw2, db2 = theirs()
        diff = {"loss_rel_diff": float((l1 - l2).abs() / l2.abs()), "hits": [int(h1), int(h2)],
                "dw_diff_of_maxabs": float((dw1 - dw2).abs().max() / dw2.abs().max()),
                "db_diff_of_maxabs": float((db1 - db2).abs().max() / db2.abs().max())}
        t_ours, t_aten, speed = alternate(ours, theirs, args.inner, args.repeats)
        print(json.dumps(dict(part="step", m=m, n=N_GALLERY, d=d, c=c, inner=args.inner, repeats=args.repeats, probe_step=t_ours,
                              aten_addmm_logsoftmax_autograd=t_aten, speedup_vs_aten=speed,
                              workspace_bytes=int(ops._lib.load().cstp_probe_workspace_bytes(m, d, c)), **diff)), flush=True)
        del x, labels, w, b, out
        torch.cuda.empty_cache()


def aten_fit(x, labels, c, epochs, batch, lr, weight_decay, seed):
    n, d = x.shape
    perm, lrs, bounds = probe.plan(n, epochs, batch, lr, seed)
    mean, inv_std = probe.standardize(x)
    xs = (x - mean) * inv_std
    lin = torch.nn.Linear(d, c, device="cuda")
    torch.nn.init.zeros_(lin.weight)
    torch.nn.init.zeros_(lin.bias)
    opt = torch.optim.AdamW([{"params": [lin.weight], "weight_decay": weight_decay}, {"params": [lin.bias], "weight_decay": 0.0}],
                            lr=lr, betas=probe.ADAM_BETAS, eps=probe.ADAM_EPS)
    perm_dev, lr_list = perm.to("cuda").to(torch.int64), lrs.tolist()
    loss_log = torch.zeros(len(lr_list), device="cuda")
    hit_log = torch.zeros(len(lr_list), dtype=torch.int64, device="cuda")
    t = 0
    for e in range(epochs):
        for lo, hi in bounds:
            idx = perm_dev[e, lo:hi]
            y = labels.index_select(0, idx)
            logits = lin(xs.index_select(0, idx))
            loss = torch.nn.functional.cross_entropy(logits, y)
            for group in opt.param_groups:
                group["lr"] = lr_list[t]
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            loss_log[t] = loss.detach()
            hit_log[t] = (logits.argmax(dim=1) == y).sum()
            t += 1
    return lin.weight.detach(), lin.bias.detach(), loss_log.cpu(), hit_log.cpu()


def bench_fit(args):
    d, c = 512, 101
    x, labels, _, _, _, _ = operands(N_GALLERY, d, c, 2)
    x += 2.0 * torch.nn.functional.one_hot(labels, d).float()                     # something to learn: a class-dependent offset
    kw = dict(epochs=probe.DEFAULT_EPOCHS, batch=probe.DEFAULT_BATCH, lr=probe.DEFAULT_LR, weight_decay=probe.DEFAULT_WD, seed=0)
    ours = lambda: probe.fit(x, labels, c, optimizer="adam", **kw)
    theirs = lambda: aten_fit(x, labels, c, **kw)
    r1, r2 = ours(), theirs()
    steps = r1.loss_log.numel()
    diff = {"steps": steps, "first_loss": [float(r1.loss_log[0]), float(r2[2][0])],
            "last_loss": [float(r1.loss_log[-1]), float(r2[2][-1])],
            "last_epoch_hits": [int(r1.hit_log[-len(r1.batch_bounds):].sum()), int(r2[3][-len(r1.batch_bounds):].sum())],
            "w_diff_of_maxabs": float((r1.w - r2[0]).abs().max() / r2[0].abs().max())}
    t_ours, t_aten, speed = alternate(ours, theirs, 1, args.repeats)
    print(json.dumps(dict(part="fit", n=N_GALLERY, d=d, c=c, repeats=args.repeats, probe_fit=t_ours, aten_adamw_loop=t_aten,
                          speedup_vs_aten=speed, ms_per_step=round(t_ours["median_ms"] / steps, 4), **kw, **diff)), flush=True)


def bench_predict(args):
    d, c = 512, 101
    x, _, w, b, mean, inv_std = operands(N_QUERY, d, c, 3)
    xs = (x - mean) * inv_std
    ours = lambda: ops.probe_predict(x, w, b, mean, inv_std, 5)
    theirs = lambda: torch.addmm(b, xs, w.T).topk(5, dim=1)
    p1, s1 = ours()
    s2, p2 = theirs()
    same = p1[:, 0].to(torch.int64) == p2[:, 0]
    diff = {"top1_agree": float(same.double().mean()), "max_abs_score_diff": float((s1 - s2).abs()[p1.to(torch.int64) == p2].max())}
    t_ours, t_aten, speed = alternate(ours, theirs, args.inner, args.repeats)
    print(json.dumps(dict(part="predict", n=N_QUERY, d=d, c=c, n_top=5, inner=args.inner, repeats=args.repeats, probe_predict=t_ours,
                          aten_addmm_topk_on_standardised_copy=t_aten, speedup_vs_aten=speed, **diff)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parts", nargs="+", default=["step", "fit", "predict"], choices=["step", "fit", "predict"])
    ap.add_argument("--inner", type=int, default=200, help="calls per timed window (step, predict)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step_cases", nargs="+", type=int, default=list(range(len(STEP_CASES))), choices=range(len(STEP_CASES)),
                    help="part step: which of its (m, d, c) cases, by position")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_probe.py needs a HIP device: there is nothing to time without one")
    for part in args.parts:
        {"step": bench_step, "fit": bench_fit, "predict": bench_predict}[part](args)


if __name__ == "__main__":
    main()

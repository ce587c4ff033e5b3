"""Linear-probe evaluation on cached features: a softmax classifier trained on the frozen encoder's per-video features.

A frozen encoder's features do not change from epoch to epoch, so they are extracted once (retrieval.extract_features) and the
classifier is trained on the [videos x d] matrix where it lies: ops.probe_step (csrc/probe.h) gathers a batch of rows, standardises
them on load and returns loss, hit count and the gradients in three launches; the update is the flat-arena Adam / SGD kernel
with a device-resident learning rate; ops.probe_predict ranks the query videos' classes in one launch.  The training loop reads
nothing back and allocates nothing per step: loss and hits of step t land in device log vectors and are read once at the end.
Serves the linear_probe.py driver.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Tuple

import torch

from . import knn, ops, retrieval

DEFAULT_EPOCHS, DEFAULT_BATCH, DEFAULT_LR, DEFAULT_WD, DEFAULT_OPTIMIZER, DEFAULT_TOP = 100, 1024, 1e-3, 0.0, "adam", 5
OPTIMIZERS = ("adam", "sgd")
ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8


class ProbeResult(NamedTuple):
    w: torch.Tensor                         # [c, d] fp32, device
    b: torch.Tensor                         # [c] fp32, device
    mean: Optional[torch.Tensor]            # [d] fp32 or None (standardize=False)
    inv_std: Optional[torch.Tensor]
    loss_log: torch.Tensor                  # [steps] fp32, CPU: the batch loss of every step
    hit_log: torch.Tensor                   # [steps] int32, CPU: the batch's correctly classified rows, before the step's update
    batch_bounds: List[Tuple[int, int]]     # the batches of one epoch as slices of its permutation


def standardize(feat: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (mean [d], inv_std [d]) fp32: per-dimension mean and 1 / sqrt(population variance) of feat [n, d], taken in fp64;
    inv_std is 0 where the variance is 0, so a dead channel is dropped (for the queries too), not amplified."""
    f = feat.to(torch.float64)
    mean = f.mean(dim=0)
    var = ((f - mean) ** 2).mean(dim=0)
    inv_std = torch.where(var > 0, 1.0 / torch.sqrt(var), torch.zeros_like(var))
    return mean.to(torch.float32), inv_std.to(torch.float32)


_standardize = standardize                  # fit's flag of the same name shadows it


def plan(n: int, epochs: int, batch: int, lr: float, seed: int):
    """The draws and the schedule of a fit, a pure function of its arguments -> (perm [epochs, n] int32 CPU, lrs [steps] fp32 CPU,
    batch_bounds): epoch e's permutation of the rows comes from a private CPU generator seeded by (seed, e); the batches of an
    epoch are the consecutive slices [lo, hi) of batch_bounds (the last one short; batch 0: one full batch); step t of
    T = epochs * len(batch_bounds) runs at lr * 0.5 * (1 + cos(pi * t / T)): from lr towards 0."""
    n, epochs, batch = int(n), int(epochs), int(batch)
    if n < 1 or epochs < 1 or batch < 0:
        raise ValueError("plan: n >= 1, epochs >= 1 and batch >= 0 are required, got %d, %d, %d" % (n, epochs, batch))
    size = n if batch == 0 else min(batch, n)
    bounds = [(lo, min(lo + size, n)) for lo in range(0, n, size)]
    perm = torch.empty((epochs, n), dtype=torch.int32)
    gen = torch.Generator(device="cpu")
    for e in range(epochs):
        gen.manual_seed((int(seed) * 1000003 + e) % (1 << 63))
        perm[e] = torch.randperm(n, generator=gen).to(torch.int32)
    steps = epochs * len(bounds)
    t = torch.arange(steps, dtype=torch.float64)
    lrs = (float(lr) * 0.5 * (1.0 + torch.cos(math.pi * t / steps))).to(torch.float32)
    return perm, lrs, bounds


def fit(feat: torch.Tensor, labels: torch.Tensor, n_classes: int, epochs: int = DEFAULT_EPOCHS, batch: int = DEFAULT_BATCH,
        lr: float = DEFAULT_LR, weight_decay: float = DEFAULT_WD, optimizer: str = DEFAULT_OPTIMIZER, momentum: float = 0.9,
        seed: int = 0, standardize: bool = True) -> ProbeResult:
    """Trains W [n_classes, d], b from zero on feat [n, d] fp32 / labels [n] int64 (device tensors).  Adam: torch.optim.AdamW
    arithmetic, the decay on W only; SGD: momentum, the decay (coupled) on W only.  The first step's loss is ln(n_classes)."""
    if optimizer not in OPTIMIZERS:
        raise ValueError("probe optimizer %r: one of %s" % (optimizer, ", ".join(OPTIMIZERS)))
    if not (lr > 0.0 and lr < float("inf")) or weight_decay < 0.0:
        raise ValueError("probe: lr must be finite and > 0 and weight_decay >= 0, got %r and %r" % (lr, weight_decay))
    if feat.dim() != 2:
        raise ValueError("probe features must be [rows, features], got %s" % (tuple(feat.shape),))
    n, d = feat.shape
    c = int(n_classes)
    dev = feat.device
    perm, lrs, bounds = plan(n, epochs, batch, lr, seed)
    mean, inv_std = _standardize(feat) if standardize else (None, None)
    feat = feat.contiguous()
    labels = labels.to(torch.int64).contiguous()
    wn = (c * d + 3) // 4 * 4                                     # b starts on a 16-byte boundary
    seg = wn + (c + 3) // 4 * 4
    arena = torch.zeros((4 if optimizer == "adam" else 3) * seg, dtype=torch.float32, device=dev)
    parts = [arena[i * seg:(i + 1) * seg] for i in range(arena.numel() // seg)]
    w, dw, *state_w = [p[:c * d].view(c, d) for p in parts]
    b, db, *state_b = [p[wn:wn + c] for p in parts]
    steps = lrs.numel()
    lrs_dev = lrs.to(dev)
    perm_dev = perm.to(dev) if batch != 0 else None
    loss_log = torch.zeros(steps, dtype=torch.float32, device=dev)
    hit_log = torch.zeros(steps, dtype=torch.int32, device=dev)
    t = 0
    for e in range(int(epochs)):
        for lo, hi in bounds:
            rows = perm_dev[e, lo:hi] if perm_dev is not None else None
            ops.probe_step(feat, labels, w, b, rows, mean, inv_std, out=(loss_log[t:t + 1], hit_log[t:t + 1], dw, db))
            step_lr = lrs_dev[t:t + 1]
            if optimizer == "adam":
                ops.adam_step_(w, dw, state_w[0], state_w[1], step_lr, ADAM_BETAS[0], ADAM_BETAS[1], ADAM_EPS, weight_decay, True,
                               t + 1)
                ops.adam_step_(b, db, state_b[0], state_b[1], step_lr, ADAM_BETAS[0], ADAM_BETAS[1], ADAM_EPS, 0.0, True, t + 1)
            else:
                ops.sgd_step_(w, dw, state_w[0], step_lr, momentum, weight_decay, None, t == 0, write_back_grad=False)
                ops.sgd_step_(b, db, state_b[0], step_lr, momentum, 0.0, None, t == 0, write_back_grad=False)
            t += 1
    return ProbeResult(w, b, mean, inv_std, loss_log.cpu(), hit_log.cpu(), bounds)      # the one host read


def epoch_means(result: ProbeResult, n: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (mean loss [epochs] fp64, hits / n [epochs] fp64) per epoch from the step logs: step losses weighted by batch size."""
    sizes = torch.tensor([hi - lo for lo, hi in result.batch_bounds], dtype=torch.float64)
    loss = result.loss_log.to(torch.float64).reshape(-1, sizes.numel())
    hits = result.hit_log.to(torch.float64).reshape(-1, sizes.numel())
    return (loss * sizes).sum(dim=1) / n, hits.sum(dim=1) / n


def predict(result: ProbeResult, feat: torch.Tensor, n_top: int = DEFAULT_TOP):
    """-> (pred [n, n_top] int32, score [n, n_top] fp32) of feat [n, d] under the fitted classifier."""
    return ops.probe_predict(feat.contiguous(), result.w, result.b, result.mean, result.inv_std, n_top)


def evaluate(model, gallery_loader, query_loader, n_classes: int, **fit_args) -> dict:
    """Features of both loaders (one whole video per item), the fit on the gallery, top-1 / top-5 of the queries.  The model runs
    in eval mode under no_grad and comes back in the mode it went in with (as knn.evaluate)."""
    net = retrieval._inner(model)
    was_outer, was_inner = model.training, net.training
    try:
        g_feat, g_labels = retrieval.extract_features(model, gallery_loader)
        q_feat, q_labels = retrieval.extract_features(model, query_loader)
    finally:
        model.train(was_outer)
        if net is not model:
            net.train(was_inner)
    res = fit(g_feat, g_labels, n_classes, **fit_args)
    pred, _ = predict(res, q_feat, DEFAULT_TOP)
    acc = knn.accuracy(pred, q_labels, (1, 5))
    n = int(g_feat.shape[0])
    loss, train_acc = epoch_means(res, n)
    return {"top1": acc[1], "top5": acc[5], "train_top1": float(train_acc[-1]), "first_loss": float(res.loss_log[0]),
            "last_epoch_loss": float(loss[-1]), "n_query": int(q_feat.shape[0]), "n_gallery": n,
            "feature_dim": int(g_feat.shape[1]), "n_classes": int(n_classes),
            "epochs": int(fit_args.get("epochs", DEFAULT_EPOCHS)), "batch": int(fit_args.get("batch", DEFAULT_BATCH)),
            "lr": float(fit_args.get("lr", DEFAULT_LR)), "weight_decay": float(fit_args.get("weight_decay", DEFAULT_WD)),
            "optimizer": str(fit_args.get("optimizer", DEFAULT_OPTIMIZER))}

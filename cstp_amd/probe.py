"""Linear-probe evaluation on cached features: a softmax classifier trained on the frozen encoder's per-video features.

A frozen encoder's features do not change from epoch to epoch, so they are extracted once (retrieval.extract_features) and the
classifier is trained on the [videos x d] matrix where it lies: ops.probe_step (csrc/probe.h) gathers a batch of rows, standardises
them on load and returns loss, hit count and the gradients in three launches; the update is the flat-arena Adam / SGD kernel
with a device-resident learning rate; ops.probe_predict ranks the query videos' classes in one launch.  The training loop reads
nothing back and allocates nothing per step: loss and hits of step t land in device log vectors and are read once at the end.
Serves the linear_probe.py driver.

sweep() trains a grid of (learning rate, weight decay) classifiers side by side on a stratified part of the train rows and
scores them on the rest (holdout_split): ops.probe_sweep_step and one table-optimizer launch per step whatever the grid's size,
every head with the bits fit() would give it alone.  select() names the winner; evaluate(lrs=...) refits it with fit() on the
whole train list, so the reported classifier is fit's and the test list never takes part in the selection.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import knn, ops, optim, retrieval

DEFAULT_EPOCHS, DEFAULT_BATCH, DEFAULT_LR, DEFAULT_WD, DEFAULT_OPTIMIZER, DEFAULT_TOP = 100, 1024, 1e-3, 0.0, "adam", 5
OPTIMIZERS = ("adam", "sgd")
ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8
DEFAULT_VAL_FRACTION, MAX_HEADS = 0.2, ops.PROBE_MAX_HEADS


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
    return perm, schedule(lr, epochs * len(bounds)), bounds


def schedule(lr: float, steps: int) -> torch.Tensor:
    """plan()'s learning rates [steps] fp32 CPU: lr * 0.5 * (1 + cos(pi * t / steps)) taken in fp64, rounded once."""
    t = torch.arange(steps, dtype=torch.float64)
    return (float(lr) * 0.5 * (1.0 + torch.cos(math.pi * t / steps))).to(torch.float32)


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


class SweepResult(NamedTuple):
    grid: List[Tuple[float, float]]         # head g = (lr, weight decay), lr-major in the order given
    val_hits: torch.Tensor                  # [G] int32, CPU: correctly classified held-out rows after the last step
    val_loss: torch.Tensor                  # [G] fp32, CPU: mean cross-entropy of the held-out rows
    loss_log: torch.Tensor                  # [steps, G] fp32, device: the batch loss of every step, per head
    hit_log: torch.Tensor                   # [steps, G] int32, device
    w: torch.Tensor                         # [G, c, d] fp32, device (strided view of the parameter arena)
    b: torch.Tensor                         # [G, c]
    mean: torch.Tensor                      # [d]: the statistics of the train part
    inv_std: torch.Tensor
    train_idx: np.ndarray                   # int32, ascending: the rows trained on
    val_idx: np.ndarray                     # int32, ascending: the rows scored
    batch_bounds: List[Tuple[int, int]]


def _seed(seed: int, k: int) -> int:
    return (int(seed) * 1000003 + int(k)) % (1 << 63)


def holdout_split(labels, fraction: float, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """-> (train_idx, val_idx) int32, ascending, disjoint, together 0..n-1: a stratified hold-out of the rows, a pure host
    function of its arguments.  Per class (ascending label value): its rows in ascending order, permuted by a private CPU
    generator seeded by (seed, class); the first floor(fraction * n_c + 0.5) of them go to validation -- at least one when the
    class has two rows or more, none when it has one."""
    fraction = float(fraction)
    if not (fraction > 0.0 and fraction <= 0.5):
        raise ValueError("holdout_split: fraction must be in (0, 0.5], got %r" % (fraction,))
    lab = np.asarray(labels.detach().cpu() if isinstance(labels, torch.Tensor) else labels).astype(np.int64)
    if lab.ndim != 1 or lab.size < 1 or lab.size >= 1 << 31:
        raise ValueError("holdout_split: labels must be a non-empty vector, got shape %s" % (lab.shape,))
    gen = torch.Generator(device="cpu")
    val = []
    for cls in np.unique(lab):
        rows = np.flatnonzero(lab == cls)
        n_c = rows.size
        k = 0 if n_c < 2 else max(1, int(math.floor(fraction * n_c + 0.5)))
        gen.manual_seed(_seed(seed, int(cls)))
        order = torch.randperm(n_c, generator=gen).numpy()
        val.append(rows[order[:k]])
    val_idx = np.sort(np.concatenate(val)).astype(np.int32)
    keep = np.ones(lab.size, dtype=bool)
    keep[val_idx] = False
    return np.flatnonzero(keep).astype(np.int32), val_idx


def grid_points(lrs: Sequence[float], wds: Sequence[float]) -> List[Tuple[float, float]]:
    """The heads of a sweep, lr-major in the order given: head i * len(wds) + j = (lrs[i], wds[j]).  Refuses an empty list,
    duplicates within a list, a rate that is not finite and > 0, a decay that is not finite and >= 0, more than 32 points."""
    lrs, wds = [float(v) for v in lrs], [float(v) for v in wds]
    if not lrs or not wds:
        raise ValueError("probe sweep: lrs and wds must not be empty")
    if any(not (v > 0.0 and v < float("inf")) for v in lrs) or any(not (v >= 0.0 and v < float("inf")) for v in wds):
        raise ValueError("probe sweep: every lr must be finite and > 0 and every wd finite and >= 0, got %r and %r" % (lrs, wds))
    if len(set(lrs)) != len(lrs) or len(set(wds)) != len(wds):
        raise ValueError("probe sweep: duplicate values in lrs %r or wds %r" % (lrs, wds))
    if len(lrs) * len(wds) > MAX_HEADS:
        raise ValueError("probe sweep: %d x %d grid points, at most %d train side by side" % (len(lrs), len(wds), MAX_HEADS))
    return [(lr, wd) for lr in lrs for wd in wds]


def sweep_tables(grid: Sequence[Tuple[float, float]], c: int, d: int, steps: int):
    """The tables of the sweep's one optimizer launch per step (csrc/optim_table.h), pure host code -> (chunks [(segment, offset,
    length)], hyper [steps, 2 G, 2] fp32 CPU).  Segment 2 g is W_g, 2 g + 1 is b_g, in the arena of ops.probe_head_views.  Row
    t of hyper is the launch's {lr scale, weight decay} table at step t: the scale column holds schedule(lr_g, steps)[t] ITSELF --
    the fp32 rate fit() would step with -- and the launch's base rate is 1.0, so lr * scale is that value exactly; the decay is
    wd_g on W_g and 0 on b_g."""
    wn = (c * d + 3) // 4 * 4
    seg = wn + (c + 3) // 4 * 4
    slots = []
    for g, (_, wd) in enumerate(grid):
        slots += [(g * seg, c * d, 1.0, wd), (g * seg + wn, c, 1.0, 0.0)]
    chunks, rows = optim.hyper_tables(slots, ops.LARS_CHUNK)
    hyper = torch.tensor(rows, dtype=torch.float32).repeat(steps, 1, 1)
    for g, (lr, _) in enumerate(grid):
        hyper[:, 2 * g:2 * g + 2, 0] = schedule(lr, steps)[:, None]
    return chunks, hyper


def sweep(feat: torch.Tensor, labels: torch.Tensor, n_classes: int, lrs: Sequence[float], wds: Sequence[float] = (DEFAULT_WD,),
          val_fraction: float = DEFAULT_VAL_FRACTION, epochs: int = DEFAULT_EPOCHS, batch: int = DEFAULT_BATCH,
          optimizer: str = DEFAULT_OPTIMIZER, momentum: float = 0.9, seed: int = 0) -> SweepResult:
    """Trains the G = len(lrs) * len(wds) classifiers of grid_points(lrs, wds) side by side, from zero, on the train part of
    holdout_split(labels, val_fraction, seed), and scores them on the held-out part.  The standardisation statistics are the
    train part's; the batches are plan(n_train, ...)'s permutations mapped through train_idx.  Head g ends with the bits of
    fit(feat[train_idx], labels[train_idx], lr=lr_g, weight_decay=wd_g, ...) at the same seed: four launches per step whatever G
    is, nothing read back or allocated per step, one host read (the validation scores) at the end."""
    if optimizer not in OPTIMIZERS:
        raise ValueError("probe optimizer %r: one of %s" % (optimizer, ", ".join(OPTIMIZERS)))
    grid = grid_points(lrs, wds)
    if feat.dim() != 2:
        raise ValueError("probe features must be [rows, features], got %s" % (tuple(feat.shape),))
    n, d = feat.shape
    c, G = int(n_classes), len(grid)
    train_idx, val_idx = holdout_split(labels, val_fraction, seed)
    if val_idx.size == 0:
        raise ValueError("probe sweep: no class has two rows, nothing can be held out")
    dev = feat.device
    n_train = int(train_idx.size)
    perm, _, bounds = plan(n_train, epochs, batch, grid[0][0], seed)
    steps = int(epochs) * len(bounds)
    chunks, hyper = sweep_tables(grid, c, d, steps)
    feat = feat.contiguous()
    labels = labels.to(torch.int64).contiguous()
    train_dev = torch.from_numpy(train_idx).to(dev)
    val_dev = torch.from_numpy(val_idx).to(dev)
    mean, inv_std = _standardize(feat[train_dev.long()])
    rows_dev = train_dev[perm.to(dev).long()] if batch != 0 else None             # [epochs, n_train] int32
    seg = (c * d + 3) // 4 * 4 + (c + 3) // 4 * 4
    n_buf = 4 if optimizer == "adam" else 3
    arena = torch.zeros(n_buf * G * seg, dtype=torch.float32, device=dev)
    bufs = [arena[i * G * seg:(i + 1) * G * seg] for i in range(n_buf)]
    (w, b), (dw, db) = ops.probe_head_views(bufs[0], G, c, d), ops.probe_head_views(bufs[1], G, c, d)
    chunks_dev = torch.tensor(chunks, dtype=torch.int32, device=dev)
    hyper_dev = hyper.to(dev)
    one = torch.ones(1, dtype=torch.float32, device=dev)
    loss_log = torch.zeros((steps, G), dtype=torch.float32, device=dev)
    hit_log = torch.zeros((steps, G), dtype=torch.int32, device=dev)
    val = torch.zeros((2, G), dtype=torch.float32, device=dev)                     # row 1 holds the int32 hit counts
    t = 0
    for e in range(int(epochs)):
        for lo, hi in bounds:
            rows = rows_dev[e, lo:hi] if rows_dev is not None else train_dev
            ops.probe_sweep_step(feat, labels, w, b, rows, mean, inv_std, out=(loss_log[t], hit_log[t], dw, db))
            if optimizer == "adam":
                ops.tab_adam_step_(bufs[0], bufs[1], bufs[2], bufs[3], chunks_dev, hyper_dev[t], one, ADAM_BETAS[0], ADAM_BETAS[1],
                                   ADAM_EPS, True, t + 1)
            else:
                ops.tab_sgd_step_(bufs[0], bufs[1], bufs[2], chunks_dev, hyper_dev[t], one, momentum, None, t == 0,
                                  write_back_grad=False)
            t += 1
    ops.probe_sweep_score(feat, labels, w, b, val_dev, mean, inv_std, out=(val[0], val[1].view(torch.int32)))
    val = val.cpu()                                                               # the one host read
    return SweepResult(grid, val[1].view(torch.int32).clone(), val[0].clone(), loss_log, hit_log, w, b, mean, inv_std, train_idx,
                       val_idx, bounds)


def select(result) -> int:
    """The winning head of a sweep: most validation hits, then the lower validation loss (a NaN loss loses to any number), then
    the lower head index.  Reads result.val_hits and result.val_loss only."""
    hits = [int(h) for h in result.val_hits]
    loss = [float(v) for v in result.val_loss]
    loss = [float("inf") if v != v else v for v in loss]
    return min(range(len(hits)), key=lambda g: (-hits[g], loss[g], g))


def evaluate(model, gallery_loader, query_loader, n_classes: int, lrs: Optional[Sequence[float]] = None,
             wds: Optional[Sequence[float]] = None, val_fraction: Optional[float] = None, **fit_args) -> dict:
    """Features of both loaders (one whole video per item), the fit on the gallery, top-1 / top-5 of the queries.  The model runs
    in eval mode under no_grad and comes back in the mode it went in with (as knn.evaluate).  With ``lrs`` (and optionally ``wds``,
    default [weight_decay], and ``val_fraction``, default 0.2) the learning rate and weight decay of the fit are first selected by
    sweep() / select() on a hold-out of the GALLERY; the fit itself, on the whole gallery, and the scoring are the same statements,
    and the result gains ``sweep`` (per grid point: lr, wd, val_top1, val_loss, last_epoch_loss), ``selected_lr``,
    ``selected_wd``, ``val_fraction`` and ``n_val``."""
    if lrs is None and (wds is not None or val_fraction is not None):
        raise ValueError("probe.evaluate: wds / val_fraction select nothing without lrs")
    if lrs is not None:
        grid_points(lrs, wds if wds is not None else [fit_args.get("weight_decay", DEFAULT_WD)])       # refused before any device work
    net = retrieval._inner(model)
    was_outer, was_inner = model.training, net.training
    try:
        g_feat, g_labels = retrieval.extract_features(model, gallery_loader)
        q_feat, q_labels = retrieval.extract_features(model, query_loader)
    finally:
        model.train(was_outer)
        if net is not model:
            net.train(was_inner)
    extra = {}
    if lrs is not None:
        fit_args, extra = _select_fit_args(g_feat, g_labels, n_classes, lrs, wds, val_fraction, fit_args)
    res = fit(g_feat, g_labels, n_classes, **fit_args)
    pred, _ = predict(res, q_feat, DEFAULT_TOP)
    acc = knn.accuracy(pred, q_labels, (1, 5))
    n = int(g_feat.shape[0])
    loss, train_acc = epoch_means(res, n)
    out = {"top1": acc[1], "top5": acc[5], "train_top1": float(train_acc[-1]), "first_loss": float(res.loss_log[0]),
           "last_epoch_loss": float(loss[-1]), "n_query": int(q_feat.shape[0]), "n_gallery": n,
           "feature_dim": int(g_feat.shape[1]), "n_classes": int(n_classes),
           "epochs": int(fit_args.get("epochs", DEFAULT_EPOCHS)), "batch": int(fit_args.get("batch", DEFAULT_BATCH)),
           "lr": float(fit_args.get("lr", DEFAULT_LR)), "weight_decay": float(fit_args.get("weight_decay", DEFAULT_WD)),
           "optimizer": str(fit_args.get("optimizer", DEFAULT_OPTIMIZER))}
    out.update(extra)
    return out


def _select_fit_args(g_feat, g_labels, n_classes, lrs, wds, val_fraction, fit_args):
    """evaluate's sweep: -> (fit_args at the selected lr / weight decay, the result keys the sweep adds)."""
    wds = list(wds) if wds is not None else [fit_args.get("weight_decay", DEFAULT_WD)]
    frac = DEFAULT_VAL_FRACTION if val_fraction is None else float(val_fraction)
    shared = {k: fit_args[k] for k in ("epochs", "batch", "optimizer", "momentum", "seed") if k in fit_args}
    sw = sweep(g_feat, g_labels, n_classes, lrs, wds, frac, **shared)
    best = select(sw)
    n_val, n_train = int(sw.val_idx.size), int(sw.train_idx.size)
    sizes = torch.tensor([hi - lo for lo, hi in sw.batch_bounds], dtype=torch.float64)
    last = (sw.loss_log[-sizes.numel():].cpu().to(torch.float64) * sizes[:, None]).sum(dim=0) / n_train
    points = [{"lr": lr, "wd": wd, "val_top1": int(sw.val_hits[g]) / n_val, "val_loss": float(sw.val_loss[g]),
               "last_epoch_loss": float(last[g])} for g, (lr, wd) in enumerate(sw.grid)]
    lr, wd = sw.grid[best]
    return dict(fit_args, lr=lr, weight_decay=wd), {"sweep": points, "selected_lr": lr, "selected_wd": wd, "val_fraction": frac,
                                                    "n_val": n_val}

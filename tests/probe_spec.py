"""The fp64 specification of the linear-probe kernels (include/cstp_hip.h: cstp_probe_step, cstp_probe_predict), the inputs of the
GPU cases and the tolerances, shared by tests/test_probe_host.py and tests/test_probe_gpu.py.

Tolerances.  The yardstick is this fp64 spec; the margin is taken over the error that a plain numpy-fp32 evaluation of the same
spec has on the same inputs (the kernel is such an evaluation with the sums in another order).  That restatement had logit errors
up to 3.9 * 2^-24 * B_r (B_r = max_c sum_k |xs_rk| |w_ck| + |b_c|, the magnitude the row's logits are summed from), loss errors
<= 1.5e-7 relative and dW / db errors <= 4.7e-7 of the tensor's largest magnitude:
  LOGIT_TOL_ULPS = 16       a logit may differ from the spec by 16 * 2^-24 * B_r
  LOSS_RTOL      = 6e-7     4 x the restatement's relative loss error
  GRAD_RTOL      = 1.9e-6   4 x the restatement's gradient error, of the tensor's max-abs
Measured on an MI355X (tests/test_probe_gpu.py prints them; MEASURED below): the kernels' logits are within 3.97 * 2^-24 * B_r,
the loss within 3.96e-7 relative (the one-row batch (1, 5, 8, 2) without standardisation; <= 4.5e-8 on every other case) and the
gradients within 1.6e-6 of max-abs ((33, 40, 2048, 101) without standardisation, where the raw features' offsets make B_r large;
<= 4.7e-7 on every other case).  Nothing was widened.
Two logits of a row are a NEAR TIE when they differ by at most 2 * LOGIT_TOL_ULPS * 2^-24 * B_r: their order is not decided at
the tolerance.  A (row, rank) pair touched by a near tie is left out of the class comparison; a row whose top-1 is a near tie
may differ in ``hits``.  MAX_NEAR_TIE_SHARE caps how many pairs may be left out: a condition on the inputs, asserted from the
spec alone by the host test on exactly the inputs the GPU test uses.
"""
import math

import numpy as np

LOGIT_TOL_ULPS = 16
LOSS_RTOL = 6e-7
GRAD_RTOL = 1.9e-6
MAX_NEAR_TIE_SHARE = 0.02
ULP = 2.0 ** -24
# the largest errors over STEP_CASES x {standardised, raw}, n_top in (1, 5), on an MI355X
MEASURED = {"logit_ulps": 3.97, "loss_rel": 3.96e-7, "grad_rel": 1.6e-6}

# (m, n, d, c, rows): rows False = the whole matrix in order (rows=None, m == n), True = a gathered permutation prefix
STEP_CASES = [(70, 70, 24, 10, False),
              (70, 300, 23, 3, True),            # odd d, a gathered permutation prefix, m not a slab multiple
              (1, 5, 8, 2, True),
              (130, 130, 512, 101, False),       # more classes than lanes
              (33, 40, 2048, 101, True),
              (257, 1000, 100, 400, True),       # four class tiles, two row slices
              (64, 64, 4, 65, False)]            # d smaller than any tile


def make_case(m, n, d, c, rows, seed=0):
    """Standard-normal features with a per-dimension scale and shift, W ~ N(0, 1 / d), b ~ 0.1 N(0, 1), labels uniform; mean and
    inv_std are the features' own per-dimension statistics (fp64, rounded to fp32).  All fp32 / int64 / int32 numpy arrays."""
    rs = np.random.RandomState(1000 * seed + 7 * m + 3 * d + c)
    scale = rs.uniform(0.5, 2.0, size=d)
    shift = rs.standard_normal(d)
    x = (rs.standard_normal((n, d)) * scale + shift).astype(np.float32)
    w = (rs.standard_normal((c, d)) / np.sqrt(d)).astype(np.float32)
    b = (0.1 * rs.standard_normal(c)).astype(np.float32)
    labels = rs.randint(0, c, size=n).astype(np.int64)
    x64 = x.astype(np.float64)
    mean = x64.mean(axis=0)
    var = ((x64 - mean) ** 2).mean(axis=0)
    inv_std = np.where(var > 0, 1.0 / np.sqrt(np.where(var > 0, var, 1.0)), 0.0)
    idx = rs.permutation(n)[:m].astype(np.int32) if rows else None
    return {"x": x, "w": w, "b": b, "labels": labels, "mean": mean.astype(np.float32), "inv_std": inv_std.astype(np.float32),
            "rows": idx, "m": m, "n": n, "d": d, "c": c}


def _standardised(x, mean, inv_std):
    xs = np.asarray(x, dtype=np.float64)
    if mean is not None:
        xs = xs - np.asarray(mean, dtype=np.float64)
    if inv_std is not None:
        xs = xs * np.asarray(inv_std, dtype=np.float64)
    return xs


def _logits(xs, w, b):
    w, b = np.asarray(w, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return xs @ w.T + b, (np.abs(xs) @ np.abs(w).T + np.abs(b)).max(axis=1)


def step_ref(x, labels, w, b, rows=None, mean=None, inv_std=None, tol_ulps=LOGIT_TOL_ULPS):
    """-> dict(loss, hits, dw [c, d], db [c], bound [m] = B_r, near_top1 [m] bool, logits [m, c]) in fp64.  A row index outside
    [0, n) or a label outside [0, c) contributes nothing to loss, gradients and hits; the row still counts in m."""
    n, d = np.shape(x)
    c = np.shape(w)[0]
    labels = np.asarray(labels, dtype=np.int64)
    idx = np.arange(n, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    m = idx.shape[0]
    row_ok = (idx >= 0) & (idx < n)
    safe = np.where(row_ok, idx, 0)
    xs = _standardised(x, mean, inv_std)[safe] * row_ok[:, None]
    logits, bound = _logits(xs, w, b)
    y = np.where(row_ok, labels[safe], -1)
    ok = row_ok & (y >= 0) & (y < c)
    ys = np.where(ok, y, 0)
    mx = logits.max(axis=1, keepdims=True)
    e = np.exp(logits - mx)
    se = e.sum(axis=1, keepdims=True)
    lse = (np.log(se) + mx)[:, 0]
    row_loss = np.where(ok, lse - logits[np.arange(m), ys], 0.0)
    onehot = np.zeros((m, c))
    onehot[np.arange(m), ys] = 1.0
    g = (e / se - onehot) * ok[:, None] / m
    srt = np.sort(logits, axis=1)
    near = ok & ((srt[:, -1] - srt[:, -2]) <= 2 * tol_ulps * ULP * bound)
    return {"loss": row_loss.sum() / m, "hits": int((ok & (logits.argmax(axis=1) == ys)).sum()), "dw": g.T @ xs, "db": g.sum(axis=0),
            "bound": bound, "near_top1": near, "logits": logits}


def predict_ref(x, w, b, mean=None, inv_std=None, n_top=5, tol_ulps=LOGIT_TOL_ULPS):
    """-> (classes [n, n_top] int64, logits [n, n_top] fp64, near [n, n_top] bool, bound [n]): the n_top best classes by (logit
    descending, class id ascending); (-1, 0.0) where n_top > c.  near marks the ranks whose logit is within the near-tie band of
    a neighbouring rank's (the first rank cut off included)."""
    logits, bound = _logits(_standardised(x, mean, inv_std), w, b)
    n, c = logits.shape
    order = np.argsort(-logits, axis=1, kind="stable")
    srt = np.take_along_axis(logits, order, axis=1)
    band = (2 * tol_ulps * ULP * bound)[:, None]
    close = (srt[:, :-1] - srt[:, 1:]) <= band                        # rank j and rank j + 1
    touched = np.zeros((n, c), dtype=bool)
    touched[:, :-1] |= close
    touched[:, 1:] |= close
    classes = np.full((n, n_top), -1, dtype=np.int64)
    scores = np.zeros((n, n_top))
    near = np.zeros((n, n_top), dtype=bool)
    k = min(n_top, c)
    classes[:, :k], scores[:, :k], near[:, :k] = order[:, :k], srt[:, :k], touched[:, :k]
    return classes, scores, near, bound


def make_clusters(n, d, c, sep, seed=0):
    """n rows in c unit-variance Gaussian clusters of d >= c dimensions whose centres lie ``sep`` standard deviations apart
    (centre k = sep / sqrt(2) along axis k), a shift and a scale per dimension on top -> (features fp32 [n, d], labels int64 [n])
    as torch CPU tensors."""
    import torch
    rs = np.random.RandomState(77 + seed)
    labels = rs.randint(0, c, size=n)
    centres = np.zeros((c, d))
    centres[np.arange(c), np.arange(c)] = sep / np.sqrt(2.0)
    x = (centres[labels] + rs.standard_normal((n, d))) * rs.uniform(0.5, 2.0, size=d) + rs.standard_normal(d)
    return torch.from_numpy(x.astype(np.float32)), torch.from_numpy(labels.astype(np.int64))


def fit_ref(feat, labels, c, epochs, batch, lr, weight_decay=0.0, optimizer="sgd", momentum=0.9, seed=0, dtype=None):
    """cstp_amd.probe.fit restated on the CPU in ``dtype`` (default fp64) from the same plan(): -> (w, b, loss_log, hit_log, mean,
    inv_std, batch_bounds).  The arithmetic of the update kernels as include/cstp_hip.h states it (cstp_sgd_step, cstp_adam_step
    with decoupled = 1); the learning rates are the fp32 values the kernels read."""
    import torch
    from cstp_amd.probe import ADAM_BETAS, ADAM_EPS, plan, standardize
    dtype = dtype or torch.float64
    n, d = feat.shape
    perm, lrs, bounds = plan(n, epochs, batch, lr, seed)
    mean, inv_std = standardize(feat)
    xs = (feat.to(dtype) - mean.to(dtype)) * inv_std.to(dtype)
    w, b = torch.zeros((c, d), dtype=dtype), torch.zeros(c, dtype=dtype)
    state = [[torch.zeros_like(w), torch.zeros_like(w)], [torch.zeros_like(b), torch.zeros_like(b)]]
    loss_log, hit_log = [], []
    t = 0
    for e in range(epochs):
        for lo, hi in bounds:
            idx = perm[e, lo:hi].long() if batch != 0 else torch.arange(n)
            xb, y = xs[idx], labels[idx]
            m = idx.numel()
            logits = xb @ w.T + b
            mx = logits.max(dim=1, keepdim=True).values
            ex = torch.exp(logits - mx)
            se = ex.sum(dim=1, keepdim=True)
            loss_log.append(float(((torch.log(se) + mx)[:, 0] - logits[torch.arange(m), y]).sum() / m))
            hit_log.append(int((logits.argmax(dim=1) == y).sum()))
            g = ex / se
            g[torch.arange(m), y] -= 1.0
            g = g / m
            step_lr = lrs[t].to(dtype)
            for p, grad, st, wd in ((w, g.T @ xb, state[0], weight_decay), (b, g.sum(dim=0), state[1], 0.0)):
                if optimizer == "sgd":
                    grad = grad + wd * p
                    st[0].copy_(grad if t == 0 else momentum * st[0] + grad)
                    p -= step_lr * st[0]
                else:
                    p *= 1.0 - step_lr * wd
                    st[0].copy_(ADAM_BETAS[0] * st[0] + (1.0 - ADAM_BETAS[0]) * grad)
                    st[1].copy_(ADAM_BETAS[1] * st[1] + (1.0 - ADAM_BETAS[1]) * grad * grad)
                    c1, c2 = 1.0 - ADAM_BETAS[0] ** (t + 1), 1.0 - ADAM_BETAS[1] ** (t + 1)
                    p -= step_lr / c1 * st[0] / (torch.sqrt(st[1]) / math.sqrt(c2) + ADAM_EPS)
            t += 1
    return w, b, np.array(loss_log), np.array(hit_log), mean, inv_std, bounds

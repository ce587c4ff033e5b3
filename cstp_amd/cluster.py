"""k-means clustering evaluation on cached features: what an encoder has learnt, measured without any label in the answer.

The features of the videos (retrieval.extract_features) are L2-normalised and clustered by spherical k-means: a row belongs to the
centroid with the largest dot product, a centroid is the normalised sum of its rows.  Several restarts run side by side, the
restart being a grid dimension of the kernels: ops.kmeans_assign streams every restart's centroids past the rows on the f32 MFMA
(no [n, k] table, the bits of ops.sim_topk), ops.kmeans_update adds every cluster's rows in ascending row order (csrc/kmeans.h).
No atomics, so a fit is a function of its arguments bit for bit, and nothing is read back inside the loop: ``moved`` and ``score``
of every iteration land in device logs that are read once at the end.  The partition is then scored against the labels by NMI,
ARI, purity and Hungarian-matched accuracy -- plain fp64 functions of the contingency table.  Serves the cluster.py driver.
"""
from __future__ import annotations

from typing import NamedTuple, Tuple

import numpy as np
import torch

from . import ops, retrieval

DEFAULT_ITERS, DEFAULT_RESTARTS = 50, 10
MAX_RESTARTS = ops.KMEANS_MAX_RESTARTS


class ClusterResult(NamedTuple):
    cent: torch.Tensor            # [k, d] fp32, device: the winning restart's centroids (unit rows)
    assign: torch.Tensor          # [n] int32, device: every row's cluster under ``cent``
    counts: torch.Tensor          # [k] int64, device: the clusters' sizes under ``assign``
    score: float                  # sum_i <x_i, cent[assign_i]> of the winner (fp64)
    restart: int                  # the winner: the highest final score, the lower index among equal ones
    final_scores: torch.Tensor    # [restarts] fp64, CPU: every restart's score under its last centroids
    score_log: torch.Tensor       # [iters, restarts] fp64, CPU: the score of the centroids iteration t STARTED from
    moved_log: torch.Tensor       # [iters, restarts] int32, CPU: rows whose cluster changed in iteration t (n in iteration 0)
    converged_at: torch.Tensor    # [restarts] int64, CPU: the first iteration with moved == 0, or -1


def plan(n: int, c: int, restarts: int, seed: int) -> torch.Tensor:
    """The draws of a fit's seeding, a pure function of its arguments -> u [restarts, c] fp64 (CPU), uniform in [0, 1): restart
    s draws from a private CPU generator seeded by (seed, s).  u[s, 0] picks the first centre, u[s, j] the j-th (init_pp)."""
    n, c, restarts = int(n), int(c), int(restarts)
    if n < 1 or c < 1 or c > n or not 1 <= restarts <= MAX_RESTARTS:
        raise ValueError("plan: 1 <= c <= n and restarts in 1..%d are required, got n = %d, c = %d, restarts = %d"
                         % (MAX_RESTARTS, n, c, restarts))
    u = torch.empty((restarts, c), dtype=torch.float64)
    gen = torch.Generator(device="cpu")
    for s in range(restarts):
        gen.manual_seed((int(seed) * 1000003 + s) % (1 << 63))
        u[s] = torch.rand(c, generator=gen, dtype=torch.float64)
    return u


def init_pp(x: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """k-means++ seeding (Arthur & Vassilvitskii 2007) of all restarts on x's device -> cent [restarts, c, d] fp32, rows of x.
    x [n, d] has unit rows, so 1 - <a, b> is half the squared distance: the first centre of restart s is row floor(u[s, 0] * n);
    every further one is drawn with probability proportional to the row's 1 - sim to its nearest centre so far.  Per step one
    [restarts, n] product, a running minimum, an fp64 cumsum and a searchsorted against u[s, j] * total.  Plain tensor ops: this
    runs once per fit and is NOT a hot path (c small products next to iters * restarts assignments).  It reads nothing back on
    the host and draws from no global generator: the only randomness is ``u`` (plan)."""
    if x.dim() != 2 or u.dim() != 2:
        raise ValueError("init_pp: x must be [rows, features] and u [restarts, clusters], got %s and %s" % (tuple(x.shape), tuple(u.shape)))
    n = x.shape[0]
    r, c = u.shape
    if c > n:
        raise ValueError("init_pp: %d clusters for %d rows" % (c, n))
    u = u.to(device=x.device, dtype=torch.float64)
    first = torch.clamp((u[:, 0] * n).to(torch.int64), max=n - 1)                 # [r]
    picks = [first]
    col = torch.arange(r, device=x.device)
    zero = torch.zeros((), dtype=torch.float64, device=x.device)
    xt = x.T                                                                      # a view: the product reads x as it lies
    mind = torch.clamp(1.0 - x[first] @ xt, min=0.0)                              # [r, n]: the scan below runs along a row
    mind[col, first] = 0.0                                                        # a centre is never drawn again, whatever 1 - <x, x> rounds to
    for j in range(1, c):
        cs = torch.cumsum(mind.to(torch.float64), dim=1)
        total = cs[:, -1]
        target = torch.minimum(u[:, j] * total, torch.nextafter(total, zero)).reshape(r, 1)   # < total: a row of positive weight
        idx = torch.clamp(torch.searchsorted(cs, target, right=True).reshape(r), max=n - 1)   # the first row with cs > target
        picks.append(idx)
        mind = torch.minimum(mind, torch.clamp(1.0 - x[idx] @ xt, min=0.0))
        mind[col, idx] = 0.0
    return x[torch.stack(picks, dim=1)].contiguous()                             # [r, c, d]


def fit(feat: torch.Tensor, k: int, iters: int = DEFAULT_ITERS, restarts: int = DEFAULT_RESTARTS, seed: int = 0,
        init: torch.Tensor = None) -> ClusterResult:
    """Spherical k-means of feat [n, d] fp32 (a device tensor) into k clusters: exactly ``iters`` rounds of assign + update for
    all restarts at once, one more assign under the last centroids, the restart with the highest final score wins (the lower
    index among equal scores).  ``init`` [restarts, k, d]: start from these centroids instead of init_pp(plan(...))."""
    k, iters, restarts = int(k), int(iters), int(restarts)
    if feat.dim() != 2:
        raise ValueError("cluster features must be [rows, features], got %s" % (tuple(feat.shape),))
    n, d = feat.shape
    if iters < 1 or not 1 <= restarts <= MAX_RESTARTS or k < 1 or k > n:
        raise ValueError("cluster: iters >= 1, restarts in 1..%d and 1 <= k <= rows are required, got iters = %d, restarts = %d, "
                         "k = %d, rows = %d" % (MAX_RESTARTS, iters, restarts, k, n))
    u = plan(n, k, restarts, seed) if init is None else None
    dev = feat.device
    with torch.no_grad():
        x = ops.l2_normalize(feat.detach().to(torch.float32).contiguous())
        cent = [init_pp(x, u) if init is None else init.to(torch.float32).contiguous().clone(), None]
        if tuple(cent[0].shape) != (restarts, k, d):
            raise ValueError("cluster: init must be %s, got %s" % ((restarts, k, d), tuple(cent[0].shape)))
        cent[1] = torch.empty_like(cent[0])                                       # ping-pong: update never writes what it reads
        assign = [torch.empty((restarts, n), dtype=torch.int32, device=dev) for _ in range(2)]
        best = torch.empty((restarts, n), dtype=torch.float32, device=dev)
        counts = torch.empty((restarts, k), dtype=torch.int32, device=dev)
        moved_log = torch.zeros((iters + 1, restarts), dtype=torch.int32, device=dev)
        score_log = torch.zeros((iters + 1, restarts), dtype=torch.float64, device=dev)
        for t in range(iters + 1):                                                # round ``iters`` only scores the last centroids
            a, b = t % 2, (t + 1) % 2
            ops.kmeans_assign(x, cent[a], assign[b] if t > 0 else None, out=(assign[a], best, moved_log[t], score_log[t]))
            if t < iters:
                ops.kmeans_update(x, assign[a], cent[a], out=(cent[b], counts))
        moved_log, score_log = moved_log.cpu(), score_log.cpu()                   # the one host read
        final = score_log[iters]
        win = max(range(restarts), key=lambda s: (float(final[s]), -s))
        last = iters % 2
        win_assign = assign[last][win].clone()
        win_counts = torch.bincount(win_assign.to(torch.int64).clamp(min=0), minlength=k)
    fixed = moved_log[:iters] == 0
    converged_at = torch.where(fixed.any(dim=0), fixed.to(torch.int64).argmax(dim=0), torch.full((restarts,), -1, dtype=torch.int64))
    return ClusterResult(cent[last][win].clone(), win_assign, win_counts, float(final[win]), int(win), final.clone(),
                         score_log[:iters].clone(), moved_log[:iters].clone(), converged_at)


def predict(result: ClusterResult, feat: torch.Tensor) -> torch.Tensor:
    """-> assign [n] int32: the cluster of every row of feat [n, d] under the fitted centroids; one kmeans_assign."""
    with torch.no_grad():
        x = ops.l2_normalize(feat.detach().to(torch.float32).contiguous())
        return ops.kmeans_assign(x, result.cent.unsqueeze(0).contiguous())[0][0]


def contingency(pred: torch.Tensor, labels: torch.Tensor, k: int, n_classes: int) -> torch.Tensor:
    """-> table [k, n_classes] int64 on pred's device: table[a, b] = rows with cluster a and label b, exact counts by
    torch.bincount.  Rows whose cluster lies outside 0..k-1 or whose label lies outside 0..n_classes-1 are left out."""
    k, n_classes = int(k), int(n_classes)
    if pred.dim() != 1 or labels.dim() != 1 or pred.shape[0] != labels.shape[0] or k < 1 or n_classes < 1:
        raise ValueError("contingency: pred %s and labels %s must be vectors of one length, k and n_classes >= 1"
                         % (tuple(pred.shape), tuple(labels.shape)))
    p = pred.to(torch.int64)
    y = labels.to(device=p.device, dtype=torch.int64)
    ok = (p >= 0) & (p < k) & (y >= 0) & (y < n_classes)
    return torch.bincount((p * n_classes + y)[ok], minlength=k * n_classes).reshape(k, n_classes)


def _table(table) -> np.ndarray:
    t = table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
    if t.ndim != 2 or t.size == 0 or (t < 0).any():
        raise ValueError("a contingency table is a non-empty 2-D array of counts, got shape %s" % (t.shape,))
    return t.astype(np.float64)


def _entropy(counts: np.ndarray) -> float:
    p = counts[counts > 0] / counts.sum()
    return float(-(p * np.log(p)).sum())


def nmi(table) -> float:
    """Normalised mutual information of the two partitions, natural log, normalised by the arithmetic mean of the entropies;
    1.0 when both partitions are a single cluster (both entropies 0), 0.0 for an empty table."""
    t = _table(table)
    n = t.sum()
    if n <= 0:
        return 0.0
    a, b = t.sum(axis=1), t.sum(axis=0)
    ha, hb = _entropy(a), _entropy(b)
    if ha == 0.0 and hb == 0.0:
        return 1.0
    nz = t > 0
    outer = np.outer(a, b)
    mi = float((t[nz] / n * (np.log(t[nz]) + np.log(n) - np.log(outer[nz]))).sum())
    return min(1.0, max(0.0, mi / (0.5 * (ha + hb))))


def ari(table) -> float:
    """Adjusted Rand index (Hubert & Arabie 1985); 1.0 where the adjustment's denominator vanishes (both partitions trivial)."""
    t = _table(table)
    n = t.sum()
    pairs = lambda v: float((v * (v - 1.0) / 2.0).sum())
    total = n * (n - 1.0) / 2.0
    if total <= 0:
        return 1.0
    sij, sa, sb = pairs(t), pairs(t.sum(axis=1)), pairs(t.sum(axis=0))
    expected = sa * sb / total
    denom = 0.5 * (sa + sb) - expected
    return 1.0 if denom == 0.0 else (sij - expected) / denom


def purity(table) -> float:
    """The share of rows that carry their cluster's most frequent label."""
    t = _table(table)
    n = t.sum()
    return float(t.max(axis=1).sum() / n) if n > 0 else 0.0


def hungarian(cost) -> Tuple[np.ndarray, np.ndarray]:
    """Minimum-cost assignment (Kuhn-Munkres with potentials, O(k^3), numpy only) -> (rows, cols): min(shape) pairs, rows
    ascending, minimising cost[rows, cols].sum().  A rectangular matrix is padded to a square with zeros -- a constant row or
    column changes no choice among the real ones -- and the pairs that touch the padding are dropped."""
    c = np.asarray(cost, dtype=np.float64)
    if c.ndim != 2 or c.size == 0 or not np.isfinite(c).all():
        raise ValueError("hungarian: a non-empty finite 2-D cost matrix is required, got shape %s" % (c.shape,))
    n0, m0 = c.shape
    k = max(n0, m0)
    sq = np.zeros((k, k))
    sq[:n0, :m0] = c
    u, v = np.zeros(k + 1), np.zeros(k + 1)
    p, way = np.zeros(k + 1, dtype=np.int64), np.zeros(k + 1, dtype=np.int64)     # p[j]: the row matched to column j (1-based)
    for i in range(1, k + 1):
        p[0] = i
        j0 = 0
        minv = np.full(k + 1, np.inf)
        used = np.zeros(k + 1, dtype=bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            cur = sq[i0 - 1] - u[i0] - v[1:]
            free = ~used[1:]
            upd = free & (cur < minv[1:])
            minv[1:][upd] = cur[upd]
            way[1:][upd] = j0
            cand = np.where(free, minv[1:], np.inf)
            j1 = int(np.argmin(cand)) + 1
            delta = cand[j1 - 1]
            u[p[used]] += delta
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0 != 0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    rows = p[1:] - 1
    cols = np.arange(k)
    keep = (rows < n0) & (cols < m0)
    rows, cols = rows[keep], cols[keep]
    order = np.argsort(rows, kind="stable")
    return rows[order], cols[order]


def matched_accuracy(table) -> float:
    """The accuracy under the best one-to-one matching of clusters to labels (hungarian on the negated table)."""
    t = _table(table)
    n = t.sum()
    if n <= 0:
        return 0.0
    rows, cols = hungarian(-t)
    return float(t[rows, cols].sum() / n)


def scores(table) -> dict:
    return {"nmi": nmi(table), "ari": ari(table), "purity": purity(table), "acc": matched_accuracy(table)}


def evaluate(model, gallery_loader, query_loader, k: int, iters: int = DEFAULT_ITERS, restarts: int = DEFAULT_RESTARTS,
             seed: int = 0) -> dict:
    """Features of both loaders (one whole video per item), the fit on the gallery (the train list), the scores of the gallery's
    partition, and those of the queries (the test list) assigned to the fitted centroids by one kmeans_assign.  The model runs in
    eval mode under no_grad and comes back in the mode it went in with (as knn.evaluate)."""
    net = retrieval._inner(model)
    was_outer, was_inner = model.training, net.training
    try:
        g_feat, g_labels = retrieval.extract_features(model, gallery_loader)
        q_feat, q_labels = retrieval.extract_features(model, query_loader)
    finally:
        model.train(was_outer)
        if net is not model:
            net.train(was_inner)
    res = fit(g_feat, k, iters, restarts, seed)
    n_classes = int(max(int(g_labels.max()), int(q_labels.max()))) + 1
    out = {"n_gallery": int(g_feat.shape[0]), "n_query": int(q_feat.shape[0]), "feature_dim": int(g_feat.shape[1]), "k": int(k),
           "n_classes": n_classes, "iters": int(iters), "restarts": int(restarts), "seed": int(seed), "restart": res.restart,
           "score": res.score, "converged_at": int(res.converged_at[res.restart]), "empty_clusters": int((res.counts == 0).sum())}
    for name, pred, labels in (("train", res.assign, g_labels), ("test", predict(res, q_feat), q_labels)):
        for key, value in scores(contingency(pred, labels, k, n_classes)).items():
            out["%s_%s" % (name, key)] = value
    return out

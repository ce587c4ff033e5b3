"""Weighted k-nearest-neighbour classification (InstDisc / DINO style): what an encoder has learnt, measured without training.

A query video takes the class that its k most similar gallery videos vote for.  Features are the per-video means of
``ByolBase.encode`` (retrieval.extract_features), L2-normalised; ops.sim_topk finds the k neighbours without the [queries x
gallery] matrix; ops.knn_vote (csrc/retrieve.hip) weighs neighbour j by exp((sim_j - sim_0) / temperature) -- the usual
exp(sim_j / temperature) divided by the row's largest weight, which changes no ranking and cannot overflow -- sums the weights per
class in slot order and returns the best classes by (score descending, class id ascending).  One launch, no [queries x classes]
table, no atomics.  Serves the knn.py driver and the --knn_every monitor of main_byol.py.
"""
from __future__ import annotations

from typing import Dict, Sequence

import torch

from . import ops, retrieval

DEFAULT_K, DEFAULT_T, DEFAULT_TOP = 20, 0.07, 5


def classify(q_feat: torch.Tensor, g_feat: torch.Tensor, g_labels: torch.Tensor, k: int = DEFAULT_K,
             temperature: float = DEFAULT_T, n_top: int = DEFAULT_TOP, exclude_self: bool = False):
    """-> (pred [nq, n_top] int32, score [nq, n_top] fp32, val [nq, k], idx [nq, k]): the n_top best classes of every query and
    the neighbour lists they were voted from; (-1, 0) where fewer than n_top classes occur among a query's neighbours.
    ``exclude_self``: the queries ARE the gallery (leave-one-out), a video never votes for itself."""
    qn, gn = ops.l2_normalize(q_feat), ops.l2_normalize(g_feat)
    val, idx = ops.sim_topk(qn, gn, k, exclude_self)
    pred, score = ops.knn_vote(val, idx, g_labels, temperature, n_top)
    return pred, score, val, idx


def accuracy(pred: torch.Tensor, q_labels: torch.Tensor, tops: Sequence[int] = (1, 5)) -> Dict[int, float]:
    """Top-n accuracy for every n of ``tops`` from pred [nq, n_top] (classes by rank, -1 where they ran out): the share of
    queries whose label is among the first n predictions.  Plain tensor ops; CPU or device tensors alike."""
    tops = [int(t) for t in tops]
    if pred.dim() != 2 or pred.shape[0] != q_labels.shape[0]:
        raise ValueError("pred %s does not match %d queries" % (tuple(pred.shape), q_labels.shape[0]))
    if not tops or min(tops) < 1 or max(tops) > pred.shape[1]:
        raise ValueError("tops %r must lie in 1..%d (the width of pred)" % (tops, pred.shape[1]))
    pred = pred.to(torch.int64)
    hit = (pred == q_labels.to(pred.device).to(torch.int64).reshape(-1, 1)) & (pred >= 0)
    return {t: float(hit[:, :t].any(dim=1).to(torch.float64).mean()) for t in tops}


def evaluate(model, gallery_loader, query_loader, k: int = DEFAULT_K, temperature: float = DEFAULT_T) -> dict:
    """Features of both loaders (one whole video per item), the vote, top-1 / top-5 -> {"top1", "top5", "n_query",
    "n_gallery", "feature_dim", "k", "temperature"}.  The model runs in eval mode under no_grad (running BatchNorm statistics,
    nothing updated, no random draw) and comes back in the mode it went in with."""
    net = retrieval._inner(model)
    was_outer, was_inner = model.training, net.training
    try:
        g_feat, g_labels = retrieval.extract_features(model, gallery_loader)
        q_feat, q_labels = retrieval.extract_features(model, query_loader)
    finally:
        model.train(was_outer)
        if net is not model:
            net.train(was_inner)
    pred, _, _, _ = classify(q_feat, g_feat, g_labels, k, temperature, DEFAULT_TOP)
    acc = accuracy(pred, q_labels, (1, 5))
    return {"top1": acc[1], "top5": acc[5], "n_query": int(q_feat.shape[0]), "n_gallery": int(g_feat.shape[0]),
            "feature_dim": int(q_feat.shape[1]), "k": int(k), "temperature": float(temperature)}

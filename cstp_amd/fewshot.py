"""Few-shot episodic evaluation: N-way K-shot accuracy of a frozen encoder, the protocol of the few-shot action-recognition
literature on UCF-101 and HMDB-51.

An EPISODE draws N classes, K labelled support videos per class from the train list and Q query videos per class from the test
list; a query takes the class whose prototype -- the sum of the class's K support features -- it is most similar to by cosine
(the nearest-centroid classifier, "ProtoNet with cosine", the usual baseline on frozen features).  The figure reported is the
mean accuracy over thousands of random episodes with its 95 % confidence interval.  Retrieval, k-NN, the linear probe and k-means
use every training label once; an episode uses N * K of them, which is what "label efficiency" means.

    sup_idx, qry_idx, classes = sample_episodes(s_labels, q_labels, n_way, max(shots), n_query, episodes, seed)   host, numpy
    hits = ops.fewshot_episodes(l2_normalize(s_feat), l2_normalize(q_feat), sup_idx, qry_idx, n_query, shots)     one launch

The shot counts of one call are NESTED: the K-shot prototype is the sum of the first K support columns of the same table, so
1-shot and 5-shot accuracy are paired on the same episodes, classes and queries.  ops.fewshot_episodes (csrc/fewshot.h) runs one
block per episode and stores one integer per episode and shot count; no [E, N (K + Q), d] gather exists.  Per shot count
``evaluate_features`` returns acc = mean_e hits / (N Q) and ci95 = 1.96 std / sqrt(E) (the population standard deviation over the
episodes, fp64 on the host).

The defaults (5-way, 1 and 5 shots, 15 queries per class, 10 000 episodes) are the literature's conventions.  They are not tuned
and no few-shot accuracy of a trained encoder on real data has been measured with this code.  Serves the fewshot.py driver.
"""
from __future__ import annotations

import math
from typing import Sequence

import numpy as np
import torch

from . import ops, retrieval

DEFAULT_WAY, DEFAULT_SHOTS, DEFAULT_QUERY, DEFAULT_EPISODES, DEFAULT_SEED = 5, (1, 5), 15, 10000, 0


def _rows_by_class(labels):
    lab = np.asarray(torch.as_tensor(labels).detach().cpu().numpy()).astype(np.int64).reshape(-1)
    order = np.argsort(lab, kind="stable")
    classes, start = np.unique(lab[order], return_index=True)
    return {int(c): order[a:b] for c, a, b in zip(classes, start, list(start[1:]) + [len(order)])}


def sample_episodes(sup_labels, qry_labels, n_way: int, max_shot: int, n_query: int, episodes: int, seed: int):
    """-> (sup_idx [E, N, max_shot], qry_idx [E, N, n_query], classes [E, N]) as CPU int32 tensors: rows of the support set, rows
    of the query set and the class ids behind the slots.  A class is ELIGIBLE with at least ``max_shot`` support videos and at
    least ``n_query`` query videos; the others are dropped with one printed line.  An episode draws its classes from the eligible
    ones without replacement, and each class's videos without replacement.  The draws come from a private
    numpy.random.default_rng(seed): equal arguments give equal tables, and no global generator is touched.  Fewer than ``n_way``
    eligible classes raise ValueError."""
    n_way, max_shot, n_query, episodes = int(n_way), int(max_shot), int(n_query), int(episodes)
    if n_way < 1 or max_shot < 1 or n_query < 1 or episodes < 1:
        raise ValueError("sample_episodes: n_way, max_shot, n_query and episodes must be at least 1, got %d, %d, %d, %d"
                         % (n_way, max_shot, n_query, episodes))
    sup, qry = _rows_by_class(sup_labels), _rows_by_class(qry_labels)
    every = sorted(set(sup) | set(qry))
    eligible = [c for c in every if len(sup.get(c, ())) >= max_shot and len(qry.get(c, ())) >= n_query]
    if len(eligible) < len(every):
        print("Few-shot sampler: dropped {} of {} classes with fewer than {} support or {} query videos".format(
            len(every) - len(eligible), len(every), max_shot, n_query))
    if len(eligible) < n_way:
        raise ValueError("sample_episodes: %d-way episodes need %d eligible classes, %d of %d have at least %d support and %d "
                         "query videos" % (n_way, n_way, len(eligible), len(every), max_shot, n_query))
    rng = np.random.default_rng(int(seed))
    sup_idx = np.empty((episodes, n_way, max_shot), dtype=np.int32)
    qry_idx = np.empty((episodes, n_way, n_query), dtype=np.int32)
    pool = np.asarray(eligible, dtype=np.int64)
    # a draw without replacement = the first entries of a uniformly random order = the smallest of independent uniform keys;
    # one key matrix for the classes of all episodes, then one per class and side for the (episode, slot) pairs that drew it
    picked = np.argsort(rng.random((episodes, len(pool))), axis=1, kind="stable")[:, :n_way]
    flat = picked.reshape(-1)
    order = np.argsort(flat, kind="stable")                # the (episode, slot) pairs of a class, in episode-major order
    bounds = np.searchsorted(flat[order], np.arange(len(pool) + 1))
    for i, c in enumerate(pool):
        ep, slot = np.divmod(order[bounds[i]:bounds[i + 1]], n_way)
        for rows, take, out in ((sup[int(c)], max_shot, sup_idx), (qry[int(c)], n_query, qry_idx)):
            keys = rng.random((len(ep), len(rows)))
            out[ep, slot] = rows[np.argsort(keys, axis=1, kind="stable")[:, :take]]
    classes = pool[picked].astype(np.int32)
    return torch.from_numpy(sup_idx), torch.from_numpy(qry_idx), torch.from_numpy(classes)


def accuracy_from_hits(hits, n_slots: int):
    """hits [S, E] (any integer tensor) -> ([acc per shot count], [ci95 per shot count]): the mean over the episodes of
    hits / n_slots and 1.96 * std / sqrt(E) with the population standard deviation, fp64 on the host."""
    h = torch.as_tensor(hits).detach().to("cpu", torch.float64)
    if h.dim() != 2 or h.shape[1] < 1:
        raise ValueError("accuracy_from_hits expects hits [shot counts, episodes], got %s" % (tuple(h.shape),))
    a = h / float(n_slots)
    mean = a.mean(dim=1)
    std = ((a - mean[:, None]) ** 2).mean(dim=1).sqrt()
    ci = 1.96 * std / math.sqrt(h.shape[1])
    return [float(v) for v in mean], [float(v) for v in ci]


def evaluate_features(s_feat: torch.Tensor, s_labels, q_feat: torch.Tensor, q_labels, n_way: int = DEFAULT_WAY,
                      shots: Sequence[int] = DEFAULT_SHOTS, n_query: int = DEFAULT_QUERY, episodes: int = DEFAULT_EPISODES,
                      seed: int = DEFAULT_SEED) -> dict:
    """Support features [ns, d] with their labels, query features [nq, d] with theirs (fp32 on a HIP device) -> {"acc": {k: ...},
    "ci95": {k: ...}, "n_way", "shots", "n_query", "episodes", "seed", "n_support", "n_queries", "feature_dim"}.  Normalises,
    samples the episodes on the host, calls ops.fewshot_episodes once and reads hits back once."""
    ks = ops.fewshot_shots([int(k) for k in shots])
    sup_idx, qry_idx, _ = sample_episodes(s_labels, q_labels, n_way, ks[-1], n_query, episodes, seed)
    xs, xq = ops.l2_normalize(s_feat), ops.l2_normalize(q_feat)
    hits = ops.fewshot_episodes(xs, xq, sup_idx, qry_idx, int(n_query), ks)
    acc, ci = accuracy_from_hits(hits.cpu(), int(n_way) * int(n_query))
    return {"acc": {k: a for k, a in zip(ks, acc)}, "ci95": {k: c for k, c in zip(ks, ci)}, "n_way": int(n_way), "shots": list(ks),
            "n_query": int(n_query), "episodes": int(episodes), "seed": int(seed), "n_support": int(s_feat.shape[0]),
            "n_queries": int(q_feat.shape[0]), "feature_dim": int(s_feat.shape[1])}


def evaluate(model, support_loader, query_loader, n_way: int = DEFAULT_WAY, shots: Sequence[int] = DEFAULT_SHOTS,
             n_query: int = DEFAULT_QUERY, episodes: int = DEFAULT_EPISODES, seed: int = DEFAULT_SEED) -> dict:
    """Features of both loaders (one whole video per item; the support loader reads the train list, the query loader the test
    list, as k-NN and the probe use them), then ``evaluate_features``.  The model runs in eval mode under no_grad and comes back
    in the mode it went in with."""
    net = retrieval._inner(model)
    was_outer, was_inner = model.training, net.training
    try:
        s_feat, s_labels = retrieval.extract_features(model, support_loader)
        q_feat, q_labels = retrieval.extract_features(model, query_loader)
    finally:
        model.train(was_outer)
        if net is not model:
            net.train(was_inner)
    return evaluate_features(s_feat, s_labels, q_feat, q_labels, n_way, shots, n_query, episodes, seed)


def format_line(res: dict, k: int) -> str:
    """``Few-shot 5-way 1-shot: 0.4321 ± 0.0045 (10000 episodes)``."""
    return "Few-shot {}-way {}-shot: {:.4f} ± {:.4f} ({} episodes)".format(res["n_way"], k, res["acc"][k], res["ci95"][k],
                                                                          res["episodes"])

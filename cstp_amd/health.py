"""Label-free collapse metrics: what a feature distribution looks like, measured without a single class label.

BYOL's characteristic failure is collapse -- the features shrink onto a point or onto a few directions while the loss keeps
falling -- and the other evaluations here (retrieval, k-NN, linear probe, clustering) all need labels to see it.  ``metrics``
takes features [n, d], L2-normalises the rows (ops.l2_normalize) and reduces them on the device with two kernels and one search:

    G, colsum = ops.feat_gram(x)                     G = x^T x and the column sums in fp64   (csrc/health.h)
    rowsum    = ops.pair_potential(x, t)             sum_{j != i} exp(2 t (s_ij - 1)) per row, no [n, n] matrix
    val, _    = ops.sim_topk(x, x, 1, exclude_self)  every row's best cosine to another row

Everything after that is fp64 host arithmetic on [d, d] and [n] results (``metrics_from_parts``; torch.linalg.eigvalsh on the
CPU).  With mu = colsum / n, C = G / n - mu mu^T and lambda(.) the eigenvalues clamped at 0:

    std_ratio   sqrt(d) * mean_k sqrt(max(C_kk, 0))            about 1 when isotropic on the sphere, 0 on collapse to a point
    erank       exp(-sum p log p), p = lambda(C) / sum lambda(C), zero terms skipped; 0.0 when tr C = 0: the effective rank of
                the centred covariance (Roy & Vetterli 2007)
    rankme      exp(-sum p log p), p = sigma / sum sigma + 1e-7, sigma = sqrt(lambda(G)): RankMe (Garrido et al. 2023) on the
                uncentred features
    top1_share  lambda_max(C) / tr C; 0.0 when tr C = 0: the share of the variance in one direction
    uniformity  log(sum_i rowsum_i / (n (n - 1))): Wang & Isola 2020, t = 2 by default; 0 on collapse to a point, more negative
                = more uniform
    nn_sim      the mean of every row's best cosine to another row: crowding

``rankme`` IS ILL-CONDITIONED WHEN G HAS ZERO EIGENVALUES (n < d, or true dimensional collapse): sigma = sqrt(lambda) turns an
eigenvalue error of 1e-16 * lambda_max into 1e-8 * sigma_max, which is the size of the 1e-7 offset, times the number of such
eigenvalues.  On a 129 x 512 rank-limited input an fp32 Gram instead of an fp64 one moves rankme by 8e-3 relative (CPU, measured)
and erank by 4e-6.  Read it where n >= d; ``erank`` is the robust one of the two.  Where the rows are identical up to rounding,
tr C is rounding noise rather than 0 and erank / top1_share describe that noise: std_ratio is the figure that reports
collapse to a point.

No effect on any accuracy is claimed for these figures and no run on real data exists; they are monitors.  Serves the health.py
driver and the --health_every monitor of main_byol.py.
"""
from __future__ import annotations

import math

import torch

from . import ops, retrieval

DEFAULT_T = 2.0
KEYS = ("std_ratio", "erank", "rankme", "top1_share", "uniformity", "nn_sim")
RANKME_EPS = 1e-7


def _entropy_rank(p: torch.Tensor) -> float:
    p = p[p > 0]
    return float(torch.exp(-(p * torch.log(p)).sum()))


def metrics_from_parts(gram, colsum, rowsum, nn_val, n: int, d: int, t: float = DEFAULT_T) -> dict:
    """The host half of ``metrics``: gram [d, d], colsum [d], rowsum [n] (ops.feat_gram / ops.pair_potential of the normalised
    rows, or any other computation of the same sums) and nn_val [n] (every row's best cosine to another row) -> the dict.
    fp64 on the CPU whatever comes in."""
    n, d = int(n), int(d)
    if n < 2:
        raise ValueError("health metrics need at least 2 rows, got %d" % n)
    g = gram.detach().to("cpu", torch.float64).reshape(d, d)
    s = colsum.detach().to("cpu", torch.float64).reshape(d)
    r = rowsum.detach().to("cpu", torch.float64).reshape(n)
    v = nn_val.detach().to("cpu", torch.float64).reshape(n)
    mu = s / n
    cov = g / n - torch.outer(mu, mu)
    std_ratio = math.sqrt(d) * float(torch.sqrt(torch.diagonal(cov).clamp_min(0.0)).mean())
    lam = torch.linalg.eigvalsh(cov).clamp_min(0.0)
    tr = float(lam.sum())
    if tr > 0.0:
        erank, top1_share = _entropy_rank(lam / tr), float(lam.max()) / tr
    else:
        erank, top1_share = 0.0, 0.0
    sigma = torch.sqrt(torch.linalg.eigvalsh(g).clamp_min(0.0))
    rankme = _entropy_rank(sigma / sigma.sum() + RANKME_EPS)
    uniformity = math.log(float(r.sum()) / (n * (n - 1.0)))
    return {"std_ratio": std_ratio, "erank": erank, "rankme": rankme, "top1_share": top1_share, "uniformity": uniformity,
            "nn_sim": float(v.mean()), "n": n, "d": d, "t": float(t)}


def metrics(feat: torch.Tensor, t: float = DEFAULT_T) -> dict:
    """feat [n, d] fp32 on a HIP device, n >= 2 -> {"std_ratio", "erank", "rankme", "top1_share", "uniformity", "nn_sim", "n",
    "d", "t"} (module docstring).  Four launches' worth of kernels and one host eigen-decomposition of two [d, d] matrices."""
    if feat.dim() != 2:
        raise ValueError("health metrics expect [rows, features], got %s" % (tuple(feat.shape),))
    n, d = feat.shape
    if n < 2:
        raise ValueError("health metrics need at least 2 rows, got %d" % n)
    x = ops.l2_normalize(feat)
    gram, colsum = ops.feat_gram(x)
    rowsum = ops.pair_potential(x, t)
    val, _ = ops.sim_topk(x, x, 1, True)
    return metrics_from_parts(gram, colsum, rowsum, val[:, 0], n, d, t)


def evaluate(model, loader, t: float = DEFAULT_T) -> dict:
    """Features of the loader's videos (retrieval.extract_features: one whole video per item, eval mode, no_grad), then
    ``metrics``.  The labels the loader carries are ignored.  The model comes back in the mode it went in with."""
    net = retrieval._inner(model)
    was_outer, was_inner = model.training, net.training
    try:
        feat, _ = retrieval.extract_features(model, loader)
    finally:
        model.train(was_outer)
        if net is not model:
            net.train(was_inner)
    return metrics(feat, t)


def format_line(res: dict) -> str:
    """``std_ratio = ...  erank = ...`` in the order of KEYS: the text behind ``Health train:`` / ``Health epoch N:``."""
    return "  ".join("{} = {:.4f}".format(k, res[k]) for k in KEYS)

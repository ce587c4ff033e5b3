"""The label-free collapse metrics restated in fp64 with plain torch on CPU tensors: the specification that cstp_amd.health is held
to.  It never imports the code under test.

``metrics_ref(feat, t)`` takes the fp32 features, widens them, normalises the rows in fp64 and follows the definitions:
mu = mean row, C = X^T X / n - mu mu^T, lambda(.) = eigenvalues clamped at 0,

    std_ratio   sqrt(d) * mean_k sqrt(max(C_kk, 0))
    erank       exp(-sum p log p), p = lambda(C) / sum lambda(C), zero terms skipped; 0.0 when tr C = 0
    rankme      exp(-sum p log p), p = sigma / sum sigma + 1e-7, sigma = sqrt(lambda(X^T X))
    top1_share  lambda_max(C) / tr C; 0.0 when tr C = 0
    uniformity  log(sum_{i != j} exp(2 t (s_ij - 1)) / (n (n - 1)))
    nn_sim      mean_i max_{j != i} s_ij

``gram_ref`` / ``pair_potential_ref`` are the two device reductions in fp64 on the input as given (the fp32-rounded values).
"""
import math

import torch


def make_features(n, d, rank, noise, seed):
    """Low rank plus noise plus a 0.5 offset, seeded: a @ b + noise * randn + 0.5, fp32 [n, d]."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(n, rank, generator=g, dtype=torch.float64)
    b = torch.randn(rank, d, generator=g, dtype=torch.float64)
    e = torch.randn(n, d, generator=g, dtype=torch.float64)
    return (a @ b + noise * e + 0.5).to(torch.float32)


def normalize_ref(feat):
    """Rows of unit length in fp64 (an all-zero row stays zero)."""
    x = feat.double()
    return x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)


def gram_ref(x):
    """x [n, d] (any float dtype) -> (X^T X [d, d], column sums [d]) in fp64."""
    x = x.double()
    return x.T @ x, x.sum(dim=0)


def pair_potential_ref(x, t):
    """x [n, d] -> rowsum [n] fp64: sum_{j != i} exp(2 t (s_ij - 1)), the diagonal left out by index."""
    x = x.double()
    e = torch.exp(2.0 * t * (x @ x.T - 1.0))
    e.fill_diagonal_(0.0)
    return e.sum(dim=1)


def nn_sim_ref(x):
    x = x.double()
    s = x @ x.T
    s.fill_diagonal_(float("-inf"))
    return s.max(dim=1).values


def _entropy_rank(p):
    p = p[p > 0]
    return float(torch.exp(-(p * torch.log(p)).sum()))


def metrics_from_sums_ref(gram, colsum, rowsum, nn_val, n, d, t):
    mu = colsum / n
    cov = gram / n - torch.outer(mu, mu)
    out = {"std_ratio": math.sqrt(d) * float(torch.sqrt(torch.diagonal(cov).clamp_min(0.0)).mean())}
    lam = torch.linalg.eigvalsh(cov).clamp_min(0.0)
    tr = float(lam.sum())
    out["erank"] = _entropy_rank(lam / tr) if tr > 0.0 else 0.0
    out["top1_share"] = float(lam.max()) / tr if tr > 0.0 else 0.0
    sigma = torch.sqrt(torch.linalg.eigvalsh(gram).clamp_min(0.0))
    out["rankme"] = _entropy_rank(sigma / sigma.sum() + 1e-7)
    out["uniformity"] = math.log(float(rowsum.sum()) / (n * (n - 1.0)))
    out["nn_sim"] = float(nn_val.mean())
    return out


def metrics_ref(feat, t=2.0):
    """fp32 features [n, d] -> the six figures, everything in fp64."""
    n, d = feat.shape
    x = normalize_ref(feat)
    gram, colsum = gram_ref(x)
    return metrics_from_sums_ref(gram, colsum, pair_potential_ref(x, t), nn_sim_ref(x), n, d, t)


def one_hot_rows(n=96, dirs=8, d=40):
    """n rows cycling through ``dirs`` one-hot directions in d dimensions: erank = dirs - 1, top1_share = 1 / (dirs - 1)."""
    x = torch.zeros(n, d, dtype=torch.float32)
    x[torch.arange(n), torch.arange(n) % dirs] = 1.0
    return x


def collapsed_rows(n=50, d=16):
    """n identical unit rows whose every product and sum is exact in fp32: (1/2, 1/2, 1/2, 1/2, 0, ...)."""
    x = torch.zeros(n, d, dtype=torch.float32)
    x[:, :4] = 0.5
    return x


ONE_HOT_ANSWERS = {"erank": 7.0, "top1_share": 1.0 / 7.0, "rankme": 8.0004, "std_ratio": 0.41833, "nn_sim": 1.0}
COLLAPSED_ANSWERS = {"std_ratio": 0.0, "erank": 0.0, "top1_share": 0.0, "uniformity": 0.0}

"""Specification of NT-Xent with a queue of extra negatives (ops.ntxent_queue, include/cstp_hip.h: cstp_ntxq_*), shared by
tests/test_ntxq_host.py (no GPU) and tests/test_ntxq_gpu.py (the HIP kernels).

    loss = 1/R sum_i [ -s_{i,(i+n) mod R} / T + log( sum_{j != i} exp(s_ij / T) + sum_{k < n_valid} exp(c_ik / T) ) ]

with the reference's cosine for s (reps against reps) and c (reps against queue rows).  ``ref`` is that formula in plain torch
with autograd and the upstream gradient DLOSS != 1; the kernels are held to BAR, the bar tests/ops_edge_cases.py uses for NT-Xent:
the global relative error (conftest.rel_err) of the loss and of dreps against the fp64 result.  The bar is a condition on the
cases, not a measurement: tests/test_ntxq_host.py checks that the fp32 evaluation of ``ref`` stays inside it on every case.
"""
import functools

import torch

BAR = 1e-4
DLOSS = 1.7

# (n, f, n_valid, cap, T, seed); R = 2n rows.
#   n: 2 = the smallest R, 3, 40 = two 64-row tiles of which the second is ragged
#   n_valid: 1, 127 / 128 / 129 around the 128-row queue tile, 300 = three tiles, 1100 = enough tiles for more than one split
#   f: 30 (no multiple of 4), 33 (no multiple of the 32-feature chunk), 128, 512 and 1024 (two and four backward slices),
#      2048 (the limit)
#   T: 0.5, 0.07, 0.01 (1/T = 100 passes 89, where exp overflows in fp32: every case holds a negative at cosine 1)
CASES = [
    (2, 30, 1, 8, 0.5, 1),
    (3, 33, 127, 128, 0.07, 2),
    (40, 128, 128, 300, 0.5, 3),
    (3, 512, 129, 300, 0.07, 4),
    (2, 1024, 300, 300, 0.01, 5),
    (40, 2048, 300, 384, 0.07, 6),
    (3, 128, 1100, 1100, 0.01, 7),
    (40, 33, 1100, 1280, 0.5, 8),
]
OVERFLOW_CASE = CASES[4]          # T = 0.01: the evaluation without max-subtraction leaves the bar here


def normalize(x):
    """x / max(|x|, 1e-8) per row, in x's dtype: what cstp_ntxq_push writes."""
    return x / x.norm(dim=1, keepdim=True).clamp_min(1e-8)


@functools.lru_cache(maxsize=None)
def inputs(n, f, n_valid, cap, seed):
    """reps [2n, f] fp32 randn and queue [cap, f] fp32 of unit rows; queue row 0 is reps row 1 normalised (a negative at cosine
    1 for that row); rows from n_valid on are zeros.  Never modified: clone before use."""
    g = torch.Generator().manual_seed(1000 + seed)
    reps = torch.randn((2 * n, f), generator=g).float()
    queue = normalize(torch.randn((cap, f), generator=g).float())
    queue[0] = normalize(reps[1:2])[0]
    queue[n_valid:] = 0
    return reps, queue


def ref(reps, queue, n_valid, T, dtype, naive=False):
    """{"loss", "dreps"} of the formula above by autograd, upstream gradient DLOSS.  naive: the same sums without subtracting the
    row maximum."""
    r = reps.detach().to(dtype).clone().requires_grad_(True)
    R = r.shape[0]
    n = R // 2
    nr = r.norm(dim=1, keepdim=True)
    s = (r @ r.t()) / torch.clamp(nr * nr.t(), min=1e-8) / T
    logits = s.masked_fill(torch.eye(R, dtype=torch.bool), float("-inf"))
    if n_valid > 0:
        q = queue[:n_valid].detach().to(dtype)
        c = (r @ q.t()) / torch.clamp(nr * q.norm(dim=1)[None, :], min=1e-8) / T
        logits = torch.cat([logits, c], dim=1)
    lse = torch.log(torch.exp(logits).sum(dim=1)) if naive else torch.logsumexp(logits, dim=1)
    idx = torch.arange(R)
    loss = (lse - s[idx, (idx + n) % R]).mean()
    (loss * DLOSS).backward()
    return {"loss": loss.detach(), "dreps": r.grad}


@functools.lru_cache(maxsize=None)
def case_ref(case):
    """The fp64 reference of a case, computed once."""
    n, f, n_valid, cap, T, seed = case
    reps, queue = inputs(n, f, n_valid, cap, seed)
    return ref(reps, queue, n_valid, T, torch.float64)


def errors(got, want):
    """name -> global relative error (max |got - want| / max |want|); NaN or inf anywhere in ``got`` gives inf."""
    out = {}
    for k, w in want.items():
        g = got[k].detach().double().cpu().reshape(w.shape)
        e = float((g - w).abs().max() / w.abs().max().clamp_min(1e-30))
        out[k] = e if e == e else float("inf")
    return out

"""The acceptance rule for a similarity top-k answer, shared by the host and the GPU tests of ops.sim_topk.

fp32 dot products of unit vectors carry an error of at most d * u * sum|q_c g_c| <= d * 2^-24; ``tau`` = d * 2^-23 is twice that.
Within tau of the k-th similarity the membership of the answer is free; everything else is pinned."""
import torch


def tau_for(d: int) -> float:
    return d * 2.0 ** -23


def unit_rows(n: int, d: int, seed: int) -> torch.Tensor:
    """[n, d] fp32 rows of unit length (CPU), a function of the seed."""
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn((n, d), generator=g, dtype=torch.float32), dim=1).contiguous()


def stable_reference(q: torch.Tensor, g: torch.Tensor, k: int, exclude_self: bool = False):
    """The fp32 answer whose tie order is the specification's: a STABLE descending sort of q @ g.T (torch.topk does not order ties
    by index).  -> (val [nq, k] fp32, idx [nq, k] int32), padded with (-inf, -1)."""
    s = q.float().cpu() @ g.float().cpu().T
    return _stable_from_scores(s, k, exclude_self)


def _stable_from_scores(s: torch.Tensor, k: int, exclude_self: bool):
    nq, ng = s.shape
    s = s.clone()
    if exclude_self:
        n = min(nq, ng)
        s[torch.arange(n), torch.arange(n)] = float("-inf")
    sv, si = torch.sort(s, dim=1, descending=True, stable=True)
    val = torch.full((nq, k), float("-inf"), dtype=s.dtype)
    idx = torch.full((nq, k), -1, dtype=torch.int32)
    m = min(k, ng)
    val[:, :m] = sv[:, :m]
    idx[:, :m] = si[:, :m].to(torch.int32)
    idx[val == float("-inf")] = -1                     # the excluded candidate (inputs are finite) sorted last: it is padding
    return val, idx


def check_topk(val, idx, q, g, k, exclude_self, tau):
    """Raises AssertionError unless (val, idx) is an acceptable answer for the k most similar rows of g per row of q."""
    val, idx = val.detach().cpu(), idx.detach().cpu().to(torch.int64)
    s = q.detach().double().cpu() @ g.detach().double().cpu().T
    nq, ng = s.shape
    assert tuple(val.shape) == (nq, k) and tuple(idx.shape) == (nq, k), (tuple(val.shape), tuple(idx.shape), (nq, k))
    assert val.dtype == torch.float32
    rows = torch.arange(nq).reshape(-1, 1)
    if exclude_self:
        assert not bool((idx == rows).any()), "a query retrieved itself"
        n = min(nq, ng)
        s[torch.arange(n), torch.arange(n)] = float("-inf")
        cand = torch.full((nq,), ng, dtype=torch.int64)
        cand[:n] -= 1
    else:
        cand = torch.full((nq,), ng, dtype=torch.int64)
    have = torch.clamp(cand, max=k)                                          # candidates each row must return
    slot = torch.arange(k).reshape(1, -1)
    live = slot < have.reshape(-1, 1)
    # padding exactly where the candidates run out
    assert bool(((idx >= 0) == live).all()), "index padding is not exactly where candidates run out"
    assert bool((idx[live] < ng).all()), "index out of range"
    assert bool((val[~live] == float("-inf")).all()) and bool(torch.isfinite(val[live]).all()), "value padding"
    if int(have.max()) == 0:
        return
    got = torch.where(live, s.gather(1, idx.clamp(min=0)), torch.zeros((), dtype=s.dtype))
    ssorted = torch.sort(s, dim=1, descending=True).values
    kth = ssorted.gather(1, (have - 1).clamp(min=0).reshape(-1, 1))          # the k-th largest (or the last candidate)
    assert bool((got >= kth - tau)[live].all()), "a returned row lies more than tau below the k-th similarity"
    must = s > kth + tau
    returned = torch.zeros((nq, ng + 1), dtype=torch.bool)
    returned.scatter_(1, torch.where(live, idx, torch.full_like(idx, ng)), True)
    assert not bool((must & ~returned[:, :ng]).any()), "a row more than tau above the k-th similarity is missing"
    assert bool(((val.double() - got).abs() <= tau)[live].all()), "val differs from the similarity of idx by more than tau"
    assert bool((val[:, 1:] <= val[:, :-1]).all()), "val increases along a row"
    bits = val.contiguous().view(torch.int32)
    tie = (bits[:, 1:] == bits[:, :-1]) & live[:, 1:]
    assert bool((idx[:, 1:] > idx[:, :-1])[tie].all()), "bit-equal similarities are not in ascending index order"
    srt = torch.sort(torch.where(live, idx, -1 - slot.expand(nq, k)), dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), "a gallery row is returned twice"

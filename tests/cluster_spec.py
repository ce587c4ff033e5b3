"""The fp64 specification of the k-means kernels (include/cstp_hip.h: cstp_kmeans_assign, cstp_kmeans_update) and of
cstp_amd.cluster.fit from given initial centroids, the inputs of the GPU cases and the tolerances, shared by
tests/test_cluster_host.py and tests/test_cluster_gpu.py.

Tolerances.
  assign: the kernel's (best, assign) must be the BITS of ops.sim_topk(x, cent[s], 1).  Against this fp64 spec a row may take
          another centroid only where the spec's two largest similarities lie within retrieval_spec.tau_for(d) = d * 2^-23 of each
          other (the tolerance tests/retrieval_spec.py uses for sim_topk: twice the error bound of an fp32 dot product of unit
          vectors); MAX_NEAR_TIE_SHARE caps the share of such rows -- a condition on the inputs, asserted from the spec alone by the
          host test on exactly the inputs the GPU test uses.
  update: the bound on |cent_out - spec| (rows of unit length, so absolute = relative to the row's norm) is UPDATE_MARGIN = 4 times
          the largest error that ``update_restated_fp32`` -- the documented summation order of csrc/kmeans.h restated in torch
          fp32 on the CPU -- has against the fp64 spec over CASES.  ``update_bound`` computes it; the host test pins the figure.
"""
import functools

import numpy as np

from retrieval_spec import tau_for

MAX_NEAR_TIE_SHARE = 0.02
UPDATE_MARGIN = 4.0

# (n, d, c, r): the smallest shapes at which the tiling can still go wrong
CASES = [(1, 1, 1, 1),
         (65, 33, 3, 2),            # ragged row tile (64 + 1) and feature chunk (32 + 1)
         (200, 512, 129, 1),        # crosses a 128-centroid tile
         (130, 7, 130, 1),          # c = n, d % 4 != 0: the scalar load path
         (600, 96, 10, 4)]


def _unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


@functools.lru_cache(maxsize=None)
def make_case(n, d, c, r, seed=0):
    """-> dict(x [n, d], cent [r, c, d], prev [r, n] int32): unit rows of standard-normal directions, rounded to fp32; prev is
    the spec's own assignment with every third row moved on by one cluster (so ``moved`` has a known answer up to near ties).
    Made once per argument tuple and shared: treat as read-only."""
    rs = np.random.RandomState(4000 * seed + 11 * n + 5 * d + 3 * c + r)
    x = _unit(rs.standard_normal((n, d))).astype(np.float32)
    cent = _unit(rs.standard_normal((r, c, d))).astype(np.float32)
    ref = assign_ref(x, cent)
    prev = ref["assign"].astype(np.int32).copy()
    prev[:, ::3] = (prev[:, ::3] + 1) % max(c, 2)           # c = 1: cluster 1 does not exist, a legal "no cluster" value
    for a in (x, cent, prev):
        a.setflags(write=False)
    return {"x": x, "cent": cent, "prev": prev, "n": n, "d": d, "c": c, "r": r}


def assign_ref(x, cent):
    """-> dict(assign [r, n] int64, best [r, n] fp64, gap [r, n] fp64, near [r, n] bool, score [r] fp64): the centroid of the
    largest fp64 dot product, the lowest id first; gap = the largest minus the second largest similarity (inf with one centroid);
    near = gap <= tau_for(d): the row's choice is not decided at fp32 precision."""
    x64, c64 = np.asarray(x, dtype=np.float64), np.asarray(cent, dtype=np.float64)
    sims = np.einsum("nd,rcd->rnc", x64, c64)
    assign = sims.argmax(axis=2)                            # numpy: the first maximum
    srt = np.sort(sims, axis=2)
    best = srt[:, :, -1]
    gap = best - srt[:, :, -2] if sims.shape[2] > 1 else np.full(best.shape, np.inf)
    return {"assign": assign, "best": best, "gap": gap, "near": gap <= tau_for(x64.shape[1]), "score": best.sum(axis=1), "sims": sims}


def update_ref(x, assign, cent):
    """-> (cent_new [r, c, d] fp64, counts [r, c] int64): the normalised fp64 sum of every cluster's rows; a cluster without rows
    (or whose sum is zero) keeps cent[s][j]; an assign value outside 0..c-1 belongs to no cluster."""
    x64, out = np.asarray(x, dtype=np.float64), np.asarray(cent, dtype=np.float64).copy()
    r, c, _ = out.shape
    counts = np.zeros((r, c), dtype=np.int64)
    for s in range(r):
        for j in range(c):
            rows = np.nonzero(np.asarray(assign[s]) == j)[0]
            counts[s, j] = rows.size
            if rows.size:
                total = x64[rows].sum(axis=0)
                norm = np.sqrt((total * total).sum())
                if norm > 0:
                    out[s, j] = total / norm
    return out, counts


def _tree64(v):
    """common.h wave_sum on 64 fp32 lanes (a torch fp32 vector): v[l] += v[l + off] for off = 32, 16, ..., 1 (lanes past the
    end add nothing)."""
    v = v.clone()
    off = 32
    while off:
        v[:64 - off] = v[:64 - off] + v[off:]
        off >>= 1
    return v[0]


def update_restated_fp32(x, assign, cent):
    """cstp_kmeans_update's documented order in torch fp32 on the CPU: per (cluster, feature) one chain over the cluster's rows
    ascending; |sum|^2 by thread t of 256 over f = t, t + 256, ..., the partials through the shuffle tree of each wave and the four
    wave sums through one more; out = sum * (1 / sqrt(|sum|^2)).  The kernel's fmaf(a, a, acc) is restated as the fp64 a * a + acc
    (the product is exact in fp64) rounded to fp32: the sum is rounded twice, so this is NOT an exact fmaf and may differ from it in
    the last bit of |sum|^2 in rare cases.  -> cent_new [r, c, d] fp32 numpy."""
    import torch
    x32, out = torch.tensor(np.asarray(x, dtype=np.float32)), torch.tensor(np.asarray(cent, dtype=np.float32))
    r, c, d = out.shape
    for s in range(r):
        for j in range(c):
            rows = np.nonzero(np.asarray(assign[s]) == j)[0]
            if not rows.size:
                continue
            total = torch.zeros(d, dtype=torch.float32)
            for i in rows:                                  # ascending
                total = total + x32[int(i)]
            padded = torch.zeros(-(-d // 256) * 256, dtype=torch.float32)
            padded[:d] = total
            part = torch.zeros(256, dtype=torch.float32)
            for q in range(padded.numel() // 256):
                a = padded[q * 256:(q + 1) * 256].to(torch.float64)
                part = (a * a + part.to(torch.float64)).to(torch.float32)
            waves = torch.zeros(64, dtype=torch.float32)
            for w in range(4):
                waves[w] = _tree64(part[64 * w:64 * w + 64])
            ss = _tree64(waves)
            if float(ss) > 0:
                out[s, j] = total * (torch.ones((), dtype=torch.float32) / torch.sqrt(ss))
    return out.numpy()


def spec_assignment(case):
    """The assignment the update cases are run on: the spec's own for ``cent``, int32 [r, n]."""
    return assign_ref(case["x"], case["cent"])["assign"].astype(np.int32)


@functools.lru_cache(maxsize=None)
def restatement_error():
    """The largest |update_restated_fp32 - update_ref| over CASES (centroid rows have unit length)."""
    worst = 0.0
    for shape in CASES:
        case = make_case(*shape)
        a = spec_assignment(case)
        ref, _ = update_ref(case["x"], a, case["cent"])
        worst = max(worst, float(np.abs(update_restated_fp32(case["x"], a, case["cent"]).astype(np.float64) - ref).max()))
    return worst


def update_bound():
    return UPDATE_MARGIN * restatement_error()


def fit_ref(x, init, iters):
    """cstp_amd.cluster.fit restated in fp64 from the same initial centroids init [r, c, d] on unit rows x [n, d]: ``iters`` rounds
    of assign + update, one more assign -> dict(cent [r, c, d], assign [r, n], final [r] scores, moved [iters, r], win)."""
    cent = np.asarray(init, dtype=np.float64)
    r = cent.shape[0]
    moved = np.zeros((iters, r), dtype=np.int64)
    prev = None
    for t in range(iters):
        a = assign_ref(x, cent)["assign"]
        moved[t] = x.shape[0] if prev is None else (a != prev).sum(axis=1)
        cent, _ = update_ref(x, a, cent)
        prev = a
    last = assign_ref(x, cent)
    win = max(range(r), key=lambda s: (last["score"][s], -s))
    return {"cent": cent, "assign": last["assign"], "final": last["score"], "moved": moved, "win": win}

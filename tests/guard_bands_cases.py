"""Case shapes and fp64 references shared by tests/test_guard_bands_ops_gpu.py (the HIP kernels between guard bands) and
tests/test_guard_bands_ops_host.py (plain torch implementations through the same Spec / impl signature, no GPU): the flat
arena of the table-driven optimiser steps, the SAME max-pool with its argmax, and the BatchNorm + ReLU concat tail with its
ReLU-kink mask.  Device-agnostic; nothing here imports the library."""
import functools

import torch
import torch.nn.functional as F

F32, F64, I32 = torch.float32, torch.float64, torch.int32
CHUNK = 4096                      # CSTP_LARS_CHUNK (include/cstp_hip.h); the GPU file asserts cstp_lars_chunk() == CHUNK


def rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=F64) * 2 - 1


def f32(v):
    """The value a c_float argument carries, as a Python float."""
    return float(torch.tensor(v, dtype=F32))


# ---- the arena of the table-driven steps -------------------------------------------------------------------------------------
# (offset, elements, padded extent, segment or None = frozen and unlisted, adapted by LARS)
TENSORS = [
    (0, 1, 4, 0, 0),                                   # one float, padded to 4
    (4, 5, 8, 1, 1),                                   # five floats, padded to 8
    (12, 8, 8, None, 0),                               # FROZEN: no chunk lists it
    (20, CHUNK, CHUNK, 2, 1),                          # exactly one full chunk
    (20 + CHUNK, CHUNK + 4, CHUNK + 4, 3, 1),          # two chunks, the second of length 4
    (24 + 2 * CHUNK, 12, 12, 4, 0),                    # ends exactly at n
]
ARENA_N = 36 + 2 * CHUNK
N_SEGS = 5
HYPER = [(1.0, 0.0), (0.5, 5e-4), (0.25, 5e-4), (1.0, 1e-3), (2.0, 0.0)]        # {lr scale, weight decay} per segment


def arena_masks():
    """(own, pad, frozen) bool [ARENA_N]: the floats of listed tensors, their zero padding, the frozen tensor."""
    own, pad, frozen = (torch.zeros(ARENA_N, dtype=torch.bool) for _ in range(3))
    for off, numel, padded, seg, _ in TENSORS:
        if seg is None:
            frozen[off:off + numel] = True
        else:
            own[off:off + numel] = True
            pad[off + numel:off + padded] = True
    assert bool((own | pad | frozen).all()) and int(own.sum() + pad.sum() + frozen.sum()) == ARENA_N
    return own, pad, frozen


def arena_values(seed, scale=1.0, nonneg=False):
    """An fp32 arena: live values in every tensor (the frozen one included), +0 in the padding."""
    v = rand((ARENA_N,), seed) * scale
    if nonneg:
        v = v.abs()
    v = v.float()
    v[arena_masks()[1]] = 0.0
    return v


def arena_tables():
    """(chunks [n_chunks][3], segs [n_segs][3]) int32, as include/cstp_hip.h describes them."""
    chunks, segs = [], []
    for off, numel, padded, seg, adapted in TENSORS:
        if seg is None:
            continue
        first = len(chunks)
        for o in range(0, padded, CHUNK):
            chunks.append((seg, off + o, min(CHUNK, padded - o)))
        segs.append((first, len(chunks) - first, adapted))
    return torch.tensor(chunks, dtype=I32), torch.tensor(segs, dtype=I32)


def malformed_chunks():
    """Entries a kernel must skip.  Every one, if a broken kernel FOLLOWED it, still lands inside the arena or its guard bands
    (64 KiB = 16384 floats either side): offsets stay within 4 floats of the arena, the segment is one past the table."""
    n = ARENA_N
    return [(N_SEGS, 0, 4),                # seg = n_segs: one past the hyper / segs table
            (0, -4, 4),                    # off = -4
            (4, n - 4, 8),                 # off + len = n + 4: starts inside, ends past the arena
            (2, 20, CHUNK + 4),            # len = CSTP_LARS_CHUNK + 4
            (0, 2, 4)]                     # off = 2: not a multiple of 4


def listed_slices():
    return [(off, off + numel) for off, numel, _, seg, _ in TENSORS if seg is not None]


# ---- SAME max-pool: ATen over the padded tensor, the argmax brought back to the unpadded volume --------------------------------
def same_pads(kernel, stride):
    """((front, back) for d, h, w): pad = max(k - s, 0), front = pad // 2 (i3d_byol.py get_padding_shape)."""
    out = []
    for k, s in zip(kernel, stride):
        pad = max(k - s, 0)
        out.append((pad // 2, pad - pad // 2))
    return out


def same_pool_aten(x, kernel, stride):
    """ATen over the zero-padded tensor (test_i3d_gpu.py's _pool_ref) -> (y, argmax): argmax int32, the flat index in the UNPADDED
    volume, or -1 where a padding zero won.  x: [rows][d][h][w], any float dtype; y is differentiable in x."""
    (fd, bd), (fh, bh), (fw, bw) = same_pads(kernel, stride)
    xp = F.pad(x, (fw, bw, fh, bh, fd, bd))
    y, idx = F.max_pool3d(xp, kernel, stride, ceil_mode=True, return_indices=True)
    pH, pW = xp.shape[2], xp.shape[3]
    D, H, W = x.shape[1:]
    i_d, i_h, i_w = idx // (pH * pW) - fd, (idx // pW) % pH - fh, idx % pW - fw
    inside = (i_d >= 0) & (i_d < D) & (i_h >= 0) & (i_h < H) & (i_w >= 0) & (i_w < W)
    return y, torch.where(inside, (i_d * H + i_h) * W + i_w, torch.full_like(idx, -1)).to(I32)


@functools.lru_cache(maxsize=None)
def same_pool_case(rows, vol, kernel, stride, negative=-1):
    """x fp32 [rows][d][h][w] on the grid of multiples of 0.5 in [-2, 2] with one volume (the last by default) all negative: every
    border window of it is won by a padding zero, argmax -1.  -> x, dy, and ATen's y, argmax and dx."""
    g = torch.Generator().manual_seed(100 + rows + sum(vol))
    x = torch.randint(-4, 5, (rows,) + tuple(vol), generator=g).double() * 0.5
    x[negative] = -x[negative].abs() - 0.5
    xr = x.clone().requires_grad_(True)
    y, arg = same_pool_aten(xr, kernel, stride)
    dy = torch.rand(tuple(y.shape), generator=g, dtype=F64) * 2 - 1
    (dx,) = torch.autograd.grad(y, xr, dy)
    assert bool((arg[negative] == -1).any()), "the case holds no window that a padding zero wins"
    return {"x": x.float(), "dy": dy.float(), "y": y.detach(), "argmax": arg, "dx": dx}


# ---- BatchNorm + ReLU into the concat -----------------------------------------------------------------------------------------
BN_EPS, BN_MOM = 1e-5, 0.1
KINK = 1e-4                       # tests/test_i3d_gpu.py _mask_kink
KINK_CAP = 0.01                   # at most 1 % of the positions may be masked this way


@functools.lru_cache(maxsize=None)
def bnc_case(cs, spatial, n, groups, seed):
    """Inputs (fp32 values held in fp64 where the reference needs them) and fp64 results of train-mode BatchNorm + ReLU of every
    branch into the concat tensor (test_i3d_gpu.py's _bnc_case / _bnc_ref), dy with the ReLU kinks masked, the eval-mode y."""
    g = torch.Generator().manual_seed(seed)
    r = lambda shape: torch.rand(shape, generator=g, dtype=F64)      # noqa: E731
    xs = [(r((n, c) + tuple(spatial)) * 3 - 1.2).float() for c in cs]
    gammas = [(r((c,)) * 2 - 1).float() for c in cs]
    betas = [((r((c,)) * 2 - 1) * 0.3).float() for c in cs]
    rms = [((r((c,)) * 2 - 1) * 0.1).float() for c in cs]
    rvs = [(r((c,)) + 0.5).float() for c in cs]
    dy = (r((n, sum(cs)) + tuple(spatial)) * 2 - 1).float()
    npg = n // groups
    red = (0, 2, 3, 4)
    xr = [x.double().requires_grad_(True) for x in xs]
    gr = [t.double().requires_grad_(True) for t in gammas]
    br = [t.double().requires_grad_(True) for t in betas]
    rm2, rv2 = [t.double().clone() for t in rms], [t.double().clone() for t in rvs]
    zs, means, invstds = [], [], []
    for x, ga, be, rm, rv in zip(xr, gr, br, rm2, rv2):
        zs.append(torch.cat([F.batch_norm(x[i * npg:(i + 1) * npg], rm, rv, ga, be, True, BN_MOM, BN_EPS) for i in range(groups)], 0))
        means.append(torch.stack([x.detach()[i * npg:(i + 1) * npg].mean(red) for i in range(groups)]))
        invstds.append(torch.stack([1.0 / torch.sqrt(x.detach()[i * npg:(i + 1) * npg].var(red, unbiased=False) + BN_EPS)
                                    for i in range(groups)]))
    z = torch.cat(zs, 1)
    kink = z.detach().abs() < KINK
    dy = torch.where(kink, torch.zeros_like(dy), dy)
    y = F.relu(z)
    grads = torch.autograd.grad(y, xr + gr + br, dy.double())
    nb = len(cs)
    mean, invstd = torch.cat(means, 1), torch.cat(invstds, 1)                # [groups][C]
    scale = invstd * torch.cat([t.double() for t in gammas]).view(1, -1)
    ss = torch.stack([scale, torch.cat([t.double() for t in betas]).view(1, -1) - mean * scale], 2)      # [groups][C][2]
    y_eval = torch.cat([F.relu(F.batch_norm(x.double(), rm.double(), rv.double(), ga.double(), be.double(), False, 0.0, BN_EPS))
                        for x, ga, be, rm, rv in zip(xs, gammas, betas, rms, rvs)], 1)
    return {"xs": xs, "gammas": gammas, "betas": betas, "rms": rms, "rvs": rvs, "dy": dy, "y": y.detach(), "mean": mean,
            "invstd": invstd, "ss": ss, "rm_new": rm2, "rv_new": rv2, "dx": grads[:nb], "dgamma": grads[nb:2 * nb],
            "dbeta": grads[2 * nb:], "kink_share": float(kink.double().mean()), "y_eval": y_eval}


def conv_sums(x, groups, pivot, nsplit=3):
    """The table cstp_conv3d_forward_bnstats leaves beside x (test_i3d_gpu.py's _conv_sums): [c][groups][nsplit] sums of
    (x - pivot) and (x - pivot)^2 in fp64, the c pivots behind them, then room for the range keys."""
    n, c = x.shape[0], x.shape[1]
    npg = n // groups
    d = x.double() - pivot.double().view(1, c, 1, 1, 1)
    part = torch.zeros(c * groups * nsplit * 3 + c, dtype=F64)
    tab = part[:c * groups * nsplit * 2].view(c, groups, nsplit, 2)
    for g in range(groups):
        for j in range(nsplit):
            rows = d[g * npg + j:(g + 1) * npg:nsplit]
            if rows.numel():
                tab[:, g, j, 0] = rows.sum(dim=(0, 2, 3, 4))
                tab[:, g, j, 1] = (rows * rows).sum(dim=(0, 2, 3, 4))
    part[c * groups * nsplit * 2:c * groups * nsplit * 2 + c] = pivot.double()
    return part


# (cs, spatial, n, groups, seed) of every concat-tail case of the GPU file; the host test holds each to KINK_CAP
BNC_CASES = {
    "ragged g1": ((24, 7, 130, 1), (3, 5, 3), 4, 1, 31),
    "ragged g2": ((24, 7, 130, 1), (3, 5, 3), 4, 2, 32),
    "float4": ((16, 8), (2, 2, 2), 4, 1, 33),
    "strided": ((230, 230), (1, 2, 2), 18, 2, 34),              # rows = 8280 > 4 * BNC_APPLY_MAX_BLOCKS at s = 4
}

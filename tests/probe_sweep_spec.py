"""The specification of the linear-probe sweep (include/cstp_hip.h: cstp_probe_sweep_step / _score; cstp_amd.probe.sweep), shared
by tests/test_probe_sweep_host.py and tests/test_probe_sweep_gpu.py: the cases, and restatements of holdout_split, the grid order,
the selection rule and the per-head schedule that share no code with cstp_amd.probe beyond plan().

The kernels' contract is bit equality with the single-head call, so the GPU test needs no tolerance of its own: head g of a sweep
call is compared with ops.probe_step on (W_g, b_g) by torch.equal, and head 0 is additionally held to probe_spec.step_ref at
probe_spec's tolerances and near-tie rule (the host test asserts the near-tie share of these inputs from the spec alone).
"""
import math

import numpy as np

from probe_spec import MAX_NEAR_TIE_SHARE, fit_ref, make_case, make_clusters, step_ref  # noqa: F401  (re-exported to the tests)

MAX_HEADS = 32

# (G, m, n, d, c, rows): rows as in probe_spec.STEP_CASES
SWEEP_CASES = [(1, 70, 70, 24, 10, False),
               (3, 70, 300, 23, 3, True),            # odd d, the scalar load path, a stride that needs padding
               (4, 130, 130, 512, 101, False),       # more classes than lanes
               (2, 257, 1000, 100, 400, True),       # four class tiles, two row slices
               (32, 9, 20, 8, 2, True),              # the head limit, one row past a slab
               (5, 64, 64, 4, 65, False)]
GUARD_STEP_CASES = [1, 3]                            # indices into SWEEP_CASES
GUARD_SCORE_CASES = [1]

# "a head trains as it would alone"
TRAIN = dict(n=96, d=24, c=5, epochs=3, batch=32, lrs=(1e-3, 3e-2), wds=(0.0, 1e-2), val_fraction=0.25, seed=5)

# selection and refit: 800 rows in 10 clusters 10 sigma apart, 10 informative dimensions among 128.  With Adam a rate of 1e-6
# moves every weight by about the same tiny amount in the direction of its first gradients' sign, so the 118 noise dimensions
# outvote the 10 informative ones; 1e-2 over 380 steps fits the clusters.  fp64 (fit_ref): 124 against 195 of 201 held-out rows.
SELECT = dict(n=800, d=128, c=10, sep=10.0, cluster_seed=0, epochs=20, batch=32, lrs=(1e-6, 1e-2), val_fraction=0.25, seed=0)


def pad4(v):
    return (v + 3) // 4 * 4


def head_stride(c, d):
    """seg = pad4(c d) + pad4(c): W_g at g * seg, b_g at g * seg + pad4(c d)."""
    return pad4(c * d) + pad4(c)


def make_sweep_case(G, m, n, d, c, rows):
    """probe_spec.make_case(m, n, d, c, rows) -- x, labels, mean, inv_std, rows, and head 0 -- with W_g, b_g of head g taken from
    make_case(seed=g): "w" [G, c, d] and "b" [G, c] fp32."""
    case = dict(make_case(m, n, d, c, rows))
    heads = [make_case(m, n, d, c, rows, seed=g) for g in range(G)]
    case["w"] = np.stack([h["w"] for h in heads])
    case["b"] = np.stack([h["b"] for h in heads])
    case["G"] = G
    return case


def arena_of(w, b):
    """The heads of (w [G, c, d], b [G, c]) laid out in one flat fp32 arena of G * head_stride floats, padding zero."""
    G, c, d = w.shape
    seg = head_stride(c, d)
    arena = np.zeros(G * seg, dtype=np.float32)
    for g in range(G):
        arena[g * seg:g * seg + c * d] = w[g].reshape(-1)
        arena[g * seg + pad4(c * d):g * seg + pad4(c * d) + c] = b[g]
    return arena


def owned_mask(G, c, d):
    """bool [G * head_stride]: the floats of an arena that belong to some W_g or b_g (the rest is inter-head padding)."""
    seg = head_stride(c, d)
    own = np.zeros(G * seg, dtype=bool)
    for g in range(G):
        own[g * seg:g * seg + c * d] = True
        own[g * seg + pad4(c * d):g * seg + pad4(c * d) + c] = True
    return own


def holdout_ref(labels, fraction, seed):
    """probe.holdout_split restated row by row: per class, the class's rows ascending, permuted by torch.randperm under a CPU
    generator seeded with (seed * 1000003 + class) mod 2^63; the first round-half-up(fraction * n_c) go to validation, at least
    one if n_c >= 2, none if n_c == 1 -> (train ascending int32, val ascending int32)."""
    import torch
    labels = [int(v) for v in labels]
    val = set()
    for cls in sorted(set(labels)):
        rows = [i for i, y in enumerate(labels) if y == cls]
        k = int(math.floor(fraction * len(rows) + 0.5))
        k = 0 if len(rows) == 1 else max(k, 1)
        gen = torch.Generator(device="cpu")
        gen.manual_seed((seed * 1000003 + cls) % (1 << 63))
        order = torch.randperm(len(rows), generator=gen).tolist()
        val.update(rows[j] for j in order[:k])
    train = [i for i in range(len(labels)) if i not in val]
    return np.array(train, dtype=np.int32), np.array(sorted(val), dtype=np.int32)


def grid_ref(lrs, wds):
    """Head i * len(wds) + j is (lrs[i], wds[j])."""
    out = [None] * (len(lrs) * len(wds))
    for i, lr in enumerate(lrs):
        for j, wd in enumerate(wds):
            out[i * len(wds) + j] = (float(lr), float(wd))
    return out


def select_ref(val_hits, val_loss):
    """Most hits; among those the lowest loss; among those the lowest index."""
    best = 0
    for g in range(1, len(val_hits)):
        if val_hits[g] > val_hits[best] or (val_hits[g] == val_hits[best] and val_loss[g] < val_loss[best]):
            best = g
    return best


def schedule_ref(grid, n_train, epochs, batch, seed):
    """[steps, G] fp32: column g is the learning rate plan(n_train, epochs, batch, lr_g, seed) gives a fit at lr_g alone."""
    from cstp_amd.probe import plan
    return np.stack([plan(n_train, epochs, batch, lr, seed)[1].numpy() for lr, _ in grid], axis=1)


def select_data():
    """-> (features fp32 [n, d], labels int64 [n]) torch CPU tensors of SELECT."""
    return make_clusters(SELECT["n"], SELECT["d"], SELECT["c"], SELECT["sep"], seed=SELECT["cluster_seed"])


def select_val_hits_fp64():
    """The validation hit counts of SELECT's two grid points in fp64 (fit_ref on the train part, Adam, no decay; arg-max of the
    held-out rows' logits) -> ([hits per lr], validation rows)."""
    feat, lab = select_data()
    train, val = holdout_ref(lab.tolist(), SELECT["val_fraction"], SELECT["seed"])
    hits = []
    for lr in SELECT["lrs"]:
        w, b, _, _, mean, inv_std, _ = fit_ref(feat[train], lab[train], SELECT["c"], SELECT["epochs"], SELECT["batch"], lr, 0.0, "adam",
                                               0.9, SELECT["seed"])
        logits = ((feat[val].double() - mean.double()) * inv_std.double()) @ w.T + b
        hits.append(int((logits.argmax(dim=1) == lab[val]).sum()))
    return hits, int(val.size)

"""Inputs, fp64 references and comparators of the edge cases of the first-generation ops (csrc/misc.hip, the train and eval
BatchNorm of csrc/bn.hip, the convolution bias path), shared by tests/test_ops_edges_gpu.py (the HIP kernels) and
tests/test_ops_edges_host.py (stock PyTorch in fp32 and deliberately naive variants through the same comparators, no GPU).

Comparators.  ``rel_err`` is conftest's global metric (max-abs-diff / max-abs-ref).  ``row_err`` is the same metric per row --
per (sample, channel) plane, per channel -- for ops whose rows are independent, where one global maximum hides every row but
the largest: a row r passes at a bar when

    max |got_r - ref_r| <= bar * max |ref_r| + floor_r,

floor_r = four fp32 roundings (U4 = 4 * 2^-24) of the largest term the op's formula adds or subtracts to form that row.  Every
floor is derived from operand magnitudes in the docstring of its case, none from a measured error.  ``row_err`` returns
max_r (err_r - floor_r)+ / max |ref_r| (infinite for a row whose reference is identically zero and whose error exceeds the
floor), a figure to hold against the same bar as the global one.

Bars are those of each op's existing test: 1e-4 cross-entropy, BYOL, NT-Xent, avg-pool, BatchNorm, convolution; 1e-5 soft
cross-entropy, L2 normalise, eval BatchNorm, Adam; 1e-6 max-pool dx, EMA / sumsq / SGD.  Max-pool outputs are compared exactly.
"""
import functools

import torch
import torch.nn.functional as F

from conftest import rel_err

U4 = 4 * 2.0 ** -24
DLOSS = 1.7          # the upstream gradient of the scalar losses (as tests/test_ops_gpu.py and tests/test_mix_gpu.py use)


def row_err(got, ref, floor, chan=False):
    """max over rows of (max|got_r - ref_r| - floor_r)+ / max|ref_r|; rows = the leading dimension (chan: dimension 1, the
    channels of an [N, C, ...] tensor).  ``floor``: a scalar or one value per row."""
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    if chan:
        got, ref = got.movedim(1, 0), ref.movedim(1, 0)
    rows = ref.shape[0] if ref.dim() > 0 else 1
    got, ref = got.reshape(rows, -1), ref.reshape(rows, -1)
    floor = torch.as_tensor(floor, dtype=torch.float64).reshape(-1)
    floor = floor.expand(rows) if floor.numel() == 1 else floor.reshape(rows)
    err = (got - ref).abs().amax(dim=1)
    err = torch.where(err.isnan(), torch.full_like(err, float("inf")), err)
    over = (err - floor).clamp_min(0.0)
    scale = ref.abs().amax(dim=1)
    ratio = torch.where(over > 0, over / scale, torch.zeros_like(over))      # x / 0 = inf: a zero row is held to the floor alone
    return float(ratio.max())


class Out:
    """One output of a case: its fp64 reference, its bar, and (row-independent outputs) the per-row floor."""
    def __init__(self, ref, bar, floor=None, chan=False, exact=False, undecided=None):
        self.ref, self.bar, self.floor, self.chan, self.exact = ref.detach(), bar, floor, chan, exact
        self.undecided = undecided      # bool mask of elements either value of which is right (a ReLU input within its floor of 0)


def compare(what, outs, got):
    """Every output of ``got`` (name -> tensor) against ``outs`` (name -> Out): prints the measured global and row-wise error of
    each and returns the list of failures (empty: the case passes)."""
    fails = []
    for name, o in outs.items():
        g = got[name].reshape(o.ref.shape)
        if o.undecided is not None and bool(o.undecided.any()):
            print("EDGE %s %s: %d elements undecided" % (what, name, int(o.undecided.sum())))
            g = torch.where(o.undecided, o.ref, g.detach().double().cpu())
        if o.exact or (o.floor is None and float(o.ref.abs().max()) == 0):
            ok = torch.equal(g.detach().double().cpu(), o.ref.double())
            print("EDGE %s %s exact=%s" % (what, name, ok))
            if not ok:
                fails.append("%s %s: not exactly the reference" % (what, name))
            continue
        ge = rel_err(g, o.ref) if float(o.ref.abs().max()) > 0 else float("nan")
        re = row_err(g, o.ref, o.floor, o.chan) if o.floor is not None else float("nan")
        print("EDGE %s %s global=%.3g row=%.3g bar=%g" % (what, name, ge, re, o.bar))
        if float(o.ref.abs().max()) > 0 and not ge < o.bar:
            fails.append("%s %s: global %.3g >= %g" % (what, name, ge, o.bar))
        if o.floor is not None and not re < o.bar:
            fails.append("%s %s: row-wise %.3g >= %g" % (what, name, re, o.bar))
    return fails


def _gen(*key):
    return torch.Generator().manual_seed(1 + sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)) % (2 ** 31))


# ---------------------------------------------------------------------------------------------------------------------------
# A. softmax heads
# ---------------------------------------------------------------------------------------------------------------------------
CE_SHAPES = [(1, 1), (1, 2), (3, 63), (3, 64), (3, 65), (2, 101), (2, 400), (257, 5), (1025, 3)]
CE_PATTERNS = ["randn30", "identical", "tie", "shift4096", "neginf", "tie4096"]


@functools.lru_cache(maxsize=None)
def ce_inputs(b, k, pattern):
    """fp32 logits [b, k] = randn * 30 with the row maxima put AT +100 (even rows) and -100 (odd rows): without the
    max-subtraction expf overflows on the even rows and underflows to log(0) on the odd ones.  Row 0 (and the last row) then
    carry the pattern: all logits identical (100.25), the maximum tied with its neighbour, the row shifted by +4096, (hard
    labels only) one -inf logit off the label, or the tie AND the shift.  The label of row 0 is its arg-max, the others are
    random.  Also ta / tb / lam of the soft targets.
    "tie4096" is the one pattern that shows an absolute error of the log-sum-exp: on randn * 30 the loss of a row is either tens
    (a wrong label) or below 1e-10 (the arg-max), so an error of ulp(4196) / 2 = 2.4e-4 in a shifted row's log-sum-exp stays
    under every bar; with the maximum tied and the arg-max as the label the row's loss is log 2 and the error is 3.5e-4 of it."""
    g = _gen(b, k, CE_PATTERNS.index(pattern))
    z = (torch.randn((b, k), generator=g) * 30).float()
    mx = z.amax(dim=1, keepdim=True)
    sign = torch.where(torch.arange(b) % 2 == 0, 100.0, -100.0).float()[:, None]
    z = z - mx + sign
    lab = torch.randint(0, k, (b,), generator=g)
    lab[0] = int(z[0].argmax())
    tb = torch.randint(0, k, (b,), generator=g)
    lam = torch.rand((b,), generator=g).float()
    for r in sorted({0, b - 1}):
        j = int(z[r].argmax())
        if pattern == "identical":
            z[r] = 100.25
        elif pattern in ("tie", "tie4096") and k > 1:
            z[r, (j + 1) % k] = z[r, j]
        if pattern in ("shift4096", "tie4096"):
            z[r] = z[r] + 4096.0
        elif pattern == "neginf" and k > 1:
            z[r, (int(lab[r]) + 1) % k] = float("-inf")
    return z, lab, tb, lam


def q64(ta, tb, lam, eps, k):
    """The soft targets in fp64 (tests/test_mix_gpu._q64)."""
    q = (1.0 - eps) * (lam.double()[:, None] * F.one_hot(ta, k).double() + (1.0 - lam.double())[:, None] * F.one_hot(tb, k).double())
    return q + eps / k


def _ce_outs(z, loss, grad, b, k, bar):
    """Floor of the gradient rows: dlogits = (dloss / b) * (softmax - q), softmax and q in [0, 1], so the largest term a row
    subtracts is |dloss| / b.  The loss is one number, mean_r (lse_r - sum_c q z_rc): it is its own single row, the terms are of
    the magnitude of the row's logits, floor U4 * mean_r max_c |z_rc| (finite logits) -- it matters where the true loss is 0 to
    fp64 (one row, the arg-max as the label).  k = 1: loss and gradient are exactly 0."""
    if k == 1:
        return {"loss": Out(loss, bar, exact=True), "dlogits": Out(grad, bar, exact=True)}
    zmax = torch.where(z.isinf(), torch.zeros_like(z), z).double().abs().amax(dim=1).mean()
    return {"loss": Out(loss.reshape(1), bar, U4 * zmax), "dlogits": Out(grad, bar, U4 * DLOSS / b)}


@functools.lru_cache(maxsize=None)
def ce_case(b, k, pattern):
    z, lab, _, _ = ce_inputs(b, k, pattern)
    x = z.double().requires_grad_(True)
    loss = F.cross_entropy(x, lab)
    (loss * DLOSS).backward()
    return _ce_outs(z, loss.detach(), x.grad, b, k, 1e-4)


SOFT_VARIANTS = [(eps, mixed) for eps in (0.0, 0.1) for mixed in (False, True)]


@functools.lru_cache(maxsize=None)
def soft_ce_case(b, k, pattern, eps, mixed):
    """mixed: tb and lam present; else absent (tb = ta, lam = 1).  Reference F.cross_entropy(fp64 logits, q)."""
    z, ta, tb, lam = ce_inputs(b, k, pattern)
    x = z.double().requires_grad_(True)
    q = q64(ta, tb if mixed else ta, lam if mixed else torch.ones(b), eps, k)
    loss = F.cross_entropy(x, q)
    (loss * DLOSS).backward()
    return _ce_outs(z, loss.detach(), x.grad, b, k, 1e-5)


def softmax_host(z, q, naive, dtype=torch.float32):
    """(loss, dlogits) of mean_r -sum_c q log_softmax(z) in ``dtype`` by autograd with the upstream gradient DLOSS: stock
    F.cross_entropy, or the NAIVE log-sum-exp without the max-subtraction."""
    x = z.detach().to(dtype).clone().requires_grad_(True)
    if naive:
        lse = torch.log(torch.exp(x).sum(dim=1, keepdim=True))
        loss = -(q.to(dtype) * (x - lse)).sum(dim=1).mean()
    else:
        loss = F.cross_entropy(x, q.to(dtype))
    (loss * DLOSS).backward()
    return {"loss": loss.detach(), "dlogits": x.grad}


# (n, f, tau).  Zero rows are left out (the clamp at 1e-8 of |r_i||r_j| has no counterpart worth pinning: the model never
# produces one) and so is f = 1: the cosine of 1-D vectors is +-1 and the true gradient is identically zero.
NTX_CASES = [(2, 2, 0.5), (3, 65, 0.01), (5, 63, 0.1), (129, 63, 0.01), (5, 2048, 0.1)]


@functools.lru_cache(maxsize=None)
def ntx_inputs(n, f):
    """zi, zj fp32 randn; zi[1] == zj[1] (a positive pair at cosine 1) and, from n = 3, zi[2] == zj[0] (identical rows in
    different pairs: a negative at cosine 1)."""
    g = _gen(n, f)
    zi, zj = torch.randn((n, f), generator=g).float(), torch.randn((n, f), generator=g).float()
    zi[1] = zj[1]
    if n >= 3:
        zi[2] = zj[0]
    return zi, zj


def ntx_host(zi, zj, tau, dtype, naive=False):
    """(loss, dreps) with reps = cat(zj, zi), by autograd, upstream gradient DLOSS.  The oracle's formula; naive: the same
    log-sum-exp over j != i without the max-subtraction."""
    from oracle import r21d_byol_oracle as orc
    a, b = zi.detach().to(dtype).clone().requires_grad_(True), zj.detach().to(dtype).clone().requires_grad_(True)
    if naive:
        n = a.shape[0]
        reps = torch.cat([b, a], 0)
        nrm = reps.norm(dim=1, keepdim=True)
        sim = (reps @ reps.t()) / torch.clamp(nrm * nrm.t(), min=1e-8) / tau
        idx = torch.arange(2 * n)
        e = torch.exp(sim) * (1.0 - torch.eye(2 * n, dtype=dtype))
        loss = (torch.log(e.sum(dim=1)) - sim[idx, (idx + n) % (2 * n)]).mean()
    else:
        loss = orc.ntxent(a, b, tau)
    (loss * DLOSS).backward()
    return {"loss": loss.detach(), "dreps": torch.cat([b.grad, a.grad], 0)}


@functools.lru_cache(maxsize=None)
def ntx_case(n, f, tau):
    """Global metric only: the rows of the gradient are coupled through the similarity matrix (row i collects G_ij + G_ji of
    every other row), so they are not independent and a row's error scales with the tensor's magnitude, not with its own."""
    zi, zj = ntx_inputs(n, f)
    r = ntx_host(zi, zj, tau, torch.float64)
    return {"loss": Out(r["loss"], 1e-4), "dreps": Out(r["dreps"], 1e-4)}


PROBE_FEATURE_SCALE = 40.0


@functools.lru_cache(maxsize=None)
def probe_case():
    """The first step case of tests/probe_spec.py (70 rows, 24 features, 10 classes, no standardisation) with the features
    scaled by 40, so the logits pass +-88 -> (numpy case, probe_spec.step_ref's fp64 result)."""
    import numpy as np
    import probe_spec
    case = dict(probe_spec.make_case(70, 70, 24, 10, False))
    case["x"] = case["x"] * np.float32(PROBE_FEATURE_SCALE)
    return case, probe_spec.step_ref(case["x"], case["labels"], case["w"], case["b"])


def probe_host(case, naive):
    """(loss, dw, db) of the spec's formula in numpy fp32; naive: without the max-subtraction."""
    import numpy as np
    x, w, b, y = case["x"], case["w"], case["b"], case["labels"]
    m = x.shape[0]
    logits = x @ w.T + b
    with np.errstate(all="ignore"):
        mx = np.zeros((m, 1), np.float32) if naive else logits.max(axis=1, keepdims=True)
        e = np.exp(logits - mx)
        se = e.sum(axis=1, keepdims=True)
        loss = ((np.log(se) + mx)[:, 0] - logits[np.arange(m), y]).sum() / np.float32(m)
        g = e / se
        g[np.arange(m), y] -= np.float32(1)
        g = g / np.float32(m)
        return loss, g.T @ x, g.sum(axis=0)


def probe_compare(what, ref, loss, dw, db):
    """The checks and bars of tests/test_probe_gpu._check_step (LOSS_RTOL, GRAD_RTOL of tests/probe_spec.py) -> failures."""
    import numpy as np
    import probe_spec
    errs = {"loss": abs(float(loss) - ref["loss"]) / abs(ref["loss"]),
            "dw": np.abs(np.asarray(dw, np.float64) - ref["dw"]).max() / np.abs(ref["dw"]).max(),
            "db": np.abs(np.asarray(db, np.float64) - ref["db"]).max() / np.abs(ref["db"]).max()}
    print("EDGE %s loss=%.3g (bar %g) dw=%.3g db=%.3g (bar %g)" % (what, errs["loss"], probe_spec.LOSS_RTOL, errs["dw"], errs["db"],
                                                                 probe_spec.GRAD_RTOL))
    return ["%s %s: %.3g" % (what, k, v) for k, v in errs.items()
            if not v <= (probe_spec.LOSS_RTOL if k == "loss" else probe_spec.GRAD_RTOL)]


# ---------------------------------------------------------------------------------------------------------------------------
# B. row-normalising ops
# ---------------------------------------------------------------------------------------------------------------------------
NORM_F = [2, 63, 64, 65, 127, 129, 2049]
NORM_B = [1, 6, "special"]
ROW_SCALES = [1e-3, 1e0, 1e3, 1e-1, 1e2, 1e1]
NORM_EPS = 1e-12


@functools.lru_cache(maxsize=None)
def norm_inputs(f, b):
    """x, t, dl (BYOL's per-row upstream gradient), dy (L2 normalise's) in fp32.  b rows scaled by ROW_SCALES, t in the opposite
    order; "special": an all-zero x row, an all-zero t row and a row at scale 1e15."""
    if b == "special":
        g = _gen(f, 99)
        x, t = torch.randn((3, f), generator=g).float(), torch.randn((3, f), generator=g).float()
        x[0] = 0.0
        t[1] = 0.0
        x[2] *= 1e15
    else:
        g = _gen(f, b)
        x, t = torch.randn((b, f), generator=g).float(), torch.randn((b, f), generator=g).float()
        sc = torch.tensor(ROW_SCALES[:b]).float()[:, None]
        x, t = x * sc, t * sc.flip(0)
    rows = x.shape[0]
    dl = (torch.rand((rows,), generator=g) * 2 - 1).float()
    dy = (torch.rand((rows, f), generator=g) * 2 - 1).float()
    return x, t, dl, dy


def byol_host(x, t, dl, dtype):
    a = x.detach().to(dtype).clone().requires_grad_(True)
    loss = 2 - 2 * (F.normalize(a, dim=-1, eps=NORM_EPS) * F.normalize(t.to(dtype), dim=-1, eps=NORM_EPS)).sum(-1)
    loss.backward(dl.to(dtype))
    return {"loss": loss.detach(), "dx": a.grad}


@functools.lru_cache(maxsize=None)
def byol_case(f, b):
    """loss_r = 2 - 2 cos: the terms are 2 and 2 cos, floor U4 * 2.  dx_r = -(2 dl_r / |x_r|) (t^ - cos x^) with |t^_i|,
    |cos x^_i| <= 1: the largest term is 2 |dl_r| / max(|x_r|, eps), floor U4 times that.  An all-zero x row: loss 2 and
    dx = -2 dl t^ / eps (the clamp has zero slope); an all-zero t row: loss 2 and dx = 0 (floor alone)."""
    x, t, dl, _ = norm_inputs(f, b)
    r = byol_host(x, t, dl, torch.float64)
    nx = x.double().norm(dim=1).clamp_min(NORM_EPS)
    return {"loss": Out(r["loss"], 1e-4, U4 * 2.0), "dx": Out(r["dx"], 1e-4, U4 * 2 * dl.double().abs() / nx)}


def l2_host(x, dy, dtype):
    a = x.detach().to(dtype).clone().requires_grad_(True)
    y = F.normalize(a, p=2, dim=1, eps=NORM_EPS)
    y.backward(dy.to(dtype))
    return {"y": y.detach(), "dx": a.grad}


@functools.lru_cache(maxsize=None)
def l2_case(f, b):
    """y = x / max(|x|, eps) is one product per element: no term is added, floor 0 (an all-zero row gives exactly 0).
    dx_r = (dy - y <y, dy>) / max(|x_r|, eps) with |y_i <y, dy>| <= |dy|: floor U4 * |dy_r| / max(|x_r|, eps), |dy_r| the
    row's 2-norm."""
    x, _, _, dy = norm_inputs(f, b)
    r = l2_host(x, dy, torch.float64)
    nx = x.double().norm(dim=1).clamp_min(NORM_EPS)
    return {"y": Out(r["y"], 1e-5, 0.0), "dx": Out(r["dx"], 1e-5, U4 * dy.double().norm(dim=1) / nx)}


# ---------------------------------------------------------------------------------------------------------------------------
# C. pools
# ---------------------------------------------------------------------------------------------------------------------------
POOL_GEOMS = [
    ((2, 3, 4, 6, 6), (3, 3, 3), (2, 2, 2), (1, 1, 1)),
    ((1, 2, 5, 7, 6), (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    ((1, 2, 3, 5, 5), (2, 2, 2), (2, 2, 2), (1, 1, 1)),        # 2p = k: the border windows hold ONE input element per axis
    ((2, 2, 4, 5, 7), (1, 1, 1), (2, 2, 2), (0, 0, 0)),        # stride > kernel: uncovered inputs get gradient exactly 0
    ((1, 2, 6, 8, 9), (3, 3, 3), (3, 3, 3), (0, 0, 0)),        # floor mode leaves the last elements uncovered
]


@functools.lru_cache(maxsize=None)
def pool_inputs(gi, nan=False):
    """Multiples of 0.5 in [-2, 2] (exact in bf16; negative values, zeros, many ties), x[0, 0] all negative: every padded border
    window of that volume must return a negative value, never a padding 0.  dy uniform in (-1, 1) rounded to bf16 (so the fp32
    and the bf16 kernels read the same numbers).  nan: about 2 % NaNs, two of them neighbours (one window holds both)."""
    shape, k, s, p = POOL_GEOMS[gi]
    g = _gen(gi, 5, int(nan))
    x = torch.randint(-4, 5, shape, generator=g).double() * 0.5
    x[0, 0] = -x[0, 0].abs() - 0.5
    if nan:
        flat = x.view(-1)
        pos = torch.randperm(flat.numel(), generator=g)[:max(4, flat.numel() // 50)]
        flat[pos] = float("nan")
        flat[pos[0].clamp(max=flat.numel() - 2) + 1] = float("nan")
    osz = tuple((sz + 2 * p[i] - k[i]) // s[i] + 1 for i, sz in enumerate(shape[2:]))
    dy = (torch.rand(shape[:2] + osz, generator=g, dtype=torch.float64) * 2 - 1).to(torch.bfloat16).double()
    return x, dy


def pool_host(x, dy, k, s, p, dtype, zero_pad=False):
    """(y, dx) of F.max_pool3d in ``dtype``; zero_pad: the NAIVE pool over a zero-padded copy (padding candidates of 0, not -inf)."""
    a = x.detach().to(dtype).clone().requires_grad_(True)
    if zero_pad:
        y = F.max_pool3d(F.pad(a, (p[2], p[2], p[1], p[1], p[0], p[0])), k, s, 0)
    else:
        y = F.max_pool3d(a, k, s, p)
    y.backward(dy.to(dtype))
    return {"y": y.detach(), "dx": a.grad}


@functools.lru_cache(maxsize=None)
def pool_case(gi, nan=False):
    """y exact.  dx of a plane sums at most ceil(k / s)^3 values of dy: floor U4 * max |dy| of the plane."""
    shape, k, s, p = POOL_GEOMS[gi]
    x, dy = pool_inputs(gi, nan)
    r = pool_host(x, dy, k, s, p, torch.float64)
    floor = U4 * dy.abs().reshape(shape[0] * shape[1], -1).amax(dim=1)
    return r["y"], r["dx"], floor


def pool_compare(what, gi, got_y, got_dx, nan=False):
    """-> failures.  y equal to ATen's (same NaN mask, same finite values); dx at 1e-6 globally and per (sample, channel)
    plane, no NaN in it, exactly 0 wherever ATen's is 0 (uncovered inputs, inputs that won no window)."""
    shape = POOL_GEOMS[gi][0]
    y, dx, floor = pool_case(gi, nan)
    gy, gdx = got_y.detach().double().cpu(), got_dx.detach().double().cpu()
    fails = []
    if tuple(gy.shape) != tuple(y.shape):
        return ["%s: y shape %s != %s" % (what, tuple(gy.shape), tuple(y.shape))]
    if nan and not bool(y.isnan().any()):
        fails.append("%s: the case holds no NaN window" % what)
    if not torch.equal(gy.isnan(), y.isnan()) or not torch.equal(torch.nan_to_num(gy, nan=0.0), torch.nan_to_num(y, nan=0.0)):
        fails.append("%s: y differs from ATen's" % what)
    if bool(gdx.isnan().any()) or bool(dx.isnan().any()):
        fails.append("%s: NaN in dx" % what)
    rows = shape[0] * shape[1]
    ge, re = rel_err(gdx, dx), row_err(gdx.reshape(rows, -1), dx.reshape(rows, -1), floor)
    print("EDGE %s dx global=%.3g row=%.3g bar=%g" % (what, ge, re, 1e-6))
    if not ge <= 1e-6:
        fails.append("%s dx: global %.3g > 1e-6" % (what, ge))
    if not re <= 1e-6:
        fails.append("%s dx: row-wise %.3g > 1e-6" % (what, re))
    if not bool((gdx[dx == 0] == 0).all()):
        fails.append("%s dx: nonzero where ATen's gradient is exactly 0" % what)
    return fails


AVG_SHAPES = [(1, 1, 1, 1, 1), (1, 3, 3, 3, 7), (1, 5, 4, 4, 4), (1, 5, 5, 13, 1), (1, 7, 10, 10, 10)]     # s = 1, 63, 64, 65, 1000


@functools.lru_cache(maxsize=None)
def avg_inputs(shape):
    """Even (sample, channel) rows 1000 + U(-1, 1), odd rows U(-1, 1) * 1e-3; dy uniform in (-1, 1)."""
    g = _gen(*shape)
    x = (torch.rand(shape, generator=g) * 2 - 1).float()
    rows = x.view(shape[0] * shape[1], -1)
    rows[0::2] += 1000.0
    rows[1::2] *= 1e-3
    dy = (torch.rand(shape[:2], generator=g) * 2 - 1).float()
    return x, dy


def avg_host(x, dy, dtype):
    a = x.detach().to(dtype).clone().requires_grad_(True)
    y = a.mean(dim=(2, 3, 4))
    y.backward(dy.to(dtype))
    return {"y": y.detach(), "dx": a.grad}


@functools.lru_cache(maxsize=None)
def avg_case(shape):
    """y_r = (sum_i x_ri) / s: the terms added are the x_ri, floor U4 * max_i |x_ri|.  dx_ri = dy_r / s: floor U4 * |dy_r| / s.
    Rows = (sample, channel)."""
    x, dy = avg_inputs(shape)
    r = avg_host(x, dy, torch.float64)
    rows, s = shape[0] * shape[1], shape[2] * shape[3] * shape[4]
    xr = x.double().reshape(rows, s)
    return {"y": Out(r["y"].reshape(rows, 1), 1e-4, U4 * xr.abs().amax(dim=1)),
            "dx": Out(r["dx"].reshape(rows, s), 1e-4, U4 * dy.double().abs().reshape(rows) / s)}


# ---------------------------------------------------------------------------------------------------------------------------
# D. BatchNorm (GPU only: no naive variant)
# ---------------------------------------------------------------------------------------------------------------------------
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def _chan_max(t):
    return t.movedim(1, 0).reshape(t.shape[1], -1).abs().amax(dim=1)


def bn_train_case(x, gamma, beta, res, relu, groups, rm, rv, dy):
    """fp64 truth of ops.batch_norm_act (groups successive F.batch_norm calls, running statistics updated in place group after
    group) and the per-channel floors, all from the fp64 channel statistics:
      y = fma(x, scale, shift) (+ res), scale = gamma * invstd, shift = beta - mean * scale: the terms are |x scale|, |shift|,
          |res| -- they cancel when |mean| >> std -- floor U4 * max over the channel's elements and groups of their sum;
      dx = scale * (g - mean(g) - xhat * mean(g xhat)), g the masked gradient, xhat = (x - mean) * invstd -- itself a difference
          of the terms |x| invstd and |mean| invstd: floor U4 * |scale| * (max |g| + |mean g| + max(|x|, |mean|) * invstd *
          |mean(g xhat)|); the residual's gradient is g itself, a copy: floor 0;
      dgamma = sum g xhat, dbeta = sum g: floors U4 * max |g xhat| and U4 * max |g|;
      running statistics r' = (1 - m) r + m v: floor U4 * max(|r|, |v|) over the groups' updates.
    With ReLU, an element whose pre-activation lies within its own floor of 0 is undecided: either mask is a correct fp32
    result, so y, dx and the residual's gradient are not compared AT that element (Out.undecided; the count is printed).
    -> (outs, rm', rv')."""
    n, c = x.shape[0], x.shape[1]
    half = n // groups
    a = x.double().requires_grad_(True)
    ga, be = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rs = None if res is None else res.double().requires_grad_(True)
    rm2, rv2 = rm.double().clone(), rv.double().clone()
    red = [0] + list(range(2, x.dim()))
    ys, fy, frm, frv, stats = [], torch.zeros(c, dtype=torch.float64), torch.zeros(c, dtype=torch.float64), \
        torch.zeros(c, dtype=torch.float64), []
    for i in range(groups):
        xs = a[i * half:(i + 1) * half]
        mu, var = xs.detach().mean(dim=red), xs.detach().var(dim=red, unbiased=False)
        cnt = xs.numel() // c
        frm = torch.maximum(frm, torch.maximum(rm2.abs(), mu.abs()))
        frv = torch.maximum(frv, torch.maximum(rv2.abs(), (var * cnt / max(cnt - 1, 1)).abs()))
        ys.append(F.batch_norm(xs, rm2, rv2, ga, be, True, BN_MOMENTUM, BN_EPS))
        invstd = 1.0 / torch.sqrt(var + BN_EPS)
        scale = ga.detach() * invstd
        shift = be.detach() - mu * scale
        bshape = [1, c] + [1] * (x.dim() - 2)
        terms = (xs.detach() * scale.view(bshape)).abs() + shift.abs().view(bshape)
        if rs is not None:
            terms = terms + rs.detach()[i * half:(i + 1) * half].abs()
        fy = torch.maximum(fy, _chan_max(terms))
        stats.append((mu, invstd, scale))
    y = torch.cat(ys, 0)
    if rs is not None:
        y = y + rs
    # a ReLU input within its floor of 0: fp32 may mask the element either way (y, dx and the residual's gradient at it)
    near = (y.detach().abs() <= (U4 * fy).view([1, c] + [1] * (x.dim() - 2))) if relu else None
    if relu:
        y = F.relu(y)
    y.backward(dy.double())
    g = dy.double() * ((y.detach() > 0) if relu else torch.ones_like(y, dtype=torch.bool))
    fdx, fdg, fdb = torch.zeros(c, dtype=torch.float64), torch.zeros(c, dtype=torch.float64), torch.zeros(c, dtype=torch.float64)
    for i, (mu, invstd, scale) in enumerate(stats):
        bshape = [1, c] + [1] * (x.dim() - 2)
        gs = g[i * half:(i + 1) * half]
        xh = (x.double()[i * half:(i + 1) * half] - mu.view(bshape)) * invstd.view(bshape)
        mg, mgx = gs.mean(dim=red).abs(), (gs * xh).mean(dim=red).abs()
        xterm = torch.maximum(_chan_max(x.double()[i * half:(i + 1) * half]), mu.abs()) * invstd
        fdx = torch.maximum(fdx, scale.abs() * (_chan_max(gs) + mg + xterm * mgx))
        fdg = torch.maximum(fdg, _chan_max(gs * xh))
        fdb = torch.maximum(fdb, _chan_max(gs))
    outs = {"y": Out(y, 1e-4, U4 * fy, chan=True, undecided=near), "dx": Out(a.grad, 1e-4, U4 * fdx, chan=True, undecided=near),
            "dgamma": Out(ga.grad, 1e-4, U4 * fdg), "dbeta": Out(be.grad, 1e-4, U4 * fdb),
            "running_mean": Out(rm2, 1e-4, U4 * frm), "running_var": Out(rv2, 1e-4, U4 * frv)}
    if rs is not None:
        outs["dres"] = Out(rs.grad, 1e-4, 0.0, chan=True, undecided=near)
    return outs


def bn_eval_case(x, gamma, beta, rm, rv, res, relu):
    """y = x * scale + shift (+ res) with the running statistics; floor as in train mode."""
    c = x.shape[1]
    y = F.batch_norm(x.double(), rm.double(), rv.double(), gamma.double(), beta.double(), False, 0.0, BN_EPS)
    scale = gamma.double() / torch.sqrt(rv.double() + BN_EPS)
    shift = beta.double() - rm.double() * scale
    bshape = [1, c] + [1] * (x.dim() - 2)
    terms = (x.double() * scale.view(bshape)).abs() + shift.abs().view(bshape)
    if res is not None:
        y = y + res.double()
        terms = terms + res.double().abs()
    if relu:
        y = F.relu(y)
    return {"y": Out(y, 1e-5, U4 * _chan_max(terms), chan=True)}


# ---------------------------------------------------------------------------------------------------------------------------
# E. flat-arena kernels
# ---------------------------------------------------------------------------------------------------------------------------
FLAT_TAILS = [1, 2, 3, 4, 5, 255, 257, 1025]
EMA_STRIDE_N = 2048 * 256 * 4 + 3        # one past the single-trip capacity of ema_kernel's grid (2048 blocks of float4 work)
SUMSQ_STRIDE_N = 1024 * 256 * 4 + 1      # ... of sumsq_partial_kernel's (1024 blocks)
STEP_STRIDE_N = 2048 * 256 + 1           # ... of sgd_kernel's and adam_kernel's (2048 blocks, one float per thread)


@functools.lru_cache(maxsize=8)
def flat_inputs(n, seed=0):
    """(t, o, g) fp32 [n]: parameters / EMA target and online weights uniform in (-1, 1), gradients in (-0.05, 0.05)."""
    gen = _gen(n, seed)
    t = (torch.rand((n,), generator=gen) * 2 - 1).float()
    o = (torch.rand((n,), generator=gen) * 2 - 1).float()
    g = ((torch.rand((n,), generator=gen) * 2 - 1) * 0.05).float()
    return t, o, g


def ema_ref(t, o, m, dtype=torch.float64):
    return t.to(dtype) * m + o.to(dtype) * (1.0 - m)


def sgd_ref(p, grads, lr, momentum, wd, coef, dtype=torch.float64):
    """torch.optim.SGD on the CPU, one step per gradient (each scaled by coef first) -> the parameters after the last step."""
    q = torch.nn.Parameter(p.to(dtype).clone())
    opt = torch.optim.SGD([q], lr=lr, momentum=momentum, weight_decay=wd)
    for g in grads:
        q.grad = g.to(dtype) * coef
        opt.step()
    return q.detach()


def adam_ref(p, grads, lr, betas, eps, wd, decoupled, dtype=torch.float64):
    q = torch.nn.Parameter(p.to(dtype).clone())
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([q], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    for g in grads:
        q.grad = g.to(dtype).clone()
        opt.step()
    return q.detach()


CLIP_MAX_NORM = 18.0


def clip_norm_cases():
    """[(sumsq, norm, coef is exactly 1)] in fp32: the sums of squares whose fp32 square root is the float one ulp below and
    one ulp above CLIP_MAX_NORM.  clip_coef computes max_norm / (norm + 1e-6) in fp32 and takes min(., 1)."""
    import numpy as np
    mx, out = np.float32(CLIP_MAX_NORM), []
    for target, one in ((np.nextafter(mx, np.float32(0)), True), (np.nextafter(mx, np.float32(np.inf)), False)):
        cand = np.float32(target * target)
        for _ in range(8):
            r = np.sqrt(cand)
            if r == target:
                break
            cand = np.nextafter(cand, np.float32(np.inf) if r < target else np.float32(0))
        assert np.sqrt(cand) == target and cand.dtype == np.float32
        out.append((float(cand), float(target), one))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# F. convolution bias
# ---------------------------------------------------------------------------------------------------------------------------
BIAS_GEOMS = {
    # name: (x shape, k, kernel, stride, pad)
    "S1": ((2, 64, 4, 14, 14), 144, (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    "stem": ((2, 3, 4, 28, 28), 83, (1, 7, 7), (1, 2, 2), (0, 3, 3)),
    "odd": ((3, 40, 3, 9, 11), 136, (3, 3, 3), (1, 2, 1), (1, 1, 1)),
}
# (geometry, pinned forward tile or None = the default route, split terms or 0 = the default arithmetic)
BIAS_CASES = [("S1", (0, 2, 1, 1), 0), ("S1", (0, 9, 1, 1), 0), ("S1", (1, 4, 0, 0), 0), ("S1", (1, 8, 2, 0), 0),
              ("S1", (1, 4, 0, 0), 3), ("stem", (1, 4, 0, 0), 0), ("odd", None, 0)]


def _urand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1


@functools.lru_cache(maxsize=None)
def bias_case(name):
    """(x, w, b, dy) fp64 and the fp64 F.conv3d truth (y, dx, dw, db), global metric at 1e-4 (the outputs of a convolution are
    sums over the whole reduction: no independent rows)."""
    xs, k, ks, st, pd = BIAS_GEOMS[name]
    x = _urand(xs, 1).requires_grad_(True)
    w = (_urand((k, xs[1]) + ks, 2) * 0.2).requires_grad_(True)
    b = _urand((k,), 4).requires_grad_(True)
    y = F.conv3d(x, w, b, st, pd)
    dy = _urand(tuple(y.shape), 3)
    y.backward(dy)
    outs = {"y": Out(y, 1e-4), "dx": Out(x.grad, 1e-4), "dw": Out(w.grad, 1e-4), "db": Out(b.grad, 1e-4)}
    return x.detach(), w.detach(), b.detach(), dy, outs


CHANNEL_SUM_SHAPES = [(130, 65), (3, 65, 2, 7, 7), (5, 1), (4, 1, 1, 3, 3)]      # s = 1, s = 98, and c = 1 on both paths

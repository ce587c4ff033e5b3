"""The edge cases of tests/ops_edge_cases.py on the CPU, before any GPU run: (1) the fp64 reference is finite wherever the case
says it is, (2) stock PyTorch in fp32 -- the same formula in the kernels' precision -- passes the case's comparator at the
case's bar and floor, so both are attainable, and (3) a deliberately naive variant is REJECTED on the case's inputs, so the
inputs have teeth: softmax without the max-subtraction, max-pool over zero padding, a BYOL gradient with one small row off by
1 % under the global metric alone.  Sections D (BatchNorm) and F (convolution bias) have no naive variant: GPU only."""
import numpy as np
import pytest
import torch

import ops_edge_cases as ec
from conftest import rel_err


def _finite(outs):
    for name, o in outs.items():
        assert bool(torch.isfinite(o.ref).all()), name


# ---- A. softmax heads ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ec.CE_PATTERNS)
@pytest.mark.parametrize("b,k", ec.CE_SHAPES)
def test_cross_entropy_cases(b, k, pattern):
    z, lab, _, _ = ec.ce_inputs(b, k, pattern)
    assert float(z[0].max()) >= 100.0 and (b < 3 or float(z[1].max()) <= -100.0)      # (with b = 2 row 1 is the last row: it carries the pattern)
    outs = ec.ce_case(b, k, pattern)
    _finite(outs)
    q = ec.q64(lab, lab, torch.ones(b), 0.0, k)
    what = "host ce b%d k%d %s" % (b, k, pattern)
    if pattern == "neginf" and k > 1:
        # (a soft-target formula multiplies q = 0 into log_softmax = -inf: the stock hard-label entry point is the formula here)
        x = z.detach().clone().requires_grad_(True)
        loss = torch.nn.functional.cross_entropy(x, lab)
        (loss * ec.DLOSS).backward()
        stock = {"loss": loss.detach(), "dlogits": x.grad}
    else:
        stock = ec.softmax_host(z, q, naive=False)
    assert ec.compare(what + " fp32", outs, stock) == []
    if not (pattern == "neginf" and k > 1):
        assert ec.compare(what + " naive", outs, ec.softmax_host(z, q, naive=True)) != []


@pytest.mark.parametrize("pattern", [p for p in ec.CE_PATTERNS if p != "neginf"])
@pytest.mark.parametrize("b,k", ec.CE_SHAPES)
def test_soft_cross_entropy_cases(b, k, pattern):
    z, ta, tb, lam = ec.ce_inputs(b, k, pattern)
    for eps, mixed in ec.SOFT_VARIANTS:
        outs = ec.soft_ce_case(b, k, pattern, eps, mixed)
        _finite(outs)
        q = ec.q64(ta, tb if mixed else ta, lam if mixed else torch.ones(b), eps, k)
        what = "host soft_ce b%d k%d %s eps%g mixed%d" % (b, k, pattern, eps, mixed)
        assert ec.compare(what + " fp32", outs, ec.softmax_host(z, q, naive=False)) == []
        assert ec.compare(what + " naive", outs, ec.softmax_host(z, q, naive=True)) != []


@pytest.mark.parametrize("n,f,tau", ec.NTX_CASES + [(3, 2049, 0.1)])
def test_ntxent_cases(n, f, tau):
    zi, zj = ec.ntx_inputs(n, f)
    assert torch.equal(zi[1], zj[1]) and (n < 3 or torch.equal(zi[2], zj[0]))
    outs = ec.ntx_case(n, f, tau)
    _finite(outs)
    what = "host ntxent n%d f%d tau%g" % (n, f, tau)
    assert ec.compare(what + " fp32", outs, ec.ntx_host(zi, zj, tau, torch.float32)) == []
    if 1.0 / tau > 89.0:            # sim / tau reaches +-1 / tau: only these cases can overflow expf, the others have no naive failure
        assert ec.compare(what + " naive", outs, ec.ntx_host(zi, zj, tau, torch.float32, naive=True)) != []


def test_probe_step_case():
    import probe_spec
    case, ref = ec.probe_case()
    assert float(np.abs(ref["logits"]).max()) > 88.0 and np.isfinite(ref["loss"]) and np.isfinite(ref["dw"]).all()
    assert ec.probe_compare("host probe fp32", ref, *ec.probe_host(case, naive=False)) == []
    assert ec.probe_compare("host probe naive", ref, *ec.probe_host(case, naive=True)) != []
    assert probe_spec.LOSS_RTOL == 6e-7 and probe_spec.GRAD_RTOL == 1.9e-6          # the bars of tests/test_probe_gpu.py


# ---- B. row-normalising ops ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", ec.NORM_B)
@pytest.mark.parametrize("f", ec.NORM_F)
def test_byol_cases(f, b):
    x, t, dl, _ = ec.norm_inputs(f, b)
    outs = ec.byol_case(f, b)
    _finite(outs)
    if b == "special":
        that = t[0].double() / t[0].double().norm()
        assert float(outs["loss"].ref[0]) == 2.0 and float(outs["loss"].ref[1]) == 2.0
        assert rel_err(outs["dx"].ref[0], -2 * float(dl[0]) * that / ec.NORM_EPS) < 1e-12
        assert float(outs["dx"].ref[1].abs().max()) == 0.0
    what = "host byol f%d b%s" % (f, b)
    stock = ec.byol_host(x, t, dl, torch.float32)
    assert ec.compare(what + " fp32", outs, stock) == []
    # one small row off by 1 %: the global metric alone lets it through (with more than one row), the row-wise one does not
    nz = outs["dx"].ref.abs().amax(dim=1)
    r = int(torch.where(nz > 0, nz, torch.full_like(nz, float("inf"))).argmin())
    bad = {"loss": stock["loss"], "dx": stock["dx"].clone()}
    bad["dx"][r] *= 1.01
    if bad["dx"].shape[0] > 1:
        assert rel_err(bad["dx"], outs["dx"].ref) < 1e-4
    fails = ec.compare(what + " perturbed", outs, bad)
    assert fails != [] and all("row-wise" in m or bad["dx"].shape[0] == 1 for m in fails)


@pytest.mark.parametrize("b", ec.NORM_B)
@pytest.mark.parametrize("f", ec.NORM_F)
def test_l2_normalize_cases(f, b):
    x, _, _, dy = ec.norm_inputs(f, b)
    outs = ec.l2_case(f, b)
    _finite(outs)
    if b == "special":
        assert float(outs["y"].ref[0].abs().max()) == 0.0
        assert rel_err(outs["dx"].ref[0], dy[0].double() / ec.NORM_EPS) < 1e-12
    assert ec.compare("host l2 f%d b%s fp32" % (f, b), outs, ec.l2_host(x, dy, torch.float32)) == []


# ---- C. pools --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gi,nan", [(gi, False) for gi in range(len(ec.POOL_GEOMS))] + [(0, True)])
def test_max_pool_cases(gi, nan):
    shape, k, s, p = ec.POOL_GEOMS[gi]
    x, dy = ec.pool_inputs(gi, nan)
    y, dx, _ = ec.pool_case(gi, nan)
    assert bool(torch.isfinite(dx).all()) and (nan or bool(torch.isfinite(y).all()))
    if not nan and any(p):
        assert float(y[0, 0].max()) < 0.0           # the all-negative volume: no window returns a padding value
    stock = ec.pool_host(x, dy, k, s, p, torch.float32)
    assert ec.pool_compare("host pool g%d nan%d fp32" % (gi, nan), gi, stock["y"], stock["dx"], nan) == []
    if any(p) and not nan:                          # (without padding the zero-padded pool IS the pool: nothing to reject)
        naive = ec.pool_host(x, dy, k, s, p, torch.float32, zero_pad=True)
        assert ec.pool_compare("host pool g%d naive" % gi, gi, naive["y"], naive["dx"]) != []


@pytest.mark.parametrize("shape", ec.AVG_SHAPES)
def test_avg_pool_cases(shape):
    x, dy = ec.avg_inputs(shape)
    outs = ec.avg_case(shape)
    _finite(outs)
    rows = shape[0] * shape[1]
    r = ec.avg_host(x, dy, torch.float32)
    got = {"y": r["y"].reshape(rows, 1), "dx": r["dx"].reshape(rows, -1)}
    assert ec.compare("host avgpool %s fp32" % (shape,), outs, got) == []


# ---- E. flat-arena kernels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ec.FLAT_TAILS + [ec.STEP_STRIDE_N])
def test_flat_cases(n):
    t, o, g = ec.flat_inputs(n)
    ref = ec.ema_ref(t, o, 0.996)
    assert bool(torch.isfinite(ref).all())
    assert rel_err(ec.ema_ref(t, o, 0.996, torch.float32), ref) < 1e-6
    nrm = g.double().norm()
    got = (g.double() ** 2).sum().float().sqrt()              # the kernels' formula: fp64 partial sums, an fp32 square root
    assert abs(float(got) - float(nrm)) <= 1e-6 * float(nrm)
    for momentum, wd, coef in ((0.9, 5e-4, 0.37), (0.0, 5e-4, 1.0), (0.9, 0.0, 0.37)):
        ref = ec.sgd_ref(t, [g, o * 0.05], 0.05, momentum, wd, coef)
        assert rel_err(ec.sgd_ref(t, [g, o * 0.05], 0.05, momentum, wd, coef, torch.float32), ref) < 1e-6
    for decoupled in (False, True):
        ref = ec.adam_ref(t, [g, o * 0.05], 0.01, (0.9, 0.99), 1e-8, 5e-2, decoupled)
        assert rel_err(ec.adam_ref(t, [g, o * 0.05], 0.01, (0.9, 0.99), 1e-8, 5e-2, decoupled, torch.float32), ref) < 1e-5


def test_clip_coef_ulp_cases():
    """One ulp below max_norm the coefficient is exactly 1, one ulp above it is below 1, in fp32 as the kernel computes it."""
    for _, nrm, want_one in ec.clip_norm_cases():
        c = np.float32(ec.CLIP_MAX_NORM) / (np.float32(nrm) + np.float32(1e-6))
        assert (min(float(c), 1.0) == 1.0) == want_one


def test_bn1d_backward_entry_point_fails_cleanly_before_any_hip_call():
    """cstp_bn1d_backward (the fp64 BatchNorm1d backward that section D's two-value case needs): its precondition checks."""
    import ctypes
    from cstp_amd import _lib
    lib = _lib.load()
    one, f = ctypes.c_void_p(8), ctypes.c_float          # any non-null address: never dereferenced before the checks fail
    for args, needle in (((None,) * 9 + (4, 8, 1, f(1e-5), 0, 0), b"null argument"),
                         ((None, one, None, one, one, one, None, one, one, 4, 8, 1, f(1e-5), 1, 0), b"ReLU mask needs y"),
                         ((None, one, one, one, one, one, None, one, one, 4, 8, 3, f(1e-5), 1, 0), b"bad shape")):
        rc = lib.cstp_bn1d_backward(*args)
        assert rc != 0 and needle in lib.cstp_last_error()

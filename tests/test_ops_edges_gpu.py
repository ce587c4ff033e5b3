"""The first-generation ops at their edges: the loss heads, pools and flat-arena kernels of csrc/misc.hip, the train and eval
BatchNorm of csrc/bn.hip and the convolution bias path, through cstp_amd.ops against the fp64 references of
tests/ops_edge_cases.py (inputs, floors and comparators are documented there; tests/test_ops_edges_host.py proves on the CPU
that stock fp32 passes them and that naive variants do not).  Every case prints its measured global and row-wise error."""
import ctypes

import pytest
import torch

import ops_edge_cases as ec
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---------------------------------------------------------------------------------------------------------------------------
# A. softmax heads
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ec.CE_PATTERNS)
@pytest.mark.parametrize("b,k", ec.CE_SHAPES)
def test_cross_entropy_edges(b, k, pattern):
    from cstp_amd import ops
    z, lab, _, _ = ec.ce_inputs(b, k, pattern)
    x = z.to(DEV).requires_grad_(True)
    loss = ops.cross_entropy(x, lab.to(DEV))
    (loss * ec.DLOSS).backward()
    got = {"loss": loss.detach(), "dlogits": x.grad}
    assert ec.compare("A ce b%d k%d %s" % (b, k, pattern), ec.ce_case(b, k, pattern), got) == []


@pytest.mark.parametrize("pattern", [p for p in ec.CE_PATTERNS if p != "neginf"])
@pytest.mark.parametrize("b,k", ec.CE_SHAPES)
def test_soft_cross_entropy_edges(b, k, pattern):
    from cstp_amd import ops
    z, ta, tb, lam = ec.ce_inputs(b, k, pattern)
    fails = []
    for eps, mixed in ec.SOFT_VARIANTS:
        x = z.to(DEV).requires_grad_(True)
        loss = ops.soft_cross_entropy(x, ta.to(DEV), tb.to(DEV) if mixed else None, lam.to(DEV) if mixed else None, eps)
        (loss * ec.DLOSS).backward()
        got = {"loss": loss.detach(), "dlogits": x.grad}
        fails += ec.compare("A soft_ce b%d k%d %s eps%g mixed%d" % (b, k, pattern, eps, mixed),
                            ec.soft_ce_case(b, k, pattern, eps, mixed), got)
    assert fails == []


@pytest.mark.parametrize("n,f,tau", ec.NTX_CASES)
def test_ntxent_edges(n, f, tau):
    from cstp_amd import ops
    zi, zj = ec.ntx_inputs(n, f)
    reps = torch.cat([zj, zi], 0).to(DEV).requires_grad_(True)
    loss = ops.ntxent(reps, tau)
    (loss * ec.DLOSS).backward()
    got = {"loss": loss.detach(), "dreps": reps.grad}
    assert ec.compare("A ntxent n%d f%d tau%g" % (n, f, tau), ec.ntx_case(n, f, tau), got) == []


def test_ntxent_past_the_backward_limit():
    """f = 2049: the forward has no limit and matches; the backward (8 features per thread of a 256-thread block) refuses."""
    from cstp_amd import _lib, ops
    n, f, tau = 3, 2049, 0.1
    zi, zj = ec.ntx_inputs(n, f)
    reps = torch.cat([zj, zi], 0).to(DEV).requires_grad_(True)
    loss = ops.ntxent(reps, tau)
    outs = ec.ntx_case(n, f, tau)
    assert ec.compare("A ntxent n3 f2049 forward", {"loss": outs["loss"]}, {"loss": loss.detach()}) == []
    with pytest.raises(_lib.CstpError):
        loss.backward()


def test_probe_step_large_logits():
    from cstp_amd import ops
    case, ref = ec.probe_case()
    d = lambda a: torch.from_numpy(a).to(DEV)
    loss, hits, dw, db = ops.probe_step(d(case["x"]), d(case["labels"]), d(case["w"]), d(case["b"]))
    assert ec.probe_compare("A probe_step", ref, float(loss), dw.cpu().numpy(), db.cpu().numpy()) == []
    assert abs(int(hits) - ref["hits"]) <= int(ref["near_top1"].sum())


# ---------------------------------------------------------------------------------------------------------------------------
# B. row-normalising ops
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", ec.NORM_B)
@pytest.mark.parametrize("f", ec.NORM_F)
def test_byol_loss_edges(f, b):
    from cstp_amd import ops
    x, t, dl, _ = ec.norm_inputs(f, b)
    xg = x.to(DEV).requires_grad_(True)
    loss = ops.byol_regression_loss(xg, t.to(DEV))
    loss.backward(dl.to(DEV))
    assert ec.compare("B byol f%d b%s" % (f, b), ec.byol_case(f, b), {"loss": loss.detach(), "dx": xg.grad}) == []


@pytest.mark.parametrize("b", ec.NORM_B)
@pytest.mark.parametrize("f", ec.NORM_F)
def test_l2_normalize_edges(f, b):
    from cstp_amd import ops
    x, _, _, dy = ec.norm_inputs(f, b)
    xg = x.to(DEV).requires_grad_(True)
    y = ops.l2_normalize(xg, ec.NORM_EPS)
    y.backward(dy.to(DEV))
    assert ec.compare("B l2 f%d b%s" % (f, b), ec.l2_case(f, b), {"y": y.detach(), "dx": xg.grad}) == []


# ---------------------------------------------------------------------------------------------------------------------------
# C. pools
# ---------------------------------------------------------------------------------------------------------------------------
def _pool_hip(gi, nan, dtype):
    from cstp_amd import ops
    _, k, s, p = ec.POOL_GEOMS[gi]
    x, dy = ec.pool_inputs(gi, nan)
    xg = x.to(dtype).to(DEV).requires_grad_(True)
    y = ops.max_pool3d(xg, k, s, p)
    y.backward(dy.to(dtype).to(DEV))
    return y.detach(), xg.grad


@pytest.mark.parametrize("gi,nan", [(gi, False) for gi in range(len(ec.POOL_GEOMS))] + [(0, True)])
def test_max_pool3d_edges(gi, nan):
    y, dx = _pool_hip(gi, nan, torch.float32)
    assert y.dtype == torch.float32
    assert ec.pool_compare("C max_pool3d g%d nan%d fp32" % (gi, nan), gi, y, dx, nan) == []
    y2, dx2 = _pool_hip(gi, nan, torch.float32)
    assert torch.equal(y.view(torch.int32), y2.view(torch.int32)) and torch.equal(dx.view(torch.int32), dx2.view(torch.int32))


@pytest.mark.parametrize("gi,nan", [(gi, False) for gi in range(len(ec.POOL_GEOMS))] + [(0, True)])
def test_max_pool3d_bf16_edges(gi, nan):
    """The inputs are exact in bf16, so y is ATen's bit for bit; dx is the correctly rounded sum (check_rounded)."""
    from test_b16_gpu import check_rounded
    y, dx = _pool_hip(gi, nan, torch.bfloat16)
    assert y.dtype == torch.bfloat16 and dx.dtype == torch.bfloat16
    yr, dxr, _ = ec.pool_case(gi, nan)
    yc = y.double().cpu()
    assert torch.equal(yc.isnan(), yr.isnan()) and torch.equal(torch.nan_to_num(yc, nan=0.0), torch.nan_to_num(yr, nan=0.0))
    assert not bool(dx.isnan().any())
    check_rounded(dx, dxr, "C max_pool3d g%d nan%d bf16 dx" % (gi, nan))
    assert bool((dx.double().cpu()[dxr == 0] == 0).all())
    y2, dx2 = _pool_hip(gi, nan, torch.bfloat16)
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16)) and torch.equal(dx.view(torch.int16), dx2.view(torch.int16))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_max_pool3d_rejects_padding_past_half_the_kernel(dtype):
    from cstp_amd import _lib, ops
    x = torch.zeros((1, 1, 4, 4, 4), device=DEV, dtype=dtype)
    with pytest.raises(_lib.CstpError):
        ops.max_pool3d(x, 2, 2, 2)
    with pytest.raises(_lib.CstpError):
        ops.max_pool3d(x, (3, 3, 3), 1, (1, 2, 1))


@pytest.mark.parametrize("shape", ec.AVG_SHAPES)
def test_global_avg_pool_edges(shape):
    from cstp_amd import ops
    x, dy = ec.avg_inputs(shape)
    rows = shape[0] * shape[1]
    xg = x.to(DEV).requires_grad_(True)
    y = ops.global_avg_pool(xg)
    assert tuple(y.shape) == shape[:2]
    y.backward(dy.to(DEV))
    got = {"y": y.detach().reshape(rows, 1), "dx": xg.grad.reshape(rows, -1)}
    assert ec.compare("C avgpool %s" % (shape,), ec.avg_case(shape), got) == []


# ---------------------------------------------------------------------------------------------------------------------------
# D. BatchNorm
# ---------------------------------------------------------------------------------------------------------------------------
def _bn_run(what, x, gamma, beta, res, relu, groups, rm, rv, dy, place=lambda t: t.to(DEV)):
    """ops.batch_norm_act forward and backward against ec.bn_train_case; ``place`` puts x / res / dy on the device."""
    from cstp_amd import ops
    outs = ec.bn_train_case(x, gamma, beta, res, relu, groups, rm, rv, dy)
    xg = place(x).requires_grad_(True)
    gg, bg = gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
    rg = None if res is None else place(res).requires_grad_(True)
    rmg, rvg = rm.to(DEV), rv.to(DEV)
    y = ops.batch_norm_act(xg, gg, bg, rmg, rvg, rg, relu, groups=groups)
    y.backward(place(dy))
    got = {"y": y.detach(), "dx": xg.grad, "dgamma": gg.grad, "dbeta": bg.grad, "running_mean": rmg, "running_var": rvg}
    if rg is not None:
        got["dres"] = rg.grad
    return ec.compare(what, outs, got)


def _bn_tensors(shape, seed, scales=None):
    g = torch.Generator().manual_seed(seed)
    c = shape[1]
    r = lambda s: (torch.rand(s, generator=g) * 2 - 1).float()
    x = r(shape) * 2 + 0.5
    gamma, beta = r((c,)), r((c,)) * 0.1
    if scales is not None:
        x = x * torch.tensor(scales).float().view([1, c] + [1] * (len(shape) - 2))
    return x, gamma, beta, r(shape), r((c,)) * 0.1, r((c,)).abs() + 0.5, r(shape)


BN_VARIANTS = [(False, False), (False, True), (True, False), (True, True)]       # (residual, relu)


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("use_res,relu", BN_VARIANTS)
def test_bn_constant_channel(use_res, relu, groups):
    """Channel 0 is constant (0.5) in the first half of the batch and ordinary in the second: with groups = 2 its variance in
    group 0 is exactly 0 (the clamp at 0 applies, invstd = 1 / sqrt(eps) = 316), xhat and dgamma's share of it are exactly 0."""
    shape = (4, 3, 2, 3, 3)
    x, gamma, beta, res, rm, rv, dy = _bn_tensors(shape, 61)
    x[:2, 0] = 0.5
    beta[0] = 0.05                   # (away from 0: the ReLU mask of y = beta + cancellation noise must not be a coin toss)
    assert _bn_run("D bn constant res%d relu%d g%d" % (use_res, relu, groups), x, gamma, beta, res if use_res else None, relu,
                   groups, rm, rv, dy) == []


@pytest.mark.parametrize("shape,groups", [((2, 3, 1, 1, 2), 1), ((4, 5), 1), ((2, 1, 1, 1, 2), 1),
                                          ((2, 2048, 1, 1, 2), 1), ((2, 2049, 1, 1, 2), 1), ((4, 2049, 1, 1, 2), 2)],
                         ids=lambda v: str(v))
def test_bn_minimum_count_and_nsplit_boundary(shape, groups):
    """Four values per channel, and c = 1 / 2048 / 2049: bn_nsplit = cdiv(2048, c) drops from 2 to 1."""
    x, gamma, beta, res, rm, rv, dy = _bn_tensors(shape, 62 + shape[1])
    fails = []
    for use_res, relu in ((False, False), (True, True)):
        fails += _bn_run("D bn min %s g%d res%d relu%d" % (shape, groups, use_res, relu), x, gamma, beta, res if use_res else None,
                         relu, groups, rm, rv, dy)
    assert fails == []


@pytest.mark.parametrize("shape,groups", [((2, 5), 1), ((4, 5), 2)], ids=lambda v: str(v))
def test_bn1d_two_values_per_channel(shape, groups):
    """BatchNorm1d at its minimum count, two values per channel and group.  With two values x1, x2 of a channel xhat = +-h,
    h^2 = var / (var + eps), and
        dx1 = -dx2 = gamma invstd (g1 - g2) / 2 * (1 - h^2) = gamma invstd (g1 - g2) / 2 * eps / (var + eps),
    the difference of two terms that agree to eps / var = 1e-5 .. 1e-4 of their size in EVERY channel, so the global metric has
    no large channel to hide behind.  An fp32 evaluation keeps 2^-24 / (eps / var) = 1e-3 .. 1e-2 of that difference whatever
    the order of its operations, and so does any evaluation from an invstd saved in fp32: the former fp32 backward
    measured 1.7e-3 .. 2.7e-3 here against the bar 1e-4, stock PyTorch fp32 on the CPU 9.3e-4.  ops routes
    BatchNorm1d's backward to cstp_bn1d_backward, which rebuilds the statistics from x and eps and forms dx in fp64."""
    x, gamma, beta, res, rm, rv, dy = _bn_tensors(shape, 62 + shape[1])
    fails = []
    for use_res, relu in ((False, False), (True, True)):
        fails += _bn_run("D bn1d two values %s g%d res%d relu%d" % (shape, groups, use_res, relu), x, gamma, beta,
                         res if use_res else None, relu, groups, rm, rv, dy)
    assert fails == []


@pytest.mark.parametrize("shape,groups", [((4, 7, 2, 3, 3), 1), ((4, 7, 2, 3, 3), 2), ((4, 7, 1, 68, 68), 1), ((6, 7), 1)],
                         ids=lambda v: str(v))
def test_bn_channel_scales(shape, groups):
    """Channels scaled by 10^-3 .. 10^3 with gamma of mixed sign: dx differs by 10^6 between channels, so the global metric sees
    the 10^-3 channel only.  (4, 7, 1, 68, 68): past the single-launch kernels, the float4 three-launch sequence."""
    x, gamma, beta, res, rm, rv, dy = _bn_tensors(shape, 63, scales=[10.0 ** e for e in range(-3, 4)])
    assert bool((gamma > 0).any()) and bool((gamma < 0).any())
    fails = []
    for use_res, relu in BN_VARIANTS:
        fails += _bn_run("D bn scales %s g%d res%d relu%d" % (shape, groups, use_res, relu), x, gamma, beta,
                         res if use_res else None, relu, groups, rm, rv, dy)
    assert fails == []


def _offset_view(t, o):
    """A contiguous device view of t's values at a storage offset of o floats (4 o bytes past a 16-byte aligned allocation)."""
    buf = torch.empty(t.numel() + 4, device=DEV, dtype=torch.float32)
    v = buf[o:o + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * o) % 16
    return v


# (4, 6, 2, 4, 4): the single-launch kernels (scalar accesses); (4, 6, 2, 68, 68): s = 9248, a multiple of 4 past their limit for
# groups 1 and 2 -- the reduce and apply kernels that come as a float4 and a scalar variant
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("shape", [(4, 6, 2, 4, 4), (4, 6, 2, 68, 68)], ids=lambda v: str(v))
def test_bn_misaligned_views(shape, offset, groups):
    """x, residual and dy as contiguous views 4, 8 and 12 bytes past a 16-byte boundary: s % 4 == 0 alone must not select the
    float4 kernels (bn.hip requires every tensor pointer of the call 16-byte aligned, as mixed.hip and gate.hip do)."""
    x, gamma, beta, res, rm, rv, dy = _bn_tensors(shape, 64)
    fails = []
    for use_res, relu in ((True, True), (False, True), (False, False)):
        fails += _bn_run("D bn misaligned %s o%d g%d res%d relu%d" % (shape, offset, groups, use_res, relu), x, gamma, beta,
                         res if use_res else None, relu, groups, rm, rv, dy, place=lambda t: _offset_view(t, offset))
    assert fails == []


@pytest.mark.parametrize("offset", [0, 1, 3])
@pytest.mark.parametrize("s", [1, 5, 8])
def test_bn_eval_edges(s, offset):
    """running_var = 0 in channel 1 (invstd = 1 / sqrt(eps)); s = 1 (BatchNorm1d), 5 (scalar) and 8 (float4, unless the view
    is misaligned)."""
    from cstp_amd import ops
    shape = (3, 4) if s == 1 else (3, 4, 1, 1, s)
    x, gamma, beta, res, rm, rv, _ = _bn_tensors(shape, 65 + s)
    rv[1] = 0.0
    fails = []
    for use_res, relu in ((False, False), (True, True)):
        outs = ec.bn_eval_case(x, gamma, beta, rm, rv, res if use_res else None, relu)
        with torch.no_grad():
            y = ops.batch_norm_eval(_offset_view(x, offset), gamma.to(DEV), beta.to(DEV), rm.to(DEV), rv.to(DEV),
                                    _offset_view(res, offset) if use_res else None, relu)
        fails += ec.compare("D bn eval s%d o%d res%d relu%d" % (s, offset, use_res, relu), outs, {"y": y})
    assert fails == []


# ---------------------------------------------------------------------------------------------------------------------------
# E. flat-arena kernels
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ec.FLAT_TAILS + [ec.EMA_STRIDE_N])
def test_ema_update_edges(n):
    from cstp_amd import ops
    t, o, _ = ec.flat_inputs(n)
    tg = t.to(DEV)
    ops.ema_update_(tg, o.to(DEV), 0.996)
    e = rel_err(tg, ec.ema_ref(t, o, 0.996))
    print("EDGE E ema n%d global=%.3g bar=1e-06" % (n, e))
    assert e < 1e-6


@pytest.mark.parametrize("n", ec.FLAT_TAILS + [ec.SUMSQ_STRIDE_N])
def test_grad_sumsq_edges(n):
    from cstp_amd import ops
    _, _, g = ec.flat_inputs(n)
    ss, coef, nrm = (torch.zeros(1, device=DEV) for _ in range(3))
    ops.grad_sumsq(g.to(DEV), ss)
    ops.clip_coef(ss, 0.01, coef, nrm)
    ref = float(g.double().norm())
    e = abs(float(nrm) - ref) / ref
    print("EDGE E sumsq n%d global=%.3g bar=1e-06" % (n, e))
    assert e < 1e-6
    assert abs(float(coef) - min(1.0, 0.01 / (ref + 1e-6))) < 1e-6


def test_clip_coef_edges():
    """An all-zero gradient: norm 0 and coefficient exactly 1.  A norm one ulp below max_norm: exactly 1; one ulp above: < 1."""
    from cstp_amd import ops
    ss, coef, nrm = (torch.zeros(1, device=DEV) for _ in range(3))
    ops.grad_sumsq(torch.zeros(1025, device=DEV), ss)
    ops.clip_coef(ss, ec.CLIP_MAX_NORM, coef, nrm)
    assert float(ss) == 0.0 and float(nrm) == 0.0 and float(coef) == 1.0
    for sumsq, norm, one in ec.clip_norm_cases():
        ops.clip_coef(torch.full((1,), sumsq, device=DEV), ec.CLIP_MAX_NORM, coef, nrm)
        assert float(nrm) == norm
        assert (float(coef) == 1.0) if one else (float(coef) < 1.0)
        ops.clip_coef(torch.full((1,), sumsq, device=DEV), ec.CLIP_MAX_NORM, coef, None)       # the norm is optional
        assert (float(coef) == 1.0) if one else (float(coef) < 1.0)


@pytest.mark.parametrize("momentum,wd,use_coef", [(0.9, 5e-4, True), (0.0, 5e-4, True), (0.9, 0.0, True), (0.9, 5e-4, False)])
@pytest.mark.parametrize("n", ec.FLAT_TAILS + [ec.STEP_STRIDE_N])
def test_sgd_step_edges(n, momentum, wd, use_coef):
    """Two steps (first_step true, then false) against torch.optim.SGD on the CPU in fp64; the gradient is written back scaled
    by the coefficient, or left bit-identical with write_back_grad=False."""
    from cstp_amd import ops
    t, o, g = ec.flat_inputs(n)
    grads, c = [g, o * 0.05], 0.37 if use_coef else 1.0
    ref = ec.sgd_ref(t, grads, 0.05, momentum, wd, c)
    coef = torch.full((1,), c, device=DEV) if use_coef else None
    lr = torch.full((1,), 0.05, device=DEV)
    for write_back in (True, False):
        pg, buf = t.to(DEV), torch.zeros(n, device=DEV)
        for step, gr in enumerate(grads):
            gg = gr.to(DEV)
            ops.sgd_step_(pg, gg, buf, lr, momentum, wd, coef, step == 0, write_back)
            if write_back:
                assert rel_err(gg, gr.double() * c) < 1e-6
            else:
                assert torch.equal(gg.view(torch.int32).cpu(), gr.view(torch.int32))
        e = rel_err(pg, ref)
        print("EDGE E sgd n%d m%g wd%g coef%d wb%d global=%.3g bar=1e-06" % (n, momentum, wd, use_coef, write_back, e))
        assert e < 1e-6


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("n", ec.FLAT_TAILS + [ec.STEP_STRIDE_N])
def test_adam_step_edges(n, decoupled):
    from cstp_amd import ops
    t, o, g = ec.flat_inputs(n)
    grads = [g, o * 0.05]
    ref = ec.adam_ref(t, grads, 0.01, (0.9, 0.99), 1e-8, 5e-2, decoupled)
    pg, m, v = t.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    lr = torch.full((1,), 0.01, device=DEV)
    for step, gr in enumerate(grads):
        ops.adam_step_(pg, gr.to(DEV), m, v, lr, 0.9, 0.99, 1e-8, 5e-2, decoupled, step + 1)
    e = rel_err(pg, ref)
    print("EDGE E adam n%d decoupled%d global=%.3g bar=1e-05" % (n, decoupled, e))
    assert e < 1e-5


def test_flat_kernels_refuse_misaligned_arenas():
    """A view at a 4-byte offset: CstpError ("16-byte aligned") and nothing is written."""
    from cstp_amd import _lib, ops
    buf, other = torch.ones(1029, device=DEV), torch.full((1028,), 2.0, device=DEV)
    with pytest.raises(_lib.CstpError, match="16-byte aligned"):
        ops.ema_update_(buf[1:1029], other, 0.5)
    with pytest.raises(_lib.CstpError, match="16-byte aligned"):
        ops.ema_update_(other, buf[1:1029], 0.5)
    ss = torch.full((1,), 7.0, device=DEV)
    with pytest.raises(_lib.CstpError, match="16-byte aligned"):
        ops.grad_sumsq(buf[1:1029], ss)
    torch.cuda.synchronize()
    assert float(ss) == 7.0 and bool((buf == 1.0).all()) and bool((other == 2.0).all())


# ---------------------------------------------------------------------------------------------------------------------------
# F. convolution bias
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tile,terms", ec.BIAS_CASES, ids=lambda v: str(v))
def test_conv3d_bias_edges(name, tile, terms):
    """y, dx, dw and db with a bias that requires a gradient, on the native epilogues, the split tiles, the stem kernel and
    the default route.  The forward pin that was there (if any) and the arithmetic are restored."""
    from cstp_amd import _lib, ops
    xs, k, ks, st, pd = ec.BIAS_GEOMS[name]
    x, w, b, dy, outs = ec.bias_case(name)
    lib = _lib.load()
    desc = ops._desc(xs, tuple(w.shape), st, pd)
    if terms:
        ops.set_split_terms(terms)
    before = (ctypes.c_int32 * 4)()
    _lib.check(lib.cstp_conv3d_get_tile(ctypes.byref(desc), 0, before), "get")
    try:
        if tile is not None:
            ops.set_conv_tile(xs, tuple(w.shape), st, pd, 0, tile)
        xg, wg, bg = (t.float().to(DEV).requires_grad_(True) for t in (x, w, b))
        y = ops.conv3d(xg, wg, bg, st, pd)
        y.backward(dy.float().to(DEV))
        ops._join_side_streams()
        torch.cuda.synchronize()
        got = {"y": y.detach(), "dx": xg.grad, "dw": wg.grad, "db": bg.grad}
        assert ec.compare("F conv bias %s tile%s terms%d" % (name, tile, terms), outs, got) == []
    finally:
        if tile is not None and before[0] != -1:
            ops.set_conv_tile(xs, tuple(w.shape), st, pd, 0, list(before))
        if terms:
            ops.set_split_terms(0)


@pytest.mark.parametrize("shape", ec.CHANNEL_SUM_SHAPES, ids=lambda v: str(v))
def test_channel_sum_edges(shape):
    """db alone: cstp_channel_sum's s == 1 path (a thread per channel) and s > 1 path (a block per channel), called as
    _Conv3d.backward calls it."""
    from cstp_amd import _lib, ops
    g = torch.Generator().manual_seed(66 + len(shape))
    dy = (torch.rand(shape, generator=g) * 2 - 1).float()
    n, c = shape[0], shape[1]
    ref = dy.double().sum(dim=[0] + list(range(2, len(shape))))
    dyg, db = dy.to(DEV), torch.full((c,), float("nan"), device=DEV)
    _lib.check(_lib.load().cstp_channel_sum(ops._stream(), dyg.data_ptr(), db.data_ptr(), n, c, dy.numel() // (n * c), None, 0),
               "cstp_channel_sum")
    # each channel is its own sum: floor U4 * max |dy| of the channel (the kernel accumulates in fp64 and rounds once)
    floor = ec.U4 * dy.double().movedim(1, 0).reshape(c, -1).abs().amax(dim=1)
    outs = {"db": ec.Out(ref.reshape(c, 1), 1e-4, floor)}
    assert ec.compare("F channel_sum %s" % (shape,), outs, {"db": db.reshape(c, 1)}) == []

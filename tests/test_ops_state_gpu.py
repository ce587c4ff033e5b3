"""Nothing an op call or a backward pass of cstp_amd.ops sets up outlives that call or that pass, whether it succeeds or raises:
the side data of a call (the statistics a convolution leaves for its BatchNorm, the absmax cell of a result) travels in a
per-call record and in tags on the result tensor, a residual join (GradJoin) and the weight-gradient side stream's join belong
to the backward pass that opened them.  Every exception below is a host-side Python exception -- ``Boom.backward`` or argument
validation; every tile is pinned, so nothing is timed."""
import pytest
import torch

from conftest import rel_err
from test_fused_bn_gpu import FUSED_GEOMS, _inputs as fused_inputs, _pin as fused_pin
from test_split_gpu import BNSTAT_GEOMS

pytestmark = pytest.mark.gpu

PAD = (0, 1, 1)
NATIVE, NATIVE_W = (0, 2, 2, 2), (0, 1, 4, 0)         # native f32 tiles: forward / data gradient, weight gradient
A_XS, A_K, A_MT = BNSTAT_GEOMS["one row block"]       # chain A: its convolution leaves the BatchNorm's statistics (patch kernel)
A_WS = (A_K, A_XS[1], 1, 3, 3)
B_XS, B_WS = (2, 8, 2, 14, 14), (16, 8, 1, 3, 3)      # chain B: untagged
BT_WS = (16, 16, 3, 1, 1)                             # ... and the temporal convolution behind its BatchNorm
J_XS, J_WS = (2, 16, 2, 14, 14), (16, 16, 1, 3, 3)    # the residual-join / side-stream graphs
FUSED = next(iter(FUSED_GEOMS))


class Boom(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, dy):
        raise RuntimeError("boom")


class _Arith:
    """f16-pair arithmetic with every tile of this module pinned; the process-wide switches are put back on exit."""

    def __enter__(self):
        from cstp_amd import ops
        ops.set_split_terms(2)
        ops.set_conv_tile(A_XS, A_WS, 1, PAD, 0, (2, A_MT, 0, 0))
        ops.set_conv_tile(B_XS, B_WS, 1, PAD, 0, NATIVE)
        ops.set_conv_tile((B_XS[0], B_WS[0]) + B_XS[2:], BT_WS, 1, (1, 0, 0), 0, NATIVE)
        fused_pin(FUSED)
        for mode, tile in ((0, NATIVE), (1, NATIVE), (2, NATIVE_W)):
            ops.set_conv_tile(J_XS, J_WS, 1, PAD, mode, tile)
        return ops

    def __exit__(self, *exc):
        from cstp_amd import ops
        ops.set_deterministic(False)
        ops.set_split_terms(0)


def _bn(k, g):
    return (torch.rand(k, generator=g) + 0.5).cuda(), torch.randn(k, generator=g).cuda()


def _bn_act(ops, y, bn, groups, residual=None):
    """batch_norm_act + ReLU on fresh running statistics -> (z, running_mean, running_var)."""
    rm, rv = torch.zeros_like(bn[0]), torch.ones_like(bn[0])
    return ops.batch_norm_act(y, bn[0], bn[1], rm, rv, residual, True, 1e-5, 0.1, groups), rm, rv


@pytest.fixture(scope="module")
def chains():
    """The inputs of chains A and B and what each chain computes ALONE (computed once, never written to)."""
    g = torch.Generator().manual_seed(5)
    c = dict(xa=(torch.randn(A_XS, generator=g) + 0.3).cuda(), wa=(torch.randn(A_WS, generator=g) * 0.1).cuda(), bna=_bn(A_K, g),
             xb=(torch.randn(B_XS, generator=g) - 0.2).cuda(), wb=(torch.randn(B_WS, generator=g) * 0.1).cuda(),
             bnb=_bn(B_WS[0], g), wtb=(torch.randn(BT_WS, generator=g) * 0.1).cuda())
    with _Arith() as ops:
        c["alone_a"] = _bn_act(ops, ops.conv3d(c["xa"], c["wa"], None, 1, PAD, bn_groups=2), c["bna"], 2)
        c["alone_b"] = _bn_act(ops, ops.conv3d(c["xb"], c["wb"], None, 1, PAD), c["bnb"], 1)
        torch.cuda.synchronize()
    return c


def _all_equal(got, ref):
    return all(torch.equal(a, b) for a, b in zip(got, ref))


def test_interleaved_chains_keep_their_pairing(chains):
    c = chains
    with _Arith() as ops:
        ya = ops.conv3d(c["xa"], c["wa"], None, 1, PAD, bn_groups=2)
        yb = ops.conv3d(c["xb"], c["wb"], None, 1, PAD)
        b = _bn_act(ops, yb, c["bnb"], 1)
        a = _bn_act(ops, ya, c["bna"], 2)
        assert ops._bnstats_of(ya, 2) is not None and getattr(yb, "_cstp_bnstats", None) is None
        assert _all_equal(a, c["alone_a"]) and _all_equal(b, c["alone_b"])
        cells = [z._cstp_absmax[0] for z in (a[0], b[0])]
        assert cells[0] is not cells[1]
        for z, cell in zip((a[0], b[0]), cells):
            assert int(cell.item()) == int(z.abs().max().view(torch.int32).item())      # the fp32 bits of max |z|


def test_interleaved_fused_chains_keep_their_pairing(chains):
    """As above with bn_relu_conv3d as the consumer: the statistics of A's producer reach A's consumer although another
    bn_relu_conv3d, on an untagged tensor, runs between the two."""
    c = chains
    mid = FUSED_GEOMS[FUSED][1]
    x, w_s, w_t, gamma, beta = [t.cuda() for t in fused_inputs(FUSED)]
    with _Arith() as ops:
        def run_b():
            rm, rv = torch.zeros(B_WS[0], device="cuda"), torch.ones(B_WS[0], device="cuda")
            y = ops.conv3d(c["xb"], c["wb"], None, 1, PAD)
            assert ops._bnstats_of(y, 1) is None
            return ops.bn_relu_conv3d(y, c["bnb"][0], c["bnb"][1], rm, rv, c["wtb"], 1, (1, 0, 0), 1, True, 1e-5, 0.1), rm, rv

        def run_a(between=None):
            rm, rv = torch.zeros(mid, device="cuda"), torch.ones(mid, device="cuda")
            y = ops.conv3d(x, w_s, None, 1, PAD, bn_groups=2, bn_pivot=rm)
            assert ops._bnstats_of(y, 2) is not None
            other = between() if between is not None else None
            return (ops.bn_relu_conv3d(y, gamma, beta, rm, rv, w_t, 1, (1, 0, 0), 2, True, 1e-5, 0.1), rm, rv), other

        a, b = run_a(run_b)
        assert _all_equal(a, run_a()[0]) and _all_equal(b, run_b())


def test_a_call_that_raises_leaves_nothing_behind(chains):
    from cstp_amd import _lib
    c = chains
    with _Arith() as ops:
        ya = ops.conv3d(c["xa"], c["wa"], None, 1, PAD, bn_groups=2)
        yb = ops.conv3d(c["xb"], c["wb"], None, 1, PAD)
        with pytest.raises(_lib.CstpError, match="residual shape"):
            _bn_act(ops, ya, c["bna"], 2, residual=ya[:1])
        assert _all_equal(_bn_act(ops, yb, c["bnb"], 1), c["alone_b"])
        assert _all_equal(_bn_act(ops, ya, c["bna"], 2), c["alone_a"])         # still from ya's own statistics
        for cls in (ops._Conv3d, ops._BNAct, ops._BNReluConv3d, ops._GateConcat, ops._BNReluConcat):
            for name in ("_last_stats", "_pre_stats", "_last_cell"):
                assert not hasattr(cls, name), (cls.__name__, name)


def test_gradjoin_check_survives_a_failed_backward():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(J_XS, generator=g).cuda().requires_grad_(True)
    z, w, bn = torch.randn(J_XS, generator=g).cuda(), (torch.randn(J_WS, generator=g) * 0.1).cuda(), _bn(J_XS[1], g)
    with _Arith() as ops:
        def bn_branch(join):
            return ops.batch_norm_act(z, bn[0], bn[1], residual=x, relu=True, grad_join=join)

        def conv_branch(join):
            return ops.conv3d(x, w, padding=PAD, grad_join=join)

        # (a) a backward pass that raises with a join in use.  The engine runs the node created last first: in the first graph
        # that is Boom, and no contributor ran; in the second the BatchNorm contributes, then Boom raises on a half-open join
        join = ops.GradJoin(2)
        with pytest.raises(RuntimeError, match="boom"):
            (bn_branch(join) + Boom.apply(conv_branch(join))).sum().backward()
        join = ops.GradJoin(2)
        boomed = Boom.apply(conv_branch(join))
        with pytest.raises(RuntimeError, match="boom"):
            (boomed + bn_branch(join)).sum().backward()
        # (b) the end-of-backward check of a LATER pass still fires
        with pytest.raises(RuntimeError, match="contributors missing"):
            (bn_branch(ops.GradJoin(2)) + conv_branch(None)).sum().backward()
        # (c) ... and a complete join still sums
        x.grad = None
        join = ops.GradJoin(2)
        (bn_branch(join) + conv_branch(join)).sum().backward()
        joined, x.grad = x.grad, None
        (bn_branch(None) + conv_branch(None)).sum().backward()
        assert rel_err(joined, x.grad) < 1e-5        # (run-to-run summation order, as test_split_gpu.py)


def test_side_stream_join_survives_a_failed_backward():
    from cstp_amd import ops
    if not ops.OVERLAP_WGRAD:
        pytest.skip("CSTP_OVERLAP_WGRAD=0: weight gradients stay on the main stream")
    g = torch.Generator().manual_seed(8)
    x = torch.randn(J_XS, generator=g).cuda()

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter((torch.randn(J_WS, generator=g) * 0.1).cuda())

    m = M()
    flat = torch.zeros(m.w.numel(), device="cuda")
    m.w.grad = flat.view_as(m.w)
    with _Arith() as ops:
        ops.mark_direct_grad(m, {"grad": flat}, True)
        # the convolution's backward launches the weight gradient on the side stream, then Boom raises: no join callback runs
        with pytest.raises(RuntimeError, match="boom"):
            ops.conv3d(Boom.apply(x.clone().requires_grad_(True)), m.w, padding=PAD).sum().backward()
        torch.cuda.synchronize()
        flat.zero_()
        ops.conv3d(x, m.w, padding=PAD).sum().backward()
        assert ops._pending_side_joins() == []
        torch.cuda.current_stream().synchronize()          # the main stream waited for the side stream: that one is idle too
        assert ops._side_stream(x.device).query()
        w2 = m.w.detach().clone().requires_grad_(True)
        ref, = torch.autograd.grad(ops.conv3d(x, w2, padding=PAD).sum(), w2)
        assert rel_err(m.w.grad, ref) < 1e-5

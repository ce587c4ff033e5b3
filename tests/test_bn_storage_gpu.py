"""The BatchNorm3d kernels exist twice, for fp32 storage (csrc/bn.hip) and for bf16 storage (csrc/b16.hip), and every numerical
rule has to hold in both.  The same cases run through both storages against ONE fp64 CPU reference (tests/ops_edge_cases.py: bn_train_case / bn_eval_case); the inputs
are rounded to bf16 first, so both storages see the same numbers.  One shape per kernel route, the smallest that reaches it:

    single-launch, 256 threads                                          (2, 3, 1, 3, 5)      15 values per row
    single-launch forward on 1024 threads, streamed backward            (2, 2, 2, 36, 36)    4096 < 5184 values per (channel, group)
    streamed, 16-byte accesses, >= 2 chunks and a ragged last one       (2, 2, 4, 48, 48)    s = 9216: 3 fp32 chunks, 2 bf16 chunks
    streamed, one element per access (s odd)                            (2, 2, 3, 55, 55)    s = 9075

each with groups 1 and 2 (n = 4) and with {residual + ReLU, ReLU alone (the mask recomputed from x), neither}, plus one run whose
parameter gradients are accumulated into existing ones.

Bounds are the project's own.  fp32: ops_edge_cases' bars and floors (1e-4 train, 1e-5 eval).  bf16: the expressions of
tests/test_b16_gpu.py::test_batch_norm_bf16_forward_backward -- every stored element within one bf16 ulp of the fp64 result
(+ 1e-5 / 2e-5 of the tensor's largest magnitude for y / dx), fp32 parameter gradients to 2e-5.  Running statistics: 1e-6 in both.
test_reference_rounded_to_bf16_is_inside_the_bf16_bounds (no GPU) holds the bf16 expressions against the reference itself.
"""
import functools

import pytest
import torch

import ops_edge_cases as ec
from test_b16_gpu import bf, check_rounded, ulp_bf16

DEV = "cuda"

SHAPES = [(2, 3, 1, 3, 5), (2, 2, 2, 36, 36), (2, 2, 4, 48, 48), (2, 2, 3, 55, 55)]
VARIANTS = [(True, True), (False, True), (False, False)]        # (residual, relu)
STORAGES = [torch.float32, torch.bfloat16]


@functools.lru_cache(maxsize=None)
def case(shape, groups, use_res, relu):
    """Inputs (values representable in bf16, held in fp32) and the fp64 references of one case; shared by both storages."""
    shape = (2 * groups,) + shape[1:]
    g = torch.Generator().manual_seed(sum(shape) + 1000 * groups)
    c = shape[1]
    rb = lambda t: bf(t).float()
    x = rb(torch.randn(shape, generator=g) * 1.5 + 0.3)
    res = rb(torch.randn(shape, generator=g)) if use_res else None
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.2
    dy = rb(torch.randn(shape, generator=g))
    rm, rv = torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5
    train = ec.bn_train_case(x, gamma, beta, res, relu, groups, rm, rv, dy)
    rm1, rv1 = train["running_mean"].ref.float(), train["running_var"].ref.float()       # eval mode runs on the updated statistics
    evl = ec.bn_eval_case(x, gamma, beta, rm1, rv1, res, relu)
    return dict(x=x, res=res, gamma=gamma, beta=beta, dy=dy, rm=rm, rv=rv, rm1=rm1, rv1=rv1, train=train, eval=evl)


def bf16_bounds(what, got, outs):
    """The assertions of test_batch_norm_bf16_forward_backward on one case's outputs (got: name -> tensor, any device)."""
    d = lambda name: got[name].detach().cpu().double()
    y, want = d("y"), outs["y"].ref
    print("BN16 %s y max|err| %.3g" % (what, float((y - want).abs().max())))
    assert float((y - want).abs().max()) <= float((ulp_bf16(want) + 2e-6 * want.abs().max()).max())
    assert bool(((y - want).abs() <= ulp_bf16(want) + 1e-5 * float(want.abs().max())).all())
    if "dx" not in got:
        return
    dx = outs["dx"].ref
    assert bool(((d("dx") - dx).abs() <= ulp_bf16(dx) + 2e-5 * float(dx.abs().max())).all())
    for name in ("dgamma", "dbeta"):
        ref = outs[name].ref
        err = float((d(name) - ref).abs().max() / ref.abs().max())
        print("BN16 %s %s %.3g" % (what, name, err))
        assert err < 2e-5
    if "dres" in outs:
        check_rounded(got["dres"], outs["dres"].ref, "residual gradient")


def running_bounds(got, outs):
    erm, erv = outs["running_mean"].ref, outs["running_var"].ref
    assert float((got["running_mean"].cpu().double() - erm).abs().max()) < 1e-6
    assert float((got["running_var"].cpu().double() - erv).abs().max() / erv.abs().max()) < 1e-6


def run(cs, dtype, relu, groups, direct=None):
    """ops.batch_norm_act forward and backward and ops.batch_norm_eval in one storage -> (train outputs, eval output)."""
    from cstp_amd import ops
    put = lambda t: None if t is None else t.to(DEV, dtype)
    x, res = put(cs["x"]).requires_grad_(True), put(cs["res"])
    if res is not None:
        res.requires_grad_(True)
    gamma, beta = cs["gamma"].to(DEV).requires_grad_(True), cs["beta"].to(DEV).requires_grad_(True)
    if direct is not None:       # the kernel adds into the parameters' existing gradients
        for p, prior in zip((gamma, beta), direct):
            p.grad = prior.to(DEV).clone()
            p._cstp_direct_grad = True
    rm, rv = cs["rm"].to(DEV), cs["rv"].to(DEV)
    y = ops.batch_norm_act(x, gamma, beta, rm, rv, res, relu, groups=groups)
    assert y.dtype == dtype
    y.backward(put(cs["dy"]))
    assert x.grad.dtype == dtype
    got = {"y": y.detach(), "dx": x.grad, "dgamma": gamma.grad, "dbeta": beta.grad, "running_mean": rm, "running_var": rv}
    if res is not None:
        got["dres"] = res.grad
    with torch.no_grad():
        ye = ops.batch_norm_eval(x.detach(), gamma.detach(), beta.detach(), cs["rm1"].to(DEV), cs["rv1"].to(DEV),
                                 None if res is None else res.detach(), relu)
    return got, {"y": ye}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", STORAGES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("use_res,relu", VARIANTS)
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_bn_both_storages(shape, groups, use_res, relu, dtype):
    cs = case(shape, groups, use_res, relu)
    what = "%s g%d res%d relu%d %s" % (shape, groups, use_res, relu, "bf16" if dtype == torch.bfloat16 else "fp32")
    got, got_eval = run(cs, dtype, relu, groups)
    if dtype == torch.float32:
        assert ec.compare("BN " + what, cs["train"], got) == []
        assert ec.compare("BN eval " + what, cs["eval"], got_eval) == []
    else:
        bf16_bounds(what, got, cs["train"])
        bf16_bounds("eval " + what, got_eval, cs["eval"])
    running_bounds(got, cs["train"])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", STORAGES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=lambda v: "x".join(map(str, v)))
def test_bn_parameter_gradients_accumulate(shape, dtype):
    """accumulate = 1 (the direct-gradient mode of cstp_amd.train): dgamma / dbeta are ADDED to what the buffers hold, by the
    single-launch kernel and by the bookkeeping block of the streamed apply pass.  The sum costs one more fp32 rounding."""
    cs = case(shape, 2, True, True)
    g = torch.Generator().manual_seed(7)
    prior = (torch.randn(shape[1], generator=g), torch.randn(shape[1], generator=g))
    got, _ = run(cs, dtype, True, 2, direct=prior)
    bar = 1e-4 if dtype == torch.float32 else 2e-5
    for name, p in zip(("dgamma", "dbeta"), prior):
        ref = cs["train"][name].ref
        err = float((got[name].cpu().double() - (p.double() + ref)).abs().max() / ref.abs().max())
        print("BN accumulate %s %s %s %.3g" % (shape, dtype, name, err))
        assert err < bar


@pytest.mark.parametrize("use_res,relu", VARIANTS)
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_reference_rounded_to_bf16_is_inside_the_bf16_bounds(shape, groups, use_res, relu):
    """No GPU: the fp64 reference itself, rounded once to bf16 where the kernels store bf16, passes the bf16 assertions -- the
    bounds ask nothing that correct rounding cannot give on these inputs."""
    cs = case(shape, groups, use_res, relu)
    tr = cs["train"]
    got = {k: (bf(o.ref) if k in ("y", "dx", "dres") else o.ref.float()) for k, o in tr.items()}
    bf16_bounds("reference", got, tr)
    bf16_bounds("reference eval", {"y": bf(cs["eval"]["y"].ref)}, cs["eval"])
    running_bounds(got, tr)

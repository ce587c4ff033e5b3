"""Dropout / stochastic depth on a real MI355X: cstp_dropout bit for bit against the numpy restatement (tests/reg_spec.py), the
stochastic-depth join against fp64, both inside the R3D-10 and depth-1 R(2+1)D fine-tune step against the fp64 restatement of the
whole forward, CSTP_REG_FUSED=0 against the kernels, and main_ft_mp.py / test.py with the new flags.

Bars.  Dropout: bit equality (an integer mask and one fp32 product).  The join: 1e-6 of the largest magnitude against fp64, the
bar of the suite's other elementwise ops (one fp32 fma and a maximum: 6e-8).  bf16 storage: one bf16 ulp of the fp32 expression
on the same inputs (round to nearest even of a correctly rounded fma against the rounding of product-then-sum).  The models:
the step-1 bars tests/test_ft_gpu.py and tests/test_r3d_gpu.py hold these backbones to -- logits and loss 1e-4, per-tensor
gradient norms 2e-2 -- since the added operations are elementwise."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import reg_spec
from conftest import rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
KEY = 0x15b7fa397883287b


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


# ---- dropout ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _flat(n):
    g = torch.Generator().manual_seed(n)
    return torch.rand(n, generator=g, dtype=torch.float64).float() * 4 - 2, torch.rand(n, generator=g, dtype=torch.float64).float() - 0.5


def _dropout_case(x, dy, p, key, offset, view):
    from cstp_amd import ops
    if view:                                       # one float into a buffer: contiguous, 4 bytes off every 16-byte boundary
        buf = torch.zeros(x.numel() + 1, device=DEV)
        xd = buf[1:]
        xd.copy_(x)
        assert xd.data_ptr() % 16 == 4
    else:
        xd = x.to(DEV)
    xd.requires_grad_(True)
    y = ops.dropout(xd, p, key, offset)
    y.backward(dy.to(DEV))
    return y.detach().cpu(), xd.grad.cpu()


@pytest.mark.parametrize("view", [False, True], ids=["aligned", "flat[1:]"])
@pytest.mark.parametrize("p", [0.3, 0.5, 0.9])
@pytest.mark.parametrize("n", [407, 2048])
def test_dropout_equals_the_restatement_bit_for_bit(n, p, view):
    x, dy = _flat(n)
    for offset in (0, 2 ** 32 + 7):
        y, dx = _dropout_case(x, dy, p, KEY, offset, view)
        assert np.array_equal(y.numpy().view(np.uint32), reg_spec.dropout_fp32(x.numpy(), p, KEY, offset).view(np.uint32))
        assert np.array_equal(dx.numpy().view(np.uint32), reg_spec.dropout_fp32(dy.numpy(), p, KEY, offset).view(np.uint32))
        y2, dx2 = _dropout_case(x, dy, p, KEY, offset, view)
        assert torch.equal(y, y2) and torch.equal(dx, dx2)
    kept = float((y != 0).float().mean())
    assert abs(kept - (1 - p)) < 0.08, kept


def test_dropout_p0_shapes_and_launches():
    from cstp_amd import _lib, ops
    x, _ = _flat(2048)
    xd = x.to(DEV).view(4, 512).requires_grad_(True)
    assert ops.dropout(xd, 0.0, KEY) is xd                                  # p == 0 returns its input
    y = ops.dropout(xd, 0.5, KEY)                                           # a [B, F] feature: the mask runs over the flat tensor
    assert y.shape == (4, 512)
    assert np.array_equal(y.detach().cpu().numpy().reshape(-1), reg_spec.dropout_fp32(x.numpy(), 0.5, KEY, 0))
    assert not torch.equal(y, ops.dropout(xd, 0.5, KEY + 1)) and not torch.equal(y, ops.dropout(xd, 0.5, KEY, 1))
    names = _kernel_names(lambda: ops.dropout(xd, 0.5, KEY).backward(torch.ones_like(xd)))
    assert sum("dropout_kernel" in n for n in names) == 2                   # one launch forward, the same call backward
    with pytest.raises(_lib.CstpError):
        ops.dropout(xd, 1.0, KEY)
    with pytest.raises(_lib.CstpError):
        ops.dropout(xd.double(), 0.5, KEY)


# ---- the stochastic-depth join -----------------------------------------------------------------------------------------------------
DP_CASES = {"odd": ((3, 5, 3, 5, 7), [1.25, 0.0, 1.25]), "vec": ((2, 8, 2, 4, 4), [0.0, 10.0 / 7.0])}


@functools.lru_cache(maxsize=None)
def _dp_case(name):
    """(z, res, dy, scale) on the host and the fp64 reference (y, dz, dres): computed once, read only."""
    shape, scale = DP_CASES[name]
    g = torch.Generator().manual_seed(len(name) + shape[1])
    z, res, dy = [(torch.rand(shape, generator=g, dtype=torch.float64) * 4 - 2).float() for _ in range(3)]
    scale = torch.tensor(scale, dtype=torch.float32)
    z64, r64 = z.double().requires_grad_(True), res.double().requires_grad_(True)
    y64 = reg_spec.drop_path_add_relu(z64, r64, scale.double())
    y64.backward(dy.double())
    return (z, res, dy, scale), (y64.detach(), z64.grad, r64.grad)


@pytest.mark.parametrize("name", sorted(DP_CASES))
def test_drop_path_fp32_matches_fp64(name):
    from cstp_amd import ops
    (z, res, dy, scale), (y64, dz64, dres64) = _dp_case(name)
    assert (z.shape[1] * z.shape[2] * z.shape[3] * z.shape[4]) % 4 == (1 if name == "odd" else 0)
    zd, rd, sd = z.to(DEV).requires_grad_(True), res.to(DEV).requires_grad_(True), scale.to(DEV)
    y = ops.drop_path_add_relu(zd, rd, sd)
    y.backward(dy.to(DEV))
    errs = rel_err(y, y64), rel_err(zd.grad, dz64), rel_err(rd.grad, dres64)
    print("drop-path %s: y %.3e  dz %.3e  dres %.3e" % ((name,) + errs))
    assert max(errs) <= 1e-6
    dropped = int((scale == 0).nonzero()[0])
    assert torch.equal(y[dropped].detach(), torch.relu(rd[dropped].detach()))          # a dropped sample: relu of the residual, bit for bit
    assert not zd.grad[dropped].any()
    cell = y._cstp_absmax[0]                                                           # the absmax by-product, exactly max |y|
    assert cell.dtype == torch.int32 and float(cell.view(torch.float32)) == float(y.detach().abs().max())
    assert ops._absmax_of(y) is cell
    # either gradient alone (the other output pointer is NULL)
    for need_z, need_r in ((True, False), (False, True)):
        z2, r2 = z.to(DEV).requires_grad_(need_z), res.to(DEV).requires_grad_(need_r)
        ops.drop_path_add_relu(z2, r2, sd).backward(dy.to(DEV))
        if need_z:
            assert r2.grad is None and torch.equal(z2.grad, zd.grad)
        else:
            assert z2.grad is None and torch.equal(r2.grad, rd.grad)
    # an unaligned view takes the element path: the same bits
    buf = torch.zeros(z.numel() + 1, device=DEV)
    zv = buf[1:].view(z.shape)
    zv.copy_(z)
    assert torch.equal(ops.drop_path_add_relu(zv, rd.detach(), sd), y.detach())


def test_drop_path_is_one_launch_each_way():
    from cstp_amd import ops
    (z, res, dy, scale), _ = _dp_case("vec")
    zd, rd, sd, dyd = z.to(DEV).requires_grad_(True), res.to(DEV).requires_grad_(True), scale.to(DEV), dy.to(DEV)
    ops.drop_path_add_relu(zd, rd, sd).backward(dyd)                                   # warm-up: library load
    box = {}
    zd.grad = rd.grad = None                                                           # (no accumulation kernels in the traces)
    fwd = _kernel_names(lambda: box.update(y=ops.drop_path_add_relu(zd, rd, sd)))
    bwd = _kernel_names(lambda: box["y"].backward(dyd))
    mine = lambda names: [n for n in names if "droppath" in n]
    assert len(mine(fwd)) == 1 and "droppath_fwd_kernel" in mine(fwd)[0], fwd
    assert len(mine(bwd)) == 1 and "droppath_bwd_kernel" in mine(bwd)[0], bwd
    assert len(fwd) == 1 and len(bwd) == 1, (fwd, bwd)                                 # nothing else: no fill, no copy


@pytest.mark.parametrize("shape", [(3, 5, 3, 5, 7), (2, 8, 2, 4, 4)], ids=["odd", "vec"])
def test_drop_path_bf16_storage(shape):
    from cstp_amd import ops
    g = torch.Generator().manual_seed(shape[1])
    z, res, dy = [(torch.rand(shape, generator=g, dtype=torch.float64) * 4 - 2).to(torch.bfloat16) for _ in range(3)]
    scale = torch.tensor([1.25, 0.0, 1.25][:shape[0]], dtype=torch.float32)
    s = scale.view(-1, 1, 1, 1, 1)

    def run():
        zd, rd = z.to(DEV).requires_grad_(True), res.to(DEV).requires_grad_(True)
        y = ops.drop_path_add_relu(zd, rd, scale.to(DEV))
        y.backward(dy.to(DEV))
        return y.detach().cpu(), zd.grad.cpu(), rd.grad.cpu()

    y, dz, dres = run()
    assert y.dtype == dz.dtype == dres.dtype == torch.bfloat16
    want = torch.relu(s * z.float() + res.float())                                      # the fp32 composition on the same bf16 inputs
    mask = (want > 0).float()
    for got, ref in ((y, want), (dz, s * dy.float() * mask), (dres, dy.float() * mask)):
        ulp = torch.maximum(ref.abs(), torch.tensor(2.0 ** -126)).log2().floor().exp2() * 2.0 ** -7     # one bf16 ulp at |ref|
        # (where the composition's own rounding moved a value across 0 the masks may differ by that one element's ulp as well)
        assert bool(((got.float() - ref).abs() <= ulp).all())
    y2, dz2, dres2 = run()
    assert torch.equal(y, y2) and torch.equal(dz, dz2) and torch.equal(dres, dres2)


# ---- inside the fine-tune step -----------------------------------------------------------------------------------------------------
B, T, HW, K = 4, 8, 32, 7


@functools.lru_cache(maxsize=None)
def _clips():
    from oracle import r21d_byol_oracle as orc
    x, _, _ = orc.closed_form_clips(B, T, HW, torch.float32)
    return x, (torch.arange(B, dtype=torch.int64) * 7 + 3) % K


@functools.lru_cache(maxsize=None)
def _state(model):
    from oracle import r21d_ft_oracle as fto
    from oracle import r3d_byol_oracle as r3d
    if model == "r21d":
        return fto.closed_form_state((1, 1, 1, 1), K, torch.float32)
    return r3d.closed_form_state(r3d.ft_spec(r3d.for_depth(10), K), torch.float32)


def _regularizer():
    from cstp_amd.regularize import Regularizer
    return Regularizer(0.5, 0.3, seed=1)


@functools.lru_cache(maxsize=None)
def _reference(model):
    """fp64 restatement of the regularised step-0 forward and backward: (logits, loss, {parameter: gradient norm})."""
    from oracle import r3d_byol_oracle as r3d
    x, lab = _clips()
    plan = _regularizer().plan(B, 4, 0, 0, 0)
    assert plan.key == KEY and plan.keep.astype(int).tolist() == [[1, 1, 1, 1], [1, 1, 0, 1], [1, 1, 1, 1], [0, 0, 1, 1]]
    sd = {k: (v.clone() if v.dtype == torch.int64 else v.double()) for k, v in _state(model).items()}
    keys = [k for k, v in sd.items() if v.dtype == torch.float64 and "running_" not in k]
    for k in keys:
        sd[k].requires_grad_(True)
    scales = [None if s is None else s.double() for s in reg_spec.plan_scales(plan)]
    if model == "r21d":
        out = reg_spec.r21d_ft_forward(sd, x.double(), (1, 1, 1, 1), scales, (0.5, plan.key))
    else:
        out = reg_spec.r3d_ft_forward(sd, x.double(), r3d.for_depth(10), scales, (0.5, plan.key))
    loss = F.cross_entropy(out, lab)
    grads = torch.autograd.grad(loss, [sd[k] for k in keys])
    return out.detach(), float(loss), {k: float(g.norm()) for k, g in zip(keys, grads)}


def _build(model, act_dtype="fp32"):
    import argparse
    from cstp_amd.optim import FlatSGD
    from cstp_amd.r21d_byol import R21DBYOL
    from cstp_amd.r3d_byol import R3DBYOL
    if model == "r21d":
        kw = {} if act_dtype == "fp32" else {"act_dtype": act_dtype}
        m = R21DBYOL(pretrain=False, num_classes=K, cls_bn=True, layer_sizes=(1, 1, 1, 1), **kw)
    else:
        m = R3DBYOL(pretrain=False, cls_bn=True, opts=argparse.Namespace(model_depth=10, sample_size=HW, sample_duration=T, sc_type="B",
                                                                        n_classes=K, act_dtype=act_dtype))
    m.load_state_dict({k: v.clone() for k, v in _state(model).items()}, strict=True)
    m.cuda().train()
    arenas = m.flatten_parameters()
    return m, FlatSGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4, arenas=arenas)


def _step(model, regularizer="default", act_dtype="fp32", **kw):
    from cstp_amd.train import FineTuneStep
    m, opt = _build(model, act_dtype)
    if regularizer == "default":
        regularizer = _regularizer()
    if regularizer != "absent":
        kw["regularizer"] = regularizer
    return m, FineTuneStep(m, opt, "ft_all", **kw)


def _run_step(model, act_dtype="fp32", **kw):
    x, lab = _clips()
    m, step = _step(model, act_dtype=act_dtype, **kw)
    loss, logits = step(x.to(DEV), lab.to(DEV))
    return m, step, float(loss), logits.cpu(), {n: float(p.grad.norm()) for n, p in m.named_parameters()}


@pytest.mark.parametrize("model", ["r3d", "r21d"])
def test_step_matches_the_fp64_restatement(model):
    want_logits, want_loss, want_norms = _reference(model)
    m, step, loss, logits, norms = _run_step(model)
    assert step.last_reg_plan.key == KEY
    e_logits, e_loss = rel_err(logits, want_logits), abs(loss - want_loss) / abs(want_loss)
    assert sorted(norms) == sorted(want_norms)
    scale = max(want_norms.values())
    e_norm = max(abs(norms[k] - want_norms[k]) / max(want_norms[k], 1e-3 * scale) for k in norms)
    print("%s with dropout 0.5 / drop_path 0.3: logits %.3e  loss %.3e  gradient norms %.3e" % (model, e_logits, e_loss, e_norm))
    assert e_logits < 1e-4 and e_loss < 1e-4 and e_norm < 2e-2
    assert m._dropout is None and all(b._drop_scale is None for b in m.residual_blocks())       # the plan left with the forward
    # it is not the plain step: the unregularised restatement is far from these logits
    plain = reg_spec.r21d_ft_forward if model == "r21d" else reg_spec.r3d_ft_forward
    sd = {k: v.clone() for k, v in _state(model).items()}
    with torch.no_grad():
        assert rel_err(logits, plain(sd, _clips()[0], (1, 1, 1, 1))) > 1e-2


@pytest.mark.parametrize("model,act_dtype", [("r3d", "fp32"), ("r21d", "fp32"), ("r3d", "bf16"), ("r21d", "bf16")])
def test_composed_path_agrees_with_the_kernels(model, act_dtype, monkeypatch):
    """CSTP_REG_FUSED=0 (the switch is read at import; the test sets the module's flag): the same mask and the same expression from
    ATen calls, no new kernel.  fp32: each path is held to 1e-4 (logits, loss) / 2e-2 (gradient norms) of fp64 above, so the two
    are within twice that of each other.  bf16 storage has no fp64 restatement of the kernels' rounding points, so this is its
    model-level check: the paths differ by the contraction of one fp32 multiply-add in front of a bf16 rounding, i.e. by isolated
    one-ulp flips of stored activations -- noise of the kind bf16 storage itself adds, which tests/test_b16_gpu.py bounds by
    1e-2 (loss), 2e-2 (logits) and 5e-2 (gradient norm) at these depths."""
    from cstp_amd import ops
    _, _, loss_f, logits_f, norms_f = _run_step(model, act_dtype)
    monkeypatch.setattr(ops, "REG_FUSED", False)
    x, lab = _clips()
    m, step = _step(model, act_dtype=act_dtype)
    box = {}
    names = _kernel_names(lambda: box.update(out=step(x.to(DEV), lab.to(DEV))))
    assert not any("droppath" in n or "dropout_kernel" in n for n in names)
    loss_c, logits_c = float(box["out"][0]), box["out"][1].cpu()
    norms_c = {n: float(p.grad.norm()) for n, p in m.named_parameters()}
    ltol, tol, gtol = (2e-4, 2e-4, 4e-2) if act_dtype == "fp32" else (1e-2, 2e-2, 5e-2)
    e_logits, e_loss = rel_err(logits_c, logits_f), abs(loss_c - loss_f) / abs(loss_f)
    e_norm = max(abs(norms_c[k] - norms_f[k]) / max(norms_f[k], 1e-3 * max(norms_f.values())) for k in norms_f)
    print("%s %s composed vs fused: logits %.3e  loss %.3e  gradient norms %.3e" % (model, act_dtype, e_logits, e_loss, e_norm))
    assert e_logits < tol and e_loss < ltol and e_norm < gtol


def test_regularised_step_launches_the_new_kernels_and_the_plain_step_none():
    x, lab = _clips()
    xd, ld = x.to(DEV), lab.to(DEV)
    count = lambda names: [sum(k in n for n in names) for k in ("dropout_kernel", "droppath_fwd_kernel", "droppath_bwd_kernel")]
    _, step = _step("r21d", None)
    step(xd, ld)
    assert count(_kernel_names(lambda: step(xd, ld))) == [0, 0, 0]
    _, step = _step("r21d")
    step(xd, ld)
    assert count(_kernel_names(lambda: step(xd, ld))) == [2, 3, 3]           # block 0 has p = 0: it keeps the fused BatchNorm kernel


@pytest.mark.parametrize("model", ["r3d", "r21d"])
def test_eval_forward_ignores_an_installed_plan(model):
    x, _ = _clips()
    m, _ = _build(model)
    m.eval()
    with torch.no_grad():
        plain = m(x.to(DEV), o_type="ft_all")
        scales = [None] + [torch.tensor([0.0, 2.0, 0.0, 2.0], device=DEV)] * 3
        with m.regularized((0.5, KEY), scales):
            assert torch.equal(m(x.to(DEV), o_type="ft_all"), plain)
        assert torch.equal(m(x.to(DEV), o_type="test"), plain)


def test_regularizer_none_is_the_step_without_the_argument(monkeypatch):
    """Bit for bit: loss, logits, every gradient and every updated parameter.  Two runs of ONE step are bit-equal only where no sum
    depends on wave timing, so the comparison runs with deterministic weight gradients and BatchNorm statistics taken by their own
    pass (the default step's float atomics differ in the last bits from run to run, whatever its arguments)."""
    from cstp_amd import ops
    monkeypatch.setattr(ops, "FUSE_BN_STATS", False)
    ops.set_deterministic(True)
    try:
        a = _run_step("r21d", regularizer=None)
        b = _run_step("r21d", regularizer="absent")
        assert a[2] == b[2] and torch.equal(a[3], b[3])
        pa, pb = dict(a[0].named_parameters()), dict(b[0].named_parameters())
        differ = [k for k in pa if not (torch.equal(pa[k], pb[k]) and torch.equal(pa[k].grad, pb[k].grad))]
        assert not differ, differ
        assert all(torch.equal(v, w) for v, w in zip(a[0].state_dict().values(), b[0].state_dict().values()))
        assert a[1].last_reg_plan is None and a[1].regularizer is None and b[1].regularizer is None
    finally:
        ops.set_deterministic(False)


def test_set_epoch_reproduces_the_plans():
    x, lab = _clips()
    xd, ld = x.to(DEV), lab.to(DEV)
    reg = _regularizer()
    _, step = _step("r21d")
    step.set_epoch(3)
    seen = []
    for s in range(3):
        step(xd, ld)
        seen.append(step.last_reg_plan)
        want = reg.plan(B, 4, 3, s, 0)
        assert seen[-1].key == want.key and np.array_equal(seen[-1].scale, want.scale)
    _, resumed = _step("r21d")                                             # a fresh process that resumes at epoch 3
    resumed.set_epoch(3)
    resumed(xd, ld)
    assert resumed.last_reg_plan.key == seen[0].key and np.array_equal(resumed.last_reg_plan.scale, seen[0].scale)
    step.set_epoch(4)
    step(xd, ld)
    assert step.last_reg_plan.key == reg.plan(B, 4, 4, 0, 0).key != seen[0].key


def test_dropout_serves_the_other_heads():
    """S3D-G and the R3D 'scratch' branch put the same op in front of their classifier (the I3D module takes the key likewise)."""
    from cstp_amd import ops
    from cstp_amd.i3d_byol import Dropout
    m, _ = _build("r3d")
    x, _ = _clips()
    with m.regularized((0.5, KEY), None):
        with torch.no_grad():
            feat = m.online_net(x.to(DEV))
            assert torch.equal(m(x.to(DEV), o_type="scratch"), m.classify(ops.dropout(feat, 0.5, KEY, 0)))
    d = Dropout(0).train()
    f = torch.rand(2, 8, 3, 1, 1, device=DEV)
    assert d(f) is f
    d.p, d.key = 0.5, KEY
    assert torch.equal(d(f), ops.dropout(f, 0.5, KEY, 0)) and d.eval()(f) is f


# ---- the drivers -----------------------------------------------------------------------------------------------------------------
def _run(args, timeout):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args[0], r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_finetune_driver_with_the_flags_then_test(tmp_path):
    from cstp_amd.r21d_byol import R21DBYOL
    res = str(tmp_path)
    ckpt = os.path.join(res, "empty.pth")
    torch.save({"epoch": 0, "arch": "r21d_byol-1", "state_dict": {}}, ckpt)
    ft = ["--dataset", "synthetic_video", "--sample_duration", "8", "--sample_size", "112", "--model_name", "r21d_byol",
          "--model_depth", "1", "--n_workers", "0", "--result_path", res, "--n_classes", "4", "--batch_size", "4",
          "--synthetic_len", "16", "--weight_decay", "1e-4", "--pb_rate", "4"]
    out = _run(["main_ft_mp.py"] + ft + ["--transform_mode", "img", "--task", "ft_all", "--pretrained_path", ckpt, "--learning_rate",
                                         "0.01", "--n_epochs", "1", "--max_steps", "3", "--dropout", "0.5", "--drop_path", "0.1"], 600)
    assert "dropout=0.5" in out and "drop_path=0.1" in out
    d = os.path.join(res, "synthetic_video", "ft_all")
    best = [f for f in os.listdir(d) if f.endswith("_max.pth")]
    assert len(best) == 1
    md = torch.load(os.path.join(d, best[0]), map_location="cpu")
    plain = R21DBYOL(pretrain=False, num_classes=4, cls_bn=True, layer_sizes=(1, 1, 1, 1))
    assert list(md["state_dict"].keys()) == ["module." + k for k in plain.state_dict().keys()]                  # unchanged keys
    assert all(bool(torch.isfinite(v.float()).all()) for v in md["state_dict"].values())
    out_test = _run(["test.py"] + ft + ["--transform_mode", "img_test", "--task", "test", "--t_ft_task", "ft_all"], 600)
    assert "Video accuracy" in out_test
    # the refusals reach the command line before any data or model is built
    for flags, needle in ((["--task", "ft_fc", "--drop_path", "0.1"], "--drop_path"), (["--task", "ft_all", "--dropout", "1.0"], "--dropout")):
        r = subprocess.run([sys.executable, "main_ft_mp.py"] + ft + ["--transform_mode", "img", "--pretrained_path", ckpt] + flags,
                           cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and needle in r.stderr, r.stderr[-2000:]

"""R(2+1)D-BYOL with bf16 activation storage (``--act_dtype bf16``) on a real MI355X: the ragged channel counts of the (2+1)D
factorisation in the bf16 convolution (csrc/b16.hip, RAG gather and padded packs), and the model on top of them.

Tolerances, stated before the first GPU run (the style and reasoning of tests/test_b16_gpu.py):
  * op level, every ragged geometry of R(2+1)D-18 at reduced batch and extents: a bf16 OUTPUT (forward, data gradient) within
    one bf16 ulp of the fp64 result on the same bf16 operands everywhere, and fewer than 1 element in 1000 different from its
    correctly rounded value; fp32 weight gradients within 2e-5 of the largest magnitude; the weight gradient bit-identical
    from run to run;
  * model level against the restated spec (tests/r21d_b16_spec.py, fp64 between the rounding points): losses 1e-2, logits 2e-2
    of their largest magnitude, global gradient norm 5e-2 -- printed beside the spec's own fp32-vs-fp64 distance.  Measured on
    the CPU before the GPU run, that distance is 7.8e-3 (depth 1) but 3.2e-2 (depth 18) on the logits at 4 clips of 8x56x56 (the
    BatchNorm1d heads over four samples amplify each flip), so the logits bar is max(2e-2, 3 x the spec's own fp32 distance);
  * model level against the reference's fp64 goldens: the price of bf16 storage measured by tests/test_r21d_b16_spec.py (losses
    <= 2.1e-3, gradient norm <= 2.0e-2, logits 2.5e-2 / 8.3e-2 / 2.8e-1 for d1 / r18 / r34) -- bars: losses 5e-3, gradient
    norm 5e-2, logits twice the measured price;
  * fine-tune wrapper: train-mode logits 5e-2 of the spec (BatchNorm1d over four samples), eval mode 5e-3;
  * the accumulating data gradient, bf16(bf16(gradient) + dx): two roundings, so within ulp(gradient) + ulp(sum) of the exact
    sum, and fewer than 1 in 1000 elements different from bf16(bf16(exact gradient) + dx).
Restated after the first GPU run: (1) the accumulate check above first allowed one ulp of the sum only -- one element of the
64 -> 230 case landed one ulp of the sum plus the first rounding's flip away, which is the spec; (2) the train-mode fine-tune
logits at depth 18 land 8.0e-2 from the spec, as the spec's own fp32 run does (BatchNorm1d over four samples after 17 layers):
that bar is now max(5e-2, 3 x the spec's own fp32 distance), as the pre-training step's logits bar is.
  * full size (cfg2): finite, loss within 5 % of the fp32-storage step from the same state, and the pack plan's seven-step
    trajectory within 1e-3 of the one without it.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import r21d_b16_spec as spec
from cstp_amd import ops
from oracle import r21d_byol_oracle as orc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def bf(t):
    return t.to(torch.bfloat16)


def ulp_bf16(ref):
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 7)


def check_rounded(got_bf16, exact64, what):
    got = got_bf16.detach().cpu().double()
    want = exact64.to(torch.bfloat16).double()
    err = (got - exact64).abs()
    floor = 1e-5 * float(exact64.abs().max())
    bad = err > ulp_bf16(exact64) + floor
    assert not bool(bad.any()), "%s: %d elements further than one bf16 ulp, worst %g" % (what, int(bad.sum()), float(err.max()))
    flips = float((got != want).double().mean())
    assert flips < 1e-3, "%s: %.2e of the elements differ from the correctly rounded value" % (what, flips)


RAGGED = [
    # (n, c, d, h, w), k, kernel, stride, padding, data gradient
    ((2, 3, 4, 32, 32), 83, (1, 7, 7), (1, 2, 2), (0, 3, 3), False),     # stem spatial: 49 taps (offset table), 83 output rows
    ((2, 83, 4, 16, 16), 64, (3, 1, 1), (1, 1, 1), (1, 0, 0), True),     # stem temporal: 83-channel reduction, octet gather
    ((1, 83, 3, 4, 56), 64, (3, 1, 1), (1, 1, 1), (1, 0, 0), True),      # ... on the 56-wide rows of cfg2
    ((2, 64, 4, 16, 16), 230, (1, 3, 3), (1, 2, 2), (0, 1, 1), True),    # conv3 spatial: 230 output rows / data-gradient reduction
    ((2, 230, 4, 8, 8), 128, (3, 1, 1), (2, 1, 1), (1, 0, 0), True),     # conv3 temporal
    ((2, 128, 2, 8, 8), 460, (1, 3, 3), (1, 2, 2), (0, 1, 1), True),     # conv4 spatial
    ((2, 460, 2, 4, 4), 256, (3, 1, 1), (2, 1, 1), (1, 0, 0), True),     # conv4 temporal
    ((2, 256, 2, 4, 4), 921, (1, 3, 3), (1, 2, 2), (0, 1, 1), True),     # conv5 spatial
    ((2, 921, 2, 2, 2), 512, (3, 1, 1), (2, 1, 1), (1, 0, 0), True),     # conv5 temporal: 3 x 921 = 2763 > the offset table
    ((2, 64, 4, 16, 16), 42, (1, 1, 1), (1, 2, 2), (0, 0, 0), True),     # conv3 shortcut (2+1)D pair: 64 -> 42 -> 128
    ((2, 42, 4, 8, 8), 128, (1, 1, 1), (2, 1, 1), (0, 0, 0), True),
    ((2, 128, 2, 8, 8), 85, (1, 1, 1), (1, 2, 2), (0, 0, 0), True),      # conv4 shortcut: 128 -> 85 -> 256
    ((2, 85, 2, 4, 4), 256, (1, 1, 1), (2, 1, 1), (0, 0, 0), True),
    ((1, 7, 3, 5, 7), 17, (3, 3, 3), (1, 1, 1), (1, 1, 1), True),        # synthetic: 7 and 17 channels, odd extents, one sample
    ((1, 17, 3, 5, 7), 7, (3, 3, 3), (1, 1, 1), (1, 1, 1), True),
    ((1, 17, 5, 7, 9), 7, (3, 3, 3), (2, 2, 2), (1, 1, 1), True),
    ((1, 7, 3, 4, 8), 17, (3, 3, 3), (1, 1, 1), (1, 1, 1), True),        # ... octet-eligible rows
    ((1, 17, 3, 4, 8), 7, (1, 3, 3), (1, 1, 1), (0, 1, 1), True),
]


def _case(xs, k, kern, seed):
    g = torch.Generator().manual_seed(seed)
    x = bf(torch.randn(xs, generator=g))
    w = torch.randn((k, xs[1]) + kern, generator=g) / np.sqrt(xs[1] * np.prod(kern))
    return g, x, w


@pytest.mark.parametrize("xs,k,kern,stride,pad,dgrad", RAGGED)
def test_conv3d_bf16_ragged_channels(xs, k, kern, stride, pad, dgrad):
    g, x, w = _case(xs, k, kern, sum(xs) + k)
    x64 = x.double().requires_grad_(True)
    w64 = bf(w).double().requires_grad_(True)
    y64 = F.conv3d(x64, w64, None, stride, pad)
    dy = bf(torch.randn(y64.shape, generator=g))
    dx64, dw64 = torch.autograd.grad(y64, (x64, w64), dy.double())

    xd = x.to(DEV).requires_grad_(dgrad)
    wd = w.to(DEV).requires_grad_(True)
    y = ops.conv3d(xd, wd, None, stride, pad)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == tuple(y64.shape)
    check_rounded(y, y64.detach(), "forward")
    y.backward(dy.to(DEV))
    err = float((wd.grad.cpu().double() - dw64).abs().max() / dw64.abs().max())
    assert err < 2e-5, "weight gradient %g" % err
    if dgrad:
        check_rounded(xd.grad, dx64, "data gradient")


def _raw(fn, xs, k, kern, stride, pad, *tensors, extra=()):
    lib = ops._lib.load()
    desc = ops._desc(xs, (k, xs[1]) + kern, stride, pad)
    nbytes = lib.cstp_b16_conv3d_workspace_bytes(ctypes.byref(desc))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    rc = getattr(lib, fn)(ops._stream(), ctypes.byref(desc), *[t.data_ptr() for t in tensors], ws.data_ptr(), ws.numel(), *extra)
    assert rc == 0, fn


@pytest.mark.parametrize("case", [3, 8, 13])
def test_conv3d_bf16_ragged_backward_data_accumulates(case):
    """cstp_b16_conv3d_backward_data_acc on ragged geometries: dx = bf16(bf16(gradient) + dx) (the residual join's epilogue)."""
    xs, k, kern, stride, pad, _ = RAGGED[case]
    g, x, w = _case(xs, k, kern, 7 + case)
    x64 = x.double().requires_grad_(True)
    y64 = F.conv3d(x64, bf(w).double(), None, stride, pad)
    dy = bf(torch.randn(y64.shape, generator=g))
    (dx64,) = torch.autograd.grad(y64, (x64,), dy.double())
    old = bf(torch.randn(xs, generator=g))
    dx = old.to(DEV).contiguous()
    _raw("cstp_b16_conv3d_backward_data_acc", xs, k, kern, stride, pad, dy.to(DEV), w.to(DEV), dx, extra=(1,))
    torch.cuda.synchronize()
    exact = dx64 + old.double()
    got = dx.cpu().double()
    err = (got - exact).abs()
    bad = err > ulp_bf16(dx64) + ulp_bf16(exact) + 1e-5 * float(exact.abs().max())
    assert not bool(bad.any()), "accumulated data gradient: %d elements beyond the two roundings, worst %g" % (int(bad.sum()), float(err.max()))
    flips = float((got != bf(bf(dx64).double() + old.double()).double()).double().mean())
    assert flips < 1e-3, flips


@pytest.mark.parametrize("case", [4, 8, 14])
def test_conv3d_bf16_ragged_weight_gradient_is_bit_reproducible(case):
    xs, k, kern, stride, pad, _ = RAGGED[case]
    g, x, w = _case(xs, k, kern, 11 + case)
    osz = ops.conv_out_shape(xs, (k, xs[1]) + kern, stride, pad)
    dy = bf(torch.randn(osz, generator=g)).to(DEV)
    xd, wd = x.to(DEV), w.to(DEV)
    outs = []
    for _ in range(2):
        dw = torch.full_like(wd, float("nan"))
        _raw("cstp_b16_conv3d_backward_weight", xs, k, kern, stride, pad, xd, dy, dw, extra=(0,))
        outs.append(dw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0]).all()) and torch.equal(outs[0], outs[1])


# ---- model level -------------------------------------------------------------------------------------------------------------
def _pretrain_step(sd, ls, lr=0.05, wd=5e-4, w=(0.1, 1.0, 1.0, 1.0, 1.0), act="bf16"):
    from cstp_amd.optim import FlatSGD
    from cstp_amd.r21d_byol import R21DBYOL
    from cstp_amd.train import PretrainStep
    model = R21DBYOL(pretrain=True, layer_sizes=ls, act_dtype=act)
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    model.cuda(0)
    arenas = model.flatten_parameters()
    model.train()
    opt = FlatSGD(model.parameters(), lr=lr, momentum=0.9, weight_decay=wd, arenas=arenas)
    return PretrainStep(model, opt, w, clip_grad_norm=True), arenas


def _run(step, x1, x2, labels):
    lab = {k: v.to(DEV) for k, v in labels.items()}
    out = step(x1.to(DEV), x2.to(DEV), lab["spa"], lab["tem"], lab["pb"], lab["rot1"], lab["rot2"])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("depth,b,t,hw", [(1, 4, 8, 56), (18, 4, 8, 56)])
def test_r21d_bf16_step_matches_the_bf16_storage_spec(depth, b, t, hw):
    ls = orc.layer_sizes_for_depth(depth)
    sd = orc.closed_form_state(ls, torch.float32)
    x1, x2, labels = orc.closed_form_clips(b, t, hw, torch.float32)
    info = spec.train_step(spec.to64(sd), x1.double(), x2.double(), labels, ls, "bf16")
    i32 = spec.train_step(sd, x1, x2, labels, ls, "bf16")
    step, arenas = _pretrain_step(sd, ls)
    out = _run(step, x1, x2, labels)
    e = {"loss_byol": spec.rel(float(out.loss_byol), info["loss_byol"]), "loss_total": spec.rel(float(out.loss_total), info["loss_total"]),
         "logits": spec.rel(torch.stack([l.cpu() for l in out.logits[:2]]), torch.stack(info["logits"][:2])),
         "grad_norm": spec.rel(float(out.grad_norm), info["grad_norm"])}
    e32 = {"loss_total": spec.rel(i32["loss_total"], info["loss_total"]),
           "logits": spec.rel(torch.stack(i32["logits"][:2]), torch.stack(info["logits"][:2])),
           "grad_norm": spec.rel(i32["grad_norm"], info["grad_norm"])}
    print("r21d bf16 depth %d: HIP vs the spec (fp64 between roundings) %s; the spec's own fp32 run vs the same %s" % (depth, e, e32))
    assert e["loss_byol"] < 1e-2 and e["loss_total"] < 1e-2 and e["grad_norm"] < 5e-2, (e, e32)
    assert e["logits"] < max(2e-2, 3.0 * e32["logits"]), (e, e32)
    assert bool(torch.isfinite(arenas["param"]).all())


@pytest.mark.parametrize("name,logits_bar", [("d1_small", 5e-2), ("r18_small", 1.7e-1), ("r34_small", 5.6e-1)])
def test_r21d_bf16_step_against_the_reference_fp64_goldens(name, logits_bar):
    g = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    depth, b, t, hw, _ = [int(v) for v in g["meta"]]
    ls = orc.layer_sizes_for_depth(depth)
    sd = orc.closed_form_state(ls, torch.float32)
    x1, x2, labels = orc.closed_form_clips(b, t, hw, torch.float32)
    step, _ = _pretrain_step(sd, ls, float(g["lr"]), float(g["wd"]), tuple(g["loss_weight"]))
    out = _run(step, x1, x2, labels)
    e = {"loss_byol": spec.rel(float(out.loss_byol), g["s1.loss_byol"]), "loss_total": spec.rel(float(out.loss_total), g["s1.loss_total"]),
         "logits": spec.rel(torch.stack([l.cpu() for l in out.logits]), g["s1.logits"]),
         "grad_norm": spec.rel(float(out.grad_norm), g["s1.grad_norm"])}
    print("%s, R(2+1)D bf16 storage vs the reference fp64 golden: %s" % (name, e))
    assert e["loss_byol"] < 5e-3 and e["loss_total"] < 5e-3 and e["grad_norm"] < 5e-2 and e["logits"] < logits_bar, e


@pytest.mark.parametrize("depth", [1, 18])
def test_r21d_bf16_finetune_wrapper_train_and_eval_mode(depth):
    from cstp_amd.r21d_byol import R21DBYOL
    from oracle import r21d_ft_oracle as fto
    ls = orc.layer_sizes_for_depth(depth)
    fsd = fto.closed_form_state(ls, 11, torch.float32)
    x1, x2, _ = orc.closed_form_clips(4, 8, 56, torch.float32)
    ft = R21DBYOL(pretrain=False, num_classes=11, cls_bn=True, layer_sizes=ls, act_dtype="bf16")
    res = ft.load_state_dict(fsd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    ft.cuda().train()
    o64 = spec.to64(fsd)
    o32 = {k: v.clone() for k, v in fsd.items()}
    with spec.storage("bf16"):
        want_train = spec.ft_forward(o64, x1.double(), ls, True)
        want_eval = spec.ft_forward(o64, x2.double(), ls, False)      # (running statistics moved by the train call)
        e32 = spec.rel(spec.ft_forward(o32, x1, ls, True), want_train)    # the spec's own fp32 run
    with torch.no_grad():
        got_train = ft(x1.to(DEV), o_type="ft_all").cpu()
        ft.eval()
        got_eval = ft(x2.to(DEV), o_type="test").cpu()
    e = (spec.rel(got_train, want_train), spec.rel(got_eval, want_eval))
    print("r21d depth %d bf16 fine-tune wrapper: train / eval vs the spec %.2e %.2e (the spec's own fp32 run, train: %.2e)"
          % ((depth,) + e + (e32,)))
    assert e[0] < max(5e-2, 3.0 * e32) and e[1] < 5e-3, (e, e32)


def test_r21d18_cfg2_bf16_full_size():
    """BASELINE configs[2]'s per-GPU shape (R(2+1)D-18, 16 pairs of 3x16x112x112) with bf16 storage: finite, close to the fp32-storage
    step from the same state; peak memory of both printed."""
    from cstp_amd.synthetic import device_batch
    x1, x2, lab = device_batch(16, 16, 112, DEV, seed=1)
    res = {}
    for act in ("bf16", "fp32"):
        torch.manual_seed(1)
        sd = orc.closed_form_state(orc.layer_sizes_for_depth(18), torch.float32)
        step, a = _pretrain_step(sd, (2, 2, 2, 2), lr=0.01, act=act)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        out = step(x1, x2, lab["spa"], lab["tem"], lab["pb"], lab["rot1"], lab["rot2"])
        torch.cuda.synchronize()
        res[act] = (float(out.loss_total), float(out.grad_norm), torch.cuda.max_memory_allocated(DEV) / 2 ** 30)
        assert np.isfinite(res[act][0]) and np.isfinite(res[act][1]) and bool(torch.isfinite(a["param"]).all())
        del step, a, out
        torch.cuda.empty_cache()
    print("cfg2 R(2+1)D-18: loss / grad norm / peak GiB  bf16 %s  fp32 %s" % (res["bf16"], res["fp32"]))
    assert abs(res["bf16"][0] - res["fp32"][0]) / abs(res["fp32"][0]) < 5e-2, res
    assert abs(res["bf16"][1] - res["fp32"][1]) / abs(res["fp32"][1]) < 2e-1, res


def test_r21d_bf16_pack_plan_covers_the_ragged_weight_packs(monkeypatch):
    """ops.PackPlan with R(2+1)D bf16 storage: the ragged packs (record kind 4, padded k per tap) replayed at the top of the step /
    behind the EMA against seven steps that pack inside every call."""
    from cstp_amd.synthetic import device_batch
    x1, x2, lab = device_batch(2, 8, 56, DEV, seed=3)
    runs = []
    try:
        for plan_on in ("1", "0"):
            monkeypatch.setenv("CSTP_PACK_PLAN", plan_on)
            sd = orc.closed_form_state(orc.layer_sizes_for_depth(18), torch.float32)
            step, a = _pretrain_step(sd, (2, 2, 2, 2))
            assert (step._packs is not None) == (plan_on == "1")
            losses = []
            for _ in range(7):
                out = step(x1, x2, lab["spa"], lab["tem"], lab["pb"], lab["rot1"], lab["rot2"])
                losses.append(float(out.loss_total))
            torch.cuda.synchronize()
            if plan_on == "1":
                st = step._packs.stats
                assert step._packs.state == "replay" and st["recorded_calls"] > 30, st
            runs.append((losses, a["param"].clone(), a["target"].clone()))
        (la, pa, ta), (lb, pb, tb) = runs
        assert max(abs(x - y) / abs(y) for x, y in zip(la, lb)) < 1e-3, list(zip(la, lb))
        assert float((pa - pb).abs().max() / pb.abs().max()) < 1e-2 and float((ta - tb).abs().max() / tb.abs().max()) < 1e-3
    finally:
        ops.pack_plan = None


def test_r21d_bf16_drivers_pretrain_finetune_test(tmp_path):
    """main_byol.py --model_name r21d_byol --act_dtype bf16, then main_ft_mp.py (ft_all) and test.py on its checkpoint, each in
    a fresh child process."""
    common = ["--dataset", "synthetic", "--n_classes", "4", "--batch_size", "8", "--sample_duration", "4", "--sample_size", "32",
              "--model_name", "r21d_byol", "--model_depth", "1", "--n_workers", "0", "--synthetic_len", "16",
              "--result_path", str(tmp_path), "--weight_decay", "1e-4", "--act_dtype", "bf16"]

    def run(script, args):
        r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + common + args, cwd=ROOT, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, (script, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
        return r.stdout
    # checkpoints go out every 100 epochs (main_byol.py): 100 one-iteration epochs write save_100.pth
    run("main_byol.py", ["--task", "loss_com", "--loss_weight", "0.1", "1", "1", "1", "1", "--n_epochs", "100", "--max_steps", "1",
                         "--learning_rate", "0.01"])
    rows = open(str(tmp_path / "synthetic" / "loss_com" / "synthetic_train_clip4modelr21d_byol1.log")).read().strip().split("\n")
    assert len(rows) == 101 and all(np.isfinite(float(r.split("\t")[1])) for r in rows[1:])
    ckpt = str(tmp_path / "synthetic" / "loss_com" / "save_100.pth")
    run("main_ft_mp.py", ["--task", "ft_all", "--pretrained_path", ckpt, "--learning_rate", "0.02", "--n_epochs", "2"])
    d = tmp_path / "synthetic" / "ft_all"
    assert len([f for f in os.listdir(d) if f.endswith("_max.pth")]) == 1
    out = run("test.py", ["--task", "test", "--t_ft_task", "ft_all"])
    assert "Video accuracy" in out

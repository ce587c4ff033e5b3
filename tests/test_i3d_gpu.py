"""I3D-BYOL on a real MI355X: the TensorFlow-SAME max-pool (ops.max_pool3d_same) against ATen on the CPU over every pooling geometry
of the model; the fused BatchNorm + ReLU + concat of the Mixed blocks (ops.bn_relu_concat) against fp64 PyTorch and, bit for bit,
against the composed path; the fine-tune head's small ops; the pre-training step and the fine-tune / eval / test forwards against
golden vectors captured from the reference in fp64 (tests/golden/i3d_*.npz); fused vs CSTP_I3D_FUSED=0; the drivers end to end; one
full-size step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import i3d_spec
from conftest import rel_err
from test_oracle_golden import STATE_TOLS, TOLS, cs_err, rel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
# (branch channels, spatial) of every Mixed block at 16x112x112
BLOCKS = [([p[0], p[2], p[4], p[5]], (8, 14, 14) if name.startswith("mixed_3") else (4, 7, 7) if name.startswith("mixed_4")
           else (2, 4, 4)) for name, (_, p) in i3d_spec.MIXED.items()]
# (kernel, stride, input volume) of every pooling of the model at 16x112x112 and at 16x224x224, then odd extents
POOLS = [((1, 3, 3), (1, 2, 2), (8, 56, 56)), ((1, 3, 3), (1, 2, 2), (8, 28, 28)), ((3, 3, 3), (1, 1, 1), (8, 14, 14)),
         ((3, 3, 3), (2, 2, 2), (8, 14, 14)), ((3, 3, 3), (1, 1, 1), (4, 7, 7)), ((2, 2, 2), (2, 2, 2), (4, 7, 7)),
         ((3, 3, 3), (1, 1, 1), (2, 4, 4)),
         ((1, 3, 3), (1, 2, 2), (8, 112, 112)), ((3, 3, 3), (1, 1, 1), (8, 28, 28)), ((3, 3, 3), (2, 2, 2), (8, 28, 28)),
         ((3, 3, 3), (1, 1, 1), (4, 14, 14)), ((2, 2, 2), (2, 2, 2), (4, 14, 14)), ((3, 3, 3), (1, 1, 1), (2, 7, 7))]
POOLS += [(k, s, v) for v in ((5, 7, 9), (1, 1, 1), (2, 13, 13))
          for k, s in (((3, 3, 3), (1, 1, 1)), ((3, 3, 3), (2, 2, 2)), ((1, 3, 3), (1, 2, 2)), ((2, 2, 2), (2, 2, 2)))]


def load(name):
    return np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


# ---------------------------------------------------------------------------------------------------------------------------
# SAME max-pool
# ---------------------------------------------------------------------------------------------------------------------------
def _pool_ref(x, kernel, stride):
    from cstp_amd.i3d_byol import get_padding_shape
    return F.max_pool3d(F.pad(x, get_padding_shape(kernel, stride)), kernel, stride, ceil_mode=True)


def _pool_hip(x, kernel, stride, dy):
    from cstp_amd import ops
    xg = x.float().cuda().requires_grad_(True)
    y = ops.max_pool3d_same(xg, kernel, stride)
    y.backward(dy.float().cuda())
    torch.cuda.synchronize()
    return y.detach(), xg.grad


@pytest.mark.parametrize("kernel,stride,vol", POOLS)
def test_max_pool3d_same_matches_aten(kernel, stride, vol):
    """Values on a coarse grid (multiples of 0.5 in [-2, 2]: negative values, exact zeros, many ties) so that the zero-padding
    candidates, the first-maximum tie rule and the dropped gradients all show."""
    n, c = (2, 5) if vol[1] <= 28 else (1, 3)
    g = torch.Generator().manual_seed(7 + sum(vol) + kernel[0] + stride[0])
    x = (torch.randint(-4, 5, (n, c) + vol, generator=g).double() * 0.5)
    x[0, 0] = -x[0, 0].abs() - 0.5                         # one all-negative volume: every border window is won by a padding zero
    xr = x.clone().requires_grad_(True)
    yr = _pool_ref(xr, kernel, stride)
    dy = torch.rand(tuple(yr.shape), generator=g, dtype=torch.float64) * 2 - 1
    yr.backward(dy)
    y, dx = _pool_hip(x, kernel, stride, dy)
    assert tuple(y.shape) == tuple(yr.shape)
    assert torch.equal(y.cpu(), yr.detach().float())
    e = rel_err(dx, xr.grad)
    print("max_pool3d_same k%s s%s %s: dx rel_err %.3g" % (kernel, stride, vol, e))
    assert e <= 1e-6
    y2, dx2 = _pool_hip(x, kernel, stride, dy)
    assert torch.equal(y, y2) and torch.equal(dx, dx2)


@pytest.mark.parametrize("kernel,stride,vol", [((3, 3, 3), (1, 1, 1), (4, 7, 7)), ((3, 3, 3), (2, 2, 2), (8, 14, 14)),
                                               ((1, 3, 3), (1, 2, 2), (8, 56, 56))])
def test_max_pool3d_same_nan_rule(kernel, stride, vol):
    """A NaN in a window wins it (ATen replaces on ``val > max || isnan(val)``), a later NaN of the same window replaces an earlier
    one, and the gradient goes to the NaN's position: same NaN mask, same finite values, same dx as ATen on the CPU."""
    g = torch.Generator().manual_seed(5 + sum(vol))
    x = torch.rand((2, 3) + vol, generator=g, dtype=torch.float64) * 2 - 1
    flat = x.view(-1)
    pos = torch.randperm(flat.numel(), generator=g)[:max(4, flat.numel() // 50)]
    flat[pos] = float("nan")
    flat[pos[0].clamp(max=flat.numel() - 2) + 1] = float("nan")          # two neighbours: one window holds more than one NaN
    xr = x.clone().requires_grad_(True)
    yr = _pool_ref(xr, kernel, stride)
    dy = torch.rand(tuple(yr.shape), generator=g, dtype=torch.float64) * 2 - 1
    yr.backward(dy)
    y, dx = _pool_hip(x, kernel, stride, dy)
    yc, yf = y.cpu(), yr.detach().float()
    assert bool(yf.isnan().any()) and torch.equal(yc.isnan(), yf.isnan())
    assert torch.equal(torch.nan_to_num(yc, nan=0.0), torch.nan_to_num(yf, nan=0.0))
    assert not bool(dx.isnan().any()) and not bool(xr.grad.isnan().any())
    assert rel_err(dx, xr.grad) <= 1e-6


def test_max_pool3d_same_model_width_and_one_launch():
    """The 3x3x3 / stride 1 pool on 832 channels (mixed_5b's input), exact against ATen; forward and backward are ONE kernel
    each: no padded copy of the activation is made."""
    from cstp_amd import ops
    g = torch.Generator().manual_seed(3)
    x = torch.randn((4, 832, 2, 4, 4), generator=g)
    yr = _pool_ref(x, (3, 3, 3), (1, 1, 1))
    xg = x.cuda().requires_grad_(True)
    y = ops.max_pool3d_same(xg, (3, 3, 3), (1, 1, 1))
    assert torch.equal(y.detach().cpu(), yr)
    dy = torch.rand_like(y)
    out = {}
    fw = _kernel_names(lambda: out.update(y=ops.max_pool3d_same(xg, (3, 3, 3), (1, 1, 1))))
    bw = _kernel_names(lambda: torch.autograd.backward(out["y"], dy))
    print("pool forward kernels:", fw, "backward kernels:", bw)
    assert len(fw) == 1 and "pool_same" in fw[0]
    assert len([k for k in bw if "pool_same" in k]) == 1 and len(bw) <= 2      # (+ autograd's accumulation into xg.grad)
    with torch.no_grad():
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y = ops.max_pool3d_same(xg, (3, 3, 3), (1, 1, 1))
        torch.cuda.synchronize()
        assert torch.cuda.max_memory_allocated() - base <= y.numel() * 4 + 4096      # the output and nothing else


# ---------------------------------------------------------------------------------------------------------------------------
# BatchNorm + ReLU into the concat
# ---------------------------------------------------------------------------------------------------------------------------
def _bnc_case(cs, spatial, n, seed):
    g = torch.Generator().manual_seed(seed)
    xs = [torch.rand((n, c) + spatial, generator=g, dtype=torch.float64) * 3 - 1.2 for c in cs]
    gammas = [torch.rand((c,), generator=g, dtype=torch.float64) * 2 - 1 for c in cs]
    betas = [(torch.rand((c,), generator=g, dtype=torch.float64) * 2 - 1) * 0.3 for c in cs]
    rms = [(torch.rand((c,), generator=g, dtype=torch.float64) * 2 - 1) * 0.1 for c in cs]
    rvs = [torch.rand((c,), generator=g, dtype=torch.float64) + 0.5 for c in cs]
    dy = torch.rand((n, sum(cs)) + spatial, generator=g, dtype=torch.float64) * 2 - 1
    return xs, gammas, betas, rms, rvs, dy


def _bnc_ref(xs, gammas, betas, rms, rvs, groups, relu=True):
    """fp64 truth; running statistics updated in place, group after group."""
    outs = []
    for x, ga, be, rm, rv in zip(xs, gammas, betas, rms, rvs):
        npg = x.shape[0] // groups
        z = torch.cat([F.batch_norm(x[i * npg:(i + 1) * npg], rm, rv, ga, be, True, 0.1, 1e-5) for i in range(groups)], 0)
        outs.append(F.relu(z) if relu else z)
    return torch.cat(outs, 1)


def _mask_kink(xs, gammas, betas, rms, rvs, groups, dy):
    """ReLU's derivative jumps at 0: where the fp64 pre-activation lies within 1e-4 of it, fp32 rounding may land on the other
    side and the whole dy of that position appears or vanishes in dx -- a property of the function, not an error of either
    implementation.  Those (rare) positions get dy = 0, so the gradient comparison does not depend on them."""
    with torch.no_grad():
        z = _bnc_ref(xs, gammas, betas, [t.clone() for t in rms], [t.clone() for t in rvs], groups, relu=False)
    dy[z.abs() < 1e-4] = 0.0
    return dy


def _conv_sums(x, groups, pivot, nsplit=3):
    """The partial-sum table a convolution leaves beside its output (cstp_conv3d_forward_bnstats): [k][groups][nsplit] sums of
    (x - pivot) and (x - pivot)^2 in fp64, the pivots behind them, then room for the (min, max) keys -- attached to ``x`` the way
    ops.conv3d attaches it, so that batch_norm_act and bn_relu_concat both start from the SAME statistics."""
    n, c = x.shape[0], x.shape[1]
    npg = n // groups
    d = x.detach().double().cpu() - pivot.double().cpu().view(1, c, 1, 1, 1)
    part = torch.zeros(c * groups * nsplit * 3 + c, dtype=torch.float64)
    tab = part[:c * groups * nsplit * 2].view(c, groups, nsplit, 2)
    for g in range(groups):
        for j in range(nsplit):
            rows = d[g * npg + j:(g + 1) * npg:nsplit]
            if rows.numel():
                tab[:, g, j, 0] = rows.sum(dim=(0, 2, 3, 4))
                tab[:, g, j, 1] = (rows * rows).sum(dim=(0, 2, 3, 4))
    part[c * groups * nsplit * 2:c * groups * nsplit * 2 + c] = pivot.double().cpu()
    x._cstp_bnstats = (part.cuda(), nsplit, groups, torch.zeros(1, dtype=torch.int32, device="cuda"), x._version)


def _bnc_hip(xs, gammas, betas, rms, rvs, dy, groups, sums, fused=True):
    from cstp_amd import ops
    xg = [x.float().cuda().requires_grad_(True) for x in xs]
    gg = [t.float().cuda().requires_grad_(True) for t in gammas]
    bg = [t.float().cuda().requires_grad_(True) for t in betas]
    rm = [t.float().cuda() for t in rms]
    rv = [t.float().cuda() for t in rvs]
    if sums:
        for x, m in zip(xg, rm):
            _conv_sums(x, groups, m)
    saved = None
    if fused:
        y = ops.bn_relu_concat(xg, list(zip(gg, bg, rm, rv)), groups)
        nb = len(xg)             # saved: nb inputs, nb weights, save_mean, save_invstd, (scale, shift)
        saved = (y.grad_fn.saved_tensors[2 * nb].view(groups, -1), y.grad_fn.saved_tensors[2 * nb + 1].view(groups, -1))
    else:
        ys = [ops.batch_norm_act(x, ga, be, m, v, None, True, groups=groups) for x, ga, be, m, v in zip(xg, gg, bg, rm, rv)]
        means = [t.grad_fn.saved_tensors[3].view(groups, -1) for t in ys]
        invs = [t.grad_fn.saved_tensors[4].view(groups, -1) for t in ys]
        saved = (torch.cat(means, 1), torch.cat(invs, 1))
        y = torch.cat(ys, 1)
    cell = ops._absmax_of(y)
    y.backward(dy.float().cuda())
    torch.cuda.synchronize()
    return {"y": y.detach(), "cell": cell, "rm": rm, "rv": rv, "saved": saved, "dx": [t.grad for t in xg],
            "dg": [t.grad for t in gg], "db": [t.grad for t in bg]}


@pytest.mark.parametrize("sums", [False, True], ids=["own_stats", "conv_sums"])
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("cs,spatial", BLOCKS + [([24, 7, 130, 1], (3, 5, 3))])
def test_bn_relu_concat_matches_fp64_and_composed(cs, spatial, groups, sums):
    n = 4
    xs, gammas, betas, rms, rvs, dy = _bnc_case(cs, spatial, n, 17 + sum(cs) + groups)
    dy = _mask_kink(xs, gammas, betas, rms, rvs, groups, dy)
    xr = [x.clone().requires_grad_(True) for x in xs]
    gr = [t.clone().requires_grad_(True) for t in gammas]
    br = [t.clone().requires_grad_(True) for t in betas]
    rmr, rvr = [t.clone() for t in rms], [t.clone() for t in rvs]
    yr = _bnc_ref(xr, gr, br, rmr, rvr, groups)
    yr.backward(dy)
    h = _bnc_hip(xs, gammas, betas, rms, rvs, dy, groups, sums)
    assert tuple(h["y"].shape) == tuple(yr.shape)
    errs = {"y": rel_err(h["y"], yr), "rm": max(rel_err(a, b) for a, b in zip(h["rm"], rmr)),
            "rv": max(rel_err(a, b) for a, b in zip(h["rv"], rvr)),
            "dx": max(rel_err(a, b.grad) for a, b in zip(h["dx"], xr)),
            "dgamma": max(rel_err(a, b.grad) for a, b in zip(h["dg"], gr)),
            "dbeta": max(rel_err(a, b.grad) for a, b in zip(h["db"], br))}
    print("bn_relu_concat %s %s groups %d sums %s vs fp64: %s" % (cs, spatial, groups, sums, errs))
    assert errs["y"] <= 1e-6 and errs["rm"] <= 1e-6 and errs["rv"] <= 1e-6
    assert errs["dx"] <= 1e-5 and errs["dgamma"] <= 1e-5 and errs["dbeta"] <= 1e-5
    # the absmax cell: max |y| as fp32 bits, exactly the value the tensor holds
    assert h["cell"] is not None and torch.equal(h["cell"].view(torch.float32).cpu()[0], h["y"].abs().max().cpu())
    # fixed-order reductions, no float atomics: a second run is bit-identical
    h2 = _bnc_hip(xs, gammas, betas, rms, rvs, dy, groups, sums)
    assert torch.equal(h["y"], h2["y"]) and torch.equal(h["cell"], h2["cell"])
    assert all(torch.equal(a, b) for k in ("rm", "rv", "dx", "dg", "db") for a, b in zip(h[k], h2[k]))
    # the composed path: batch_norm_act(relu=True) x 4 + torch.cat
    c = _bnc_hip(xs, gammas, betas, rms, rvs, dy, groups, sums, fused=False)
    if sums:       # both sides start from the convolution's sums: the same bits
        assert torch.equal(h["y"], c["y"])
        assert all(torch.equal(a, b) for k in ("rm", "rv") for a, b in zip(h[k], c[k]))
        assert torch.equal(h["saved"][0], c["saved"][0]) and torch.equal(h["saved"][1], c["saved"][1])
    else:          # each side takes its own statistics pass: the reduction order differs
        assert rel_err(h["y"], c["y"]) <= 1e-6
        assert all(rel_err(a, b) <= 1e-6 for k in ("rm", "rv") for a, b in zip(h[k], c[k]))
        assert rel_err(h["saved"][0], c["saved"][0]) <= 1e-6 and rel_err(h["saved"][1], c["saved"][1]) <= 1e-6
    for k in ("dx", "dg", "db"):      # gradients agree to reduction-order rounding either way
        assert all(rel_err(a, b) <= 1e-5 for a, b in zip(h[k], c[k])), k


def test_bn_relu_concat_launches_and_no_grad():
    """<= 2 launches forward when every branch brings its sums, <= 3 otherwise, <= 3 backward; no_grad saves nothing."""
    from cstp_amd import ops
    from cstp_amd._lib import CstpError
    cs, spatial = BLOCKS[2]
    xs, gammas, betas, rms, rvs, dy = _bnc_case(cs, spatial, 4, 5)
    dyg = dy.float().cuda()
    for sums, limit in ((True, 2), (False, 3)):
        xg = [x.float().cuda().requires_grad_(True) for x in xs]
        bns = [(ga.float().cuda().requires_grad_(True), be.float().cuda().requires_grad_(True), m.float().cuda(), v.float().cuda())
               for ga, be, m, v in zip(gammas, betas, rms, rvs)]
        if sums:
            for x, b in zip(xg, bns):
                _conv_sums(x, 2, b[2])
        ops.bn_relu_concat(xg, bns, 2).backward(dyg)          # warm-up (library load, workspace)
        out = {}
        fw = _kernel_names(lambda: out.update(y=ops.bn_relu_concat(xg, bns, 2)))
        bw = _kernel_names(lambda: torch.autograd.backward(out["y"], dyg))
        print("sums %s forward kernels:" % sums, fw, "backward kernels:", bw)
        assert len(fw) <= limit and all("bnc_" in k for k in fw)
        assert (len(fw) == 2) == sums
        assert len([k for k in bw if "bnc_" in k]) <= 3
        # what else the backward pass launches is autograd's gradient accumulation into the 12 existing .grad tensors, not the op
        assert len([k for k in bw if "bnc_" not in k]) <= 12
    # (two samples: every tensor of the call stays below the caching allocator's 1 MiB small-block limit, where a block is
    #  exactly the request rounded up to 512 B)
    xh = [x.detach()[:2].contiguous() for x in xg]
    with torch.no_grad():
        y = ops.bn_relu_concat(xh, bns, 2)           # (the workspace exists by now)
        del y
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y = ops.bn_relu_concat(xh, bns, 2)
        torch.cuda.synchronize()
        peak, kept = torch.cuda.max_memory_allocated() - base, torch.cuda.memory_allocated() - base
    ybytes, cbytes = y.numel() * 4, 2 * sum(cs) * 4
    print("no_grad bn_relu_concat: output %d B, peak +%d B, kept +%d B" % (ybytes, peak, kept))
    # while it runs: the output, save_mean / save_invstd [2][C], the (scale, shift) table [2][C][2], the absmax cell (each rounded
    # up to the allocator's 512 B); afterwards: the output and the cell it is tagged with -- nothing is saved for a backward
    assert peak <= ybytes + 4 * cbytes + 5 * 512
    assert kept <= ybytes + 2 * 512
    assert y.grad_fn is None and tuple(y.shape) == (2, sum(cs)) + spatial and ybytes < 2 ** 20
    with pytest.raises(CstpError, match="one N, D, H, W"):
        ops.bn_relu_concat([xg[0], torch.rand(4, cs[1], 4, 7, 8, device="cuda")], bns[:2], 2)
    with pytest.raises(CstpError, match="weight and bias"):
        ops.bn_relu_concat([xg[0]], [bns[1]], 2)


def test_bn_relu_concat_eval_equals_batch_norm_eval():
    from cstp_amd import ops
    cs, spatial = BLOCKS[4]
    xs, gammas, betas, rms, rvs, _ = _bnc_case(cs, spatial, 3, 9)
    xg = [x.float().cuda() for x in xs]
    bns = [tuple(t.float().cuda() for t in b) for b in zip(gammas, betas, rms, rvs)]
    with torch.no_grad():
        y = ops.bn_relu_concat_eval(xg, bns)
        ref = torch.cat([ops.batch_norm_eval(x, *b, relu=True) for x, b in zip(xg, bns)], 1)
    assert torch.equal(y, ref)
    yr = torch.cat([F.relu(F.batch_norm(x, m, v, ga, be, False, 0.1, 1e-5)) for x, ga, be, m, v in zip(xs, gammas, betas, rms, rvs)], 1)
    assert rel_err(y, yr) <= 1e-6
    assert torch.equal(ops._absmax_of(y).view(torch.float32).cpu()[0], y.abs().max().cpu())


# ---------------------------------------------------------------------------------------------------------------------------
# the fine-tune head's ops
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vol,kernel", [((3, 8, 8), (2, 7, 7)), ((2, 7, 7), (2, 7, 7)), ((4, 9, 7), (2, 7, 7)), ((3, 4, 5), (1, 2, 3))])
def test_avg_pool3d_window(vol, kernel):
    from cstp_amd import ops
    g = torch.Generator().manual_seed(21)
    x = (torch.rand((2, 6) + vol, generator=g, dtype=torch.float64) * 2 - 1).requires_grad_(True)
    y = F.avg_pool3d(x, kernel, (1, 1, 1))
    dy = torch.rand(tuple(y.shape), generator=g, dtype=torch.float64) * 2 - 1
    y.backward(dy)
    xg = x.detach().float().cuda().requires_grad_(True)
    yg = ops.avg_pool3d_window(xg, kernel)
    yg.backward(dy.float().cuda())
    assert tuple(yg.shape) == tuple(y.shape)
    assert rel_err(yg, y) <= 1e-6 and rel_err(xg.grad, x.grad) <= 1e-6


@pytest.mark.parametrize("n,t,k", [(2, 1, 11), (4, 1, 101), (2, 3, 11), (2, 8, 5)])
def test_classifier_convolution_7x1x1(n, t, k):
    """conv3d_0c_1x1_custom: a bare 1024 -> n_classes (7, 1, 1) convolution with padding (3, 0, 0) on a map whose time extent is 1
    at 16 frames (six of its seven taps see only padding).  Forward, dx and dw against fp64 F.conv3d at the convolution bar of
    tests/test_ops_gpu.py (1e-4)."""
    from cstp_amd import ops
    g = torch.Generator().manual_seed(31 + t)
    x = (torch.rand((n, 1024, t, 1, 1), generator=g, dtype=torch.float64) * 2 - 1).requires_grad_(True)
    w = ((torch.rand((k, 1024, 7, 1, 1), generator=g, dtype=torch.float64) * 2 - 1) * 0.05).requires_grad_(True)
    y = F.conv3d(x, w, None, 1, (3, 0, 0))
    dy = torch.rand(tuple(y.shape), generator=g, dtype=torch.float64) * 2 - 1
    y.backward(dy)
    xg = x.detach().float().cuda().requires_grad_(True)
    wg = w.detach().float().cuda().requires_grad_(True)
    yg = ops.conv3d(xg, wg, None, 1, (3, 0, 0))
    assert tuple(yg.shape) == tuple(y.shape)
    yg.backward(dy.float().cuda())
    torch.cuda.synchronize()
    e = (rel_err(yg, y), rel_err(xg.grad, x.grad), rel_err(wg.grad, w.grad))
    print("classifier conv n %d t %d k %d: y %.3g dx %.3g dw %.3g" % ((n, t, k) + e))
    assert max(e) < 1e-4
    assert rel_err(ops.global_avg_pool(yg), y.squeeze(3).squeeze(3).mean(2)) < 1e-4


# ---------------------------------------------------------------------------------------------------------------------------
# the model against the reference's golden vectors
# ---------------------------------------------------------------------------------------------------------------------------
def _build_pretrain(sd):
    from cstp_amd.i3d_byol import I3DBYOL
    m = I3DBYOL(pretrain=True, opts=None)
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    m.cuda()
    m.flatten_parameters()
    return m.train()


# A quantity passes under the project's usual bar, or within this factor of what the reference's own fp32 run leaves against the
# same fp64 truth (recorded per fixture as fp32.fwd / fp32.dev by make_golden_i3d.py) -- the rule of tests/test_s3dg_gpu.py: I3D's
# last Mixed blocks normalise over few values per channel too (4 per view at 8x64x64, 32 at 16x112x112).
HIP_VS_FP32 = 4.0


def _tol(base, dev):
    return max(base, HIP_VS_FP32 * float(dev))


# the smallest case also runs with the target forward on the main stream (ByolBase._two_view_step's serial branch); the ids of
# the existing cases are unchanged
GOLDEN_CASES = ["i3d_small", "i3d_112"]
@pytest.mark.parametrize("name,overlap", [pytest.param(n, True if n == "i3d_small" else None, id=n) for n in GOLDEN_CASES]
                         + [pytest.param("i3d_small", False, id="i3d_small-serial")])
def test_i3d_pretrain_matches_reference_golden(name, overlap, monkeypatch):
    if overlap is not None:
        from cstp_amd import r21d_byol
        monkeypatch.setattr(r21d_byol, "OVERLAP_TARGET_FORWARD", overlap)
    from cstp_amd.optim import FlatSGD
    from cstp_amd.train import PretrainStep
    from oracle import r21d_byol_oracle as orc
    from oracle import r3d_byol_oracle as r3d
    g = load(name)
    b, t, hw, steps = [int(v) for v in g["meta"]]
    dev = g["fp32.dev"]
    sd = i3d_spec.closed_form(i3d_spec.model_spec(), torch.float32)
    keys = list(sd.keys())
    x1, x2, _ = orc.closed_form_clips(b, t, hw, torch.float32)
    x1d, x2d = x1.cuda(), x2.cuda()
    lab = {k: v.cuda() for k, v in r3d.closed_form_labels(b).items()}
    model = _build_pretrain(sd)
    with torch.no_grad():
        f1 = model.online_net(x1d)
        f2 = model.online_net(x2d)
        p1, p2 = model.predictor(f1), model.predictor(f2)
        model._update_target_net()
        t1 = model.target_net(x1d)
        t2 = model.target_net(x2d)
    for i, (k, v) in enumerate((("feat_1", f1), ("feat_2", f2), ("pred_1", p1), ("pred_2", p2), ("tfeat_1", t1), ("tfeat_2", t2))):
        e = rel(v.cpu().numpy(), g["fwd." + k])
        print("%s fwd.%s: HIP %.3g, reference fp32 %.3g" % (name, k, e, g["fp32.fwd"][i]))
        assert e < _tol(TOLS[1][0], g["fp32.fwd"][i]), k

    model = _build_pretrain(sd)
    opt = FlatSGD(model.parameters(), lr=float(g["lr"]), momentum=0.9, weight_decay=float(g["wd"]),
                  arenas=model.flatten_parameters())
    step = PretrainStep(model, opt, tuple(g["loss_weight"]), clip_grad_norm=True)
    pkeys = [str(k) for k in g["param_keys"]]
    for s in range(1, steps + 1):
        pre = "s%d." % s
        tol = _tol(TOLS[s][0], dev[s - 1][2])
        gtol = _tol(TOLS[s][1], dev[s - 1][3])
        out = step(x1d, x2d, lab["spa"], lab["tem"], lab["pb"], lab["rot1"], lab["rot2"])
        lg = torch.cat([l.cpu() for l in out.logits], 1).numpy()        # [B, 5 + 5 + 4 x 4], as the fixture stores them
        print("%s step %d: logits HIP %.3g (reference fp32 %.3g), grad_norm HIP %.3g (reference fp32 %.3g)"
              % (name, s, rel(lg, g[pre + "logits"]), dev[s - 1][2], rel(float(out.grad_norm), g[pre + "grad_norm"]), dev[s - 1][3]))
        assert rel(float(out.loss_byol), g[pre + "loss_byol"]) < tol
        assert rel(float(out.loss_total), g[pre + "loss_total"]) < tol
        assert rel([float(c) for c in out.ce], g[pre + "ce"]) < tol
        assert rel(lg, g[pre + "logits"]) < tol
        assert rel(float(out.grad_norm), g[pre + "grad_norm"]) < gtol
        # .grad holds the CLIPPED gradient after the fused optimizer pass: undo the coefficient (clip_grad_norm_, main_byol.py:89)
        coef = min(1.0, 18.0 / (float(out.grad_norm) + 1e-6))
        gn = {k: float(p.grad.norm()) / coef for k, p in model.named_parameters() if p.requires_grad}
        gn = np.array([gn.get(k, -1.0) for k in pkeys])
        ref_gn = g[pre + "grad_norms"]
        per = np.abs(gn - ref_gn) / np.maximum(np.abs(ref_gn), 1e-3 * np.abs(ref_gn).max())
        worst = [(pkeys[i], float(gn[i]), float(ref_gn[i])) for i in np.argsort(-per)[:5]]
        print("%s step %d: grad_norms HIP %.3g (reference fp32 %.3g), worst tensors %s" % (name, s, rel(gn, ref_gn), dev[s - 1][4], worst))
        assert rel(gn, ref_gn) < _tol(TOLS[s][1], dev[s - 1][4]), worst
        st = model.state_dict()
        cs = np.array([[float(st[k].double().sum()), float(st[k].double().abs().sum())] for k in keys])
        osd = opt.state_dict()["state"]
        mcs = np.array([[float(osd[i]["momentum_buffer"].double().sum()), float(osd[i]["momentum_buffer"].double().abs().sum())]
                        if i in osd else [0.0, 0.0] for i in range(len(pkeys))])
        print("%s step %d: state_cs HIP %.3g (reference fp32 %.3g), mom_cs HIP %.3g (reference fp32 %.3g)"
              % (name, s, cs_err(cs, g[pre + "state_cs"]), dev[s - 1][5], cs_err(mcs, g[pre + "mom_cs"]), dev[s - 1][6]))
        assert cs_err(cs, g[pre + "state_cs"]) < _tol(STATE_TOLS[s], dev[s - 1][5])
        assert cs_err(mcs, g[pre + "mom_cs"]) < _tol(gtol, dev[s - 1][6])
    msd = model.state_dict()
    assert int(msd["online_net.conv3d_1a_7x7.batch3d.num_batches_tracked"]) == 2 * steps
    assert int(msd["online_net.mixed_4d.branch_2.1.batch3d.num_batches_tracked"]) == 2 * steps
    assert int(msd["target_net.mixed_5c.branch_3.1.batch3d.num_batches_tracked"]) == 2 * steps
    assert int(msd["predictor.net.1.num_batches_tracked"]) == 2 * steps
    assert model.last_projections[0].shape == (b, 1024)


def test_i3d_finetune_eval_test_match_reference_golden():
    from cstp_amd.i3d_byol import I3DBYOL, get_fine_tuning_parameters
    from oracle import r21d_ft_oracle as ftorc
    name = "i3d_ft_all"
    g = load(name)
    b, t, hw, k, steps = [int(v) for v in g["meta"]]
    task = str(g["task"])
    sd = i3d_spec.closed_form(i3d_spec.ft_spec(k), torch.float32)
    import types
    model = I3DBYOL(pretrain=False, opts=types.SimpleNamespace(n_classes=k))
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    model.cuda()
    params = get_fine_tuning_parameters(model, 0)
    opt = torch.optim.SGD(params, lr=float(g["lr"]), momentum=0.9, weight_decay=float(g["wd"]))
    x_train, x_val, labels = ftorc.closed_form_batch(b, t, hw, k, dtype=torch.float32)
    xt, xv, lab = x_train.cuda(), x_val.cuda(), labels.cuda()
    assert np.array_equal([p.requires_grad for p in model.parameters()], g["requires_grad"])
    for s in range(1, steps + 1):
        pre = "s%d." % s
        tol = TOLS[s][0]
        model.train()
        outputs = model(xt, o_type=task)
        assert tuple(outputs.shape) == (b, k)
        loss = F.cross_entropy(outputs, lab)
        opt.zero_grad()
        loss.backward()
        gn = np.array([float(p.grad.norm()) if p.grad is not None else -1.0 for p in model.parameters()])
        opt.step()
        dv = g["fp32.dev"][s - 1]   # the reference's own fp32 run: [loss, logits, grad_norms, val_logits, video_mean, state checksums]
        st = model.state_dict()
        cs = np.array([[float(v.double().sum()), float(v.double().abs().sum())] for v in st.values()])
        e_state = cs_err(cs, g[pre + "state_cs"])       # the SGD update itself: every tensor after the step, before the eval forwards
        e = {"loss": rel(float(loss.detach()), g[pre + "loss"]), "logits": rel(outputs.detach().cpu().numpy(), g[pre + "logits"])}
        ref_gn = g[pre + "grad_norms"]
        assert np.array_equal(gn < 0, ref_gn < 0)
        live = ref_gn >= 0
        e["grad_norms"] = rel(gn[live], ref_gn[live])
        model.eval()
        with torch.no_grad():
            e["val_logits"] = rel(model(xv, o_type=task).cpu().numpy(), g[pre + "val_logits"])
            vid = model(xv, None, o_type="test").mean(dim=0, keepdim=True)
            e["video_mean"] = rel(vid.cpu().numpy(), g[pre + "video_mean"])
        print("%s step %d: (HIP, reference fp32) %s" % (name, s, {kk: (v, float(d)) for (kk, v), d in zip(e.items(), dv)}))
        assert e["loss"] < _tol(tol, dv[0]) and e["logits"] < _tol(tol, dv[1])
        assert e["grad_norms"] < _tol(TOLS[s][1], dv[2])
        assert e["val_logits"] < _tol(2e-3, dv[3]) and e["video_mean"] < _tol(2e-3, dv[4])
        print("%s step %d: state_cs HIP %.3g (reference fp32 %.3g)" % (name, s, e_state, float(dv[5])))
        assert e_state < _tol(STATE_TOLS[s], dv[5])


# ---------------------------------------------------------------------------------------------------------------------------
# child processes: the A/B switch, the drivers
# ---------------------------------------------------------------------------------------------------------------------------
def _run(args, timeout, extra_env=None):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env.update(extra_env or {})
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args[0], r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


_ONE_STEP = r"""
import json, sys, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
import i3d_spec
from cstp_amd import i3d_byol
from cstp_amd.optim import FlatSGD
from cstp_amd.train import PretrainStep
from oracle import r21d_byol_oracle as orc
from oracle import r3d_byol_oracle as r3d
m = i3d_byol.I3DBYOL(pretrain=True, opts=None)
m.load_state_dict(i3d_spec.closed_form(i3d_spec.model_spec(), torch.float32), strict=True)
m.cuda(); arenas = m.flatten_parameters(); m.train()
opt = FlatSGD(m.parameters(), lr=0.005, momentum=0.9, weight_decay=5e-4, arenas=arenas)
step = PretrainStep(m, opt, (0.1, 1.0, 1.0, 1.0, 1.0), clip_grad_norm=True)
x1, x2, _ = orc.closed_form_clips(4, 8, 64, torch.float32)
lab = {k: v.cuda() for k, v in r3d.closed_form_labels(4).items()}
out = step(x1.cuda(), x2.cuda(), lab["spa"], lab["tem"], lab["pb"], lab["rot1"], lab["rot2"])
torch.cuda.synchronize()
print("RESULT " + json.dumps({"fused": i3d_byol.FUSED, "loss_byol": float(out.loss_byol), "loss_total": float(out.loss_total),
                              "grad_norm": float(out.grad_norm),
                              "logits": torch.cat([l.cpu() for l in out.logits], 1).tolist()}))
"""


def test_fused_and_composed_paths_agree(tmp_path):
    """CSTP_I3D_FUSED=0 (F.pad + ATen max_pool3d(ceil_mode=True), per-branch batch_norm_act, torch.cat) computes what the fused
    kernels do: one pre-training step at the i3d_small size in two child processes (the switch is read at import)."""
    script = tmp_path / "one_step.py"
    script.write_text(_ONE_STEP % (ROOT, os.path.join(ROOT, "tests")))
    res = {}
    for flag in ("1", "0"):
        out = _run([str(script)], 600, {"CSTP_I3D_FUSED": flag})
        res[flag] = json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    assert res["1"]["fused"] is True and res["0"]["fused"] is False
    for k in ("loss_byol", "loss_total"):
        assert rel(res["1"][k], res["0"][k]) < 1e-6, (k, res["1"][k], res["0"][k])
    e = rel(np.array(res["1"]["logits"]), np.array(res["0"]["logits"]))
    print("fused vs composed: logits %.3g, grad_norm %.6f vs %.6f" % (e, res["1"]["grad_norm"], res["0"]["grad_norm"]))
    assert e < 1e-6


def test_i3d_driver_chain(tmp_path):
    """main_byol.py --model_name i3d_byol on synthetic clips (100 one-step epochs: the driver checkpoints every 100), its
    checkpoint fine-tuned by main_ft_mp.py --task ft_all at 16x224x224 (loaded through neq_load_customized: the classifier
    convolution keeps its initialisation), the best fine-tune checkpoint tested by test.py -- each a child process with a time
    limit.  No model-specific code in any driver."""
    res = str(tmp_path)
    pre = ["--dataset", "synthetic", "--sample_duration", "8", "--sample_size", "64", "--model_name", "i3d_byol",
           "--model_depth", "1", "--n_workers", "0", "--result_path", res]
    _run(["main_byol.py"] + pre + ["--batch_size", "4", "--synthetic_len", "4", "--task", "loss_com", "--loss_weight", "0.1",
                                   "1", "1", "1", "1", "--n_epochs", "100", "--learning_rate", "0.005", "--weight_decay", "5e-4"],
         900)
    ckpt = os.path.join(res, "synthetic", "loss_com", "save_100.pth")
    md = torch.load(ckpt, map_location="cpu")
    assert md["arch"] == "i3d_byol-1"
    assert [k[len("module."):] for k in md["state_dict"]] == [k for k, _, _ in i3d_spec.model_spec()]
    assert all(torch.isfinite(v.float()).all() for v in md["state_dict"].values())
    ft = ["--dataset", "synthetic", "--sample_duration", "16", "--sample_size", "224", "--model_name", "i3d_byol",
          "--model_depth", "1", "--n_workers", "0", "--result_path", res, "--n_classes", "4", "--batch_size", "4",
          "--synthetic_len", "8", "--weight_decay", "1e-4"]
    _run(["main_ft_mp.py"] + ft + ["--task", "ft_all", "--pretrained_path", ckpt, "--learning_rate", "0.01", "--n_epochs", "2"], 900)
    d = os.path.join(res, "synthetic", "ft_all")
    best = [f for f in os.listdir(d) if f.endswith("_max.pth")]
    assert len(best) == 1
    fmd = torch.load(os.path.join(d, best[0]), map_location="cpu")
    assert [k[len("module."):] for k in fmd["state_dict"]] == [k for k, _, _ in i3d_spec.ft_spec(4)]
    assert all(torch.isfinite(v.float()).all() for v in fmd["state_dict"].values())
    out = _run(["test.py"] + ft + ["--task", "test", "--t_ft_task", "ft_all"], 900)
    assert "Video accuracy" in out


def test_i3d_full_size_step():
    """BASELINE-size step: 16 clip pairs of 3x16x112x112 through PretrainStep; finite loss and gradients, peak memory reported."""
    from cstp_amd.i3d_byol import I3DBYOL
    from cstp_amd.optim import FlatSGD
    from cstp_amd.train import PretrainStep
    torch.manual_seed(0)
    model = I3DBYOL(pretrain=True, opts=None).cuda()
    arenas = model.flatten_parameters()
    model.train()
    opt = FlatSGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=5e-4, arenas=arenas)
    step = PretrainStep(model, opt, (0.1, 1.0, 1.0, 1.0, 1.0), clip_grad_norm=True)
    b = 16
    g = torch.Generator(device="cuda").manual_seed(0)
    x1 = torch.rand((b, 3, 16, 112, 112), device="cuda", generator=g) * 2 - 1
    x2 = torch.rand((b, 3, 16, 112, 112), device="cuda", generator=g) * 2 - 1
    lab = [torch.randint(0, 5, (b,), device="cuda", generator=g) for _ in range(2)]
    lab += [torch.randint(0, 4, (b,), device="cuda", generator=g) for _ in range(3)]
    torch.cuda.reset_peak_memory_stats()
    out = step(x1, x2, *lab)
    torch.cuda.synchronize()
    print("i3d_byol B=16 pairs 3x16x112x112: loss_total %.4f grad_norm %.3f peak memory %.2f GiB"
          % (float(out.loss_total), float(out.grad_norm), torch.cuda.max_memory_allocated() / 2 ** 30))
    assert np.isfinite(float(out.loss_total)) and np.isfinite(float(out.grad_norm))
    assert bool(torch.isfinite(arenas["grad"]).all()) and bool(torch.isfinite(arenas["param"]).all())

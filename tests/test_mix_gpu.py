"""Label smoothing / mixup / CutMix on a real MI355X: the soft-target cross-entropy kernels (cstp_soft_cross_entropy_*) and the
clip blend (cstp_clip_mix) against fp64 PyTorch, their launch counts inside FineTuneStep, the step itself under a mixer and
main_ft_mp.py with the new flags.

Bars.  Loss / gradient: 1e-5 of the largest magnitude -- the same expression evaluated in fp32 on a CPU sits at 1.9e-7 (loss) /
2.6e-7 (gradient) from fp64 on exactly these cases; a dropped eps/k term at k = 1000 is 1e-4.  mixup: 1e-6 of the largest
magnitude (two fp32 products and a sum: the fp32 CPU blend measures 6.7e-8).  Copies and CutMix: bit equality."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"

CE_SHAPES = [(1, 2), (3, 5), (5, 7), (16, 101), (7, 400), (64, 51), (33, 1000)]


# ---- soft-target cross-entropy -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ce_case(b, k):
    """logits uniform in +-3, two targets, lam random with one row exactly 1 and one exactly 0 (b = 1: the row is 1)."""
    g = torch.Generator().manual_seed(1000 * b + k)
    logits = (torch.rand((b, k), generator=g, dtype=torch.float64) * 6 - 3).float()
    ta = torch.randint(0, k, (b,), generator=g)
    tb = torch.randint(0, k, (b,), generator=g)
    lam = torch.rand((b,), generator=g, dtype=torch.float32)
    lam[-1] = 0.0
    lam[0] = 1.0
    return logits, ta, tb, lam


def _q64(ta, tb, lam, eps, k):
    q = (1.0 - eps) * (lam.double()[:, None] * F.one_hot(ta, k).double() + (1.0 - lam.double())[:, None] * F.one_hot(tb, k).double())
    return q + eps / k


@functools.lru_cache(maxsize=None)
def _ce_reference(b, k, eps):
    """(loss, dlogits) of F.cross_entropy(logits, q) in fp64 with the upstream gradient 1.7."""
    logits, ta, tb, lam = _ce_case(b, k)
    x = logits.double().requires_grad_(True)
    loss = F.cross_entropy(x, _q64(ta, tb, lam, eps, k))
    (loss * 1.7).backward()
    return loss.detach(), x.grad


def _run_soft_ce(logits, ta, tb, lam, eps):
    from cstp_amd import ops
    x = logits.to(DEV).requires_grad_(True)
    d = lambda t: None if t is None else t.to(DEV)
    loss = ops.soft_cross_entropy(x, d(ta), d(tb), d(lam), eps)
    (loss * 1.7).backward()
    return loss.detach().cpu(), x.grad.cpu()


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("b,k", CE_SHAPES)
def test_soft_cross_entropy_matches_fp64(b, k, eps):
    logits, ta, tb, lam = _ce_case(b, k)
    want_loss, want_grad = _ce_reference(b, k, eps)
    loss, grad = _run_soft_ce(logits, ta, tb, lam, eps)
    e_loss = abs(float(loss) - float(want_loss)) / abs(float(want_loss))
    e_grad = float((grad.double() - want_grad).abs().max() / want_grad.abs().max())
    print("soft CE b=%d k=%d eps=%g: loss %.3e  dlogits %.3e" % (b, k, eps, e_loss, e_grad))
    assert loss.shape == () and grad.shape == (b, k)
    assert e_loss < 1e-5 and e_grad < 1e-5
    loss2, grad2 = _run_soft_ce(logits, ta, tb, lam, eps)                   # fixed-order reductions: equal bits
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


@pytest.mark.parametrize("b,k", CE_SHAPES)
def test_soft_cross_entropy_single_target_forms(b, k):
    from cstp_amd import ops
    logits, ta, tb, lam = _ce_case(b, k)
    ones = torch.ones(b)
    # eps = 0, lam = 1 is the hard-label loss
    x = logits.to(DEV).requires_grad_(True)
    hard = ops.cross_entropy(x, ta.to(DEV))
    (hard * 1.7).backward()
    hard = hard.detach()
    loss, grad = _run_soft_ce(logits, ta, tb, ones, 0.0)
    assert abs(float(loss) - float(hard)) <= 1e-5 * abs(float(hard))
    assert float((grad - x.grad.cpu()).abs().max()) <= 1e-5 * float(x.grad.abs().max())
    # tb = None is tb = ta; lam = None is lam = 1; both are F.cross_entropy(logits, ta, label_smoothing=eps)
    want = F.cross_entropy(logits.double(), ta, label_smoothing=0.1)
    for args in ((ta, None, lam), (ta, ta, lam), (ta, None, None), (ta, tb, None), (ta, tb, ones)):
        got, _ = _run_soft_ce(logits, *args, 0.1)
        assert abs(float(got) - float(want)) <= 1e-5 * abs(float(want)), args
    a, ga = _run_soft_ce(logits, ta, None, lam, 0.1)
    c, gc = _run_soft_ce(logits, ta, ta, lam, 0.1)
    assert torch.equal(a, c) and torch.equal(ga, gc)


def test_soft_cross_entropy_ignores_targets_outside_the_classes():
    """A target outside [0, k) carries no one-hot mass and is never an index: the loss is that of q without it."""
    b, k, eps = 5, 7, 0.1
    logits, ta, tb, lam = _ce_case(b, k)
    ta, tb = ta.clone(), tb.clone()
    ta[1], tb[2], ta[3], tb[3] = k, -1, 1 << 40, -(1 << 40)
    q = torch.full((b, k), eps / k, dtype=torch.float64)
    for r in range(b):
        if 0 <= int(ta[r]) < k:
            q[r, ta[r]] += (1 - eps) * float(lam[r])
        if 0 <= int(tb[r]) < k:
            q[r, tb[r]] += (1 - eps) * (1 - float(lam[r]))
    x = logits.double().requires_grad_(True)
    want = -(q * F.log_softmax(x, dim=1)).sum(dim=1).mean()
    (want * 1.7).backward()
    want_grad = x.grad                                                      # = 1.7 * (softmax * sum_c q - q) / b
    loss, grad = _run_soft_ce(logits, ta, tb, lam, eps)
    assert abs(float(loss) - float(want)) < 1e-5 * abs(float(want))
    assert float((grad.double() - want_grad).abs().max()) < 1e-5 * float(want_grad.abs().max())


# ---- clip blend ----------------------------------------------------------------------------------------------------------------
MIX_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (4, 6, 8, 12), (4, 12, 28, 28), "view"]


@functools.lru_cache(maxsize=None)
def _clip_host(shape):
    if shape == "view":
        shape = (3, 2, 9, 16)
    g = torch.Generator().manual_seed(sum(shape))
    return torch.rand(shape, generator=g, dtype=torch.float64).float() * 2 - 1


def _clip(shape):
    """The case on the device; "view" is (3, 2, 9, 16) one float into its buffer: w % 4 == 0 but unaligned -> the scalar path."""
    x = _clip_host(shape)
    if shape != "view":
        return x, x.to(DEV)
    buf = torch.zeros(x.numel() + 1, device=DEV)
    xd = buf[1:].view(x.shape)
    xd.copy_(x)
    assert xd.data_ptr() % 16 == 4 and xd.is_contiguous()
    return x, xd


def _boxes(h, w):
    boxes = [(0, 0, 0, 0), (h // 2, h // 2, 0, w), (0, h, w // 2, w // 2),                        # empty
             (0, h, 0, w),                                                                        # the whole frame
             (0, 1, 0, w), (h - 1, h, 0, w), (0, h, 0, 1), (0, h, w - 1, w),                      # the four borders
             (0, max(h // 2, 1), 0, max(w // 2, 1)), (h // 2, h, w // 2, w),                      # corners
             (h // 2, h // 2 + 1, w // 2, w // 2 + 1),                                            # one pixel
             (1, h - 1, 1, w - 1), (0, h, 3, 6), (2, 5, 5, 7), (0, h, 2, 3), (1, h, 6, w - 2), (0, 1, 1, w)]  # x0 / x1 off the groups
    ok = [b for b in boxes if 0 <= b[0] <= b[1] <= h and 0 <= b[2] <= b[3] <= w]
    return sorted(set(ok))


@pytest.mark.parametrize("shape", MIX_SHAPES, ids=str)
def test_clip_mix_mixup(shape):
    from cstp_amd import ops
    x, xd = _clip(shape)
    b = x.shape[0]
    partner = [(i + 1) % b for i in range(b)]
    before = xd.clone()
    for lam in (0.0, 1.0, 0.3):
        y = ops.clip_mix(xd, partner, 1, lam)
        l32 = float(np.float32(lam))
        want = l32 * x.double() + (1.0 - l32) * x.double()[partner]
        err = float((y.cpu().double() - want).abs().max() / want.abs().max())
        print("mixup %s lam=%g: %.3e" % (shape, lam, err))
        assert y.shape == x.shape and y.data_ptr() != xd.data_ptr() and err < 1e-6
        if lam == 1.0:
            assert torch.equal(y, xd)
    assert torch.equal(ops.clip_mix(xd, list(range(b)), 1, 0.3), xd)                 # its own partner: a copy, bit for bit
    assert torch.equal(ops.clip_mix(xd, list(range(b)), 2, 0.3, (0, x.shape[-2], 0, x.shape[-1])), xd)
    assert torch.equal(ops.clip_mix(xd, partner, 0, 0.3, (0, x.shape[-2], 0, x.shape[-1])), xd)      # mode 0 ignores the rest
    assert torch.equal(xd, before)                                                   # x is read only


@pytest.mark.parametrize("shape", MIX_SHAPES, ids=str)
def test_clip_mix_cutmix_copies_bits(shape):
    from cstp_amd import ops
    x, xd = _clip(shape)
    b, h, w = x.shape[0], x.shape[-2], x.shape[-1]
    partner = [(i + 1) % b for i in range(b)]
    before = xd.clone()
    for (y0, y1, x0, x1) in _boxes(h, w):
        want = x.clone()
        want[:, :, y0:y1, x0:x1] = x[partner][:, :, y0:y1, x0:x1]
        got = ops.clip_mix(xd, partner, 2, 0.5, (y0, y1, x0, x1)).cpu()
        assert torch.equal(got, want), (shape, (y0, y1, x0, x1))
    # a different box per sample in one table
    boxes = (_boxes(h, w) * b)[3:3 + b]
    want = x.clone()
    for i, (y0, y1, x0, x1) in enumerate(boxes):
        want[i, :, y0:y1, x0:x1] = x[partner[i], :, y0:y1, x0:x1]
    assert torch.equal(ops.clip_mix(xd, partner, 2, 0.5, boxes).cpu(), want)
    assert torch.equal(xd, before)


def test_clip_mix_one_table_mixes_the_modes():
    from cstp_amd import ops
    x, xd = _clip((4, 12, 28, 28))
    x5 = xd.view(4, 3, 4, 28, 28)                                                    # a [B, 3, T, S, S] batch, as the step passes it
    partner, mode, lam = [2, 0, 3, 3], [0, 1, 2, 1], [1.0, 0.25, 0.5, 0.75]
    boxes = [(0, 0, 0, 0), (0, 0, 0, 0), (3, 17, 5, 22), (1, 2, 3, 4)]
    y = ops.clip_mix(x5, partner, mode, lam, boxes)
    assert y.shape == x5.shape
    y = y.view(4, 12, 28, 28).cpu()
    assert torch.equal(y[0], x[0])
    want1 = 0.25 * x[1].double() + 0.75 * x[0].double()
    assert float((y[1].double() - want1).abs().max()) < 1e-6 * float(want1.abs().max())
    want2 = x[2].clone()
    want2[:, 3:17, 5:22] = x[3][:, 3:17, 5:22]
    assert torch.equal(y[2], want2)
    assert torch.equal(y[3], x[3])                                                   # its own partner


# ---- inside the step -------------------------------------------------------------------------------------------------------------
NEW_KERNELS = ("clip_mix_kernel", "soft_ce_fwd_kernel", "soft_ce_bwd_kernel")


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


@functools.lru_cache(maxsize=None)
def _ft_inputs():
    from oracle import r21d_byol_oracle as orc
    from oracle import r21d_ft_oracle as fto
    sd = fto.closed_form_state((1, 1, 1, 1), 11, torch.float32)
    x, _, _ = orc.closed_form_clips(4, 8, 56, torch.float32)
    return sd, x, (torch.arange(4, dtype=torch.int64) * 7 + 3) % 11


def _ft_step(mixer, act_dtype="fp32"):
    from cstp_amd.optim import FlatSGD
    from cstp_amd.r21d_byol import R21DBYOL, get_fine_tuning_parameters
    from cstp_amd.train import FineTuneStep
    sd, x, lab = _ft_inputs()
    kw = {} if act_dtype == "fp32" else {"act_dtype": act_dtype}
    model = R21DBYOL(pretrain=False, num_classes=11, cls_bn=True, layer_sizes=(1, 1, 1, 1), **kw)
    model.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    model.cuda().train()
    arenas = model.flatten_parameters()
    opt = FlatSGD(get_fine_tuning_parameters(model, 0), lr=0.01, momentum=0.9, weight_decay=1e-4, arenas=arenas)
    return model, FineTuneStep(model, opt, "ft_all", mixer=mixer), x.to(DEV), lab.to(DEV)


def _count(names):
    return [sum(k in n for n in names) for k in NEW_KERNELS]


def test_launch_counts():
    from cstp_amd.mix import Mixer
    _, step, x, lab = _ft_step(None)
    step(x, lab)                                                                     # warm-up: library load, tile lookup
    assert _count(_kernel_names(lambda: step(x, lab))) == [0, 0, 0]                  # the default step launches nothing new
    mixer = Mixer(0.1, 1.0, 1.0, 1.0, 0.5, seed=1)
    _, step, x, lab = _ft_step(mixer)
    step(x, lab)
    names = _kernel_names(lambda: step(x, lab))
    assert not step.last_plan.identity
    assert _count(names) == [1, 1, 1], [n for n in names if any(k in n for k in NEW_KERNELS)]
    _, step, x, lab = _ft_step(Mixer(0.1, 1.0, 1.0, 0.0, 0.5, seed=1))               # prob 0: identity plans
    step(x, lab)
    names = _kernel_names(lambda: step(x, lab))
    assert step.last_plan.identity and _count(names) == [0, 1, 1]


def _soft_ce64(outputs, lab, plan, eps):
    k = outputs.shape[1]
    lam = torch.full((lab.shape[0],), float(np.float32(plan.lam)))
    q = _q64(lab, lab[torch.tensor(plan.partner)], lam, eps, k)
    return float(F.cross_entropy(outputs.double().cpu(), q))


def test_step_under_a_mixer():
    from cstp_amd import ops
    from cstp_amd.mix import MODE_CUTMIX, MODE_MIXUP, Mixer
    mixer = Mixer(0.1, 1.0, 1.0, 1.0, 0.5, seed=1)
    model, step, x, lab = _ft_step(mixer)
    seen = []
    model.register_forward_pre_hook(lambda mod, args: seen.append(args[0]))
    modes = set()
    for s in range(3):
        loss, outputs = step(x, lab)
        plan = mixer.plan(4, 56, 56, 0, s, 0)                                        # re-derived from (seed, epoch, step, rank)
        assert step.last_plan == plan and not plan.identity
        modes.add(plan.mode)
        want = _soft_ce64(outputs, lab.cpu(), plan, 0.1)
        print("step %d mode %d lam %.3f: loss %.6f (fp64 of the outputs %.6f)" % (s, plan.mode, plan.lam, float(loss), want))
        assert abs(float(loss) - want) < 1e-5 * abs(want)
        assert torch.equal(seen[-1], ops.clip_mix(x, plan.partner, plan.mode, plan.lam, plan.box))
        heavier = lab if plan.lam >= 0.5 else lab[torch.tensor(plan.partner, device=DEV)]
        assert torch.equal(step.accuracy_targets(lab), heavier)
    assert modes == {MODE_MIXUP, MODE_CUTMIX}                                        # this seed's first three plans hold both
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    step.set_epoch(4)                                                                # positions the plan
    step(x, lab)
    assert step.last_plan == mixer.plan(4, 56, 56, 4, 0, 0)


def test_identity_mixer_is_the_plain_step():
    from cstp_amd.mix import Mixer
    _, plain, x, lab = _ft_step(None)
    _, mixed, _, _ = _ft_step(Mixer(0.0, 1.0, 1.0, 0.0, 0.5, seed=1))                # mix_prob 0, no smoothing
    a, _ = plain(x, lab)
    b, _ = mixed(x, lab)
    assert mixed.last_plan.identity
    assert abs(float(a) - float(b)) <= 1e-5 * abs(float(a))


def test_step_under_a_mixer_bf16_storage():
    from cstp_amd.mix import Mixer
    mixer = Mixer(0.1, 1.0, 1.0, 1.0, 0.5, seed=1)
    model, step, x, lab = _ft_step(mixer, act_dtype="bf16")
    for s in range(2):
        loss, outputs = step(x, lab)
        assert step.last_plan == mixer.plan(4, 56, 56, 0, s, 0)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(outputs).all())
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def _run(args, timeout):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args[0], r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.parametrize("flags", [["--label_smoothing", "0.1", "--mixup_alpha", "0.8", "--cutmix_alpha", "1.0"], []],
                         ids=["mixing", "defaults"])
def test_finetune_driver(tmp_path, flags):
    _run(["main_ft_mp.py", "--task", "scratch", "--dataset", "synthetic", "--model_name", "r21d_byol", "--model_depth", "1",
          "--n_classes", "4", "--batch_size", "8", "--sample_duration", "4", "--sample_size", "32", "--n_epochs", "2",
          "--result_path", str(tmp_path)] + flags, 600)
    d = tmp_path / "synthetic" / "scratch"
    for kind, cols in (("train", 4), ("val", 3)):
        rows = open(str(d / ("synthetic_%s_clip4modelr21d_byol1.log" % kind))).read().strip().split("\n")
        assert len(rows) == 3 and [r.split("\t")[0] for r in rows[1:]] == ["1", "2"], rows
        for r in rows[1:]:
            vals = [float(v) for v in r.split("\t")]
            assert len(vals) == cols and all(np.isfinite(vals)), r
    assert len([f for f in os.listdir(str(d)) if f.endswith("_max.pth")]) == 1

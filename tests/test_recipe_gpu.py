"""The fine-tuning recipe on a real MI355X: TableSGD / TableAdam (cstp_tab_sgd_step / cstp_tab_adam_step, the EMA in the same launch)
against the restatement of tests/recipe_spec.py run in fp64 on CPU tensors -- not the code under test -- on the hand-built arena
and the three steps of tests/test_lars_gpu.py; bit equality with FlatSGD / FlatAdam where the hyper-parameters are uniform; the
arena invariants; launch counts; two FineTuneSteps on real models; ema_applied; and the drivers in child processes.

Every comparison is PER TENSOR (conftest.rel_err: max-abs-diff / max-abs-ref).  Bars: SGD (p, written-back g, buf, ema) 1e-6, what
test_ops_gpu.test_flat_utils and test_lars_gpu hold the SGD kernels to; Adam / AdamW (p, m, v, ema) 1e-5, the bar of
test_ops_edges_gpu.test_adam_step_edges.  The same restatement run in fp32 on the CPU stays inside both on these inputs (asserted
below, so an input that is too hard for fp32 shows up as such)."""
import functools
import os
import subprocess
import sys

import pytest
import torch

import recipe_spec
from conftest import rel_err
from test_lars_gpu import STEPS, Arena, _values
from test_reg_gpu import B, HW, K, T, _clips, _kernel_names, _state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TOL = {"sgd": 1e-6, "adam": 1e-5, "adamw": 1e-5}
LR, MOM, BETAS, EPS = 0.1, 0.9, (0.9, 0.99), 1e-8
EMA_M = 0.2              # update 1 runs at (1 + 1) / (10 + 1) < 0.2, updates 2 and 3 at 0.2: both sides of the warm-up
SCALES = (1.0, 0.5, 0.125)
DECAYS = (5e-4, 1e-4)
ZERO_W, ZERO_G = 8, 2    # the all-zero weight (8, 8); (5, 7) gets an all-zero gradient on step 2, which also runs without decay


def _shapes():
    from cstp_amd import ops
    return [(1, 1), (3, 1), (5, 7), (64,), (17,), (1023, 3), (64, 3, 1, 7, 7), (2 * ops.LARS_CHUNK + 5, 1), (8, 8)]


def _scale(i):
    return SCALES[i % 3]


def _decay(i, step_wd):
    """Two decays mixed over the tensors; the step of test_lars_gpu.STEPS that runs at weight decay 0 runs every tensor at 0."""
    return 0.0 if step_wd == 0.0 else DECAYS[(i // 2) % 2]


def _weights(shapes):
    w = _values(shapes, 1, 0)
    w[ZERO_W] = torch.zeros(shapes[ZERO_W], dtype=torch.float64)
    return w


def _grads(shapes, step):
    gs = _values(shapes, 100 + step, 3 + step)
    if step == 1:
        gs[ZERO_G] = torch.zeros(shapes[ZERO_G], dtype=torch.float64)
    return gs


def _make(kind, plist, arenas, table=True):
    from cstp_amd.optim import FlatAdam, FlatSGD, TableAdam, TableSGD
    if kind == "sgd":
        return (TableSGD if table else FlatSGD)(plist, lr=LR, momentum=MOM, weight_decay=DECAYS[0], arenas=arenas)
    return (TableAdam if table else FlatAdam)(plist, lr=LR, betas=BETAS, eps=EPS, weight_decay=DECAYS[0], decoupled=kind == "adamw",
                                              arenas=arenas)


def _state_arenas(opt):
    return [opt._buf] if hasattr(opt, "_buf") else [opt._m, opt._v]


def _run_three_steps(kind, frozen=(), ema=True, uniform=False, table=True):
    """-> the arena, the optimizer and per step the arenas (p, g, state..., ema) after it.  ``uniform``: every scale 1, one decay, one
    parameter list (what FlatSGD / FlatAdam serve in one run); otherwise one group per tensor with mixed scales and decays."""
    shapes = _shapes()
    a = Arena(shapes, _weights(shapes), frozen)
    if uniform:
        plist = a.params
    else:
        plist = [dict({"params": p, "lr_scale": _scale(i), "weight_decay": _decay(i, STEPS[0][1])}, **({} if p.requires_grad else {"lr": 0.0}))
                 for i, p in enumerate(a.params)]
    opt = _make(kind, plist, a.arenas, table)
    if ema:
        opt.enable_ema(EMA_M)
    snaps = []
    for step, (c, wd) in enumerate(STEPS):
        for i, g in enumerate(opt.param_groups):
            g["weight_decay"] = wd if uniform else _decay(i, wd)
        a.set_grads(_grads(shapes, step))
        if c is not None:
            opt._coef.fill_(c)
            opt._clip_pending = True
        opt.step()
        snaps.append([a.arenas["param"].clone(), a.arenas["grad"].clone()] + [s.clone() for s in _state_arenas(opt)] +
                     ([opt._ema.clone()] if ema else []))
    torch.cuda.synchronize()
    return a, opt, snaps


@functools.lru_cache(maxsize=None)
def _three_steps(kind):
    return _run_three_steps(kind)


@functools.lru_cache(maxsize=None)
def _reference(kind):
    """The restatement over the same three steps, per step and tensor: {dtype: [[(p, g, state..., ema)]]} in fp64 and in fp32."""
    shapes = _shapes()
    out = {}
    for dt in (torch.float64, torch.float32):
        p = [v.float().to(dt) for v in _weights(shapes)]                      # the fp32 values the device holds
        state = [[torch.zeros_like(v) for v in p] for _ in range(1 if kind == "sgd" else 2)]
        ema = [v.clone() for v in p]
        steps = []
        for step, (c, wd) in enumerate(STEPS):
            gs = [g.float().to(dt) for g in _grads(shapes, step)]
            cf = 1.0 if c is None else float(torch.tensor(c, dtype=torch.float32))       # the coefficient is an fp32 device scalar
            res = []
            for i in range(len(shapes)):
                if kind == "sgd":
                    pn, gn, bn = recipe_spec.sgd_step(p[i], gs[i], state[0][i], cf, LR, _scale(i), MOM, _decay(i, wd), step == 0)
                    new = [bn]
                else:
                    gn = cf * gs[i]                                                       # FlatAdam's pre-pass writes c * g back
                    pn, mn, vn = recipe_spec.adam_step(p[i], gn, state[0][i], state[1][i], LR, _scale(i), BETAS[0], BETAS[1], EPS,
                                                       _decay(i, wd), kind == "adamw", step + 1)
                    new = [mn, vn]
                en = recipe_spec.ema_update(ema[i], pn, EMA_M, step + 1)
                p[i], ema[i] = pn, en
                for s, n in zip(state, new):
                    s[i] = n
                res.append([pn, gn] + new + [en])
            steps.append(res)
        out[dt] = steps
    return out


KINDS = ["sgd", "adam", "adamw"]


@pytest.mark.parametrize("kind", KINDS)
def test_fp32_restatement_is_inside_the_bar(kind):
    ref = _reference(kind)
    for s64, s32 in zip(ref[torch.float64], ref[torch.float32]):
        for t64, t32 in zip(s64, s32):
            for x, y in zip(t32, t64):
                if float(y.abs().max()) > 0:
                    assert rel_err(x, y) < TOL[kind]


@pytest.mark.parametrize("kind", KINDS)
def test_op_level_parity_per_tensor(kind):
    a, _, snaps = _three_steps(kind)
    shapes, worst = a.shapes, {}
    names = ["p", "g"] + (["buf"] if kind == "sgd" else ["m", "v"]) + ["ema"]
    for step, (arenas, ref) in enumerate(zip(snaps, _reference(kind)[torch.float64])):
        assert len(arenas) == len(names)
        for arena in arenas:
            assert bool(torch.isfinite(arena).all())
        for i, wants in enumerate(ref):
            for name, arena, want in zip(names, arenas, wants):
                got = a.tensor(arena, i)
                if float(want.abs().max()) == 0.0:
                    assert float(got.abs().max()) == 0.0, (step, shapes[i], name)
                    continue
                e = rel_err(got, want)
                worst[name] = max(worst.get(name, 0.0), e)
                assert e < TOL[kind], (kind, step, shapes[i], name, e)
    print("%s: worst per-tensor errors over three steps: %s" % (kind, worst))
    # the hyper-parameters were really per tensor: the uniform step from the same state lands elsewhere
    _, _, plain = _run_three_steps(kind, ema=False, uniform=True)
    assert _scale(2) != 1.0 and rel_err(a.tensor(snaps[0][0], 2), a.tensor(plain[0][0], 2)) > 1e-2


@pytest.mark.parametrize("kind", KINDS)
def test_uniform_hyper_parameters_give_the_single_run_kernels_bits(kind):
    """All scales 1, one decay, no EMA: p, g and the state arenas equal FlatSGD's / FlatAdam's after each of the three steps."""
    _, topt, table = _run_three_steps(kind, ema=False, uniform=True)
    _, fopt, flat = _run_three_steps(kind, ema=False, uniform=True, table=False)
    assert type(topt).__name__.startswith("Table") and type(fopt).__name__.startswith("Flat")
    for s, (x, y) in enumerate(zip(table, flat)):
        assert len(x) == len(y) == (3 if kind == "sgd" else 4)
        for name, u, v in zip("pgsv", x, y):
            assert torch.equal(u, v), (kind, s, name, float((u - v).abs().max()))


@pytest.mark.parametrize("kind", KINDS)
def test_padding_stays_bit_zero_and_two_runs_give_the_same_bits(kind):
    a, _, snaps = _three_steps(kind)
    m = a.pad_mask()
    assert int(m.sum()) > 0
    for arenas in snaps:
        for arena in arenas:
            assert bool((arena.cpu()[m].view(torch.int32) == 0).all())
    _, _, again = _run_three_steps(kind)
    for s1, s2 in zip(snaps, again):
        for x, y in zip(s1, s2):
            assert torch.equal(x, y)


@pytest.mark.parametrize("kind", KINDS)
def test_frozen_tensors_and_their_shadow_are_left_alone(kind):
    frozen = (1, 4, 7)
    a, opt, snaps = _run_three_steps(kind, frozen=frozen)
    assert len(opt._plan()) == 4                                             # the frozen tensors split the arena; nothing else does
    w = _weights(a.shapes)
    ref = _reference(kind)[torch.float64][-1]
    final = snaps[-1]
    for i in range(len(a.shapes)):
        if i in frozen:
            want = w[i].float()
            assert torch.equal(a.tensor(final[0], i).cpu(), want) and torch.equal(a.tensor(final[-1], i).cpu(), want)
            for state in final[2:-1]:
                assert float(a.tensor(state, i).abs().max()) == 0.0
            continue
        for arena, want in zip([final[0]] + final[2:], [ref[i][0]] + ref[i][2:]):
            if float(want.abs().max()) == 0.0:
                assert float(a.tensor(arena, i).abs().max()) == 0.0
            else:
                assert rel_err(a.tensor(arena, i), want) < TOL[kind], (a.shapes[i],)
    assert sorted(opt.state_dict()["state"]) == [i for i in range(len(a.shapes)) if i not in frozen]


def _launches(fn):
    """Kernel names of one call (torch wraps Optimizer.step in a profiler range of its own, which is not a launch)."""
    return [n for n in _kernel_names(fn) if not n.startswith("Optimizer.step#")]


def test_one_optimizer_launch_per_step_whatever_the_grouping():
    shapes = _shapes()
    for kind, kernel, plain in (("sgd", "tab_sgd_kernel", "sgd_kernel"), ("adamw", "tab_adam_kernel", "adam_kernel")):
        a, opt, _ = _run_three_steps(kind, ema=False)
        a.set_grads(_grads(shapes, 0))
        names = _launches(opt.step)
        assert len(names) == 1 and kernel in names[0], names
        a, opt, _ = _run_three_steps(kind, ema=True)
        names = _launches(opt.step)                                      # the EMA rides in the same launch
        assert len(names) == 1 and kernel in names[0], names
        # the same groups through the runs of _plan(): one launch per run of equal hyper-parameters
        a, flat, _ = _run_three_steps(kind, ema=False, table=False)
        names = [n for n in _launches(flat.step) if plain in n and "tab_" not in n]
        assert len(names) == len(flat._plan()) > 1, names


# ---- on real models: two FineTuneSteps with --layer_decay 0.75 --wd_skip_1d 1 --model_ema 0.9 ------------------------------------
FT_LR, FT_WD, FT_DECAY, FT_EMA = 0.01, 1e-4, 0.75, 0.9


def _build(model, state=None):
    import argparse
    from cstp_amd.r21d_byol import R21DBYOL
    from cstp_amd.r3d_byol import R3DBYOL
    if model == "r21d":
        m = R21DBYOL(pretrain=False, num_classes=K, cls_bn=True, layer_sizes=(1, 1, 1, 1))
    else:
        m = R3DBYOL(pretrain=False, cls_bn=True, opts=argparse.Namespace(model_depth=10, sample_size=HW, sample_duration=T, sc_type="B",
                                                                        n_classes=K, act_dtype="fp32"))
    m.load_state_dict({k: v.clone() for k, v in (_state(model) if state is None else state).items()}, strict=True)
    m.cuda().train()
    m.flatten_parameters()
    return m


def _table_sgd(m):
    from cstp_amd import recipe
    from cstp_amd.optim import TableSGD
    groups = recipe.param_groups(m, m.parameters(), FT_DECAY, FT_WD, True)
    opt = TableSGD(groups, lr=FT_LR, momentum=MOM, weight_decay=FT_WD, arenas=m.flatten_parameters())
    opt.enable_ema(FT_EMA)
    return opt, groups


@functools.lru_cache(maxsize=None)
def _model_run(model):
    from cstp_amd.train import FineTuneStep
    m = _build(model)
    opt, groups = _table_sgd(m)
    step = FineTuneStep(m, opt, "ft_all")
    named = list(m.named_parameters())
    arenas = m.flatten_parameters()
    x, lab = _clips()
    xd, ld = x.cuda(), lab.cuda()
    records = []
    for s in range(2):
        before = {k: p.detach().double().cpu() for k, p in named}
        step(xd, ld)
        records.append(dict(before=before, after={k: p.detach().clone() for k, p in named},
                            grad={k: p.grad.detach().double().cpu() for k, p in named},
                            ema=opt._ema.clone(), buffers=arenas["buffers"].clone(), ema_buffers=opt._ema_buffers.clone()))
    torch.cuda.synchronize()
    return m, opt, step, groups, named, records


@pytest.mark.parametrize("model", ["r21d", "r3d"])
def test_two_finetune_steps_on_a_real_model(model):
    from cstp_amd import recipe
    m, opt, _, groups, named, records = _model_run(model)
    assert len(opt._plan()) == 1 and len(opt.param_groups) == len(named)
    ids = recipe.layer_ids(m)
    top = max(ids.values())
    arenas = m.flatten_parameters()
    p0 = {k: torch.as_tensor(v).double() for k, v in _state(model).items()}
    bufs = {k: torch.zeros(p.shape, dtype=torch.float64) for k, p in named}
    ema = {k: p0[k].float().double() for k, _ in named}
    ema_b = None
    skipped = decayed = 0
    for s, r in enumerate(records):
        worst = 0.0
        for (k, p), g in zip(named, groups):
            scale, wd = FT_DECAY ** (top - ids[k]), (0.0 if p.dim() <= 1 else FT_WD)
            assert g["lr_scale"] == scale and g["weight_decay"] == wd
            skipped, decayed = skipped + (wd == 0.0), decayed + (wd != 0.0)
            # FineTuneStep does not clip: .grad holds what the optimizer met
            want, _, bufs[k] = recipe_spec.sgd_step(r["before"][k], r["grad"][k], bufs[k], 1.0, FT_LR, scale, MOM, wd, s == 0)
            ema[k] = recipe_spec.ema_update(ema[k], want, FT_EMA, s + 1)
            off = (p.data_ptr() - arenas["param"].data_ptr()) // 4
            e = max(rel_err(r["after"][k], want), rel_err(r["ema"][off:off + p.numel()].view_as(p), ema[k]))
            worst = max(worst, e)
            assert e < TOL["sgd"], (model, s, k, e)
        # the BatchNorm statistics' shadow follows the buffer arena with the same momentum
        ema_b = recipe_spec.ema_update(torch.as_tensor(_buffers0(model)).double() if ema_b is None else ema_b, r["buffers"].double().cpu(),
                                       FT_EMA, s + 1)
        assert rel_err(r["ema_buffers"], ema_b) < TOL["sgd"]
        print("%s step %d: worst per-tensor parameter / shadow error %.3g" % (model, s + 1, worst))
    assert skipped > 10 and decayed > 10 and top == 5


@functools.lru_cache(maxsize=None)
def _buffers0(model):
    return _build(model).flatten_parameters()["buffers"].cpu()


def test_ema_applied_swaps_in_the_shadow_and_back_bit_for_bit():
    from cstp_amd import recipe
    m, opt, step, _, _, records = _model_run("r21d")
    arenas = m.flatten_parameters()
    x, lab = _clips()
    xd, ld = x.cuda(), lab.cuda()
    raw_p, raw_b = arenas["param"].clone(), arenas["buffers"].clone()
    shadow_p, shadow_b = opt._ema.clone(), opt._ema_buffers.clone()
    assert not torch.equal(raw_p, shadow_p) and not torch.equal(raw_b, shadow_b)
    sd_raw = {k: v.clone() for k, v in m.state_dict().items()}
    sd_ema = recipe.ema_state_dict(m, m, opt)
    assert list(sd_ema) == list(sd_raw) and torch.equal(arenas["param"], raw_p)
    m.eval()
    with torch.no_grad():
        raw_logits = m(xd, o_type="ft_all")
        with recipe.ema_applied(m, opt):
            assert torch.equal(arenas["param"], shadow_p) and torch.equal(arenas["buffers"], shadow_b)
            assert torch.equal(opt._ema, raw_p)
            ema_logits = m(xd, o_type="ft_all")
    assert torch.equal(arenas["param"], raw_p) and torch.equal(arenas["buffers"], raw_b)
    assert torch.equal(opt._ema, shadow_p) and torch.equal(opt._ema_buffers, shadow_b)
    assert all(torch.equal(v, sd_raw[k]) for k, v in m.state_dict().items())
    assert not torch.equal(ema_logits, raw_logits)
    fresh = _build("r21d", sd_ema).eval()
    with torch.no_grad():
        assert torch.equal(fresh(xd, o_type="ft_all"), ema_logits)
    # the shadows load back from such a dict, and the next training step runs
    opt._ema.zero_()
    recipe.load_ema_state_dict(m, m, opt, sd_ema)
    assert torch.equal(opt._ema, shadow_p) and torch.equal(opt._ema_buffers, shadow_b) and torch.equal(arenas["param"], raw_p)
    m.train()
    loss, _ = step(xd, ld)
    assert bool(torch.isfinite(loss)) and not torch.equal(arenas["param"], raw_p) and not torch.equal(opt._ema, shadow_p)
    with pytest.raises(ValueError, match="enable_ema"):
        from cstp_amd.optim import FlatSGD
        with recipe.ema_applied(m, FlatSGD(m.parameters(), lr=0.1, arenas=arenas)):
            pass


def test_lars_takes_the_ema_as_a_separate_pass():
    from cstp_amd.optim import FlatLARS
    shapes = _shapes()
    a = Arena(shapes, _weights(shapes), (1,))
    plist = [{"params": p} if p.requires_grad else {"params": p, "lr": 0.0} for p in a.params]
    opt = FlatLARS(plist, lr=LR, momentum=MOM, weight_decay=5e-4, eta=1e-3, arenas=a.arenas)
    opt.enable_ema(EMA_M)
    before = a.arenas["param"].clone()
    a.set_grads(_grads(shapes, 0))
    opt.step()
    m = recipe_spec.ema_momentum(EMA_M, 1)
    for i in range(len(shapes)):
        if i == 1:
            assert torch.equal(a.tensor(opt._ema, i), a.tensor(before, i))
        elif i != ZERO_W:
            want = m * a.tensor(before, i).double().cpu() + (1.0 - m) * a.tensor(a.arenas["param"], i).double().cpu()
            assert rel_err(a.tensor(opt._ema, i), want) < TOL["sgd"]


# ---- the drivers -----------------------------------------------------------------------------------------------------------------
def _run(args, timeout=600, ok=True):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert (r.returncode == 0) == ok, (args[0], r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r


def test_finetune_driver_with_the_flags_on_and_off_then_test(tmp_path):
    from cstp_amd.r21d_byol import R21DBYOL
    keys = ["module." + k for k in R21DBYOL(pretrain=False, num_classes=4, cls_bn=True, layer_sizes=(1, 1, 1, 1)).state_dict().keys()]
    common = ["--dataset", "synthetic_video", "--sample_duration", "8", "--sample_size", "112", "--model_name", "r21d_byol",
              "--model_depth", "1", "--n_workers", "0", "--n_classes", "4", "--batch_size", "4", "--synthetic_len", "16",
              "--weight_decay", "1e-4", "--pb_rate", "4"]
    train = ["--transform_mode", "img", "--task", "scratch", "--learning_rate", "0.01", "--n_epochs", "2", "--max_steps", "2"]
    test = ["--transform_mode", "img_test", "--task", "test", "--t_ft_task", "scratch"]

    def best(res):
        d = os.path.join(res, "synthetic_video", "scratch")
        found = [f for f in os.listdir(d) if f.endswith("_max.pth")]
        assert len(found) == 1
        return torch.load(os.path.join(d, found[0]), map_location="cpu")

    on = str(tmp_path / "on")
    out = _run(["main_ft_mp.py"] + common + train + ["--result_path", on, "--layer_decay", "0.75", "--wd_skip_1d", "1", "--model_ema", "0.9",
                                                     "--lr_schedule", "cosine", "--warmup_epochs", "1", "--min_lr", "1e-5"]).stdout
    assert "layer_decay=0.75" in out and "Optimizer: TableSGD" in out
    assert "Lr 0.005000" in out                                          # iteration 1 of a two-iteration warm-up to 0.01
    md = best(on)
    assert list(md["state_dict"].keys()) == keys and list(md["state_dict_ema"].keys()) == keys
    assert all(bool(torch.isfinite(v.float()).all()) for v in md["state_dict_ema"].values())
    assert any(not torch.equal(md["state_dict"][k], md["state_dict_ema"][k]) for k in keys)
    groups = md["optimizer"]["param_groups"]
    assert len(groups) == len([k for k in keys if "running_" not in k and "num_batches" not in k])
    assert groups[0]["lr_scale"] == 0.75 ** 5 and groups[-1]["lr_scale"] == 1.0
    assert "Video accuracy" in _run(["test.py"] + common + test + ["--result_path", on, "--test_ema", "1"]).stdout

    off = str(tmp_path / "off")
    assert "Optimizer: FlatSGD" in _run(["main_ft_mp.py"] + common + train + ["--result_path", off]).stdout
    md = best(off)
    assert sorted(md) == ["arch", "epoch", "optimizer", "state_dict"] and list(md["state_dict"].keys()) == keys
    groups = md["optimizer"]["param_groups"]                                # FlatSGD on model.parameters(): one group, no lr_scale
    assert len(groups) == 1 and "lr_scale" not in groups[0] and groups[0]["lr"] == 0.01
    r = _run(["test.py"] + common + test + ["--result_path", off, "--test_ema", "1"], ok=False)
    assert "--test_ema 1" in r.stderr and "state_dict_ema" in r.stderr

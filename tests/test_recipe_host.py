"""The fine-tuning recipe (--layer_decay, --wd_skip_1d, --model_ema, --lr_schedule cosine), the parts that need no GPU: layer ids
and parameter groups on CPU-built models, the table builder, the merged _plan() and the checkpoint format of the table optimizers
on CPU arena tensors, the schedule against its closed form (tests/recipe_spec.py), the EMA momentum warm-up, every flag refusal,
and that the defaults build what the driver built before."""
import argparse
import ctypes
import math

import pytest
import torch

import recipe_spec
from test_abi import header_symbols
from test_lars_host import _cpu_model, _declared_arity, _layout

NAMES = ("cstp_tab_sgd_step", "cstp_tab_adam_step")


# ---- models on the CPU -------------------------------------------------------------------------------------------------------------
def _model(name, depth):
    from cstp_amd.r21d_byol import R21DBYOL, layer_sizes_for_depth
    from cstp_amd.r3d_byol import R3DBYOL
    if name == "r21d_byol":
        return R21DBYOL(pretrain=False, num_classes=5, cls_bn=True, layer_sizes=layer_sizes_for_depth(depth))
    return R3DBYOL(pretrain=False, cls_bn=True, opts=argparse.Namespace(model_depth=depth, sample_size=32, sample_duration=8, sc_type="B",
                                                                      n_classes=5, act_dtype="fp32"))


CASES = [("r21d_byol", 1, 4), ("r21d_byol", 18, 8), ("r3d_byol", 10, 4), ("r3d_byol", 18, 8)]


@pytest.mark.parametrize("name,depth,blocks", CASES)
def test_layer_ids_cover_every_parameter_in_order(name, depth, blocks):
    from cstp_amd.recipe import layer_ids
    m = _model(name, depth)
    ids = layer_ids(m)
    names = [n for n, _ in m.named_parameters()]
    assert list(ids) == names                                               # every parameter, registration order
    top = blocks + 1
    assert len(m.residual_blocks()) == blocks
    seq = [ids[n] for n in names]
    assert seq == sorted(seq) and set(seq) == set(range(top + 1))           # monotone, every layer present
    for n in names:
        if n.startswith(("online_net.conv1.", "online_net.bn1.")):
            assert ids[n] == 0, n
        elif not n.startswith("online_net."):
            assert ids[n] == top, n                                         # classify, cls_bn / classify_bn
        else:
            assert 1 <= ids[n] <= blocks, n
    assert ids["classify.weight"] == top and ids["classify.bias"] == top
    for b, block in enumerate(m.residual_blocks(), 1):
        mine = {id(p) for p in block.parameters()}
        assert all(ids[n] == b for n, p in m.named_parameters() if id(p) in mine)


def test_layer_ids_refuse_an_encoder_parameter_outside_the_numbering():
    from cstp_amd.recipe import layer_ids
    m = _model("r21d_byol", 1)
    m.online_net.extra = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError, match="online_net.extra"):
        layer_ids(m)


def test_layer_ids_refuse_backbones_without_residual_blocks():
    from cstp_amd.recipe import layer_ids
    from cstp_amd.s3dg_byol import S3DGBYOL
    with pytest.raises(ValueError, match="--layer_decay"):
        layer_ids(S3DGBYOL(pretrain=False, gating=True, slow=False, num_classes=5))


def test_param_groups_scales_decays_and_frozen_conventions():
    from cstp_amd.r21d_byol import get_fine_tuning_parameters
    from cstp_amd.recipe import layer_ids, param_groups
    m = _model("r21d_byol", 1)
    ids, top = layer_ids(m), 5
    named = list(m.named_parameters())
    groups = param_groups(m, m.parameters(), 0.75, 1e-4, True)
    assert len(groups) == len(named)
    for (n, p), g in zip(named, groups):
        assert g["params"] is p and "lr" not in g
        assert g["lr_scale"] == 0.75 ** (top - ids[n])
        assert g["weight_decay"] == (0.0 if p.dim() <= 1 else 1e-4)
    assert groups[-1]["lr_scale"] == 1.0 and groups[0]["lr_scale"] == 0.75 ** 5
    assert any(p.dim() <= 1 for _, p in named) and any(p.dim() > 1 for _, p in named)
    # without the skip every tensor is decayed; at layer_decay 1 every scale is 1 and no layer numbering is needed
    for g in param_groups(m, m.parameters(), 1.0, 1e-4, False):
        assert g["lr_scale"] == 1.0 and g["weight_decay"] == 1e-4
    # the ft_fc list of get_fine_tuning_parameters: frozen tensors stay listed, at lr 0.0, in the same order
    plan = get_fine_tuning_parameters(m, 5)
    groups = param_groups(m, plan, 1.0, 1e-4, True)
    assert [g["params"] for g in groups] == [e["params"] for e in plan]
    for (n, p), g in zip(named, groups):
        if n.startswith("classify."):
            assert p.requires_grad and "lr" not in g
        else:
            assert not p.requires_grad and g["lr"] == 0.0
    with pytest.raises(ValueError):
        param_groups(m, [torch.nn.Parameter(torch.zeros(3))], 1.0, 0.0, False)


# ---- tables ------------------------------------------------------------------------------------------------------------------------
def test_hyper_tables_chunks_stay_inside_one_tensor_and_skip_frozen_ones():
    from cstp_amd import ops
    from cstp_amd.optim import hyper_tables
    C = ops.LARS_CHUNK
    shapes = [(1,), (3, 1), (4,), (5, 1), (64,), (C - 1,), (C, 1), (C + 1,), (2 * C + 5, 1)]
    frozen = 4
    offs, total = _layout(shapes)
    live = [i for i in range(len(shapes)) if i != frozen]
    numel = lambda i: int(torch.Size(shapes[i]).numel())
    slots = [(offs[i], numel(i), 0.5 ** i, 1e-4 * (i % 2)) for i in live]
    chunks, hyper = hyper_tables(slots, C)
    assert hyper == [(0.5 ** i, 1e-4 * (i % 2)) for i in live]
    hits = [0] * total
    for seg, off, length in chunks:
        i = live[seg]
        assert off % 4 == 0 and length % 4 == 0 and 0 < length <= C
        assert offs[i] <= off and off + length <= offs[i] + (numel(i) + 3) // 4 * 4
        for k in range(off, off + length):
            hits[k] += 1
    for i in range(len(shapes)):
        pad = (numel(i) + 3) // 4 * 4
        assert set(hits[offs[i]:offs[i] + pad]) == ({0} if i == frozen else {1}), i
    assert [c[0] for c in chunks] == sorted(c[0] for c in chunks)
    for bad in ((0, 4, -1.0, 0.0), (0, 4, 1.0, float("nan")), (0, 4, float("inf"), 0.0)):
        with pytest.raises(ValueError):
            hyper_tables([bad], C)
    with pytest.raises(ValueError):
        hyper_tables([(2, 5, 1.0, 0.0)], C)


def test_entry_points_are_declared_bound_and_exported_without_an_abi_bump():
    from cstp_amd import _lib
    syms = header_symbols()
    for n in NAMES:
        assert n in syms and n in _lib.SIGNATURES
        assert _declared_arity(n) == len(_lib.SIGNATURES[n][1]), n
    assert _lib.ABI_VERSION == 18
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n)


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    from cstp_amd import _lib
    lib = _lib.load()
    one, odd, n = ctypes.c_void_p(16), ctypes.c_void_p(20), 4096
    # (stream, p, g, buf, ema, n, chunks, n_chunks, hyper, n_segs, lr, momentum, coef, first, write_back, ema_momentum)
    sgd = [((None, None, one, one, None, n, one, 3, one, 2, one, 0.9, None, 0, 1, 0.0), b"null argument"),
           ((None, one, one, one, None, n, None, 3, one, 2, one, 0.9, None, 0, 1, 0.0), b"null argument"),
           ((None, one, one, one, None, n, one, 3, None, 2, one, 0.9, None, 0, 1, 0.0), b"null argument"),
           ((None, one, one, one, None, n, one, 3, one, 2, None, 0.9, None, 0, 1, 0.0), b"null argument"),
           ((None, one, one, one, None, n, one, 0, one, 2, one, 0.9, None, 0, 1, 0.0), b"bad table size"),
           ((None, one, one, one, None, n, one, 3, one, 4, one, 0.9, None, 0, 1, 0.0), b"bad table size"),
           ((None, one, one, one, None, 1 << 31, one, 3, one, 2, one, 0.9, None, 0, 1, 0.0), b"arena must hold"),
           ((None, one, one, one, ctypes.c_void_p(32), n, one, 3, one, 2, one, 0.9, None, 0, 1, 1.5), b"ema momentum"),
           ((None, one, one, one, odd, n, one, 3, one, 2, one, 0.9, None, 0, 1, 0.5), b"16-byte aligned"),
           ((None, one, one, one, one, n, one, 3, one, 2, one, 0.9, None, 0, 1, 0.5), b"must not alias")]
    for args, needle in sgd:
        rc = lib.cstp_tab_sgd_step(*args)
        assert rc != 0 and needle in lib.cstp_last_error(), (args, lib.cstp_last_error())
    # (stream, p, g, m, v, ema, n, chunks, n_chunks, hyper, n_segs, lr, b1, b2, eps, decoupled, step, ema_momentum)
    adam = [((None, one, one, None, one, None, n, one, 3, one, 2, one, 0.9, 0.99, 1e-8, 1, 1, 0.0), b"null argument"),
            ((None, one, one, one, one, None, n, one, 3, one, 2, one, 0.9, 0.99, 1e-8, 1, 0, 0.0), b"step counts from 1"),
            ((None, one, one, one, one, None, n, one, 3, one, 0, one, 0.9, 0.99, 1e-8, 1, 1, 0.0), b"bad table size"),
            ((None, one, one, one, one, None, 0, one, 3, one, 2, one, 0.9, 0.99, 1e-8, 1, 1, 0.0), b"arena must hold"),
            ((None, one, odd, one, one, None, n, one, 3, one, 2, one, 0.9, 0.99, 1e-8, 1, 1, 0.0), b"16-byte aligned"),
            ((None, one, one, one, one, one, n, one, 3, one, 2, one, 0.9, 0.99, 1e-8, 1, 1, 0.5), b"must not alias")]
    for args, needle in adam:
        rc = lib.cstp_tab_adam_step(*args)
        assert rc != 0 and needle in lib.cstp_last_error(), (args, lib.cstp_last_error())


def test_table_ops_refuse_cpu_tables():
    from cstp_amd import ops
    from cstp_amd._lib import CstpError
    p = torch.zeros(8)
    with pytest.raises(CstpError, match="HIP device"):
        ops.tab_sgd_step_(p, p, p, torch.zeros((1, 3), dtype=torch.int32), torch.zeros((1, 2)), torch.zeros(1), 0.9, None, True)


# ---- the optimizers on CPU arena tensors -----------------------------------------------------------------------------------------
def _groups(params, frozen=()):
    out = []
    for i, p in enumerate(params):
        g = {"params": p, "lr_scale": 0.5 ** (len(params) - 1 - i), "weight_decay": 0.0 if p.dim() <= 1 else 1e-4}
        if i in frozen:
            p.requires_grad = False
            g["lr"] = 0.0
        out.append(g)
    return out


def test_plan_merges_across_differing_hyper_parameters():
    from cstp_amd.optim import FlatSGD, TableAdam, TableSGD
    params, arenas = _cpu_model()                       # (5,7) | (7,) | (3,2,1,2,2) | (3,): 36 + 8 + 24 + 4 floats
    flat = FlatSGD(_groups(params), lr=0.1, momentum=0.9, weight_decay=1e-4, arenas=arenas)
    assert len(flat._plan()) == 4                       # every tensor its own run: lr and weight decay alternate
    for cls in (TableSGD, TableAdam):
        opt = cls(_groups(params), lr=0.1, weight_decay=1e-4, arenas=arenas)
        assert [(off, n) for off, n, _, _ in opt._plan()] == [(0, 72)]
        assert [g["lr"] for g in opt.param_groups] == [0.1 * 0.5 ** 3, 0.1 * 0.5 ** 2, 0.1 * 0.5, 0.1]
        assert opt.base_lr() == 0.1
    params, arenas = _cpu_model()
    opt = TableSGD(_groups(params, frozen=(1,)), lr=0.1, momentum=0.9, weight_decay=1e-4, arenas=arenas)
    assert [(off, n) for off, n, _, _ in opt._plan()] == [(0, 36), (44, 28)]      # the frozen (7,) splits the arena, nothing else does
    assert opt._live() == [0, 2, 3]
    params[1].requires_grad = True                      # thawing it is noticed
    assert [(off, n) for off, n, _, _ in opt._plan()] == [(0, 72)]


def test_base_rate_follows_the_groups_and_disagreement_is_refused():
    from cstp_amd.optim import TableSGD
    from cstp_amd.scheduler import ReduceLROnPlateau
    params, arenas = _cpu_model()
    opt = TableSGD(_groups(params, frozen=(1,)), lr=0.1, momentum=0.9, weight_decay=1e-4, arenas=arenas)
    sched = ReduceLROnPlateau(opt, "min", patience=0)
    sched.step(1.0)
    sched.step(2.0)                                     # every group times 0.1, the frozen one stays at 0.0
    assert opt.param_groups[1]["lr"] == 0.0
    assert opt.base_lr() == pytest.approx(0.01, rel=1e-12)
    opt.param_groups[0]["lr"] *= 3.0
    with pytest.raises(ValueError, match="lr_scale"):
        opt.base_lr()


def test_state_dicts_keep_the_torch_wire_format_and_carry_lr_scale():
    from cstp_amd.optim import TableAdam, TableSGD
    params, arenas = _cpu_model()
    opt = TableSGD(_groups(params), lr=0.1, momentum=0.9, weight_decay=1e-4, arenas=arenas)
    assert not opt.state_dict()["state"]
    gen = torch.Generator().manual_seed(4)
    for _, off, _, numel, _ in opt._slots:
        opt._buf[off:off + numel] = torch.randn(numel, generator=gen)
    opt._steps = 1
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [0, 1, 2, 3] and [g["lr_scale"] for g in sd["param_groups"]] == [0.125, 0.25, 0.5, 1.0]
    params2, arenas2 = _cpu_model()
    fresh = TableSGD([{"params": p} for p in params2], lr=0.5, arenas=arenas2)
    fresh.load_state_dict(sd)
    assert torch.equal(fresh._buf, opt._buf) and fresh._steps == 1
    assert [(g["lr"], g["lr_scale"], g["weight_decay"]) for g in fresh.param_groups] == \
        [(g["lr"], g["lr_scale"], g["weight_decay"]) for g in opt.param_groups]
    ref = torch.optim.SGD([{"params": [torch.nn.Parameter(p.detach().clone())]} for p in params], lr=0.3)
    ref.load_state_dict(sd)                             # the reference's optimizer takes it and steps
    for i, g in enumerate(ref.param_groups):
        assert g["lr"] == opt.param_groups[i]["lr"]
        assert torch.equal(ref.state[g["params"][0]]["momentum_buffer"], sd["state"][i]["momentum_buffer"])
        g["params"][0].grad = torch.zeros_like(g["params"][0])
    ref.step()

    adam = TableAdam(_groups(params), lr=0.1, betas=(0.9, 0.99), weight_decay=1e-4, decoupled=True, arenas=arenas)
    adam._m.normal_(generator=gen)
    adam._v.uniform_(generator=gen)
    adam._steps = 3
    sd = adam.state_dict()
    params3, arenas3 = _cpu_model()
    fresh = TableAdam([{"params": p} for p in params3], arenas=arenas3)
    fresh.load_state_dict(sd)
    assert fresh._steps == 3 and fresh.param_groups[0]["betas"] == (0.9, 0.99) and fresh.param_groups[0]["lr_scale"] == 0.125
    for i, (_, off, _, numel, _) in enumerate(adam._slots):
        assert torch.equal(fresh._m[off:off + numel], adam._m[off:off + numel])
        assert torch.equal(fresh._v[off:off + numel], adam._v[off:off + numel])
    ref = torch.optim.AdamW([{"params": [torch.nn.Parameter(p.detach().clone())]} for p in params], lr=0.3)
    ref.load_state_dict(sd)


# ---- schedule and EMA momentum -----------------------------------------------------------------------------------------------------
class _Groups:
    def __init__(self, lrs, scales=None):
        self.param_groups = [dict(lr=lr, **({} if scales is None else {"lr_scale": s})) for lr, s in zip(lrs, scales or lrs)]


@pytest.mark.parametrize("warmup", [0, 7])
def test_warmup_cosine_against_the_closed_form(warmup):
    from cstp_amd.recipe import WarmupCosine, warmup_cosine
    base, total, min_lr = 0.05, 40, 1e-4
    opt = _Groups([base, base, 0.0], [1.0, 0.25, 1.0])
    sched = WarmupCosine(opt, base, total, warmup, min_lr)
    for i in range(total):
        want = recipe_spec.warmup_cosine(i, base, total, warmup, min_lr)
        assert sched.value() == pytest.approx(want, rel=1e-12, abs=1e-18)
        assert sched.step() == pytest.approx(want, rel=1e-12, abs=1e-18)
        assert [g["lr"] for g in opt.param_groups] == [pytest.approx(want, rel=1e-12), pytest.approx(0.25 * want, rel=1e-12), 0.0]
    if warmup:
        assert warmup_cosine(0, base, total, warmup, min_lr) == pytest.approx(base / warmup)
        assert warmup_cosine(warmup - 1, base, total, warmup, min_lr) == pytest.approx(base)
    assert warmup_cosine(warmup, base, total, warmup, min_lr) == pytest.approx(base)               # the cosine starts at the peak
    # the closed form reaches min_lr at i = N: the last iteration, N - 1, is one cosine step above it and the schedule ends there
    last = warmup_cosine(total - 1, base, total, warmup, min_lr)
    step = (base - min_lr) * (1 - math.cos(math.pi / (total - warmup))) / 2
    assert last == pytest.approx(min_lr + step, rel=1e-9) and last > min_lr
    assert warmup_cosine(total, base, total, warmup, min_lr) == pytest.approx(min_lr, rel=1e-12)
    assert sched.value() == pytest.approx(min_lr, rel=1e-12) and sched.iteration == total


def test_warmup_cosine_resumes_where_the_uninterrupted_run_is():
    from cstp_amd.recipe import build_scheduler, WarmupCosine
    opts = argparse.Namespace(lr_schedule="cosine", warmup_epochs=2, min_lr=1e-5, n_epochs=6, learning_rate=0.02, lr_patience=10,
                              layer_decay=1.0, wd_skip_1d=0, model_ema=0.0, model_name="r21d_byol", task="ft_all", optimizer="sgd")
    whole = build_scheduler(opts, _Groups([0.02]), 5, 1)
    assert isinstance(whole, WarmupCosine) and (whole.total_iters, whole.warmup_iters, whole.iteration) == (30, 10, 0)
    seen = [whole.step() for _ in range(30)]
    resumed = build_scheduler(opts, _Groups([0.02]), 5, 4)                 # a run resumed at begin_epoch 4
    assert resumed.iteration == 15
    assert [resumed.step() for _ in range(15)] == seen[15:]
    with pytest.raises(ValueError):
        WarmupCosine(_Groups([0.1]), 0.1, 10, 10)


def test_ema_momentum_warm_up():
    from cstp_amd.optim import ema_momentum_at
    assert [ema_momentum_at(0.999, t) for t in (1, 2, 3)] == [2 / 11, 3 / 12, 4 / 13]
    for t in (1, 5, 80, 81, 82, 10 ** 6):
        assert ema_momentum_at(0.9, t) == recipe_spec.ema_momentum(0.9, t)
    assert ema_momentum_at(0.9, 80) == 0.9 and ema_momentum_at(0.9, 79) == 80 / 89 < 0.9      # (1 + t) / (10 + t) = 0.9 at t = 80
    assert ema_momentum_at(0.0, 1) == 0.0
    with pytest.raises(ValueError):
        ema_momentum_at(0.9, 0)
    from cstp_amd.optim import TableSGD
    params, arenas = _cpu_model()
    opt = TableSGD(params, lr=0.1, arenas=arenas)
    with pytest.raises(ValueError):
        opt.enable_ema(1.0)
    opt.enable_ema(0.9)
    assert torch.equal(opt._ema, arenas["param"]) and opt._ema.data_ptr() != arenas["param"].data_ptr()
    assert opt._ema_buffers is None                      # a hand-built arena has no BatchNorm buffers
    assert [opt._next_ema_momentum() for _ in range(2)] == [2 / 11, 3 / 12]


# ---- flags -------------------------------------------------------------------------------------------------------------------------
FT = ["--model_name", "r21d_byol", "--task", "ft_all", "--n_epochs", "5"]


def _parse(*extra):
    from cstp_amd.opts import parse_opts
    return parse_opts(FT + list(extra))


def test_flags_default_to_off():
    from cstp_amd.recipe import check_flags
    o = _parse()
    assert (o.layer_decay, o.wd_skip_1d, o.model_ema, o.lr_schedule, o.warmup_epochs, o.min_lr, o.test_ema) == \
        (1.0, 0, 0.0, "plateau", 0, 0.0, 0)
    plan = check_flags(o)
    assert not plan.table and plan.lr_schedule == "plateau"
    assert check_flags(_parse("--layer_decay", "0.75")).table and check_flags(_parse("--wd_skip_1d", "1")).table
    assert check_flags(_parse("--model_ema", "0.99")).table
    assert not check_flags(_parse("--lr_schedule", "cosine", "--warmup_epochs", "4", "--min_lr", "1e-6")).table


@pytest.mark.parametrize("flags,needle", [
    (["--layer_decay", "0"], "--layer_decay"),
    (["--layer_decay", "1.5"], "--layer_decay"),
    (["--layer_decay", "nan"], "--layer_decay"),
    (["--layer_decay", "0.75", "--model_name", "s3d_byol"], "--layer_decay"),
    (["--layer_decay", "0.75", "--model_name", "i3d_byol"], "--layer_decay"),
    (["--layer_decay", "0.75", "--task", "ft_fc"], "--layer_decay"),
    (["--layer_decay", "0.75", "--optimizer", "lars"], "--layer_decay"),
    (["--wd_skip_1d", "2"], "--wd_skip_1d"),
    (["--wd_skip_1d", "1", "--optimizer", "lars"], "--wd_skip_1d"),
    (["--model_ema", "1.0"], "--model_ema"),
    (["--model_ema", "-0.1"], "--model_ema"),
    (["--lr_schedule", "linear"], "--lr_schedule"),
    (["--lr_schedule", "cosine", "--warmup_epochs", "5"], "--warmup_epochs"),
    (["--warmup_epochs", "-1"], "--warmup_epochs"),
    (["--min_lr=-1e-3"], "--min_lr"),
    (["--min_lr", "inf"], "--min_lr"),
    (["--test_ema", "2"], "--test_ema"),
])
def test_flag_refusals_name_the_flag(flags, needle):
    from cstp_amd.recipe import check_flags
    with pytest.raises(ValueError, match=needle):
        check_flags(_parse(*flags))


def test_accepted_combinations():
    from cstp_amd.recipe import check_flags
    for flags in (["--layer_decay", "0.75", "--task", "scratch"], ["--layer_decay", "0.75", "--task", "resume", "--model_name", "r3d_byol"],
                  ["--model_ema", "0.999", "--model_name", "i3d_byol"], ["--model_ema", "0.9", "--task", "ft_fc", "--wd_skip_1d", "1"],
                  ["--model_ema", "0.9", "--optimizer", "lars"], ["--layer_decay", "1", "--model_name", "s3d_byol"],
                  ["--lr_schedule", "cosine", "--warmup_epochs", "4"]):
        check_flags(_parse(*flags))


def test_defaults_build_the_flat_optimizers_and_the_plateau_scheduler():
    from cstp_amd import recipe
    from cstp_amd.optim import FlatAdam, FlatLARS, FlatSGD, TableAdam, TableSGD
    from cstp_amd.scheduler import ReduceLROnPlateau
    for name, cls, decoupled in (("sgd", FlatSGD, None), ("adam", FlatAdam, False), ("adamw", FlatAdam, True), ("lars", FlatLARS, None)):
        params, arenas = _cpu_model()
        o = _parse("--optimizer", name, "--learning_rate", "0.1")
        opt = recipe.build_optimizer(o, None, params, arenas)
        assert type(opt) is cls and len(opt.param_groups) == 1
        if decoupled is not None:
            assert opt.decoupled is decoupled
        sched = recipe.build_scheduler(o, opt, 7, 1)
        assert type(sched) is ReduceLROnPlateau and sched.patience == o.lr_patience and sched.mode == "min"
    # with a flag on: the table classes on one group per tensor (a model is needed to name the tensors)
    m = _model("r21d_byol", 1)
    plist = list(m.parameters())
    offs, total = _layout([tuple(p.shape) for p in plist])
    arenas = {"param": torch.zeros(total), "grad": torch.zeros(total)}
    for p, o_ in zip(plist, offs):
        v = arenas["param"][o_:o_ + p.numel()].view_as(p)
        v.copy_(p.data)
        p.data = v
    for name, cls, decoupled in (("sgd", TableSGD, None), ("adam", TableAdam, False), ("adamw", TableAdam, True)):
        o = _parse("--optimizer", name, "--learning_rate", "0.1", "--layer_decay", "0.5", "--wd_skip_1d", "1", "--weight_decay", "1e-3")
        opt = recipe.build_optimizer(o, m, m.parameters(), arenas)
        assert type(opt) is cls and len(opt.param_groups) == len(plist) and len(opt._plan()) == 1
        assert opt.param_groups[-1]["lr"] == 0.1 and opt.param_groups[0]["lr"] == 0.1 * 0.5 ** 5
        assert {g["weight_decay"] for g in opt.param_groups} == {0.0, 1e-3}
        if decoupled is not None:
            assert opt.decoupled is decoupled and opt.param_groups[0]["betas"] == ((0.9, 0.99) if decoupled else (0.9, 0.999))
    lars = recipe.build_optimizer(_parse("--optimizer", "lars", "--model_ema", "0.9"), m, m.parameters(), arenas)
    assert type(lars) is FlatLARS

"""Host side of label smoothing / mixup / CutMix for fine-tuning (cstp_amd.mix, the flags, the C ABI's refusals, ops.clip_mix's
table validation, FineTuneStep's untouched default path).  No GPU needed."""
import ctypes
import math
import os
import random
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cstp_hip.h")
NEW_SYMBOLS = ("cstp_soft_cross_entropy_forward", "cstp_soft_cross_entropy_backward", "cstp_clip_mix")
FRAMES = ((7, 5), (112, 112), (1, 1))


# ---- flags ---------------------------------------------------------------------------------------------------------------
def test_flag_defaults_and_parsing():
    from cstp_amd.mix import build_mixer
    from cstp_amd.opts import parse_opts
    d = parse_opts([])
    assert (d.label_smoothing, d.mixup_alpha, d.cutmix_alpha, d.mix_prob, d.mix_switch_prob) == (0.0, 0.0, 0.0, 1.0, 0.5)
    assert build_mixer(d) is None
    assert build_mixer(parse_opts(["--mix_prob", "0.3", "--mix_switch_prob", "0.9"])) is None      # nothing to mix or smooth
    o = parse_opts(["--label_smoothing", "0.1", "--mixup_alpha", "0.8", "--cutmix_alpha", "1.0", "--mix_prob", "0.7",
                    "--mix_switch_prob", "0.25", "--manual_seed", "5"])
    m = build_mixer(o)
    assert (m.label_smoothing, m.mixup_alpha, m.cutmix_alpha, m.prob, m.switch_prob, m.seed) == (0.1, 0.8, 1.0, 0.7, 0.25, 5)
    only = build_mixer(parse_opts(["--label_smoothing", "0.2"]))
    assert only is not None and not only.mixes and only.plan(4, 8, 8, 1, 0, 0).identity


@pytest.mark.parametrize("flag,value", [("mixup_alpha", "-0.1"), ("cutmix_alpha", "-1"), ("label_smoothing", "1.0"),
                                        ("label_smoothing", "-0.01"), ("mix_prob", "1.5"), ("mix_prob", "-0.1"),
                                        ("mix_switch_prob", "2"), ("mix_switch_prob", "nan")])
def test_refusals_name_the_flag(flag, value):
    from cstp_amd.mix import build_mixer
    from cstp_amd.opts import parse_opts
    opts = parse_opts(["--mixup_alpha", "1.0", "--" + flag, value] if flag != "mixup_alpha" else ["--" + flag, value])
    with pytest.raises(ValueError, match="--" + flag):
        build_mixer(opts)


# ---- the plan ------------------------------------------------------------------------------------------------------------
def _global_rng_states():
    return torch.get_rng_state().clone(), np.random.get_state(), random.getstate()


def test_plan_is_pure_and_leaves_the_global_streams_alone():
    from cstp_amd.mix import Mixer
    m = Mixer(0.1, 1.0, 1.0, 0.8, 0.5, seed=11)
    base = dict(epoch=3, step=7, rank=1)
    first = m.plan(8, 32, 32, **base)
    assert m.plan(8, 32, 32, **base) == first and Mixer(0.1, 1.0, 1.0, 0.8, 0.5, seed=11).plan(8, 32, 32, **base) == first
    # any of seed / epoch / step / rank moves the plan: over 20 positions the (mode, lam, partner, box) sequences differ
    def seq(seed=11, epoch=3, rank=1, off=0):
        mm = Mixer(0.1, 1.0, 1.0, 0.8, 0.5, seed=seed)
        return [mm.plan(8, 32, 32, epoch, s + off, rank) for s in range(20)]
    ref = seq()
    assert seq() == ref
    assert seq(seed=12) != ref and seq(epoch=4) != ref and seq(rank=0) != ref and seq(off=1) != ref
    assert seq(off=1)[:-1] == ref[1:]                 # the plan depends on the step number alone, not on what was drawn before
    torch.manual_seed(123)
    np.random.seed(123)
    random.seed(123)
    before = _global_rng_states()
    for s in range(100):
        m.plan(8, 32, 32, 1, s, 0)
    after = _global_rng_states()
    assert torch.equal(before[0], after[0])
    assert before[1][0] == after[1][0] and np.array_equal(before[1][1], after[1][1]) and before[1][2:] == after[1][2:]
    assert before[2] == after[2]


def _plans(mixer, h, w, n=1000):
    return [mixer.plan(6, h, w, 2, s, 0) for s in range(n)]


@pytest.mark.parametrize("h,w", FRAMES)
def test_plan_geometry(h, w):
    from cstp_amd.mix import MODE_COPY, MODE_CUTMIX, MODE_MIXUP, Mixer
    plans = _plans(Mixer(0.0, 1.0, 1.0, 1.0, 0.5, seed=4), h, w)
    for p in plans:
        y0, y1, x0, x1 = p.box
        assert 0 <= y0 <= y1 <= h and 0 <= x0 <= x1 <= w
        assert 0.0 <= p.lam <= 1.0
        assert sorted(p.partner) == list(range(6))
        if p.mode == MODE_CUTMIX:
            assert p.lam == 1.0 - ((y1 - y0) * (x1 - x0)) / float(h * w) and p.lam < 1.0
        elif p.mode == MODE_MIXUP:
            assert p.box == (0, 0, 0, 0) and p.lam < 1.0
        else:
            assert p.mode == MODE_COPY and p.lam == 1.0 and p.partner == list(range(6)) and p.box == (0, 0, 0, 0)
    modes = {p.mode for p in plans}
    assert MODE_MIXUP in modes
    if (h, w) != (1, 1):          # in a 1 x 1 frame int(1 * sqrt(1 - lam)) is 0 unless lam is exactly 0: every box is empty
        assert MODE_CUTMIX in modes
    # the switch follows its probability: mixup is chosen in about half of the 1000 plans (5 sigma of the binomial)
    n_mixup = sum(p.mode == MODE_MIXUP for p in plans)
    assert abs(n_mixup - 500) < 5 * math.sqrt(1000 * 0.25)
    # one alpha at 0: only the other mode (or, for an empty CutMix box, the identity) occurs
    assert {p.mode for p in _plans(Mixer(0.0, 0.7, 0.0, 1.0, 0.5, seed=4), h, w)} == {MODE_MIXUP}
    assert {p.mode for p in _plans(Mixer(0.0, 0.0, 0.7, 1.0, 0.5, seed=4), h, w)} <= {MODE_CUTMIX, MODE_COPY}
    assert MODE_MIXUP not in {p.mode for p in _plans(Mixer(0.0, 0.0, 0.7, 1.0, 1.0, seed=4), h, w)}


@pytest.mark.parametrize("h,w", FRAMES)
@pytest.mark.parametrize("prob", [0.0, 0.3, 1.0])
def test_identity_rate_follows_prob(h, w, prob):
    """The identity occurs at the rate 1 - prob, within 5 sigma of the binomial over 1 000 plans.  Under mixup the identity has
    no other source (Beta(1, 1) gives exactly 1 with probability ~2^-53).  Under CutMix an EMPTY box is an identity too -- always
    in a 1 x 1 frame, whenever a side int(7 r) or int(5 r) is 0 in a 7 x 5 one -- so there the bound is asserted on the draw itself
    (``applied``), and on the identity only at 112 x 112, where a box is empty only for int(112 r) = 0, i.e. 1 - lam < 112^-2: 8 CutMix plans in 100 000."""
    from cstp_amd.mix import Mixer
    sigma = math.sqrt(1000 * prob * (1 - prob))
    plans = _plans(Mixer(0.0, 1.0, 0.0, prob, 0.5, seed=9), h, w)
    assert abs(sum(p.identity for p in plans) - 1000 * (1 - prob)) <= 5 * sigma
    both = _plans(Mixer(0.0, 1.0, 1.0, prob, 0.5, seed=9), h, w)
    assert abs(sum(not p.applied for p in both) - 1000 * (1 - prob)) <= 5 * sigma
    assert all(p.identity for p in both if not p.applied)
    if (h, w) == (112, 112):
        assert abs(sum(p.identity for p in both) - 1000 * (1 - prob)) <= 5 * sigma


def test_target_distribution_rows_sum_to_one():
    from cstp_amd.mix import target_distribution
    g = np.random.default_rng(0)
    for k in (2, 5, 101, 400, 1000):
        b = 9
        ta, tb = g.integers(k, size=b), g.integers(k, size=b)
        lam = g.random(b)
        lam[0], lam[1] = 1.0, 0.0
        for eps in (0.0, 0.1, 0.9):
            q = target_distribution(ta, tb, lam, eps, k)
            assert q.dtype == np.float64 and q.shape == (b, k) and (q >= 0).all()
            assert np.abs(q.sum(axis=1) - 1.0).max() < 1e-12
            r = 3
            want = (1 - eps) * (lam[r] * (np.arange(k) == ta[r]) + (1 - lam[r]) * (np.arange(k) == tb[r])) + eps / k
            assert np.abs(q[r] - want).max() < 1e-15
    # a target outside [0, k) carries no mass
    q = target_distribution([7, -1], [1, 1], [0.25, 0.25], 0.2, 5)
    assert abs(q[0].sum() - (0.8 * 0.75 + 0.2)) < 1e-12 and abs(q[1].sum() - (0.8 * 0.75 + 0.2)) < 1e-12


# ---- C ABI ---------------------------------------------------------------------------------------------------------------
def _header_arity(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
    assert m, name + " is not declared in include/cstp_hip.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_new_symbols_in_header_and_binding_table():
    from cstp_amd import _lib
    assert _lib.ABI_VERSION == 18
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == _header_arity(name), name
    assert ctypes.sizeof(_lib.ClipMixEntry) == 32
    from cstp_amd import ops
    assert ops._MIX_ENTRY.itemsize == 32 and list(ops._MIX_ENTRY.names) == [f for f, _ in _lib.ClipMixEntry._fields_]
    assert _lib.load().cstp_abi_version() == 18


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    from cstp_amd import _lib
    lib = _lib.load()
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(48)       # non-null addresses: never dereferenced before the checks fail
    f = ctypes.c_float
    calls = [
        ("cstp_soft_cross_entropy_forward", (None, None, one, one, one, f(0.1), one, 4, 5), b"null argument"),
        ("cstp_soft_cross_entropy_forward", (None, one, None, one, one, f(0.1), one, 4, 5), b"null argument"),
        ("cstp_soft_cross_entropy_forward", (None, one, one, one, one, f(0.1), None, 4, 5), b"null argument"),
        ("cstp_soft_cross_entropy_forward", (None, one, one, one, one, f(0.1), two, 0, 5), b"bad shape"),
        ("cstp_soft_cross_entropy_forward", (None, one, one, one, one, f(0.1), two, 4, -1), b"bad shape"),
        ("cstp_soft_cross_entropy_forward", (None, one, one, one, one, f(0.1), two, 70000, 70000), b"bad shape"),
        ("cstp_soft_cross_entropy_forward", (None, one, one, one, one, f(1.0), two, 4, 5), b"label smoothing outside [0, 1)"),
        ("cstp_soft_cross_entropy_forward", (None, one, one, one, one, f(-0.5), two, 4, 5), b"label smoothing outside [0, 1)"),
        ("cstp_soft_cross_entropy_backward", (None, one, one, one, one, f(0.1), None, two, 4, 5), b"null argument"),
        ("cstp_soft_cross_entropy_backward", (None, one, one, one, one, f(0.1), one, None, 4, 5), b"null argument"),
        ("cstp_soft_cross_entropy_backward", (None, one, one, one, one, f(0.1), one, two, 4, 0), b"bad shape"),
        ("cstp_soft_cross_entropy_backward", (None, one, one, one, one, f(0.1), one, two, 1 << 16, 1 << 15), b"bad shape"),
        ("cstp_soft_cross_entropy_backward", (None, one, one, one, one, f(1.0), one, two, 4, 5), b"label smoothing outside [0, 1)"),
        ("cstp_soft_cross_entropy_backward", (None, one, one, one, one, f(0.1), one, one, 4, 5), b"must not alias"),
        ("cstp_clip_mix", (None, None, two, one, 2, 3, 4, 4), b"null argument"),
        ("cstp_clip_mix", (None, one, None, one, 2, 3, 4, 4), b"null argument"),
        ("cstp_clip_mix", (None, one, two, None, 2, 3, 4, 4), b"null argument"),
        ("cstp_clip_mix", (None, one, two, one, 0, 3, 4, 4), b"bad shape"),
        ("cstp_clip_mix", (None, one, two, one, 2, 3, 4, -4), b"bad shape"),
        ("cstp_clip_mix", (None, one, two, one, 70000, 3, 4, 4), b"bad shape"),
        ("cstp_clip_mix", (None, one, two, one, 64, 48, 1024, 1024), b"bad shape"),          # 2^31 + values
        ("cstp_clip_mix", (None, one, one, one, 2, 3, 4, 4), b"must not alias"),
    ]
    for name, args, needle in calls:
        rc = getattr(lib, name)(*args)
        msg = lib.cstp_last_error()
        assert rc != 0 and needle in msg, (name, args, rc, msg)
        assert b"line" in msg                                   # the fixed "<text> (line N)" format of CSTP_REQUIRE


# ---- ops.clip_mix: the table is checked on the host, before the device check the ops raise on CPU tensors ------------------
def test_clip_mix_validates_its_table_on_the_host():
    from cstp_amd import ops
    from cstp_amd._lib import CstpError
    x = torch.zeros(3, 6, 8, 12)
    ok = dict(partner=[1, 2, 0], mode=[0, 1, 2], lam=[1.0, 0.3, 0.5], boxes=[(0, 0, 0, 0), (0, 0, 0, 0), (1, 4, 2, 9)])
    bad = [
        (dict(partner=[1, 3, 0]), "outside the batch"),
        (dict(partner=[-1, 2, 0]), "outside the batch"),
        (dict(boxes=[(0, 0, 0, 0), (0, 0, 0, 0), (1, 9, 2, 9)]), "leaves the 8 x 12 frame"),
        (dict(boxes=[(0, 0, 0, 0), (0, 0, 0, 0), (1, 4, 2, 13)]), "leaves the 8 x 12 frame"),
        (dict(boxes=[(0, 0, 0, 0), (0, 0, 0, 0), (5, 4, 2, 9)]), "leaves the 8 x 12 frame"),
        (dict(boxes=[(0, 0, 0, 0), (0, 0, 0, 0), (-1, 4, 2, 9)]), "leaves the 8 x 12 frame"),
        (dict(mode=[0, 3, 2]), "mode"),
        (dict(lam=[1.0, 1.5, 0.5]), "outside \\[0, 1\\]"),
        (dict(partner=[1, 2]), "2 entries for a batch of 3"),
        (dict(mode=[0, 1, 2, 0]), "4 entries for a batch of 3"),
        (dict(lam=[0.5]), "1 entries for a batch of 3"),
        (dict(boxes=[(0, 0, 0, 0)] * 2), "2 entries for a batch of 3"),
    ]
    for change, needle in bad:
        with pytest.raises(CstpError, match=needle):
            ops.clip_mix(x, **dict(ok, **change))
    # a valid table reaches the device check (there is no CPU path), with the message of every other op
    with pytest.raises(CstpError, match="must be on a HIP device"):
        ops.clip_mix(x, **ok)
    with pytest.raises(CstpError, match="must be on a HIP device"):
        ops.soft_cross_entropy(torch.zeros(3, 5), torch.zeros(3, dtype=torch.int64), None, None, 0.1)
    with pytest.raises(CstpError, match="eps"):
        ops.soft_cross_entropy(torch.zeros(3, 5), torch.zeros(3, dtype=torch.int64), None, None, 1.0)


# ---- FineTuneStep: without a mixer nothing new runs ---------------------------------------------------------------------------
class _StubModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(6, 5)
        self.seen = []

    def forward(self, x, o_type=None):
        self.seen.append(x)
        return self.fc(x.mean(dim=(1, 2, 3)))


def _stub_batch():
    g = torch.Generator().manual_seed(2)
    return torch.randn(4, 3, 2, 6, 6, generator=g), torch.tensor([1, 4, 0, 2])


def test_default_step_runs_the_present_path_only(monkeypatch):
    import torch.nn.functional as F
    from cstp_amd import ops
    from cstp_amd.train import FineTuneStep

    def boom(*a, **k):
        raise AssertionError("the default step must not reach the mixing ops")
    monkeypatch.setattr(ops, "soft_cross_entropy", boom)
    monkeypatch.setattr(ops, "clip_mix", boom)
    calls = []

    def ce(logits, labels):
        calls.append((logits, labels))
        return F.cross_entropy(logits, labels)
    model = _StubModel()
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    step = FineTuneStep(model, opt, "ft_all", cross_entropy=ce, mixer=None)
    assert FineTuneStep(model, opt, "ft_all", cross_entropy=ce).mixer is None          # the keyword is optional
    x, lab = _stub_batch()
    step.set_epoch(3)
    for n in range(1, 4):
        loss, out = step(x, lab)
        assert len(calls) == n and calls[-1][1] is lab and model.seen[-1] is x         # the untouched batch, one loss per step
        assert torch.isfinite(loss) and out.shape == (4, 5)
        assert step.accuracy_targets(lab) is lab and step.last_plan is None


def test_step_with_a_mixer_follows_the_plan(monkeypatch):
    """The control flow with a mixer, on CPU stand-ins for the two ops: the plan of (seed, epoch, step, rank) is drawn, the blend is
    skipped for an identity plan, tb = targets[partner], the loss gets the smoothing weight, set_epoch positions the plan."""
    from cstp_amd import ops
    from cstp_amd.mix import Mixer
    from cstp_amd.train import FineTuneStep
    log = []

    def fake_mix(x, partner, mode, lam, boxes=None):
        log.append(("mix", list(partner), mode, lam, boxes))
        return x + 0.0

    def fake_loss(logits, ta, tb=None, lam=None, eps=0.0):
        log.append(("loss", ta, tb, lam, eps))
        return logits.square().mean()
    monkeypatch.setattr(ops, "clip_mix", fake_mix)
    monkeypatch.setattr(ops, "soft_cross_entropy", fake_loss)
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self, *a, **k: self)         # no accelerator here
    mixer = Mixer(0.1, 1.0, 1.0, 0.6, 0.5, seed=21)
    model = _StubModel()
    step = FineTuneStep(model, torch.optim.SGD(model.parameters(), lr=0.1), "ft_all", mixer=mixer)
    x, lab = _stub_batch()
    seen_identity = seen_mixed = False
    for epoch in (5, 6):
        step.set_epoch(epoch)
        for s in range(8):
            del log[:]
            step(x, lab)
            plan = mixer.plan(4, 6, 6, epoch, s, 0)
            assert step.last_plan == plan
            kinds = [e[0] for e in log]
            if plan.identity:
                seen_identity = True
                assert kinds == ["loss"] and model.seen[-1] is x
                assert log[0][1] is lab and log[0][2] is None and log[0][3] is None and log[0][4] == 0.1
                assert step.accuracy_targets(lab) is lab
            else:
                seen_mixed = True
                assert kinds == ["mix", "loss"] and model.seen[-1] is not x
                assert log[0][1:] == (plan.partner, plan.mode, plan.lam, plan.box)
                _, ta, tb, lam, eps = log[1]
                assert ta is lab and torch.equal(tb, lab[torch.tensor(plan.partner)]) and eps == 0.1
                assert lam.dtype == torch.float32 and lam.shape == (4,) and bool((lam == np.float32(plan.lam)).all())
                heavier = lab if plan.lam >= 0.5 else lab[torch.tensor(plan.partner)]
                assert torch.equal(step.accuracy_targets(lab), heavier)
    assert seen_identity and seen_mixed

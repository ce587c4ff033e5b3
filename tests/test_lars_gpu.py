"""FlatLARS on a real MI355X against a restatement of its spec (include/cstp_hip.h, cstp_lars_ratio) written here in fp64 torch on
CPU tensors -- not the code under test, and the upstream project has no LARS to compare with.  Every comparison is PER TENSOR
(max-abs-diff / max-abs-ref, conftest.rel_err): an arena-wide maximum would hide the small tensors behind the large ones.

The bar is 1e-6, the one test_ops_gpu.test_flat_utils sets for the SGD kernel.  The same restatement run in fp32 on the CPU stays
within it on these inputs (asserted below, so an input that is too hard for fp32 shows up as such)."""
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-6
LR, MOM, ETA = 0.1, 0.9, 1e-3


def lars_reference(p, g, buf, c, lr, momentum, wd, eta):
    """The spec for one tensor, in the dtype of its arguments: -> (p, written-back g, buf, q)."""
    g = c * g
    q = 1.0
    if p.dim() > 1:
        d = g + wd * p
        wn, dn = float(p.double().norm()), float(d.double().norm())
        q = eta * wn / dn if wn > 0 and dn > 0 else 1.0
        d = q * d
    else:
        d = g
    buf = momentum * buf + d
    return p - lr * buf, g, buf, q


def _shapes():
    from cstp_amd import ops
    return [(1, 1), (3, 1), (5, 7), (64,), (17,), (1023, 3), (33, 5, 3, 1, 1), (64, 3, 1, 7, 7), (2 * ops.LARS_CHUNK + 5, 1), (8, 8)]


ZERO_W, ZERO_G = 9, 2        # the all-zero weight (8, 8): wn = 0; (5, 7) gets an all-zero gradient on step 2: dn = 0 at wd = 0


def _numel(s):
    return int(torch.Size(s).numel())


def _layout(shapes):
    offs, n = [], 0
    for s in shapes:
        offs.append(n)
        n += (_numel(s) + 3) // 4 * 4
    return offs, n


def _values(shapes, seed, scale_seed):
    """One fp64 tensor per shape, magnitudes spread over 1e-2 .. 1e2 from tensor to tensor."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for i, s in enumerate(shapes):
        mag = 10.0 ** (-2.0 + 4.0 * ((i * 7 + scale_seed) % len(shapes)) / (len(shapes) - 1))
        out.append((torch.rand(s, generator=gen, dtype=torch.float64) * 2 - 1) * mag)
    return out


class Arena:
    """A hand-built flat arena (the layout of R21DBYOL.flatten_parameters: 16-byte starts, zero padding) on the GPU."""

    def __init__(self, shapes, values, frozen=()):
        self.shapes, (self.offs, self.total) = shapes, _layout(shapes)
        self.arenas = {"param": torch.zeros(self.total, device="cuda"), "grad": torch.zeros(self.total, device="cuda")}
        self.params = []
        for i, (s, o, v) in enumerate(zip(shapes, self.offs, values)):
            p = torch.nn.Parameter(torch.empty(0, device="cuda"), requires_grad=i not in frozen)
            self.arenas["param"][o:o + _numel(s)] = v.float().flatten().cuda()
            p.data = self.arenas["param"][o:o + _numel(s)].view(s)
            if i not in frozen:
                p.grad = self.arenas["grad"][o:o + _numel(s)].view(s)
            self.params.append(p)

    def set_grads(self, grads):
        self.arenas["grad"].zero_()
        for s, o, g in zip(self.shapes, self.offs, grads):
            self.arenas["grad"][o:o + _numel(s)] = g.float().flatten().cuda()

    def tensor(self, arena, i):
        o = self.offs[i]
        return arena[o:o + _numel(self.shapes[i])].view(self.shapes[i])

    def pad_mask(self):
        m = torch.ones(self.total, dtype=torch.bool)
        for s, o in zip(self.shapes, self.offs):
            m[o:o + _numel(s)] = False
        return m


# three steps: no pending clip on the first, a coefficient below 1 on the others; step 2 runs with weight_decay = 0 and an
# all-zero gradient for (5, 7)
STEPS = [(None, 5e-4), (0.37, 0.0), (0.81, 5e-4)]


def _grads(shapes, step):
    gs = _values(shapes, 100 + step, 3 + step)
    if step == 1:
        gs[ZERO_G] = torch.zeros(shapes[ZERO_G], dtype=torch.float64)
    return gs


def _run_three_steps(frozen=(), groups=False):
    """-> per step: the (p, g, buf) arenas, trust_ratios() and the optimizer, after that step."""
    from cstp_amd.optim import FlatLARS
    shapes = _shapes()
    w = _values(shapes, 1, 0)
    w[ZERO_W] = torch.zeros(shapes[ZERO_W], dtype=torch.float64)
    a = Arena(shapes, w, frozen)
    plist = [{"params": p} if p.requires_grad else {"params": p, "lr": 0.0} for p in a.params] if groups else a.params
    opt = FlatLARS(plist, lr=LR, momentum=MOM, weight_decay=STEPS[0][1], eta=ETA, arenas=a.arenas)
    snaps = []
    for step, (c, wd) in enumerate(STEPS):
        for g in opt.param_groups:
            g["weight_decay"] = wd
        a.set_grads(_grads(shapes, step))
        if c is not None:
            opt._coef.fill_(c)
            opt._clip_pending = True
        opt.step()
        q, idx = opt.trust_ratios()
        assert idx.tolist() == list(range(len(shapes)))
        snaps.append((a.arenas["param"].clone(), a.arenas["grad"].clone(), opt._buf.clone(), q.clone()))
    return a, opt, snaps


@pytest.fixture(scope="module")
def three_steps():
    a, opt, snaps = _run_three_steps()
    torch.cuda.synchronize()
    return a, snaps


@pytest.fixture(scope="module")
def reference_steps():
    """The restatement over the same three steps: per step and tensor (p, g, buf, q) in fp64, and in fp32 (c and the hyper-parameters
    as Python floats, tensors fp32) to show what fp32 arithmetic alone costs."""
    shapes = _shapes()
    out = {}
    for dt in (torch.float64, torch.float32):
        w = _values(shapes, 1, 0)
        w[ZERO_W] = torch.zeros(shapes[ZERO_W], dtype=torch.float64)
        p = [v.float().to(dt) for v in w]                       # the fp32 values the device holds
        buf = [torch.zeros_like(v) for v in p]
        steps = []
        for step, (c, wd) in enumerate(STEPS):
            gs = [g.float().to(dt) for g in _grads(shapes, step)]
            cf = 1.0 if c is None else float(torch.tensor(c, dtype=torch.float32))       # the coefficient is an fp32 device scalar
            res = [lars_reference(p[i], gs[i], buf[i], cf, LR, MOM, wd, ETA) for i in range(len(shapes))]
            p, buf = [r[0] for r in res], [r[2] for r in res]
            steps.append(res)
        out[dt] = steps
    return out


def test_fp32_restatement_is_inside_the_bar(reference_steps):
    for s64, s32 in zip(reference_steps[torch.float64], reference_steps[torch.float32]):
        for (p, g, b, q), (p32, g32, b32, q32) in zip(s64, s32):
            for x, y in ((p32, p), (g32, g), (b32, b)):
                if float(y.abs().max()) > 0:
                    assert rel_err(x, y) < TOL
            assert abs(q32 - q) <= TOL * abs(q)


def test_op_level_parity_per_tensor(three_steps, reference_steps):
    a, snaps = three_steps
    shapes = a.shapes
    worst = {"p": 0.0, "g": 0.0, "buf": 0.0, "q": 0.0}
    for step, ((pa, ga, ba, q), ref) in enumerate(zip(snaps, reference_steps[torch.float64])):
        assert bool(torch.isfinite(pa).all()) and bool(torch.isfinite(ba).all()) and bool(torch.isfinite(q).all())
        qh = q.cpu().double()
        for i, (p, g, b, qr) in enumerate(ref):
            for name, arena, want in (("p", pa, p), ("g", ga, g), ("buf", ba, b)):
                got = a.tensor(arena, i)
                if float(want.abs().max()) == 0.0:
                    assert float(got.abs().max()) == 0.0, (step, shapes[i], name)
                    continue
                e = rel_err(got, want)
                worst[name] = max(worst[name], e)
                assert e < TOL, (step, shapes[i], name, e)
            e = abs(float(qh[i]) - qr) / abs(qr)
            worst["q"] = max(worst["q"], e)
            assert e < TOL, (step, shapes[i], "q", float(qh[i]), qr)
            if len(shapes[i]) == 1:
                assert float(qh[i]) == 1.0
    print("worst per-tensor errors over three steps:", worst)
    # the two degenerate branches were taken: q = 1 exactly, and nothing turned into NaN
    assert float(snaps[0][3][ZERO_W]) == 1.0 and float(snaps[1][3][ZERO_G]) == 1.0
    assert float(snaps[0][3][5]) != 1.0


def test_padding_stays_bit_zero(three_steps):
    a, snaps = three_steps
    m = a.pad_mask()
    assert int(m.sum()) > 0
    for arenas in snaps:
        for arena in arenas[:3]:
            pad = arena.cpu()[m]
            assert bool((pad.view(torch.int32) == 0).all())


def test_two_runs_give_the_same_bits(three_steps):
    _, snaps = three_steps
    _, _, again = _run_three_steps()
    for s1, s2 in zip(snaps, again):
        for x, y in zip(s1, s2):
            assert torch.equal(x, y)


def test_frozen_tensors_are_left_alone(reference_steps):
    """The per-tensor group list of get_fine_tuning_parameters with three frozen tensors: several runs, each with its own tables."""
    frozen = (1, 4, 7)
    a, opt, snaps = _run_three_steps(frozen=frozen, groups=True)
    assert len(opt._plan()) == 4 and len(opt._run_tables()) == 4
    shapes = a.shapes
    w = _values(shapes, 1, 0)
    pa, ga, ba, q = snaps[-1]
    ref = reference_steps[torch.float64][-1]
    for i in range(len(shapes)):
        if i in frozen:
            assert torch.equal(a.tensor(pa, i).cpu(), w[i].float())
            assert float(a.tensor(ba, i).abs().max()) == 0.0
            assert bool(torch.isnan(q[i]))
            continue
        p, g, b, qr = ref[i]
        for arena, want in ((pa, p), (ba, b)):
            if float(want.abs().max()) == 0.0:
                assert float(a.tensor(arena, i).abs().max()) == 0.0
            else:
                assert rel_err(a.tensor(arena, i), want) < TOL, (shapes[i],)
        assert abs(float(q[i]) - qr) <= TOL * abs(qr)
    sd = opt.state_dict()["state"]
    assert sorted(sd) == [i for i in range(len(shapes)) if i not in frozen]


# ---- on a real model: the depth-1 R(2+1)D-BYOL pre-training model at the smallest clip of test_model_gpu.py -------------------
def _model_and_batch():
    from cstp_amd.r21d_byol import R21DBYOL
    from oracle import r21d_byol_oracle as orc
    ls = orc.layer_sizes_for_depth(1)
    model = R21DBYOL(pretrain=True, layer_sizes=ls)
    model.load_state_dict(orc.closed_form_state(ls, torch.float32))
    model.cuda()
    model.flatten_parameters()
    model.train()
    x1, x2, labels = orc.closed_form_clips(3, 6, 36, torch.float32, seed_phase=5)
    lab = {k: v.cuda() for k, v in labels.items()}
    return model, (x1.cuda(), x2.cuda(), lab["spa"], lab["tem"], lab["pb"], lab["rot1"], lab["rot2"])


W = (0.1, 1.0, 1.0, 1.0, 1.0)
MODEL_WD = 5e-4


def _lars_for(model):
    from cstp_amd.optim import FlatLARS
    return FlatLARS(model.parameters(), lr=0.05, momentum=0.9, weight_decay=MODEL_WD, eta=ETA, arenas=model.flatten_parameters())


@pytest.fixture(scope="module")
def model_run():
    """Two PretrainSteps with FlatLARS and clipping on.  Per step: the parameters before it, the raw gradient arena and the clip
    coefficient the optimizer met, and what it left (parameters, .grad, ratios); plus the checkpoint after step 1."""
    from cstp_amd.train import PretrainStep
    model, batch = _model_and_batch()
    opt = _lars_for(model)
    step = PretrainStep(model, opt, W, clip_grad_norm=True)
    arenas = model.flatten_parameters()
    named = list(model.named_parameters())
    met = {}
    inner = opt.step

    def spy():
        met["grad"], met["coef"] = arenas["grad"].clone(), opt._coef.clone()
        inner()
    opt.step = spy
    records, checkpoint = [], None
    for s in range(2):
        before = {k: p.detach().double().cpu() for k, p in named}
        out = step(*batch)
        records.append(dict(before=before, raw_grad=met["grad"], coef=met["coef"], grad_norm=float(out.grad_norm),
                            after={k: p.detach().clone() for k, p in named},
                            grad={k: p.grad.detach().double().cpu() for k, p in named if p.requires_grad},
                            q=opt.trust_ratios()[0].cpu(), param=arenas["param"].clone(), buf=opt._buf.clone()))
        if s == 0:
            checkpoint = ({k: v.clone() for k, v in model.state_dict().items()}, opt.state_dict())
    torch.cuda.synchronize()
    return named, records, checkpoint


def test_two_pretrain_steps_on_a_real_model(model_run):
    named, records, _ = model_run
    bufs = {k: torch.zeros(p.shape, dtype=torch.float64) for k, p in named if p.requires_grad}
    plain = adapted = 0
    for s, r in enumerate(records):
        assert 0.0 < r["grad_norm"] < float("inf") and float(r["coef"]) <= 1.0
        q, worst = r["q"], 0.0
        for i, (k, p) in enumerate(named):
            if not p.requires_grad:                             # the EMA target network: listed, never stepped
                assert bool(torch.isnan(q[i])), k
                continue
            # .grad is clipped and written back: c is already in it
            want, _, bufs[k], qr = lars_reference(r["before"][k], r["grad"][k], bufs[k], 1.0, 0.05, 0.9, MODEL_WD, ETA)
            e = rel_err(r["after"][k], want)
            worst = max(worst, e)
            assert e < TOL, (s, k, e)
            assert abs(float(q[i]) - qr) <= TOL * abs(qr), (s, k, float(q[i]), qr)
            if p.dim() <= 1:                                    # BatchNorm gamma / beta, the heads' biases: the plain path
                assert float(q[i]) == 1.0, k
                plain += 1
            else:
                adapted += float(q[i]) != 1.0
        print("step %d: worst per-tensor parameter error %.3g" % (s + 1, worst))
    assert plain > 20 and adapted > 20
    assert any(k.endswith("bias") and p.dim() == 1 and p.requires_grad for k, p in named)


def test_resume_from_a_checkpoint_repeats_step_two_bit_for_bit(model_run):
    """state_dict() after step 1 into a fresh FlatLARS on a cloned model: its step 2 equals the uninterrupted one bit for bit.
    The optimizer is what resumes here, so it is given the gradient the uninterrupted step 2 met: a second forward / backward is not
    bit-reproducible (test_model_gpu.test_pack_plan_steps_match_steps_that_pack_inside_every_call says why), the clip norm and the
    three LARS launches are."""
    _, records, (model_sd, opt_sd) = model_run
    model2, _ = _model_and_batch()
    model2.load_state_dict(model_sd)
    arenas2 = model2.flatten_parameters()
    assert torch.equal(arenas2["param"], records[0]["param"])
    opt2 = _lars_for(model2)
    opt2.load_state_dict(opt_sd)
    assert torch.equal(opt2._buf, records[0]["buf"])
    arenas2["grad"].copy_(records[1]["raw_grad"])
    opt2.clip_grad_norm_(18)
    assert torch.equal(opt2._coef, records[1]["coef"])
    opt2.step()
    assert torch.equal(arenas2["param"], records[1]["param"])
    assert torch.equal(opt2._buf, records[1]["buf"])
    assert torch.equal(opt2.trust_ratios()[0].cpu().nan_to_num(-1.0), records[1]["q"].nan_to_num(-1.0))

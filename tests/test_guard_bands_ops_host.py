"""The case shapes and helpers of tests/test_guard_bands_ops_gpu.py on the CPU, before any GPU run: plain torch implementations
written into the same Guarded views through the same ``impl(views)`` signature keep the contract under both fills -- a
table-driven arena step (frozen tensor and padding included), a concat tail that accumulates into a shared gradient arena, the
SAME max-pool forward and backward, an NT-Xent pair that stages in the workspace, the ring push -- and five sloppy variants are
each REJECTED, each for the reason it is sloppy:
  (a) an arena step that works in whole 8-float units, so a chunk's end is rounded up: untouched_check names the frozen tensor;
  (b) a row mean that reads s rounded up to 4: wrong on every row but the last; on the last row of the last branch it passes
      between zeros and fails between NaNs;
  (c) a pool backward that uses the argmax -1 as an index: "wrote 1 element before the start of dx";
  (d) a push that wraps modulo cap instead of refusing: rows outside the window change;
  (e) a table step that follows the entry with off + len = n + 4: the guard is reported, with the offset.
Then untouched_check itself, and the share of ReLU kinks masked in every concat-tail case of the GPU file."""
import pytest
import torch
import torch.nn.functional as F

import guard_bands as gb
import guard_bands_cases as gc

CPU = torch.device("cpu")
F32, F64, I32 = torch.float32, torch.float64, torch.int32
LR, MOM, COEF, EMA_M = gc.f32(0.05), gc.f32(0.9), gc.f32(0.37), gc.f32(0.99)
OWN, PAD, FROZEN = gc.arena_masks()


def _past(t, off, length):
    """``length`` elements of the memory t lives in, from element ``off`` of t on -- past its end or before its start if asked."""
    return t.as_strided((length,), (1,), t.storage_offset() + off)


# ---- a table-driven arena step ----------------------------------------------------------------------------------------------------
def _tab_spec(extra=()):
    n = gc.ARENA_N
    chunks, _ = gc.arena_tables()
    if extra:
        chunks = torch.cat([chunks, torch.tensor(list(extra), dtype=I32)], 0)
    hyper = torch.tensor(gc.HYPER, dtype=F32)
    p0, g0, b0, e0 = gc.arena_values(1), gc.arena_values(2, 0.05), gc.arena_values(3, 0.1), gc.arena_values(4)
    p, g, b, e = (t.double().clone() for t in (p0, g0, b0, e0))
    for off, numel, padded, seg, _ in gc.TENSORS:
        if seg is None:
            continue
        sl = slice(off, off + numel)
        lr, wd = float(torch.tensor(LR, dtype=F32) * hyper[seg, 0]), float(hyper[seg, 1])
        g[sl] = COEF * g0.double()[sl]
        b[sl] = MOM * b0.double()[sl] + g[sl] + wd * p0.double()[sl]
        p[sl] = p0.double()[sl] - lr * b[sl]
        e[sl] = EMA_M * e0.double()[sl] + (1.0 - EMA_M) * p[sl]

    def arena(ref, prior):
        def check(got):
            for a, z in gc.listed_slices():
                gb.rel_check(ref[a:z], 1e-6)(got[a:z])
        return gb.all_checks(gb.untouched_check(prior, ~OWN), check)
    return gb.Spec("host table step", {"chunks": chunks, "hyper": hyper, "lr": torch.tensor([LR]), "coef": torch.tensor([COEF])},
                   {k: ((n,), F32) for k in ("p", "g", "buf", "ema")},
                   {"p": arena(p, p0), "g": arena(g, g0), "buf": arena(b, b0), "ema": arena(e, e0)},
                   priors={"p": p0, "g": g0, "buf": b0, "ema": e0})


def _tab_step(v, whole_units=False, follow=False):
    """cstp_tab_sgd_step in torch: one chunk after the other, a malformed entry skipped (lars_chunk's check)."""
    n = v["p"].numel()
    lr0, coef = v["lr"][0], v["coef"][0]
    for seg, off, ln in v["chunks"].tolist():
        ok = 0 <= seg < gc.N_SEGS and off >= 0 and 0 < ln <= gc.CHUNK and ((off | ln) & 3) == 0
        if not (ok and (follow or off + ln <= n)):
            continue
        if whole_units:                  # (a): the chunk's end rounded up to a whole 8-float unit
            ln = (off + ln + 7) // 8 * 8 - off
        p, g, b, e = (_past(v[k], off, ln) for k in ("p", "g", "buf", "ema"))
        lr, wd = lr0 * v["hyper"][seg, 0], v["hyper"][seg, 1]
        g.mul_(coef)
        b.mul_(MOM).add_(g + wd * p)
        p.sub_(lr * b)
        e.mul_(EMA_M).add_((1.0 - EMA_M) * p)


def test_a_correct_table_step_keeps_the_contract_with_and_without_malformed_entries():
    assert gb.three_runs(_tab_spec(), _tab_step, CPU) == [] and gb.live_run(_tab_spec(), _tab_step, CPU) == []
    spec = _tab_spec(tuple(gc.malformed_chunks()))
    clean = gb.one_run(_tab_spec(), gb.Operands(_tab_spec(), CPU), _tab_step, "nan")[0]
    for name in spec.checks:
        spec.checks[name] = gb.all_checks(spec.checks[name], gb.bits_check(clean[name]))
    assert gb.three_runs(spec, _tab_step, CPU) == []


def test_a_step_in_whole_8_float_units_is_rejected_by_untouched_check_naming_the_frozen_tensor():
    found = gb.three_runs(_tab_spec(), lambda v: _tab_step(v, whole_units=True), CPU)
    assert found and bool(FROZEN[12]) and not bool(FROZEN[11])
    for name in ("p", "buf", "ema"):          # (g: 0.37 * g changes the frozen gradient as well)
        assert any(" %s against the reference: changed 4 elements that the call must leave untouched (first: element 12 of %d" % (
            name, gc.ARENA_N) in f for f in found), found


def test_a_step_that_follows_the_entry_past_the_arena_is_rejected_as_a_broken_guard_with_its_offset():
    spec = _tab_spec(tuple(gc.malformed_chunks()))
    sloppy = lambda v: _tab_step(v, follow=True)      # noqa: E731
    # between poisoned guards the update of the four floats past the arena is NaN -> NaN: the guard bytes do not change, and only
    # the second update of the last tensor's floats inside the arena shows, as a numeric error
    found = gb.three_runs(spec, sloppy, CPU)
    assert len(found) >= 3 and not any("wrote" in f for f in found) and all("relative error" in f for f in found), found
    # between live guards the store itself shows, with its offset
    found = gb.live_run(spec, sloppy, CPU)
    assert len(found) == 4, found
    for name in ("p", "g", "buf", "ema"):
        assert any("wrote 1 element past the end of %s (first changed guard byte: element +1 from its last; farthest: +4)" % name in f
                   for f in found), found
    assert gb.live_run(_tab_spec(tuple(gc.malformed_chunks())), _tab_step, CPU) == []
    # ... and every entry of malformed_chunks, followed, stays inside the guard bands: the rule of the GPU cases
    G = gb.guard_bytes(gc.ARENA_N * 4) // 4
    assert all(-G <= off and off + ln <= gc.ARENA_N + G and seg <= gc.N_SEGS for seg, off, ln in gc.malformed_chunks())


# ---- a concat tail: self-gating into the concat tensor, dw | db accumulated into one gradient arena ----------------------------------
GATE_CS, GATE_SPATIAL, GATE_N = (5, 3), (3, 5, 3), 2                # s = 45: 48 when rounded up to 4


def _gate_layout(cs):
    slices, pos = [], 5
    for c in cs:
        slices.append((pos, pos + c * c + 3))
        pos += c * c + 3 + c + 7
    own = torch.zeros(pos, dtype=torch.bool)
    for (a, b), c in zip(slices, cs):
        own[a:a + c * c] = True
        own[b:b + c] = True
    return slices, pos, own


def _gate_forward(xs, ws, bs, mean):
    gates = [torch.sigmoid(F.linear(mean(x), w, b)) for x, w, b in zip(xs, ws, bs)]
    return torch.cat([g[:, :, None, None, None] * x for g, x in zip(gates, xs)], 1)


def _plain_mean(x):
    return x.mean(dim=[2, 3, 4])


def _gate_spec(cs=GATE_CS, n=GATE_N):
    xs = [gc.rand((n, c) + GATE_SPATIAL, 20 + i).float() for i, c in enumerate(cs)]
    ws = [(gc.rand((c, c), 30 + i) / c ** 0.5).float() for i, c in enumerate(cs)]
    bs = [gc.rand((c,), 40 + i).float() for i, c in enumerate(cs)]
    dy = gc.rand((n, sum(cs)) + GATE_SPATIAL, 50).float()
    xr, wr, br = ([t.double().requires_grad_(True) for t in ts] for ts in (xs, ws, bs))
    y = _gate_forward(xr, wr, br, _plain_mean)
    grads = torch.autograd.grad(y, wr + br, dy.double())
    slices, total, own = _gate_layout(cs)
    prior = (gc.rand((total,), 60) * 0.5).float()
    ref = prior.double().clone()
    for (a, b), c, dw, db in zip(slices, cs, grads[:len(cs)], grads[len(cs):]):
        ref[a:a + c * c] += dw.flatten()
        ref[b:b + c] += db
    inputs = {"dy": dy}
    for i in range(len(cs)):
        inputs.update({"x%d" % i: xs[i], "w%d" % i: ws[i], "b%d" % i: bs[i]})

    def grads_check(got):
        gb.rel_check(ref[own], 1e-5)(got[own])
    return gb.Spec("host gate tail", inputs, {"y": (tuple(y.shape), F32), "grads": ((total,), F32)},
                   {"y": gb.rel_check(y.detach(), 1e-6), "grads": gb.all_checks(gb.untouched_check(prior, ~own), grads_check)},
                   priors={"grads": prior}), slices


def _gate_impl(cs, slices, mean=_plain_mean):
    def impl(v):
        xs = [v["x%d" % i] for i in range(len(cs))]
        ws = [v["w%d" % i].clone().requires_grad_(True) for i in range(len(cs))]
        bs = [v["b%d" % i].clone().requires_grad_(True) for i in range(len(cs))]
        y = _gate_forward(xs, ws, bs, mean)
        v["y"].copy_(y.detach())
        grads = torch.autograd.grad(y, ws + bs, v["dy"])
        for (a, b), c, dw, db in zip(slices, cs, grads[:len(cs)], grads[len(cs):]):
            v["grads"][a:a + c * c] += dw.flatten()            # accumulate != 0: added to what the arena holds
            v["grads"][b:b + c] += db
    return impl


def _mean_of_s_rounded_up(x):
    """(b): every row read as ceil4(s) values -- the next row's first ones; behind the last row, whatever follows x."""
    n, c = x.shape[:2]
    s = x[0, 0].numel()
    s4 = (s + 3) // 4 * 4
    return x.as_strided((n, c, s4), (c * s, s, 1)).sum(2) / s


def test_a_correct_concat_tail_keeps_the_contract():
    spec, slices = _gate_spec()
    assert gb.three_runs(spec, _gate_impl(GATE_CS, slices), CPU) == [] and gb.live_run(spec, _gate_impl(GATE_CS, slices), CPU) == []


def test_a_row_mean_over_s_rounded_up_is_wrong_on_every_row_but_the_last_and_there_only_between_nans():
    spec, slices = _gate_spec()
    found = gb.three_runs(spec, _gate_impl(GATE_CS, slices, _mean_of_s_rounded_up), CPU)
    assert len(found) >= 3 and all(" y " in f or "grads" in f for f in found), found         # wrong under every fill
    assert any("[zero]" in f and "relative error" in f for f in found) and any("[nan]" in f and "non-finite" in f for f in found)
    # one sample of one single-channel branch: its only row is the last row of the last branch
    spec, slices = _gate_spec(cs=(1,), n=1)
    ops = gb.Operands(spec, CPU)
    impl = _gate_impl((1,), slices, _mean_of_s_rounded_up)
    assert gb.one_run(spec, ops, impl, "zero")[1] == []
    found = gb.one_run(spec, ops, impl, "nan")[1]
    assert found and all("[nan]" in f and "non-finite output" in f for f in found), found


# ---- the SAME max-pool ------------------------------------------------------------------------------------------------------------
POOL = (3, (2, 4, 4), (3, 3, 3), (1, 1, 1))


def _pool_specs(negative):
    rows, vol, k, s = POOL
    r = gc.same_pool_case(rows, vol, k, s, negative)
    oshape = tuple(r["y"].shape)
    fwd = gb.Spec("host SAME pool forward", {"x": r["x"]}, {"y": (oshape, F32), "argmax": (oshape, I32)},
                  {"y": gb.bits_check(r["y"].float()), "argmax": gb.bits_check(r["argmax"])}, finite_as={"argmax": None})
    bwd = gb.Spec("host SAME pool backward", {"dy": r["dy"], "argmax": r["argmax"]}, {"dx": ((rows,) + vol, F32)},
                  {"dx": gb.rel_check(r["dx"], 1e-6)})
    return fwd, bwd


def _pool_fwd(v):
    y, arg = gc.same_pool_aten(v["x"], POOL[2], POOL[3])
    v["y"].copy_(y)
    v["argmax"].copy_(arg)


def _pool_bwd(v, index_with_minus_one=False):
    rows = v["dx"].shape[0]
    vol = v["dx"][0].numel()
    v["dx"].zero_()
    arg, dy = v["argmax"].reshape(rows, -1).long(), v["dy"].reshape(rows, -1)
    for r in range(rows):
        won = arg[r] >= 0
        if index_with_minus_one:          # (c): -1 taken for an index: the dropped gradients are summed one element before the row
            tile = torch.zeros(vol + 1).index_add_(0, arg[r] + 1, dy[r])
            v["dx"][r].view(-1).copy_(tile[1:])
            if bool((~won).any()):
                _past(v["dx"], r * vol - 1, 1)[0] = tile[0]
        else:
            v["dx"][r].view(-1).index_add_(0, arg[r][won], dy[r][won])


@pytest.mark.parametrize("negative", [0, -1], ids=["first volume negative", "last volume negative"])
def test_a_correct_same_pool_keeps_the_contract(negative):
    fwd, bwd = _pool_specs(negative)
    assert gb.three_runs(fwd, _pool_fwd, CPU) == []
    assert gb.three_runs(bwd, _pool_bwd, CPU) == []


def test_a_pool_backward_that_indexes_with_minus_one_is_rejected_as_a_store_before_dx():
    _, bwd = _pool_specs(0)               # the padding zeros win in the FIRST volume: one before it is the guard
    found = gb.three_runs(bwd, lambda v: _pool_bwd(v, index_with_minus_one=True), CPU)
    assert len(found) == 3 and all("wrote 1 element before the start of dx" in f for f in found), found
    _, bwd = _pool_specs(-1)              # in the last volume: the dropped gradient lands in the volume before it
    found = gb.three_runs(bwd, lambda v: _pool_bwd(v, index_with_minus_one=True), CPU)
    assert len(found) == 3 and all("dx against the reference" in f for f in found), found


# ---- an NT-Xent pair that stages in the workspace -----------------------------------------------------------------------------------
NTX_R, NTX_F, NTX_T, NTX_DLOSS = 6, 5, 0.5, 1.7


def _ntx_sim(reps):
    nrm = reps.norm(dim=1, keepdim=True)
    return (reps @ reps.t()) / torch.clamp(nrm * nrm.t(), min=1e-8) / NTX_T


def _ntx_spec():
    reps = gc.rand((NTX_R, NTX_F), 70).float()
    r = reps.double().requires_grad_(True)
    logits = _ntx_sim(r).masked_fill(torch.eye(NTX_R, dtype=torch.bool), float("-inf"))
    idx = torch.arange(NTX_R)
    loss = (torch.logsumexp(logits, dim=1) - _ntx_sim(r)[idx, (idx + NTX_R // 2) % NTX_R]).mean()
    (loss * NTX_DLOSS).backward()
    return gb.Spec("host ntxent pair", {"reps": reps, "dloss": torch.tensor([NTX_DLOSS])},
                   {"loss": ((1,), F32), "dreps": ((NTX_R, NTX_F), F32)},
                   {"loss": gb.rel_check(loss.detach().reshape(1), 1e-4), "dreps": gb.rel_check(r.grad, 1e-4)},
                   ws_bytes=(NTX_R * NTX_R + NTX_R) * 4)


def _ntx_pair(v, forward_writes=True):
    """forward: the similarity matrix and the row log-sum-exps go to the workspace; backward: reads them back from there."""
    R = NTX_R
    ws = v["ws"].view(F32)
    sim, lse = ws[:R * R].view(R, R), ws[R * R:R * R + R]
    idx = torch.arange(R)
    if forward_writes:
        sim.copy_(_ntx_sim(v["reps"]))
        lse.copy_(torch.logsumexp(sim.masked_fill(torch.eye(R, dtype=torch.bool), float("-inf")), dim=1))
    else:                                  # a forward that ADDS into scratch nobody cleared
        sim.add_(_ntx_sim(v["reps"]))
        lse.add_(torch.logsumexp(sim.masked_fill(torch.eye(R, dtype=torch.bool), float("-inf")), dim=1))
    v["loss"][0] = (lse - sim[idx, (idx + R // 2) % R]).mean()
    # ---- backward: dL/dsim from the staged values, then through the similarity
    G = torch.exp(sim - lse[:, None]).masked_fill(torch.eye(R, dtype=torch.bool), 0.0)
    G[idx, (idx + R // 2) % R] -= 1.0
    reps = v["reps"].clone().requires_grad_(True)
    _ntx_sim(reps).backward(G * v["dloss"][0] / R)
    v["dreps"].copy_(reps.grad)


def test_a_correct_ntxent_pair_keeps_the_contract_and_one_that_sums_into_uncleared_scratch_does_not():
    assert gb.three_runs(_ntx_spec(), _ntx_pair, CPU) == []
    found = gb.three_runs(_ntx_spec(), lambda v: _ntx_pair(v, forward_writes=False), CPU)
    assert found and all("non-finite output" in f for f in found), found


# ---- the ring push -----------------------------------------------------------------------------------------------------------------
PUSH_R, PUSH_F, PUSH_CAP = 3, 7, 8


def _push_spec(ptr):
    reps = gc.rand((PUSH_R, PUSH_F), 80).float() * 3
    reps[1] = 0
    before = gc.rand((PUSH_CAP, PUSH_F), 81).float()
    keep = torch.ones(PUSH_CAP, PUSH_F, dtype=torch.bool)
    keep[ptr:ptr + PUSH_R] = False                                        # (rows of the window that exist)
    want = reps.double() / reps.double().norm(dim=1, keepdim=True).clamp_min(1e-8)

    def rows_check(got):
        hi = min(ptr + PUSH_R, PUSH_CAP)
        gb.rel_check(want[:hi - ptr], 1e-6)(got[ptr:hi])
    return gb.Spec("host push ptr%d" % ptr, {"reps": reps}, {"queue": ((PUSH_CAP, PUSH_F), F32)},
                   {"queue": gb.all_checks(gb.untouched_check(before, keep), rows_check)}, priors={"queue": before}), before


def _push(v, ptr, wrap=False):
    rows = v["reps"] / v["reps"].norm(dim=1, keepdim=True).clamp_min(1e-8)
    if ptr < 0 or ptr + PUSH_R > PUSH_CAP:
        if not wrap:
            raise ValueError("rows [ptr, ptr + R) must lie inside the queue")
        for i in range(PUSH_R):          # (d): modulo cap instead of a refusal
            v["queue"][(ptr + i) % PUSH_CAP] = rows[i]
        return
    v["queue"][ptr:ptr + PUSH_R] = rows


@pytest.mark.parametrize("ptr", [0, 5])
def test_a_correct_push_keeps_the_contract(ptr):
    spec, _ = _push_spec(ptr)
    assert gb.three_runs(spec, lambda v: _push(v, ptr), CPU) == [] and gb.live_run(spec, lambda v: _push(v, ptr), CPU) == []


def test_a_refused_push_touches_nothing_and_one_that_wraps_is_rejected():
    spec, before = _push_spec(6)
    operands = gb.Operands(spec, CPU)
    operands.arm("nan")
    with pytest.raises(ValueError):
        _push(operands.views(), 6)
    assert operands.problems() == [] and torch.equal(operands.outs["queue"].view, before)
    found = gb.three_runs(spec, lambda v: _push(v, 6, wrap=True), CPU)
    assert len(found) == 3 and all("changed 7 elements that the call must leave untouched (first: element 0 of 56" in f
                                   for f in found), found


# ---- untouched_check itself ----------------------------------------------------------------------------------------------------------
def test_untouched_check_reports_the_count_and_the_first_changed_element():
    prior = torch.arange(12, dtype=F32).view(3, 4)
    mask = torch.zeros(3, 4, dtype=torch.bool)
    mask[1:] = True
    check = gb.untouched_check(prior, mask)
    got = prior.clone()
    got[0] = -1.0                                        # outside the mask: the call's own elements
    check(got)
    got[2, 1], got[1, 3] = 0.5, 7.5
    with pytest.raises(AssertionError) as e:
        check(got)
    assert "changed 2 elements that the call must leave untouched (first: element 7 of 12; was 7.0, is 7.5)" in str(e.value)
    # bit equality, not value equality: -0.0 for +0.0 is a change (the padding must stay +0), NaN for the same NaN is none
    zeros = torch.zeros(4)
    with pytest.raises(AssertionError) as e:
        gb.untouched_check(zeros, torch.ones(4, dtype=torch.bool))(torch.tensor([0.0, -0.0, 0.0, 0.0]))
    assert "changed 1 element " in str(e.value) and "(first: element 1 of 4" in str(e.value)
    nan = torch.full((3,), float("nan"))
    gb.untouched_check(nan, torch.ones(3, dtype=torch.bool))(nan.clone())
    with pytest.raises(AssertionError):
        gb.untouched_check(prior, mask)(prior.to(torch.float64))         # another dtype is not "untouched"


def test_bits_check_under_a_mask_and_all_checks_in_order():
    ref = torch.tensor([1.0, 2.0, 3.0])
    gb.bits_check(ref, torch.tensor([True, False, True]))(torch.tensor([1.0, 9.0, 3.0]))
    with pytest.raises(AssertionError) as e:
        gb.bits_check(ref)(torch.tensor([1.0, 9.0, 3.0]))
    assert "1 element differ in their bits (first: element 1; expected 2.0, got 9.0)" in str(e.value)
    seen = []
    gb.all_checks(lambda g: seen.append(1), lambda g: seen.append(2))(ref)
    assert seen == [1, 2]


# ---- the case tables of the GPU file -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gc.BNC_CASES))
def test_relu_kinks_masked_in_a_concat_tail_case_stay_under_one_percent(name):
    r = gc.bnc_case(*gc.BNC_CASES[name])
    assert r["kink_share"] <= gc.KINK_CAP, r["kink_share"]
    assert float(r["dy"].abs().max()) > 0 and all(bool(torch.isfinite(t).all()) for t in r["dx"])


def test_the_arena_layout_is_the_one_the_cases_claim():
    chunks, segs = gc.arena_tables()
    assert chunks.tolist() == [[0, 0, 4], [1, 4, 8], [2, 20, 4096], [3, 4116, 4096], [3, 8212, 4], [4, 8216, 12]]
    assert segs.tolist() == [[0, 1, 0], [1, 1, 1], [2, 1, 1], [3, 2, 1], [5, 1, 0]]
    assert gc.ARENA_N == 8228 and int(FROZEN.sum()) == 8 and int(PAD.sum()) == 6 and chunks[-1, 1] + chunks[-1, 2] == gc.ARENA_N
    for seed in (1, 2, 3, 4):
        v = gc.arena_values(seed)
        assert bool((v[PAD].view(I32) == 0).all()) and bool((v[FROZEN] != 0).all())

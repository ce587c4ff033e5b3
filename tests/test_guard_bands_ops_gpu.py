"""The rest of the training step between poisoned guard bands (tests/guard_bands.py; DESIGN.md, "What an in-place call may
touch"): the flat-arena optimisers and their table-driven forms, the concat tails, the pools, the heads, the regularisers, the
bf16 cast and the mix kernel.  Every case makes raw C-ABI calls three times -- operands between zero guards, again, then between
NaN guards, outputs and workspace 0xFF inside and out -- with ``control_must_hold``: none of these kernels uses float atomics.
References are PyTorch CPU fp64 (ATen's exact result for masks and argmax); every bar is the one the op's parity test already
uses and is named beside the case.  In-place operands are outputs with a prior; what a call must leave alone (padding, a frozen
tensor, the live values between the slices of a gradient arena, the rows of a ring outside the window) is held to bit equality
with the prior by ``untouched_check``.  Malformed table entries are chosen so that even a kernel that FOLLOWED them would stay
inside the test's own allocations (tests/guard_bands_cases.py)."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guard_bands as gb
import guard_bands_cases as gc
import ntxq_spec
import ops_edge_cases as ec
import reg_spec

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, B16, I32, I64, F64, U8 = torch.float32, torch.bfloat16, torch.int32, torch.int64, torch.float64, torch.uint8
f32, _rand = gc.f32, gc.rand


def _libs():
    from cstp_amd import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(v, name):
    t = v.get(name)
    return None if t is None else t.data_ptr()


def _run3(spec, impl):
    """zero, zero, nan; and for a call with in-place operands the run between live guards (guard_bands.live_run)."""
    found = gb.three_runs(spec, impl, DEV, torch.cuda.synchronize)
    if spec.priors:
        found += gb.live_run(spec, impl, DEV, torch.cuda.synchronize)
    assert found == [], "\n".join(found)


def _i3(v):
    return (ctypes.c_int32 * 3)(*v)


def _bits(t):
    return t.contiguous().view(U8).flatten()


def _assert_refused(spec, call, needle):
    """A documented refusal: an error return whose message holds ``needle``, and NOTHING touched -- every guard intact, every input
    unchanged, outputs with a prior still that prior, the other outputs and the workspace still 0xFF."""
    _l, lib = _libs()
    operands = gb.Operands(spec, DEV)
    for fill in ("zero", "nan"):
        operands.arm(fill)
        rc = call(operands.views())
        torch.cuda.synchronize()
        assert rc != 0 and needle in lib.cstp_last_error(), (rc, lib.cstp_last_error())
        assert operands.problems() == []
        for n, g in operands.outs.items():
            if n in spec.priors:
                assert torch.equal(_bits(g.view.cpu()), _bits(spec.priors[n].to(g.dtype))), "a refused call wrote " + n
            else:
                assert bool((g.buf == 0xFF).all()), "a refused call wrote " + n
        assert bool((operands.ws.buf == 0xFF).all()), "a refused call wrote the workspace"


# ============================================================================================================================
# Flat arenas: cstp_ema_update, cstp_sumsq, cstp_clip_coef, cstp_sgd_step, cstp_adam_step (misc.hip)
# ============================================================================================================================
FLAT_N = [1, 3, 4, 5, 1027]                 # a tail of 1..3 after the float4 body; below one float4
LR, MOM, WD, COEF = f32(0.05), f32(0.9), f32(5e-4), f32(0.37)


@pytest.mark.parametrize("n", FLAT_N + [ec.EMA_STRIDE_N])
def test_ema_update(n):
    """target is read and written: an output with a prior.  Bar 1e-6: test_ops_edges_gpu.py test_ema_update_edges."""
    _l, lib = _libs()
    t, o, _ = ec.flat_inputs(n)
    spec = gb.Spec("ema_update n%d" % n, {"o": o}, {"t": ((n,), F32)}, {"t": gb.rel_check(ec.ema_ref(t, o, 0.996), 1e-6)},
                   priors={"t": t})
    _run3(spec, lambda v: _l.check(lib.cstp_ema_update(_stream(), v["t"].data_ptr(), v["o"].data_ptr(), n, 0.996), "cstp_ema_update"))


@pytest.mark.parametrize("norm_out", [True, False], ids=["norm", "no norm"])
@pytest.mark.parametrize("n", FLAT_N + [ec.SUMSQ_STRIDE_N])
def test_sumsq_and_clip_coef(n, norm_out):
    """The workspace is exactly the documented minimum (8 KiB).  Bars 1e-6: test_grad_sumsq_edges."""
    _l, lib = _libs()
    _, _, g = ec.flat_inputs(n)
    ref = float(g.double().norm())

    def norm_check(square):
        def check(got):
            v = float(got[0]) ** (0.5 if square else 1.0)
            assert abs(v - ref) / ref < 1e-6, (v, ref)
        return check

    def coef_check(got):
        assert abs(float(got[0]) - min(1.0, 0.01 / (ref + 1e-6))) < 1e-6, float(got[0])
    outputs = {"ss": ((1,), F32), "coef": ((1,), F32)}
    checks = {"ss": norm_check(True), "coef": coef_check}
    if norm_out:
        outputs["nrm"] = ((1,), F32)
        checks["nrm"] = norm_check(False)
    spec = gb.Spec("sumsq + clip_coef n%d" % n, {"g": g}, outputs, checks, ws_bytes=8192)

    def impl(v):
        _l.check(lib.cstp_sumsq(_stream(), v["g"].data_ptr(), n, v["ss"].data_ptr(), v["ws"].data_ptr(), 8192), "cstp_sumsq")
        _l.check(lib.cstp_clip_coef(_stream(), v["ss"].data_ptr(), 0.01, v["coef"].data_ptr(), _ptr(v, "nrm")), "cstp_clip_coef")
    _run3(spec, impl)


@pytest.mark.parametrize("first,wb,use_coef", [(1, 1, 1), (0, 1, 1), (0, 0, 1), (1, 0, 0), (0, 1, 0)])
@pytest.mark.parametrize("n", FLAT_N + [ec.STEP_STRIDE_N])
def test_sgd_step(n, first, wb, use_coef):
    """p, g and buf are priors; with first_step the kernel must not READ buf (it starts poisoned), without write_back_grad g keeps
    its bits.  Bar 1e-6: test_sgd_step_edges."""
    _l, lib = _libs()
    t, o, g = ec.flat_inputs(n)
    bp = (o * 0.1).float()
    c = COEF if use_coef else 1.0
    gcl = g.double() * c
    d = gcl + WD * t.double()
    b = d if first else MOM * bp.double() + d
    inputs = {"lr": torch.tensor([LR], dtype=F32)}
    if use_coef:
        inputs["coef"] = torch.tensor([COEF], dtype=F32)
    priors = {"p": t, "g": g}
    if not first:
        priors["buf"] = bp
    checks = {"p": gb.rel_check(t.double() - LR * b, 1e-6), "buf": gb.rel_check(b, 1e-6),
              "g": gb.rel_check(gcl, 1e-6) if wb else gb.bits_check(g)}
    spec = gb.Spec("sgd_step n%d first%d wb%d coef%d" % (n, first, wb, use_coef), inputs,
                   {k: ((n,), F32) for k in ("p", "g", "buf")}, checks, priors=priors)
    _run3(spec, lambda v: _l.check(lib.cstp_sgd_step(_stream(), v["p"].data_ptr(), v["g"].data_ptr(), v["buf"].data_ptr(), n,
                                                     v["lr"].data_ptr(), MOM, WD, _ptr(v, "coef"), first, wb), "cstp_sgd_step"))


B1, B2, AEPS, AWD, ALR = f32(0.9), f32(0.99), f32(1e-8), f32(5e-2), f32(0.01)


def _adam_ref(p, g, m, v, lr, wd, decoupled, step):
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    if decoupled:
        p = p * (1.0 - lr * wd)
    else:
        g = g + wd * p
    m = B1 * m + (1.0 - B1) * g
    v = B2 * v + (1.0 - B2) * g * g
    p = p - lr / (1.0 - B1 ** step) * m / (v.sqrt() / (1.0 - B2 ** step) ** 0.5 + AEPS)
    return p, m, v


@pytest.mark.parametrize("decoupled", [0, 1])
@pytest.mark.parametrize("n", FLAT_N + [ec.STEP_STRIDE_N])
def test_adam_step(n, decoupled):
    """Step 2 from finite moments.  Bar 1e-5: test_adam_step_edges."""
    _l, lib = _libs()
    t, o, g = ec.flat_inputs(n)
    m0, v0 = (o * 0.01).float(), (g * g * 3 + 1e-4).float()
    p, m, v = _adam_ref(t, g, m0, v0, ALR, AWD, decoupled, 2)
    spec = gb.Spec("adam_step n%d decoupled%d" % (n, decoupled), {"g": g, "lr": torch.tensor([ALR], dtype=F32)},
                   {k: ((n,), F32) for k in ("p", "m", "v")},
                   {"p": gb.rel_check(p, 1e-5), "m": gb.rel_check(m, 1e-5), "v": gb.rel_check(v, 1e-5)},
                   priors={"p": t, "m": m0, "v": v0})
    _run3(spec, lambda w: _l.check(lib.cstp_adam_step(_stream(), w["p"].data_ptr(), w["g"].data_ptr(), w["m"].data_ptr(),
                                                      w["v"].data_ptr(), n, w["lr"].data_ptr(), B1, B2, AEPS, AWD, decoupled, 2),
                                   "cstp_adam_step"))


# ============================================================================================================================
# Table-driven steps on one arena (lars.h, optim_table.h): tests/guard_bands_cases.py lays it out
# ============================================================================================================================
ETA, EMA_M = f32(1e-3), f32(0.99)
OWN, PAD, FROZEN = gc.arena_masks()


def _arena_check(ref64, prior, tol):
    """Per listed tensor max |got - ref| / max |ref| < tol (test_lars_gpu.py compares per tensor: an arena-wide maximum would hide
    the small tensors), after bit equality with the prior on everything else: the padding stays +0, the frozen tensor its bits
    (first: a trampled neighbour is the more specific finding)."""
    def check(got):
        for a, b in gc.listed_slices():
            r = ref64[a:b]
            err = float((got[a:b].double() - r).abs().max() / r.abs().max().clamp_min(1e-30))
            assert err < tol, "tensor [%d, %d): relative error %.3e (bar %.1e)" % (a, b, err, tol)
    return gb.all_checks(gb.untouched_check(prior, ~OWN), check)


def _tables(extra):
    chunks, segs = gc.arena_tables()
    if extra:
        chunks = torch.cat([chunks, torch.tensor(list(extra), dtype=I32)], 0)
    return chunks, segs


def _lars_case(wb, use_coef, extra=()):
    """cstp_lars_ratio + cstp_lars_step: adapted and plain segments mixed.  Bar 1e-6 per tensor and on q: test_lars_gpu.py."""
    _l, lib = _libs()
    assert lib.cstp_lars_chunk() == gc.CHUNK
    n = gc.ARENA_N
    chunks, segs = _tables(extra)
    p0, g0, b0 = gc.arena_values(1), gc.arena_values(2, 0.05), gc.arena_values(3, 0.1)
    c = COEF if use_coef else 1.0
    p, g, b = p0.double().clone(), g0.double().clone(), b0.double().clone()
    q = torch.ones(gc.N_SEGS, dtype=F64)
    for off, numel, padded, seg, adapted in gc.TENSORS:
        if seg is None:
            continue
        sl = slice(off, off + numel)
        gcl = c * g0.double()[sl]
        d = gcl
        if adapted:
            d = gcl + WD * p0.double()[sl]
            wn, dn = float(p0.double()[sl].norm()), float(d.norm())
            q[seg] = ETA * wn / dn if wn > 0 and dn > 0 else 1.0
            d = q[seg] * d
        b[sl] = MOM * b0.double()[sl] + d
        p[sl] = p0.double()[sl] - LR * b[sl]
        if wb:
            g[sl] = gcl

    def q_check(got):
        err = float(((got.double() - q).abs() / q.abs()).max())
        assert err < 1e-6, "trust ratios: %.3e" % err
        assert all(float(got[s]) == 1.0 for s in (0, 4)), "a segment that is not adapted has q != 1"
    inputs = {"chunks": chunks, "segs": segs, "lr": torch.tensor([LR], dtype=F32)}
    if use_coef:
        inputs["coef"] = torch.tensor([COEF], dtype=F32)
    nc = chunks.shape[0]
    spec = gb.Spec("lars wb%d coef%d extra%d" % (wb, use_coef, len(extra)), inputs,
                   {"p": ((n,), F32), "g": ((n,), F32), "buf": ((n,), F32), "ratio": ((gc.N_SEGS,), F32)},
                   {"p": _arena_check(p, p0, 1e-6), "buf": _arena_check(b, b0, 1e-6),
                    "g": _arena_check(g, g0, 1e-6) if wb else gb.bits_check(g0), "ratio": q_check},
                   ws_bytes=lib.cstp_lars_workspace_bytes(nc), priors={"p": p0, "g": g0, "buf": b0})

    def impl(v):
        _l.check(lib.cstp_lars_ratio(_stream(), v["p"].data_ptr(), v["g"].data_ptr(), n, v["chunks"].data_ptr(), nc,
                                     v["segs"].data_ptr(), gc.N_SEGS, WD, ETA, _ptr(v, "coef"), v["ratio"].data_ptr(),
                                     v["ws"].data_ptr(), spec.ws_bytes), "cstp_lars_ratio")
        _l.check(lib.cstp_lars_step(_stream(), v["p"].data_ptr(), v["g"].data_ptr(), v["buf"].data_ptr(), n, v["chunks"].data_ptr(),
                                    nc, v["segs"].data_ptr(), gc.N_SEGS, v["ratio"].data_ptr(), v["lr"].data_ptr(), MOM, WD,
                                    _ptr(v, "coef"), wb), "cstp_lars_step")
    return spec, impl


def _hyper(uniform):
    return torch.tensor([(1.0, 5e-4)] * gc.N_SEGS if uniform else gc.HYPER, dtype=F32)


def _listed():
    """(slice, segment) of every listed tensor."""
    for off, numel, padded, seg, _ in gc.TENSORS:
        if seg is not None:
            yield slice(off, off + numel), seg


def _tab_sgd_case(ema, wb, first, use_coef=True, uniform=False, extra=()):
    """cstp_tab_sgd_step.  Bars 1e-6: cstp_sgd_step's and cstp_ema_update's (test_ops_edges_gpu.py); test_recipe_gpu.py holds the
    table steps to the same."""
    _l, lib = _libs()
    n = gc.ARENA_N
    chunks, _ = _tables(extra)
    hyper = _hyper(uniform)
    p0, g0, b0, e0 = gc.arena_values(1), gc.arena_values(2, 0.05), gc.arena_values(3, 0.1), gc.arena_values(4)
    c = COEF if use_coef else 1.0
    p, g, b, e = (t.double().clone() for t in (p0, g0, b0, e0))
    eom = f32(1.0 - EMA_M)
    for sl, seg in _listed():
        lr = float(torch.tensor(LR, dtype=F32) * hyper[seg, 0])
        wd = float(hyper[seg, 1])
        gcl = c * g0.double()[sl]
        d = gcl + wd * p0.double()[sl]
        b[sl] = d if first else MOM * b0.double()[sl] + d
        p[sl] = p0.double()[sl] - lr * b[sl]
        e[sl] = EMA_M * e0.double()[sl] + eom * p[sl]
        if wb:
            g[sl] = gcl
    inputs = {"chunks": chunks, "hyper": hyper, "lr": torch.tensor([LR], dtype=F32)}
    if use_coef:
        inputs["coef"] = torch.tensor([COEF], dtype=F32)
    outputs = {"p": ((n,), F32), "g": ((n,), F32), "buf": ((n,), F32)}
    checks = {"p": _arena_check(p, p0, 1e-6), "buf": _arena_check(b, b0, 1e-6),
              "g": _arena_check(g, g0, 1e-6) if wb else gb.bits_check(g0)}
    priors = {"p": p0, "g": g0, "buf": b0}
    if ema:
        outputs["ema"], checks["ema"], priors["ema"] = ((n,), F32), _arena_check(e, e0, 1e-6), e0
    nc = chunks.shape[0]
    spec = gb.Spec("tab_sgd ema%d wb%d first%d uniform%d extra%d" % (ema, wb, first, uniform, len(extra)), inputs, outputs, checks,
                   priors=priors)

    def impl(v):
        _l.check(lib.cstp_tab_sgd_step(_stream(), v["p"].data_ptr(), v["g"].data_ptr(), v["buf"].data_ptr(), _ptr(v, "ema"), n,
                                       v["chunks"].data_ptr(), nc, v["hyper"].data_ptr(), gc.N_SEGS, v["lr"].data_ptr(), MOM,
                                       _ptr(v, "coef"), first, wb, EMA_M), "cstp_tab_sgd_step")
    return spec, impl


def _tab_adam_case(ema, decoupled, uniform=False, extra=()):
    """cstp_tab_adam_step.  Bar 1e-5: cstp_adam_step's (test_adam_step_edges); the EMA arena 1e-6 as above."""
    _l, lib = _libs()
    n = gc.ARENA_N
    chunks, _ = _tables(extra)
    hyper = _hyper(uniform)
    p0, g0, e0 = gc.arena_values(1), gc.arena_values(2, 0.05), gc.arena_values(4)
    m0, v0 = gc.arena_values(5, 0.01), gc.arena_values(6, 0.01, nonneg=True)
    p, m, w, e = (t.double().clone() for t in (p0, m0, v0, e0))
    eom = f32(1.0 - EMA_M)
    for sl, seg in _listed():
        lr = float(torch.tensor(ALR, dtype=F32) * hyper[seg, 0])
        p[sl], m[sl], w[sl] = _adam_ref(p0[sl], g0[sl], m0[sl], v0[sl], lr, float(hyper[seg, 1]), decoupled, 2)
        e[sl] = EMA_M * e0.double()[sl] + eom * p[sl]
    outputs = {k: ((n,), F32) for k in ("p", "m", "v")}
    checks = {"p": _arena_check(p, p0, 1e-5), "m": _arena_check(m, m0, 1e-5), "v": _arena_check(w, v0, 1e-5)}
    priors = {"p": p0, "m": m0, "v": v0}
    if ema:
        outputs["ema"], checks["ema"], priors["ema"] = ((n,), F32), _arena_check(e, e0, 1e-6), e0
    nc = chunks.shape[0]
    spec = gb.Spec("tab_adam ema%d decoupled%d uniform%d extra%d" % (ema, decoupled, uniform, len(extra)),
                   {"g": g0, "chunks": chunks, "hyper": hyper, "lr": torch.tensor([ALR], dtype=F32)}, outputs, checks, priors=priors)

    def impl(v):
        _l.check(lib.cstp_tab_adam_step(_stream(), v["p"].data_ptr(), v["g"].data_ptr(), v["m"].data_ptr(), v["v"].data_ptr(),
                                        _ptr(v, "ema"), n, v["chunks"].data_ptr(), nc, v["hyper"].data_ptr(), gc.N_SEGS,
                                        v["lr"].data_ptr(), B1, B2, AEPS, decoupled, 2, EMA_M), "cstp_tab_adam_step")
    return spec, impl


@pytest.mark.parametrize("wb,use_coef", [(1, 1), (0, 1), (1, 0)])
def test_lars_on_the_arena(wb, use_coef):
    _run3(*_lars_case(wb, use_coef))


@pytest.mark.parametrize("ema,wb,first", [(0, 1, 0), (1, 1, 0), (1, 0, 0), (1, 1, 1), (0, 0, 1)])
def test_tab_sgd_on_the_arena(ema, wb, first):
    _run3(*_tab_sgd_case(ema, wb, first))


@pytest.mark.parametrize("ema,decoupled", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_tab_adam_on_the_arena(ema, decoupled):
    _run3(*_tab_adam_case(ema, decoupled))


def test_tab_sgd_with_uniform_hyper_parameters_has_the_flat_step_bits():
    """include/cstp_hip.h: "with every scale 1 and one wd the results are theirs bit for bit" (test_recipe_gpu.py asserts it
    through the optimisers); here on the listed floats and the padding, with the frozen tensor untouched."""
    _l, lib = _libs()
    n = gc.ARENA_N
    p, g, b = (gc.arena_values(s, k).to(DEV) for s, k in ((1, 1.0), (2, 0.05), (3, 0.1)))
    lr, coef = torch.tensor([LR], device=DEV), torch.tensor([COEF], device=DEV)
    _l.check(lib.cstp_sgd_step(_stream(), p.data_ptr(), g.data_ptr(), b.data_ptr(), n, lr.data_ptr(), MOM, f32(5e-4), coef.data_ptr(),
                               0, 1), "cstp_sgd_step")          # the flat step over whole arenas: the reference
    torch.cuda.synchronize()
    p, g, b = p.cpu(), g.cpu(), b.cpu()
    spec, impl = _tab_sgd_case(0, 1, 0, uniform=True)
    for name, flat in (("p", p), ("g", g), ("buf", b)):
        spec.checks[name] = gb.all_checks(spec.checks[name], gb.bits_check(flat, ~FROZEN))
    _run3(spec, impl)


def test_tab_adam_with_uniform_hyper_parameters_has_the_flat_step_bits():
    _l, lib = _libs()
    n = gc.ARENA_N
    p, g, m, v = (gc.arena_values(s, k, nn).to(DEV) for s, k, nn in ((1, 1.0, False), (2, 0.05, False), (5, 0.01, False),
                                                                      (6, 0.01, True)))
    lr = torch.tensor([ALR], device=DEV)
    _l.check(lib.cstp_adam_step(_stream(), p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr.data_ptr(), B1, B2, AEPS,
                                f32(5e-4), 0, 2), "cstp_adam_step")
    torch.cuda.synchronize()
    p, m, v = p.cpu(), m.cpu(), v.cpu()
    spec, impl = _tab_adam_case(0, 0, uniform=True)
    for name, flat in (("p", p), ("m", m), ("v", v)):
        spec.checks[name] = gb.all_checks(spec.checks[name], gb.bits_check(flat, ~FROZEN))
    _run3(spec, impl)


@pytest.mark.parametrize("kind", ["lars", "tab_sgd", "tab_adam"])
def test_malformed_table_entries_are_skipped_not_followed(kind):
    """Five extra entries -- seg = n_segs, off = -4, off + len = n + 4, len = CSTP_LARS_CHUNK + 4, off = 2 -- behind the good ones:
    every arena (and the trust ratios) comes out bit-equal to a run without them, and every guard is intact."""
    build = {"lars": lambda extra: _lars_case(1, 1, extra), "tab_sgd": lambda extra: _tab_sgd_case(1, 1, 0, extra=extra),
             "tab_adam": lambda extra: _tab_adam_case(1, 1, extra=extra)}[kind]
    spec, impl = build(())
    clean, found = gb.one_run(spec, gb.Operands(spec, DEV), impl, "nan", torch.cuda.synchronize)
    assert found == [], "\n".join(found)
    spec, impl = build(tuple(gc.malformed_chunks()))
    for name in spec.checks:
        spec.checks[name] = gb.all_checks(spec.checks[name], gb.bits_check(clean[name]))
    _run3(spec, impl)


def test_refused_lars_step_on_a_misaligned_arena_touches_nothing():
    _l, lib = _libs()
    spec, _ = _lars_case(1, 1)
    spec.shifts = {"p": 4}
    spec.priors["ratio"] = torch.ones(gc.N_SEGS)
    chunks, _ = gc.arena_tables()
    _assert_refused(spec, lambda v: lib.cstp_lars_step(_stream(), v["p"].data_ptr(), v["g"].data_ptr(), v["buf"].data_ptr(), gc.ARENA_N,
                                                       v["chunks"].data_ptr(), chunks.shape[0], v["segs"].data_ptr(), gc.N_SEGS,
                                                       v["ratio"].data_ptr(), v["lr"].data_ptr(), MOM, WD, v["coef"].data_ptr(), 1),
                    b"16-byte aligned")


def test_refused_tab_sgd_step_with_ema_aliasing_p_touches_nothing():
    _l, lib = _libs()
    spec, _ = _tab_sgd_case(0, 1, 0)
    chunks, _ = gc.arena_tables()
    _assert_refused(spec, lambda v: lib.cstp_tab_sgd_step(_stream(), v["p"].data_ptr(), v["g"].data_ptr(), v["buf"].data_ptr(),
                                                          v["p"].data_ptr(), gc.ARENA_N, v["chunks"].data_ptr(), chunks.shape[0],
                                                          v["hyper"].data_ptr(), gc.N_SEGS, v["lr"].data_ptr(), MOM,
                                                          v["coef"].data_ptr(), 0, 1, EMA_M), b"must not alias")


# ============================================================================================================================
# Concat tails: cstp_gate_concat_* (gate.hip)
# ============================================================================================================================
@functools.lru_cache(maxsize=None)
def _gate_ref(cs, spatial, n, seed):
    """test_s3dg_gpu.py's _gate_case / _gate_ref on fp32 values, with the fp64 means, gates and gradients."""
    g = torch.Generator().manual_seed(seed)
    r = lambda shape: torch.rand(shape, generator=g, dtype=F64)       # noqa: E731
    xs = []
    for c in cs:
        x = r((n, c) + spatial) * 2
        x[x < 0.5] = 0.0                                               # ReLU outputs
        xs.append(x.float())
    ws = [((r((c, c)) * 2 - 1) / c ** 0.5).float() for c in cs]
    bs = [(r((c,)) * 2 - 1).float() for c in cs]
    dy = (r((n, sum(cs)) + spatial) * 2 - 1).float()
    xr, wr, br = ([t.double().requires_grad_(True) for t in ts] for ts in (xs, ws, bs))
    ms = [x.mean(dim=[2, 3, 4]) for x in xr]
    gs = [torch.sigmoid(F.linear(m, w, b)) for m, w, b in zip(ms, wr, br)]
    y = torch.cat([gt[:, :, None, None, None] * x for gt, x in zip(gs, xr)], 1)
    grads = torch.autograd.grad(y, xr + wr + br, dy.double())
    nb = len(cs)
    return {"xs": xs, "ws": ws, "bs": bs, "dy": dy, "y": y.detach(), "m": torch.cat(ms, 1).detach(), "g": torch.cat(gs, 1).detach(),
            "dx": grads[:nb], "dw": grads[nb:2 * nb], "db": grads[2 * nb:]}


GATES = {
    # name: (cs, spatial, n)
    "ragged": ((24, 7, 130), (3, 5, 3), 3),        # s = 45: the scalar bodies; rows = 483: the last block is one wave short
    "float4": ((16, 8), (2, 2, 2), 3),             # s = 8: the float4 bodies
    "single": ((16,), (1, 1, 1), 3),               # one branch, one position
    "strided": ((230, 230), (1, 2, 2), 9),         # rows = 4140 > 4 * GATE_APPLY_MAX_BLOCKS at s = 4: the apply loop strides
}


def _gate_branches(_l, v, cs, bwd_slices=None):
    arr = (_l.GateBranch * len(cs))()
    for i, c in enumerate(cs):
        arr[i].x, arr[i].w, arr[i].b, arr[i].c = v["x%d" % i].data_ptr(), v["w%d" % i].data_ptr(), v["b%d" % i].data_ptr(), c
        if bwd_slices is not None:
            arr[i].dx = v["dx%d" % i].data_ptr()
            arr[i].dw = v["grads"].data_ptr() + 4 * bwd_slices[i][0]
            arr[i].db = v["grads"].data_ptr() + 4 * bwd_slices[i][1]
    return arr


def _gate_fwd_case(name, want_g=True, want_cell=True, shifts=None):
    """y at 1e-6 (test_gate_concat_matches_fp64); the means and gates it is the product of at the same bar."""
    _l, lib = _libs()
    cs, spatial, n = GATES[name]
    r = _gate_ref(cs, spatial, n, 11 + sum(cs))
    C, s = sum(cs), int(np.prod(spatial))
    inputs = {}
    for i in range(len(cs)):
        inputs.update({"x%d" % i: r["xs"][i], "w%d" % i: r["ws"][i], "b%d" % i: r["bs"][i]})
    outputs = {"y": ((n, C) + spatial, F32), "m": ((n, C), F32)}
    checks = {"y": gb.rel_check(r["y"], 1e-6), "m": gb.rel_check(r["m"], 1e-6)}
    finite_as = {}
    if want_g:
        outputs["g"], checks["g"] = ((n, C), F32), gb.rel_check(r["g"], 1e-6)
    if want_cell:          # zeroed by the first launch: it starts poisoned
        outputs["cell"], finite_as["cell"] = ((1,), I32), F32
    spec = gb.Spec("gate forward %s g%d cell%d %s" % (name, want_g, want_cell, shifts or ""), inputs, outputs, checks, shifts=shifts,
                   finite_as=finite_as)
    cells = []

    def impl(v):
        _l.check(lib.cstp_gate_concat_forward(_stream(), _gate_branches(_l, v, cs), len(cs), n, s, v["y"].data_ptr(), v["m"].data_ptr(),
                                              _ptr(v, "g"), _ptr(v, "cell")), "cstp_gate_concat_forward")
        if want_cell:      # max |y| of THIS y, to the bit
            torch.cuda.synchronize()
            cells.append((int(v["cell"].item()), int(v["y"].abs().max().view(I32).item())))
    return spec, impl, cells


def _gate_layout(cs):
    """dw_i | db_i as slices of one gradient arena with live values between them -> ([(dw offset, db offset)], elements, own mask)."""
    slices, pos = [], 5
    for c in cs:
        slices.append((pos, pos + c * c + 3))
        pos += c * c + 3 + c + 7
    own = torch.zeros(pos, dtype=torch.bool)
    for (a, b), c in zip(slices, cs):
        own[a:a + c * c] = True
        own[b:b + c] = True
    return slices, pos, own


def _gate_bwd_case(name, accumulate, shifts=None, ws_short=0):
    """dx, dw, db at 1e-5 (test_gate_concat_matches_fp64).  m and g are the fp64 reference's, rounded to fp32; the workspace is
    exactly cstp_gate_workspace_bytes; with accumulate the slices start from live values, without it from NaN (unwritten shows)."""
    _l, lib = _libs()
    cs, spatial, n = GATES[name]
    r = _gate_ref(cs, spatial, n, 11 + sum(cs))
    C, s = sum(cs), int(np.prod(spatial))
    slices, total, own = _gate_layout(cs)
    prior = (_rand((total,), 77) * 0.5).float()
    ref = prior.double().clone()
    if not accumulate:
        prior[own] = float("nan")
        ref[own] = 0.0
    for (a, b), c, dw, db in zip(slices, cs, r["dw"], r["db"]):
        ref[a:a + c * c] += dw.flatten()
        ref[b:b + c] += db

    def grads_check(got):
        for (a, b), c in zip(slices, cs):
            for lo, hi in ((a, a + c * c), (b, b + c)):
                gb.rel_check(ref[lo:hi], 1e-5)(got[lo:hi])
    inputs = {"dy": r["dy"], "m": r["m"].float(), "g": r["g"].float()}
    outputs = {"grads": ((total,), F32)}
    checks = {"grads": gb.all_checks(gb.untouched_check(prior, ~own), grads_check)}
    for i in range(len(cs)):
        inputs.update({"x%d" % i: r["xs"][i], "w%d" % i: r["ws"][i], "b%d" % i: r["bs"][i]})
        outputs["dx%d" % i] = (tuple(r["xs"][i].shape), F32)
        checks["dx%d" % i] = gb.rel_check(r["dx"][i], 1e-5)
    nbytes = lib.cstp_gate_workspace_bytes(n, C)
    spec = gb.Spec("gate backward %s accumulate%d %s" % (name, accumulate, shifts or ""), inputs, outputs, checks, ws_bytes=nbytes,
                   priors={"grads": prior}, shifts=shifts)

    def call(v):
        return lib.cstp_gate_concat_backward(_stream(), _gate_branches(_l, v, cs, slices), len(cs), n, s, v["dy"].data_ptr(),
                                             v["m"].data_ptr(), v["g"].data_ptr(), v["ws"].data_ptr(), nbytes - ws_short, accumulate)
    return spec, (lambda v: _l.check(call(v), "cstp_gate_concat_backward")), call


@pytest.mark.parametrize("want_g,want_cell", [(True, True), (False, True), (True, False)], ids=["g+cell", "no g", "no cell"])
@pytest.mark.parametrize("name", list(GATES))
def test_gate_concat_forward(name, want_g, want_cell):
    spec, impl, cells = _gate_fwd_case(name, want_g, want_cell)
    _run3(spec, impl)
    assert all(a == b for a, b in cells), cells


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("name", list(GATES))
def test_gate_concat_backward(name, accumulate):
    spec, impl, _ = _gate_bwd_case(name, accumulate)
    _run3(spec, impl)


def _same_bits_as(aligned, spec, impl):
    """Run the aligned case once, then hold the misaligned one to its bits as well."""
    clean, found = gb.one_run(aligned[0], gb.Operands(aligned[0], DEV), aligned[1], "nan", torch.cuda.synchronize)
    assert found == [], "\n".join(found)
    for name in spec.checks:
        spec.checks[name] = gb.all_checks(spec.checks[name], gb.bits_check(clean[name]))
    if "cell" in clean:
        spec.checks["cell"] = gb.bits_check(clean["cell"])
    _run3(spec, impl)


def test_gate_concat_forward_with_y_off_16_bytes_takes_the_scalar_bodies_and_gives_the_same_bits():
    spec, impl, cells = _gate_fwd_case("float4", shifts={"y": 4})
    _same_bits_as(_gate_fwd_case("float4")[:2], spec, impl)
    assert all(a == b for a, b in cells), cells


def test_gate_concat_backward_with_dy_off_16_bytes_takes_the_scalar_bodies_and_gives_the_same_bits():
    spec, impl, _ = _gate_bwd_case("float4", 1, shifts={"dy": 4})
    _same_bits_as(_gate_bwd_case("float4", 1)[:2], spec, impl)


def test_refused_gate_backward_with_a_short_workspace_touches_nothing():
    spec, _, call = _gate_bwd_case("ragged", 1, ws_short=1)
    _assert_refused(spec, call, b"workspace too small")


# ============================================================================================================================
# Concat tails: cstp_bnrelu_concat_* (mixed.hip)
# ============================================================================================================================
def _bnc_branches(_l, v, cs, parts=(), running=True, bwd=None, cells=()):
    arr = (_l.BncBranch * len(cs))()
    for i, c in enumerate(cs):
        arr[i].x, arr[i].gamma, arr[i].c = v["x%d" % i].data_ptr(), v["gamma%d" % i].data_ptr(), c
        arr[i].beta = _ptr(v, "beta%d" % i)
        if running:
            arr[i].running_mean, arr[i].running_var = v["rm%d" % i].data_ptr(), v["rv%d" % i].data_ptr()
        if i in parts:
            arr[i].part, arr[i].nsplit = v["part%d" % i].data_ptr(), 3
        if bwd is not None:
            arr[i].dx = v["dx%d" % i].data_ptr()
            arr[i].dgamma = v["grads"].data_ptr() + 4 * bwd[i][0]
            arr[i].dbeta = v["grads"].data_ptr() + 4 * bwd[i][1]
            if i in cells:
                arr[i].dx_absmax = v["cell%d" % i].data_ptr()
    return arr


def _bnc_fwd_case(name, stats, running=True, shifts=None):
    """stats: "own" (one statistics launch), "part" (every branch brings the producing convolution's sums, nsplit = 3), "mixed"
    (branch 1 alone does).  y, running statistics 1e-6, the saved statistics 1e-6 (test_bn_relu_concat_matches_fp64_and_composed)."""
    _l, lib = _libs()
    cs, spatial, n, groups, seed = gc.BNC_CASES[name]
    r = gc.bnc_case(cs, spatial, n, groups, seed)
    C, s = sum(cs), int(np.prod(spatial))
    parts = {"own": (), "part": tuple(range(len(cs))), "mixed": (1,)}[stats]
    inputs, outputs, checks, priors = {}, {}, {}, {}
    for i in range(len(cs)):
        inputs.update({"x%d" % i: r["xs"][i], "gamma%d" % i: r["gammas"][i], "beta%d" % i: r["betas"][i]})
        if i in parts:
            inputs["part%d" % i] = gc.conv_sums(r["xs"][i], groups, r["rms"][i])
        if running:
            for k, old, new in (("rm", r["rms"], r["rm_new"]), ("rv", r["rvs"], r["rv_new"])):
                outputs["%s%d" % (k, i)], priors["%s%d" % (k, i)] = ((cs[i],), F32), old[i]
                checks["%s%d" % (k, i)] = gb.rel_check(new[i], 1e-6)
    outputs.update({"y": ((n, C) + spatial, F32), "mean": ((groups, C), F32), "invstd": ((groups, C), F32), "ss": ((groups, C, 2), F32),
                    "cell": ((1,), I32)})
    checks.update({"y": gb.rel_check(r["y"], 1e-6), "mean": gb.rel_check(r["mean"], 1e-6), "invstd": gb.rel_check(r["invstd"], 1e-6),
                   "ss": gb.rel_check(r["ss"], 1e-6)})
    nbytes = lib.cstp_bnrelu_concat_workspace_bytes(C, groups)
    spec = gb.Spec("bnrelu_concat forward %s %s running%d %s" % (name, stats, running, shifts or ""), inputs, outputs, checks,
                   ws_bytes=nbytes, priors=priors, shifts=shifts, finite_as={"cell": F32})
    cells = []

    def impl(v):
        _l.check(lib.cstp_bnrelu_concat_forward(_stream(), _bnc_branches(_l, v, cs, parts, running), len(cs), n, s, groups, gc.BN_EPS,
                                                gc.BN_MOM, v["y"].data_ptr(), v["mean"].data_ptr(), v["invstd"].data_ptr(),
                                                v["ss"].data_ptr(), v["ws"].data_ptr(), nbytes, v["cell"].data_ptr()),
                 "cstp_bnrelu_concat_forward")
        torch.cuda.synchronize()
        cells.append((int(v["cell"].item()), int(v["y"].abs().max().view(I32).item())))
    return spec, impl, cells


@pytest.mark.parametrize("stats", ["own", "part", "mixed"])
@pytest.mark.parametrize("name", ["ragged g1", "ragged g2"])
def test_bnrelu_concat_forward(name, stats):
    spec, impl, cells = _bnc_fwd_case(name, stats)
    _run3(spec, impl)
    assert all(a == b for a, b in cells), cells


@pytest.mark.parametrize("name,shifts", [("float4", None), ("float4", {"y": 4}), ("strided", None)],
                         ids=["float4", "float4 y misaligned", "strided"])
def test_bnrelu_concat_forward_vector_and_strided(name, shifts):
    spec, impl, cells = _bnc_fwd_case(name, "own", shifts=shifts)
    _run3(spec, impl)
    assert all(a == b for a, b in cells), cells


def test_bnrelu_concat_forward_without_running_statistics():
    spec, impl, cells = _bnc_fwd_case("ragged g2", "mixed", running=False)
    _run3(spec, impl)
    assert all(a == b for a, b in cells), cells


def test_bnrelu_concat_eval():
    """1e-6: test_bn_relu_concat_eval_equals_batch_norm_eval.  The running statistics are inputs here."""
    _l, lib = _libs()
    cs, spatial, n, groups, seed = gc.BNC_CASES["ragged g1"]
    r = gc.bnc_case(cs, spatial, n, groups, seed)
    C, s = sum(cs), int(np.prod(spatial))
    inputs = {}
    for i in range(len(cs)):
        inputs.update({"x%d" % i: r["xs"][i], "gamma%d" % i: r["gammas"][i], "beta%d" % i: r["betas"][i], "rm%d" % i: r["rms"][i],
                       "rv%d" % i: r["rvs"][i]})
    spec = gb.Spec("bnrelu_concat eval", inputs, {"y": ((n, C) + spatial, F32), "ss": ((C, 2), F32), "cell": ((1,), I32)},
                   {"y": gb.rel_check(r["y_eval"], 1e-6)}, finite_as={"cell": F32})
    cells = []

    def impl(v):
        _l.check(lib.cstp_bnrelu_concat_eval(_stream(), _bnc_branches(_l, v, cs), len(cs), n, s, gc.BN_EPS, v["y"].data_ptr(),
                                             v["ss"].data_ptr(), v["cell"].data_ptr()), "cstp_bnrelu_concat_eval")
        torch.cuda.synchronize()
        cells.append((int(v["cell"].item()), int(v["y"].abs().max().view(I32).item())))
    _run3(spec, impl)
    assert all(a == b for a, b in cells), cells


def _bnc_layout(cs):
    slices, pos = [], 3
    for c in cs:
        slices.append((pos, pos + c + 2))
        pos += 2 * c + 2 + 5
    own = torch.zeros(pos, dtype=torch.bool)
    for (a, b), c in zip(slices, cs):
        own[a:a + c] = True
        own[b:b + c] = True
    return slices, pos, own


def _bnc_bwd_case(name, accumulate, shifts=None):
    """dx, dgamma, dbeta at 1e-5 (test_bn_relu_concat_matches_fp64_and_composed).  The saved statistics and the affine table are
    the fp64 reference's, rounded to fp32; dy is 0 at the ReLU kinks; dx_absmax cells on the odd branches only."""
    _l, lib = _libs()
    cs, spatial, n, groups, seed = gc.BNC_CASES[name]
    r = gc.bnc_case(cs, spatial, n, groups, seed)
    assert r["kink_share"] <= gc.KINK_CAP
    C, s = sum(cs), int(np.prod(spatial))
    slices, total, own = _bnc_layout(cs)
    prior = (_rand((total,), 78) * 0.5).float()
    ref = prior.double().clone()
    if not accumulate:
        prior[own] = float("nan")
        ref[own] = 0.0
    for (a, b), c, dg, db in zip(slices, cs, r["dgamma"], r["dbeta"]):
        ref[a:a + c] += dg
        ref[b:b + c] += db

    def grads_check(got):
        for (a, b), c in zip(slices, cs):
            for lo in (a, b):
                gb.rel_check(ref[lo:lo + c], 1e-5)(got[lo:lo + c])
    cell_on = tuple(i for i in range(len(cs)) if i % 2 == 1)
    inputs = {"dy": r["dy"], "mean": r["mean"].float(), "invstd": r["invstd"].float(), "ss": r["ss"].float()}
    outputs = {"grads": ((total,), F32)}
    checks = {"grads": gb.all_checks(gb.untouched_check(prior, ~own), grads_check)}
    finite_as = {}
    for i in range(len(cs)):
        inputs.update({"x%d" % i: r["xs"][i], "gamma%d" % i: r["gammas"][i]})
        outputs["dx%d" % i] = (tuple(r["xs"][i].shape), F32)
        checks["dx%d" % i] = gb.rel_check(r["dx"][i], 1e-5)
        if i in cell_on:
            outputs["cell%d" % i], finite_as["cell%d" % i] = ((1,), I32), F32
    nbytes = lib.cstp_bnrelu_concat_workspace_bytes(C, groups)
    spec = gb.Spec("bnrelu_concat backward %s accumulate%d %s" % (name, accumulate, shifts or ""), inputs, outputs, checks,
                   ws_bytes=nbytes, priors={"grads": prior}, shifts=shifts, finite_as=finite_as)
    cells = []

    def impl(v):
        _l.check(lib.cstp_bnrelu_concat_backward(_stream(), _bnc_branches(_l, v, cs, running=False, bwd=slices, cells=cell_on), len(cs),
                                                 n, s, groups, v["dy"].data_ptr(), v["mean"].data_ptr(), v["invstd"].data_ptr(),
                                                 v["ss"].data_ptr(), v["ws"].data_ptr(), nbytes, accumulate),
                 "cstp_bnrelu_concat_backward")
        torch.cuda.synchronize()
        cells.extend((int(v["cell%d" % i].item()), int(v["dx%d" % i].abs().max().view(I32).item())) for i in cell_on)
    return spec, impl, cells


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("name,shifts", [("ragged g1", None), ("ragged g2", None), ("float4", None), ("float4", {"dy": 4}),
                                         ("strided", None)],
                         ids=["ragged g1", "ragged g2", "float4", "float4 dy misaligned", "strided"])
def test_bnrelu_concat_backward(name, shifts, accumulate):
    spec, impl, cells = _bnc_bwd_case(name, accumulate, shifts)
    _run3(spec, impl)
    assert all(a == b for a, b in cells), cells


# ============================================================================================================================
# Pools: pool.h through misc.hip (fp32) and b16.hip (bf16); the SAME pool and the windowed average of mixed.hip
# ============================================================================================================================
MAXPOOLS = {
    # name: (rows, volume, kernel, stride, pad)
    "k3s2p1": (3, (5, 7, 9), (3, 3, 3), (2, 2, 2), (1, 1, 1)),       # the last window of a row reaches one past its end
    "k2s2p0": (3, (4, 7, 7), (2, 2, 2), (2, 2, 2), (0, 0, 0)),       # the last row / column of inputs lies in no window
}


@functools.lru_cache(maxsize=None)
def _maxpool_ref(name):
    """Multiples of 0.5 (exact in bf16), the LAST volume all negative: a padding candidate, or whatever follows x, must not win."""
    rows, vol, k, s, p = MAXPOOLS[name]
    g = torch.Generator().manual_seed(3 + sum(vol))
    x = torch.randint(-4, 5, (rows,) + vol, generator=g).double() * 0.5
    x[-1] = -x[-1].abs() - 0.5
    xr = x.clone().requires_grad_(True)
    y, idx = F.max_pool3d(xr, k, s, p, return_indices=True)
    dy = (torch.rand(tuple(y.shape), generator=g, dtype=F64) * 2 - 1).to(B16).double()
    (dx,) = torch.autograd.grad(y, xr, dy)
    return {"x": x, "y": y.detach(), "argmax": idx.to(I32), "dy": dy, "dx": dx}


def _dx_check(ref64, dtype):
    """fp32: 1e-6 and exactly 0 where ATen's gradient is 0 (ops_edge_cases.pool_compare); bf16: the correctly rounded sum."""
    if dtype == B16:
        return gb.all_checks(gb.rounded_check(ref64), lambda got: _zero_where(ref64, got))
    return gb.all_checks(gb.rel_check(ref64, 1e-6), lambda got: _zero_where(ref64, got))


def _zero_where(ref64, got):
    assert bool((got.double()[ref64 == 0] == 0).all()), "nonzero where ATen's gradient is exactly 0"


@pytest.mark.parametrize("dtype", [F32, B16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(MAXPOOLS))
def test_max_pool3d(name, dtype):
    """y and argmax are ATen's, bit for bit (test_max_pool3d_edges / _bf16_edges); the backward reads ATen's argmax."""
    _l, lib = _libs()
    rows, vol, k, s, p = MAXPOOLS[name]
    r = _maxpool_ref(name)
    fwd, bwd = (lib.cstp_maxpool3d_forward, lib.cstp_maxpool3d_backward) if dtype == F32 else \
        (lib.cstp_b16_maxpool3d_forward, lib.cstp_b16_maxpool3d_backward)
    oshape = tuple(r["y"].shape)
    spec = gb.Spec("max_pool3d forward %s %s" % (name, dtype), {"x": r["x"].to(dtype)}, {"y": (oshape, dtype), "argmax": (oshape, I32)},
                   {"y": gb.bits_check(r["y"].to(dtype)), "argmax": gb.bits_check(r["argmax"])}, finite_as={"argmax": None})
    _run3(spec, lambda v: _l.check(fwd(_stream(), v["x"].data_ptr(), v["y"].data_ptr(), v["argmax"].data_ptr(), rows, *vol, _i3(k),
                                       _i3(s), _i3(p)), "maxpool3d_forward"))
    spec = gb.Spec("max_pool3d backward %s %s" % (name, dtype), {"dy": r["dy"].to(dtype), "argmax": r["argmax"]},
                   {"dx": ((rows,) + vol, dtype)}, {"dx": _dx_check(r["dx"], dtype)})
    _run3(spec, lambda v: _l.check(bwd(_stream(), v["dy"].data_ptr(), v["argmax"].data_ptr(), v["dx"].data_ptr(), rows, *vol, _i3(k),
                                       _i3(s), _i3(p)), "maxpool3d_backward"))


def test_refused_max_pool_with_padding_past_half_the_kernel_touches_nothing():
    _l, lib = _libs()
    x = _rand((2, 4, 4, 4), 1).float()
    spec = gb.Spec("max_pool3d 2 * pad > kernel", {"x": x}, {"y": ((2, 3, 3, 3), F32), "argmax": ((2, 3, 3, 3), I32)}, {})
    _assert_refused(spec, lambda v: lib.cstp_maxpool3d_forward(_stream(), v["x"].data_ptr(), v["y"].data_ptr(), v["argmax"].data_ptr(),
                                                               2, 4, 4, 4, _i3((2, 2, 2)), _i3((2, 2, 2)), _i3((2, 2, 2))),
                    b"bad pooling geometry")


@pytest.mark.parametrize("dtype", [F32, B16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("s", [1, 65])
def test_global_avg_pool(s, dtype):
    """rows = 5: the last block (4 rows per block) holds one row; odd s puts bf16 rows on 2-byte boundaries.  fp32: 1e-4
    (ops_edge_cases.avg_case); bf16: the mean within 1e-5, dx the correctly rounded value (test_b16_gpu.py test_pooling_bf16)."""
    _l, lib = _libs()
    rows = 5
    x = _rand((rows, s), 40 + s).to(dtype)
    dy = _rand((rows,), 41 + s).float()
    mean = x.double().mean(1)
    dx = (dy.double() / s).view(rows, 1).expand(rows, s).contiguous()
    fwd, bwd = (lib.cstp_avgpool_forward, lib.cstp_avgpool_backward) if dtype == F32 else \
        (lib.cstp_b16_avgpool_forward, lib.cstp_b16_avgpool_backward)

    def mean_check(got):
        assert float((got.double() - mean).abs().max()) < 1e-5
    spec = gb.Spec("avgpool forward s%d %s" % (s, dtype), {"x": x}, {"y": ((rows,), F32)},
                   {"y": gb.rel_check(mean, 1e-4) if dtype == F32 else mean_check})
    _run3(spec, lambda v: _l.check(fwd(_stream(), v["x"].data_ptr(), v["y"].data_ptr(), rows, s), "avgpool_forward"))
    spec = gb.Spec("avgpool backward s%d %s" % (s, dtype), {"dy": dy}, {"dx": ((rows, s), dtype)},
                   {"dx": gb.rel_check(dx, 1e-4) if dtype == F32 else gb.rounded_check(dx)})
    _run3(spec, lambda v: _l.check(bwd(_stream(), v["dy"].data_ptr(), v["dx"].data_ptr(), rows, s), "avgpool_backward"))


SAME_POOLS = {
    # name: (rows, volume, kernel, stride)
    "k3s1 R64": (65, (2, 4, 4), (3, 3, 3), (1, 1, 1)),               # R = 64: the second block stages ONE volume
    "k3s2 ceil": (7, (5, 7, 9), (3, 3, 3), (2, 2, 2)),               # R = 6; the ceil-mode window past the padded extent
    "direct fwd": (2, (8, 40, 40), (1, 3, 3), (1, 2, 2)),            # 12800 floats > POOL_LDS_FLOATS: direct forward, LDS backward, R = 1
    "direct bwd": (2, (8, 56, 56), (1, 3, 3), (1, 2, 2)),            # 2 * 6272 outputs > POOL_LDS_FLOATS: the direct backward
}


@pytest.mark.parametrize("name", list(SAME_POOLS))
def test_max_pool3d_same(name):
    """y and argmax are ATen's over the padded tensor (test_max_pool3d_same_matches_aten), -1 where a padding zero won; dx 1e-6."""
    _l, lib = _libs()
    rows, vol, k, s = SAME_POOLS[name]
    r = gc.same_pool_case(rows, vol, k, s)
    oshape = tuple(r["y"].shape)
    assert oshape[1:] == tuple(lib.cstp_maxpool3d_same_out(vol[i], k[i], s[i]) for i in range(3))
    spec = gb.Spec("max_pool3d_same forward " + name, {"x": r["x"]}, {"y": (oshape, F32), "argmax": (oshape, I32)},
                   {"y": gb.bits_check(r["y"].float()), "argmax": gb.bits_check(r["argmax"])}, finite_as={"argmax": None})
    _run3(spec, lambda v: _l.check(lib.cstp_maxpool3d_same_forward(_stream(), v["x"].data_ptr(), v["y"].data_ptr(), v["argmax"].data_ptr(),
                                                                   rows, *vol, _i3(k), _i3(s)), "cstp_maxpool3d_same_forward"))
    spec = gb.Spec("max_pool3d_same backward " + name, {"dy": r["dy"], "argmax": r["argmax"]}, {"dx": ((rows,) + vol, F32)},
                   {"dx": _dx_check(r["dx"], F32)})
    _run3(spec, lambda v: _l.check(lib.cstp_maxpool3d_same_backward(_stream(), v["dy"].data_ptr(), v["argmax"].data_ptr(),
                                                                    v["dx"].data_ptr(), rows, *vol, _i3(k), _i3(s)),
                                   "cstp_maxpool3d_same_backward"))


def test_max_pool3d_same_forward_without_argmax():
    _l, lib = _libs()
    rows, vol, k, s = SAME_POOLS["k3s1 R64"]
    r = gc.same_pool_case(rows, vol, k, s)
    spec = gb.Spec("max_pool3d_same forward, argmax NULL", {"x": r["x"]}, {"y": (tuple(r["y"].shape), F32)},
                   {"y": gb.bits_check(r["y"].float())})
    _run3(spec, lambda v: _l.check(lib.cstp_maxpool3d_same_forward(_stream(), v["x"].data_ptr(), v["y"].data_ptr(), None, rows, *vol,
                                                                   _i3(k), _i3(s)), "cstp_maxpool3d_same_forward"))


@pytest.mark.parametrize("vol,k", [((3, 4, 5), (1, 2, 3)), ((2, 7, 7), (2, 7, 7))], ids=["windows", "single output"])
def test_avg_pool3d_window(vol, k):
    """1e-6: test_i3d_gpu.py test_avg_pool3d_window."""
    _l, lib = _libs()
    rows = 3
    x = _rand((rows,) + vol, 50).float()
    xr = x.double().requires_grad_(True)
    y = F.avg_pool3d(xr, k, 1)
    dy = _rand(tuple(y.shape), 51).float()
    (dx,) = torch.autograd.grad(y, xr, dy.double())
    spec = gb.Spec("avg_pool3d_window forward %s" % (vol,), {"x": x}, {"y": (tuple(y.shape), F32)}, {"y": gb.rel_check(y.detach(), 1e-6)})
    _run3(spec, lambda v: _l.check(lib.cstp_avgpool3d_window_forward(_stream(), v["x"].data_ptr(), v["y"].data_ptr(), rows, *vol, _i3(k)),
                                   "cstp_avgpool3d_window_forward"))
    spec = gb.Spec("avg_pool3d_window backward %s" % (vol,), {"dy": dy}, {"dx": ((rows,) + vol, F32)}, {"dx": gb.rel_check(dx, 1e-6)})
    _run3(spec, lambda v: _l.check(lib.cstp_avgpool3d_window_backward(_stream(), v["dy"].data_ptr(), v["dx"].data_ptr(), rows, *vol,
                                                                      _i3(k)), "cstp_avgpool3d_window_backward"))


# ============================================================================================================================
# Heads (misc.hip, ntxq.h)
# ============================================================================================================================
def _edge_check(what, name, out):
    """ops_edge_cases.compare on one output: the global AND the row-wise metric at the bar of the parity test."""
    def check(got):
        fails = ec.compare(what, {name: out}, {name: got})
        assert fails == [], "; ".join(fails)
    return check


@pytest.mark.parametrize("f", [1, 65])
def test_byol_loss(f):
    """rows = 3 with an all-zero x row and an all-zero target row (ops_edge_cases "special"); bars 1e-4 (byol_case)."""
    _l, lib = _libs()
    x, t, dl, _ = ec.norm_inputs(f, "special")
    outs = ec.byol_case(f, "special")
    what = "byol f%d" % f
    spec = gb.Spec(what + " forward", {"x": x, "t": t}, {"loss": ((3,), F32)}, {"loss": _edge_check(what, "loss", outs["loss"])})
    _run3(spec, lambda v: _l.check(lib.cstp_byol_loss_forward(_stream(), v["x"].data_ptr(), v["t"].data_ptr(), v["loss"].data_ptr(), 3, f),
                                   "cstp_byol_loss_forward"))
    spec = gb.Spec(what + " backward", {"x": x, "t": t, "dl": dl}, {"dx": ((3, f), F32)}, {"dx": _edge_check(what, "dx", outs["dx"])})
    _run3(spec, lambda v: _l.check(lib.cstp_byol_loss_backward(_stream(), v["x"].data_ptr(), v["t"].data_ptr(), v["dl"].data_ptr(),
                                                               v["dx"].data_ptr(), 3, f), "cstp_byol_loss_backward"))


@pytest.mark.parametrize("f", [1, 65])
def test_l2_normalize(f):
    """Bars 1e-5 (l2_case); the backward reads y and norm of the fp64 reference, rounded to fp32."""
    _l, lib = _libs()
    x, _, _, dy = ec.norm_inputs(f, "special")
    outs = ec.l2_case(f, "special")
    norm = x.double().norm(dim=1).clamp_min(ec.NORM_EPS)
    what = "l2_normalize f%d" % f
    spec = gb.Spec(what + " forward", {"x": x}, {"y": ((3, f), F32), "norm": ((3,), F32)},
                   {"y": _edge_check(what, "y", outs["y"]), "norm": _edge_check(what, "norm", ec.Out(norm.reshape(3, 1), 1e-5, 0.0))})
    _run3(spec, lambda v: _l.check(lib.cstp_l2_normalize_forward(_stream(), v["x"].data_ptr(), v["y"].data_ptr(), v["norm"].data_ptr(), 3,
                                                                 f, ec.NORM_EPS), "cstp_l2_normalize_forward"))
    spec = gb.Spec(what + " backward", {"y": outs["y"].ref.float(), "norm": norm.float(), "dy": dy}, {"dx": ((3, f), F32)},
                   {"dx": _edge_check(what, "dx", outs["dx"])})
    _run3(spec, lambda v: _l.check(lib.cstp_l2_normalize_backward(_stream(), v["y"].data_ptr(), v["norm"].data_ptr(), v["dy"].data_ptr(),
                                                                  v["dx"].data_ptr(), 3, f, ec.NORM_EPS), "cstp_l2_normalize_backward"))


@pytest.mark.parametrize("b,k", [(3, 5), (1025, 2)])
def test_cross_entropy(b, k):
    """b = 1025: more rows than a block has threads.  Bars 1e-4 (ce_case); the int64 labels sit between -1 guards."""
    _l, lib = _libs()
    z, lab, _, _ = ec.ce_inputs(b, k, "randn30")
    outs = ec.ce_case(b, k, "randn30")
    what = "ce b%d k%d" % (b, k)
    spec = gb.Spec(what + " forward", {"z": z, "lab": lab}, {"loss": ((1,), F32)}, {"loss": _edge_check(what, "loss", outs["loss"])})
    _run3(spec, lambda v: _l.check(lib.cstp_cross_entropy_forward(_stream(), v["z"].data_ptr(), v["lab"].data_ptr(), v["loss"].data_ptr(),
                                                                  b, k), "cstp_cross_entropy_forward"))
    spec = gb.Spec(what + " backward", {"z": z, "lab": lab, "dloss": torch.tensor([ec.DLOSS], dtype=F32)}, {"dz": ((b, k), F32)},
                   {"dz": _edge_check(what, "dlogits", outs["dlogits"])})
    _run3(spec, lambda v: _l.check(lib.cstp_cross_entropy_backward(_stream(), v["z"].data_ptr(), v["lab"].data_ptr(),
                                                                   v["dloss"].data_ptr(), v["dz"].data_ptr(), b, k),
                                   "cstp_cross_entropy_backward"))


@pytest.mark.parametrize("mixed", [True, False], ids=["tb+lam", "tb lam NULL"])
def test_soft_cross_entropy(mixed):
    """b = 17, k = 65: 16 waves plus one row, a lane tail.  One target one past the classes and one at -1: no one-hot mass, never
    an index (between NaN guards an indexed read would show).  Bars 1e-5: test_mix_gpu.py
    test_soft_cross_entropy_ignores_targets_outside_the_classes."""
    _l, lib = _libs()
    b, k, eps = 17, 65, f32(0.1)
    z, ta, tb, lam = ec.ce_inputs(b, k, "randn30")
    ta, tb = ta.clone(), tb.clone()
    ta[1], tb[2] = k, -1
    if not mixed:
        tb, lam = ta, torch.ones(b)
    q = torch.full((b, k), eps / k, dtype=F64)
    for r in range(b):
        if 0 <= int(ta[r]) < k:
            q[r, ta[r]] += (1 - eps) * float(lam[r])
        if 0 <= int(tb[r]) < k:
            q[r, tb[r]] += (1 - eps) * (1 - float(lam[r]))
    x = z.double().requires_grad_(True)
    want = -(q * F.log_softmax(x, dim=1)).sum(dim=1).mean()
    (want * ec.DLOSS).backward()
    want = float(want.detach())

    def loss_check(got):
        assert abs(float(got[0]) - want) < 1e-5 * abs(want), (float(got[0]), want)

    def grad_check(got):
        assert float((got.double() - x.grad).abs().max()) < 1e-5 * float(x.grad.abs().max())
    inputs = {"z": z, "ta": ta}
    if mixed:
        inputs.update({"tb": tb, "lam": lam})
    spec = gb.Spec("soft_ce forward mixed%d" % mixed, inputs, {"loss": ((1,), F32)}, {"loss": loss_check})
    _run3(spec, lambda v: _l.check(lib.cstp_soft_cross_entropy_forward(_stream(), v["z"].data_ptr(), v["ta"].data_ptr(), _ptr(v, "tb"),
                                                                       _ptr(v, "lam"), eps, v["loss"].data_ptr(), b, k),
                                   "cstp_soft_cross_entropy_forward"))
    inputs = dict(inputs, dloss=torch.tensor([ec.DLOSS], dtype=F32))
    spec = gb.Spec("soft_ce backward mixed%d" % mixed, inputs, {"dz": ((b, k), F32)}, {"dz": grad_check})
    _run3(spec, lambda v: _l.check(lib.cstp_soft_cross_entropy_backward(_stream(), v["z"].data_ptr(), v["ta"].data_ptr(), _ptr(v, "tb"),
                                                                        _ptr(v, "lam"), eps, v["dloss"].data_ptr(), v["dz"].data_ptr(),
                                                                        b, k), "cstp_soft_cross_entropy_backward"))


@pytest.mark.parametrize("n,f", [(2, 5), (3, 257)])
def test_ntxent_forward_backward_pair(n, f):
    """The pair shares a workspace of exactly cstp_ntxent_workspace_bytes, poisoned before the forward only: the backward must
    find what the forward wrote.  Bars 1e-4 (ops_edge_cases.ntx_case)."""
    _l, lib = _libs()
    tau = 0.5
    zi, zj = ec.ntx_inputs(n, f)
    reps = torch.cat([zj, zi], 0)
    r = ec.ntx_host(zi, zj, tau, F64)
    nbytes = lib.cstp_ntxent_workspace_bytes(2 * n, f)
    spec = gb.Spec("ntxent 2n%d f%d" % (2 * n, f), {"reps": reps, "dloss": torch.tensor([ec.DLOSS], dtype=F32)},
                   {"loss": ((1,), F32), "dreps": ((2 * n, f), F32)},
                   {"loss": gb.rel_check(r["loss"].reshape(1), 1e-4), "dreps": gb.rel_check(r["dreps"], 1e-4)}, ws_bytes=nbytes)

    def impl(v):
        _l.check(lib.cstp_ntxent_forward(_stream(), v["reps"].data_ptr(), v["loss"].data_ptr(), 2 * n, f, tau, v["ws"].data_ptr(), nbytes),
                 "cstp_ntxent_forward")
        _l.check(lib.cstp_ntxent_backward(_stream(), v["reps"].data_ptr(), v["dloss"].data_ptr(), v["dreps"].data_ptr(), 2 * n, f, tau,
                                          v["ws"].data_ptr(), nbytes), "cstp_ntxent_backward")
    _run3(spec, impl)


@pytest.mark.parametrize("n,f,n_valid,cap", [(3, 33, 129, 129), (2, 260, 5, 5), (2, 33, 0, 8)],
                         ids=["second tile holds one row", "second feature slice of 4", "empty queue"])
def test_ntxq_forward_backward_pair(n, f, n_valid, cap):
    """cap = n_valid = 129: what follows the single row of the second queue tile is the guard, not masked rows.  The queue is an
    input: unchanged.  Bar 1e-4 (ntxq_spec.BAR)."""
    _l, lib = _libs()
    T = 0.5
    reps, queue = ntxq_spec.inputs(n, f, n_valid, cap, 7)
    r = ntxq_spec.ref(reps, queue, n_valid, T, F64)
    R = 2 * n
    nbytes = lib.cstp_ntxq_workspace_bytes(R, f, n_valid)
    spec = gb.Spec("ntxq R%d f%d n_valid%d" % (R, f, n_valid),
                   {"reps": reps, "queue": queue, "dloss": torch.tensor([ntxq_spec.DLOSS], dtype=F32)},
                   {"loss": ((1,), F32), "dreps": ((R, f), F32)},
                   {"loss": gb.rel_check(r["loss"].double().reshape(1), ntxq_spec.BAR),
                    "dreps": gb.rel_check(r["dreps"].double(), ntxq_spec.BAR)}, ws_bytes=nbytes)

    def impl(v):
        _l.check(lib.cstp_ntxq_forward(_stream(), v["reps"].data_ptr(), v["queue"].data_ptr(), v["loss"].data_ptr(), R, f, cap, n_valid, T,
                                       v["ws"].data_ptr(), nbytes), "cstp_ntxq_forward")
        _l.check(lib.cstp_ntxq_backward(_stream(), v["reps"].data_ptr(), v["queue"].data_ptr(), v["dloss"].data_ptr(),
                                        v["dreps"].data_ptr(), R, f, cap, n_valid, T, v["ws"].data_ptr(), nbytes), "cstp_ntxq_backward")
    _run3(spec, impl)


def _push_case(ptr):
    R, f, cap = 3, 33, 8
    g = torch.Generator().manual_seed(R + f)
    reps = torch.randn(R, f, generator=g) * 3
    reps[1] = 0
    before = torch.randn(cap, f, generator=g)
    return R, f, cap, reps, before


@pytest.mark.parametrize("ptr", [0, 5])
def test_ntxq_push(ptr):
    """The ring is a prior: rows outside [ptr, ptr + R) keep their bits; inside, test_ntxq_gpu.py test_push's one-ulp criterion
    and a zero row written as zeros."""
    _l, lib = _libs()
    R, f, cap, reps, before = _push_case(ptr)
    keep = torch.ones(cap, f, dtype=torch.bool)
    keep[ptr:ptr + R] = False
    want = ntxq_spec.normalize(reps.double())

    def rows_check(got):
        rows = got[ptr:ptr + R]
        assert torch.equal(rows[1], torch.zeros(f)), "the zero row"
        ulp = 2.0 ** -23
        excess = (rows.double() - want).abs() - ulp * (1 + 2.0 ** -20) * want.abs()
        assert float(excess.max()) <= 0, float(excess.max())
        norms = rows.double().norm(dim=1)
        assert float((torch.cat([norms[:1], norms[2:]]) - 1).abs().max()) <= ulp
    spec = gb.Spec("ntxq_push ptr%d" % ptr, {"reps": reps}, {"queue": ((cap, f), F32)},
                   {"queue": gb.all_checks(gb.untouched_check(before, keep), rows_check)}, priors={"queue": before})
    _run3(spec, lambda v: _l.check(lib.cstp_ntxq_push(_stream(), v["reps"].data_ptr(), v["queue"].data_ptr(), R, f, cap, ptr),
                                   "cstp_ntxq_push"))


def test_refused_ntxq_push_past_the_end_of_the_ring_touches_nothing():
    _l, lib = _libs()
    R, f, cap, reps, before = _push_case(6)
    spec = gb.Spec("ntxq_push ptr 6 of 8, 3 rows", {"reps": reps}, {"queue": ((cap, f), F32)}, {}, priors={"queue": before})
    _assert_refused(spec, lambda v: lib.cstp_ntxq_push(_stream(), v["reps"].data_ptr(), v["queue"].data_ptr(), R, f, cap, 6),
                    b"must lie inside the queue")


# ============================================================================================================================
# Regularisers, cast, mix (reg.h, b16.hip, clip.hip)
# ============================================================================================================================
KEY, OFFSET = 0x1234567890ABCDEF, 3


@pytest.mark.parametrize("shift", [0, 4], ids=["aligned", "x 4 bytes off"])
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("n", [1, 5, 1027])
def test_dropout(n, p, shift):
    """The mask of tests/reg_spec.py, bit for bit (test_dropout_equals_the_restatement_bit_for_bit); x 4 bytes off a 16-byte
    boundary takes the element path and must give the same bits -- the same reference serves both."""
    _l, lib = _libs()
    x = _rand((n,), 60 + n).float()
    want = torch.from_numpy(reg_spec.dropout_fp32(x.numpy(), p, KEY, OFFSET))
    spec = gb.Spec("dropout n%d p%g shift%d" % (n, p, shift), {"x": x}, {"y": ((n,), F32)}, {"y": gb.bits_check(want)},
                   shifts={"x": shift})
    _run3(spec, lambda v: _l.check(lib.cstp_dropout(_stream(), v["x"].data_ptr(), v["y"].data_ptr(), n, p, KEY, OFFSET), "cstp_dropout"))


def test_refused_dropout_with_p_1_touches_nothing():
    _l, lib = _libs()
    x = _rand((5,), 61).float()
    spec = gb.Spec("dropout p = 1", {"x": x}, {"y": ((5,), F32)}, {})
    _assert_refused(spec, lambda v: lib.cstp_dropout(_stream(), v["x"].data_ptr(), v["y"].data_ptr(), 5, 1.0, KEY, OFFSET),
                    b"dropout probability outside")


def _bf16_ulp_check(ref32):
    """test_reg_gpu.py test_drop_path_bf16_storage: within one bf16 ulp (at |ref|) of the fp32 composition on the same inputs."""
    def check(got):
        ulp = torch.maximum(ref32.abs(), torch.tensor(2.0 ** -126)).log2().floor().exp2() * 2.0 ** -7
        assert bool(((got.float() - ref32).abs() <= ulp).all())
    return check


@pytest.mark.parametrize("row", [6, 8])
@pytest.mark.parametrize("dtype", [F32, B16], ids=["fp32", "bf16"])
def test_drop_path_add_relu(dtype, row):
    """Three samples with scale [0, 2, 1]; row 6 takes the element bodies, 8 the 16-byte ones.  fp32: 1e-6
    (test_drop_path_fp32_matches_fp64), a dropped sample is relu(res) bit for bit, the absmax cell (a ZERO prior: it "holds 0 on
    entry") is max |y| of this y; bf16: one ulp.  Backward with dz NULL, with dres NULL and with both: dres is dy's bits or +0."""
    _l, lib = _libs()
    bf = 1 if dtype == B16 else 0
    z, res, dy = ((_rand((3, row), 70 + i + row) * 2).to(dtype) for i in range(3))
    scale = torch.tensor([0.0, 2.0, 1.0])
    y64 = torch.relu(scale.double().view(3, 1) * z.double() + res.double())
    y32 = torch.relu(scale.view(3, 1) * z.float() + res.float())
    outputs, checks, priors, finite_as = {"y": ((3, row), dtype)}, {}, {}, {}
    if bf:
        checks["y"] = _bf16_ulp_check(y32)
    else:
        checks["y"] = gb.all_checks(gb.rel_check(y64, 1e-6), gb.bits_check(torch.relu(res), torch.arange(3).view(3, 1).expand(3, row) == 0))
        outputs["cell"], priors["cell"], finite_as["cell"] = ((1,), I32), torch.zeros(1, dtype=I32), F32
    spec = gb.Spec("droppath forward %s row%d" % (dtype, row), {"z": z, "res": res, "scale": scale}, outputs, checks, priors=priors,
                   finite_as=finite_as)
    cells = []

    def impl(v):
        _l.check(lib.cstp_droppath_add_relu_forward(_stream(), v["z"].data_ptr(), v["res"].data_ptr(), v["scale"].data_ptr(),
                                                    v["y"].data_ptr(), 3 * row, row, bf, _ptr(v, "cell")), "cstp_droppath_add_relu_forward")
        if not bf:
            torch.cuda.synchronize()
            cells.append((int(v["cell"].item()), int(v["y"].abs().max().view(I32).item())))
    _run3(spec, impl)
    assert all(a == b for a, b in cells), cells
    y = y64.to(dtype)
    mask = y.float() > 0
    dres = torch.where(mask, dy, torch.zeros_like(dy))
    dz32 = scale.view(3, 1) * dres.float()
    for want_dz, want_dres in ((False, True), (True, False), (True, True)):
        outputs, checks = {}, {}
        if want_dz:
            outputs["dz"] = ((3, row), dtype)
            checks["dz"] = _bf16_ulp_check(dz32) if bf else gb.rel_check(scale.double().view(3, 1) * dres.double(), 1e-6)
        if want_dres:
            outputs["dres"], checks["dres"] = ((3, row), dtype), gb.bits_check(dres)
        spec = gb.Spec("droppath backward %s row%d dz%d dres%d" % (dtype, row, want_dz, want_dres), {"y": y, "dy": dy, "scale": scale},
                       outputs, checks)
        _run3(spec, lambda v: _l.check(lib.cstp_droppath_add_relu_backward(_stream(), v["y"].data_ptr(), v["dy"].data_ptr(),
                                                                           v["scale"].data_ptr(), _ptr(v, "dz"), _ptr(v, "dres"),
                                                                           3 * row, row, bf), "cstp_droppath_add_relu_backward"))


@pytest.mark.parametrize("n", [1, 3, 4, 1027])
def test_b16_cast(n):
    """Round to nearest even, bit for bit (test_b16_gpu.py test_cast_bf16_is_round_to_nearest_even)."""
    _l, lib = _libs()
    x = (_rand((n,), 80 + n) * 100).float()
    x[0] = 1.00390625                                     # a tie: to even
    spec = gb.Spec("b16_cast n%d" % n, {"x": x}, {"y": ((n,), B16)}, {"y": gb.bits_check(x.to(B16))})
    _run3(spec, lambda v: _l.check(lib.cstp_b16_cast(_stream(), v["x"].data_ptr(), v["y"].data_ptr(), n), "cstp_b16_cast"))


def _mix_table(_l, entries):
    arr = (_l.ClipMixEntry * len(entries))()
    for e, (partner, mode, lam, y0, y1, x0, x1) in zip(arr, entries):
        e.partner, e.mode, e.lam, e.y0, e.y1, e.x0, e.x1 = partner, mode, lam, y0, y1, x0, x1
    return torch.frombuffer(bytearray(bytes(arr)), dtype=U8).clone()


MIX_TABLES = {
    # (partner, mode, lam, y0, y1, x0, x1) per sample; b = 3
    "modes": [(1, 2, 0.5, 0, 2, 0, 3),          # CutMix, a box touching two edges
              (0, 1, 0.3, 0, 0, 0, 0),          # mixup
              (0, 0, 0.3, 0, 3, 0, 3)],         # copy (mode 0 ignores the rest)
    "edges": [(2, 2, 0.5, 1, 1, 2, 2),          # CutMix with an empty box: a copy
              (1, 1, 0.3, 0, 0, 0, 0),          # its own partner: a copy, bit for bit
              (3, 1, 0.3, 0, 3, 0, 3)],         # partner = b: served as mode 0; followed, it would read the guard behind x
}


@pytest.mark.parametrize("table", list(MIX_TABLES))
@pytest.mark.parametrize("w", [5, 8])
def test_clip_mix(w, table):
    """b = 3, planes = 2, h = 3; w = 8 takes the 16-byte bodies.  Copies and CutMix are bit copies, mixup 1e-6 (test_mix_gpu.py)."""
    _l, lib = _libs()
    b, planes, h = 3, 2, 3
    x = _rand((b, planes, h, w), 90 + w).float()
    want = x.double().clone()
    exact = torch.ones(b, dtype=torch.bool)
    for i, (partner, mode, lam, y0, y1, x0, x1) in enumerate(MIX_TABLES[table]):
        if partner == i or not 0 <= partner < b:
            continue
        if mode == 1:
            want[i] = f32(lam) * x[i].double() + (1.0 - f32(lam)) * x[partner].double()
            exact[i] = False
        elif mode == 2:
            want[i, :, y0:y1, x0:x1] = x[partner, :, y0:y1, x0:x1].double()
    emask = exact.view(b, 1, 1, 1).expand(x.shape)

    def blend_check(got):
        for i in range(b):
            if not exact[i]:
                gb.rel_check(want[i], 1e-6)(got[i])
    spec = gb.Spec("clip_mix w%d %s" % (w, table), {"x": x, "table": _mix_table(_l, MIX_TABLES[table])}, {"y": (tuple(x.shape), F32)},
                   {"y": gb.all_checks(blend_check, gb.bits_check(want.float(), emask))})
    _run3(spec, lambda v: _l.check(lib.cstp_clip_mix(_stream(), v["x"].data_ptr(), v["y"].data_ptr(), v["table"].data_ptr(), b, planes,
                                                     h, w), "cstp_clip_mix"))

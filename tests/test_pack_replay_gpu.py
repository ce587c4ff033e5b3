"""The weight-pack replay (cstp_pack_record / cstp_pack_replay / cstp_pack_register, include/cstp_hip.h) when a call on a
REGISTERED workspace does not run the kernel variant that was recorded there: a misaligned operand (the patch kernels hand
over to the f16-pair gather kernel), an absmax cell missing (a fused input transform falls back to a native tile), a tile or
the arithmetic changed through the C ABI behind the host's back, another weight tensor.  The replayed pack then has another
layout than the one the call needs; the call must pack for itself rather than skip.  Every case follows the same steps:
record the aligned call, scrub the workspace with 0xFF bytes, replay the records, register their workspace, make the call
under the condition -- and its result must equal both PyTorch fp64 (1e-4) and the same call on a workspace of its own, bit
for bit.  The control shows that a matching call still skips.  Everything a test changes in the library's process-wide state
(tile entries, arithmetic, registrations) is put back in ``finally``; the 0xFF scrub stays inside allocated workspaces."""
import contextlib
import ctypes

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4
B16_TOL = 2.0 ** -8          # bf16 outputs: rounded to 8 significant bits
DEV = "cuda"

# the pack-replay geometries of test_model_gpu.py::test_pack_replay_writes_what_the_call_packs
TPATCH = ((2, 48, 8, 14, 14), 64, (3, 1, 1), (1, 0, 0))     # temporal patch kernel; misaligned: f16-pair gather Tile{9,1,0,1,1}
PATCH = ((2, 32, 4, 14, 14), 48, (1, 3, 3), (0, 1, 1))      # LDS-patch kernels
SPLIT = ((2, 24, 2, 7, 7), 40, (1, 3, 3), (0, 1, 1))        # f16-pair gather kernels
NATIVE = ((2, 24, 2, 7, 7), 40, (1, 1, 1), (0, 0, 0))       # native f32 tiles
SPLIT_AFF = ((2, 48, 8, 16, 16), 64, (3, 1, 1), (1, 0, 0))  # fused input transform on the f16-pair kernel (positions % 128 == 0)


def _lib():
    from cstp_amd import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _on_device(t, offset=0, dtype=None):
    """``t`` on the GPU at a storage offset of ``offset`` elements (fp32 1: 4 bytes past a 16-byte boundary)."""
    dtype = dtype or t.dtype
    buf = torch.zeros(t.numel() + 8, dtype=dtype, device=DEV)
    v = buf[offset:offset + t.numel()].view(t.shape)
    v.copy_(t.to(dtype))
    assert (v.data_ptr() % 16 == 0) == (offset == 0)
    return v


def _record(call):
    _l, lib = _lib()
    lib.cstp_pack_mode(1)
    try:
        call()
    finally:
        lib.cstp_pack_mode(0)
    n = lib.cstp_pack_recorded(None, 0)
    recs = (_l.PackRec * max(n, 1))()
    assert lib.cstp_pack_recorded(recs, n) == n
    assert n >= 1, "the recorded call packed nothing"
    return [recs[i] for i in range(n)]


def _replay(recs, ws):
    """Scrub ``ws`` (NaN patterns wherever the replay does not write), then run the records from one launch."""
    _l, lib = _lib()
    ws.fill_(0xFF)
    arr = (_l.PackRec * len(recs))(*recs)
    first, tot = [], 0
    for r in recs:
        first.append(tot)
        tot += int(r.nblocks)
    recs_dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).clone().to(DEV)
    first_dev = torch.tensor(first, dtype=torch.int32, device=DEV)
    _l.check(lib.cstp_pack_replay(_stream(), recs_dev.data_ptr(), first_dev.data_ptr(), len(recs), tot), "cstp_pack_replay")
    torch.cuda.synchronize()          # (the tables die with this frame)


@contextlib.contextmanager
def _registered(recs):
    """Register the records' workspaces; unregister exactly these afterwards (another live plan may own others)."""
    _l, lib = _lib()
    dsts = sorted({int(r.dst) for r in recs})
    arr = (ctypes.c_void_p * len(dsts))(*dsts)
    _l.check(lib.cstp_pack_register(arr, len(dsts), 1), "cstp_pack_register")
    try:
        yield
    finally:
        torch.cuda.synchronize()
        lib.cstp_pack_register(arr, len(dsts), 0)


@contextlib.contextmanager
def _tile_restored(desc, mode):
    """Put the tile entry of (desc, mode) back as it was (cstp_conv3d_get_tile) when the block ends."""
    _l, lib = _lib()
    old = (ctypes.c_int32 * 4)()
    _l.check(lib.cstp_conv3d_get_tile(ctypes.byref(desc), mode, old), "cstp_conv3d_get_tile")
    try:
        yield
    finally:
        if old[0] >= 0:
            lib.cstp_conv3d_set_tile(ctypes.byref(desc), mode, old)


@contextlib.contextmanager
def _split_terms_restored():
    _l, lib = _lib()
    try:
        yield
    finally:
        lib.cstp_gemm_set_split_terms(0)


def _set_tile(desc, mode, tile):
    _l, lib = _lib()
    _l.check(lib.cstp_conv3d_set_tile(ctypes.byref(desc), mode, (ctypes.c_int32 * 4)(*tile)), "cstp_conv3d_set_tile")


class Conv:
    """One fp32 convolution (stride 1) through the raw C ABI, with its fp64 reference."""

    def __init__(self, geom, tile_f=None, tile_d=None, seed=4):
        from cstp_amd import ops
        self.xs, self.k, self.ks, self.pad = geom
        self.wshape = (self.k, self.xs[1]) + self.ks
        if tile_f is not None:
            ops.set_conv_tile(self.xs, self.wshape, 1, self.pad, 0, tile_f)
        if tile_d is not None:
            ops.set_conv_tile(self.xs, self.wshape, 1, self.pad, 1, tile_d)
        self.desc = ops._desc(self.xs, self.wshape, (1, 1, 1), self.pad)
        self.ys = ops.conv_out_shape(self.xs, self.wshape, (1, 1, 1), self.pad)
        g = torch.Generator().manual_seed(seed)
        self.x = torch.randn(self.xs, generator=g) + 0.1
        self.w = torch.randn(self.wshape, generator=g) * 0.1
        self.w2 = torch.randn(self.wshape, generator=g) * 0.1
        self.dy = torch.randn(self.ys, generator=g)
        _l, lib = _lib()
        self.nbytes = lib.cstp_conv3d_workspace_bytes(ctypes.byref(self.desc))
        assert self.nbytes > 0

    def ws(self):
        return torch.zeros(self.nbytes, dtype=torch.uint8, device=DEV)

    def fwd(self, x, w, y, ws, aff=None, absmax=None):
        _l, lib = _lib()
        _l.check(lib.cstp_conv3d_forward_am(_stream(), ctypes.byref(self.desc), x.data_ptr(), w.data_ptr(), None,
                                            None if aff is None else ctypes.byref(aff), y.data_ptr(), ws.data_ptr(), ws.numel(),
                                            None if absmax is None else absmax.data_ptr()), "cstp_conv3d_forward")

    def dgrad(self, dy, w, dx, ws):
        _l, lib = _lib()
        _l.check(lib.cstp_conv3d_backward_data_am(_stream(), ctypes.byref(self.desc), dy.data_ptr(), w.data_ptr(), dx.data_ptr(),
                                                  ws.data_ptr(), ws.numel(), None), "cstp_conv3d_backward_data")

    def ref_fwd(self, w=None, x=None):
        x = self.x if x is None else x
        return F.conv3d(x.double(), (self.w if w is None else w).double(), None, 1, self.pad)

    def ref_dgrad(self, w=None):
        return torch.nn.grad.conv3d_input(self.xs, (self.w if w is None else w).double(), self.dy.double(), 1, self.pad)


def _check(out, call, record, ws, ref64, tol=TOL, what=""):
    """record() = the recorded call on ``ws``; call(ws) = the call under the condition, writing ``out``.  The condition's result
    after the replay into the registered ``ws`` must equal fp64 and the same call on a workspace of its own, bit for bit."""
    own = torch.zeros_like(ws)
    call(own)
    torch.cuda.synchronize()
    want = out.clone()
    recs = _record(record)
    _replay(recs, ws)
    with _registered(recs):
        out.zero_()
        call(ws)
    got = out.clone()
    err = rel_err(got, ref64)
    assert err < tol, "%s: %.3e against fp64 (recorded kinds %s)" % (what, err, [int(r.kind) for r in recs])
    assert torch.equal(got, want), "%s: differs from the call that packs for itself" % what


# ---- C1: an operand at a 4-byte offset: the temporal patch pack (kind 2) was recorded, the gather kernel wants kind 1

@pytest.mark.parametrize("which", ["x", "y"])
def test_misaligned_forward_operand_does_not_read_the_patch_pack(which):
    c = Conv(TPATCH, tile_f=(2, 4, 0, 0))
    x, w, y = _on_device(c.x), _on_device(c.w), _on_device(torch.zeros(c.ys))
    xm = _on_device(c.x, 1 if which == "x" else 0)
    ym = _on_device(torch.zeros(c.ys), 1 if which == "y" else 0)
    ws = c.ws()
    _check(ym, lambda s: c.fwd(xm, w, ym, s), lambda: c.fwd(x, w, y, ws), ws, c.ref_fwd(), what="forward, misaligned " + which)


@pytest.mark.parametrize("which", ["dy", "dx"])
def test_misaligned_data_gradient_operand_does_not_read_the_patch_pack(which):
    c = Conv(TPATCH, tile_d=(2, 4, 0, 0))
    dy, w, dx = _on_device(c.dy), _on_device(c.w), _on_device(torch.zeros(c.xs))
    dym = _on_device(c.dy, 1 if which == "dy" else 0)
    dxm = _on_device(torch.zeros(c.xs), 1 if which == "dx" else 0)
    ws = c.ws()
    _check(dxm, lambda s: c.dgrad(dym, w, dxm, s), lambda: c.dgrad(dy, w, dx, ws), ws, c.ref_dgrad(),
           what="data gradient, misaligned " + which)


# ---- C2: a fused input transform with its absmax cell at the recording, without it at the call (native tile: kind 3)

@pytest.mark.parametrize("geom,tile", [(TPATCH, (2, 4, 0, 0)), (SPLIT_AFF, (1, 4, 0, 0))], ids=["temporal patch", "f16-pair"])
def test_in_affine_call_without_absmax_cell_does_not_read_the_fused_pack(geom, tile):
    from cstp_amd import _lib as L
    c = Conv(geom, tile_f=tile)
    g = torch.Generator().manual_seed(9)
    cin = c.xs[1]
    scale = torch.rand(cin, generator=g) * 1.5 - 0.25
    shift = torch.randn(cin, generator=g) * 0.5
    z64 = torch.relu(c.x.double() * scale.double().view(1, -1, 1, 1, 1) + shift.double().view(1, -1, 1, 1, 1))
    ref = F.conv3d(z64, c.w.double(), None, 1, c.pad)
    zmax = float(z64.abs().max()) * 1.01               # an upper bound of the transformed operand is all the kernels need
    cell = torch.tensor([zmax], dtype=torch.float32).view(torch.int32).to(DEV)
    ss = torch.stack([scale, shift], 1).reshape(-1).to(DEV)
    aff = L.InAffine(ss.data_ptr(), 1, 1)
    x, w, y = _on_device(c.x), _on_device(c.w), _on_device(torch.zeros(c.ys))
    ws = c.ws()
    _check(y, lambda s: c.fwd(x, w, y, s, aff, None), lambda: c.fwd(x, w, y, ws, aff, cell), ws, ref,
           what="in_affine forward, absmax cell dropped")


# ---- C3: the tile entry changed through the raw C ABI after the recording (no host invalidate)

C3_CASES = [
    ("split 4 -> 8 row tiles", SPLIT, (1, 4, 0, 0), (1, 8, 0, 0)),
    ("patch 64 -> 128 rows", PATCH, (2, 4, 0, 0), (2, 8, 0, 0)),
    ("native 64 -> 144 rows", NATIVE, (0, 2, 1, 1), (0, 9, 1, 1)),
    ("split -> native", SPLIT, (1, 4, 0, 0), (0, 2, 1, 1)),
]


@pytest.mark.parametrize("mode", [0, 1], ids=["forward", "data gradient"])
@pytest.mark.parametrize("name,geom,before,after", C3_CASES, ids=[c[0] for c in C3_CASES])
def test_tile_changed_behind_the_host_repacks(name, geom, before, after, mode):
    c = Conv(geom, **({"tile_f": before} if mode == 0 else {"tile_d": before}))
    w = _on_device(c.w)
    ws = c.ws()
    if mode == 0:
        x, out = _on_device(c.x), _on_device(torch.zeros(c.ys))
        run, ref = (lambda s: c.fwd(x, w, out, s)), c.ref_fwd()
    else:
        dy, out = _on_device(c.dy), _on_device(torch.zeros(c.xs))
        run, ref = (lambda s: c.dgrad(dy, w, out, s)), c.ref_dgrad()
    _l, lib = _lib()
    with _tile_restored(c.desc, mode):
        recs = _record(lambda: run(ws))
        _set_tile(c.desc, mode, after)
        own = torch.zeros_like(ws)
        run(own)
        torch.cuda.synchronize()
        want = out.clone()
        _replay(recs, ws)
        with _registered(recs):
            out.zero_()
            run(ws)
        got = out.clone()
    assert rel_err(got, ref) < TOL, (name, mode, rel_err(got, ref))
    assert torch.equal(got, want), (name, mode)


# ---- C4: the arithmetic switched through the raw C ABI after the recording

@pytest.mark.parametrize("terms", [1, 3], ids=["f32 native", "bf16 triple"])
@pytest.mark.parametrize("geom,tile", [(SPLIT, (1, 4, 0, 0)), (PATCH, (2, 4, 0, 0))], ids=["split", "patch"])
def test_arithmetic_switched_behind_the_host_repacks(geom, tile, terms):
    c = Conv(geom, tile_f=tile)
    x, w, y = _on_device(c.x), _on_device(c.w), _on_device(torch.zeros(c.ys))
    ws = c.ws()
    _l, lib = _lib()
    with _split_terms_restored():
        lib.cstp_gemm_set_split_terms(2)
        recs = _record(lambda: c.fwd(x, w, y, ws))
        _l.check(lib.cstp_gemm_set_split_terms(terms), "cstp_gemm_set_split_terms")
        own = torch.zeros_like(ws)
        c.fwd(x, w, y, own)
        torch.cuda.synchronize()
        want = y.clone()
        _replay(recs, ws)
        with _registered(recs):
            y.zero_()
            c.fwd(x, w, y, ws)
        got = y.clone()
    assert rel_err(got, c.ref_fwd()) < TOL, rel_err(got, c.ref_fwd())
    assert torch.equal(got, want)


# ---- C5: another weight tensor on the registered workspace

@pytest.mark.parametrize("geom,tile", [(TPATCH, (2, 4, 0, 0)), (SPLIT, (1, 4, 0, 0)), (NATIVE, (0, 2, 1, 1))],
                         ids=["temporal patch", "split", "native"])
def test_other_weight_tensor_on_a_registered_workspace_repacks(geom, tile):
    c = Conv(geom, tile_f=tile)
    x, w, w2, y = _on_device(c.x), _on_device(c.w), _on_device(c.w2), _on_device(torch.zeros(c.ys))
    ws = c.ws()
    _check(y, lambda s: c.fwd(x, w2, y, s), lambda: c.fwd(x, w, y, ws), ws, c.ref_fwd(c.w2), what="other weight tensor")


# ---- C6: bf16 storage (record kind 4): the pack depends on the descriptor only, the pointwise forward packs nothing
# (operand offsets of 4 elements: 8 bytes past a 16-byte boundary, what turns the octet / pointwise paths off)

B16_CASES = [
    ("ragged 83 channels", ((2, 83, 4, 16, 16), 64, (3, 1, 1), (1, 0, 0)), 0, 4),
    ("64 channels", ((2, 64, 4, 8, 8), 48, (3, 1, 1), (1, 0, 0)), 0, 4),
    ("pointwise, recorded misaligned", ((2, 64, 4, 8, 8), 32, (1, 1, 1), (0, 0, 0)), 4, 0),
]


@pytest.mark.parametrize("dgrad", [False, True], ids=["forward", "data gradient"])
@pytest.mark.parametrize("name,geom,off_rec,off_call", B16_CASES, ids=[c[0] for c in B16_CASES])
def test_bf16_pack_replays_across_operand_alignment(name, geom, off_rec, off_call, dgrad):
    from cstp_amd import ops
    _l, lib = _lib()
    xs, k, ks, pad = geom
    wshape = (k, xs[1]) + ks
    desc = ops._desc(xs, wshape, (1, 1, 1), pad)
    ys = ops.conv_out_shape(xs, wshape, (1, 1, 1), pad)
    g = torch.Generator().manual_seed(sum(xs) + k)
    x = torch.randn(xs, generator=g).to(torch.bfloat16)
    wf = torch.randn(wshape, generator=g) / (xs[1] * ks[0] * ks[1] * ks[2]) ** 0.5
    dy = torch.randn(ys, generator=g).to(torch.bfloat16)
    w64 = wf.to(torch.bfloat16).double()              # (the kernels round the weights to bf16)
    w = _on_device(wf)
    nbytes = lib.cstp_b16_conv3d_workspace_bytes(ctypes.byref(desc))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    if dgrad:
        src_r, src_c = _on_device(dy, off_rec), _on_device(dy, off_call)
        out_r, out_c = _on_device(torch.zeros(xs), dtype=torch.bfloat16), _on_device(torch.zeros(xs), dtype=torch.bfloat16)
        fn, ref = "cstp_b16_conv3d_backward_data", torch.nn.grad.conv3d_input(xs, w64, dy.double(), 1, pad)
    else:
        src_r, src_c = _on_device(x, off_rec), _on_device(x, off_call)
        out_r, out_c = _on_device(torch.zeros(ys), dtype=torch.bfloat16), _on_device(torch.zeros(ys), dtype=torch.bfloat16)
        fn, ref = "cstp_b16_conv3d_forward", F.conv3d(x.double(), w64, None, 1, pad)

    def run(src, out, s):
        _l.check(getattr(lib, fn)(_stream(), ctypes.byref(desc), src.data_ptr(), w.data_ptr(), out.data_ptr(), s.data_ptr(),
                                  s.numel()), fn)
    _check(out_c, lambda s: run(src_c, out_c, s), lambda: run(src_r, out_r, ws), ws, ref, tol=B16_TOL, what=name)


# ---- the control: a matching call on the registered workspace still skips its pack

@pytest.mark.parametrize("geom,tile", [(TPATCH, (2, 4, 0, 0)), (SPLIT, (1, 4, 0, 0)), (NATIVE, (0, 2, 1, 1))],
                         ids=["temporal patch", "split", "native"])
def test_matching_call_still_skips_its_pack(geom, tile):
    """After the replay the weights are overwritten IN PLACE (same pointer): a call that skips its pack computes with the
    replayed, old weights."""
    c = Conv(geom, tile_f=tile)
    x, w, y = _on_device(c.x), _on_device(c.w), _on_device(torch.zeros(c.ys))
    ws = c.ws()
    recs = _record(lambda: c.fwd(x, w, y, ws))
    torch.cuda.synchronize()
    want = y.clone()
    _replay(recs, ws)
    w.copy_(c.w2.to(DEV))
    with _registered(recs):
        y.zero_()
        c.fwd(x, w, y, ws)
    assert torch.equal(y, want)
    assert rel_err(y, c.ref_fwd(c.w)) < TOL


def test_mismatch_then_match_then_new_replay():
    """One registered workspace: a mismatching call (misaligned x), a matching call, a new replay and a matching call -- each
    correct, whatever the call before left in the buffer."""
    c = Conv(TPATCH, tile_f=(2, 4, 0, 0))
    x, w, y = _on_device(c.x), _on_device(c.w), _on_device(torch.zeros(c.ys))
    xm = _on_device(c.x, 1)
    ref = c.ref_fwd()
    ws = c.ws()
    recs = _record(lambda: c.fwd(x, w, y, ws))
    torch.cuda.synchronize()
    want = y.clone()
    _replay(recs, ws)
    with _registered(recs):
        for step, xin in (("mismatching", xm), ("matching", x)):
            y.zero_()
            c.fwd(xin, w, y, ws)
            torch.cuda.synchronize()
            assert rel_err(y, ref) < TOL, step
        _replay(recs, ws)
    with _registered(recs):
        y.zero_()
        c.fwd(x, w, y, ws)
    assert torch.equal(y, want)


# ---- through ops: PackPlan's key tells a misaligned call from the recorded one

def test_pack_plan_misaligned_view_gets_its_own_workspace():
    """A PackPlan armed by hand as train.PretrainStep arms it: one aligned forward + backward records, the tables replay, then
    the same layer runs on a misaligned view (ops._req keeps its storage offset) holding the same values."""
    from cstp_amd import ops
    c = Conv(TPATCH, tile_f=(2, 4, 0, 0), tile_d=(2, 4, 0, 0))
    ops.set_conv_tile(c.xs, c.wshape, 1, c.pad, 2, (1, 4, 8, 0))
    x64 = c.x.double().requires_grad_(True)
    w64 = c.w.double().requires_grad_(True)
    y64 = F.conv3d(x64, w64, None, 1, c.pad)
    dx64, dw64 = torch.autograd.grad(y64, (x64, w64), c.dy.double())
    w = c.w.to(DEV).requires_grad_(True)
    dy = c.dy.to(DEV)
    plan = ops.PackPlan()
    try:
        ops.pack_plan = plan
        plan.state, plan.armed = "record", True
        xa = _on_device(c.x).requires_grad_(True)
        ya = ops.conv3d(xa, w, None, 1, c.pad)
        ya.backward(dy)
        ops._join_side_streams()
        plan.finish_record(torch.device(DEV))
        assert plan.state == "replay" and plan.stats["recorded_calls"] == 2
        plan.replay("online")
        plan.replay("online_d")
        w.grad = None
        xm = _on_device(c.x, 1).detach().requires_grad_(True)
        ym = ops.conv3d(xm, w, None, 1, c.pad)
        ym.backward(dy)
        ops._join_side_streams()
        torch.cuda.synchronize()
        assert rel_err(ym, y64) < TOL, rel_err(ym, y64)
        assert rel_err(xm.grad, dx64) < TOL, rel_err(xm.grad, dx64)
        assert rel_err(w.grad, dw64) < TOL, rel_err(w.grad, dw64)
        assert plan.stats["skipped_calls"] >= 1          # (the data gradient's operands are aligned: that pack is skipped)
    finally:
        plan.armed = False
        plan.invalidate()
        ops.pack_plan = None


# ---- model level: a tile changed through the raw C ABI while the plan replays

def test_pack_plan_steps_survive_a_tile_changed_behind_the_host(monkeypatch):
    """test_model_gpu.py::test_pack_plan_steps_match_steps_that_pack_inside_every_call with one layer's forward tile switched
    through raw cstp_conv3d_set_tile (bypassing ops.set_conv_tile's invalidate) once the plan replays (after step 4): the
    7-step trajectory must match a plan-off run that makes the same switch at the same step."""
    from cstp_amd import ops
    from cstp_amd.optim import FlatSGD
    from cstp_amd.synthetic import device_batch
    from cstp_amd.train import PretrainStep
    from test_model_gpu import build_model, trel
    _l, lib = _lib()
    seen = []
    real_desc = ops._desc

    def spy(x_shape, w_shape, stride, padding):
        seen.append((tuple(x_shape), tuple(w_shape), tuple(stride), tuple(padding)))
        return real_desc(x_shape, w_shape, stride, padding)
    monkeypatch.setattr(ops, "_desc", spy)
    ops.set_deterministic(True)
    target = None
    try:
        dev = torch.device("cuda", 0)
        x1, x2, lab = device_batch(2, 8, 56, dev, seed=3)
        finals = []
        for plan_on in ("1", "0"):
            monkeypatch.setenv("CSTP_PACK_PLAN", plan_on)
            torch.manual_seed(5)
            model = build_model((1, 1, 1, 1))
            opt = FlatSGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4, arenas=model._arenas)
            step = PretrainStep(model, opt, (0.1, 1.0, 1.0, 1.0, 1.0), clip_grad_norm=True)
            losses = []
            for i in range(7):
                if i == 4:
                    if target is None:
                        # a temporal layer whose forward runs a split / patch kernel: switched to a native tile (another pack kind)
                        for xs, wsh, st, pd in seen:
                            if wsh[2:] != (3, 1, 1) or st != (1, 1, 1) or pd != (1, 0, 0):
                                continue
                            d = real_desc(xs, wsh, st, pd)
                            q = (ctypes.c_int32 * 4)()
                            if lib.cstp_conv3d_query_tile(ctypes.byref(d), 0, q) == 0 and q[2] != 0:
                                target = d
                                break
                        assert target is not None, "no split / patch forward layer found"
                        old = (ctypes.c_int32 * 4)()
                        _l.check(lib.cstp_conv3d_get_tile(ctypes.byref(target), 0, old), "cstp_conv3d_get_tile")
                        old = list(old)
                    _set_tile(target, 0, (0, 2, 1, 1))
                    skipped = step._packs.stats["skipped_calls"] if step._packs is not None else 0
                    if plan_on == "1":
                        assert step._packs.state == "replay"
                out = step(x1, x2, lab["spa"], lab["tem"], lab["pb"], lab["rot1"], lab["rot2"])
                losses.append(float(out.loss_total))
            torch.cuda.synchronize()
            if old[0] >= 0:
                _set_tile(target, 0, old)
            if plan_on == "1":
                assert step._packs.state == "replay" and step._packs.stats["skipped_calls"] > skipped, step._packs.stats
            assert all(l == l and abs(l) < float("inf") for l in losses), losses
            finals.append((losses, {k: v.clone() for k, v in model.state_dict().items()}))
        (la, sa), (lb, sb) = finals
        assert max(abs(a - b) / abs(b) for a, b in zip(la, lb)) < 1e-5, list(zip(la, lb))
        for k in sa:
            if sa[k].dtype.is_floating_point:
                assert bool(torch.isfinite(sa[k]).all()), k
                assert trel(sa[k], sb[k]) < 1e-3, k
            else:
                assert torch.equal(sa[k], sb[k]), k
    finally:
        ops.set_deterministic(False)
        ops.pack_plan = None

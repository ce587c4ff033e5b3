"""The convolution and BatchNorm kernels between poisoned guard bands (tests/guard_bands.py; DESIGN.md, "What a call may
touch").  Every case makes one raw C-ABI call three times -- operands between zero guards, again, then between NaN guards, the
workspace 0xFF inside and out every time -- and holds it to: success on the pinned route (cstp_conv3d_query_tile), finite
outputs within the route's existing bar of PyTorch CPU fp64 (1e-4 for fp32, BASELINE.json; the bars of test_b16_gpu.py /
test_r21d_b16_gpu.py for bf16 storage), every guard intact and every input unchanged, and results that do not depend on what
surrounds the operands.  The geometries are the smallest ragged ones the parity tests already name.  Everything a case changes
in the library's process-wide state (tile entries, arithmetic, deterministic mode) is put back in ``finally``."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guard_bands as gb

pytestmark = pytest.mark.gpu

TOL = 1e-4
DEV = "cuda"
F32, B16, I32, F64 = torch.float32, torch.bfloat16, torch.int32, torch.float64

# name: (x shape, k, kernel, stride, pad) -- test_split_gpu.py's GEOMS / PATCH_GEOMS / STEMS, test_tpatch_gpu.py's tables
GEOMS = {
    "odd": ((3, 40, 3, 9, 11), 136, (3, 3, 3), (1, 2, 1), (1, 1, 1)),           # ragged everything; 40 channels = 2.5 groups of 16
    "lin": ((6, 96, 1, 1, 1), 40, (1, 1, 1), (1, 1, 1), (0, 0, 0)),
    "single": ((1, 6, 1, 1, 1), 9, (1, 1, 1), (1, 1, 1), (0, 0, 0)),            # a single position
    "T2s": ((2, 230, 8, 7, 7), 128, (3, 1, 1), (2, 1, 1), (1, 0, 0)),           # 230 channels: padded group on the last sample; parity classes
    "short": ((2, 64, 4, 14, 14), 42, (1, 1, 1), (1, 2, 2), (0, 0, 0)),         # 42 output channels: the data gradient's padded group
    "s2odd": ((2, 16, 3, 7, 7), 20, (1, 3, 3), (1, 2, 2), (0, 1, 1)),           # stride 2 on odd H / W
    "stem21": ((3, 3, 3, 23, 19), 83, (1, 7, 7), (1, 2, 2), (0, 3, 3)),
    "stem3d": ((1, 3, 6, 20, 20), 64, (7, 7, 7), (1, 2, 2), (3, 3, 3)),
    "p_ragged": ((3, 40, 3, 9, 11), 136, (1, 3, 3), (1, 1, 1), (0, 1, 1)),      # "past the end read row 0"; last channel block 8 of 32
    "p_thin": ((2, 16, 1, 5, 6), 24, (1, 3, 3), (1, 1, 1), (0, 1, 1)),          # half a channel block
    "p_wide": ((1, 32, 3, 6, 120), 48, (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    "p_stats": ((4, 16, 2, 28, 28), 136, (1, 3, 3), (1, 1, 1), (0, 1, 1)),      # 136 rows in a 144-row block: padded rows leave no sums
    "t_ragged": ((2, 48, 8, 14, 14), 80, (3, 1, 1), (1, 1, 1), (1, 0, 0)),      # halo frames; half-empty channel block
    "t_48rows": ((1, 96, 8, 14, 28), 48, (3, 1, 1), (1, 1, 1), (1, 0, 0)),      # fewer rows than the block
    "w_2col": ((2, 48, 4, 8, 8), 80, (3, 1, 1), (1, 1, 1), (1, 0, 0)),
    "w_2row": ((1, 160, 4, 8, 4), 32, (3, 1, 1), (1, 1, 1), (1, 0, 0)),
    "w_83": ((2, 83, 4, 8, 8), 64, (3, 1, 1), (1, 1, 1), (1, 0, 0)),            # the ragged 4-channel piece
    "w_16pos": ((2, 48, 8, 4, 12), 64, (3, 1, 1), (1, 1, 1), (1, 0, 0)),        # 16-position chunks
    "aff_split": ((2, 48, 8, 16, 16), 64, (3, 1, 1), (1, 1, 1), (1, 0, 0)),     # positions % 128 == 0: the transform inside igemm_k1s
    "aff_tpatch": ((2, 48, 8, 14, 14), 64, (3, 1, 1), (1, 1, 1), (1, 0, 0)),    # 14 x 14 frames: the temporal patch kernel's tiles
    "aff_native": ((2, 40, 3, 9, 11), 24, (3, 1, 1), (1, 1, 1), (1, 0, 0)),     # c % 16 != 0: the host declines, a native kernel applies it
    "lin64": ((6, 192, 1, 1, 1), 128, (1, 1, 1), (1, 1, 1), (0, 0, 0)),         # csrc/linear.h, all three directions
    "lin5": ((4, 1024, 1, 1, 1), 5, (1, 1, 1), (1, 1, 1), (0, 0, 0)),           # short fout
}


def _libs():
    from cstp_amd import _lib, ops
    return _lib, _lib.load(), ops


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(v, name):
    t = v.get(name)
    return None if t is None else t.data_ptr()


def _rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=F64) * 2 - 1


def _run3(spec, impl):
    found = gb.three_runs(spec, impl, DEV, torch.cuda.synchronize)
    assert found == [], "\n".join(found)


def _run1(spec, impl):
    found = gb.single_run(spec, impl, DEV, torch.cuda.synchronize)
    assert found == [], "\n".join(found)


# ---- the harness on device memory ------------------------------------------------------------------------------------------

def test_harness_rejects_sloppy_device_code():
    """tests/test_guard_bands_host.py's sloppy variants as plain torch code on the GPU: the fills reach device memory and the
    comparisons read it back (every access stays inside the test's own allocations)."""
    x = _rand((1000,), 5).float()

    def spec():
        return gb.Spec("device", {"x": x}, {"y": ((1000,), F32)}, {"y": gb.rel_check(x.double() * 2, TOL)}, ws_bytes=4000)

    def good(v):
        v["y"].copy_(v["x"] * 2)

    def store(v):
        good(v)
        v["y"].as_strided((1001,), (1,))[-1] = 1.0

    def read(v):
        good(v)
        v["y"][-1] += 0.0 * v["x"].as_strided((1001,), (1,))[-1]

    def scratch(v):
        w = v["ws"].view(F32)[:1000]
        w.add_(v["x"] * 2)
        v["y"].copy_(w)

    def touch(v):
        good(v)
        v["x"][17] += 1.0
    run = lambda impl: gb.three_runs(spec(), impl, DEV, torch.cuda.synchronize)      # noqa: E731
    assert run(good) == []
    found = run(store)
    assert len(found) == 3 and all("wrote 1 element past the end of y" in f for f in found), found
    found = run(read)
    assert len(found) == 1 and "[nan]" in found[0] and "non-finite output: 1 element of y" in found[0], found
    assert all("non-finite output: 1000 elements of y" in f for f in run(scratch))
    assert all("changed 1 element of the input x (first: element 17 of 1000)" in f for f in run(touch))


# ---- fp32 convolutions -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _conv_ref(name, bias=False):
    """Operands (fp32, test_split_gpu.py's _run) and the fp64 results of one geometry, computed once and shared."""
    xs, k, ks, st, pd = GEOMS[name]
    x = _rand(xs, 1).float()
    w = (_rand((k, xs[1]) + ks, 2) * 0.2).float()
    b = _rand((k,), 4).float() if bias else None
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = F.conv3d(x64, w64, None if b is None else b.double(), st, pd)
    dy = _rand(y.shape, 3).float()
    dx, dw = torch.autograd.grad(y, (x64, w64), dy.double())
    return {"x": x, "w": w, "bias": b, "dy": dy, "y": y.detach(), "dx": dx, "dw": dw, "db": dy.double().sum(dim=(0, 2, 3, 4))}


class Conv:
    def __init__(self, name):
        _l, lib, ops = _libs()
        self.name = name
        self.xs, self.k, self.ks, self.st, self.pd = GEOMS[name]
        self.wshape = (self.k, self.xs[1]) + self.ks
        self.desc = ops._desc(self.xs, self.wshape, self.st, self.pd)
        self.ys = ops.conv_out_shape(self.xs, self.wshape, self.st, self.pd)

    def ws_bytes(self):
        _l, lib, ops = _libs()
        return lib.cstp_conv3d_workspace_bytes(ctypes.byref(self.desc))

    def query(self, mode):
        _l, lib, ops = _libs()
        out = (ctypes.c_int32 * 4)()
        _l.check(lib.cstp_conv3d_query_tile(ctypes.byref(self.desc), mode, out), "cstp_conv3d_query_tile")
        return list(out)

    def get_tile(self, mode):
        _l, lib, ops = _libs()
        out = (ctypes.c_int32 * 4)()
        _l.check(lib.cstp_conv3d_get_tile(ctypes.byref(self.desc), mode, out), "cstp_conv3d_get_tile")
        return list(out)


def expected_query(conv, mode, tile, terms):
    """What cstp_conv3d_query_tile reports when the pinned tile is what runs (None: not compared)."""
    sp, mt = tile[0], tile[1]
    if mode == 2:
        if sp == 2:
            return [144, 288 if conv.ks == (1, 3, 3) else 192, 2, 0]
        if sp == 1:
            return [16 * mt, 128, terms, tile[2]]
        return [144 if mt == 9 else 32 * mt, 128, 0, tile[2]]
    if sp == 2:
        return [16 * mt, 224, 2, None]
    if sp == 1:
        return [16 * mt, 256 if tile[2] == 2 else 128, terms, None]
    return [144 if mt == 9 else 32 * mt * tile[2], None, 0, tile[3]]


@contextlib.contextmanager
def pinned(conv, terms, tiles, det=False, confirm=True):
    """The arithmetic, the tiles {mode: tile4} and the deterministic mode of one case; all put back when the block ends."""
    _l, lib, ops = _libs()
    ops.set_split_terms(terms)
    old = {}
    try:
        if det:
            ops.set_deterministic(True)
        for mode, tile in tiles.items():
            old[mode] = conv.get_tile(mode)
            ops.set_conv_tile(conv.xs, conv.wshape, conv.st, conv.pd, mode, tile)
            if confirm:          # assertion 1: the pinned route is what runs; a refused tile is a failure
                got = conv.query(mode)
                want = expected_query(conv, mode, tile, terms)
                assert all(w is None or g == w for g, w in zip(got, want)), \
                    "%s mode %d: tile %s pinned, the call would run %s (expected %s)" % (conv.name, mode, tile, got, want)
                assert conv.get_tile(mode)[:2] == [tile[0], tile[1]], (conv.name, mode, tile, conv.get_tile(mode))
        yield
    finally:
        torch.cuda.synchronize()
        for mode, tile in old.items():
            if tile[0] >= 0:
                lib.cstp_conv3d_set_tile(ctypes.byref(conv.desc), mode, (ctypes.c_int32 * 4)(*tile))
        if det:
            ops.set_deterministic(False)
        ops.set_split_terms(0)


def fwd_case(conv, what, bias=False, shifts=None, aff=None):
    """cstp_conv3d_forward_am.  aff: (scale_shift table [groups][c][2] fp32, groups, relu, cell int32 or None, fp64 reference)."""
    _l, lib, ops = _libs()
    r = _conv_ref(conv.name, bias)
    inputs = {"x": r["x"], "w": r["w"]}
    ref = r["y"]
    if bias:
        inputs["bias"] = r["bias"]
    if aff is not None:
        inputs["ss"] = aff[0]
        if aff[3] is not None:
            inputs["cell"] = aff[3]
        ref = aff[4]
    spec = gb.Spec(what, inputs, {"y": (conv.ys, F32)}, {"y": gb.rel_check(ref, TOL)}, ws_bytes=conv.ws_bytes(), shifts=shifts)

    def impl(v):
        a = None if aff is None else ctypes.byref(_l.InAffine(v["ss"].data_ptr(), aff[1], aff[2]))
        _l.check(lib.cstp_conv3d_forward_am(_stream(), ctypes.byref(conv.desc), v["x"].data_ptr(), v["w"].data_ptr(),
                                            _ptr(v, "bias"), a, v["y"].data_ptr(), v["ws"].data_ptr(), spec.ws_bytes,
                                            _ptr(v, "cell")), "cstp_conv3d_forward_am")
    return spec, impl


def dgrad_case(conv, what, shifts=None, accumulate=False):
    _l, lib, ops = _libs()
    r = _conv_ref(conv.name)
    prior = _rand(conv.xs, 44).float() if accumulate else None
    ref = r["dx"] + prior.double() if accumulate else r["dx"]
    spec = gb.Spec(what, {"dy": r["dy"], "w": r["w"]}, {"dx": (conv.xs, F32)}, {"dx": gb.rel_check(ref, TOL)},
                   ws_bytes=conv.ws_bytes(), shifts=shifts, priors={"dx": prior} if accumulate else None)

    def impl(v):
        _l.check(lib.cstp_conv3d_backward_data_acc(_stream(), ctypes.byref(conv.desc), v["dy"].data_ptr(), v["w"].data_ptr(),
                                                   v["dx"].data_ptr(), v["ws"].data_ptr(), spec.ws_bytes, None,
                                                   1 if accumulate else 0), "cstp_conv3d_backward_data_acc")
    return spec, impl


def wgrad_case(conv, what, det, accumulate=False):
    """cstp_conv3d_backward_weight_acc; the workspace is sized when the case is built: after the deterministic switch."""
    _l, lib, ops = _libs()
    r = _conv_ref(conv.name)
    prior = torch.full(conv.wshape, 0.75) if accumulate else None
    ref = r["dw"] + 0.75 if accumulate else r["dw"]
    spec = gb.Spec(what, {"x": r["x"], "dy": r["dy"]}, {"dw": (conv.wshape, F32)}, {"dw": gb.rel_check(ref, TOL)},
                   ws_bytes=conv.ws_bytes(), priors={"dw": prior} if accumulate else None, control_must_hold=det)

    def impl(v):
        _l.check(lib.cstp_conv3d_backward_weight_acc(_stream(), ctypes.byref(conv.desc), v["x"].data_ptr(), None,
                                                     v["dy"].data_ptr(), v["dw"].data_ptr(), v["ws"].data_ptr(), spec.ws_bytes,
                                                     None, None, 1 if accumulate else 0), "cstp_conv3d_backward_weight_acc")
    return spec, impl


def _fwd_dgrad(name, terms, tile, mode):
    conv = Conv(name)
    with pinned(conv, terms, {mode: tile}):
        what = "%s %s tile %s terms %d" % (name, "forward" if mode == 0 else "data gradient", tile, terms)
        _run3(*(fwd_case(conv, what) if mode == 0 else dgrad_case(conv, what)))


def _wgrad(name, terms, tile, confirm=True):
    """Three runs in deterministic mode, held to all four assertions; one default-mode (atomics) run held to 1-3."""
    conv = Conv(name)
    with pinned(conv, terms, {2: tile}, det=True, confirm=confirm):
        _run3(*wgrad_case(conv, "%s weight gradient tile %s terms %d, deterministic" % (name, tile, terms), det=True))
    with pinned(conv, terms, {2: tile}, confirm=confirm):
        _run1(*wgrad_case(conv, "%s weight gradient tile %s terms %d, atomics" % (name, tile, terms), det=False))


MODES = pytest.mark.parametrize("mode", [0, 1], ids=["forward", "dgrad"])
TERMS = pytest.mark.parametrize("terms", [2, 3], ids=["f16x2", "bf16x3"])


@pytest.mark.parametrize("name,tile", [("odd", (0, 1, 1, 1)), ("odd", (1, 4, 0, 0)), ("T2s", (1, 9, 0, 0)), ("p_ragged", (2, 4, 0, 0)),
                                       ("t_ragged", (2, 8, 0, 0))], ids=["native", "igemm_k1s", "parity classes", "spatial patch",
                                                                         "temporal patch"])
def test_accumulating_data_gradient(name, tile):
    """accumulate != 0: dx holds a finite prior, the reference adds it (the residual join's epilogue)."""
    conv = Conv(name)
    with pinned(conv, 2, {1: tile}):
        _run3(*dgrad_case(conv, "%s data gradient tile %s, accumulating" % (name, tile), accumulate=True))


@pytest.mark.parametrize("name,tile", [("odd", (0, 3, 4, 0)), ("odd", (1, 4, 4, 0)), ("p_thin", (2, 9, 1, 0)), ("w_83", (2, 9, 1, 0))],
                         ids=["native", "igemm_k2s", "igemm_k2p", "igemm_k2t"])
def test_accumulating_weight_gradient(name, tile):
    conv = Conv(name)
    with pinned(conv, 2, {2: tile}, det=True):
        _run3(*wgrad_case(conv, "%s weight gradient tile %s, accumulating" % (name, tile), det=True, accumulate=True))


@MODES
@pytest.mark.parametrize("tile", [(0, 1, 1, 1), (0, 3, 1, 2), (0, 1, 4, 2)], ids=str)
@pytest.mark.parametrize("name", ["odd", "lin", "single"])
def test_native_tiles(name, tile, mode):
    _fwd_dgrad(name, 2, tile, mode)


@pytest.mark.parametrize("name", ["odd", "lin", "single"])
def test_native_weight_gradient(name):
    _wgrad(name, 2, (0, 3, 4, 0))


@MODES
@TERMS
@pytest.mark.parametrize("tile", [(1, 2, 0, 0), (1, 4, 0, 0), (1, 9, 0, 0), (1, 9, 2, 0)], ids=str)
@pytest.mark.parametrize("name", ["odd", "T2s", "short", "s2odd"])
def test_gather_kernel_k1s(name, tile, terms, mode):
    """igemm_k1s: the channel block and the channel stride ride in the SCALAR offset of every gather; the padded channels of the
    last sample (40, 230 gathered channels forward; 136, 42, 20 in the data gradient) point past the end of the gathered tensor,
    into the guard.  Between NaN guards the result must be what it is between zeros -- it is, because gfx950 range-checks vector
    plus scalar offset; a descriptor one channel group too long fails exactly these cases."""
    _fwd_dgrad(name, terms, tile, mode)


@TERMS
@pytest.mark.parametrize("mt,blocks", [(4, 4), (8, 8), (9, 16)])
@pytest.mark.parametrize("name", ["odd", "short", "lin"])
def test_gather_weight_gradient_k2s(name, mt, blocks, terms):
    """igemm_k2s: clamped rows and channels ("finite garbage whose products land in outputs nobody reads"), split tails."""
    _wgrad(name, terms, (1, mt, blocks, 0))


@pytest.mark.parametrize("mt", [4, 6])
@pytest.mark.parametrize("name", ["stem21", "stem3d"])
def test_stem_forward(name, mt):
    """The zero-padded copy of the clip in the workspace and the padding columns of the offset table."""
    _fwd_dgrad(name, 2, (1, mt, 0, 0), 0)


@pytest.mark.parametrize("name", ["stem21", "stem3d"])
def test_stem_weight_gradient(name):
    _wgrad(name, 2, (1, 9, 16, 0))


@MODES
@pytest.mark.parametrize("mt", [4, 8, 9])
@pytest.mark.parametrize("name", ["p_ragged", "p_thin"])
def test_spatial_patch_kernel(name, mt, mode):
    _fwd_dgrad(name, 2, (2, mt, 0, 0), mode)


@pytest.mark.parametrize("name", ["p_ragged", "p_thin", "p_wide"])
def test_spatial_patch_weight_gradient(name):
    _wgrad(name, 2, (2, 9, 1, 0))


@MODES
@pytest.mark.parametrize("mt", [4, 8, 9])
@pytest.mark.parametrize("name", ["t_ragged", "t_48rows"])
def test_temporal_patch_kernel(name, mt, mode):
    _fwd_dgrad(name, 2, (2, mt, 0, 0), mode)


@pytest.mark.parametrize("name", ["t_ragged", "t_48rows"])
def test_weight_resident_temporal_forward(name):
    """(2, 4, 2, .): igemm_k1w where the packed weights fit LDS (48 rows), the ring kernel igemm_k1t where not (80 rows)."""
    _fwd_dgrad(name, 2, (2, 4, 2, 0), 0)


@pytest.mark.parametrize("name", ["w_2col", "w_2row", "w_83", "w_16pos"])
def test_temporal_stream_weight_gradient_k2t(name):
    _wgrad(name, 2, (2, 9, 1, 0))


@pytest.mark.parametrize("name", ["lin64", "lin5"])
def test_streaming_linear_kernels(name):
    """csrc/linear.h (<= 32 rows): no tile is pinned -- a linear layer's route is decided by its shape, its alignment and the
    workspace it is given; whatever serves the call is held to the assertions."""
    conv = Conv(name)
    with pinned(conv, 2, {}):
        _run3(*fwd_case(conv, name + " forward"))
        _run3(*dgrad_case(conv, name + " data gradient"))
        _run3(*dgrad_case(conv, name + " data gradient, accumulating", accumulate=True))
    with pinned(conv, 2, {}, det=True):
        _run3(*wgrad_case(conv, name + " weight gradient", det=True))
        _run3(*wgrad_case(conv, name + " weight gradient, accumulating", det=True, accumulate=True))


@pytest.mark.parametrize("name,tile", [("odd", (0, 1, 1, 1)), ("odd", (1, 4, 0, 0)), ("lin", (1, 2, 0, 0))],
                         ids=["native", "split", "split linear"])
def test_bias_path(name, tile):
    """bias inside guards in the forward epilogue; db = cstp_channel_sum(dy) inside guards."""
    _l, lib, ops = _libs()
    conv = Conv(name)
    with pinned(conv, 2, {0: tile}):
        _run3(*fwd_case(conv, "%s forward with bias, tile %s" % (name, tile), bias=True))
    r = _conv_ref(name)
    n, k = conv.ys[0], conv.ys[1]
    s = int(np.prod(conv.ys[2:]))
    spec = gb.Spec(name + " bias gradient", {"dy": r["dy"]}, {"db": ((k,), F32)}, {"db": gb.rel_check(r["db"], TOL)})
    _run3(spec, lambda v: _l.check(lib.cstp_channel_sum(_stream(), v["dy"].data_ptr(), v["db"].data_ptr(), n, k, s, None, 0),
                                   "cstp_channel_sum"))


# ---- the fused input transform: the scale_shift table and the absmax cell inside guards ------------------------------------

def _affine(conv, groups=1):
    g = torch.Generator().manual_seed(9)
    cin = conv.xs[1]
    r = _conv_ref(conv.name)
    scale = torch.rand(groups, cin, generator=g) * 1.5 - 0.25
    shift = torch.randn(groups, cin, generator=g) * 0.5
    n = conv.xs[0]
    sc = scale.double().repeat_interleave(n // groups, 0).view(n, cin, 1, 1, 1)
    sh = shift.double().repeat_interleave(n // groups, 0).view(n, cin, 1, 1, 1)
    z64 = torch.relu(r["x"].double() * sc + sh)
    ref = F.conv3d(z64, r["w"].double(), None, conv.st, conv.pd)
    cell = torch.tensor([float(z64.abs().max()) * 1.01], dtype=F32).view(I32)       # an upper bound is all the kernels need
    return torch.stack([scale, shift], 2).contiguous(), groups, 1, cell, ref


@pytest.mark.parametrize("name,tile,want", [("aff_split", (1, 4, 0, 0), [64, 128, 2]), ("aff_tpatch", (2, 4, 0, 0), [64, 224, 2])],
                         ids=["igemm_k1s", "temporal patch"])
def test_fused_input_transform(name, tile, want):
    conv = Conv(name)
    with pinned(conv, 2, {0: tile}, confirm=False):
        assert conv.query(3)[:3] == want, (name, conv.query(3))        # mode 3: the forward that carries an in_affine
        _run3(*fwd_case(conv, name + " forward with in_affine", aff=_affine(conv)))


def test_input_transform_on_a_native_kernel_where_the_host_declines():
    """40 channels: no whole 16-channel groups, the split kernels do not apply the table; a native tile does (return code only:
    the query entry points describe the plain forward)."""
    conv = Conv("aff_native")
    with pinned(conv, 2, {0: (1, 4, 0, 0)}):
        a = _affine(conv, groups=2)
        _run3(*fwd_case(conv, "aff_native forward with in_affine", aff=a))
        _run3(*fwd_case(conv, "aff_native forward with in_affine, no cell", aff=a[:3] + (None,) + a[4:]))


# ---- forward_bnstats: part, the pivots and z_cell inside guards -------------------------------------------------------------

def _keys_to_float(keys_i32):
    k = keys_i32.to(torch.int64) & 0xFFFFFFFF
    bits = torch.where((k & 0x80000000) != 0, k ^ 0x80000000, (~k) & 0xFFFFFFFF)
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits)
    return bits.to(I32).view(F32)


@pytest.mark.parametrize("groups", [1, 2])
def test_forward_bnstats(groups):
    _l, lib, ops = _libs()
    conv = Conv("p_stats")
    k = conv.k
    with pinned(conv, 2, {0: (2, 9, 0, 0)}):
        ns = lib.cstp_conv3d_bnstats_nsplit(ctypes.byref(conv.desc), groups)
        assert ns > 0, "the patch kernel leaves no sums for this geometry"
        r = _conv_ref("p_stats")
        pivot = (_rand((k,), 12) * 0.1).float()
        ngs = k * groups * ns
        yg = r["y"].view(groups, conv.ys[0] // groups, k, -1).permute(2, 0, 1, 3).reshape(k, groups, -1)     # [k][groups][values]
        mean, var = yg.mean(2), yg.var(2, unbiased=False)
        count = yg.shape[2]

        def check_part(part):
            sums = part[:ngs * 2].view(k, groups, ns, 2)
            assert bool(torch.isfinite(part[:ngs * 2 + k]).all()), "non-finite sums or pivots"
            assert torch.equal(part[ngs * 2:ngs * 2 + k], pivot.double()), "the pivots behind the sums are not the ones given"
            m = sums[..., 0].sum(2) / count
            got_mean = m + pivot.double().view(k, 1)
            got_var = sums[..., 1].sum(2) / count - m * m
            gb.rel_check(mean, TOL)(got_mean)
            gb.rel_check(var, TOL)(got_var)
            mm = _keys_to_float(part[ngs * 2 + k:].contiguous().view(I32)[:ngs * 2]).view(k, groups, ns, 2).double()
            lo = torch.where(torch.isnan(mm[..., 0]), torch.full_like(mm[..., 0], float("inf")), mm[..., 0]).amin(2)
            hi = torch.where(torch.isnan(mm[..., 1]), torch.full_like(mm[..., 1], float("-inf")), mm[..., 1]).amax(2)
            top = float(r["y"].abs().max())
            assert float((lo - yg.amin(2)).abs().max()) < TOL * top and float((hi - yg.amax(2)).abs().max()) < TOL * top, \
                "the range keys behind the pivots"

        def check_zcell(cell):
            assert int(cell[0]) == 0, "z_cell is zeroed by the launch"

        spec = gb.Spec("p_stats forward_bnstats groups %d" % groups, {"x": r["x"], "w": r["w"], "pivot": pivot},
                       {"y": (conv.ys, F32), "part": ((ngs * 3 + k,), F64), "z_cell": ((1,), I32)},
                       {"y": gb.rel_check(r["y"], TOL), "part": check_part, "z_cell": check_zcell}, ws_bytes=conv.ws_bytes(),
                       finite_as={"part": None, "z_cell": None})

        def impl(v):
            got = ctypes.c_int32(0)
            _l.check(lib.cstp_conv3d_forward_bnstats(_stream(), ctypes.byref(conv.desc), v["x"].data_ptr(), v["w"].data_ptr(),
                                                     v["y"].data_ptr(), v["ws"].data_ptr(), spec.ws_bytes, None, groups,
                                                     v["pivot"].data_ptr(), v["part"].data_ptr(), v["part"].numel() * 8,
                                                     ctypes.byref(got), v["z_cell"].data_ptr(), None), "cstp_conv3d_forward_bnstats")
            assert got.value == ns, "nsplit %d, announced %d" % (got.value, ns)
        _run3(spec, impl)


# ---- misaligned operands: the host hands over to another kernel (tests/test_pack_replay_gpu.py names which) ---------------

@pytest.mark.parametrize("mode,which", [(0, "x"), (0, "y"), (1, "dy"), (1, "dx")])
@pytest.mark.parametrize("name,tile", [("odd", (1, 4, 0, 0)), ("p_thin", (2, 4, 0, 0)), ("t_ragged", (2, 4, 0, 0))],
                         ids=["igemm_k1s", "spatial patch", "temporal patch"])
def test_misaligned_operand(name, tile, mode, which):
    """The gathered operand, or the output, one element off the allocation's alignment (assertion 1: the return code only)."""
    conv = Conv(name)
    with pinned(conv, 2, {mode: tile}):
        what = "%s tile %s, %s shifted by one element" % (name, tile, which)
        _run3(*(fwd_case(conv, what, shifts={which: 4}) if mode == 0 else dgrad_case(conv, what, shifts={which: 4})))


# ---- bf16 storage: cstp_b16_conv3d_* ----------------------------------------------------------------------------------------

B16_CONVS = {
    # name: (x shape, k, kernel, stride, pad, data gradient served) -- test_b16_gpu.py's CONVS, test_r21d_b16_gpu.py's RAGGED
    "5x5": ((2, 48, 2, 5, 5), 80, (1, 3, 3), (1, 1, 1), (0, 1, 1), True),
    "pointwise": ((3, 48, 2, 6, 4), 80, (1, 1, 1), (1, 1, 1), (0, 0, 0), True),
    "stride 2": ((3, 64, 3, 9, 7), 128, (1, 1, 1), (2, 2, 2), (0, 0, 0), True),
    "83 channels": ((2, 83, 4, 16, 16), 64, (3, 1, 1), (1, 1, 1), (1, 0, 0), True),       # RAG groups, octet gather
    "stem": ((2, 3, 4, 32, 32), 83, (1, 7, 7), (1, 2, 2), (0, 3, 3), False),              # the offset table
    "85 channels": ((2, 85, 2, 4, 4), 256, (1, 1, 1), (2, 1, 1), (0, 0, 0), True),
    "octets": ((2, 64, 3, 8, 16), 64, (3, 3, 3), (1, 1, 1), (1, 1, 1), True),             # the neighbouring dword at the last row
}


ulp_bf16, rounded_check = gb.ulp_bf16, gb.rounded_check      # (shared with tests/test_guard_bands_ops_gpu.py)


@functools.lru_cache(maxsize=None)
def _b16_ref(name):
    xs, k, ks, st, pd, _ = B16_CONVS[name]
    g = torch.Generator().manual_seed(sum(xs) + k)
    x = torch.randn(xs, generator=g).to(B16)
    w = torch.randn((k, xs[1]) + ks, generator=g) / np.sqrt(xs[1] * np.prod(ks))
    x64, w64 = x.double().requires_grad_(True), w.to(B16).double().requires_grad_(True)       # (the kernels round the weights to bf16)
    y = F.conv3d(x64, w64, None, st, pd)
    dy = torch.randn(y.shape, generator=g).to(B16)
    dx, dw = torch.autograd.grad(y, (x64, w64), dy.double())
    old = torch.randn(xs, generator=g).to(B16)
    return {"x": x, "w": w, "dy": dy, "y": y.detach(), "dx": dx, "dw": dw, "old": old}


def _b16_call(fn, desc, spec, names, extra=()):
    _l, lib, ops = _libs()

    def impl(v):
        _l.check(getattr(lib, fn)(_stream(), ctypes.byref(desc), *[v[n].data_ptr() for n in names], v["ws"].data_ptr(),
                                  spec.ws_bytes, *extra), fn)
    return impl


# (the 3-channel stem has no data gradient: forward and weight gradient only, include/cstp_hip.h)
B16_CASES = [(n, op) for n in B16_CONVS for op in ("forward", "dgrad", "dgrad_acc", "wgrad", "wgrad_acc")
             if B16_CONVS[n][5] or not op.startswith("dgrad")]


@pytest.mark.parametrize("name,op", B16_CASES, ids=["%s-%s" % c for c in B16_CASES])
def test_bf16_convolution(name, op):
    _b16_conv(name, op, None)


def _b16_conv(name, op, shifts):
    _l, lib, ops = _libs()
    xs, k, ks, st, pd, _ = B16_CONVS[name]
    wshape = (k, xs[1]) + ks
    desc = ops._desc(xs, wshape, st, pd)
    ys = ops.conv_out_shape(xs, wshape, st, pd)
    nbytes = lib.cstp_b16_conv3d_workspace_bytes(ctypes.byref(desc))
    r = _b16_ref(name)
    what = "bf16 %s %s" % (name, op) + ("" if not shifts else ", shifted %s" % sorted(shifts))
    if op == "forward":
        spec = gb.Spec(what, {"x": r["x"], "w": r["w"]}, {"y": (ys, B16)}, {"y": rounded_check(r["y"])}, nbytes, shifts=shifts)
        impl = _b16_call("cstp_b16_conv3d_forward", desc, spec, ("x", "w", "y"))
    elif op == "dgrad":
        spec = gb.Spec(what, {"dy": r["dy"], "w": r["w"]}, {"dx": (xs, B16)}, {"dx": rounded_check(r["dx"])}, nbytes, shifts=shifts)
        impl = _b16_call("cstp_b16_conv3d_backward_data", desc, spec, ("dy", "w", "dx"))
    elif op == "dgrad_acc":
        old, dx64 = r["old"], r["dx"]

        def check(got_b16):     # test_r21d_b16_gpu.py::test_conv3d_bf16_ragged_backward_data_accumulates
            exact, got = dx64 + old.double(), got_b16.double()
            err = (got - exact).abs()
            bad = err > ulp_bf16(dx64) + ulp_bf16(exact) + 1e-5 * float(exact.abs().max())
            assert not bool(bad.any()), "%d elements beyond the two roundings, worst %g" % (int(bad.sum()), float(err.max()))
            flips = float((got != (dx64.to(B16).double() + old.double()).to(B16).double()).double().mean())
            assert flips < 1e-3, flips
        spec = gb.Spec(what, {"dy": r["dy"], "w": r["w"]}, {"dx": (xs, B16)}, {"dx": check}, nbytes, priors={"dx": old},
                       shifts=shifts)
        impl = _b16_call("cstp_b16_conv3d_backward_data_acc", desc, spec, ("dy", "w", "dx"), extra=(1,))
    else:
        acc = op == "wgrad_acc"
        prior = torch.full(wshape, 0.75) if acc else None

        def check(got):
            err = float(((got.double() - (0.75 if acc else 0.0)) - r["dw"]).abs().max() / r["dw"].abs().max())
            assert err < 2e-5, "weight gradient %g" % err
        spec = gb.Spec(what, {"x": r["x"], "dy": r["dy"]}, {"dw": (wshape, F32)}, {"dw": check}, nbytes,
                       priors={"dw": prior} if acc else None, shifts=shifts)
        impl = _b16_call("cstp_b16_conv3d_backward_weight", desc, spec, ("x", "dy", "dw"), extra=(1 if acc else 0,))
    _run3(spec, impl)


@pytest.mark.parametrize("op,which,shift", [("forward", "x", 2), ("dgrad", "dy", 2), ("forward", "y", 8), ("dgrad", "dx", 8)])
def test_bf16_pointwise_misaligned_operand(op, which, shift):
    """The gathered operand one bf16 element (2 bytes) off: the pointwise and octet paths need 16-byte rows, the scalar gather
    takes over.  The output four elements (8 bytes) off a 16-byte boundary: the least the entry points accept (below)."""
    _b16_conv("pointwise", op, {which: shift})


@pytest.mark.parametrize("op,which", [("forward", "y"), ("dgrad", "dx")])
def test_bf16_output_off_an_8_byte_boundary_is_refused_and_nothing_is_touched(op, which):
    """cstp_b16_conv3d_forward / _backward_data store four bf16 values at a time and REFUSE an output that is not 8-byte aligned
    (include/cstp_hip.h: refused, not emulated).  The refusal must come before anything is launched: every guard intact, every
    input unchanged, the output and the workspace still 0xFF."""
    _l, lib, ops = _libs()
    xs, k, ks, st, pd, _ = B16_CONVS["pointwise"]
    wshape = (k, xs[1]) + ks
    desc = ops._desc(xs, wshape, st, pd)
    ys = ops.conv_out_shape(xs, wshape, st, pd)
    nbytes = lib.cstp_b16_conv3d_workspace_bytes(ctypes.byref(desc))
    r = _b16_ref("pointwise")
    src, out, oshape, fn = (("x", "y", ys, "cstp_b16_conv3d_forward") if op == "forward"
                            else ("dy", "dx", xs, "cstp_b16_conv3d_backward_data"))
    spec = gb.Spec("bf16 pointwise %s, %s one element off" % (op, which), {src: r[src], "w": r["w"]}, {out: (oshape, B16)}, {},
                   nbytes, shifts={which: 2})
    operands = gb.Operands(spec, DEV)
    for fill in ("zero", "nan"):
        operands.arm(fill)
        v = operands.views()
        rc = getattr(lib, fn)(_stream(), ctypes.byref(desc), v[src].data_ptr(), v["w"].data_ptr(), v[out].data_ptr(),
                              v["ws"].data_ptr(), nbytes)
        torch.cuda.synchronize()
        assert rc != 0 and b"unaligned output" in lib.cstp_last_error(), (rc, lib.cstp_last_error())
        assert operands.problems() == []
        assert bool((operands.outs[out].buf == 0xFF).all()) and bool((operands.ws.buf == 0xFF).all()), "a refused call wrote"


# ---- BatchNorm ---------------------------------------------------------------------------------------------------------------

BNS = {
    # name: (shape, groups)
    "3x7": ((3, 7, 1, 1, 1), 1),             # BatchNorm1d: three rows
    "6x7x25": ((6, 7, 1, 5, 5), 1),          # the single-launch kernels; 25 positions: vector tails
    "4x9x49": ((4, 9, 1, 7, 7), 1),
    "8x40": ((8, 40, 1, 1, 1), 1),           # BatchNorm1d [8][40]
    "32x24 g2": ((32, 24, 2, 7, 7), 2),
}
EPS, MOM = 1e-5, 0.1


@functools.lru_cache(maxsize=None)
def _bn_ref(shape, groups, use_res, relu, bf16=False):
    """Operands and fp64 results of y = act(bn_train(x) + residual) per group, running statistics group after group."""
    n, c = shape[0], shape[1]
    rnd = (lambda t: t.to(B16)) if bf16 else (lambda t: t.float())
    x = rnd(_rand(shape, 8) * 2 + 0.5)
    res = rnd(_rand(shape, 11)) if use_res else None
    gamma, beta = (_rand((c,), 9).abs() + 0.5).float(), (_rand((c,), 10) * 0.1).float()
    rm, rv = (_rand((c,), 12) * 0.1).float(), (_rand((c,), 13).abs() + 0.5).float()
    dy = rnd(_rand(shape, 14))
    x64 = x.double().requires_grad_(True)
    r64 = None if res is None else res.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    ys, means, invstds = [], [], []
    for xg in x64.chunk(groups, 0):
        ys.append(F.batch_norm(xg, rm64, rv64, g64, b64, True, MOM, EPS))
        d = tuple(i for i in range(xg.dim()) if i != 1)
        means.append(xg.detach().mean(d))
        invstds.append(1.0 / torch.sqrt(xg.detach().var(d, unbiased=False) + EPS))
    y = torch.cat(ys, 0)
    if use_res:
        y = y + r64
    if relu:
        y = F.relu(y)
    grads = torch.autograd.grad(y, [x64, g64, b64] + ([r64] if use_res else []), dy.double())
    mean, invstd = torch.stack(means), torch.stack(invstds)
    scale = invstd * gamma.double()
    ss = torch.stack([scale, beta.double() - mean * scale], 2)
    yev = (x.double() - rm.double().view(1, -1, 1, 1, 1)) / torch.sqrt(rv.double().view(1, -1, 1, 1, 1) + EPS) \
        * gamma.double().view(1, -1, 1, 1, 1) + beta.double().view(1, -1, 1, 1, 1)
    if use_res:
        yev = yev + res.double()
    if relu:
        yev = F.relu(yev)
    return {"x": x, "res": res, "gamma": gamma, "beta": beta, "rm": rm, "rv": rv, "dy": dy, "y": y.detach(), "mean": mean,
            "invstd": invstd, "ss": ss, "rm_new": rm64, "rv_new": rv64, "dx": grads[0], "dgamma": grads[1], "dbeta": grads[2],
            "dres": grads[3] if use_res else None, "y_eval": yev}


def _cell_check(what):
    """An absmax cell holds the fp32 bits (sign cleared) of a finite maximum: compared with the tensor it belongs to below."""
    def check(cell):
        v = float(cell.view(F32)[0])
        assert v > 0.0 and v == v and v != float("inf"), "%s cell holds %r" % (what, v)
    return check


@pytest.mark.parametrize("use_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("name", list(BNS))
def test_batch_norm_forward_train(name, use_res):
    _l, lib, ops = _libs()
    shape, groups = BNS[name]
    n, c = shape[0], shape[1]
    s = int(np.prod(shape[2:]))
    r = _bn_ref(shape, groups, use_res, True)
    nbytes = lib.cstp_bn_workspace_bytes(n, c, s, groups)
    inputs = {"x": r["x"], "gamma": r["gamma"], "beta": r["beta"]}
    if use_res:
        inputs["res"] = r["res"]
    outputs = {"y": (shape, F32), "mean": ((groups, c), F32), "invstd": ((groups, c), F32), "rm": ((c,), F32), "rv": ((c,), F32)}
    checks = {"y": gb.rel_check(r["y"], TOL), "mean": gb.rel_check(r["mean"], TOL), "invstd": gb.rel_check(r["invstd"], TOL),
              "rm": gb.rel_check(r["rm_new"], TOL), "rv": gb.rel_check(r["rv_new"], TOL)}
    finite_as = {}
    if s > 1:         # the affine table and the absmax cell: s > 1 only (include/cstp_hip.h)
        outputs.update({"ss": ((groups, c, 2), F32), "cell": ((1,), I32)})
        checks.update({"ss": gb.rel_check(r["ss"], TOL), "cell": _cell_check("y")})
        finite_as["cell"] = F32
    spec = gb.Spec("bn_forward_train_am %s%s" % (name, " + residual" if use_res else ""), inputs, outputs, checks, nbytes,
                   priors={"rm": r["rm"], "rv": r["rv"]}, finite_as=finite_as, control_must_hold=False)
    cells = []

    def impl(v):
        _l.check(lib.cstp_bn_forward_train_am(_stream(), v["x"].data_ptr(), _ptr(v, "res"), v["y"].data_ptr(), v["gamma"].data_ptr(),
                                              v["beta"].data_ptr(), v["rm"].data_ptr(), v["rv"].data_ptr(), v["mean"].data_ptr(),
                                              v["invstd"].data_ptr(), _ptr(v, "ss"), n, c, s, groups, EPS, MOM, 1, v["ws"].data_ptr(),
                                              spec.ws_bytes, _ptr(v, "cell")), "cstp_bn_forward_train_am")
        if s > 1:     # the cell is max |y| of THIS y, to the bit (test_ops_gpu.py)
            torch.cuda.synchronize()
            cells.append((int(v["cell"].item()), int(v["y"].abs().max().view(I32).item())))
    _run3(spec, impl)
    assert all(a == b for a, b in cells), cells


@pytest.mark.parametrize("name", [n for n in BNS if int(np.prod(BNS[n][0][2:])) > 1])
def test_batch_norm_stats_train(name):
    """cstp_bn_stats_train: the statistics and the affine table a consumer convolution applies in its gather; no y at all."""
    _l, lib, ops = _libs()
    shape, groups = BNS[name]
    n, c = shape[0], shape[1]
    s = int(np.prod(shape[2:]))
    r = _bn_ref(shape, groups, False, True)
    spec = gb.Spec("bn_stats_train " + name, {"x": r["x"], "gamma": r["gamma"], "beta": r["beta"]},
                   {"mean": ((groups, c), F32), "invstd": ((groups, c), F32), "ss": ((groups, c, 2), F32), "rm": ((c,), F32),
                    "rv": ((c,), F32)},
                   {"mean": gb.rel_check(r["mean"], TOL), "invstd": gb.rel_check(r["invstd"], TOL), "ss": gb.rel_check(r["ss"], TOL),
                    "rm": gb.rel_check(r["rm_new"], TOL), "rv": gb.rel_check(r["rv_new"], TOL)},
                   lib.cstp_bn_workspace_bytes(n, c, s, groups), priors={"rm": r["rm"], "rv": r["rv"]}, control_must_hold=False)

    def impl(v):
        _l.check(lib.cstp_bn_stats_train(_stream(), v["x"].data_ptr(), v["gamma"].data_ptr(), v["beta"].data_ptr(), v["rm"].data_ptr(),
                                         v["rv"].data_ptr(), v["mean"].data_ptr(), v["invstd"].data_ptr(), v["ss"].data_ptr(), n, c, s,
                                         groups, EPS, MOM, v["ws"].data_ptr(), spec.ws_bytes), "cstp_bn_stats_train")
    _run3(spec, impl)


@pytest.mark.parametrize("use_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("name", list(BNS))
def test_batch_norm_backward(name, use_res):
    """cstp_bn_backward_am (s > 1; with a ReLU and no residual the mask comes from x and the affine table, as ops.py calls it) and
    cstp_bn1d_backward (s = 1).  The saved statistics and y are the fp64 reference's, rounded to fp32."""
    _l, lib, ops = _libs()
    shape, groups = BNS[name]
    n, c = shape[0], shape[1]
    s = int(np.prod(shape[2:]))
    r = _bn_ref(shape, groups, use_res, True)
    remask = s > 1 and not use_res
    inputs = {"x": r["x"], "dy": r["dy"], "gamma": r["gamma"]}
    if remask:
        inputs["ss"] = r["ss"].float()
    else:
        inputs["y"] = r["y"].float()
    if s > 1:
        inputs.update({"mean": r["mean"].float(), "invstd": r["invstd"].float()})
    outputs = {"dx": (shape, F32), "dgamma": ((c,), F32), "dbeta": ((c,), F32)}
    checks = {"dx": gb.rel_check(r["dx"], TOL), "dgamma": gb.rel_check(r["dgamma"], TOL), "dbeta": gb.rel_check(r["dbeta"], TOL)}
    finite_as = {}
    if use_res:
        outputs["dres"] = (shape, F32)
        checks["dres"] = gb.rel_check(r["dres"], TOL)
    if s > 1:
        outputs["cell"] = ((1,), I32)
        checks["cell"] = _cell_check("dx")
        finite_as["cell"] = F32
    nbytes = lib.cstp_bn_workspace_bytes(n, c, s, groups) if s > 1 else 0
    spec = gb.Spec("bn backward %s%s" % (name, " + residual" if use_res else ""), inputs, outputs, checks, nbytes,
                   finite_as=finite_as, control_must_hold=False)
    cells = []

    def impl(v):
        if s == 1:
            _l.check(lib.cstp_bn1d_backward(_stream(), v["x"].data_ptr(), v["y"].data_ptr(), v["dy"].data_ptr(), v["gamma"].data_ptr(),
                                            v["dx"].data_ptr(), _ptr(v, "dres"), v["dgamma"].data_ptr(), v["dbeta"].data_ptr(), n, c,
                                            groups, EPS, 1, 0), "cstp_bn1d_backward")
            return
        _l.check(lib.cstp_bn_backward_am(_stream(), v["x"].data_ptr(), _ptr(v, "y"), v["dy"].data_ptr(), v["gamma"].data_ptr(),
                                         v["mean"].data_ptr(), v["invstd"].data_ptr(), _ptr(v, "ss"), v["dx"].data_ptr(),
                                         _ptr(v, "dres"), v["dgamma"].data_ptr(), v["dbeta"].data_ptr(), n, c, s, groups, 1,
                                         v["ws"].data_ptr(), spec.ws_bytes, v["cell"].data_ptr(), 0), "cstp_bn_backward_am")
        torch.cuda.synchronize()
        cells.append((int(v["cell"].item()), int(v["dx"].abs().max().view(I32).item())))
    _run3(spec, impl)
    assert all(a == b for a, b in cells), cells


@pytest.mark.parametrize("use_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("name", list(BNS))
def test_batch_norm_forward_eval(name, use_res):
    _l, lib, ops = _libs()
    shape, groups = BNS[name]
    n, c = shape[0], shape[1]
    s = int(np.prod(shape[2:]))
    r = _bn_ref(shape, groups, use_res, True)
    inputs = {"x": r["x"], "gamma": r["gamma"], "beta": r["beta"], "rm": r["rm"], "rv": r["rv"]}
    if use_res:
        inputs["res"] = r["res"]
    nbytes = lib.cstp_bn_eval_workspace_bytes(c) if s > 1 else 0
    spec = gb.Spec("bn_forward_eval %s%s" % (name, " + residual" if use_res else ""), inputs, {"y": (shape, F32)},
                   {"y": gb.rel_check(r["y_eval"], TOL)}, nbytes, control_must_hold=False)

    def impl(v):
        _l.check(lib.cstp_bn_forward_eval(_stream(), v["x"].data_ptr(), _ptr(v, "res"), v["y"].data_ptr(), v["gamma"].data_ptr(),
                                          v["beta"].data_ptr(), v["rm"].data_ptr(), v["rv"].data_ptr(), n, c, s, EPS, 1,
                                          v["ws"].data_ptr(), spec.ws_bytes), "cstp_bn_forward_eval")
    _run3(spec, impl)


# ---- BatchNorm on bf16 storage (the bars of test_b16_gpu.py::test_batch_norm_bf16_forward_backward) ------------------------

B16_BNS = {"2x5 odd": ((2, 5, 6, 9, 11), 1), "4x64 g2": ((4, 64, 4, 14, 14), 2)}      # 8-element tails; two groups


def _within_ulp(ref64, rel_floor, worst_floor=None):
    def check(got):
        err = (got.double() - ref64).abs()
        if worst_floor is not None:
            assert float(err.max()) <= float((ulp_bf16(ref64) + worst_floor * ref64.abs().max()).max()), "worst element %g" % float(err.max())
        bad = err > ulp_bf16(ref64) + rel_floor * float(ref64.abs().max())
        assert not bool(bad.any()), "%d elements further than one bf16 ulp + %g of the maximum" % (int(bad.sum()), rel_floor)
    return check


@pytest.mark.parametrize("use_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("name", list(B16_BNS))
def test_bf16_batch_norm_forward_train(name, use_res):
    _l, lib, ops = _libs()
    shape, groups = B16_BNS[name]
    n, c = shape[0], shape[1]
    s = int(np.prod(shape[2:]))
    r = _bn_ref(shape, groups, use_res, True, True)
    inputs = {"x": r["x"], "gamma": r["gamma"], "beta": r["beta"]}
    if use_res:
        inputs["res"] = r["res"]

    def rm_check(got):
        assert float((got.double() - r["rm_new"]).abs().max()) < 1e-6

    def rv_check(got):
        assert float((got.double() - r["rv_new"]).abs().max() / r["rv_new"].abs().max()) < 1e-6
    outputs = {"y": (shape, B16), "mean": ((groups, c), F32), "invstd": ((groups, c), F32), "ss": ((groups, c, 2), F32),
               "rm": ((c,), F32), "rv": ((c,), F32)}
    checks = {"y": _within_ulp(r["y"], 1e-5, 2e-6), "mean": gb.rel_check(r["mean"], TOL), "invstd": gb.rel_check(r["invstd"], TOL),
              "ss": gb.rel_check(r["ss"], TOL), "rm": rm_check, "rv": rv_check}
    spec = gb.Spec("b16_bn_forward_train %s%s" % (name, " + residual" if use_res else ""), inputs, outputs, checks,
                   lib.cstp_b16_bn_workspace_bytes(n, c, s, groups), priors={"rm": r["rm"], "rv": r["rv"]}, control_must_hold=False)

    def impl(v):
        _l.check(lib.cstp_b16_bn_forward_train(_stream(), v["x"].data_ptr(), _ptr(v, "res"), v["y"].data_ptr(), v["gamma"].data_ptr(),
                                               v["beta"].data_ptr(), v["rm"].data_ptr(), v["rv"].data_ptr(), v["mean"].data_ptr(),
                                               v["invstd"].data_ptr(), v["ss"].data_ptr(), n, c, s, groups, EPS, MOM, 1,
                                               v["ws"].data_ptr(), spec.ws_bytes), "cstp_b16_bn_forward_train")
    _run3(spec, impl)


@pytest.mark.parametrize("use_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("name", list(B16_BNS))
def test_bf16_batch_norm_backward(name, use_res):
    _l, lib, ops = _libs()
    shape, groups = B16_BNS[name]
    n, c = shape[0], shape[1]
    s = int(np.prod(shape[2:]))
    r = _bn_ref(shape, groups, use_res, True, True)
    inputs = {"x": r["x"], "dy": r["dy"], "gamma": r["gamma"], "mean": r["mean"].float(), "invstd": r["invstd"].float(),
              "ss": r["ss"].float()}
    if use_res:
        inputs["y"] = r["y"].to(B16)
    outputs = {"dx": (shape, B16), "dgamma": ((c,), F32), "dbeta": ((c,), F32)}

    def rel2e5(ref):
        def check(got):
            assert float((got.double() - ref).abs().max() / ref.abs().max()) < 2e-5
        return check
    checks = {"dx": _within_ulp(r["dx"], 2e-5), "dgamma": rel2e5(r["dgamma"]), "dbeta": rel2e5(r["dbeta"])}
    if use_res:
        outputs["dres"] = (shape, B16)
        checks["dres"] = rounded_check(r["dres"])
    spec = gb.Spec("b16_bn_backward %s%s" % (name, " + residual" if use_res else ""), inputs, outputs, checks,
                   lib.cstp_b16_bn_workspace_bytes(n, c, s, groups), control_must_hold=False)

    def impl(v):
        _l.check(lib.cstp_b16_bn_backward(_stream(), v["x"].data_ptr(), _ptr(v, "y"), v["dy"].data_ptr(), v["gamma"].data_ptr(),
                                          v["mean"].data_ptr(), v["invstd"].data_ptr(), v["ss"].data_ptr(), v["dx"].data_ptr(),
                                          _ptr(v, "dres"), v["dgamma"].data_ptr(), v["dbeta"].data_ptr(), n, c, s, groups, 1,
                                          v["ws"].data_ptr(), spec.ws_bytes, 0), "cstp_b16_bn_backward")
    _run3(spec, impl)


@pytest.mark.parametrize("use_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("name", list(B16_BNS))
def test_bf16_batch_norm_forward_eval(name, use_res):
    _l, lib, ops = _libs()
    shape, groups = B16_BNS[name]
    n, c = shape[0], shape[1]
    s = int(np.prod(shape[2:]))
    r = _bn_ref(shape, groups, use_res, True, True)
    inputs = {"x": r["x"], "gamma": r["gamma"], "beta": r["beta"], "rm": r["rm"], "rv": r["rv"]}
    if use_res:
        inputs["res"] = r["res"]
    spec = gb.Spec("b16_bn_forward_eval %s%s" % (name, " + residual" if use_res else ""), inputs, {"y": (shape, B16)},
                   {"y": _within_ulp(r["y_eval"], 1e-5, 2e-6)}, 0, control_must_hold=False)

    def impl(v):
        _l.check(lib.cstp_b16_bn_forward_eval(_stream(), v["x"].data_ptr(), _ptr(v, "res"), v["y"].data_ptr(), v["gamma"].data_ptr(),
                                              v["beta"].data_ptr(), v["rm"].data_ptr(), v["rv"].data_ptr(), n, c, s, EPS, 1),
                 "cstp_b16_bn_forward_eval")
    _run3(spec, impl)

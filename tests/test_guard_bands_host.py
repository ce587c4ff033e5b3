"""tests/guard_bands.py on the CPU, before any GPU run: a plain torch convolution written into Guarded views through the call
signature of the GPU cases keeps the contract under both fills, and four deliberately sloppy variants are each REJECTED, each
for the reason it is sloppy: (a) a store one element past y, (b) a 16-channel gather of a padded channel group straight from
memory, multiplied by zero weights -- invisible between zero guards, NaN between NaN guards, which is why both fills exist --
(c) a workspace read before it is written, (d) an input scaled in place and restored only approximately.  Then Guarded itself:
alignment with and without the shift, the guard size, the offsets in the messages."""
import pytest
import torch
import torch.nn.functional as F

import guard_bands as gb

CPU = torch.device("cpu")
XS, K, KS, ST, PD = (3, 40, 3, 9, 11), 24, (1, 3, 3), (1, 2, 1), (0, 1, 1)     # 40 channels: the last group of 16 is half empty


def _spec(shifts=None):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(XS, generator=g) + 0.1
    w = torch.randn((K, XS[1]) + KS, generator=g) * 0.1
    ref = F.conv3d(x.double(), w.double(), None, ST, PD)
    return gb.Spec("host conv", {"x": x, "w": w}, {"y": (tuple(ref.shape), torch.float32)}, {"y": gb.rel_check(ref, 1e-4)},
                   ws_bytes=ref.numel() * 4, shifts=shifts)


def good(v):
    """Stages the result in the workspace (written, then read), as a split-K kernel does."""
    stage = v["ws"].view(torch.float32)[:v["y"].numel()].view(v["y"].shape)
    stage.copy_(F.conv3d(v["x"], v["w"], None, ST, PD))
    v["y"].copy_(stage)


def sloppy_store(v):
    good(v)
    v["y"].as_strided((v["y"].numel() + 1,), (1,))[-1] = 1.0


def sloppy_gather(v):
    """Channels 40..47 of a sample are the next sample's first channels; of the LAST sample, whatever follows x."""
    x, w = v["x"], v["w"]
    cp = (XS[1] + 15) // 16 * 16
    xg = x.as_strided((XS[0], cp) + XS[2:], x.stride())
    wp = torch.zeros((K, cp) + KS)
    wp[:, :XS[1]] = w
    v["y"].copy_(F.conv3d(xg, wp, None, ST, PD))


def sloppy_workspace(v):
    stage = v["ws"].view(torch.float32)[:v["y"].numel()].view(v["y"].shape)
    stage.add_(F.conv3d(v["x"], v["w"], None, ST, PD))          # "+=" into scratch nobody cleared
    v["y"].copy_(stage)


def sloppy_restore(v):
    v["x"].mul_(3.0)
    v["y"].copy_(F.conv3d(v["x"], v["w"], None, ST, PD) / 3.0)
    v["x"].mul_(1.0 / 3.0)


@pytest.mark.parametrize("shifts", [None, {"x": 4}, {"y": 4}], ids=["aligned", "x shifted", "y shifted"])
def test_a_correct_convolution_keeps_the_contract(shifts):
    assert gb.three_runs(_spec(shifts), good, CPU) == []
    assert gb.single_run(_spec(shifts), good, CPU) == []


def test_store_past_the_end_is_rejected_as_a_broken_guard():
    found = gb.three_runs(_spec(), sloppy_store, CPU)
    assert found and all("wrote 1 element past the end of y" in f for f in found), found
    assert len(found) == 3           # under every fill


def test_padded_channel_gather_passes_between_zeros_and_fails_between_nans():
    spec = _spec()
    ops = gb.Operands(spec, CPU)
    assert gb.one_run(spec, ops, sloppy_gather, "zero")[1] == []
    found = gb.one_run(spec, ops, sloppy_gather, "nan")[1]
    assert found and all("non-finite output" in f and " y " in f for f in found), found
    found = gb.three_runs(_spec(), sloppy_gather, CPU)
    assert len(found) == 1 and "[nan]" in found[0] and "non-finite" in found[0], found


def test_finite_garbage_from_the_surroundings_is_rejected_as_dependence():
    """A value from behind x that a clamp made finite and that moves one output by less than the parity bar: neither the
    finiteness check nor the reference sees it; bit-equality of the nan run with the two zero runs does."""
    def clamped(v):
        good(v)
        past = torch.nan_to_num(v["x"].as_strided((v["x"].numel() + 1,), (1,))[-1], nan=1.0)
        v["y"].view(-1)[0] += 1e-6 * past
    found = gb.three_runs(_spec(), clamped, CPU)
    assert found and any("depends on what surrounds the operands" in f for f in found), found


def test_workspace_read_before_write_is_rejected_as_non_finite():
    found = gb.three_runs(_spec(), sloppy_workspace, CPU)
    assert found and all("non-finite output" in f for f in found), found


def test_approximate_restore_is_rejected_as_a_changed_input():
    found = gb.three_runs(_spec(), sloppy_restore, CPU)
    assert found and all("of the input x" in f for f in found), found


def test_untouched_output_elements_are_rejected():
    def lazy(v):
        good(v)
        v["y"].view(-1)[-5:].view(torch.int32).fill_(-1)        # as if the tail had never been stored
    found = gb.three_runs(_spec(), lazy, CPU)
    assert found and all("non-finite output: 5 elements of y" in f for f in found), found


def test_accumulating_outputs_start_from_their_prior():
    g = torch.Generator().manual_seed(3)
    x, prior = torch.randn(7, 5, generator=g), torch.randn(7, 5, generator=g)
    spec = gb.Spec("acc", {"x": x}, {"y": ((7, 5), torch.float32)}, {"y": gb.rel_check(x.double() + prior.double(), 1e-6)},
                   priors={"y": prior})
    assert gb.three_runs(spec, lambda v: v["y"].add_(v["x"]), CPU) == []
    assert gb.three_runs(spec, lambda v: v["y"].copy_(v["x"]), CPU) != []


def test_a_control_that_does_not_hold_is_reported_only_where_it_must():
    state = {"n": 0}

    def noisy(v):
        state["n"] += 1
        v["y"].copy_(v["x"] * (1.0 + 1e-7 * state["n"]))
    x = torch.arange(1.0, 9.0)
    kw = dict(inputs={"x": x}, outputs={"y": ((8,), torch.float32)}, checks={"y": gb.rel_check(x.double(), 1e-4)})
    assert any("the control" in f for f in gb.three_runs(gb.Spec("noisy", **kw), noisy, CPU))
    assert gb.three_runs(gb.Spec("noisy", control_must_hold=False, **kw), noisy, CPU) == []


# ---- Guarded itself

@pytest.mark.parametrize("dtype,item", [(torch.float32, 4), (torch.bfloat16, 2), (torch.int32, 4)])
def test_guarded_alignment_and_shift(dtype, item):
    a = gb.Guarded((3, 5, 7), dtype, CPU)
    assert a.view.is_contiguous() and tuple(a.view.shape) == (3, 5, 7) and a.view.dtype == dtype
    assert a.data_ptr() - a.buf.data_ptr() == a.G and a.G % gb.PAGE == 0
    assert (a.data_ptr() - a.buf.data_ptr()) % 4096 == 0          # the view keeps the allocation's alignment
    b = gb.Guarded((3, 5, 7), dtype, CPU, shift=item)
    assert b.data_ptr() - b.buf.data_ptr() == b.G + item and b.view.is_contiguous()
    assert b.buf.numel() == a.buf.numel() == 2 * a.G + 3 * 5 * 7 * item
    with pytest.raises(AssertionError):
        gb.Guarded((4,), dtype, CPU, shift=item + 1)


def test_guard_size_formula():
    assert gb.guard_bytes(1) == 64 * 1024 and gb.guard_bytes(64 * 1024) == 64 * 1024
    assert gb.guard_bytes(64 * 1024 + 1) == 68 * 1024 and gb.guard_bytes(10 * 4096 * 4096 + 5) == 10 * 4096 * 4096 + 4096
    g = gb.Guarded((100000,), torch.float32, CPU)
    assert g.G == 401408 and g.G >= g.nbytes        # an index error of a whole operand stays inside the allocation


@pytest.mark.parametrize("fill", ["zero", "nan"])
def test_messages_carry_signed_element_offsets(fill):
    g = gb.Guarded((10,), torch.float32, CPU, name="dx")
    g.set_guards(gb.FILLS[fill])
    g.load(torch.arange(10.0))
    g.remember()
    assert g.intact() is None and g.unchanged() is None
    flat = g.view.as_strided((16,), (1,))
    flat[12] = 5.0                                   # element 12 of a 10-element operand: the third past the end
    assert "wrote 3 elements past the end of dx" in g.intact() and "element +3 from its last" in g.intact()
    g.set_guards(gb.FILLS[fill])
    g.buf[g.lo - 5] ^= 0x55                          # one byte, in the second element before the start
    assert "wrote 2 elements before the start of dx" in g.intact() and "element -2 from its first" in g.intact()
    g.set_guards(gb.FILLS[fill])
    g.view[4] = -4.0
    g.view[7] = 0.5
    assert "changed 2 elements of the input dx (first: element 4 of 10)" in g.unchanged()
    h = gb.Guarded((6,), torch.bfloat16, CPU, shift=2, name="x")
    h.set_guards(gb.FILLS[fill])
    h.view.as_strided((7,), (1,))[6] = 1.0
    assert "wrote 1 element past the end of x" in h.intact()


def test_nan_fill_is_nan_in_both_float_formats_and_minus_one_as_int32():
    g = gb.Guarded((4,), torch.float32, CPU)
    g.set_guards(0xFF)
    g.poison_interior()
    assert bool(torch.isnan(g.buf.view(torch.float32)).all()) and bool(torch.isnan(g.buf.view(torch.bfloat16)).all())
    assert bool((g.buf.view(torch.int32) == -1).all())

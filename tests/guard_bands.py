"""Guard bands around every operand of one kernel call ("What a call may touch").

``Guarded`` is one uint8 allocation of G + nbytes + G bytes with the operand as a contiguous view G (+ shift) bytes in, so that
an index error of up to one whole operand lands in memory the test owns.  ``Spec`` describes one call -- its inputs, its
outputs, its workspace and the fp64 checks of its results -- and ``three_runs`` makes it under the fills ``zero``, ``zero``,
``nan`` and holds it to the four assertions of the contract:

  1. the call succeeds (whatever ``impl`` raises fails the case),
  2. every output is finite and passes its check against the fp64 reference,
  3. every guard of every operand and of the workspace is intact, every input interior unchanged bit for bit,
  4. if the two ``zero`` runs are bit-equal, the ``nan`` run equals them (``control_must_hold``: the control itself is asserted).

Inputs take the run's fill in both guards (``nan`` = 0xFF bytes: NaN as fp32 and as bf16, -1 as int32).  Outputs always have
0xFF guards and a 0xFF interior, so an element the call never wrote reads as NaN; an output with a ``prior`` (an accumulating
call, running statistics) starts from those finite values instead.  The workspace is 0xFF inside and out: its content on entry
is unspecified.  Device-agnostic: the host test drives the same code with plain torch implementations on the CPU.

In-place operands ("What an in-place call may touch").  An operand that a call reads AND writes -- p, g, buf, the
moments, ema, running statistics, a ring, an accumulate target -- is an output with a ``prior``.  Its check is usually two checks
(``all_checks``): the numeric one on the elements the call owns, and ``untouched_check(prior, mask)`` on the rest, which asserts
BIT equality with the prior wherever ``mask`` is set and names the first changed element.

Several tensors inside one operand.  A case may carve slices out of one guarded arena -- the tensors of a parameter arena, or
dw | db | dgamma | dbeta of a gradient arena -- by handing the call ``view.data_ptr() + 4 * offset``.  What lies between the
slices (padding, a frozen tensor, another layer's live gradient) is part of the prior and goes into the mask of
``untouched_check``; no class of its own is needed.

A call may be a pair.  Where a workspace carries state from a forward to its backward (cstp_ntxent_*, cstp_ntxq_*), ``impl``
makes both calls: the workspace is poisoned before the forward only, and the backward must find there what the forward wrote.

What poison cannot show.  A read-modify-write of a guard leaves 0xFF (and 0x00) bytes unchanged: NaN in, NaN out.  Cases with
in-place operands therefore make a fourth run, ``live_run``, in which the guards of those operands hold a finite non-zero
pattern, as a live neighbour in an arena would."""
import torch

MIN_GUARD = 64 * 1024
PAGE = 4096
FILLS = {"zero": 0x00, "nan": 0xFF}
LIVE = 0x3C                  # 0x3C3C3C3C is 0.0115 as fp32, 0x3C3C 0.0115 as bf16: a finite, non-zero neighbour


def guard_bytes(nbytes):
    """G = max(64 KiB, nbytes rounded up to 4 KiB)."""
    return max(MIN_GUARD, (nbytes + PAGE - 1) // PAGE * PAGE)


def _plural(n, what):
    return "%d %s%s" % (n, what, "" if n == 1 else "s")


class Guarded:
    """An operand between two guard bands.  ``shift`` (bytes): 0, or one element for the misaligned variant (whole elements below
    16 bytes are taken: bf16 outputs must be 8-byte aligned, so their misaligned variant is four elements off)."""

    def __init__(self, shape, dtype, device, shift=0, name="operand"):
        self.name, self.shape, self.dtype, self.shift = name, tuple(shape), dtype, int(shift)
        self.itemsize = torch.empty(0, dtype=dtype).element_size()
        assert 0 <= self.shift < 16 and self.shift % self.itemsize == 0, "shift: whole elements, less than 16 bytes"
        numel = 1
        for s in self.shape:
            numel *= int(s)
        self.nbytes = numel * self.itemsize
        self.G = guard_bytes(self.nbytes)
        self.buf = torch.empty(2 * self.G + self.nbytes, dtype=torch.uint8, device=device)
        self.lo = self.G + self.shift
        self.hi = self.lo + self.nbytes
        self.view = self.buf[self.lo:self.hi].view(dtype).view(self.shape)
        self.guard_fill = 0xFF
        self._before = None

    # -- filling
    def set_guards(self, byte):
        self.guard_fill = int(byte)
        self.buf[:self.lo].fill_(self.guard_fill)
        self.buf[self.hi:].fill_(self.guard_fill)

    def poison_interior(self):
        self.buf[self.lo:self.hi].fill_(0xFF)

    def load(self, values):
        self.view.copy_(values.to(self.dtype).reshape(self.shape))

    def remember(self):
        self._before = self.buf[self.lo:self.hi].clone()

    def data_ptr(self):
        return self.view.data_ptr()

    # -- checking
    def intact(self):
        """None, or what happened to the guards: the first changed guard byte as a signed element offset from the operand's
        first (negative) or last (positive) element."""
        head = (self.buf[:self.lo] != self.guard_fill).nonzero()
        if head.numel():
            first, last = int(head[0]), int(head[-1])
            off = -((self.lo - first + self.itemsize - 1) // self.itemsize)
            near = (self.lo - last + self.itemsize - 1) // self.itemsize
            return "wrote %s before the start of %s (first changed guard byte: element %d from its first; nearest: %d before)" % (
                _plural(-off, "element"), self.name, off, near)
        tail = (self.buf[self.hi:] != self.guard_fill).nonzero()
        if tail.numel():
            first, last = int(tail[0]), int(tail[-1])
            off = first // self.itemsize + 1
            return "wrote %s past the end of %s (first changed guard byte: element +%d from its last; farthest: +%d)" % (
                _plural(off, "element"), self.name, off, last // self.itemsize + 1)
        return None

    def unchanged(self):
        """None, or the first element of the interior that differs from the copy ``remember`` took."""
        assert self._before is not None, "remember() first"
        diff = (self.buf[self.lo:self.hi] != self._before).nonzero()
        if diff.numel():
            first = int(diff[0]) // self.itemsize
            n = int(torch.unique(diff.flatten() // self.itemsize).numel())
            return "changed %s of the input %s (first: element %d of %d)" % (_plural(n, "element"), self.name, first,
                                                                              self.nbytes // self.itemsize)
        return None


class Spec:
    """One call.  inputs: {name: CPU tensor of values}; outputs: {name: (shape, dtype)}; priors: {name: CPU tensor} for the
    outputs that start from finite values (the reference includes them); ws_bytes: the workspace; checks: {output name:
    f(got CPU tensor) -> None, raising AssertionError}; shifts: {name: bytes}; finite_as: {output name: dtype} to view an integer
    cell as the floating-point value it holds (None: not a floating-point value, no finiteness check)."""

    def __init__(self, what, inputs, outputs, checks, ws_bytes=0, priors=None, shifts=None, finite_as=None,
                 control_must_hold=True):
        self.what, self.inputs, self.outputs, self.checks = what, inputs, outputs, checks
        self.ws_bytes, self.priors, self.shifts = int(ws_bytes), priors or {}, shifts or {}
        self.finite_as, self.control_must_hold = finite_as or {}, control_must_hold
        assert set(self.priors) <= set(outputs) and not (set(inputs) & set(outputs))


class Operands:
    """The guarded operands of a Spec on one device, allocated once and re-armed before every run."""

    def __init__(self, spec, device):
        self.spec = spec
        self.ins = {n: Guarded(t.shape, t.dtype, device, spec.shifts.get(n, 0), n) for n, t in spec.inputs.items()}
        self.outs = {n: Guarded(s, d, device, spec.shifts.get(n, 0), n) for n, (s, d) in spec.outputs.items()}
        self.ws = Guarded((max(spec.ws_bytes, 1),), torch.uint8, device, 0, "the workspace")

    def arm(self, fill, live=False):
        """live: the guards of every output with a prior hold LIVE bytes (a finite neighbour) instead of 0xFF (live_run)."""
        byte = FILLS[fill]
        for n, g in self.ins.items():
            g.set_guards(byte)
            g.load(self.spec.inputs[n])
            g.remember()
        for n, g in self.outs.items():
            g.set_guards(LIVE if live and n in self.spec.priors else 0xFF)
            if n in self.spec.priors:
                g.load(self.spec.priors[n])
            else:
                g.poison_interior()
        self.ws.set_guards(0xFF)
        self.ws.poison_interior()

    def views(self):
        v = {n: g.view for n, g in self.ins.items()}
        v.update({n: g.view for n, g in self.outs.items()})
        v["ws"] = self.ws.view
        return v

    def problems(self):
        """Assertion 3: every guard intact, every input interior unchanged."""
        found = []
        for g in list(self.ins.values()) + list(self.outs.values()) + [self.ws]:
            msg = g.intact()
            if msg:
                found.append(msg)
        for g in self.ins.values():
            msg = g.unchanged()
            if msg:
                found.append(msg)
        return found


def _finite_problem(spec, name, got):
    as_dtype = spec.finite_as.get(name, got.dtype)
    if as_dtype is None:
        return None
    t = got if as_dtype == got.dtype else got.view(as_dtype)
    if not t.dtype.is_floating_point:
        return None
    bad = ~torch.isfinite(t)
    if bool(bad.any()):
        return "non-finite output: %s of %s (first: element %d)" % (_plural(int(bad.sum()), "element"), name,
                                                                    int(bad.flatten().nonzero()[0]))
    return None


def one_run(spec, ops, impl, fill, sync=None, live=False):
    """Arm, call, and hold the run to assertions 1-3.  Returns ({output: CPU copy}, [problems])."""
    ops.arm(fill, live)
    impl(ops.views())
    if sync is not None:
        sync()
    found = ["%s [%s]: %s" % (spec.what, fill, p) for p in ops.problems()]
    outs = {n: g.view.detach().cpu().clone() for n, g in ops.outs.items()}
    for n, got in outs.items():
        msg = _finite_problem(spec, n, got)
        if msg:
            found.append("%s [%s]: %s" % (spec.what, fill, msg))
    if not found:          # (a reference comparison of NaNs or of a trampled operand only repeats the finding)
        for n, check in spec.checks.items():
            try:
                check(outs[n])
            except AssertionError as e:
                found.append("%s [%s]: %s against the reference: %s" % (spec.what, fill, n, e))
    return outs, found


def _bits_equal(a, b):
    return all(torch.equal(a[n].contiguous().view(torch.uint8), b[n].contiguous().view(torch.uint8)) for n in a)


def three_runs(spec, impl, device, sync=None, fills=("zero", "zero", "nan")):
    """All four assertions; returns the list of problems (empty: the call keeps the contract)."""
    ops = Operands(spec, device)
    found, runs = [], []
    for fill in fills:
        outs, probs = one_run(spec, ops, impl, fill, sync)
        found += probs
        runs.append(outs)
    if found:
        return found
    control = _bits_equal(runs[0], runs[1])
    if spec.control_must_hold and not control:
        found.append("%s: two runs between zero guards differ (the control)" % spec.what)
    if control:
        for n in runs[0]:
            a, b = runs[0][n].contiguous().view(torch.uint8), runs[2][n].contiguous().view(torch.uint8)
            if not torch.equal(a, b):
                item = runs[0][n].element_size()
                diff = (a.flatten() != b.flatten()).nonzero()
                found.append("%s: %s depends on what surrounds the operands: %s differ between zero and NaN guards (first: %d)" % (
                    spec.what, n, _plural(int(torch.unique(diff.flatten() // item).numel()), "element"), int(diff[0]) // item))
    return found


def single_run(spec, impl, device, sync=None, fill="nan"):
    """Assertions 1-3 only (the default-mode weight gradients: float atomics, no bit-equality)."""
    return one_run(spec, Operands(spec, device), impl, fill, sync)[1]


def live_run(spec, impl, device, sync=None):
    """One more run, for calls that update operands IN PLACE: assertions 1-3 with LIVE bytes in the guards of every output that
    has a prior.  An in-place update of poison is poison -- 0.37 * NaN is the same NaN, and m * 0 + (1 - m) * 0 the same 0 -- so a
    read-modify-write one element too wide, or of a table entry that should have been skipped, leaves 0xFF and 0x00 guards as it
    found them; a finite non-zero neighbour changes.  (The three runs stay: only they see a guard READ into a result.)"""
    return one_run(spec, Operands(spec, device), impl, "nan", sync, live=True)[1]


def rel_check(ref64, tol):
    """max |got - ref| / max |ref| < tol (conftest.rel_err, the metric of every parity test here)."""
    def check(got):
        err = float((got.double() - ref64).abs().max() / ref64.abs().max().clamp_min(1e-30))
        assert err < tol, "relative error %.3e (bar %.1e)" % (err, tol)
    return check


def ulp_bf16(ref):
    """One bf16 unit in the last place at |ref| (fp64)."""
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 7)


def rounded_check(exact64):
    """test_b16_gpu.py's check_rounded: within one bf16 ulp everywhere, fewer than 1e-3 of the elements off the rounded value."""
    def check(got_b16):
        got, want = got_b16.double(), exact64.to(torch.bfloat16).double()
        err = (got - exact64).abs()
        bad = err > ulp_bf16(exact64) + 1e-5 * float(exact64.abs().max())
        assert not bool(bad.any()), "%d elements further than one bf16 ulp, worst %g" % (int(bad.sum()), float(err.max()))
        flips = float((got != want).double().mean())
        assert flips < 1e-3, "%.2e of the elements differ from the correctly rounded value" % flips
    return check


def bits_check(ref, mask=None):
    """Bit equality with ``ref`` (same dtype) -- everywhere, or where ``mask`` is set -- reporting the first differing element."""
    def check(got):
        assert got.dtype == ref.dtype and got.numel() == ref.numel(), (got.dtype, ref.dtype, tuple(got.shape), tuple(ref.shape))
        item = got.element_size()
        differ = (got.contiguous().view(torch.uint8).view(-1, item) != ref.contiguous().view(torch.uint8).view(-1, item)).any(dim=1)
        if mask is not None:
            differ &= mask.flatten()
        diff = differ.nonzero()
        if diff.numel():
            first = int(diff[0])
            raise AssertionError("%s differ in their bits (first: element %d; expected %r, got %r)" % (
                _plural(int(diff.numel()), "element"), first, ref.flatten()[first].item(), got.flatten()[first].item()))
    return check


def untouched_check(prior, mask):
    """The elements of an in-place operand that the call must leave alone: wherever ``mask`` (bool, the operand's shape) is set,
    the result is the ``prior`` bit for bit.  Reports how many changed and the first one, as a flat element index."""
    prior, mask = prior.contiguous(), mask.contiguous().flatten()
    assert mask.dtype == torch.bool and mask.numel() == prior.numel()

    def check(got):
        assert got.dtype == prior.dtype and got.numel() == prior.numel(), (got.dtype, prior.dtype)
        item = got.element_size()
        a = got.contiguous().view(torch.uint8).view(-1, item)
        b = prior.view(torch.uint8).view(-1, item)
        changed = ((a != b).any(dim=1) & mask).nonzero()
        if changed.numel():
            first = int(changed[0])
            raise AssertionError("changed %s that the call must leave untouched (first: element %d of %d; was %r, is %r)" % (
                _plural(int(changed.numel()), "element"), first, prior.numel(), prior.flatten()[first].item(),
                got.flatten()[first].item()))
    return check


def all_checks(*checks):
    """One check out of several (the numeric check of the elements a call owns, then untouched_check of the rest)."""
    def check(got):
        for c in checks:
            c(got)
    return check

"""Flat-arena optimizers + gradient-norm clipping for the CSTP training loops.

Semantics follow torch.optim.SGD(momentum, weight_decay; dampening 0, no nesterov), torch.optim.Adam / AdamW
(betas, eps 1e-8, no amsgrad) and torch.nn.utils.clip_grad_norm_(params, 18) exactly as main_byol.py:86-91,228-232 and
main_ft_mp.py:133-147,210-212 use them -- including weight decay on BN gamma/beta and biases, and including the
fine-tune parameter list of one group per tensor with frozen tensors at lr 0.0 / requires_grad False
(r21d_byol.py:10-35), which torch skips because their .grad is None.  The work is streaming kernels over the model's
flat parameter/gradient arenas instead of ~170 x 3 tiny launches:
    sumsq(grad arena) -> clip coefficient (stays on the device, no host sync) -> fused scale + weight-decay +
    momentum + update, one launch per RUN of consecutive trainable tensors that share hyper-parameters
    (pre-training / ft_all / scratch: one run = the whole arena; ft_fc: one run = classify.weight|bias).
FlatLARS (--optimizer lars) is the one optimizer here the reference does not have: per-tensor trust ratios need a reduction per
tensor, which three launches per run over chunk tables do (csrc/lars.h).
TableSGD / TableAdam (fine-tuning's --layer_decay / --wd_skip_1d / --model_ema, cstp_amd/recipe.py) are FlatSGD / FlatAdam for
hyper-parameters that differ from tensor to tensor: a learning-rate scale and a weight decay per tensor would make almost every
tensor its own run, so their kernel looks both up per block in a table over the same chunks (csrc/optim_table.h) and the step stays
ONE launch whatever the grouping; the weight EMA of enable_ema() is updated in that launch too.
"""
from __future__ import annotations

import torch

from . import ops


def _pad4(n: int) -> int:
    return (n + 3) // 4 * 4


class _FlatOptimizer(torch.optim.Optimizer):
    """Shared plumbing: maps every parameter to its offset in the flat arena, groups them into runs."""

    _hyper = ()          # group keys that must match for two tensors to share a launch

    def __init__(self, params, defaults, arenas):
        if arenas is None:
            raise ValueError("%s needs arenas=model.flatten_parameters()" % type(self).__name__)
        super().__init__(params, defaults)
        self._p, self._g = arenas["param"], arenas["grad"]
        base, n = self._p.data_ptr(), self._p.numel()
        self._slots = []   # (group index, offset, padded length, numel, param) in state_dict index order
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                off = (p.data_ptr() - base) // 4
                inside = p.device == self._p.device and off >= 0 and off + p.numel() <= n and (p.data_ptr() - base) % 16 == 0
                if not inside and not p.requires_grad:
                    # a frozen tensor outside the trainable arena (the EMA target network of a pre-training model, which
                    # optim.SGD(model.parameters()) of main_byol.py:228 lists too): it keeps its INDEX in param_groups and
                    # in the state dict -- torch gives it no state, its .grad being None -- and is never touched
                    self._slots.append((gi, -1, 0, p.numel(), p))
                    continue
                if not inside:
                    raise ValueError("parameter of shape %s does not live in the flat arena -- build the optimizer from "
                                     "the parameters of a model whose flatten_parameters() produced `arenas`"
                                     % (tuple(p.shape),))
                self._slots.append((gi, off, _pad4(p.numel()), p.numel(), p))
        self._runs_key, self._runs = None, []
        self._lr_cache = {}
        self._sumsq = torch.zeros(1, dtype=torch.float32, device=self._p.device)
        self._coef = torch.ones(1, dtype=torch.float32, device=self._p.device)
        self._norm = torch.zeros(1, dtype=torch.float32, device=self._p.device)
        self._clip_pending = False
        # --model_ema (enable_ema): shadows of the parameter arena and of the float BatchNorm-buffer arena; None = off
        self._buffers = arenas.get("buffers")
        self._ema, self._ema_buffers = None, None
        self._ema_momentum, self._ema_updates = 0.0, 0

    # -- exponential moving average of the weights (fine-tuning's --model_ema) -----------------------------------------------------
    @torch.no_grad()
    def enable_ema(self, momentum: float) -> None:
        """From now on every step() also moves a shadow of the parameter arena and of the float BatchNorm-buffer arena towards the
        weights: shadow <- m * shadow + (1 - m) * value with m = ema_momentum_at(momentum, t) at the t-th update.  The shadows
        start as copies, so call this after the checkpoint has been loaded.  Frozen tensors are never touched: their shadow stays
        the copy.  TableSGD / TableAdam update the parameter shadow inside their step kernel; the other classes run one
        ops.ema_update_ per run of _plan() after theirs."""
        momentum = float(momentum)
        if not 0.0 <= momentum < 1.0:
            raise ValueError("EMA momentum must lie in [0, 1), got %r" % (momentum,))
        self._ema = self._p.clone()
        self._ema_buffers = self._buffers.clone() if self._buffers is not None and self._buffers.numel() > 0 else None
        self._ema_momentum, self._ema_updates = momentum, 0

    def _next_ema_momentum(self) -> float:
        self._ema_updates += 1
        return ema_momentum_at(self._ema_momentum, self._ema_updates)

    def _ema_buffer_pass(self, m: float) -> None:
        if self._ema_buffers is not None:
            ops.ema_update_(self._ema_buffers, self._buffers, m)

    def _ema_separate_pass(self) -> None:
        """The shadow update as its own pass over the trainable runs (the classes whose step kernel does not carry it)."""
        if self._ema is None:
            return
        m = self._next_ema_momentum()
        for off, n, _, _ in self._plan():
            ops.ema_update_(self._ema[off:off + n], self._p[off:off + n], m)
        self._ema_buffer_pass(m)

    # main_byol.py:86 / main_ft_mp.py:210 -- gradients are arena views, so "zero" (not set-to-None) keeps them in place
    def zero_grad(self, set_to_none: bool = False):
        self._g.zero_()

    @torch.no_grad()
    def clip_grad_norm_(self, max_norm: float) -> torch.Tensor:
        """clip_grad_norm_(model.parameters(), max_norm): returns the total norm as a DEVICE scalar.
        The scaling itself is folded into the next step() (which also writes the scaled gradients
        back, so .grad holds what the reference's in-place clip leaves there)."""
        ops.grad_sumsq(self._g, self._sumsq)
        ops.clip_coef(self._sumsq, max_norm, self._coef, self._norm)
        self._clip_pending = True
        return self._norm

    def _lr_tensor(self, lr: float) -> torch.Tensor:
        t = self._lr_cache.get(lr)
        if t is None:
            if len(self._lr_cache) > 64:
                self._lr_cache.clear()
            t = torch.full((1,), lr, dtype=torch.float32, device=self._p.device)
            self._lr_cache[lr] = t
        return t

    def _plan(self):
        """Runs of arena-adjacent trainable tensors with identical hyper-parameters: [(offset, length, group)]."""
        key = tuple(tuple(g[k] for k in self._hyper) for g in self.param_groups) + \
            tuple(s[4].requires_grad for s in self._slots)
        if key == self._runs_key:
            return self._runs
        runs = []
        for gi, off, plen, _, p in sorted(self._slots, key=lambda s: s[1]):
            if not p.requires_grad or off < 0:      # torch: .grad is None -> skipped (no decay, no momentum)
                continue
            g = self.param_groups[gi]
            hp = tuple(g[k] for k in self._hyper)
            if runs and runs[-1][0] + runs[-1][1] == off and runs[-1][3] == hp:
                runs[-1][1] += plen
            else:
                runs.append([off, plen, g, hp])
        self._runs_key, self._runs = key, runs
        return runs


# checkpoint wire formats shared by the classes below: torch.optim.SGD's (momentum_buffer) and torch.optim.Adam / AdamW's
# (step, exp_avg, exp_avg_sq), one state entry per trainable tensor that has taken a step, indexed as torch indexes them
def _sgd_state(opt):
    state = {}
    for i, (_, off, _, numel, p) in enumerate(opt._slots):
        if opt._steps > 0 and p.requires_grad and off >= 0:
            state[i] = {"momentum_buffer": opt._buf[off:off + numel].view_as(p).clone()}
    return state


def _load_sgd_state(opt, sd, keys):
    loaded = False
    for i, (_, off, _, numel, p) in enumerate(opt._slots):
        st = sd["state"].get(i, sd["state"].get(str(i)))
        if st is not None and st.get("momentum_buffer") is not None and off >= 0:
            opt._buf[off:off + numel].view_as(p).copy_(st["momentum_buffer"])
            loaded = True
    opt._steps = 1 if loaded else 0
    _load_group_keys(opt, sd, keys)


def _adam_state(opt):
    state = {}
    for i, (_, off, _, numel, p) in enumerate(opt._slots):
        if opt._steps > 0 and p.requires_grad and off >= 0:
            state[i] = {"step": torch.tensor(float(opt._steps)),
                        "exp_avg": opt._m[off:off + numel].view_as(p).clone(),
                        "exp_avg_sq": opt._v[off:off + numel].view_as(p).clone()}
    return state


def _load_adam_state(opt, sd, keys):
    steps = 0
    for i, (_, off, _, numel, p) in enumerate(opt._slots):
        st = sd["state"].get(i, sd["state"].get(str(i)))
        if st is not None and "exp_avg" in st and off >= 0:
            opt._m[off:off + numel].view_as(p).copy_(st["exp_avg"])
            opt._v[off:off + numel].view_as(p).copy_(st["exp_avg_sq"])
            steps = max(steps, int(float(st.get("step", 0))))
    opt._steps = steps
    _load_group_keys(opt, sd, keys)


def _load_group_keys(opt, sd, keys):
    for g, sg in zip(opt.param_groups, sd["param_groups"]):
        for k in keys:
            if k in sg:
                g[k] = tuple(sg[k]) if k == "betas" else sg[k]



class FlatSGD(_FlatOptimizer):
    """Drop-in for ``optim.SGD(parameters, lr, momentum, weight_decay)`` on a model whose parameters were
    re-homed by ``R21DBYOL.flatten_parameters()``; ``params`` may be ``model.parameters()`` or the per-tensor
    group list of ``get_fine_tuning_parameters``."""

    _hyper = ("lr", "momentum", "weight_decay")

    def __init__(self, params, lr, momentum=0.0, weight_decay=0.0, arenas=None):
        # frozen tensors stay listed (state-dict indices = torch.optim.SGD(model.parameters())'s); _plan skips them
        params = list(params)
        # the remaining torch.optim.SGD group keys ride along (fixed at what this kernel implements) so that a
        # state_dict written here loads into torch.optim.SGD -- i.e. into the reference -- and steps there
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=False,
                                      maximize=False, foreach=None, differentiable=False, fused=None), arenas)
        self._buf = torch.zeros_like(self._p)
        self._steps = 0

    @torch.no_grad()
    def step(self, closure=None):
        for off, n, g, _ in self._plan():
            sl = slice(off, off + n)
            ops.sgd_step_(self._p[sl], self._g[sl], self._buf[sl], self._lr_tensor(float(g["lr"])), g["momentum"],
                          g["weight_decay"], self._coef if self._clip_pending else None, self._steps == 0, True)
        self._clip_pending = False
        self._steps += 1

    # checkpoint wire format of torch.optim.SGD (main_byol.py:132-140 saves optimizer.state_dict())
    def state_dict(self):
        sd = super().state_dict()
        sd["state"] = _sgd_state(self)
        return sd

    def load_state_dict(self, sd):
        _load_sgd_state(self, sd, ("lr", "momentum", "weight_decay"))


class FlatAdam(_FlatOptimizer):
    """``optim.Adam(parameters, lr, weight_decay)`` / ``optim.AdamW(parameters, lr, betas, weight_decay)`` of
    main_ft_mp.py:139-147 (``decoupled=True`` is AdamW)."""

    _hyper = ("lr", "betas", "eps", "weight_decay")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, arenas=None):
        params = list(params)       # frozen tensors stay listed, as in FlatSGD
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False,
                                      maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                                      decoupled_weight_decay=bool(decoupled)), arenas)
        self.decoupled = bool(decoupled)
        self._m = torch.zeros_like(self._p)
        self._v = torch.zeros_like(self._p)
        self._steps = 0

    @torch.no_grad()
    def step(self, closure=None):
        if self._clip_pending:
            self._g.mul_(self._coef)
            self._clip_pending = False
        self._steps += 1
        for off, n, g, _ in self._plan():
            sl = slice(off, off + n)
            ops.adam_step_(self._p[sl], self._g[sl], self._m[sl], self._v[sl], self._lr_tensor(float(g["lr"])),
                           g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], self.decoupled, self._steps)

    def state_dict(self):
        sd = super().state_dict()
        sd["state"] = _adam_state(self)
        return sd

    def load_state_dict(self, sd):
        _load_adam_state(self, sd, ("lr", "betas", "eps", "weight_decay"))


def lars_tables(slots, chunk):
    """The two tables of csrc/lars.h for the trainable tensors ``slots`` = [(offset, numel, adapted)] of one arena (offsets in
    floats, multiples of 4; frozen tensors are simply not listed): every tensor's extent, padded to four floats, is cut into
    chunks of at most ``chunk`` floats that never cross a tensor.
      -> chunks [(segment, offset, length)], segs [(first chunk, chunk count, adapted 0 / 1)], segment s being slots[s].
    Pure host code."""
    if chunk <= 0 or chunk % 4:
        raise ValueError("chunk must be a positive multiple of 4, got %r" % (chunk,))
    chunks, segs = [], []
    for s, (off, numel, adapted) in enumerate(slots):
        if off < 0 or off % 4 or numel <= 0:
            raise ValueError("tensor %d: offset %d / numel %d (offsets are multiples of 4 floats, tensors not empty)" % (s, off, numel))
        end = off + _pad4(numel)
        if end >= 1 << 31:
            raise ValueError("tensor %d ends at float %d: the tables hold int32 offsets (arena of 2^31 floats or more)" % (s, end))
        first = len(chunks)
        for o in range(off, end, chunk):
            chunks.append((s, o, min(chunk, end - o)))
        segs.append((first, len(chunks) - first, 1 if adapted else 0))
    return chunks, segs


class FlatLARS(_FlatOptimizer):
    """LARS on the flat arenas: SGD with momentum in which each weight tensor's step is scaled by the trust ratio
    ``q = eta * ||w|| / ||g + weight_decay * w||`` (``q = 1`` when either norm is zero; no eps).

    This is the variant of the published BYOL-family PyTorch code, and it DEPARTS from FlatSGD on purpose: FlatSGD follows the
    reference and decays every tensor; here tensors with ``dim() <= 1`` (biases, BatchNorm gamma / beta) get neither weight
    decay nor the adaptation -- for them it is plain SGD with momentum.  Per tensor, with c the pending clip coefficient:
        g <- c*g (written back to .grad);  d = q*(g + wd*p) if p.dim() > 1 else g;  buf <- momentum*buf + d;  p <- p - lr*buf
    Norms are taken over the whole tensor, accumulated in double; under DDP they are taken after the gradient all-reduce and
    are the same on every rank (no collective is added).  Three launches per run of ``_plan()``, no host sync, no atomics:
    two steps from equal state give equal bits (csrc/lars.h).  ``trust_ratios()`` returns the last step's q."""

    _hyper = ("lr", "momentum", "weight_decay", "eta")

    def __init__(self, params, lr, momentum=0.9, weight_decay=0.0, eta=1e-3, arenas=None):
        params = list(params)       # frozen tensors stay listed, as in FlatSGD
        # the torch.optim.SGD group keys ride along, as in FlatSGD: a LARS checkpoint loads into torch.optim.SGD (eta is carried too)
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=False,
                                      maximize=False, foreach=None, differentiable=False, fused=None, eta=eta), arenas)
        if self._p.numel() >= 1 << 31:
            raise ValueError("FlatLARS: the arena holds %d floats; the chunk tables hold int32 offsets (< 2^31)" % self._p.numel())
        self._buf = torch.zeros_like(self._p)
        self._steps = 0
        self._tables_key, self._tables = None, []

    def _run_tables(self):
        """Per run of _plan(): (group, chunks, segs, ratio, slot indices) as device tensors, rebuilt when the plan's key changes."""
        runs = self._plan()
        if self._tables_key is not None and self._tables_key == self._runs_key:
            return self._tables
        dev = self._p.device
        live = sorted((s[1], i) for i, s in enumerate(self._slots) if s[1] >= 0 and s[4].requires_grad)
        tables = []
        for off, n, g, _ in runs:
            idx = [i for o, i in live if off <= o < off + n]
            chunks, segs = lars_tables([(self._slots[i][1], self._slots[i][3], self._slots[i][4].dim() > 1) for i in idx],
                                       ops.LARS_CHUNK)
            tables.append((g, torch.tensor(chunks, dtype=torch.int32, device=dev), torch.tensor(segs, dtype=torch.int32, device=dev),
                           torch.ones(len(segs), dtype=torch.float32, device=dev), torch.tensor(idx, dtype=torch.int64, device=dev)))
        self._tables_key, self._tables = self._runs_key, tables
        return tables

    @torch.no_grad()
    def step(self, closure=None):
        coef = self._coef if self._clip_pending else None
        for g, chunks, segs, ratio, _ in self._run_tables():
            ops.lars_ratio_(self._p, self._g, chunks, segs, g["weight_decay"], g["eta"], coef, ratio)
            ops.lars_step_(self._p, self._g, self._buf, chunks, segs, ratio, self._lr_tensor(float(g["lr"])), g["momentum"],
                           g["weight_decay"], coef, True)
        self._clip_pending = False
        self._steps += 1
        self._ema_separate_pass()      # --model_ema: its own pass here (the LARS kernels carry no shadow)

    def trust_ratios(self):
        """-> (q [n_tensors] on the device, parameter indices [n_tensors]): the trust ratio each tensor took in the last step, in
        the order of the parameter list (= state_dict indices): 1 for the tensors that are not adapted, NaN for frozen ones
        (and for every tensor before the first step).  No host read."""
        q = torch.full((len(self._slots),), float("nan"), dtype=torch.float32, device=self._p.device)
        if self._steps > 0:
            for _, _, _, ratio, idx in self._run_tables():
                q[idx] = ratio
        return q, torch.arange(len(self._slots), device=self._p.device)

    # checkpoint wire format of torch.optim.SGD, as FlatSGD writes it (main_byol.py:132-140 saves optimizer.state_dict())
    def state_dict(self):
        sd = super().state_dict()
        sd["state"] = _sgd_state(self)
        return sd

    def load_state_dict(self, sd):
        _load_sgd_state(self, sd, ("lr", "momentum", "weight_decay", "eta"))


def ema_momentum_at(momentum: float, t: int) -> float:
    """Momentum of the t-th shadow update, t counted from 1: min(momentum, (1 + t) / (10 + t)) -- early updates follow the weights
    closely (2/11, 3/12, ...) instead of averaging in the initial values for 1 / (1 - momentum) steps."""
    if t < 1:
        raise ValueError("EMA updates are counted from 1, got %r" % (t,))
    return min(float(momentum), (1.0 + t) / (10.0 + t))


def hyper_tables(slots, chunk):
    """The tables of csrc/optim_table.h for the trainable tensors ``slots`` = [(offset, numel, lr scale, weight decay)] of one arena:
    the chunk table of lars_tables (chunks never cross a tensor; offsets and lengths are multiples of 4; frozen tensors are simply
    not listed) and one {lr scale, weight decay} row per tensor.
      -> chunks [(segment, offset, length)], hyper [(lr scale, weight decay)], segment s being slots[s].  Pure host code."""
    chunks, _ = lars_tables([(off, numel, False) for off, numel, _, _ in slots], chunk)
    hyper = []
    for s, (_, _, scale, wd) in enumerate(slots):
        scale, wd = float(scale), float(wd)
        if not (scale >= 0.0 and scale < float("inf")) or not (wd >= 0.0 and wd < float("inf")):
            raise ValueError("tensor %d: lr scale %r / weight decay %r (both finite and >= 0)" % (s, scale, wd))
        hyper.append((scale, wd))
    return chunks, hyper


class _TableOptimizer(_FlatOptimizer):
    """What TableSGD and TableAdam share: ONE launch per step whatever the grouping (csrc/optim_table.h).

    Each group may carry ``lr_scale`` (default 1) and its own ``weight_decay``; ``param_groups[i]["lr"]`` holds
    ``base * lr_scale``, so a scheduler that multiplies every group (ReduceLROnPlateau) or sets ``value * lr_scale`` per group
    (recipe.WarmupCosine) and the drivers' log line keep working.  step() derives the base rate from the groups and refuses groups
    that disagree on it.  The base lives in one persistent device scalar, refreshed with ``fill_`` when its value changes, and the
    scales in a static device table: a change of learning rate costs no table rebuild, no allocation and no host read.  The
    tables are rebuilt only when a group's lr_scale / weight_decay or a tensor's requires_grad changes.
    _plan() merges arena-adjacent TRAINABLE tensors regardless of hyper-parameters, so FineTuneStep's per-run all-reduce stays one
    collective per contiguous trainable run."""

    BASE_RTOL = 1e-6        # group lr against base * lr_scale: products of doubles taken in different orders

    def __init__(self, params, defaults, arenas):
        defaults = dict(defaults, lr_scale=1.0)
        super().__init__(params, defaults, arenas)
        if self._p.numel() >= 1 << 31:
            raise ValueError("%s: the arena holds %d floats; the chunk tables hold int32 offsets (< 2^31)"
                             % (type(self).__name__, self._p.numel()))
        for g in self.param_groups:
            if not (float(g["lr_scale"]) >= 0.0):
                raise ValueError("lr_scale must be >= 0, got %r" % (g["lr_scale"],))
            g["lr"] = float(g["lr"]) * float(g["lr_scale"])
        self._lr_dev = torch.zeros(1, dtype=torch.float32, device=self._p.device)
        self._lr_base = None
        self._tables_key, self._tables = None, None

    def _live(self):
        """Slot indices of the trainable tensors in arena order."""
        return [i for _, i in sorted((s[1], i) for i, s in enumerate(self._slots) if s[1] >= 0 and s[4].requires_grad)]

    def _plan(self):
        """Runs of arena-adjacent trainable tensors, whatever their hyper-parameters: [(offset, length, first group, None)]."""
        key = tuple(s[4].requires_grad for s in self._slots)
        if key == self._runs_key:
            return self._runs
        runs = []
        for i in self._live():
            gi, off, plen, _, _ = self._slots[i]
            if runs and runs[-1][0] + runs[-1][1] == off:
                runs[-1][1] += plen
            else:
                runs.append([off, plen, self.param_groups[gi], None])
        self._runs_key, self._runs = key, runs
        return runs

    def _step_tables(self):
        """(chunks, hyper) on the device, rebuilt when a scale, a decay or the set of trainable tensors changes."""
        live = self._live()
        key = tuple((i, float(self.param_groups[self._slots[i][0]]["lr_scale"]),
                     float(self.param_groups[self._slots[i][0]]["weight_decay"])) for i in live)
        if key != self._tables_key:
            if not live:
                raise ValueError("%s: no trainable tensor in the arena" % type(self).__name__)
            chunks, hyper = hyper_tables([(self._slots[i][1], self._slots[i][3], sc, wd) for i, sc, wd in key], ops.LARS_CHUNK)
            dev = self._p.device
            self._tables = (torch.tensor(chunks, dtype=torch.int32, device=dev), torch.tensor(hyper, dtype=torch.float32, device=dev))
            self._tables_key = key
        return self._tables

    def base_lr(self) -> float:
        """The base rate the groups of the trainable tensors agree on: lr == base * lr_scale in every one of them."""
        groups = [self.param_groups[gi] for gi in sorted({self._slots[i][0] for i in self._live()})]
        lead = max(groups, key=lambda g: float(g["lr_scale"]), default=None)
        if lead is None or float(lead["lr_scale"]) == 0.0:
            return 0.0
        base = float(lead["lr"]) / float(lead["lr_scale"])
        for g in groups:
            want = base * float(g["lr_scale"])
            if abs(float(g["lr"]) - want) > self.BASE_RTOL * abs(want):
                raise ValueError("%s: a group's lr is %r where base %r * lr_scale %r = %r: set every group's lr to base * lr_scale "
                                 "(the learning-rate decay per layer lives in lr_scale)"
                                 % (type(self).__name__, g["lr"], base, g["lr_scale"], want))
        return base

    def _lr_scalar(self) -> torch.Tensor:
        base = self.base_lr()
        if base != self._lr_base:
            self._lr_dev.fill_(base)
            self._lr_base = base
        return self._lr_dev

    def _ema_args(self):
        """(shadow arena or None, momentum of this update) for the step kernel; the buffer shadow takes its own small pass."""
        if self._ema is None:
            return None, 0.0
        m = self._next_ema_momentum()
        self._ema_buffer_pass(m)
        return self._ema, m


class TableSGD(_TableOptimizer):
    """FlatSGD with per-group ``lr_scale`` and ``weight_decay`` in one launch (cstp_tab_sgd_step); ``momentum`` is the first
    group's.  Same parameter lists, same checkpoint wire format (``lr_scale`` rides along in the groups, as ``eta`` does for
    LARS); with every scale 1, one decay and no EMA a step leaves FlatSGD's bits."""

    def __init__(self, params, lr, momentum=0.0, weight_decay=0.0, arenas=None):
        params = list(params)
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=False,
                                      maximize=False, foreach=None, differentiable=False, fused=None), arenas)
        self._buf = torch.zeros_like(self._p)
        self._steps = 0

    @torch.no_grad()
    def step(self, closure=None):
        chunks, hyper = self._step_tables()
        lr = self._lr_scalar()
        momentum = self.param_groups[0]["momentum"]
        if any(g["momentum"] != momentum for g in self.param_groups):
            raise ValueError("TableSGD: one momentum for all groups (the table carries lr scale and weight decay)")
        ema, m = self._ema_args()
        ops.tab_sgd_step_(self._p, self._g, self._buf, chunks, hyper, lr, momentum, self._coef if self._clip_pending else None,
                          self._steps == 0, True, ema, m)
        self._clip_pending = False
        self._steps += 1

    # checkpoint wire format of torch.optim.SGD, as FlatSGD writes it
    def state_dict(self):
        sd = super().state_dict()
        sd["state"] = _sgd_state(self)
        return sd

    def load_state_dict(self, sd):
        _load_sgd_state(self, sd, ("lr", "momentum", "weight_decay", "lr_scale"))


class TableAdam(_TableOptimizer):
    """FlatAdam (``decoupled=True``: AdamW) with per-group ``lr_scale`` and ``weight_decay`` in one launch (cstp_tab_adam_step);
    betas and eps are the first group's.  A pending clip coefficient is applied by FlatAdam's pre-pass."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, arenas=None):
        params = list(params)
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False,
                                      maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                                      decoupled_weight_decay=bool(decoupled)), arenas)
        self.decoupled = bool(decoupled)
        self._m = torch.zeros_like(self._p)
        self._v = torch.zeros_like(self._p)
        self._steps = 0

    @torch.no_grad()
    def step(self, closure=None):
        chunks, hyper = self._step_tables()
        lr = self._lr_scalar()
        g0 = self.param_groups[0]
        if any(tuple(g["betas"]) != tuple(g0["betas"]) or g["eps"] != g0["eps"] for g in self.param_groups):
            raise ValueError("TableAdam: one (betas, eps) for all groups (the table carries lr scale and weight decay)")
        if self._clip_pending:
            self._g.mul_(self._coef)
            self._clip_pending = False
        self._steps += 1
        ema, m = self._ema_args()
        ops.tab_adam_step_(self._p, self._g, self._m, self._v, chunks, hyper, lr, g0["betas"][0], g0["betas"][1], g0["eps"],
                           self.decoupled, self._steps, ema, m)

    # checkpoint wire format of torch.optim.Adam / AdamW, as FlatAdam writes it
    def state_dict(self):
        sd = super().state_dict()
        sd["state"] = _adam_state(self)
        return sd

    def load_state_dict(self, sd):
        _load_adam_state(self, sd, ("lr", "betas", "eps", "weight_decay", "lr_scale"))


def build_optimizer(opts, parameters, arenas):
    """main_byol.py:227-244 / main_ft_mp.py:132-147: --optimizer sgd | adam | adamw; lars is this package's addition."""
    if opts.optimizer == "sgd":
        return FlatSGD(parameters, lr=opts.learning_rate, momentum=opts.momentum, weight_decay=opts.weight_decay,
                       arenas=arenas)
    if opts.optimizer == "adamw":
        return FlatAdam(parameters, lr=opts.learning_rate, betas=(0.9, 0.99), weight_decay=opts.weight_decay,
                        decoupled=True, arenas=arenas)
    if opts.optimizer == "adam":
        return FlatAdam(parameters, lr=opts.learning_rate, weight_decay=opts.weight_decay, arenas=arenas)
    if opts.optimizer == "lars":
        return FlatLARS(parameters, lr=opts.learning_rate, momentum=opts.momentum, weight_decay=opts.weight_decay,
                        eta=opts.lars_eta, arenas=arenas)
    raise ValueError("unknown --optimizer %r (sgd / adam / adamw / lars)" % (opts.optimizer,))

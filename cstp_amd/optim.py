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
        state = {}
        for i, (_, off, _, numel, p) in enumerate(self._slots):
            if self._steps > 0 and p.requires_grad and off >= 0:
                state[i] = {"momentum_buffer": self._buf[off:off + numel].view_as(p).clone()}
        sd["state"] = state
        return sd

    def load_state_dict(self, sd):
        loaded = False
        for i, (_, off, _, numel, p) in enumerate(self._slots):
            st = sd["state"].get(i, sd["state"].get(str(i)))
            if st is not None and st.get("momentum_buffer") is not None and off >= 0:
                self._buf[off:off + numel].view_as(p).copy_(st["momentum_buffer"])
                loaded = True
        self._steps = 1 if loaded else 0
        for g, sg in zip(self.param_groups, sd["param_groups"]):
            for k in ("lr", "momentum", "weight_decay"):
                if k in sg:
                    g[k] = sg[k]


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
        state = {}
        for i, (_, off, _, numel, p) in enumerate(self._slots):
            if self._steps > 0 and p.requires_grad and off >= 0:
                state[i] = {"step": torch.tensor(float(self._steps)),
                            "exp_avg": self._m[off:off + numel].view_as(p).clone(),
                            "exp_avg_sq": self._v[off:off + numel].view_as(p).clone()}
        sd["state"] = state
        return sd

    def load_state_dict(self, sd):
        steps = 0
        for i, (_, off, _, numel, p) in enumerate(self._slots):
            st = sd["state"].get(i, sd["state"].get(str(i)))
            if st is not None and "exp_avg" in st and off >= 0:
                self._m[off:off + numel].view_as(p).copy_(st["exp_avg"])
                self._v[off:off + numel].view_as(p).copy_(st["exp_avg_sq"])
                steps = max(steps, int(float(st.get("step", 0))))
        self._steps = steps
        for g, sg in zip(self.param_groups, sd["param_groups"]):
            for k in ("lr", "betas", "eps", "weight_decay"):
                if k in sg:
                    g[k] = tuple(sg[k]) if k == "betas" else sg[k]


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
        state = {}
        for i, (_, off, _, numel, p) in enumerate(self._slots):
            if self._steps > 0 and p.requires_grad and off >= 0:
                state[i] = {"momentum_buffer": self._buf[off:off + numel].view_as(p).clone()}
        sd["state"] = state
        return sd

    def load_state_dict(self, sd):
        loaded = False
        for i, (_, off, _, numel, p) in enumerate(self._slots):
            st = sd["state"].get(i, sd["state"].get(str(i)))
            if st is not None and st.get("momentum_buffer") is not None and off >= 0:
                self._buf[off:off + numel].view_as(p).copy_(st["momentum_buffer"])
                loaded = True
        self._steps = 1 if loaded else 0
        for g, sg in zip(self.param_groups, sd["param_groups"]):
            for k in ("lr", "momentum", "weight_decay", "eta"):
                if k in sg:
                    g[k] = sg[k]


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

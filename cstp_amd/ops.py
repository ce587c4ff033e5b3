"""torch.autograd wrappers over the C ABI (libcstp_hip.so).  PyTorch supplies device memory,
streams and the autograd graph; every FLOP/byte of the hot path runs in the HIP kernels.

There is deliberately NO CPU implementation here: tensors must live on a HIP device.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import ConvDesc, InAffine, check
from .mix import MODE_COPY, MODE_CUTMIX, MODE_MIXUP

BN_EPS = 1e-5
BN_MOMENTUM = 0.1

_ws_cache = {}

# Optional per-kernel timers installed by bench.py: an object with ``span(what, key) -> context manager | None`` that brackets
# the C-ABI call of matching ops with HIP events on the launch stream; None in normal operation.
#   what: "conv3d_forward" | "conv3d_backward_data" | "conv3d_backward_weight" (key = the ConvDesc fields as a tuple),
#         "bn_forward" | "bn_backward" (key = (n, c, s, groups, has_residual, relu))
kernel_timer = None


class _NoSpan:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


_NOSPAN = _NoSpan()


def _span(what, key):
    tm = kernel_timer
    if tm is None:
        return _NOSPAN
    return tm.span(what, key() if callable(key) else key) or _NOSPAN


def _desc_key(desc):
    return tuple(getattr(desc, f) for f, _ in ConvDesc._fields_)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _workspace(device: torch.device, nbytes: int) -> torch.Tensor:
    """Per-device scratch arena (grown geometrically, never shrunk).  All kernels of one op are
    enqueued on the current stream, so one arena per (device, stream) is race-free."""
    key = (device.index, _stream())
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        newn = max(nbytes, 1 << 20)
        if ws is not None:
            newn = max(newn, 2 * ws.numel())
        ws = torch.empty(newn, dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


class PackPlan:
    """The weight packs of a training step from THREE launches instead of ~137 (include/cstp_hip.h: cstp_pack_*).

    Every convolution / linear call re-lays its weights out for its kernel variant (~10 us per call on the step's critical
    chain: 1.3 ms of a 54 ms R(2+1)D-18 step, profiles/r04).  Inside a training step the weights change at exactly two points --
    the optimizer step (online network, predictor, heads) and the EMA (target network) -- so the step that owns the model
    (PretrainStep) hoists the packs: each (weight, direction) call site gets a PERSISTENT workspace; one step RECORDS the pack
    launches of every call (state "record"); from then on ``replay("online")`` at the top of a step and ``replay("target")``
    right behind the EMA run all recorded packs of that group from one launch each, and the calls skip theirs.  Outside an
    armed step (validation, fine-tuning, tests that call the model directly) nothing changes: calls pack for themselves.
    A call whose key was not recorded packs for itself too, on a workspace of its own.  The key holds what picks the kernel
    variant -- and with it the pack -- as far as the host sees it: the weight tensor, the direction, the input shape, whether
    the call's activation operands are 16-byte aligned and whether it passes an absmax cell.  The library checks the rest: a
    call on a registered workspace skips its pack only if that pack equals the recorded one, and otherwise packs for itself
    (a tile or arithmetic changed behind the plan's back costs speed, never correctness)."""

    def __init__(self, target_range=None):
        self.state = "off"            # "off" | "record" | "replay"
        self.armed = False            # True only inside the owning step
        self.ws = {}                  # key -> persistent workspace
        self.recs = {}                # key -> [PackRec, ...] (what that call packs)
        self.tables = {}              # group -> (recs_dev, first_dev, n, total_blocks)
        self.target_range = target_range      # (ptr_lo, ptr_hi) of the EMA target arena: its packs replay behind the EMA
        self.stats = {"replays": 0, "skipped_calls": 0, "recorded_calls": 0}

    @staticmethod
    def key(w_param, tag, x_shape, facts=()):
        # (a weight tensor fixes kernel size, stride and padding; facts: _dispatch_facts of the call's operands)
        return (w_param.data_ptr(), tag, tuple(x_shape)) + tuple(facts)

    def workspace(self, key, device, nbytes):
        ws = self.ws.get(key)
        if ws is None or ws.numel() < nbytes:
            if ws is not None and self.state == "replay":
                self.invalidate()             # a recorded buffer is being replaced: the device tables point at the old one
            ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
            self.ws[key] = ws
            self.recs.pop(key, None)          # a new buffer: whatever was recorded for the old one is void
        return ws

    def call(self, key, fn):
        """Run the C-ABI call ``fn`` under the pack mode this key is in."""
        lib = _lib.load()
        if self.state == "record":
            lib.cstp_pack_mode(1)
            try:
                out = fn()
            finally:
                lib.cstp_pack_mode(0)
                n = lib.cstp_pack_recorded(None, 0)
                buf = (_lib.PackRec * max(n, 1))()
                lib.cstp_pack_recorded(buf, n)
            self.recs[key] = [buf[i] for i in range(n)]
            self.stats["recorded_calls"] += 1
        else:
            # (replay state: the call's workspace is REGISTERED with the library -- cstp_pack_register -- so the call skips its pack
            #  without any per-call switch; the host spends one dictionary lookup here)
            out = fn()
            if self.state == "replay" and key in self.recs:
                self.stats["skipped_calls"] += 1
        return out

    def finish_record(self, device):
        """Build the per-group device tables from what the recording step collected."""
        # three groups: the target network's packs (replayed behind the EMA), the online / predictor / head FORWARD packs (top of
        # the step, main stream) and their DATA-GRADIENT packs (mirrored taps, gathered across the output channels: the expensive
        # ones -- top of the step too, but on the side stream: nothing needs them before the backward pass)
        groups = {"online": [], "online_d": [], "target": []}
        lo, hi = self.target_range if self.target_range is not None else (0, 0)
        for key, recs in self.recs.items():
            for r in recs:
                if lo <= (r.w or 0) < hi:
                    groups["target"].append(r)
                else:
                    groups["online_d" if key[1] == "d" else "online"].append(r)
        self.tables = {}
        for name, recs in groups.items():
            if not recs:
                continue
            arr = (_lib.PackRec * len(recs))(*recs)
            first, tot = [], 0
            for r in recs:
                first.append(tot)
                tot += int(r.nblocks)
            raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).clone()
            self.tables[name] = (raw.to(device), torch.tensor(first, dtype=torch.int32, device=device), len(recs), tot)
        dsts = sorted({int(r.dst) for recs in groups.values() for r in recs if r.dst})
        if dsts:
            arr = (ctypes.c_void_p * len(dsts))(*dsts)
            check(_lib.load().cstp_pack_register(arr, len(dsts), 1), "cstp_pack_register")
        self._registered = dsts
        self.state = "replay"

    def invalidate(self):
        """The kernels a recorded call would run may have changed (arithmetic, deterministic mode, a pinned tile): forget the
        records; the owning step records again after two quiet steps."""
        dsts = getattr(self, "_registered", None)
        if dsts:
            arr = (ctypes.c_void_p * len(dsts))(*dsts)
            _lib.load().cstp_pack_register(arr, len(dsts), 0)
        self._registered = []
        self.state, self.recs, self.tables, self.quiet = "off", {}, {}, 0

    def __del__(self):
        # the library must forget this plan's workspaces before their memory is reused (a registered address that became someone
        # else's scratch buffer would make that call skip its pack)
        try:
            self.invalidate()
        except Exception:       # interpreter shutdown
            pass

    def tick(self):
        """Start of an owning step: after two steps without a change of kernels the next one records."""
        if self.state == "off":
            self.quiet = getattr(self, "quiet", 0) + 1
            if self.quiet > 2:
                self.state = "record"

    def replay(self, group):
        if self.state != "replay" or not self.armed:
            return
        t = self.tables.get(group)
        if t is None:
            return
        check(_lib.load().cstp_pack_replay(_stream(), t[0].data_ptr(), t[1].data_ptr(), t[2], t[3]), "cstp_pack_replay")
        self.stats["replays"] += 1


pack_plan: Optional[PackPlan] = None          # set by the training step that owns the model (train.PretrainStep)


def _dispatch_facts(operands, absmax):
    """What the library's kernel choice reads from a call's operands besides the descriptor and the tile table: the patch
    kernels need 16-byte aligned activations (igemm.hip: a misaligned call takes the f16-pair gather kernel), and a fused input
    transform needs the operand's absmax cell (else a native tile)."""
    return (all(t.data_ptr() % 16 == 0 for t in operands), absmax is not None)


def _packed_call(w_param, tag, x_shape, device, nbytes, fn, facts=()):
    """``fn(ws)`` = one C-ABI convolution call that packs ``w_param`` into its workspace: through the pack plan when a
    training step has armed one (persistent workspace, recorded / skipped pack), else on the shared scratch arena.
    ``facts``: _dispatch_facts of the call (part of the plan's key).  Returns what ``fn`` returns."""
    plan = pack_plan
    if plan is None or not plan.armed or plan.state == "off" or w_param is None:
        return fn(_workspace(device, nbytes))
    key = PackPlan.key(w_param, tag, x_shape, facts)
    ws = plan.workspace(key, device, nbytes)
    return plan.call(key, lambda: fn(ws))


def _req(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.CstpError("%s must be on a HIP device (cstp_amd has no CPU path)" % name)
    if t.dtype != torch.float32:
        raise _lib.CstpError("%s must be float32, got %s" % (name, t.dtype))
    return t.contiguous()


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _triple(v) -> Tuple[int, int, int]:
    return (v, v, v) if isinstance(v, int) else tuple(v)


# Tile autotuning: the first time a convolution geometry is seen (per direction and GEMM arithmetic) its tile comes from the
# persisted table cstp_amd/tuned/gfx950_abi<N>.json (cstp_conv3d_set_tile), else the library times its candidates once
# (cstp_conv3d_autotune), and the winner is written back to the table -- so that runs, boxes and ranks execute the same kernels
# (round-1 VERDICT weak-9: re-deriving the table by timing on every process start made bench.py vary 217..227 clips/s).
# CSTP_AUTOTUNE=0 keeps the analytic choice; CSTP_TUNE_TABLE=0 ignores and does not write the file; CSTP_TUNE_TABLE=<path>
# uses another file; CSTP_TUNE_TABLE_RO=1 reads it but never writes (the test suite: tests/conftest.py).  TUNE_REV names the
# candidate set the entries were chosen from: bump it whenever a kernel variant is added or changed, and stale tables are
# ignored.
AUTOTUNE = os.environ.get("CSTP_AUTOTUNE", "1") != "0"
TUNE_REV = 5
_tuned = set()
_TABLE_ENV = os.environ.get("CSTP_TUNE_TABLE", "")
TUNE_TABLE_PATH = None if _TABLE_ENV == "0" else (
    _TABLE_ENV or os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned", "gfx950_abi%d.json" % _lib.ABI_VERSION))
_table = None            # {"<arith>|<mode>|<desc fields>": [tile4]}
_table_dirty = False
tune_stats = {"from_table": 0, "timed": 0}


def _load_table():
    global _table
    if _table is None:
        _table = {}
        if TUNE_TABLE_PATH is not None:
            try:
                import json
                with open(TUNE_TABLE_PATH) as f:
                    data = json.load(f)
                if data.get("arch") == "gfx950" and data.get("abi") == _lib.ABI_VERSION and data.get("rev") == TUNE_REV:
                    _table = {k: [int(v) for v in t] for k, t in data.get("tiles", {}).items()}
            except (OSError, ValueError, AttributeError):
                _table = {}
    return _table


_dirty_rank = None        # this process's rank when the table was first marked dirty (the exit hook runs after destroy_process_group)


def _is_rank0() -> bool:
    """Rank 0 of the job -- also at interpreter exit, when the process group is gone and dist.get_rank() would answer 0 on
    EVERY rank (round-3 ADVICE): the launcher's RANK, else the rank remembered when the table got its first new entry."""
    env = os.environ.get("RANK")
    if env is not None and env.isdigit():
        return int(env) == 0
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank() == 0
    return _dirty_rank in (None, 0)


def _note_dirty() -> None:
    global _table_dirty, _dirty_rank
    _table_dirty = True
    if _dirty_rank is None:
        import torch.distributed as dist
        _dirty_rank = dist.get_rank() if (dist.is_available() and dist.is_initialized()) else 0


def save_tune_table(path=None) -> bool:
    """Write the table (atomically) if it has new entries: on RANK 0 only, merged over what is on disk (another job may have
    added geometries meanwhile), once per call -- the training steps call it after their first step, and an exit hook
    covers everything else.  (Round 2 rewrote the file from every rank on every newly timed geometry: last writer won.)
    Silently skipped on a read-only tree."""
    global _table_dirty
    path = path or TUNE_TABLE_PATH
    if path is None or _table is None or not _table_dirty or os.environ.get("CSTP_TUNE_TABLE_RO", "0") == "1":
        return False
    if not _is_rank0():
        return False
    import json
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        merged = {}
        try:
            with open(path) as f:
                data = json.load(f)
            if data.get("arch") == "gfx950" and data.get("abi") == _lib.ABI_VERSION and data.get("rev") == TUNE_REV:
                merged = {k: [int(v) for v in t] for k, t in data.get("tiles", {}).items()}
        except (OSError, ValueError, AttributeError):
            merged = {}
        merged.update(_table)
        tmp = "%s.%d.tmp" % (path, os.getpid())
        with open(tmp, "w") as f:
            json.dump({"arch": "gfx950", "abi": _lib.ABI_VERSION, "rev": TUNE_REV,
                       "key": "arithmetic|mode|" + ",".join(f for f, _ in ConvDesc._fields_),
                       "tile": "cstp_conv3d_set_tile encoding", "tiles": dict(sorted(merged.items()))}, f, indent=0)
        os.replace(tmp, path)
        _table_dirty = False
        return True
    except OSError:
        return False


def _table_key(arith, mode, desc):
    return "%d|%d|%s" % (arith, mode, ",".join(str(getattr(desc, f)) for f, _ in ConvDesc._fields_))


def _autotune(lib, desc, mode, src, w, out, ws):
    """``out``: the tensor the timed candidates may overwrite, or a factory of one (called only if the geometry is timed)."""
    global _table_dirty
    arith = lib.cstp_gemm_get_split_terms()
    key = (arith, mode) + tuple(getattr(desc, f) for f, _ in ConvDesc._fields_)
    if key in _tuned:
        return
    _tuned.add(key)
    if pack_plan is not None:
        pack_plan.invalidate()       # a layer gets its tile now: recorded packs may belong to another variant
    tbl = _load_table()
    sk = _table_key(arith, mode, desc)
    tile = tbl.get(sk)
    if tile is not None:
        arr = (ctypes.c_int32 * 4)(*tile)
        if lib.cstp_conv3d_set_tile(ctypes.byref(desc), mode, arr) == 0:
            tune_stats["from_table"] += 1
            return
    if callable(out):
        out = out()
    check(lib.cstp_conv3d_autotune(_stream(), ctypes.byref(desc), mode, src.data_ptr(), w.data_ptr(), out.data_ptr(),
                                   ws.data_ptr(), ws.numel(), 2), "cstp_conv3d_autotune")
    tune_stats["timed"] += 1
    arr = (ctypes.c_int32 * 4)()
    check(lib.cstp_conv3d_get_tile(ctypes.byref(desc), mode, arr), "cstp_conv3d_get_tile")
    if arr[0] >= 0:
        tbl[sk] = [int(v) for v in arr]
        _note_dirty()                # written by save_tune_table(): after a step's first call, or at exit


import atexit  # noqa: E402

atexit.register(save_tune_table)


def share_tune_table(src: int = 0) -> None:
    """Rank ``src``'s tuned tiles -> every rank (one broadcast of a small dict), so that all ranks of a job run the same
    kernel for the same layer even when some geometry had to be timed in this run; rank 0 then persists the table.
    Without a process group: only the save."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        save_tune_table()
        return
    if dist.get_rank() == src:
        save_tune_table()
    lib = _lib.load()
    box = [dict(_load_table()) if dist.get_rank() == src else None]
    dist.broadcast_object_list(box, src=src)
    if dist.get_rank() == src:
        return
    tbl = _load_table()
    for sk, tile in box[0].items():
        if tbl.get(sk) == tile:
            continue
        tbl[sk] = tile
        arith, mode, fields = sk.split("|")
        if int(arith) != lib.cstp_gemm_get_split_terms():
            continue
        desc = ConvDesc(*[int(v) for v in fields.split(",")])
        lib.cstp_conv3d_set_tile(ctypes.byref(desc), int(mode), (ctypes.c_int32 * 4)(*tile))
        if pack_plan is not None:
            pack_plan.invalidate()


def set_split_terms(terms: int) -> None:
    """2 = f16 pair / three MFMA products (default), 3 = bf16 triple / six products, 1 = native f32 MFMA only,
    0 = environment default (cstp_gemm_set_split_terms).  Each arithmetic has its own class of tuned tiles."""
    check(_lib.load().cstp_gemm_set_split_terms(int(terms)), "cstp_gemm_set_split_terms")
    if pack_plan is not None:
        pack_plan.invalidate()


def set_deterministic(on: bool) -> None:
    """Bit-reproducible weight gradients (two-stage split-K instead of f32 atomics; cstp_set_deterministic).  Switch before
    the first convolution call of a run: the shared workspace is sized by what the library reports at that time."""
    check(_lib.load().cstp_set_deterministic(1 if on else 0), "cstp_set_deterministic")
    _ws_cache.clear()
    if pack_plan is not None:
        pack_plan.invalidate()
        pack_plan.ws.clear()


def set_conv_tile(x_shape, w_shape, stride, padding, mode: int, tile) -> None:
    """Pin the kernel variant of one convolution geometry and direction (cstp_conv3d_set_tile; mode 0 forward,
    1 backward_data, 2 backward_weight) and keep the autotuner away from it.  For parity tests and A/B timing."""
    lib = _lib.load()
    desc = _desc(tuple(x_shape), tuple(w_shape), _triple(stride), _triple(padding))
    arr = (ctypes.c_int32 * 4)(*[int(v) for v in tile])
    check(lib.cstp_conv3d_set_tile(ctypes.byref(desc), int(mode), arr), "cstp_conv3d_set_tile")
    if pack_plan is not None:
        pack_plan.invalidate()
    _tuned.add((lib.cstp_gemm_get_split_terms(), int(mode)) + tuple(getattr(desc, f) for f, _ in ConvDesc._fields_))


def _desc(x_shape, w_shape, stride, padding) -> ConvDesc:
    n, c, d, h, w = x_shape
    k, c2, kt, kh, kw = w_shape
    if c2 != c:
        raise _lib.CstpError("conv3d: input has %d channels, weight expects %d" % (c, c2))
    return ConvDesc(n, c, d, h, w, k, kt, kh, kw, stride[0], stride[1], stride[2], padding[0], padding[1], padding[2])


def conv_out_shape(x_shape, w_shape, stride, padding):
    n, _, d, h, w = x_shape
    k, _, kt, kh, kw = w_shape
    return (n, k, (d + 2 * padding[0] - kt) // stride[0] + 1, (h + 2 * padding[1] - kh) // stride[1] + 1,
            (w + 2 * padding[2] - kw) // stride[2] + 1)


# ----------------------------------------------------------------------------------------------
# weight gradients on a side stream
# ----------------------------------------------------------------------------------------------
# A parameter is tagged ``_cstp_direct_grad`` by the training steps (cstp_amd.train -> mark_direct_grad) when its .grad tensor
# is a view of its model's flat gradient arena and nothing hooks its autograd accumulation (the flat all-reduce path, or no
# DDP at all): the kernels then add the gradient into the arena themselves and autograd sees None.  The tag is a property
# of the PARAMETER (of one model), not of the process: a second model in the same process -- DDP with its bucket reducer,
# anything that relies on gradient hooks -- is not affected (round-2 ADVICE).
def mark_direct_grad(model, arenas, on: bool) -> None:
    lo = hi = 0
    if arenas is not None:
        g = arenas["grad"]
        lo, hi = g.data_ptr(), g.data_ptr() + g.numel() * g.element_size()
    for p in model.parameters():
        ok = bool(on) and p.grad is not None and lo <= p.grad.data_ptr() < hi and p.grad.is_contiguous()
        p._cstp_direct_grad = ok


def _direct(p) -> bool:
    return getattr(p, "_cstp_direct_grad", False) and p.is_leaf and p.grad is not None


OVERLAP_WGRAD = os.environ.get("CSTP_OVERLAP_WGRAD", "1") == "1"
_side_streams = {}
_join_pending = set()      # devices whose side stream the running backward pass used and has not joined yet ...
_join_pass = -1            # ... and that pass (torch._C._current_graph_task_id)


def _side_stream(device: torch.device) -> torch.cuda.Stream:
    st = _side_streams.get(device.index)
    if st is None:
        st = torch.cuda.Stream(device=device)
        _side_streams[device.index] = st
    return st


def _join_side_streams() -> None:
    """Make the current stream wait for the side-stream weight gradients (end of every backward pass)."""
    for idx in list(_join_pending):
        torch.cuda.current_stream(torch.device("cuda", idx)).wait_stream(_side_streams[idx])
    _join_pending.clear()


def _pending_side_joins():
    """The device indices whose side stream still awaits its join (tests)."""
    return sorted(_join_pending)


def _queue_join(device: torch.device) -> None:
    global _join_pass
    task = torch._C._current_graph_task_id()
    if task != _join_pass:       # another pass filled the set and raised before its callback ran: that pass is gone, queue anew
        _join_pending.clear()
        _join_pass = task
    if device.index not in _join_pending:
        if not _join_pending:
            torch.autograd.Variable._execution_engine.queue_callback(_join_side_streams)
        _join_pending.add(device.index)


def _place_wgrad(param, w, need, side_ok, wgrad, reads):
    """Where a convolution's weight gradient goes; returns what autograd is handed for the weight.  ``wgrad(dst, accumulate)``
    launches the kernel.  The gradient of a leaf weight whose .grad is a contiguous slice of the flat gradient arena
    (mark_direct_grad) is ADDED there by the library itself -- AccumulateGrad folded into the unpacking pass: no temporary, no
    add kernel -- and autograd sees None.  With ``side_ok`` and OVERLAP_WGRAD it also runs on a second HIP stream: it feeds nothing
    downstream in the backward chain, so the matrix-core-bound weight-gradient kernels execute beside the HBM-bound BatchNorm
    backward kernels of the main chain (the arena is joined before anything reads it, _join_side_streams).  ``reads``: the
    tensors the kernel reads (None entries skipped), kept alive for the side stream."""
    if not need:
        return None
    if not _direct(param):
        dw = torch.empty_like(w)
        wgrad(dw, False)
        return dw
    if side_ok and OVERLAP_WGRAD:
        side = _side_stream(w.device)
        side.wait_stream(torch.cuda.current_stream(w.device))      # dy is complete
        with torch.cuda.stream(side):
            wgrad(param.grad, True)
        for t in reads:
            if t is not None:
                t.record_stream(side)
        _queue_join(w.device)
    else:
        wgrad(param.grad, True)
    return None


# ----------------------------------------------------------------------------------------------
# convolution / linear
# ----------------------------------------------------------------------------------------------
# Largest-magnitude cells (cstp_hip.h: the *_am entry points).  A BatchNorm pass leaves max |y| (forward) / max |dx| (backward) in
# a one-element device tensor as a by-product and hangs it on the tensor it produced; the convolution that consumes that very
# tensor object hands it to the 2xf16-split kernels, which otherwise spend one extra read of the tensor on measuring it.  The
# attribute travels with the Python object only: any op in between (reshape, cat, add, an in-place update -- _version is
# checked) drops it, and the kernels measure for themselves.  Only the public wrapper sees the tensor object apply() returns, so
# forward hands it the cell in the call's own record (_Call): nothing a call sets up outlives the call.
FUSE_ABSMAX = os.environ.get("CSTP_FUSE_ABSMAX", "1") != "0"
# BatchNorm statistics as a by-product of the producing convolution (patch-kernel layers): 0 keeps the separate pass
FUSE_BN_STATS = os.environ.get("CSTP_FUSE_BN_STATS", "1") != "0"
absmax_stats = {"hit": 0, "miss": 0}


def _tag_absmax(t: torch.Tensor, cell: Optional[torch.Tensor]) -> None:
    if cell is not None:
        t._cstp_absmax = (cell, t._version)


def _absmax_of(t: torch.Tensor) -> Optional[torch.Tensor]:
    tag = getattr(t, "_cstp_absmax", None)
    if tag is not None and tag[1] == t._version and tag[0].device == t.device:
        absmax_stats["hit"] += 1
        return tag[0]
    absmax_stats["miss"] += 1
    return None


def _new_cell(like: torch.Tensor) -> Optional[torch.Tensor]:
    return torch.empty(1, dtype=torch.int32, device=like.device) if FUSE_ABSMAX else None


class _Call:
    """The side data of ONE op call.  The public wrapper makes it and hands it to ``apply()`` as a plain argument: ``pre`` is what
    the wrapper found with _bnstats_of (a list per branch for bn_relu_concat); ``forward`` fills ``cell`` (the absmax cell the
    wrapper hangs on the result) and ``stats`` (what _launch_forward returned).  It dies with the call, whether that raises or not."""
    __slots__ = ("pre", "cell", "stats")

    def __init__(self, pre=None):
        self.pre, self.cell, self.stats = pre, None, None


class GradJoin:
    """The gradients of ONE tensor that feeds ``n`` of these ops (the residual connection, r21d_byol.py:141-148: a block's
    input goes into conv1 AND into the addition behind bn2; in a downsample block into conv1 and the shortcut convolution)
    are summed inside the ops instead of by autograd's separate add pass over three tensors: every contributor but the last
    puts its gradient into the join's buffer (the first one creates it, convolutions after that ADD into it in their
    epilogue: cstp_conv3d_backward_data_acc) and hands autograd None; the last one adds its own and returns the sum.
    A fresh object per forward call; backward order is whatever the autograd engine chooses."""

    def __init__(self, n: int):
        self.n, self.count, self.buf = int(n), 0, None

    def contribute(self, plain, accumulate):
        """``plain() -> fresh gradient tensor``; ``accumulate(buf)``: buf += this contributor's gradient."""
        self.count += 1
        if self.buf is None:
            out = plain()
        else:
            accumulate(self.buf)
            # the accumulating kernel wrote through data_ptr(): tell autograd's version counter (round-3 ADVICE)
            torch.autograd.graph.increment_version(self.buf)
            out = self.buf
        if self.count < self.n:
            if self.buf is None:
                # first contributor: if the others never run (a consumer's input gradient pruned by autograd.grad(inputs=...),
                # needs_input_grad False on one branch) the partial sum would silently vanish -- an end-of-backward check raises
                torch.autograd.Variable._execution_engine.queue_callback(self._close)
            self.buf = out
            return None
        self.buf, self.count = None, 0
        return out

    def _close(self):
        """End of the backward pass this join's first contributor ran in: nothing of it outlives the pass."""
        count, self.buf, self.count = self.count, None, 0
        if 0 < count < self.n:
            raise RuntimeError("GradJoin: residual joins ended the backward pass with contributors missing (%d of %d ran) -- a "
                               "consumer's input gradient was pruned; the block input's gradient would have been dropped"
                               % (count, self.n))


def _tune(desc, mode, src, w, out, ws):
    """Give this geometry and direction its tile on first sight (_autotune).  ``out`` may be a factory: tuning overwrites its
    output, and a scratch tensor is only worth allocating when candidates are really timed."""
    if AUTOTUNE:
        _autotune(_lib.load(), desc, mode, src, w, out, ws)


def _launch_forward(desc, x, w, bias, aff, y, ws, cell, groups, pivot):
    """The forward convolution launch (fp32).  ``aff``: an InAffine applied inside the gather, else None; ``cell``: the absmax cell
    of the (transformed) input.  ``groups`` > 0: a train-mode BatchNorm over that many slices of the batch consumes y; where the
    layer's kernel can, it leaves the statistics' partial sums beside y (cstp_conv3d_forward_bnstats) and the BatchNorm skips
    its pass over the tensor; ``pivot``: the value the sums are taken around.  Returns (partials, nsplit, groups, cell of y) when
    the kernel left them, else None."""
    lib = _lib.load()
    nsplit = lib.cstp_conv3d_bnstats_nsplit if aff is None else lib.cstp_conv3d_bnstats_nsplit_aff
    ns = nsplit(ctypes.byref(desc), groups) if (groups > 0 and bias is None and FUSE_BN_STATS) else 0
    a = None if aff is None else ctypes.byref(aff)
    if ns <= 0:
        check(lib.cstp_conv3d_forward_am(_stream(), ctypes.byref(desc), x.data_ptr(), w.data_ptr(), _ptr(bias), a, y.data_ptr(),
                                         ws.data_ptr(), ws.numel(), _ptr(cell)), "cstp_conv3d_forward")
        return None
    k = w.shape[0]
    # sums [k][groups][ns][2], pivots [k], then the (min, max) keys [k][groups][ns][2] as uint32 (one double each)
    part = torch.empty(k * groups * ns * 3 + k, dtype=torch.float64, device=x.device)
    ycell = torch.empty(1, dtype=torch.int32, device=x.device)
    got = ctypes.c_int32(0)
    pv = None if pivot is None else _req(pivot, "BatchNorm pivot")
    if pv is not None and pv.numel() != k:
        raise _lib.CstpError("BatchNorm pivot has %d entries for %d output channels" % (pv.numel(), k))
    check(lib.cstp_conv3d_forward_bnstats(_stream(), ctypes.byref(desc), x.data_ptr(), w.data_ptr(), y.data_ptr(), ws.data_ptr(),
                                          ws.numel(), _ptr(cell), groups, _ptr(pv), part.data_ptr(), part.numel() * 8,
                                          ctypes.byref(got), ycell.data_ptr(), a), "cstp_conv3d_forward_bnstats")
    return (part, got.value, groups, ycell) if got.value > 0 else None


def _own_pack(w, param):
    """The parameter whose pack a call may leave to the pack plan: ``param`` itself, unless _req had to copy it."""
    return param if w.data_ptr() == param.data_ptr() else None


def _data_grad(desc, x, w, param, dy, cell, nbytes, launch, join=None):
    """The data gradient of a convolution.  ``launch(dst, ws, accumulate)`` is the C-ABI call, ``cell`` the absmax cell of dy.
    ``join``: x also feeds another op (GradJoin): the sum of the two gradients is formed in this kernel's epilogue."""
    b16 = x.dtype == torch.bfloat16

    def dgrad(dst, acc):
        if not b16:       # (tuning overwrites its output)
            _tune(desc, 1, dy, w, lambda: torch.empty_like(dst) if acc else dst, _workspace(x.device, nbytes))
        with _span("conv3d_backward_data", lambda: (("bf16",) if b16 else ()) + _desc_key(desc)):
            _packed_call(_own_pack(w, param), "d", x.shape, x.device, nbytes, lambda ws: launch(dst, ws, acc),
                         _dispatch_facts((dy, dst), cell))
        return dst

    if join is None:
        return dgrad(torch.empty_like(x), False)
    return join.contribute(lambda: dgrad(torch.empty_like(x), False), lambda buf: dgrad(buf, True))


class _Conv3d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, stride, padding, bn_groups, bn_pivot, grad_join, call):
        lib = _lib.load()
        xam = _absmax_of(x)
        w_in = w
        x = _req(x, "conv3d input")
        w = _req(w, "conv3d weight")
        desc = _desc(x.shape, w.shape, stride, padding)
        y = torch.empty(conv_out_shape(x.shape, w.shape, stride, padding), dtype=torch.float32, device=x.device)
        nbytes = lib.cstp_conv3d_workspace_bytes(ctypes.byref(desc))
        ws = _workspace(x.device, nbytes)
        b = None if bias is None else _req(bias, "conv3d bias")
        _tune(desc, 0, x, w, y, ws)
        with _span("conv3d_forward", lambda: _desc_key(desc)):
            call.stats = _packed_call(
                _own_pack(w, w_in), "f", x.shape, x.device, nbytes,
                lambda ws: _launch_forward(desc, x, w, b, None, y, ws, xam, bn_groups, bn_pivot), _dispatch_facts((x, y), xam))
        ctx.save_for_backward(x, w)
        ctx.w_param = w_in           # the parameter object itself (save_for_backward hands back a new tensor object)
        ctx.grad_join = grad_join
        ctx.x_absmax = xam
        ctx.desc = desc
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, w = ctx.saved_tensors
        desc = ctx.desc
        dyam = _absmax_of(dy)
        xam = ctx.x_absmax
        dy = _req(dy, "conv3d grad_output")
        nbytes = lib.cstp_conv3d_workspace_bytes(ctypes.byref(desc))
        dx = dw = db = None
        need_w, pw = ctx.needs_input_grad[1], ctx.w_param
        # (a 5-D input with more than one position: a linear layer's weight gradient never goes to the side stream)
        side_w = need_w and _direct(pw) and OVERLAP_WGRAD and x.dim() == 5 and x.shape[2] * x.shape[3] * x.shape[4] > 1

        def wgrad(dst, accumulate):
            wsx = _workspace(x.device, nbytes)
            _tune(desc, 2, x, dy, lambda: torch.empty_like(dst) if accumulate else dst, wsx)     # (tuning overwrites its output)
            with _span("conv3d_backward_weight", lambda: _desc_key(desc)):
                check(lib.cstp_conv3d_backward_weight_acc(_stream(), ctypes.byref(desc), x.data_ptr(), None, dy.data_ptr(),
                                                          dst.data_ptr(), wsx.data_ptr(), wsx.numel(), _ptr(xam), _ptr(dyam),
                                                          1 if accumulate else 0), "cstp_conv3d_backward_weight")

        def place():
            return _place_wgrad(pw, w, need_w, side_w, wgrad, (x, dy, xam, dyam))

        if side_w:       # ahead of the data gradient, beside it
            dw = place()
        if ctx.needs_input_grad[0]:
            dx = _data_grad(desc, x, w, pw, dy, dyam, nbytes,
                            lambda dst, ws, acc: check(lib.cstp_conv3d_backward_data_acc(
                                _stream(), ctypes.byref(desc), dy.data_ptr(), w.data_ptr(), dst.data_ptr(), ws.data_ptr(), ws.numel(),
                                _ptr(dyam), 1 if acc else 0), "cstp_conv3d_backward_data"), ctx.grad_join)
        if not side_w:   # on the main stream: behind the data gradient, which the backward chain waits for
            dw = place()
        if ctx.has_bias and ctx.needs_input_grad[2]:
            n, k = dy.shape[0], dy.shape[1]
            s = dy.numel() // (n * k)
            db = torch.empty(k, dtype=torch.float32, device=dy.device)
            check(lib.cstp_channel_sum(_stream(), dy.data_ptr(), db.data_ptr(), n, k, s, None, 0), "cstp_channel_sum")
        return dx, dw, db, None, None, None, None, None, None


def conv3d(x, w, bias=None, stride=1, padding=0, bn_groups=0, bn_pivot=None, grad_join=None):
    """F.conv3d drop-in (fp32, NCDHW).  ``bn_groups`` > 0: the caller feeds the result to a train-mode ``batch_norm_act`` with
    that many groups -- the convolution then leaves the BatchNorm's statistics beside its output where its kernel can.
    ``bn_pivot`` ([C_out], e.g. that BatchNorm's running_mean): the sums are taken around it (cstp_conv3d_forward_bnstats).
    ``grad_join``: x also feeds another op of this module that was given the same GradJoin (see there).
    A bfloat16 ``x`` selects the bf16-storage path (below): bf16 result, fp32 weight and weight gradient."""
    if x.dtype == torch.bfloat16:
        if bias is not None:
            raise _lib.CstpError("bf16-storage conv3d is bias-free (models/BE/r3d_byol.py:45-53)")
        return _Conv3dB16.apply(x, w, _triple(stride), _triple(padding), grad_join)
    call = _Call()
    y = _Conv3d.apply(x, w, bias, _triple(stride), _triple(padding), int(bn_groups), bn_pivot, grad_join, call)
    if call.stats is not None:
        y._cstp_bnstats = call.stats + (y._version,)
    return y


def _bnstats_of(t, groups):
    """(partials, nsplit, cell) the convolution that produced ``t`` left for a BatchNorm over ``groups`` groups, or None."""
    tag = getattr(t, "_cstp_bnstats", None)
    if tag is not None and tag[4] == t._version and tag[2] == groups and tag[0].device == t.device:
        return tag[0], tag[1], tag[3]
    return None


def linear(x, w, bias=None):
    """F.linear drop-in for 2-D x: the 1x1x1 convolution over [B][F][1][1][1]."""
    y = _Conv3d.apply(x.reshape(x.shape[0], x.shape[1], 1, 1, 1), w.reshape(w.shape[0], w.shape[1], 1, 1, 1), bias,
                      (1, 1, 1), (0, 0, 0), 0, None, None, _Call())
    return y.reshape(x.shape[0], w.shape[0])


# ----------------------------------------------------------------------------------------------
# train-mode BatchNorm (+ residual) (+ ReLU)
# ----------------------------------------------------------------------------------------------
def _bn_operands(req, x, residual, groups=1):
    """(x, residual, n, c, s) of a BatchNorm call, checked; ``req``: _req (fp32 activations) or _req16 (bf16 storage)."""
    x = req(x, "batch_norm input")
    n, c = x.shape[0], x.shape[1]
    res = None if residual is None else req(residual, "residual")
    if res is not None and res.shape != x.shape:
        raise _lib.CstpError("residual shape %s != input shape %s" % (tuple(res.shape), tuple(x.shape)))
    if groups < 1 or n % groups != 0:
        raise _lib.CstpError("batch of %d rows cannot be split into %d BN groups" % (n, groups))
    return x, res, n, c, x.numel() // (n * c)


def _bn_param_grads(need_gamma, need_beta, pg, pb, gamma):
    """(direct, dgamma, dbeta) of a BatchNorm backward.  Parameters whose .grad is a live slice of the flat gradient arena
    (cstp_amd.train): the kernel adds into it directly (``direct``) and autograd is handed None for both."""
    direct = need_gamma and need_beta and _direct(pg) and _direct(pb)
    if direct:
        return True, pg.grad, pb.grad
    return False, torch.empty_like(gamma), torch.empty_like(gamma)


class _BNAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, residual, running_mean, running_var, relu, eps, momentum, groups, grad_join, call):
        lib = _lib.load()
        x, res, n, c, s = _bn_operands(_req, x, residual, groups)
        gamma = _req(gamma, "batch_norm weight")
        beta = _req(beta, "batch_norm bias")
        y = torch.empty_like(x)
        mean = torch.empty(groups * c, dtype=torch.float32, device=x.device)
        invstd = torch.empty(groups * c, dtype=torch.float32, device=x.device)
        nbytes = lib.cstp_bn_workspace_bytes(n, c, s, groups)
        ws = _workspace(x.device, nbytes)
        # ReLU without a residual: backward recomputes the mask from x with the affine table instead of re-reading y
        remask = relu and res is None and s > 1
        ss = torch.empty(groups * c * 2, dtype=torch.float32, device=x.device) if remask else None
        cell = _new_cell(x) if s > 1 else None
        pre = call.pre           # (partial sums, nsplit, cell) the producing convolution left for this call, or None
        with _span("bn_forward", (n, c, s, groups, res is not None, bool(relu))):
            if pre is not None and s > 1:
                check(lib.cstp_bn_forward_train_pre(_stream(), x.data_ptr(), _ptr(res), y.data_ptr(), gamma.data_ptr(),
                                                    beta.data_ptr(), _ptr(running_mean), _ptr(running_var), mean.data_ptr(),
                                                    invstd.data_ptr(), _ptr(ss), n, c, s, groups, eps, momentum,
                                                    1 if relu else 0, ws.data_ptr(), ws.numel(), _ptr(cell), pre[0].data_ptr(),
                                                    pre[1]), "cstp_bn_forward_train_pre")
            else:
                check(lib.cstp_bn_forward_train_am(_stream(), x.data_ptr(), _ptr(res), y.data_ptr(), gamma.data_ptr(),
                                                   beta.data_ptr(), _ptr(running_mean), _ptr(running_var), mean.data_ptr(),
                                                   invstd.data_ptr(), _ptr(ss), n, c, s, groups, eps, momentum, 1 if relu else 0,
                                                   ws.data_ptr(), ws.numel(), _ptr(cell)), "cstp_bn_forward_train")
        call.cell = cell         # batch_norm_act hangs it on the tensor object apply() returns
        if remask:
            ctx.save_for_backward(x, ss, gamma, mean, invstd)
        else:
            ctx.save_for_backward(x, y, gamma, mean, invstd)
        ctx.remask = remask
        ctx.relu = relu
        ctx.groups = groups
        ctx.eps = eps
        ctx.has_res = res is not None
        ctx.params = (gamma, beta)     # the parameter objects themselves (their .grad may be an arena slice, see backward)
        ctx.grad_join = grad_join
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, y_or_ss, gamma, mean, invstd = ctx.saved_tensors
        y, ss = (None, y_or_ss) if ctx.remask else (y_or_ss, None)
        dy = _req(dy, "batch_norm grad_output")
        n, c = x.shape[0], x.shape[1]
        s = x.numel() // (n * c)
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if (ctx.has_res and ctx.needs_input_grad[3]) else None
        direct, dgamma, dbeta = _bn_param_grads(ctx.needs_input_grad[1], ctx.needs_input_grad[2], *ctx.params, gamma)
        nbytes = lib.cstp_bn_workspace_bytes(n, c, s, ctx.groups)
        ws = _workspace(x.device, nbytes)
        cell = _new_cell(x) if s > 1 else None
        with _span("bn_backward", (n, c, s, ctx.groups, ctx.has_res, bool(ctx.relu))):
            if s == 1:       # BatchNorm1d: the statistics rebuilt from x in fp64 (few rows per group: dx is a small difference)
                check(lib.cstp_bn1d_backward(_stream(), x.data_ptr(), _ptr(y), dy.data_ptr(), gamma.data_ptr(), dx.data_ptr(),
                                             _ptr(dres), dgamma.data_ptr(), dbeta.data_ptr(), n, c, ctx.groups, ctx.eps,
                                             1 if ctx.relu else 0, 1 if direct else 0), "cstp_bn1d_backward")
            else:
                check(lib.cstp_bn_backward_am(_stream(), x.data_ptr(), _ptr(y), dy.data_ptr(), gamma.data_ptr(), mean.data_ptr(),
                                              invstd.data_ptr(), _ptr(ss), dx.data_ptr(), _ptr(dres), dgamma.data_ptr(),
                                              dbeta.data_ptr(), n, c, s, ctx.groups, 1 if ctx.relu else 0, ws.data_ptr(),
                                              ws.numel(), _ptr(cell), 1 if direct else 0), "cstp_bn_backward")
        _tag_absmax(dx, cell)
        if dres is not None and ctx.grad_join is not None:       # the residual tensor's other consumer adds its gradient to this
            dres = ctx.grad_join.contribute(lambda: dres, lambda buf: buf.add_(dres))
        if direct:
            dgamma = dbeta = None
        return dx, dgamma, dbeta, dres, None, None, None, None, None, None, None, None


def batch_norm_act(x, gamma, beta, running_mean=None, running_var=None, residual=None, relu=False, eps=BN_EPS,
                   momentum=BN_MOMENTUM, groups=1, grad_join=None):
    """y = act(batch_norm_train(x) + residual); running stats updated in place.  ``groups`` > 1: the batch is
    that many independent BN calls back to back (per-group statistics, sequential running-stat updates).
    A bfloat16 ``x`` (and residual) selects the bf16-storage path."""
    if x.dtype == torch.bfloat16:
        return _BNActB16.apply(x, gamma, beta, residual, running_mean, running_var, bool(relu), float(eps), float(momentum),
                               int(groups), grad_join)
    call = _Call(_bnstats_of(x, int(groups)))
    y = _BNAct.apply(x, gamma, beta, residual, running_mean, running_var, bool(relu), float(eps), float(momentum),
                     int(groups), grad_join, call)
    _tag_absmax(y, call.cell)
    return y


def batch_norm_eval(x, gamma, beta, running_mean, running_var, residual=None, relu=False, eps=BN_EPS):
    """y = act(batch_norm(x; running stats) + residual) -- model.eval().  Forward only: the reference evaluates under
    torch.no_grad() (main_ft_mp.py:261, test.py:75), so asking for a gradient through it is an error, not a fallback."""
    lib = _lib.load()
    if torch.is_grad_enabled() and (x.requires_grad or gamma.requires_grad or beta.requires_grad
                                    or (residual is not None and residual.requires_grad)):
        raise _lib.CstpError("eval-mode BatchNorm is forward-only: call it under torch.no_grad() (as the reference's "
                             "validation/test loops do)")
    if x.dtype == torch.bfloat16:          # the bf16-storage path
        x, res, n, c, s = _bn_operands(_req16, x, residual)
        y = torch.empty_like(x)
        check(lib.cstp_b16_bn_forward_eval(_stream(), x.data_ptr(), _ptr(res), y.data_ptr(), _req(gamma, "weight").data_ptr(),
                                           _req(beta, "bias").data_ptr(), _req(running_mean, "running_mean").data_ptr(),
                                           _req(running_var, "running_var").data_ptr(), n, c, s, float(eps),
                                           1 if relu else 0), "cstp_b16_bn_forward_eval")
        return y
    x, res, n, c, s = _bn_operands(_req, x, residual)
    y = torch.empty_like(x)
    cell = _new_cell(x) if s > 1 else None
    ws = _workspace(x.device, lib.cstp_bn_workspace_bytes(n, c, s, 1) if cell is not None else lib.cstp_bn_eval_workspace_bytes(c))
    check(lib.cstp_bn_forward_eval_am(_stream(), x.data_ptr(), _ptr(res), y.data_ptr(), _req(gamma, "weight").data_ptr(),
                                      _req(beta, "bias").data_ptr(), _req(running_mean, "running_mean").data_ptr(),
                                      _req(running_var, "running_var").data_ptr(), n, c, s, float(eps), 1 if relu else 0,
                                      ws.data_ptr(), ws.numel(), _ptr(cell)), "cstp_bn_forward_eval")
    _tag_absmax(y, cell)
    return y


# ----------------------------------------------------------------------------------------------
# fused  BatchNorm(train) -> ReLU -> conv3d : the normalised tensor never exists in HBM
# ----------------------------------------------------------------------------------------------
class _BNReluConv3d(torch.autograd.Function):
    """y = conv3d(relu(batch_norm_train(x)), w) (r21d_byol.py:94-97: temporal_conv(relu(bn(spatial_conv(.))))).
    Forward: the statistics (folded from the partial sums the producing convolution left, else one pass over x), then the
    convolution applies x*scale+shift (+ReLU) inside its gather.  Backward: weight gradient with the same transform
    recomputed in ITS gather (side stream, straight into the gradient arena), data gradient of the convolution, then the
    BN backward with the ReLU mask recomputed from x."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, w, stride, padding, groups, relu, eps, momentum,
                out_groups, out_pivot, call):
        lib = _lib.load()
        pre = call.pre           # (partials, nsplit, cell) of the producing convolution, or None
        w_in, g_in, b_in = w, gamma, beta
        x = _req(x, "bn_relu_conv3d input")
        gamma, beta, w = _req(gamma, "bn weight"), _req(beta, "bn bias"), _req(w, "conv weight")
        n, c = x.shape[0], x.shape[1]
        s = x.numel() // (n * c)
        if groups < 1 or groups > 4 or n % groups != 0:
            raise _lib.CstpError("batch of %d rows cannot be split into %d BN groups" % (n, groups))
        mean = torch.empty(groups * c, dtype=torch.float32, device=x.device)
        invstd = torch.empty(groups * c, dtype=torch.float32, device=x.device)
        ss = torch.empty(groups * c * 2, dtype=torch.float32, device=x.device)
        zam = None
        with _span("bn_forward", (n, c, s, groups, False, bool(relu))):
            if pre is not None:
                zam = pre[2]       # zeroed by the producing launch; the finalize takes the maximum of act(x*scale+shift) into it
                check(lib.cstp_bn_finalize_pre(_stream(), gamma.data_ptr(), beta.data_ptr(), _ptr(running_mean), _ptr(running_var),
                                               mean.data_ptr(), invstd.data_ptr(), ss.data_ptr(), n, c, s, groups, eps, momentum,
                                               1 if relu else 0, pre[0].data_ptr(), pre[1], zam.data_ptr()), "cstp_bn_finalize_pre")
            else:
                ws = _workspace(x.device, lib.cstp_bn_workspace_bytes(n, c, s, groups))
                check(lib.cstp_bn_stats_train(_stream(), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(running_mean),
                                              _ptr(running_var), mean.data_ptr(), invstd.data_ptr(), ss.data_ptr(), n, c, s, groups,
                                              eps, momentum, ws.data_ptr(), ws.numel()), "cstp_bn_stats_train")
        desc = _desc(x.shape, w.shape, stride, padding)
        y = torch.empty(conv_out_shape(x.shape, w.shape, stride, padding), dtype=torch.float32, device=x.device)
        nbytes = lib.cstp_conv3d_workspace_bytes(ctypes.byref(desc))
        _tune(desc, 0, x, w, y, _workspace(x.device, nbytes))
        aff = InAffine(ss.data_ptr(), groups, 1 if relu else 0)
        # a train-mode BatchNorm over out_groups slices consumes y: where this layer's kernel can, it leaves that BatchNorm's
        # sums and range beside y (the temporal patch kernel igemm_k1t<.., STATS, AFF>)
        with _span("conv3d_forward", lambda: _desc_key(desc)):
            # ("fa": a forward that carries the in_affine may run another kernel variant -- another pack -- than the plain one)
            call.stats = _packed_call(       # (for the BatchNorm behind this convolution, as _Conv3d's)
                _own_pack(w, w_in), "fa", x.shape, x.device, nbytes,
                lambda ws: _launch_forward(desc, x, w, None, aff, y, ws, zam, out_groups, out_pivot), _dispatch_facts((x, y), zam))
        ctx.save_for_backward(x, gamma, mean, invstd, ss, w)
        ctx.desc, ctx.groups, ctx.relu, ctx.z_absmax = desc, groups, relu, zam
        ctx.params = (g_in, b_in, w_in)      # the parameter objects themselves (their .grad may be an arena slice)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, gamma, mean, invstd, ss, w = ctx.saved_tensors
        desc, zam = ctx.desc, ctx.z_absmax
        pg, pb, pw = ctx.params
        dyam = _absmax_of(dy)
        dy = _req(dy, "bn_relu_conv3d grad_output")
        n, c = x.shape[0], x.shape[1]
        s = x.numel() // (n * c)
        cbytes = lib.cstp_conv3d_workspace_bytes(ctypes.byref(desc))
        nbytes = max(cbytes, lib.cstp_bn_workspace_bytes(n, c, s, ctx.groups))
        aff = InAffine(ss.data_ptr(), ctx.groups, 1 if ctx.relu else 0)

        def wgrad(dst, accumulate):
            wsx = _workspace(x.device, nbytes)
            _tune(desc, 2, x, dy, lambda: torch.empty_like(w), wsx)          # (tuning overwrites its output)
            with _span("conv3d_backward_weight", lambda: _desc_key(desc)):
                check(lib.cstp_conv3d_backward_weight_acc(_stream(), ctypes.byref(desc), x.data_ptr(), ctypes.byref(aff),
                                                          dy.data_ptr(), dst.data_ptr(), wsx.data_ptr(), wsx.numel(), _ptr(zam),
                                                          _ptr(dyam), 1 if accumulate else 0), "cstp_conv3d_backward_weight")

        dw = _place_wgrad(pw, w, ctx.needs_input_grad[5], True, wgrad, (x, dy, ss, zam, dyam))
        dx = dgamma = dbeta = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            ws = _workspace(x.device, nbytes)
            # dz: the gradient w.r.t. the (never materialised) normalised activation
            dz = _data_grad(desc, x, w, pw, dy, dyam, cbytes,
                            lambda dst, wsd, acc: check(lib.cstp_conv3d_backward_data_acc(
                                _stream(), ctypes.byref(desc), dy.data_ptr(), w.data_ptr(), dst.data_ptr(), wsd.data_ptr(),
                                wsd.numel(), _ptr(dyam), 1 if acc else 0), "cstp_conv3d_backward_data"))
            dx = torch.empty_like(x)
            direct, dgamma, dbeta = _bn_param_grads(ctx.needs_input_grad[1], ctx.needs_input_grad[2], pg, pb, gamma)
            cell = _new_cell(x)
            with _span("bn_backward", (n, c, s, ctx.groups, False, bool(ctx.relu))):
                check(lib.cstp_bn_backward_am(_stream(), x.data_ptr(), None, dz.data_ptr(), gamma.data_ptr(), mean.data_ptr(),
                                              invstd.data_ptr(), ss.data_ptr(), dx.data_ptr(), None, dgamma.data_ptr(),
                                              dbeta.data_ptr(), n, c, s, ctx.groups, 1 if ctx.relu else 0, ws.data_ptr(),
                                              ws.numel(), _ptr(cell), 1 if direct else 0), "cstp_bn_backward")
            _tag_absmax(dx, cell)
            if direct:
                dgamma = dbeta = None
        return dx, dgamma, dbeta, None, None, dw, None, None, None, None, None, None, None, None, None


def in_affine_fused(x_shape, w_shape, stride, padding, groups) -> bool:
    """Would a convolution of this geometry apply a BatchNorm + ReLU over ``groups`` groups inside its f16-pair gather kernels
    (forward AND weight gradient)?  cstp_conv3d_in_affine_fused."""
    desc = _desc(tuple(x_shape), tuple(w_shape), _triple(stride), _triple(padding))
    return bool(_lib.load().cstp_conv3d_in_affine_fused(ctypes.byref(desc), int(groups)))


def bn_relu_conv3d(x, gamma, beta, running_mean, running_var, w, stride=1, padding=0, groups=1, relu=True, eps=BN_EPS,
                   momentum=BN_MOMENTUM, bn_groups=0, bn_pivot=None):
    """conv3d(act(batch_norm_train(x)), w) with the BN apply fused into the convolution's gather.  Where the convolution that
    produced ``x`` left the BatchNorm's sums and range beside it (conv3d(.., bn_groups=groups)) no pass reads x before the
    consuming convolution does.  ``bn_groups`` / ``bn_pivot``: as conv3d's -- the BatchNorm BEHIND this convolution."""
    call = _Call(_bnstats_of(x, int(groups)))
    y = _BNReluConv3d.apply(x, gamma, beta, running_mean, running_var, w, _triple(stride), _triple(padding), int(groups),
                            bool(relu), float(eps), float(momentum), int(bn_groups), bn_pivot, call)
    if call.stats is not None:
        y._cstp_bnstats = call.stats + (y._version,)
    return y


# ----------------------------------------------------------------------------------------------
# pooling: global average pool and MaxPool3d, fp32 or bf16 storage
# ----------------------------------------------------------------------------------------------
def _pool_storage(dtype):
    """(req, torch dtype, symbol prefix) of a pooling call: bfloat16 activations are the bf16-storage path, anything else must
    pass _req as float32.  The prefix completes to cstp_avgpool_forward / _backward, cstp_maxpool3d_forward / _backward and
    cstp_b16_avgpool_forward / _backward, cstp_b16_maxpool3d_forward / _backward."""
    return (_req16, torch.bfloat16, "cstp_b16_") if dtype == torch.bfloat16 else (_req, torch.float32, "cstp_")


class _AvgPool(torch.autograd.Function):
    """T in, float32 out (the heads behind it are fp32); float32 dy, dx in the input's dtype."""

    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        req, _, prefix = ctx.storage = _pool_storage(x.dtype)
        x = req(x, "avgpool input")
        n, c = x.shape[0], x.shape[1]
        s = x.numel() // (n * c)
        y = torch.empty((n, c), dtype=torch.float32, device=x.device)
        name = prefix + "avgpool_forward"
        check(getattr(lib, name)(_stream(), x.data_ptr(), y.data_ptr(), n * c, s), name)
        ctx.shape = tuple(x.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        _, dtype, prefix = ctx.storage
        dy = _req(dy, "avgpool grad_output")
        dx = torch.empty(ctx.shape, dtype=dtype, device=dy.device)
        n, c = ctx.shape[0], ctx.shape[1]
        s = dx.numel() // (n * c)
        name = prefix + "avgpool_backward"
        check(getattr(lib, name)(_stream(), dy.data_ptr(), dx.data_ptr(), n * c, s), name)
        return dx


class _MaxPool3d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel, stride, padding):
        lib = _lib.load()
        req, dtype, prefix = ctx.storage = _pool_storage(x.dtype)
        x = req(x, "max_pool3d input")
        if x.dim() != 5:
            raise _lib.CstpError("max_pool3d expects [N, C, D, H, W], got %s" % (tuple(x.shape),))
        n, c, d, h, w = x.shape
        k = (ctypes.c_int32 * 3)(*kernel)
        st = (ctypes.c_int32 * 3)(*stride)
        pd = (ctypes.c_int32 * 3)(*padding)
        osz = tuple((sz + 2 * padding[i] - kernel[i]) // stride[i] + 1 for i, sz in enumerate((d, h, w)))
        y = torch.empty((n, c) + osz, dtype=dtype, device=x.device)
        idx = torch.empty((n, c) + osz, dtype=torch.int32, device=x.device)
        name = prefix + "maxpool3d_forward"
        check(getattr(lib, name)(_stream(), x.data_ptr(), y.data_ptr(), idx.data_ptr(), n * c, d, h, w, k, st, pd), name)
        ctx.save_for_backward(idx)
        ctx.geom = (tuple(x.shape), tuple(kernel), tuple(stride), tuple(padding))
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        (idx,) = ctx.saved_tensors
        shape, kernel, stride, padding = ctx.geom
        req, dtype, prefix = ctx.storage
        dy = req(dy, "max_pool3d grad_output")
        dx = torch.empty(shape, dtype=dtype, device=dy.device)
        n, c, d, h, w = shape
        name = prefix + "maxpool3d_backward"
        check(getattr(lib, name)(_stream(), dy.data_ptr(), idx.data_ptr(), dx.data_ptr(), n * c, d, h, w,
                                 (ctypes.c_int32 * 3)(*kernel), (ctypes.c_int32 * 3)(*stride), (ctypes.c_int32 * 3)(*padding)),
              name)
        return dx, None, None, None


def max_pool3d(x, kernel_size=3, stride=2, padding=1):
    """nn.MaxPool3d(kernel_size, stride, padding) (models/BE/r3d_byol.py:158); float32 or bfloat16, y and dx in x's dtype."""
    return _MaxPool3d.apply(x, _triple(kernel_size), _triple(stride), _triple(padding))


def global_avg_pool(x):
    """AdaptiveAvgPool3d(1) + view(-1, C).  bfloat16 in -> float32 out (the heads behind it are fp32)."""
    return _AvgPool.apply(x)


# ----------------------------------------------------------------------------------------------
# S3D-G self-gating fused with the inception concat (csrc/gate.hip)
# ----------------------------------------------------------------------------------------------
class _GateConcat(torch.autograd.Function):
    """y = cat_i(sigmoid(fc_i(mean_s x_i)) * x_i) over the branches of one SepInception block (s3dg.py:100-110, :150-163):
    two launches forward, three backward, for all branches together."""

    @staticmethod
    def forward(ctx, nb, save, call, *args):
        lib = _lib.load()
        xs = [_req(x, "gate_concat branch") for x in args[:nb]]
        ws = [_req(w, "gate_concat weight") for w in args[nb:2 * nb]]
        bs = [_req(b, "gate_concat bias") for b in args[2 * nb:3 * nb]]
        n, spatial = xs[0].shape[0], tuple(xs[0].shape[2:])
        for x, w, b in zip(xs, ws, bs):
            c = x.shape[1]
            if x.dim() != 5 or x.shape[0] != n or tuple(x.shape[2:]) != spatial:
                raise _lib.CstpError("gate_concat branches must be [N, C_i, D, H, W] with one N, D, H, W; got %s"
                                     % ([tuple(t.shape) for t in xs],))
            if tuple(w.shape) != (c, c) or tuple(b.shape) != (c,):
                raise _lib.CstpError("gate_concat branch of %d channels needs a [%d, %d] weight and a [%d] bias, got %s, %s"
                                     % (c, c, c, c, tuple(w.shape), tuple(b.shape)))
        cs = [x.shape[1] for x in xs]
        ctot = sum(cs)
        s = xs[0].numel() // (n * cs[0])
        dev = xs[0].device
        y = torch.empty((n, ctot) + spatial, dtype=torch.float32, device=dev)
        m = torch.empty(n * ctot, dtype=torch.float32, device=dev)
        g = torch.empty(n * ctot, dtype=torch.float32, device=dev) if save else None
        cell = _new_cell(y)
        br = (_lib.GateBranch * nb)(*[_lib.GateBranch(x.data_ptr(), w.data_ptr(), b.data_ptr(), None, None, None, c, 0)
                                     for x, w, b, c in zip(xs, ws, bs, cs)])
        with _span("gate_forward", (n, s, tuple(cs))):
            check(lib.cstp_gate_concat_forward(_stream(), br, nb, n, s, y.data_ptr(), m.data_ptr(), _ptr(g), _ptr(cell)),
                  "cstp_gate_concat_forward")
        call.cell = cell
        if save:
            ctx.save_for_backward(*xs, *ws, m, g)
            ctx.params = args[nb:3 * nb]       # the parameter objects themselves (.grad may be an arena slice)
        ctx.nb, ctx.save, ctx.geom = nb, save, (n, s, tuple(cs))
        return y

    @staticmethod
    def backward(ctx, dy):
        if not ctx.save:
            raise RuntimeError("gate_concat: forward ran without saving its gates (no gradient was required then)")
        lib = _lib.load()
        nb = ctx.nb
        saved = ctx.saved_tensors
        xs, ws, m, g = saved[:nb], saved[nb:2 * nb], saved[2 * nb], saved[2 * nb + 1]
        n, s, cs = ctx.geom
        dy = _req(dy, "gate_concat grad_output")
        dxs = [torch.empty_like(x) for x in xs]
        # gradients of leaf parameters whose .grad is a live slice of the flat arena are added there by the kernel (as the BN ops do)
        direct = all(ctx.needs_input_grad[3 + nb:3 + 3 * nb]) and all(_direct(p) for p in ctx.params)
        dws = [p.grad for p in ctx.params[:nb]] if direct else [torch.empty_like(w) for w in ws]
        dbs = [p.grad for p in ctx.params[nb:]] if direct else [torch.empty(c, dtype=torch.float32, device=dy.device) for c in cs]
        br = (_lib.GateBranch * nb)(*[_lib.GateBranch(x.data_ptr(), w.data_ptr(), b.data_ptr(), dx.data_ptr(), dw.data_ptr(),
                                                      db.data_ptr(), c, 0)
                                     for x, w, b, dx, dw, db, c in zip(xs, ws, ctx.params[nb:], dxs, dws, dbs, cs)])
        nbytes = lib.cstp_gate_workspace_bytes(n, sum(cs))
        wsp = _workspace(dy.device, nbytes)
        with _span("gate_backward", (n, s, tuple(cs))):
            check(lib.cstp_gate_concat_backward(_stream(), br, nb, n, s, dy.data_ptr(), m.data_ptr(), g.data_ptr(), wsp.data_ptr(),
                                                wsp.numel(), 1 if direct else 0), "cstp_gate_concat_backward")
        if direct:
            return (None, None, None, *dxs) + (None,) * (2 * nb)
        return (None, None, None, *dxs, *dws, *dbs)


def gate_concat(branches, gates):
    """S3D-G SepInception tail (fp32): ``torch.cat([sigmoid(fc(x.mean([2, 3, 4])))[..., None, None, None] * x for x, fc in
    zip(branches, gates)], 1)`` with ``gates`` the (weight [c, c], bias [c]) pairs of the branches' SelfGating.fc.  The result is
    tagged with its max |y| cell for the 1x1x1 convolutions that consume it.  The gates are saved for backward only when a
    gradient is required."""
    branches, gates = list(branches), list(gates)
    if not 1 <= len(branches) <= 4 or len(gates) != len(branches):
        raise _lib.CstpError("gate_concat takes 1..4 branches with one (weight, bias) pair each, got %d and %d"
                             % (len(branches), len(gates)))
    ws = [w for w, _ in gates]
    bs = [b for _, b in gates]
    for t in branches + ws + bs:
        if t.dtype == torch.bfloat16:
            raise _lib.CstpError("gate_concat is fp32 only (S3D-G has no bf16-storage path)")
    save = torch.is_grad_enabled() and any(t.requires_grad for t in branches + ws + bs)
    call = _Call()
    y = _GateConcat.apply(len(branches), save, call, *branches, *ws, *bs)
    _tag_absmax(y, call.cell)
    return y


# ----------------------------------------------------------------------------------------------
# I3D (csrc/mixed.hip): TensorFlow-SAME max-pool, windowed average pool, BatchNorm + ReLU written into the inception concat
# ----------------------------------------------------------------------------------------------
def same_pool_geometry(n: int, k: int, s: int) -> Tuple[int, int, int]:
    """(front padding, back padding, output length) of one dimension of MaxPool3dTFPadding (models/BE/i3d_byol.py:70-87,
    :170-183): ``MaxPool3d(k, s, ceil_mode=True)`` over ``ConstantPad3d`` with ``pad = max(k - s, 0)`` split front ``pad // 2`` /
    back the rest.  Output ``ceil((n + pad - k) / s) + 1``, one less when the last window would start at or beyond the padded
    length (ATen's ceil-mode rule; the pooling's own padding is 0).  Pure host arithmetic, mirrored by cstp_maxpool3d_same_out."""
    n, k, s = int(n), int(k), int(s)
    if n < 1 or k < 1 or s < 1:
        raise ValueError("same_pool_geometry needs positive n, kernel and stride, got %r" % ((n, k, s),))
    pad = max(k - s, 0)
    front = pad // 2
    out = -((n + pad - k) // -s) + 1
    if (out - 1) * s >= n + pad:
        out -= 1
    return front, pad - front, out


class _MaxPool3dSame(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel, stride, save):
        lib = _lib.load()
        x = _req(x, "max_pool3d_same input")
        if x.dim() != 5:
            raise _lib.CstpError("max_pool3d_same expects [N, C, D, H, W], got %s" % (tuple(x.shape),))
        n, c, d, h, w = x.shape
        osz = tuple(same_pool_geometry(sz, kernel[i], stride[i])[2] for i, sz in enumerate((d, h, w)))
        y = torch.empty((n, c) + osz, dtype=torch.float32, device=x.device)
        idx = torch.empty((n, c) + osz, dtype=torch.int32, device=x.device) if save else None
        check(lib.cstp_maxpool3d_same_forward(_stream(), x.data_ptr(), y.data_ptr(), _ptr(idx), n * c, d, h, w,
                                              (ctypes.c_int32 * 3)(*kernel), (ctypes.c_int32 * 3)(*stride)),
              "cstp_maxpool3d_same_forward")
        if save:
            ctx.save_for_backward(idx)
        ctx.geom = (tuple(x.shape), tuple(kernel), tuple(stride))
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        (idx,) = ctx.saved_tensors
        shape, kernel, stride = ctx.geom
        dy = _req(dy, "max_pool3d_same grad_output")
        dx = torch.empty(shape, dtype=torch.float32, device=dy.device)
        n, c, d, h, w = shape
        check(lib.cstp_maxpool3d_same_backward(_stream(), dy.data_ptr(), idx.data_ptr(), dx.data_ptr(), n * c, d, h, w,
                                               (ctypes.c_int32 * 3)(*kernel), (ctypes.c_int32 * 3)(*stride)),
              "cstp_maxpool3d_same_backward")
        return dx, None, None, None


def max_pool3d_same(x, kernel_size, stride):
    """MaxPool3dTFPadding (i3d_byol.py:170-183): ``MaxPool3d(k, s, ceil_mode=True)(ConstantPad3d(get_padding_shape(k, s), 0)(x))``
    in one kernel, without the padded copy: a padding position is a candidate of value 0 (and swallows the gradient when it
    wins).  fp32 only."""
    if x.dtype == torch.bfloat16:
        raise _lib.CstpError("max_pool3d_same is fp32 only (I3D has no bf16-storage path)")
    # the argmax is written only when a gradient can be asked for
    return _MaxPool3dSame.apply(x, _triple(kernel_size), _triple(stride), torch.is_grad_enabled() and x.requires_grad)


class _AvgPool3dWindow(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel):
        lib = _lib.load()
        x = _req(x, "avg_pool3d_window input")
        n, c, d, h, w = x.shape
        y = torch.empty((n, c, d - kernel[0] + 1, h - kernel[1] + 1, w - kernel[2] + 1), dtype=torch.float32, device=x.device)
        check(lib.cstp_avgpool3d_window_forward(_stream(), x.data_ptr(), y.data_ptr(), n * c, d, h, w,
                                                (ctypes.c_int32 * 3)(*kernel)), "cstp_avgpool3d_window_forward")
        ctx.geom = (tuple(x.shape), tuple(kernel))
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        shape, kernel = ctx.geom
        dy = _req(dy, "avg_pool3d_window grad_output")
        dx = torch.empty(shape, dtype=torch.float32, device=dy.device)
        n, c, d, h, w = shape
        check(lib.cstp_avgpool3d_window_backward(_stream(), dy.data_ptr(), dx.data_ptr(), n * c, d, h, w,
                                                 (ctypes.c_int32 * 3)(*kernel)), "cstp_avgpool3d_window_backward")
        return dx, None


def avg_pool3d_window(x, kernel_size):
    """nn.AvgPool3d(kernel_size, stride 1) over valid windows (i3d_byol.py:297), [N, C, D, H, W] fp32.  A window that covers the
    whole volume is the global average pool and goes to its kernel."""
    kernel = _triple(kernel_size)
    if x.dim() != 5:
        raise _lib.CstpError("avg_pool3d_window expects [N, C, D, H, W], got %s" % (tuple(x.shape),))
    if any(k < 1 or k > sz for k, sz in zip(kernel, x.shape[2:])):
        raise _lib.CstpError("avg_pool3d_window: kernel %s does not fit the %s volume" % (kernel, tuple(x.shape[2:])))
    if tuple(x.shape[2:]) == kernel:
        return global_avg_pool(x).reshape(x.shape[0], x.shape[1], 1, 1, 1)
    return _AvgPool3dWindow.apply(x, kernel)


class _BNReluConcat(torch.autograd.Function):
    """y = cat_i(relu(batch_norm_train(x_i))) over the branches of one I3D Mixed block (i3d_byol.py:214-220): two launches
    forward (three when a branch brings no statistics), two backward, for all branches together.  Saved for backward, in this
    order: the nb inputs, the nb weights, save_mean and save_invstd [groups * C], the (scale, shift) table."""

    @staticmethod
    def forward(ctx, nb, save, groups, eps, momentum, running, call, *args):
        lib = _lib.load()
        xs = [_req(x, "bn_relu_concat branch") for x in args[:nb]]
        gammas = [_req(g, "bn_relu_concat weight") for g in args[nb:2 * nb]]
        betas = [_req(b, "bn_relu_concat bias") for b in args[2 * nb:3 * nb]]
        n, spatial = xs[0].shape[0], tuple(xs[0].shape[2:])
        for x, g, b in zip(xs, gammas, betas):
            if x.dim() != 5 or x.shape[0] != n or tuple(x.shape[2:]) != spatial:
                raise _lib.CstpError("bn_relu_concat branches must be [N, C_i, D, H, W] with one N, D, H, W; got %s"
                                     % ([tuple(t.shape) for t in xs],))
            if tuple(g.shape) != (x.shape[1],) or tuple(b.shape) != (x.shape[1],):
                raise _lib.CstpError("bn_relu_concat branch of %d channels needs [%d] weight and bias, got %s, %s"
                                     % (x.shape[1], x.shape[1], tuple(g.shape), tuple(b.shape)))
        if groups < 1 or n % groups != 0:
            raise _lib.CstpError("batch of %d rows cannot be split into %d BN groups" % (n, groups))
        cs = [x.shape[1] for x in xs]
        ctot = sum(cs)
        s = xs[0].numel() // (n * cs[0])
        dev = xs[0].device
        pre = call.pre           # per branch: what the producing convolution left, or None
        y = torch.empty((n, ctot) + spatial, dtype=torch.float32, device=dev)
        mean = torch.empty(groups * ctot, dtype=torch.float32, device=dev)
        invstd = torch.empty(groups * ctot, dtype=torch.float32, device=dev)
        ss = torch.empty(groups * ctot * 2, dtype=torch.float32, device=dev)
        cell = _new_cell(y)
        wsp = _workspace(dev, lib.cstp_bnrelu_concat_workspace_bytes(ctot, groups))
        br = (_lib.BncBranch * nb)(*[
            _lib.BncBranch(x.data_ptr(), g.data_ptr(), b.data_ptr(), _ptr(rm), _ptr(rv), None if p is None else p[0].data_ptr(),
                           None, None, None, None, c, 0 if p is None else p[1])
            for x, g, b, (rm, rv), p, c in zip(xs, gammas, betas, running, pre, cs)])
        with _span("bnc_forward", (n, s, groups, tuple(cs))):
            check(lib.cstp_bnrelu_concat_forward(_stream(), br, nb, n, s, groups, eps, momentum, y.data_ptr(), mean.data_ptr(),
                                                 invstd.data_ptr(), ss.data_ptr(), wsp.data_ptr(), wsp.numel(), _ptr(cell)),
                  "cstp_bnrelu_concat_forward")
        call.cell = cell
        if save:
            ctx.save_for_backward(*xs, *gammas, mean, invstd, ss)
            ctx.params = args[nb:3 * nb]       # the parameter objects themselves (.grad may be an arena slice)
        ctx.nb, ctx.save, ctx.geom = nb, save, (n, s, groups, tuple(cs))
        return y

    @staticmethod
    def backward(ctx, dy):
        if not ctx.save:
            raise RuntimeError("bn_relu_concat: forward ran without saving its statistics (no gradient was required then)")
        lib = _lib.load()
        nb = ctx.nb
        saved = ctx.saved_tensors
        xs, gammas = saved[:nb], saved[nb:2 * nb]
        mean, invstd, ss = saved[2 * nb:2 * nb + 3]
        n, s, groups, cs = ctx.geom
        dy = _req(dy, "bn_relu_concat grad_output")
        dxs = [torch.empty_like(x) for x in xs]
        # gradients of leaf parameters whose .grad is a live slice of the flat arena are added there by the kernel (as _BNAct does)
        direct = all(ctx.needs_input_grad[7 + nb:7 + 3 * nb]) and all(_direct(p) for p in ctx.params)
        dgs = [p.grad for p in ctx.params[:nb]] if direct else [torch.empty_like(g) for g in gammas]
        dbs = [p.grad for p in ctx.params[nb:]] if direct else [torch.empty_like(g) for g in gammas]
        cells = torch.empty(nb, dtype=torch.int32, device=dy.device) if FUSE_ABSMAX else None
        br = (_lib.BncBranch * nb)(*[
            _lib.BncBranch(x.data_ptr(), g.data_ptr(), None, None, None, None, dx.data_ptr(), dg.data_ptr(), db.data_ptr(),
                           None if cells is None else cells[i:i + 1].data_ptr(), c, 0)
            for i, (x, g, dx, dg, db, c) in enumerate(zip(xs, gammas, dxs, dgs, dbs, cs))])
        wsp = _workspace(dy.device, lib.cstp_bnrelu_concat_workspace_bytes(sum(cs), groups))
        with _span("bnc_backward", (n, s, groups, tuple(cs))):
            check(lib.cstp_bnrelu_concat_backward(_stream(), br, nb, n, s, groups, dy.data_ptr(), mean.data_ptr(),
                                                  invstd.data_ptr(), ss.data_ptr(), wsp.data_ptr(), wsp.numel(),
                                                  1 if direct else 0), "cstp_bnrelu_concat_backward")
        if cells is not None:
            for i, dx in enumerate(dxs):
                _tag_absmax(dx, cells[i:i + 1])
        head = (None,) * 7
        if direct:
            return head + tuple(dxs) + (None,) * (2 * nb)
        return head + tuple(dxs) + tuple(dgs) + tuple(dbs)


def _bnc_check(branches, bns):
    branches, bns = list(branches), [tuple(b) for b in bns]
    if not 1 <= len(branches) <= 4 or len(bns) != len(branches) or any(len(b) != 4 for b in bns):
        raise _lib.CstpError("bn_relu_concat takes 1..4 branches with one (weight, bias, running_mean, running_var) each, got "
                             "%d and %d" % (len(branches), len(bns)))
    for t in branches + [b[0] for b in bns] + [b[1] for b in bns]:
        if t.dtype == torch.bfloat16:
            raise _lib.CstpError("bn_relu_concat is fp32 only (I3D has no bf16-storage path)")
    return branches, bns


def bn_relu_concat(branches, bns, groups=1, eps=BN_EPS, momentum=BN_MOMENTUM):
    """I3D Mixed tail (fp32): ``torch.cat([relu(batch_norm_train(x, ...)) for x in branches], 1)`` with ``bns`` the
    (weight, bias, running_mean, running_var) of each branch's BatchNorm3d; the running statistics are updated in place
    (``groups`` > 1: group after group, as batch_norm_act).  A branch whose convolution left its partial sums (ops.conv3d(...,
    bn_groups=groups)) uses them -- the result then equals batch_norm_act + cat bit for bit -- the others share one statistics
    launch.  The result is tagged with its max |y| cell for the 1x1x1 convolutions that consume it."""
    branches, bns = _bnc_check(branches, bns)
    nb = len(branches)
    gammas, betas = [b[0] for b in bns], [b[1] for b in bns]
    running = [(None if b[2] is None else _req(b[2], "running_mean"), None if b[3] is None else _req(b[3], "running_var"))
               for b in bns]
    save = torch.is_grad_enabled() and any(t.requires_grad for t in branches + gammas + betas)
    call = _Call([_bnstats_of(x, int(groups)) for x in branches])
    y = _BNReluConcat.apply(nb, save, int(groups), float(eps), float(momentum), running, call, *branches, *gammas, *betas)
    _tag_absmax(y, call.cell)
    return y


def bn_relu_concat_eval(branches, bns, eps=BN_EPS):
    """model.eval() form of bn_relu_concat: ``torch.cat([relu(batch_norm_eval(x, ...)) for x in branches], 1)`` (running
    statistics, nothing updated).  Forward only, as batch_norm_eval."""
    lib = _lib.load()
    branches, bns = _bnc_check(branches, bns)
    if torch.is_grad_enabled() and any(t.requires_grad for t in branches + [b[0] for b in bns] + [b[1] for b in bns]):
        raise _lib.CstpError("eval-mode BatchNorm is forward-only: call it under torch.no_grad() (as the reference's "
                             "validation/test loops do)")
    xs = [_req(x, "bn_relu_concat branch") for x in branches]
    n, spatial = xs[0].shape[0], tuple(xs[0].shape[2:])
    if any(x.dim() != 5 or x.shape[0] != n or tuple(x.shape[2:]) != spatial for x in xs):
        raise _lib.CstpError("bn_relu_concat branches must be [N, C_i, D, H, W] with one N, D, H, W; got %s"
                             % ([tuple(t.shape) for t in xs],))
    cs = [x.shape[1] for x in xs]
    ctot = sum(cs)
    s = xs[0].numel() // (n * cs[0])
    y = torch.empty((n, ctot) + spatial, dtype=torch.float32, device=xs[0].device)
    ss = torch.empty(ctot * 2, dtype=torch.float32, device=y.device)
    cell = _new_cell(y)
    keep = [[_req(t, "BatchNorm tensor") for t in b] for b in bns]
    br = (_lib.BncBranch * len(xs))(*[
        _lib.BncBranch(x.data_ptr(), k[0].data_ptr(), k[1].data_ptr(), k[2].data_ptr(), k[3].data_ptr(), None, None, None, None,
                       None, c, 0) for x, k, c in zip(xs, keep, cs)])
    check(lib.cstp_bnrelu_concat_eval(_stream(), br, len(xs), n, s, float(eps), y.data_ptr(), ss.data_ptr(), _ptr(cell)),
          "cstp_bnrelu_concat_eval")
    _tag_absmax(y, cell)
    return y


# ----------------------------------------------------------------------------------------------
# the bf16-STORAGE path (csrc/b16.hip; BASELINE configs[4]), selected by the dtype of the activation tensor:
# 5-D activations and their gradients bf16, parameters / their gradients / statistics fp32 (cstp_hip.h "bf16-STORAGE path")
# ----------------------------------------------------------------------------------------------
def _req16(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.CstpError("%s must be on a HIP device (cstp_amd has no CPU path)" % name)
    if t.dtype != torch.bfloat16:
        raise _lib.CstpError("%s must be bfloat16 on the bf16-storage path, got %s" % (name, t.dtype))
    return t.contiguous()


def to_bf16(x: torch.Tensor) -> torch.Tensor:
    """The fp32 clip rounded to bf16 (what autocast does to the first convolution's input); no gradient flows into a clip."""
    lib = _lib.load()
    x = _req(x.detach(), "clip")
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    check(lib.cstp_b16_cast(_stream(), x.data_ptr(), y.data_ptr(), x.numel()), "cstp_b16_cast")
    return y


class _Conv3dB16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, stride, padding, grad_join=None):
        lib = _lib.load()
        w_in = w
        ctx.grad_join = grad_join
        x = _req16(x, "conv3d input")
        w = _req(w, "conv3d weight")
        desc = _desc(x.shape, w.shape, stride, padding)
        y = torch.empty(conv_out_shape(x.shape, w.shape, stride, padding), dtype=torch.bfloat16, device=x.device)
        nbytes = lib.cstp_b16_conv3d_workspace_bytes(ctypes.byref(desc))
        with _span("conv3d_forward", lambda: ("bf16",) + _desc_key(desc)):
            _packed_call(_own_pack(w, w_in), "f", x.shape, x.device, nbytes,
                         lambda ws: check(lib.cstp_b16_conv3d_forward(_stream(), ctypes.byref(desc), x.data_ptr(), w.data_ptr(), y.data_ptr(),
                                                                      ws.data_ptr(), ws.numel()), "cstp_b16_conv3d_forward"),
                         _dispatch_facts((x, y), None))
        ctx.save_for_backward(x, w)
        ctx.w_param = w_in
        ctx.desc = desc
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, w = ctx.saved_tensors
        desc = ctx.desc
        dy = _req16(dy, "conv3d grad_output")
        nbytes = lib.cstp_b16_conv3d_workspace_bytes(ctypes.byref(desc))
        dx = None

        def wgrad(dst, accumulate):
            wsx = _workspace(x.device, nbytes)
            with _span("conv3d_backward_weight", lambda: ("bf16",) + _desc_key(desc)):
                check(lib.cstp_b16_conv3d_backward_weight(_stream(), ctypes.byref(desc), x.data_ptr(), dy.data_ptr(), dst.data_ptr(),
                                                          wsx.data_ptr(), wsx.numel(), 1 if accumulate else 0),
                      "cstp_b16_conv3d_backward_weight")

        dw = _place_wgrad(ctx.w_param, w, ctx.needs_input_grad[1], True, wgrad, (x, dy))
        if ctx.needs_input_grad[0]:
            dx = _data_grad(desc, x, w, ctx.w_param, dy, None, nbytes,
                            lambda dst, ws, acc: check(lib.cstp_b16_conv3d_backward_data_acc(
                                _stream(), ctypes.byref(desc), dy.data_ptr(), w.data_ptr(), dst.data_ptr(), ws.data_ptr(), ws.numel(),
                                1 if acc else 0), "cstp_b16_conv3d_backward_data"), ctx.grad_join)
        return dx, dw, None, None, None


class _BNActB16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, residual, running_mean, running_var, relu, eps, momentum, groups, grad_join=None):
        lib = _lib.load()
        ctx.param_objs = (gamma, beta)     # the parameter objects themselves (their .grad may be an arena slice)
        ctx.grad_join = grad_join
        x, res, n, c, s = _bn_operands(_req16, x, residual, groups)
        gamma = _req(gamma, "batch_norm weight")
        beta = _req(beta, "batch_norm bias")
        y = torch.empty_like(x)
        mean = torch.empty(groups * c, dtype=torch.float32, device=x.device)
        invstd = torch.empty(groups * c, dtype=torch.float32, device=x.device)
        ss = torch.empty(groups * c * 2, dtype=torch.float32, device=x.device)
        ws = _workspace(x.device, lib.cstp_b16_bn_workspace_bytes(n, c, s, groups))
        with _span("bn_forward", (n, c, s, groups, res is not None, bool(relu), "bf16")):
            check(lib.cstp_b16_bn_forward_train(_stream(), x.data_ptr(), _ptr(res), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                                _ptr(running_mean), _ptr(running_var), mean.data_ptr(), invstd.data_ptr(),
                                                ss.data_ptr(), n, c, s, groups, eps, momentum, 1 if relu else 0, ws.data_ptr(),
                                                ws.numel()), "cstp_b16_bn_forward_train")
        # ReLU without a residual: backward recomputes the mask from x with the affine table instead of re-reading y
        ctx.remask = bool(relu and res is None)
        ctx.save_for_backward(x, ss if ctx.remask else y, gamma, mean, invstd, ss)
        ctx.relu, ctx.groups, ctx.has_res = relu, groups, res is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, y_or_ss, gamma, mean, invstd, ss = ctx.saved_tensors
        y = None if ctx.remask else y_or_ss
        dy = _req16(dy, "batch_norm grad_output")
        n, c = x.shape[0], x.shape[1]
        s = x.numel() // (n * c)
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if (ctx.has_res and ctx.needs_input_grad[3]) else None
        direct, dgamma, dbeta = _bn_param_grads(ctx.needs_input_grad[1], ctx.needs_input_grad[2], *ctx.param_objs, gamma)
        ws = _workspace(x.device, lib.cstp_b16_bn_workspace_bytes(n, c, s, ctx.groups))
        with _span("bn_backward", (n, c, s, ctx.groups, ctx.has_res, bool(ctx.relu), "bf16")):
            check(lib.cstp_b16_bn_backward(_stream(), x.data_ptr(), _ptr(y), dy.data_ptr(), gamma.data_ptr(), mean.data_ptr(),
                                           invstd.data_ptr(), ss.data_ptr(), dx.data_ptr(), _ptr(dres), dgamma.data_ptr(),
                                           dbeta.data_ptr(), n, c, s, ctx.groups, 1 if ctx.relu else 0, ws.data_ptr(), ws.numel(),
                                           1 if direct else 0), "cstp_b16_bn_backward")
        if direct:
            dgamma = dbeta = None
        if dres is not None and ctx.grad_join is not None:       # the residual tensor's other consumer adds its gradient to this
            dres = ctx.grad_join.contribute(lambda: dres, lambda buf: buf.add_(dres))
        return dx, dgamma, dbeta, dres, None, None, None, None, None, None, None


# ----------------------------------------------------------------------------------------------
# losses
# ----------------------------------------------------------------------------------------------
class _ByolLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y):
        lib = _lib.load()
        x = _req(x, "byol x")
        y = _req(y, "byol y")
        b, f = x.shape
        loss = torch.empty(b, dtype=torch.float32, device=x.device)
        check(lib.cstp_byol_loss_forward(_stream(), x.data_ptr(), y.data_ptr(), loss.data_ptr(), b, f), "cstp_byol_loss_forward")
        ctx.save_for_backward(x, y)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        lib = _lib.load()
        x, y = ctx.saved_tensors
        dloss = _req(dloss, "byol grad_output")
        dx = torch.empty_like(x)
        check(lib.cstp_byol_loss_backward(_stream(), x.data_ptr(), y.data_ptr(), dloss.data_ptr(), dx.data_ptr(), x.shape[0],
                                          x.shape[1]), "cstp_byol_loss_backward")
        return dx, None


def byol_regression_loss(x, y):
    """2 - 2*cos(x, y) per row; y is treated as a constant (the detached target projection)."""
    return _ByolLoss.apply(x, y.detach())


class _L2Normalize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eps):
        lib = _lib.load()
        x = _req(x, "normalize input")
        rows, f = x.shape
        y = torch.empty_like(x)
        norm = torch.empty(rows, dtype=torch.float32, device=x.device)
        check(lib.cstp_l2_normalize_forward(_stream(), x.data_ptr(), y.data_ptr(), norm.data_ptr(), rows, f, eps),
              "cstp_l2_normalize_forward")
        ctx.save_for_backward(y, norm)
        ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        y, norm = ctx.saved_tensors
        dy = _req(dy, "normalize grad_output")
        dx = torch.empty_like(y)
        check(lib.cstp_l2_normalize_backward(_stream(), y.data_ptr(), norm.data_ptr(), dy.data_ptr(), dx.data_ptr(),
                                             y.shape[0], y.shape[1], ctx.eps), "cstp_l2_normalize_backward")
        return dx, None


def l2_normalize(x, eps=1e-12):
    """F.normalize(x, p=2, dim=1) for 2-D x (r21d_byol.py:396)."""
    if x.dim() != 2:
        raise _lib.CstpError("l2_normalize expects [rows, features], got %s" % (tuple(x.shape),))
    return _L2Normalize.apply(x, float(eps))


class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels):
        lib = _lib.load()
        logits = _req(logits, "cross_entropy logits")
        if labels.dtype != torch.int64 or not labels.is_cuda:
            raise _lib.CstpError("cross_entropy labels must be int64 on the HIP device")
        labels = labels.contiguous()
        b, k = logits.shape
        loss = torch.empty(1, dtype=torch.float32, device=logits.device)
        check(lib.cstp_cross_entropy_forward(_stream(), logits.data_ptr(), labels.data_ptr(), loss.data_ptr(), b, k),
              "cstp_cross_entropy_forward")
        ctx.save_for_backward(logits, labels)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        lib = _lib.load()
        logits, labels = ctx.saved_tensors
        dloss = _req(dloss.reshape(1), "cross_entropy grad_output")
        dl = torch.empty_like(logits)
        check(lib.cstp_cross_entropy_backward(_stream(), logits.data_ptr(), labels.data_ptr(), dloss.data_ptr(), dl.data_ptr(),
                                              logits.shape[0], logits.shape[1]), "cstp_cross_entropy_backward")
        return dl, None


def cross_entropy(logits, labels):
    """nn.CrossEntropyLoss() (mean reduction)."""
    return _CrossEntropy.apply(logits, labels)


class _SoftCrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, ta, tb, lam, eps):
        lib = _lib.load()
        logits = _req(logits, "soft_cross_entropy logits")
        if logits.dim() != 2:
            raise _lib.CstpError("soft_cross_entropy expects logits [batch, classes], got %s" % (tuple(logits.shape),))
        b, k = logits.shape
        for name, t in (("ta", ta), ("tb", tb)):
            if t is not None and (t.dtype != torch.int64 or not t.is_cuda or t.shape != (b,)):
                raise _lib.CstpError("soft_cross_entropy %s must be int64 [%d] on the HIP device" % (name, b))
        if lam is not None and (lam.dtype != torch.float32 or not lam.is_cuda or lam.shape != (b,)):
            raise _lib.CstpError("soft_cross_entropy lam must be float32 [%d] on the HIP device" % b)
        ta = ta.contiguous()
        tb = None if tb is None else tb.contiguous()
        lam = None if lam is None else lam.contiguous()
        loss = torch.empty(1, dtype=torch.float32, device=logits.device)
        check(lib.cstp_soft_cross_entropy_forward(_stream(), logits.data_ptr(), ta.data_ptr(), _ptr(tb), _ptr(lam), eps,
                                                  loss.data_ptr(), b, k), "cstp_soft_cross_entropy_forward")
        ctx.save_for_backward(logits, ta, tb, lam)
        ctx.eps = eps
        return loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        lib = _lib.load()
        logits, ta, tb, lam = ctx.saved_tensors
        dloss = _req(dloss.reshape(1), "soft_cross_entropy grad_output")
        dl = torch.empty_like(logits)
        check(lib.cstp_soft_cross_entropy_backward(_stream(), logits.data_ptr(), ta.data_ptr(), _ptr(tb), _ptr(lam), ctx.eps,
                                                   dloss.data_ptr(), dl.data_ptr(), logits.shape[0], logits.shape[1]),
              "cstp_soft_cross_entropy_backward")
        return dl, None, None, None, None


def soft_cross_entropy(logits, ta, tb=None, lam=None, eps=0.0):
    """Mean cross-entropy against q = (1-eps)*(lam*onehot(ta) + (1-lam)*onehot(tb)) + eps/classes: label smoothing and the two
    weighted targets of mixup / CutMix (F.cross_entropy(logits, q)).  ta / tb: int64 [batch], lam: fp32 [batch], all on the
    device; tb = None means tb = ta, lam = None means lam = 1 (the smoothing-only form, F.cross_entropy(logits, ta,
    label_smoothing=eps)).  A target outside [0, classes) adds no one-hot mass."""
    eps = float(eps)
    if not 0.0 <= eps < 1.0:
        raise _lib.CstpError("soft_cross_entropy eps must lie in [0, 1), got %r" % (eps,))
    return _SoftCrossEntropy.apply(logits, ta, tb, lam, eps)


# struct cstp_clip_mix_entry (include/cstp_hip.h), packed by hand into the pinned upload buffer
_MIX_ENTRY = np.dtype([("partner", "<i4"), ("mode", "<i4"), ("lam", "<f4"), ("y0", "<i4"), ("y1", "<i4"), ("x0", "<i4"),
                       ("x1", "<i4"), ("reserved", "<i4")])


def _per_sample(v, b, name):
    v = [v] * b if isinstance(v, (int, float)) else list(v)
    if len(v) != b:
        raise _lib.CstpError("clip_mix %s has %d entries for a batch of %d" % (name, len(v), b))
    return v


def clip_mix(x, partner, mode, lam, boxes=None):
    """mixup / CutMix of a batch of clips in one launch (cstp_clip_mix): x [B, ..., H, W] fp32 -> a new tensor of that shape.
    Per sample i (host sequences of B entries; ``mode`` and ``lam`` may be one value for all, ``boxes`` one box for all or None):
    mode 0 copies x[i], mode 1 gives lam*x[i] + (1-lam)*x[partner[i]], mode 2 pastes x[partner[i]] into the half-open box
    (y0, y1, x0, x1) of every plane.  The table is validated completely here -- a bad entry raises CstpError before anything is
    uploaded or launched -- and travels in one pinned, asynchronous upload; nothing is read back."""
    if x.dim() < 3:
        raise _lib.CstpError("clip_mix expects [batch, ..., height, width], got %s" % (tuple(x.shape),))
    b, h, w = x.shape[0], x.shape[-2], x.shape[-1]
    partner = _per_sample(partner, b, "partner")
    mode = _per_sample(mode, b, "mode")
    lam = _per_sample(lam, b, "lam")
    if boxes is None:
        boxes = (0, 0, 0, 0)
    if len(boxes) == 4 and all(isinstance(v, (int, np.integer)) for v in boxes):
        boxes = [boxes] * b
    boxes = _per_sample(boxes, b, "boxes")
    for i in range(b):
        if int(partner[i]) != partner[i] or not 0 <= partner[i] < b:
            raise _lib.CstpError("clip_mix partner[%d] = %r is outside the batch of %d" % (i, partner[i], b))
        if mode[i] not in (MODE_COPY, MODE_MIXUP, MODE_CUTMIX):
            raise _lib.CstpError("clip_mix mode[%d] = %r: 0 (copy), 1 (mixup) and 2 (CutMix) exist" % (i, mode[i]))
        if not 0.0 <= float(lam[i]) <= 1.0:
            raise _lib.CstpError("clip_mix lam[%d] = %r is outside [0, 1]" % (i, lam[i]))
        if len(boxes[i]) != 4 or any(int(v) != v for v in boxes[i]):
            raise _lib.CstpError("clip_mix boxes[%d] = %r: a box is four integers (y0, y1, x0, x1)" % (i, boxes[i]))
        y0, y1, x0, x1 = boxes[i]
        if not (0 <= y0 <= y1 <= h and 0 <= x0 <= x1 <= w):
            raise _lib.CstpError("clip_mix boxes[%d] = %r leaves the %d x %d frame" % (i, tuple(boxes[i]), h, w))
    lib = _lib.load()
    x = _req(x, "clip_mix input")
    planes = x.numel() // (b * h * w) if x.numel() else 0
    host = torch.empty(b * _MIX_ENTRY.itemsize, dtype=torch.uint8, pin_memory=True)
    tab = host.numpy().view(_MIX_ENTRY)
    for i in range(b):
        tab[i] = (int(partner[i]), int(mode[i]), float(lam[i])) + tuple(int(v) for v in boxes[i]) + (0,)
    table = torch.empty(host.numel(), dtype=torch.uint8, device=x.device)
    table.copy_(host, non_blocking=True)
    y = torch.empty_like(x)
    check(lib.cstp_clip_mix(_stream(), x.data_ptr(), y.data_ptr(), table.data_ptr(), b, planes, h, w), "cstp_clip_mix")
    return y


# ----------------------------------------------------------------------------------------------
# fine-tuning regularisers (csrc/reg.h, cstp_amd/regularize.py): dropout with a counter-based mask, the stochastic-depth join
# ----------------------------------------------------------------------------------------------
# A/B switch, read at import: 0 composes both operations from ATen calls on device tensors (the same mask, the same expression),
# for comparison on one machine; the product path is the kernels.
REG_FUSED = os.environ.get("CSTP_REG_FUSED", "1") != "0"
_M32 = 0xFFFFFFFF


def _mulhilo_aten(m: int, c: torch.Tensor):
    """(hi, lo) 32-bit halves of m * c for int64 tensors holding values below 2^32: int64 products of 16 x 32 bits cannot wrap."""
    a, b = (m >> 16) * c, (m & 0xFFFF) * c
    t = ((a & 0xFFFF) << 16) + b
    return (a >> 16) + (t >> 32), t & _M32


def _dropout_keep_aten(n: int, p: float, key: int, offset: int, device) -> torch.Tensor:
    """The keep mask of cstp_dropout for elements 0 .. n - 1 (bool [n]) from ATen integer arithmetic: CSTP_REG_FUSED=0 only."""
    q = torch.arange((n + 3) // 4, dtype=torch.int64, device=device)
    c = [q & _M32, q >> 32, torch.full_like(q, offset & _M32), torch.full_like(q, (offset >> 32) & _M32)]
    k0, k1 = key & _M32, (key >> 32) & _M32
    for _ in range(10):
        hi0, lo0 = _mulhilo_aten(0xD2511F53, c[0])
        hi1, lo1 = _mulhilo_aten(0xCD9E8D57, c[2])
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    w = torch.stack(c, dim=1).reshape(-1)[:n]
    u = (w >> 8).to(torch.float32) * float(2.0 ** -24)
    return u >= torch.tensor(p, dtype=torch.float32, device=device)


class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, key, offset):
        ctx.args = (p, key, offset)
        return _Dropout._run(_req(x, "dropout input"), p, key, offset)

    @staticmethod
    def _run(x, p, key, offset):
        y = torch.empty_like(x)
        if x.numel():
            check(_lib.load().cstp_dropout(_stream(), x.data_ptr(), y.data_ptr(), x.numel(), p, key, offset), "cstp_dropout")
        return y

    @staticmethod
    def backward(ctx, dy):
        return _Dropout._run(_req(dy, "dropout grad_output"), *ctx.args), None, None, None


def dropout(x, p, key, offset=0):
    """Inverted dropout with the counter-based mask of cstp_dropout: element e of the (contiguous) tensor is kept iff
    Philox4x32-10((e >> 2, offset), key)[e & 3], as a 24-bit fraction, is >= p, and then scaled by 1 / (1 - p) in fp32.  ``key`` is the
    step's uint64 (cstp_amd.regularize), ``offset`` numbers the call site.  The gradient is the same call on the incoming
    gradient; no mask is stored.  p == 0 returns ``x`` itself."""
    if not x.is_cuda:
        raise _lib.CstpError("dropout input must be on a HIP device (cstp_amd has no CPU path)")
    p = float(np.float32(p))
    if not 0.0 <= p < 1.0:
        raise _lib.CstpError("dropout p must lie in [0, 1), got %r" % (p,))
    key, offset = int(key), int(offset)
    if not (0 <= key < 2 ** 64 and 0 <= offset < 2 ** 64):
        raise _lib.CstpError("dropout key and offset are unsigned 64-bit numbers, got %r, %r" % (key, offset))
    if p == 0.0:
        return x
    if not REG_FUSED:
        x = _req(x, "dropout input")
        keep = _dropout_keep_aten(x.numel(), p, key, offset, x.device).view(x.shape)
        inv = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))             # the kernel's fp32 quotient
        return torch.where(keep, x * inv, torch.zeros((), dtype=x.dtype, device=x.device))
    return _Dropout.apply(x, p, key, offset)


_zero_cells = {}
ZERO_CELLS = 1024


def _zeroed_cell(like: torch.Tensor) -> Optional[torch.Tensor]:
    """An absmax cell that holds 0, for a kernel that takes its maximum with atomics in ONE launch: cells are dealt out of a pool
    zeroed ZERO_CELLS at a time (per device and stream, as _workspace) and never reused, so no call pays a fill launch."""
    if not FUSE_ABSMAX:
        return None
    key = (like.device.index, _stream())
    pool = _zero_cells.get(key)
    if pool is None or pool[1] >= ZERO_CELLS:
        pool = _zero_cells[key] = [torch.zeros(ZERO_CELLS, dtype=torch.int32, device=like.device), 0]
    cell = pool[0][pool[1]:pool[1] + 1]
    pool[1] += 1
    return cell


class _DropPathAddRelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, residual, scale, call):
        lib = _lib.load()
        b16 = z.dtype == torch.bfloat16
        req = _req16 if b16 else _req
        z, res = req(z, "drop_path branch"), req(residual, "drop_path residual")
        y = torch.empty_like(z)
        cell = None if b16 else _zeroed_cell(z)
        n = z.numel()
        check(lib.cstp_droppath_add_relu_forward(_stream(), z.data_ptr(), res.data_ptr(), scale.data_ptr(), y.data_ptr(), n,
                                                 n // z.shape[0], 1 if b16 else 0, _ptr(cell)), "cstp_droppath_add_relu_forward")
        call.cell = cell
        ctx.save_for_backward(y, scale)
        ctx.b16 = b16
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        y, scale = ctx.saved_tensors
        need_z, need_r = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_z or need_r):
            return None, None, None, None
        dy = (_req16 if ctx.b16 else _req)(dy, "drop_path grad_output")
        dz = torch.empty_like(y) if need_z else None
        dres = torch.empty_like(y) if need_r else None
        n = y.numel()
        check(lib.cstp_droppath_add_relu_backward(_stream(), y.data_ptr(), dy.data_ptr(), scale.data_ptr(), _ptr(dz), _ptr(dres), n,
                                                  n // y.shape[0], 1 if ctx.b16 else 0), "cstp_droppath_add_relu_backward")
        return dz, dres, None, None


def drop_path_add_relu(z, residual, scale):
    """relu(scale[b] * z[b] + residual[b]): the end of a residual block under stochastic depth, one launch forward and one backward
    (cstp_droppath_add_relu_*).  z / residual: [B, ...] of one shape, both fp32 or both bf16 (bf16 storage: fp32 arithmetic,
    rounded to nearest even); scale: fp32 [B] on the device, 0 for a dropped sample and 1 / (1 - p) for a kept one.  The fp32
    result carries its absmax for the consuming convolution."""
    for name, t in (("branch", z), ("residual", residual), ("scale", scale)):
        if not t.is_cuda:
            raise _lib.CstpError("drop_path %s must be on a HIP device (cstp_amd has no CPU path)" % name)
    if z.dim() < 2 or residual.shape != z.shape or residual.dtype != z.dtype:
        raise _lib.CstpError("drop_path residual %s %s != branch %s %s" % (tuple(residual.shape), residual.dtype, tuple(z.shape), z.dtype))
    if z.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.CstpError("drop_path activations must be float32 or bfloat16, got %s" % (z.dtype,))
    if scale.dtype != torch.float32 or scale.shape != (z.shape[0],) or z.shape[0] == 0 or z.numel() == 0:
        raise _lib.CstpError("drop_path scale must be float32 [%d] for a non-empty batch" % (z.shape[0],))
    scale = scale.contiguous()
    if not REG_FUSED:
        s = scale.view((-1,) + (1,) * (z.dim() - 1))
        if z.dtype == torch.bfloat16:
            return torch.relu(s * z.float() + residual.float()).to(torch.bfloat16)
        return torch.relu(s * z + residual)
    call = _Call()
    y = _DropPathAddRelu.apply(z, residual, scale, call)
    _tag_absmax(y, call.cell)
    return y


class _NTXent(torch.autograd.Function):
    @staticmethod
    def forward(ctx, reps, temperature):
        lib = _lib.load()
        reps = _req(reps, "ntxent representations")
        two_n, f = reps.shape
        nbytes = lib.cstp_ntxent_workspace_bytes(two_n, f)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=reps.device)  # private: lives until backward
        loss = torch.empty(1, dtype=torch.float32, device=reps.device)
        check(lib.cstp_ntxent_forward(_stream(), reps.data_ptr(), loss.data_ptr(), two_n, f, temperature, ws.data_ptr(),
                                      ws.numel()), "cstp_ntxent_forward")
        ctx.save_for_backward(reps, ws)
        ctx.temperature = temperature
        return loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        lib = _lib.load()
        reps, ws = ctx.saved_tensors
        dloss = _req(dloss.reshape(1), "ntxent grad_output")
        dreps = torch.empty_like(reps)
        check(lib.cstp_ntxent_backward(_stream(), reps.data_ptr(), dloss.data_ptr(), dreps.data_ptr(), reps.shape[0],
                                       reps.shape[1], ctx.temperature, ws.data_ptr(), ws.numel()), "cstp_ntxent_backward")
        return dreps, None


def ntxent(reps, temperature):
    """NT-Xent over reps = cat(zjs, zis) [2N, F] (loss/NTXent.py:46-62)."""
    return _NTXent.apply(reps, float(temperature))


NTXQ_MAX_F = 2048


class _NTXentQueue(torch.autograd.Function):
    @staticmethod
    def forward(ctx, reps, queue, n_valid, temperature):
        lib = _lib.load()
        two_n, f = reps.shape
        cap = queue.shape[0]
        nbytes = lib.cstp_ntxq_workspace_bytes(two_n, f, n_valid)
        if nbytes == 0:
            raise _lib.CstpError("ntxent_queue: unsupported shape reps [%d, %d], n_valid %d (rows even in 4..8192, features in "
                                 "1..%d)" % (two_n, f, n_valid, NTXQ_MAX_F))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=reps.device)  # private: lives until backward
        loss = torch.empty(1, dtype=torch.float32, device=reps.device)
        check(lib.cstp_ntxq_forward(_stream(), reps.data_ptr(), queue.data_ptr(), loss.data_ptr(), two_n, f, cap, n_valid,
                                    temperature, ws.data_ptr(), ws.numel()), "cstp_ntxq_forward")
        ctx.save_for_backward(reps, queue, ws)
        ctx.n_valid, ctx.temperature = n_valid, temperature
        return loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        lib = _lib.load()
        reps, queue, ws = ctx.saved_tensors
        dloss = _req(dloss.reshape(1), "ntxent_queue grad_output")
        dreps = torch.empty_like(reps)
        check(lib.cstp_ntxq_backward(_stream(), reps.data_ptr(), queue.data_ptr(), dloss.data_ptr(), dreps.data_ptr(),
                                     reps.shape[0], reps.shape[1], queue.shape[0], ctx.n_valid, ctx.temperature, ws.data_ptr(),
                                     ws.numel()), "cstp_ntxq_backward")
        return dreps, None, None, None


def _ntxq_operands(what, reps, queue):
    for t, name in ((reps, "%s representations" % what), (queue, "%s queue" % what)):
        if not t.is_cuda:
            raise _lib.CstpError("%s must be on a HIP device (cstp_amd has no CPU path)" % name)
        if t.dtype != torch.float32:
            raise _lib.CstpError("%s must be float32, got %s" % (name, t.dtype))
        if t.dim() != 2:
            raise _lib.CstpError("%s must be [rows, features], got %s" % (name, tuple(t.shape)))
        if not t.is_contiguous():
            raise _lib.CstpError("%s must be contiguous" % name)
    if reps.shape[1] != queue.shape[1]:
        raise _lib.CstpError("%s: the representations have %d features, the queue %d" % (what, reps.shape[1], queue.shape[1]))
    if reps.device != queue.device:
        raise _lib.CstpError("%s: the representations are on %s, the queue on %s" % (what, reps.device, queue.device))


def ntxent_queue(reps, queue, n_valid, temperature):
    """NT-Xent over reps = cat(zjs, zis) [2N, F] with rows [0, n_valid) of ``queue`` [cap, F] as extra negatives of every row
    (include/cstp_hip.h: cstp_ntxq_forward).  The queue's rows are constants of unit length (ntxent_queue_push writes them): no
    gradient reaches it, neither pass writes it and rows from n_valid on are not read.  The [2N, n_valid] score matrix is never
    built (csrc/ntxq.h).  n_valid == 0 IS ``ntxent(reps, temperature)``: the same call, the same bits."""
    _ntxq_operands("ntxent_queue", reps, queue)
    if isinstance(n_valid, bool) or not isinstance(n_valid, int) or not 0 <= n_valid <= queue.shape[0]:
        raise _lib.CstpError("ntxent_queue: n_valid must be an int in [0, %d], got %r" % (queue.shape[0], n_valid))
    if n_valid == 0:
        return ntxent(reps, temperature)
    return _NTXentQueue.apply(reps, queue, n_valid, float(temperature))


def ntxent_queue_splits(two_n, f, n_valid):
    """Blocks along the queue per 64-row tile that ntxent_queue uses for these sizes (0 for an empty queue), read off the
    workspace size: cstp_ntxq_workspace_bytes = the in-batch block + nsplit * two_n * (2 + f) floats."""
    lib = _lib.load()
    total, base = lib.cstp_ntxq_workspace_bytes(two_n, f, n_valid), lib.cstp_ntxent_workspace_bytes(two_n, f)
    if total == 0:
        raise _lib.CstpError("ntxent_queue_splits: unsupported sizes (%d, %d, %d)" % (two_n, f, n_valid))
    return (total - base) // (two_n * (2 + f) * 4)


def ntxent_queue_push(reps, queue, ptr):
    """queue[ptr + i] <- reps[i] / max(|reps[i]|, 1e-8) for every row of reps [R, F] (cstp_ntxq_push); ptr + R <= cap is the
    caller's to guarantee (NTXentLoss keeps cap a multiple of R).  One launch on the current stream; no autograd."""
    _ntxq_operands("ntxent_queue_push", reps, queue)
    r, cap = reps.shape[0], queue.shape[0]
    if isinstance(ptr, bool) or not isinstance(ptr, int) or ptr < 0 or ptr + r > cap:
        raise _lib.CstpError("ntxent_queue_push: rows [%r, %r + %d) do not lie inside a queue of %d rows" % (ptr, ptr, r, cap))
    lib = _lib.load()
    check(lib.cstp_ntxq_push(_stream(), reps.detach().data_ptr(), queue.data_ptr(), r, reps.shape[1], cap, ptr), "cstp_ntxq_push")


SIM_TOPK_MAX_K = 64


def sim_topk(q, g, k, exclude_self=False):
    """The k most similar rows of g [ng, d] for every row of q [nq, d] (dot products; L2-normalise both first for cosine):
    -> (val [nq, k] fp32, idx [nq, k] int32), by similarity descending, the lower gallery row first where two similarities are
    bit-equal, (-inf, -1) where candidates run out.  ``exclude_self``: q and g are the same set, row i skips candidate i.
    The [nq, ng] matrix never exists (csrc/retrieve.hip); scratch grows with nq * k.  No autograd."""
    if q.dim() != 2 or g.dim() != 2:
        raise _lib.CstpError("sim_topk expects [rows, features] tensors, got %s and %s" % (tuple(q.shape), tuple(g.shape)))
    if q.shape[1] != g.shape[1]:
        raise _lib.CstpError("sim_topk: queries have %d features, the gallery %d" % (q.shape[1], g.shape[1]))
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= SIM_TOPK_MAX_K:
        raise _lib.CstpError("sim_topk: k must be an int in 1..%d, got %r" % (SIM_TOPK_MAX_K, k))
    for t, name in ((q, "sim_topk queries"), (g, "sim_topk gallery")):      # the dtype first: _req asks for the device first
        if t.dtype != torch.float32:
            raise _lib.CstpError("%s must be float32, got %s" % (name, t.dtype))
    q, g = _req(q.detach(), "sim_topk queries"), _req(g.detach(), "sim_topk gallery")
    lib = _lib.load()
    if q.device != g.device:
        raise _lib.CstpError("sim_topk: queries on %s, gallery on %s" % (q.device, g.device))
    nq, d = q.shape
    ng = g.shape[0]
    if nq < 1 or ng < 1 or d < 1:
        raise _lib.CstpError("sim_topk: empty operand %s x %s" % (tuple(q.shape), tuple(g.shape)))
    nbytes = lib.cstp_simtopk_workspace_bytes(nq, ng, d, k)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device)      # private and exact: not the geometric arena
    val = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    idx = torch.empty((nq, k), dtype=torch.int32, device=q.device)
    check(lib.cstp_simtopk(_stream(), q.data_ptr(), g.data_ptr(), nq, ng, d, k, 1 if exclude_self else 0, val.data_ptr(),
                           idx.data_ptr(), ws.data_ptr(), ws.numel()), "cstp_simtopk")
    return val, idx


KNN_VOTE_MAX_TOP = 8


def knn_vote(val, idx, g_labels, temperature, n_top=5):
    """The weighted k-nearest-neighbour vote on a sim_topk answer (val [nq, k] fp32, idx [nq, k] int32) with the gallery's class
    ids g_labels [ng] (int64 or int32, >= 0): slot j weighs exp((val_j - val_0) / temperature), a class scores the sum of its
    slots' weights in slot order, -> (pred [nq, n_top] int32, score [nq, n_top] fp32): the n_top best distinct classes by
    (score descending, class id ascending), (-1, 0) where they run out.  Slots with idx outside 0..ng-1 are dead.
    One launch, no class table, no atomics (include/cstp_hip.h: cstp_knn_vote).  No autograd."""
    if val.dim() != 2 or idx.dim() != 2 or val.shape != idx.shape:
        raise _lib.CstpError("knn_vote expects val and idx of one shape [queries, k], got %s and %s"
                             % (tuple(val.shape), tuple(idx.shape)))
    if g_labels.dim() != 1:
        raise _lib.CstpError("knn_vote: gallery labels must be [gallery rows], got %s" % (tuple(g_labels.shape),))
    if val.dtype != torch.float32:
        raise _lib.CstpError("knn_vote val must be float32, got %s" % (val.dtype,))
    if idx.dtype != torch.int32:
        raise _lib.CstpError("knn_vote idx must be int32, got %s" % (idx.dtype,))
    if g_labels.dtype not in (torch.int64, torch.int32):
        raise _lib.CstpError("knn_vote gallery labels must be int64 or int32, got %s" % (g_labels.dtype,))
    if isinstance(n_top, bool) or not isinstance(n_top, int) or not 1 <= n_top <= KNN_VOTE_MAX_TOP:
        raise _lib.CstpError("knn_vote: n_top must be an int in 1..%d, got %r" % (KNN_VOTE_MAX_TOP, n_top))
    temperature = float(temperature)
    if not (temperature > 0.0 and temperature < float("inf")):
        raise _lib.CstpError("knn_vote: temperature must be finite and positive, got %r" % (temperature,))
    nq, k = val.shape
    ng = g_labels.shape[0]
    if not 1 <= k <= SIM_TOPK_MAX_K:
        raise _lib.CstpError("knn_vote: k must be in 1..%d, got %d" % (SIM_TOPK_MAX_K, k))
    if nq < 1 or ng < 1:
        raise _lib.CstpError("knn_vote: empty operand, %d queries and %d gallery labels" % (nq, ng))
    for t, name in ((val, "knn_vote val"), (idx, "knn_vote idx"), (g_labels, "knn_vote gallery labels")):
        if not t.is_cuda:
            raise _lib.CstpError("%s must be on a HIP device (cstp_amd has no CPU path)" % name)
    if not (val.device == idx.device == g_labels.device):
        raise _lib.CstpError("knn_vote: val on %s, idx on %s, gallery labels on %s" % (val.device, idx.device, g_labels.device))
    lib = _lib.load()
    val, idx = val.detach().contiguous(), idx.contiguous()
    labels = g_labels.to(torch.int32).contiguous()                   # the one conversion
    pred = torch.empty((nq, n_top), dtype=torch.int32, device=val.device)
    score = torch.empty((nq, n_top), dtype=torch.float32, device=val.device)
    check(lib.cstp_knn_vote(_stream(), val.data_ptr(), idx.data_ptr(), labels.data_ptr(), nq, ng, k, 1.0 / temperature, n_top,
                            pred.data_ptr(), score.data_ptr()), "cstp_knn_vote")
    return pred, score


PROBE_MAX_CLASSES = 1024
PROBE_MAX_TOP = 8


def _probe_operands(op, x, w, b, mean, inv_std):
    """The shared checks of probe_step / probe_predict on (x [n, d], w [c, d], b [c], mean / inv_std [d] or None) -> (n, d, c)."""
    if x.dim() != 2:
        raise _lib.CstpError("%s: x must be [rows, features], got %s" % (op, tuple(x.shape)))
    if w.dim() != 2 or w.shape[1] != x.shape[1]:
        raise _lib.CstpError("%s: w must be [classes, %d], got %s" % (op, x.shape[1], tuple(w.shape)))
    n, d = x.shape
    c = w.shape[0]
    if b.dim() != 1 or b.shape[0] != c:
        raise _lib.CstpError("%s: b must be [%d], got %s" % (op, c, tuple(b.shape)))
    for t, name in ((mean, "mean"), (inv_std, "inv_std")):
        if t is not None and (t.dim() != 1 or t.shape[0] != d):
            raise _lib.CstpError("%s: %s must be [%d], got %s" % (op, name, d, tuple(t.shape)))
    for t, name in ((x, "x"), (w, "w"), (b, "b"), (mean, "mean"), (inv_std, "inv_std")):
        if t is not None and t.dtype != torch.float32:
            raise _lib.CstpError("%s: %s must be float32, got %s" % (op, name, t.dtype))
    if not 2 <= c <= PROBE_MAX_CLASSES:
        raise _lib.CstpError("%s: the number of classes c must be in 2..%d, got %d" % (op, PROBE_MAX_CLASSES, c))
    if n < 1 or d < 1:
        raise _lib.CstpError("%s: empty operand, x is %s" % (op, tuple(x.shape)))
    return n, d, c


def _probe_devices(op, named):
    named = [(t, name) for t, name in named if t is not None]
    for t, name in named:
        if not t.is_cuda:
            raise _lib.CstpError("%s: %s must be on a HIP device (cstp_amd has no CPU path)" % (op, name))
    for t, name in named[1:]:
        if t.device != named[0][0].device:
            raise _lib.CstpError("%s: %s on %s, %s on %s" % (op, named[0][1], named[0][0].device, name, t.device))


def _probe_c(op, t, name):
    if not t.is_contiguous():
        raise _lib.CstpError("%s: %s must be contiguous" % (op, name))
    return t


def probe_step(x, labels, w, b, rows=None, mean=None, inv_std=None, out=None):
    """One step of a softmax classifier on rows gathered from the feature matrix x [n, d] fp32 (include/cstp_hip.h:
    cstp_probe_step): labels [n] int64 indexed by the gathered row, rows [m] int32 or None (the whole matrix in order),
    mean / inv_std [d] fp32 or None standardise on load, w [c, d], b [c] -> (loss [1] fp32, hits [1] int32, dw [c, d], db [c]):
    the mean cross-entropy of the batch, the number of rows whose arg-max class is their label, and the gradients of the loss.
    ``out`` = (loss, hits, dw, db) preallocated, contiguous and not aliasing w / b: then nothing is allocated.  Three launches,
    no atomics, no host read, equal bits on equal inputs.  Not an autograd Function: the caller owns the update."""
    op = "probe_step"
    n, d, c = _probe_operands(op, x, w, b, mean, inv_std)
    if labels.dim() != 1 or labels.shape[0] != n:
        raise _lib.CstpError("%s: labels must be [%d], one per row of x, got %s" % (op, n, tuple(labels.shape)))
    if labels.dtype != torch.int64:
        raise _lib.CstpError("%s: labels must be int64, got %s" % (op, labels.dtype))
    if rows is not None:
        if rows.dim() != 1 or rows.shape[0] < 1:
            raise _lib.CstpError("%s: rows must be a non-empty [m] vector, got %s" % (op, tuple(rows.shape)))
        if rows.dtype != torch.int32:
            raise _lib.CstpError("%s: rows must be int32, got %s" % (op, rows.dtype))
    m = n if rows is None else rows.shape[0]
    if out is not None:
        if len(out) != 4:
            raise _lib.CstpError("%s: out must be (loss, hits, dw, db)" % op)
        for t, name, shape, dtype in ((out[0], "out loss", (1,), torch.float32), (out[1], "out hits", (1,), torch.int32),
                                      (out[2], "out dw", (c, d), torch.float32), (out[3], "out db", (c,), torch.float32)):
            if tuple(t.shape) != shape or t.dtype != dtype:
                raise _lib.CstpError("%s: %s must be %s of shape %s, got %s %s" % (op, name, dtype, shape, t.dtype, tuple(t.shape)))
    named = [(x, "x"), (labels, "labels"), (w, "w"), (b, "b"), (rows, "rows"), (mean, "mean"), (inv_std, "inv_std")]
    if out is not None:
        named += [(out[0], "out loss"), (out[1], "out hits"), (out[2], "out dw"), (out[3], "out db")]
    _probe_devices(op, named)
    for t, name in named:
        if t is not None:
            _probe_c(op, t, name)
    lib = _lib.load()
    if out is None:
        out = (torch.empty(1, dtype=torch.float32, device=x.device), torch.empty(1, dtype=torch.int32, device=x.device),
               torch.empty((c, d), dtype=torch.float32, device=x.device), torch.empty(c, dtype=torch.float32, device=x.device))
    loss, hits, dw, db = out
    ws = _workspace(x.device, lib.cstp_probe_workspace_bytes(m, d, c))
    check(lib.cstp_probe_step(_stream(), x.data_ptr(), _ptr(rows), labels.data_ptr(), _ptr(mean), _ptr(inv_std), w.data_ptr(),
                              b.data_ptr(), m, n, d, c, loss.data_ptr(), hits.data_ptr(), dw.data_ptr(), db.data_ptr(),
                              ws.data_ptr(), ws.numel()), "cstp_probe_step")
    return loss, hits, dw, db


def probe_predict(x, w, b, mean=None, inv_std=None, n_top=5):
    """The n_top best classes of every row of x [n, d] under the classifier (w [c, d], b [c]) on the features standardised on load
    -> (pred [n, n_top] int32, score [n, n_top] fp32): classes by (logit descending, class id ascending) and their logits,
    (-1, 0) where n_top > c -- the layout knn_vote writes, so knn.accuracy serves.  One launch, no logits table
    (include/cstp_hip.h: cstp_probe_predict).  No autograd."""
    op = "probe_predict"
    n, d, c = _probe_operands(op, x, w, b, mean, inv_std)
    if isinstance(n_top, bool) or not isinstance(n_top, int) or not 1 <= n_top <= PROBE_MAX_TOP:
        raise _lib.CstpError("%s: n_top must be an int in 1..%d, got %r" % (op, PROBE_MAX_TOP, n_top))
    named = [(x, "x"), (w, "w"), (b, "b"), (mean, "mean"), (inv_std, "inv_std")]
    _probe_devices(op, named)
    for t, name in named:
        if t is not None:
            _probe_c(op, t, name)
    lib = _lib.load()
    pred = torch.empty((n, n_top), dtype=torch.int32, device=x.device)
    score = torch.empty((n, n_top), dtype=torch.float32, device=x.device)
    check(lib.cstp_probe_predict(_stream(), x.data_ptr(), _ptr(mean), _ptr(inv_std), w.data_ptr(), b.data_ptr(), n, d, c, n_top,
                                 pred.data_ptr(), score.data_ptr()), "cstp_probe_predict")
    return pred, score


PROBE_MAX_HEADS = 32


def _pad4(v: int) -> int:
    return (v + 3) // 4 * 4


def probe_head_views(arena: torch.Tensor, heads: int, c: int, d: int):
    """(w [heads, c, d], b [heads, c]) as views of a flat fp32 arena of heads * seg floats, seg = pad4(c d) + pad4(c): head h's
    W at h * seg and b at h * seg + pad4(c d) -- probe.fit's single-head layout, repeated."""
    wn = _pad4(c * d)
    seg = wn + _pad4(c)
    if arena.dim() != 1 or not arena.is_contiguous() or arena.numel() < heads * seg:
        raise _lib.CstpError("probe_head_views: the arena must be flat with at least %d floats, got %s" % (heads * seg, tuple(arena.shape)))
    at = arena.storage_offset()                                   # as_strided counts from the storage, not from the view
    return arena.as_strided((heads, c, d), (seg, d, 1), at), arena.as_strided((heads, c), (seg, 1), at + wn)


def _probe_heads(op, w, b, what="w / b"):
    """The head checks of the sweep calls on (w [G, c, d], b [G, c]) strided views -> (G, head stride in floats)."""
    if w.dim() != 3 or b.dim() != 2 or w.shape[0] != b.shape[0]:
        raise _lib.CstpError("%s: %s must be [heads, classes, features] and [heads, classes], got %s and %s"
                             % (op, what, tuple(w.shape), tuple(b.shape)))
    heads, c, d = w.shape
    if not 1 <= heads <= PROBE_MAX_HEADS:
        raise _lib.CstpError("%s: the number of heads must be in 1..%d, got %d" % (op, PROBE_MAX_HEADS, heads))
    if w.dtype != torch.float32 or b.dtype != torch.float32:
        raise _lib.CstpError("%s: %s must be float32, got %s and %s" % (op, what, w.dtype, b.dtype))
    if c >= 1 and d >= 1 and (w.stride()[1:] != (d, 1) or b.stride(1) != 1):
        raise _lib.CstpError("%s: every head of %s must be contiguous, strides are %s and %s" % (op, what, w.stride(), b.stride()))
    if heads == 1:
        return 1, _pad4(c * d) + _pad4(c)
    if w.stride(0) != b.stride(0):
        raise _lib.CstpError("%s: %s disagree on the head stride: %d and %d floats" % (op, what, w.stride(0), b.stride(0)))
    stride = w.stride(0)
    if stride % 4 or stride < _pad4(c * d) + c:
        raise _lib.CstpError("%s: the head stride of %s must be a multiple of 4 floats and at least pad4(c d) + c = %d, got %d"
                             % (op, what, _pad4(c * d) + c, stride))
    return heads, stride


def _probe_sweep(op, grads, x, labels, w, b, rows, mean, inv_std, out):
    heads, stride = _probe_heads(op, w, b)
    n, d, c = _probe_operands(op, x, w[0], b[0], mean, inv_std)
    if labels.dim() != 1 or labels.shape[0] != n:
        raise _lib.CstpError("%s: labels must be [%d], one per row of x, got %s" % (op, n, tuple(labels.shape)))
    if labels.dtype != torch.int64:
        raise _lib.CstpError("%s: labels must be int64, got %s" % (op, labels.dtype))
    if rows is not None:
        if rows.dim() != 1 or rows.shape[0] < 1:
            raise _lib.CstpError("%s: rows must be a non-empty [m] vector, got %s" % (op, tuple(rows.shape)))
        if rows.dtype != torch.int32:
            raise _lib.CstpError("%s: rows must be int32, got %s" % (op, rows.dtype))
    m = n if rows is None else rows.shape[0]
    n_out = 4 if grads else 2
    if out is not None:
        if len(out) != n_out:
            raise _lib.CstpError("%s: out must be %s" % (op, "(loss, hits, dw, db)" if grads else "(loss, hits)"))
        for t, name, dtype in ((out[0], "out loss", torch.float32), (out[1], "out hits", torch.int32)):
            if tuple(t.shape) != (heads,) or t.dtype != dtype:
                raise _lib.CstpError("%s: %s must be %s of shape (%d,), got %s %s" % (op, name, dtype, heads, t.dtype, tuple(t.shape)))
        if grads:
            if tuple(out[2].shape) != tuple(w.shape) or tuple(out[3].shape) != tuple(b.shape):
                raise _lib.CstpError("%s: out dw / db must have the shapes of w / b, got %s and %s"
                                     % (op, tuple(out[2].shape), tuple(out[3].shape)))
            if _probe_heads(op, out[2], out[3], "out dw / db")[1] != stride:
                raise _lib.CstpError("%s: out dw / db must have the head stride of w / b (%d floats)" % (op, stride))
    named = [(x, "x"), (labels, "labels"), (w, "w"), (b, "b"), (rows, "rows"), (mean, "mean"), (inv_std, "inv_std")]
    if out is not None:
        named += list(zip(out, ("out loss", "out hits", "out dw", "out db")))
    _probe_devices(op, named)
    for t, name in ((x, "x"), (labels, "labels"), (rows, "rows"), (mean, "mean"), (inv_std, "inv_std")) + \
            (((out[0], "out loss"), (out[1], "out hits")) if out is not None else ()):
        if t is not None:
            _probe_c(op, t, name)
    lib = _lib.load()
    if out is None:
        out = (torch.empty(heads, dtype=torch.float32, device=x.device), torch.empty(heads, dtype=torch.int32, device=x.device))
        if grads:
            arena = torch.zeros(heads * stride, dtype=torch.float32, device=x.device)
            off = _pad4(c * d)
            out += (arena.as_strided((heads, c, d), (stride, d, 1), 0), arena.as_strided((heads, c), (stride, 1), off))
    ws = _workspace(x.device, lib.cstp_probe_sweep_workspace_bytes(heads, m, d, c))
    if grads:
        check(lib.cstp_probe_sweep_step(_stream(), x.data_ptr(), _ptr(rows), labels.data_ptr(), _ptr(mean), _ptr(inv_std),
                                        w.data_ptr(), b.data_ptr(), stride, heads, m, n, d, c, out[0].data_ptr(), out[1].data_ptr(),
                                        out[2].data_ptr(), out[3].data_ptr(), ws.data_ptr(), ws.numel()), "cstp_probe_sweep_step")
    else:
        check(lib.cstp_probe_sweep_score(_stream(), x.data_ptr(), _ptr(rows), labels.data_ptr(), _ptr(mean), _ptr(inv_std),
                                         w.data_ptr(), b.data_ptr(), stride, heads, m, n, d, c, out[0].data_ptr(), out[1].data_ptr(),
                                         ws.data_ptr(), ws.numel()), "cstp_probe_sweep_score")
    return out


def probe_sweep_step(x, labels, w, b, rows=None, mean=None, inv_std=None, out=None):
    """probe_step for G <= 32 classifiers on the same batch in the same three launches (include/cstp_hip.h: cstp_probe_sweep_step):
    w [G, c, d] and b [G, c] are strided views of one arena (probe_head_views) that agree on the head stride -> (loss [G] fp32,
    hits [G] int32, dw [G, c, d], db [G, c]), head g's slices holding the bits probe_step gives for (w[g], b[g]) alone.  ``out`` =
    (loss, hits, dw, db) preallocated, dw / db at the stride of w / b and not aliasing them: then nothing is allocated."""
    return _probe_sweep("probe_sweep_step", True, x, labels, w, b, rows, mean, inv_std, out)


def probe_sweep_score(x, labels, w, b, rows=None, mean=None, inv_std=None, out=None):
    """Loss and hit count of every head on the gathered rows, no gradients: two launches, the bits of probe_sweep_step's first two
    results (cstp_probe_sweep_score) -> (loss [G] fp32, hits [G] int32); ``out`` = (loss, hits) preallocated."""
    return _probe_sweep("probe_sweep_score", False, x, labels, w, b, rows, mean, inv_std, out)


KMEANS_MAX_ROWS,KMEANS_MAX_DIM, KMEANS_MAX_CLUSTERS, KMEANS_MAX_RESTARTS = 1 << 24, 4096, 4096, 32


def _kmeans_operands(op, x, cent):
    """The shared checks of kmeans_assign / kmeans_update on (x [n, d], cent [r, c, d]) -> (n, d, c, r)."""
    if x.dim() != 2:
        raise _lib.CstpError("%s: x must be [rows, features], got %s" % (op, tuple(x.shape)))
    if cent.dim() != 3 or cent.shape[2] != x.shape[1]:
        raise _lib.CstpError("%s: cent must be [restarts, clusters, %d], got %s" % (op, x.shape[1], tuple(cent.shape)))
    for t, name in ((x, "x"), (cent, "cent")):
        if t.dtype != torch.float32:
            raise _lib.CstpError("%s: %s must be float32, got %s" % (op, name, t.dtype))
    n, d = x.shape
    r, c = cent.shape[0], cent.shape[1]
    if n < 1 or d < 1 or c < 1 or r < 1:
        raise _lib.CstpError("%s: empty operand, x is %s and cent %s" % (op, tuple(x.shape), tuple(cent.shape)))
    if n > KMEANS_MAX_ROWS or d > KMEANS_MAX_DIM or c > KMEANS_MAX_CLUSTERS or r > KMEANS_MAX_RESTARTS:
        raise _lib.CstpError("%s: at most %d rows, %d features, %d clusters and %d restarts are served, got x %s and cent %s"
                             % (op, KMEANS_MAX_ROWS, KMEANS_MAX_DIM, KMEANS_MAX_CLUSTERS, KMEANS_MAX_RESTARTS, tuple(x.shape),
                                tuple(cent.shape)))
    if c > n:
        raise _lib.CstpError("%s: %d clusters for %d rows: the number of clusters must not exceed the rows" % (op, c, n))
    return n, d, c, r


def _kmeans_assignment(op, t, name, r, n):
    if t.dim() != 2 or tuple(t.shape) != (r, n):
        raise _lib.CstpError("%s: %s must be [%d, %d] (restarts, rows), got %s" % (op, name, r, n, tuple(t.shape)))
    if t.dtype != torch.int32:
        raise _lib.CstpError("%s: %s must be int32, got %s" % (op, name, t.dtype))


def _kmeans_out(op, out, specs, device):
    """``out``: preallocated results, checked against (name, shape, dtype) -- or None: new tensors."""
    if out is None:
        return tuple(torch.empty(shape, dtype=dtype, device=device) for _, shape, dtype in specs)
    if len(out) != len(specs):
        raise _lib.CstpError("%s: out must be (%s)" % (op, ", ".join(name for name, _, _ in specs)))
    for t, (name, shape, dtype) in zip(out, specs):
        if tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            raise _lib.CstpError("%s: out %s must be %s of shape %s, got %s %s" % (op, name, dtype, tuple(shape), t.dtype, tuple(t.shape)))
        if t.device != device or not t.is_contiguous():
            raise _lib.CstpError("%s: out %s must be contiguous and on %s" % (op, name, device))
    return tuple(out)


def kmeans_assign(x, cent, prev=None, out=None):
    """The assignment step of spherical k-means for all restarts in one call (include/cstp_hip.h: cstp_kmeans_assign): x [n, d]
    fp32 rows, cent [r, c, d] fp32 centroids (both L2-normalised by the caller), prev [r, n] int32 or None ->
    (assign [r, n] int32, best [r, n] fp32, moved [r] int32, score [r] fp64): every row's most similar centroid of every restart
    -- the bits of sim_topk(x, cent[s], 1), the lowest id among bit-equal similarities --, the number of rows whose assignment
    differs from prev (n without prev) and the fp64 sum of best in a fixed order.  No [n, c] table, no atomics, nothing read back;
    the scratch is private and exact.  ``out`` = (assign, best, moved, score) preallocated: then only the scratch is allocated.
    No autograd."""
    op = "kmeans_assign"
    n, d, c, r = _kmeans_operands(op, x, cent)
    if prev is not None:
        _kmeans_assignment(op, prev, "prev", r, n)
    named = [(x, "x"), (cent, "cent"), (prev, "prev")]
    _probe_devices(op, named)
    x, cent = x.detach(), cent.detach()
    for t, name in named:
        if t is not None:
            _probe_c(op, t, name)
    lib = _lib.load()
    dev = x.device
    ws = torch.empty(lib.cstp_kmeans_workspace_bytes(n, d, c, r), dtype=torch.uint8, device=dev)    # private and exact
    assign, best, moved, score = _kmeans_out(op, out, (("assign", (r, n), torch.int32), ("best", (r, n), torch.float32),
                                                       ("moved", (r,), torch.int32), ("score", (r,), torch.float64)), dev)
    check(lib.cstp_kmeans_assign(_stream(), x.data_ptr(), cent.data_ptr(), _ptr(prev), n, d, c, r, assign.data_ptr(), best.data_ptr(),
                                 moved.data_ptr(), score.data_ptr(), ws.data_ptr(), ws.numel()), "cstp_kmeans_assign")
    return assign, best, moved, score


def kmeans_update(x, assign, cent, out=None):
    """The centroid step of spherical k-means for all restarts in one call (include/cstp_hip.h: cstp_kmeans_update): x [n, d] fp32,
    assign [r, n] int32, cent [r, c, d] fp32 (the centroids the assignment was made with) -> (cent_new [r, c, d] fp32,
    counts [r, c] int32): the L2-normalised fp32 sum of every cluster's rows, added in ascending row order, and the clusters'
    sizes.  A cluster without rows (or whose sum has no length) keeps its row of ``cent``; an assign value outside 0..c-1 belongs
    to no cluster.  cent_new is a new tensor, or ``out`` = (cent_new, counts) preallocated; it may not overlap ``cent``.  One
    launch, no atomics, equal bits on equal inputs.  No autograd."""
    op = "kmeans_update"
    n, d, c, r = _kmeans_operands(op, x, cent)
    _kmeans_assignment(op, assign, "assign", r, n)
    named = [(x, "x"), (cent, "cent"), (assign, "assign")]
    _probe_devices(op, named)
    x, cent = x.detach(), cent.detach()
    for t, name in named:
        _probe_c(op, t, name)
    lib = _lib.load()
    cent_new, counts = _kmeans_out(op, out, (("cent_new", (r, c, d), torch.float32), ("counts", (r, c), torch.int32)), x.device)
    check(lib.cstp_kmeans_update(_stream(), x.data_ptr(), assign.data_ptr(), cent.data_ptr(), n, d, c, r, cent_new.data_ptr(),
                                 counts.data_ptr()), "cstp_kmeans_update")
    return cent_new, counts


HEALTH_MAX_DIM = 4096


def _health_operand(op, x):
    """The checks of feat_gram / pair_potential on x [n, d] -> (x detached, n, d)."""
    if x.dim() != 2:
        raise _lib.CstpError("%s: x must be [rows, features], got %s" % (op, tuple(x.shape)))
    if x.dtype != torch.float32:
        raise _lib.CstpError("%s: x must be float32, got %s" % (op, x.dtype))
    n, d = x.shape
    if n < 1 or d < 1:
        raise _lib.CstpError("%s: empty operand, x is %s" % (op, tuple(x.shape)))
    if d > HEALTH_MAX_DIM or n * d >= 1 << 31:
        raise _lib.CstpError("%s: at most %d features and fewer than 2^31 elements are served, got x %s"
                             % (op, HEALTH_MAX_DIM, tuple(x.shape)))
    _probe_devices(op, [(x, "x")])
    x = x.detach()
    _probe_c(op, x, "x")
    return x, n, d


def feat_gram(x):
    """x [n, d] fp32 -> (gram [d, d] fp64, colsum [d] fp64): gram[a, b] = sum_i x[i, a] * x[i, b] and colsum[a] = sum_i x[i, a]
    (include/cstp_hip.h: cstp_feat_gram).  Rows go in slabs of 32: one fp32 fmaf chain per pair and slab on the f32 MFMA, the
    slabs added in fp64 in ascending order; gram equals its transpose bit for bit, two calls give equal bits, no atomics.  The
    scratch (ceil(n / 1024) * d doubles) is private and exact.  No autograd."""
    op = "feat_gram"
    x, n, d = _health_operand(op, x)
    lib = _lib.load()
    ws = torch.empty(lib.cstp_feat_gram_workspace_bytes(n, d), dtype=torch.uint8, device=x.device)
    gram = torch.empty((d, d), dtype=torch.float64, device=x.device)
    colsum = torch.empty((d,), dtype=torch.float64, device=x.device)
    check(lib.cstp_feat_gram(_stream(), x.data_ptr(), n, d, gram.data_ptr(), colsum.data_ptr(), ws.data_ptr(), ws.numel()),
          "cstp_feat_gram")
    return gram, colsum


def pair_potential(x, t=2.0):
    """x [n, d] fp32, rows L2-normalised by the caller, t > 0 -> rowsum [n] fp64: rowsum[i] = sum_{j != i} exp(2 t (s_ij - 1)) with
    s_ij the bits of sim_topk's similarity -- for unit rows exp(-t |x_i - x_j|^2), the Gaussian potential of Wang & Isola's
    uniformity (include/cstp_hip.h: cstp_pair_potential).  The gallery streams past resident row tiles as in sim_topk: the [n, n]
    matrix never exists, the scratch is at most 32 doubles per row.  fp32 expf per pair, fp64 sums in a fixed order, row i's own
    column left out by index; no atomics, equal bits on equal inputs.  No autograd."""
    op = "pair_potential"
    if isinstance(t, bool) or not isinstance(t, (int, float)) or not (t > 0.0 and 2.0 * t < 3.0e38):
        raise _lib.CstpError("%s: t must be a finite positive number, got %r" % (op, t))
    x, n, d = _health_operand(op, x)
    lib = _lib.load()
    ws = torch.empty(lib.cstp_pair_potential_workspace_bytes(n, d), dtype=torch.uint8, device=x.device)
    rowsum = torch.empty((n,), dtype=torch.float64, device=x.device)
    check(lib.cstp_pair_potential(_stream(), x.data_ptr(), n, d, float(t), rowsum.data_ptr(), ws.data_ptr(), ws.numel()),
          "cstp_pair_potential")
    return rowsum


FEWSHOT_MAX_WAY, FEWSHOT_MAX_QUERY, FEWSHOT_MAX_SLOTS = 20, 32, 320
FEWSHOT_MAX_SHOTS, FEWSHOT_MAX_SHOT = 4, 16
FEWSHOT_MAX_DIM, FEWSHOT_MAX_EPISODES = 8192, 1 << 20


def fewshot_shots(shots):
    """The shot counts of a call as a tuple: 1..4 ints, strictly ascending, each in 1..16 (CstpError otherwise)."""
    try:
        ks = tuple(shots)
    except TypeError:
        ks = None
    if not ks or len(ks) > FEWSHOT_MAX_SHOTS or any(isinstance(k, bool) or not isinstance(k, int) for k in ks):
        raise _lib.CstpError("fewshot_episodes: shots must be 1..%d ints, got %r" % (FEWSHOT_MAX_SHOTS, shots))
    if any(not 1 <= k <= FEWSHOT_MAX_SHOT for k in ks) or any(b <= a for a, b in zip(ks, ks[1:])):
        raise _lib.CstpError("fewshot_episodes: shots must be strictly ascending in 1..%d, got %r" % (FEWSHOT_MAX_SHOT, ks))
    return ks


def _fewshot_table(t, name, rows):
    """An index table as the kernel wants it.  A CPU table is range-checked against ``rows`` here; a device table is trusted."""
    if t.dtype != torch.int32:
        raise _lib.CstpError("fewshot_episodes: %s must be int32, got %s" % (name, t.dtype))
    _probe_c("fewshot_episodes", t, name)
    if not t.is_cuda:
        lo, hi = int(t.min()), int(t.max())
        if lo < 0 or hi >= rows:
            raise _lib.CstpError("fewshot_episodes: %s holds rows %d..%d, the features have rows 0..%d" % (name, lo, hi, rows - 1))
    return t


def fewshot_episodes(xs, xq, sup_idx, qry_idx, n_query, shots, want_pred=False, want_score=False):
    """N-way K-shot episodes under the cosine nearest-centroid classifier (include/cstp_hip.h: cstp_fewshot_episodes).
    xs [ns, d], xq [nq, d] fp32 with rows L2-normalised by the caller; sup_idx [E, N, Kmax] int32 rows of xs, qry_idx [E, N, Q]
    int32 rows of xq, the query in slot (c, j) belonging to class slot c; shots = (k_1 < ... < k_S), k_S = Kmax.  For every shot
    count the prototype of a class slot is the sum of its FIRST k support columns, a query's score its dot product with the
    prototype over the prototype's norm (0 for a zero prototype), its prediction the best slot, the lowest on a tie.
    -> hits [S, E] int32 on the device (queries answered with their own slot), then pred [S, E, N * Q] int32 and
    score [S, E, N * Q, N] fp32 where asked for.  One launch, one block per episode, no gather tensor, no atomics; equal bits on
    equal inputs, and an episode's bits do not depend on the other episodes or shot counts of the call.
    Index tables given as CPU tensors are range-checked against ns / nq and then uploaded; tables already on the device ARE TAKEN
    AS VALID -- the kernel reads whatever row they name.  No autograd."""
    op = "fewshot_episodes"
    ks = fewshot_shots(shots)
    for t, name in ((xs, "xs"), (xq, "xq")):
        if t.dim() != 2:
            raise _lib.CstpError("%s: %s must be [rows, features], got %s" % (op, name, tuple(t.shape)))
        if t.dtype != torch.float32:
            raise _lib.CstpError("%s: %s must be float32, got %s" % (op, name, t.dtype))
    (ns, d), nq = xs.shape, xq.shape[0]
    if xq.shape[1] != d:
        raise _lib.CstpError("%s: xs has %d features, xq %d" % (op, d, xq.shape[1]))
    if ns < 1 or nq < 1 or d < 1:
        raise _lib.CstpError("%s: empty operand, xs %s and xq %s" % (op, tuple(xs.shape), tuple(xq.shape)))
    if d > FEWSHOT_MAX_DIM:
        raise _lib.CstpError("%s: at most %d features are served, got %d" % (op, FEWSHOT_MAX_DIM, d))
    if sup_idx.dim() != 3 or qry_idx.dim() != 3:
        raise _lib.CstpError("%s: sup_idx must be [episodes, ways, shots] and qry_idx [episodes, ways, queries], got %s and %s"
                             % (op, tuple(sup_idx.shape), tuple(qry_idx.shape)))
    e, n, kmax = sup_idx.shape
    if isinstance(n_query, bool) or not isinstance(n_query, int) or not 1 <= n_query <= FEWSHOT_MAX_QUERY:
        raise _lib.CstpError("%s: n_query must be an int in 1..%d, got %r" % (op, FEWSHOT_MAX_QUERY, n_query))
    if tuple(qry_idx.shape) != (e, n, n_query):
        raise _lib.CstpError("%s: qry_idx must be %s beside sup_idx %s and n_query %d, got %s"
                             % (op, (e, n, n_query), tuple(sup_idx.shape), n_query, tuple(qry_idx.shape)))
    if kmax != ks[-1]:
        raise _lib.CstpError("%s: sup_idx has %d support columns, the largest shot count is %d" % (op, kmax, ks[-1]))
    if not 2 <= n <= FEWSHOT_MAX_WAY or n * n_query > FEWSHOT_MAX_SLOTS:
        raise _lib.CstpError("%s: 2..%d ways and at most %d query slots are served, got %d ways x %d queries"
                             % (op, FEWSHOT_MAX_WAY, FEWSHOT_MAX_SLOTS, n, n_query))
    if not 1 <= e <= FEWSHOT_MAX_EPISODES:
        raise _lib.CstpError("%s: 1..2^20 episodes are served, got %d" % (op, e))
    sup_idx, qry_idx = _fewshot_table(sup_idx, "sup_idx", ns), _fewshot_table(qry_idx, "qry_idx", nq)
    _probe_devices(op, [(xs, "xs"), (xq, "xq")])
    xs, xq = xs.detach(), xq.detach()
    _probe_c(op, xs, "xs")
    _probe_c(op, xq, "xq")
    sup_idx, qry_idx = sup_idx.to(xs.device), qry_idx.to(xs.device)
    lib = _lib.load()
    s = len(ks)
    hits = torch.empty((s, e), dtype=torch.int32, device=xs.device)
    pred = torch.empty((s, e, n * n_query), dtype=torch.int32, device=xs.device) if want_pred else None
    score = torch.empty((s, e, n * n_query, n), dtype=torch.float32, device=xs.device) if want_score else None
    check(lib.cstp_fewshot_episodes(_stream(), xs.data_ptr(), ns, xq.data_ptr(), nq, d, sup_idx.data_ptr(), qry_idx.data_ptr(), e, n,
                                    n_query, (ctypes.c_int32 * s)(*ks), s, hits.data_ptr(), _ptr(pred), _ptr(score)),
          "cstp_fewshot_episodes")
    out = (hits,) + ((pred,) if want_pred else ()) + ((score,) if want_score else ())
    return out[0] if len(out) == 1 else out


# ----------------------------------------------------------------------------------------------
# flat-arena utilities (no autograd)
# ----------------------------------------------------------------------------------------------
def ema_update_(target: torch.Tensor, online: torch.Tensor, m: float) -> None:
    lib = _lib.load()
    assert target.is_cuda and target.is_contiguous() and online.is_contiguous() and target.numel() == online.numel()
    check(lib.cstp_ema_update(_stream(), target.data_ptr(), online.data_ptr(), target.numel(), float(m)), "cstp_ema_update")


def grad_sumsq(g: torch.Tensor, out: torch.Tensor) -> None:
    lib = _lib.load()
    ws = _workspace(g.device, 8192)
    check(lib.cstp_sumsq(_stream(), g.data_ptr(), g.numel(), out.data_ptr(), ws.data_ptr(), ws.numel()), "cstp_sumsq")


def clip_coef(sumsq: torch.Tensor, max_norm: float, coef: torch.Tensor, norm_out: Optional[torch.Tensor]) -> None:
    lib = _lib.load()
    check(lib.cstp_clip_coef(_stream(), sumsq.data_ptr(), float(max_norm), coef.data_ptr(), _ptr(norm_out)), "cstp_clip_coef")


def sgd_step_(p, g, buf, lr: torch.Tensor, momentum: float, weight_decay: float, coef: Optional[torch.Tensor],
              first_step: bool, write_back_grad: bool = True) -> None:
    lib = _lib.load()
    check(lib.cstp_sgd_step(_stream(), p.data_ptr(), g.data_ptr(), buf.data_ptr(), p.numel(), lr.data_ptr(), float(momentum),
                            float(weight_decay), _ptr(coef), 1 if first_step else 0, 1 if write_back_grad else 0),
          "cstp_sgd_step")


LARS_CHUNK = 4096         # CSTP_LARS_CHUNK: floats per block of the LARS kernels; optim.lars_tables deals tensors out in these


def _lars_tables(chunks: torch.Tensor, segs: torch.Tensor, ratio: torch.Tensor):
    for t, name in ((chunks, "chunks"), (segs, "segs")):
        if t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] != 3 or not t.is_contiguous() or not t.is_cuda:
            raise _lib.CstpError("lars %s table must be a contiguous int32 [n, 3] tensor on a HIP device" % name)
    if ratio.dtype != torch.float32 or ratio.numel() != segs.shape[0] or not ratio.is_contiguous():
        raise _lib.CstpError("lars ratio must be float32 [%d]" % segs.shape[0])


def lars_ratio_(p, g, chunks, segs, weight_decay: float, eta: float, coef: Optional[torch.Tensor], ratio) -> None:
    """ratio[s] = the trust ratio q of segment s (include/cstp_hip.h: cstp_lars_ratio); two launches, no host read."""
    lib = _lib.load()
    _lars_tables(chunks, segs, ratio)
    assert p.is_cuda and p.numel() == g.numel()
    ws = _workspace(p.device, lib.cstp_lars_workspace_bytes(chunks.shape[0]))
    check(lib.cstp_lars_ratio(_stream(), p.data_ptr(), g.data_ptr(), p.numel(), chunks.data_ptr(), chunks.shape[0],
                              segs.data_ptr(), segs.shape[0], float(weight_decay), float(eta), _ptr(coef), ratio.data_ptr(),
                              ws.data_ptr(), ws.numel()), "cstp_lars_ratio")


def lars_step_(p, g, buf, chunks, segs, ratio, lr: torch.Tensor, momentum: float, weight_decay: float,
               coef: Optional[torch.Tensor], write_back_grad: bool = True) -> None:
    """The LARS update of every chunk with its segment's ratio (cstp_lars_step); p, g, buf are the WHOLE arenas."""
    lib = _lib.load()
    _lars_tables(chunks, segs, ratio)
    assert p.is_cuda and p.numel() == g.numel() == buf.numel()
    check(lib.cstp_lars_step(_stream(), p.data_ptr(), g.data_ptr(), buf.data_ptr(), p.numel(), chunks.data_ptr(), chunks.shape[0],
                             segs.data_ptr(), segs.shape[0], ratio.data_ptr(), lr.data_ptr(), float(momentum),
                             float(weight_decay), _ptr(coef), 1 if write_back_grad else 0), "cstp_lars_step")


def _tab_tables(chunks: torch.Tensor, hyper: torch.Tensor, arenas) -> None:
    if chunks.dtype != torch.int32 or chunks.dim() != 2 or chunks.shape[1] != 3 or not chunks.is_contiguous() or not chunks.is_cuda:
        raise _lib.CstpError("table-step chunks table must be a contiguous int32 [n, 3] tensor on a HIP device")
    if hyper.dtype != torch.float32 or hyper.dim() != 2 or hyper.shape[1] != 2 or not hyper.is_contiguous() or not hyper.is_cuda:
        raise _lib.CstpError("table-step hyper table must be a contiguous float32 [n_tensors, 2] tensor on a HIP device")
    n = arenas[0].numel()
    for a in arenas:
        if a is not None and (a.dtype != torch.float32 or a.numel() != n or not a.is_contiguous() or a.device != chunks.device):
            raise _lib.CstpError("table-step arenas must be contiguous float32 tensors of one length on the tables' device")


def tab_sgd_step_(p, g, buf, chunks, hyper, lr: torch.Tensor, momentum: float, coef: Optional[torch.Tensor], first_step: bool,
                  write_back_grad: bool = True, ema: Optional[torch.Tensor] = None, ema_momentum: float = 0.0) -> None:
    """cstp_tab_sgd_step: the SGD update of every chunk with its tensor's {lr scale, weight decay} (``hyper``), and with ``ema`` the
    shadow update ema = m * ema + (1 - m) * p in the same launch; p, g, buf, ema are the WHOLE arenas."""
    lib = _lib.load()
    _tab_tables(chunks, hyper, (p, g, buf, ema))
    check(lib.cstp_tab_sgd_step(_stream(), p.data_ptr(), g.data_ptr(), buf.data_ptr(), _ptr(ema), p.numel(), chunks.data_ptr(),
                                chunks.shape[0], hyper.data_ptr(), hyper.shape[0], lr.data_ptr(), float(momentum), _ptr(coef),
                                1 if first_step else 0, 1 if write_back_grad else 0, float(ema_momentum)), "cstp_tab_sgd_step")


def tab_adam_step_(p, g, exp_avg, exp_avg_sq, chunks, hyper, lr: torch.Tensor, beta1: float, beta2: float, eps: float,
                   decoupled: bool, step: int, ema: Optional[torch.Tensor] = None, ema_momentum: float = 0.0) -> None:
    """cstp_tab_adam_step: Adam (coupled decay) / AdamW (decoupled) likewise; ``step`` counts from 1."""
    lib = _lib.load()
    _tab_tables(chunks, hyper, (p, g, exp_avg, exp_avg_sq, ema))
    check(lib.cstp_tab_adam_step(_stream(), p.data_ptr(), g.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), _ptr(ema),
                                 p.numel(), chunks.data_ptr(), chunks.shape[0], hyper.data_ptr(), hyper.shape[0], lr.data_ptr(),
                                 float(beta1), float(beta2), float(eps), 1 if decoupled else 0, int(step), float(ema_momentum)),
          "cstp_tab_adam_step")


def adam_step_(p, g, exp_avg, exp_avg_sq, lr: torch.Tensor, beta1: float, beta2: float, eps: float, weight_decay: float,
               decoupled: bool, step: int) -> None:
    lib = _lib.load()
    check(lib.cstp_adam_step(_stream(), p.data_ptr(), g.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), p.numel(),
                             lr.data_ptr(), float(beta1), float(beta2), float(eps), float(weight_decay),
                             1 if decoupled else 0, int(step)), "cstp_adam_step")

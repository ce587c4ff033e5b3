"""LARS (--optimizer lars), the parts that need no GPU: the flags, the C ABI of the two entry points (declared, bound, exported at
ABI 18, refusing bad arguments before any HIP call), the chunk tables of optim.lars_tables, and FlatLARS's checkpoint format on
CPU arena tensors."""
import ctypes
import os
import re

import pytest
import torch

from test_abi import HEADER, header_symbols

NAMES = ("cstp_lars_ratio", "cstp_lars_step", "cstp_lars_chunk", "cstp_lars_workspace_bytes")


def test_opts_carry_the_lars_flags():
    from cstp_amd.opts import parse_opts
    o = parse_opts(["--optimizer", "lars"])
    assert o.optimizer == "lars" and o.lars_eta == 1e-3
    assert parse_opts(["--optimizer", "lars", "--lars_eta", "0.02"]).lars_eta == 0.02
    assert parse_opts([]).optimizer == "sgd"


def _declared_arity(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    args = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1).strip()
    return 0 if args in ("", "void") else len(args.split(","))


def test_lars_entry_points_are_declared_bound_and_exported():
    from cstp_amd import _lib, ops
    syms = header_symbols()
    for n in NAMES:
        assert n in syms and n in _lib.SIGNATURES
        assert _declared_arity(n) == len(_lib.SIGNATURES[n][1]), n
    assert _lib.ABI_VERSION == 18                       # added without a bump
    assert "#define CSTP_ABI_VERSION 18" in open(HEADER).read()
    assert "#define CSTP_LARS_CHUNK %d\n" % ops.LARS_CHUNK in open(HEADER).read()
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n)
    assert lib.cstp_abi_version() == 18
    assert lib.cstp_lars_chunk() == ops.LARS_CHUNK and ops.LARS_CHUNK % 1024 == 0


def test_lars_entry_points_refuse_bad_arguments_before_any_hip_call():
    from cstp_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)                           # never dereferenced: the checks fail first
    odd = ctypes.c_void_p(20)                           # 4-byte aligned only
    big = 1 << 20
    n = 4096
    # (stream, p, g, n, chunks, n_chunks, segs, n_segs, wd, eta, coef, ratio, ws, ws_bytes)
    ratio_calls = [
        ((None, None, one, n, one, 3, one, 2, 0.0, 1e-3, None, one, one, big), b"null argument"),
        ((None, one, None, n, one, 3, one, 2, 0.0, 1e-3, None, one, one, big), b"null argument"),
        ((None, one, one, n, None, 3, one, 2, 0.0, 1e-3, None, one, one, big), b"null argument"),
        ((None, one, one, n, one, 3, None, 2, 0.0, 1e-3, None, one, one, big), b"null argument"),
        ((None, one, one, n, one, 3, one, 2, 0.0, 1e-3, None, None, one, big), b"null argument"),
        ((None, one, one, n, one, 3, one, 2, 0.0, 1e-3, None, one, None, big), b"null argument"),
        ((None, one, one, n, one, 0, one, 2, 0.0, 1e-3, None, one, one, big), b"bad table size"),
        ((None, one, one, n, one, -1, one, 2, 0.0, 1e-3, None, one, one, big), b"bad table size"),
        ((None, one, one, n, one, 3, one, 0, 0.0, 1e-3, None, one, one, big), b"bad table size"),
        ((None, one, one, n, one, 3, one, 4, 0.0, 1e-3, None, one, one, big), b"bad table size"),       # more tensors than chunks
        ((None, one, one, 0, one, 3, one, 2, 0.0, 1e-3, None, one, one, big), b"arena must hold"),
        ((None, one, one, 1 << 31, one, 3, one, 2, 0.0, 1e-3, None, one, one, big), b"arena must hold"),
        ((None, one, one, n, one, 3, one, 2, 0.0, 1e-3, None, one, one, 3 * 16 - 1), b"workspace too small"),
        ((None, odd, one, n, one, 3, one, 2, 0.0, 1e-3, None, one, one, big), b"16-byte aligned"),
        ((None, one, odd, n, one, 3, one, 2, 0.0, 1e-3, None, one, one, big), b"16-byte aligned"),
    ]
    for args, needle in ratio_calls:
        rc = lib.cstp_lars_ratio(*args)
        msg = lib.cstp_last_error()
        assert rc != 0 and needle in msg and b"line" in msg, (args, rc, msg)
    # (stream, p, g, buf, n, chunks, n_chunks, segs, n_segs, ratio, lr, momentum, wd, coef, write_back)
    step_calls = [
        ((None, None, one, one, n, one, 3, one, 2, one, one, 0.9, 0.0, None, 1), b"null argument"),
        ((None, one, None, one, n, one, 3, one, 2, one, one, 0.9, 0.0, None, 1), b"null argument"),
        ((None, one, one, None, n, one, 3, one, 2, one, one, 0.9, 0.0, None, 1), b"null argument"),
        ((None, one, one, one, n, None, 3, one, 2, one, one, 0.9, 0.0, None, 1), b"null argument"),
        ((None, one, one, one, n, one, 3, None, 2, one, one, 0.9, 0.0, None, 1), b"null argument"),
        ((None, one, one, one, n, one, 3, one, 2, None, one, 0.9, 0.0, None, 1), b"null argument"),
        ((None, one, one, one, n, one, 3, one, 2, one, None, 0.9, 0.0, None, 1), b"null argument"),
        ((None, one, one, one, n, one, 0, one, 2, one, one, 0.9, 0.0, None, 1), b"bad table size"),
        ((None, one, one, one, n, one, 3, one, 0, one, one, 0.9, 0.0, None, 1), b"bad table size"),
        ((None, one, one, one, 1 << 31, one, 3, one, 2, one, one, 0.9, 0.0, None, 1), b"arena must hold"),
        ((None, one, one, odd, n, one, 3, one, 2, one, one, 0.9, 0.0, None, 1), b"16-byte aligned"),
        ((None, odd, one, one, n, one, 3, one, 2, one, one, 0.9, 0.0, None, 1), b"16-byte aligned"),
    ]
    for args, needle in step_calls:
        rc = lib.cstp_lars_step(*args)
        msg = lib.cstp_last_error()
        assert rc != 0 and needle in msg and b"line" in msg, (args, rc, msg)
    assert lib.cstp_lars_workspace_bytes(0) == 0 and lib.cstp_lars_workspace_bytes(-3) == 0
    assert lib.cstp_lars_workspace_bytes(7) == 7 * 16


def test_lars_ops_refuse_cpu_tables():
    from cstp_amd import ops
    from cstp_amd._lib import CstpError
    p = torch.zeros(8)
    t = torch.zeros((1, 3), dtype=torch.int32)
    with pytest.raises(CstpError, match="HIP device"):
        ops.lars_ratio_(p, p, t, t, 0.0, 1e-3, None, torch.zeros(1))


def _layout(shapes):
    offs, n = [], 0
    for s in shapes:
        offs.append(n)
        n += (int(torch.Size(s).numel()) + 3) // 4 * 4
    return offs, n


def test_lars_tables_cover_every_trainable_tensor_once():
    from cstp_amd import ops
    from cstp_amd.optim import lars_tables
    C = ops.LARS_CHUNK
    shapes = [(1,), (3, 1), (4,), (5, 1), (64,), (C - 1,), (C, 1), (C + 1,), (2 * C + 5, 1)]
    frozen = 4                                                               # the (64,) tensor in the middle
    offs, total = _layout(shapes)
    live = [i for i in range(len(shapes)) if i != frozen]
    slots = [(offs[i], int(torch.Size(shapes[i]).numel()), len(shapes[i]) > 1) for i in live]
    chunks, segs = lars_tables(slots, C)
    hits = [0] * total
    for seg, off, length in chunks:
        i = live[seg]
        numel = int(torch.Size(shapes[i]).numel())
        assert off % 4 == 0 and length % 4 == 0 and 0 < length <= C
        assert offs[i] <= off and off + length <= offs[i] + (numel + 3) // 4 * 4         # inside ONE tensor's padded extent
        for k in range(off, off + length):
            hits[k] += 1
    for i, s in enumerate(shapes):
        pad = (int(torch.Size(s).numel()) + 3) // 4 * 4
        assert set(hits[offs[i]:offs[i] + pad]) == ({0} if i == frozen else {1}), i
    assert len(segs) == len(live)
    assert [a for _, _, a in segs] == [1 if len(shapes[i]) > 1 else 0 for i in live]
    nxt = 0
    for s, (first, count, _) in enumerate(segs):                             # a segment's chunks are consecutive, in offset order
        assert first == nxt and count >= 1
        assert [c[0] for c in chunks[first:first + count]] == [s] * count
        assert [c[1] for c in chunks[first:first + count]] == sorted(c[1] for c in chunks[first:first + count])
        nxt = first + count
    assert nxt == len(chunks)
    counts = {live[s]: c for s, (_, c, _) in enumerate(segs)}
    assert counts[5] == 1 and counts[6] == 1 and counts[7] == 2 and counts[8] == 3
    with pytest.raises(ValueError):
        lars_tables([(2, 5, True)], C)                                       # a tensor that starts off a 16-byte boundary
    with pytest.raises(ValueError):
        lars_tables([((1 << 31) - 8, 16, True)], C)                          # past int32


class _Opts:
    optimizer, learning_rate, momentum, weight_decay, lars_eta = "lars", 0.1, 0.9, 1e-4, 0.02


def _cpu_model():
    shapes = [(5, 7), (7,), (3, 2, 1, 2, 2), (3,)]
    offs, total = _layout(shapes)
    arenas = {"param": torch.zeros(total), "grad": torch.zeros(total)}
    gen = torch.Generator().manual_seed(3)
    params = []
    for s, o in zip(shapes, offs):
        n = int(torch.Size(s).numel())
        p = torch.nn.Parameter(torch.empty(0))
        arenas["param"][o:o + n] = torch.randn(n, generator=gen)
        p.data = arenas["param"][o:o + n].view(s)
        p.grad = arenas["grad"][o:o + n].view(s)
        params.append(p)
    return params, arenas


def test_flat_lars_state_dict_round_trip_and_sgd_wire_format():
    from cstp_amd.optim import FlatLARS, build_optimizer
    params, arenas = _cpu_model()
    opt = build_optimizer(_Opts, params, arenas)
    assert isinstance(opt, FlatLARS)
    g = opt.param_groups[0]
    assert (g["lr"], g["momentum"], g["weight_decay"], g["eta"]) == (0.1, 0.9, 1e-4, 0.02)
    assert not opt.state_dict()["state"]                                     # no step taken: no state, as torch.optim.SGD
    gen = torch.Generator().manual_seed(4)
    for _, off, _, numel, _ in opt._slots:                                   # what a step leaves behind (a step needs the GPU);
        opt._buf[off:off + numel] = torch.randn(numel, generator=gen)        # the padding between tensors stays zero
    opt._steps = 1
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [0, 1, 2, 3]
    for i, p in enumerate(params):
        assert sd["state"][i]["momentum_buffer"].shape == p.shape
    assert sd["param_groups"][0]["eta"] == 0.02 and sd["param_groups"][0]["params"] == [0, 1, 2, 3]

    params2, arenas2 = _cpu_model()
    fresh = FlatLARS(params2, lr=0.5, momentum=0.0, weight_decay=0.0, eta=1e-3, arenas=arenas2)
    fresh.load_state_dict(sd)
    assert torch.equal(fresh._buf, opt._buf) and fresh._steps == 1
    g2 = fresh.param_groups[0]
    assert (g2["lr"], g2["momentum"], g2["weight_decay"], g2["eta"]) == (0.1, 0.9, 1e-4, 0.02)
    sd2 = fresh.state_dict()
    for i in range(4):
        assert torch.equal(sd2["state"][i]["momentum_buffer"], sd["state"][i]["momentum_buffer"])

    # the same dict loads into torch.optim.SGD over the same parameter list (the reference's optimizer) and steps there
    ref = torch.optim.SGD([torch.nn.Parameter(p.detach().clone()) for p in params], lr=0.3)
    ref.load_state_dict(sd)
    assert ref.param_groups[0]["lr"] == 0.1 and ref.param_groups[0]["momentum"] == 0.9
    for i, p in enumerate(ref.param_groups[0]["params"]):
        assert torch.equal(ref.state[p]["momentum_buffer"], sd["state"][i]["momentum_buffer"])
        p.grad = torch.zeros_like(p)
    ref.step()


def test_flat_lars_keeps_frozen_tensors_out_of_state_and_tables():
    from cstp_amd.optim import FlatLARS
    params, arenas = _cpu_model()
    params[1].requires_grad = False
    groups = [{"params": p} if p.requires_grad else {"params": p, "lr": 0.0} for p in params]
    opt = FlatLARS(groups, lr=0.1, momentum=0.9, weight_decay=1e-4, arenas=arenas)
    runs = opt._plan()
    assert [(off, n) for off, n, _, _ in runs] == [(0, 36), (44, 28)]          # (5,7) | frozen (7,) | (3,2,1,2,2) + (3,)
    opt._steps = 1
    assert sorted(opt.state_dict()["state"]) == [0, 2, 3]


def test_build_optimizer_still_refuses_an_unknown_name():
    from cstp_amd.optim import build_optimizer

    class Bad(_Opts):
        optimizer = "lamb"
    params, arenas = _cpu_model()
    with pytest.raises(ValueError, match="lars"):
        build_optimizer(Bad, params, arenas)

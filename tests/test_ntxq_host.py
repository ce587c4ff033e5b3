"""NT-Xent with a queue of negatives, everything that needs no GPU: the specification against the oracle and against its own
bar, the flag, the ring buffer of cstp_amd.ntxent.NTXentLoss driven with injected CPU kernels, the C ABI's refusals, and two gloo
ranks that end with equal queues."""
import ctypes
import os
import re

import pytest
import torch

import ntxq_spec as spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cstp_ntxq_workspace_bytes", "cstp_ntxq_forward", "cstp_ntxq_backward", "cstp_ntxq_push")


# ---- the specification ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,f,T", [(2, 30, 0.5), (5, 63, 0.1), (40, 33, 0.01)])
def test_ref_with_an_empty_queue_is_the_oracle(n, f, T):
    from oracle import r21d_byol_oracle as orc
    reps, queue = spec.inputs(n, f, 0, 8, 99)
    got = spec.ref(reps, queue, 0, T, torch.float64)
    zj, zi = reps[:n].double(), reps[n:].double()
    assert abs(float(got["loss"]) - float(orc.ntxent(zi, zj, T))) < 1e-12


@pytest.mark.parametrize("case", spec.CASES, ids=str)
def test_fp32_reference_is_inside_the_bar(case):
    """The bar is a condition on the cases: plain fp32 torch meets it on every input the GPU test uses."""
    n, f, n_valid, cap, T, seed = case
    reps, queue = spec.inputs(n, f, n_valid, cap, seed)
    err = spec.errors(spec.ref(reps, queue, n_valid, T, torch.float32), spec.case_ref(case))
    print("NTXQ fp32", case, err)
    assert err["loss"] < spec.BAR and err["dreps"] < spec.BAR


def test_naive_evaluation_leaves_the_bar():
    """1/T = 100 with a negative at cosine 1: exp(100) overflows fp32, so the max-subtraction is needed."""
    n, f, n_valid, cap, T, seed = spec.OVERFLOW_CASE
    reps, queue = spec.inputs(n, f, n_valid, cap, seed)
    err = spec.errors(spec.ref(reps, queue, n_valid, T, torch.float32, naive=True), spec.case_ref(spec.OVERFLOW_CASE))
    assert not (err["loss"] < spec.BAR and err["dreps"] < spec.BAR)


def test_cases_cover_what_they_claim():
    assert {c[0] for c in spec.CASES} == {2, 3, 40}
    assert {c[2] for c in spec.CASES} >= {1, 127, 128, 129, 300}
    assert {c[1] for c in spec.CASES} == {30, 33, 128, 512, 1024, 2048}
    assert {c[4] for c in spec.CASES} == {0.5, 0.07, 0.01}
    for n, f, n_valid, cap, T, seed in spec.CASES:
        reps, queue = spec.inputs(n, f, n_valid, cap, seed)
        cos = float((spec.normalize(reps[1:2].double()) @ queue[0].double()))
        assert abs(cos - 1.0) < 1e-6 and n_valid <= cap


# ---- the flag ---------------------------------------------------------------------------------------------------------------
def test_flag_parses_and_defaults_to_off():
    from cstp_amd.opts import parse_opts
    assert parse_opts([]).ntxent_queue == 0
    assert parse_opts(["--ntxent_queue", "65536"]).ntxent_queue == 65536
    import cstp_amd.opts as o
    assert "--ntxent_queue" in o.__doc__ and "not checkpointed" in o.__doc__.lower()


def test_driver_refuses_unusable_queues():
    import main_byol
    from cstp_amd.opts import parse_opts
    main_byol.check_ntxent_queue_opts(parse_opts([]))                                   # off: nothing to check
    main_byol.check_ntxent_queue_opts(parse_opts(["--ntxent_queue", "128", "--batch_size", "16", "--ntxent_weight", "1"]))
    with pytest.raises(ValueError, match="--ntxent_queue"):
        main_byol.check_ntxent_queue_opts(parse_opts(["--ntxent_queue", "-32", "--ntxent_weight", "1"]))
    with pytest.raises(ValueError, match="multiple of 2 \\* batch_size"):
        main_byol.check_ntxent_queue_opts(parse_opts(["--ntxent_queue", "100", "--batch_size", "16", "--ntxent_weight", "1"]))
    with pytest.raises(ValueError, match="switched off"):
        main_byol.check_ntxent_queue_opts(parse_opts(["--ntxent_queue", "128", "--batch_size", "16"]))


def test_loss_module_refuses_bad_queue_sizes():
    from cstp_amd.ntxent import NTXentLoss
    for bad in (-8, 12, 7):
        with pytest.raises(ValueError, match="--ntxent_queue"):
            NTXentLoss(device="cpu", batch_size=4, temperature=0.5, gather=False, queue_size=bad)


# ---- the ring ---------------------------------------------------------------------------------------------------------------
def _cpu_loss(reps, queue, n_valid, T):
    r = reps
    nr = r.norm(dim=1, keepdim=True)
    s = (r @ r.t()) / torch.clamp(nr * nr.t(), min=1e-8) / T
    logits = s.masked_fill(torch.eye(r.shape[0], dtype=torch.bool), float("-inf"))
    if n_valid:
        logits = torch.cat([logits, (r / nr.clamp_min(1e-8)) @ queue[:n_valid].to(r.dtype).t() / T], dim=1)
    idx = torch.arange(r.shape[0])
    return (torch.logsumexp(logits, dim=1) - s[idx, (idx + r.shape[0] // 2) % r.shape[0]]).mean()


def _cpu_push(reps, queue, ptr):
    assert not reps.requires_grad
    queue[ptr:ptr + reps.shape[0]] = spec.normalize(reps)


def test_ring_with_injected_kernels():
    """cap = 3 pushes of R = 8 rows, 2 * cap / R + 1 = 7 steps: the loss sees the queue as it stood before its own step's push,
    and after every step the buffer holds exactly the most recent rows, normalised, in push order."""
    from cstp_amd.ntxent import NTXentLoss
    b, f, cap = 4, 6, 24
    R = 2 * b
    seen = []

    def loss_kernel(reps, queue, n_valid, T):
        seen.append((queue.clone(), n_valid))
        return _cpu_loss(reps, queue, n_valid, T)

    def never(*a):
        raise AssertionError("the queue-less kernel must not run with a queue")

    ntx = NTXentLoss(device="cpu", batch_size=b, temperature=0.5, gather=False, kernel=never, queue_size=cap,
                     queue_kernel=loss_kernel, push_kernel=_cpu_push)
    g = torch.Generator().manual_seed(5)
    want = torch.zeros(cap, f)
    pushed = []
    for step in range(2 * cap // R + 1):
        zi = torch.randn(b, f, generator=g, requires_grad=True)
        zj = torch.randn(b, f, generator=g, requires_grad=True)
        before = want.clone()
        loss = ntx(zi, zj)
        assert ntx.ptr == (step * R) % cap        # the backward pass re-reads the queue: the push waits for its end
        loss.backward()
        assert zi.grad is not None and torch.isfinite(zi.grad).all()
        q_seen, nv_seen = seen[-1]
        assert nv_seen == min(step * R, cap) and torch.equal(q_seen, before)
        rows = spec.normalize(torch.cat([zj, zi], 0).detach())
        want[(step * R) % cap:(step * R) % cap + R] = rows
        pushed.append(rows)
        assert ntx.ptr == ((step + 1) * R) % cap and ntx.n_valid == min((step + 1) * R, cap)
        assert torch.equal(ntx.queue, want) and not ntx.queue.requires_grad
        live = ntx.queue[:ntx.n_valid]
        assert float((live.norm(dim=1) - 1).abs().max()) < 1e-6
        recent = torch.cat(pushed[-(cap // R):], 0)           # the most recent rows, oldest first
        ring = torch.roll(ntx.queue[:ntx.n_valid], -ntx.ptr, 0) if ntx.n_valid == cap else live
        assert torch.equal(ring, recent)


def test_ring_without_grad_pushes_at_once():
    from cstp_amd.ntxent import NTXentLoss
    ntx = NTXentLoss(device="cpu", batch_size=2, temperature=0.5, gather=False, queue_size=8, queue_kernel=_cpu_loss,
                     push_kernel=_cpu_push)
    z = torch.randn(2, 5)
    with torch.no_grad():
        ntx(z, z + 1)
    assert ntx.ptr == 4 and ntx.n_valid == 4 and torch.equal(ntx.queue[:4], spec.normalize(torch.cat([z + 1, z], 0)))
    ntx(z, z + 1)                                              # embeddings that need no gradient
    assert ntx.ptr == 0 and ntx.n_valid == 8


def test_queue_size_zero_is_todays_call():
    from cstp_amd.ntxent import NTXentLoss
    calls = []

    def kern(reps, T):
        calls.append((reps.clone(), T))
        return reps.sum()

    def never(*a):
        raise AssertionError("no queue kernel may run with queue_size=0")

    zi, zj = torch.randn(4, 3), torch.randn(4, 3)
    a = NTXentLoss(device="cpu", batch_size=4, temperature=0.3, gather=False, kernel=kern)(zi, zj)
    mod = NTXentLoss(device="cpu", batch_size=4, temperature=0.3, gather=False, kernel=kern, queue_size=0, queue_kernel=never,
                     push_kernel=never)
    b = mod(zi, zj)
    assert torch.equal(a, b) and len(calls) == 2 and calls[0][1] == calls[1][1] == 0.3
    assert torch.equal(calls[0][0], calls[1][0]) and torch.equal(calls[1][0], torch.cat([zj, zi], 0))
    assert not hasattr(mod, "queue")


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_header_and_binding_table_agree():
    from cstp_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cstp_hip.h")).read(), flags=re.S)
    for name in SYMBOLS:
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
    assert _lib.ABI_VERSION == 18 and _lib.load().cstp_abi_version() == 18


def test_refusals_without_gpu():
    """Every refusal comes with a (line N) message before any HIP call: the pointers here are never dereferenced."""
    from cstp_amd import _lib
    lib = _lib.load()
    P = 4096                                                   # a non-null address that no refused call touches
    ws = lib.cstp_ntxq_workspace_bytes(8, 64, 100)
    assert ws >= lib.cstp_ntxent_workspace_bytes(8, 64) + 8 * (2 + 64) * 4
    assert lib.cstp_ntxq_workspace_bytes(8, 64, 0) == lib.cstp_ntxent_workspace_bytes(8, 64)
    for bad in ((7, 64, 10), (2, 64, 10), (8, 0, 10), (8, 2049, 10), (8, 64, -1)):
        assert lib.cstp_ntxq_workspace_bytes(*bad) == 0

    def fwd(reps=P, queue=P, loss=P, R=8, f=64, cap=128, n_valid=100, T=0.5, w=P, nbytes=ws):
        return lib.cstp_ntxq_forward(None, reps, queue, loss, R, f, cap, n_valid, T, w, nbytes)

    def bwd(reps=P, queue=P, dloss=P, dreps=P, R=8, f=64, cap=128, n_valid=100, T=0.5, w=P, nbytes=ws):
        return lib.cstp_ntxq_backward(None, reps, queue, dloss, dreps, R, f, cap, n_valid, T, w, nbytes)

    for call in (fwd, bwd):
        for kw, text in (({"reps": None}, b"null argument"), ({"queue": None}, b"null argument"), ({"w": None}, b"null argument"),
                         ({"R": 7}, b"R must be even"), ({"R": 2}, b"R must be even"), ({"f": 0}, b"f must be in 1..2048"),
                         ({"f": 2049}, b"f must be in 1..2048"), ({"T": 0.0}, b"temperature must be positive"),
                         ({"T": -1.0}, b"temperature must be positive"), ({"n_valid": -1}, b"n_valid must be in [0, cap]"),
                         ({"n_valid": 129}, b"n_valid must be in [0, cap]"), ({"nbytes": ws - 1}, b"workspace too small")):
            assert call(**kw) != 0, kw
            msg = lib.cstp_last_error()
            assert text in msg and re.search(rb"\(line \d+\)", msg), (kw, msg)
    assert fwd(loss=None) != 0 and b"null argument" in lib.cstp_last_error()
    assert bwd(dloss=None) != 0 and b"null argument" in lib.cstp_last_error()
    assert bwd(dreps=None) != 0 and b"null argument" in lib.cstp_last_error()
    for args in ((None, P, 8, 64, 128, 0), (P, None, 8, 64, 128, 0), (P, P, 8, 64, 128, 121), (P, P, 8, 64, 128, -1),
                 (P, P, 8, 2049, 128, 0), (P, P, 0, 64, 128, 0)):
        assert lib.cstp_ntxq_push(None, *args) != 0, args
        assert re.search(rb"\(line \d+\)", lib.cstp_last_error())


def test_ops_refuse_cpu_tensors():
    from cstp_amd import _lib, ops
    reps, queue = torch.randn(4, 8), torch.zeros(16, 8)
    with pytest.raises(_lib.CstpError, match="must be on a HIP device"):
        ops.ntxent_queue(reps, queue, 0, 0.5)
    with pytest.raises(_lib.CstpError, match="must be on a HIP device"):
        ops.ntxent_queue_push(reps, queue, 0)


# ---- two ranks --------------------------------------------------------------------------------------------------------------
def _worker_queue_step(rank, port, q):
    """test_dist_gloo's stub step under the real DistributedDataParallel, with a queue: every rank pushes the gathered rows."""
    import torch.distributed as dist
    import torch.nn.functional as F
    from torch.nn.parallel import DistributedDataParallel
    from cstp_amd.ntxent import NTXentLoss
    from cstp_amd.train import PretrainStep
    import test_dist_gloo as tdg
    tdg._init(rank, port)
    model = tdg._make_stub()
    ddp = DistributedDataParallel(model)
    opt = tdg._CpuFlatSGD(model._arenas, 0.05)
    ntx = NTXentLoss(device="cpu", batch_size=8, temperature=0.5, queue_size=32, queue_kernel=_cpu_loss, push_kernel=_cpu_push)
    step = PretrainStep(ddp, opt, (0.1, 1.0, 1.0, 1.0, 1.0), clip_grad_norm=True, ntxent=ntx, ntxent_weight=0.7,
                        cross_entropy=F.cross_entropy)
    x1, x2, lab = tdg._stub_data()
    sl = slice(4 * rank, 4 * rank + 4)
    vals = []
    for _ in range(3):
        out = step(x1[sl], x2[sl], lab[0][sl], lab[1][sl], lab[2][sl], lab[3][sl], lab[4][sl])
        vals.append(float(out.ntxent))
    q.put((rank, ntx.queue.numpy().copy(), ntx.ptr, ntx.n_valid, vals))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_keep_equal_queues():
    import test_dist_gloo as tdg
    res = sorted(tdg._run(_worker_queue_step, tdg.WORLD), key=lambda r: r[0])
    (_, q0, p0, n0, v0), (_, q1, p1, n1, v1) = res
    assert p0 == p1 == 16 and n0 == n1 == 32
    assert q0.tobytes() == q1.tobytes() and abs(q0).max() > 0
    assert v0 == v1

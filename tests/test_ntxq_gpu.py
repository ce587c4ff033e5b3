"""NT-Xent with a queue of negatives on the HIP kernels (csrc/ntxq.h through ops.ntxent_queue / ops.ntxent_queue_push and
cstp_amd.ntxent.NTXentLoss): parity with tests/ntxq_spec.py at its bar, masking, determinism, the push, the step."""
import pytest
import torch

import ntxq_spec as spec

pytestmark = pytest.mark.gpu
DEV = "cuda"


def run(reps, queue, n_valid, T):
    """loss and dreps of the HIP path on device copies of the inputs (upstream gradient spec.DLOSS), plus the queue afterwards."""
    from cstp_amd import ops
    r = reps.to(DEV).clone().requires_grad_(True)
    q = queue.to(DEV).clone()
    loss = ops.ntxent_queue(r, q, n_valid, T)
    (loss * spec.DLOSS).backward()
    return {"loss": loss.detach(), "dreps": r.grad}, q


@pytest.mark.parametrize("case", spec.CASES, ids=str)
def test_parity_with_the_specification(case):
    n, f, n_valid, cap, T, seed = case
    reps, queue = spec.inputs(n, f, n_valid, cap, seed)
    got, q_after = run(reps, queue, n_valid, T)
    err = spec.errors(got, spec.case_ref(case))
    print("NTXQ hip", case, err)
    assert err["loss"] < spec.BAR and err["dreps"] < spec.BAR
    assert torch.equal(q_after.cpu(), queue)                  # neither pass writes the queue


def test_both_split_counts_occur():
    from cstp_amd import ops
    splits = {case: ops.ntxent_queue_splits(2 * case[0], case[1], case[2]) for case in spec.CASES}
    print("NTXQ splits", splits)
    assert 1 in splits.values() and max(splits.values()) > 1
    assert ops.ntxent_queue_splits(8, 64, 0) == 0


def test_feature_limit_is_refused():
    from cstp_amd import _lib, ops
    reps = torch.randn(6, 2049, device=DEV, requires_grad=True)
    queue = spec.normalize(torch.randn(16, 2049, device=DEV))
    with pytest.raises(_lib.CstpError):
        ops.ntxent_queue(reps, queue, 16, 0.5)
    lib = _lib.load()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    out = torch.empty(1, device=DEV)
    d = torch.empty_like(reps)
    s = torch.cuda.current_stream().cuda_stream
    assert lib.cstp_ntxq_forward(s, reps.data_ptr(), queue.data_ptr(), out.data_ptr(), 6, 2049, 16, 16, 0.5, ws.data_ptr(),
                                 ws.numel()) != 0
    assert b"f must be in 1..2048" in lib.cstp_last_error()
    assert lib.cstp_ntxq_backward(s, reps.data_ptr(), queue.data_ptr(), out.data_ptr(), d.data_ptr(), 6, 2049, 16, 16, 0.5,
                                  ws.data_ptr(), ws.numel()) != 0
    assert b"f must be in 1..2048" in lib.cstp_last_error()


def test_operand_checks():
    from cstp_amd import _lib, ops
    reps = torch.randn(6, 32, device=DEV)
    queue = spec.normalize(torch.randn(16, 32, device=DEV))
    for bad_r, bad_q, nv in ((reps.double(), queue, 4), (reps, queue.half(), 4), (reps.t().contiguous().t(), queue, 4),
                             (reps, queue[:, :16], 4), (reps, queue[:, :16].contiguous(), 4), (reps, queue, 17), (reps, queue, -1),
                             (reps, queue, 1.0)):
        with pytest.raises(_lib.CstpError):
            ops.ntxent_queue(bad_r, bad_q, nv, 0.5)
    for ptr in (-1, 11, 16):
        with pytest.raises(_lib.CstpError):
            ops.ntxent_queue_push(reps, queue, ptr)


@pytest.mark.parametrize("case", [spec.CASES[1], spec.CASES[6]], ids=str)
def test_rows_past_n_valid_are_never_used(case):
    """NaN in rows [n_valid, cap): bit-equal to zeros there (n_valid = 127 leaves one masked row inside the last tile)."""
    n, f, n_valid, cap, T, seed = case
    reps, queue = spec.inputs(n, f, n_valid, cap + 64, seed)
    poisoned = queue.clone()
    poisoned[n_valid:] = float("nan")
    a, _ = run(reps, queue, n_valid, T)
    b, _ = run(reps, poisoned, n_valid, T)
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["dreps"], b["dreps"])
    assert bool(torch.isfinite(a["dreps"]).all())


@pytest.mark.parametrize("n,f,T", [(2, 30, 0.5), (40, 33, 0.01)])
def test_empty_queue_is_ntxent(n, f, T):
    from cstp_amd import ops
    reps, queue = spec.inputs(n, f, 0, 8, 50)
    got, _ = run(reps, queue, 0, T)
    r = reps.to(DEV).clone().requires_grad_(True)
    loss = ops.ntxent(r, T)
    (loss * spec.DLOSS).backward()
    assert torch.equal(got["loss"], loss.detach()) and torch.equal(got["dreps"], r.grad)


@pytest.mark.parametrize("case", [spec.CASES[5], spec.CASES[7]], ids=str)
def test_equal_inputs_give_equal_bits(case):
    n, f, n_valid, cap, T, seed = case
    reps, queue = spec.inputs(n, f, n_valid, cap, seed)
    a, _ = run(reps, queue, n_valid, T)
    b, _ = run(reps, queue, n_valid, T)
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["dreps"], b["dreps"])


def test_no_gradient_reaches_the_queue():
    from cstp_amd import ops
    reps, queue = spec.inputs(3, 33, 127, 128, 2)
    r = reps.to(DEV).requires_grad_(True)
    q = queue.to(DEV).requires_grad_(True)
    ops.ntxent_queue(r, q, 127, 0.07).backward()
    assert q.grad is None and r.grad is not None
    assert torch.equal(q.detach().cpu(), queue)


@pytest.mark.parametrize("R,f,cap,ptr", [(4, 30, 12, 8), (80, 33, 240, 80), (6, 2048, 6, 0)])
def test_push(R, f, cap, ptr):
    """The rows land at [ptr, ptr + R), every other row keeps its bits.  1 ulp: an element is within 2^-23 (relative) of the fp64
    quotient -- the norm rounded to fp32 and the division are one rounding of 2^-24 each -- and a row's length within 2^-23 of 1.
    A zero row is written as zeros (the clamp at 1e-8)."""
    from cstp_amd import ops
    g = torch.Generator().manual_seed(R + f)
    reps = torch.randn(R, f, generator=g) * 3
    reps[1] = 0
    before = torch.randn(cap, f, generator=g)
    q = before.to(DEV).clone()
    ops.ntxent_queue_push(reps.to(DEV), q, ptr)
    q = q.cpu()
    keep = torch.ones(cap, dtype=torch.bool)
    keep[ptr:ptr + R] = False
    assert torch.equal(q[keep], before[keep])
    rows = q[ptr:ptr + R]
    assert torch.equal(rows[1], torch.zeros(f))
    want = spec.normalize(reps.double())
    ulp = 2.0 ** -23
    excess = (rows.double() - want).abs() - ulp * (1 + 2.0 ** -20) * want.abs()      # (1 + e)(1 + e) - 1 = 2e + e^2
    norms = rows.double().norm(dim=1)
    print("NTXQ push", R, f, float(excess.max()), float((torch.cat([norms[:1], norms[2:]]) - 1).abs().max()))
    assert float(excess.max()) <= 0
    assert float((torch.cat([norms[:1], norms[2:]]) - 1).abs().max()) <= ulp


def _step_fixture():
    from oracle import r21d_byol_oracle as orc
    ls = (1, 1, 1, 1)
    sd = orc.closed_form_state(ls, torch.float32)
    x1, x2, labels = orc.closed_form_clips(2, 4, 32, torch.float32)
    return ls, sd, x1.to(DEV), x2.to(DEV), {k: v.to(DEV) for k, v in labels.items()}


def _build_step(ls, sd, **ntx_kwargs):
    from cstp_amd.ntxent import NTXentLoss
    from cstp_amd.optim import FlatSGD
    from cstp_amd.r21d_byol import R21DBYOL
    from cstp_amd.train import PretrainStep
    model = R21DBYOL(pretrain=True, layer_sizes=ls)
    model.load_state_dict(sd)
    model.cuda()
    arenas = model.flatten_parameters()
    model.train()
    opt = FlatSGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4, arenas=arenas)
    ntx = NTXentLoss(device=DEV, batch_size=2, temperature=0.1, use_cosine_similarity=True, **ntx_kwargs)
    return model, ntx, PretrainStep(model, opt, (0.1, 1.0, 1.0, 1.0, 1.0), clip_grad_norm=True, ntxent=ntx, ntxent_weight=1.0)


def test_step_reports_the_queued_loss():
    """Three steps of the smallest model (depth 1, B = 2: R = 4) with room for two steps' rows: the ``ntxent`` each step reports is
    the specification on that step's projections and on a queue replayed on the host from the earlier steps' projections."""
    ls, sd, x1, x2, lab = _step_fixture()
    model, ntx, step = _build_step(ls, sd, queue_size=8)
    replay, ptr, n_valid = None, 0, 0
    for s in range(3):
        out = step(x1, x2, lab["spa"], lab["tem"], lab["pb"], lab["rot1"], lab["rot2"])
        z1, z2 = [z.detach().cpu() for z in model.last_projections]
        reps = torch.cat([z2, z1], 0)
        if replay is None:
            replay = torch.zeros(8, reps.shape[1])
        want = spec.ref(reps, replay, n_valid, 0.1, torch.float64)["loss"]
        err = abs(float(out.ntxent) - float(want)) / abs(float(want))
        print("NTXQ step", s, float(out.ntxent), float(want), err)
        assert err < spec.BAR
        replay[ptr:ptr + 4] = spec.normalize(reps)
        ptr, n_valid = (ptr + 4) % 8, min(n_valid + 4, 8)
        assert (ntx.ptr, ntx.n_valid) == (ptr, n_valid)
        assert float((ntx.queue.cpu() - replay).abs().max()) <= 2 * 2.0 ** -23      # two fp32 normalisations, 1 ulp each


def test_queue_size_zero_is_the_step_without_the_argument(monkeypatch):
    """Bit for bit over three steps, under the conditions in which two runs of one step are bit-equal at all (deterministic weight
    gradients, BatchNorm statistics by their own pass: tests/test_reg_gpu.py)."""
    from cstp_amd import ops
    monkeypatch.setattr(ops, "FUSE_BN_STATS", False)
    ops.set_deterministic(True)
    try:
        ls, sd, x1, x2, lab = _step_fixture()
        runs = []
        for kwargs in ({}, {"queue_size": 0}):
            model, ntx, step = _build_step(ls, sd, **kwargs)
            outs = [step(x1, x2, lab["spa"], lab["tem"], lab["pb"], lab["rot1"], lab["rot2"]) for _ in range(3)]
            runs.append((model, outs))
            assert not hasattr(ntx, "queue")
        (ma, oa), (mb, ob) = runs
        for a, b in zip(oa, ob):
            assert torch.equal(a.loss_total, b.loss_total) and torch.equal(a.ntxent, b.ntxent)
            assert torch.equal(a.loss_byol, b.loss_byol) and torch.equal(a.grad_norm, b.grad_norm)
            assert all(torch.equal(u, v) for u, v in zip(a.logits, b.logits))
        assert all(torch.equal(v, w) for v, w in zip(ma.state_dict().values(), mb.state_dict().values()))
    finally:
        ops.set_deterministic(False)

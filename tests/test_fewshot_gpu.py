"""Few-shot episodes on the GPU: ops.fewshot_episodes (csrc/fewshot.h) against the fp64 specification of tests/fewshot_spec.py,
its internal consistency and determinism in bits, independence of an episode from the episodes and shot counts around it, zero
prototypes, duplicate indices, the call between poisoned guard bands, fewshot.evaluate_features end to end and the fewshot.py
driver in a child process.

THE BAR is tol = 2 (2 d + Kmax + 8) 2^-24 on a score (fewshot_spec.tol): the worst-case fp32 bound for forming the prototype, a
length-d dot product, a length-d norm and one divide where the exact score is at most 1 in magnitude.  Predictions are compared
with the specification's wherever the fp64 margin between the two best slots exceeds 2 tol; tests/test_fewshot_host.py bounds the
share of decisions this leaves out at 1 % per case.  Every case prints its worst score error beside the bar."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fewshot_spec as spec
import guard_bands as gb

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _call(xs, xq, sup, qry, n_query, shots, **kw):
    """Host numpy / torch operands -> the op's answer; the tables go in as CPU tensors (range-checked, then uploaded)."""
    from cstp_amd import ops
    t = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))      # noqa: E731
    return ops.fewshot_episodes(t(xs).to(DEV), t(xq).to(DEV), t(sup), t(qry), n_query, tuple(shots), **kw)


def _own_slots(n, q):
    return (torch.arange(n * q) // q).to(torch.int32)


def _check_consistency(hits, pred, score, n, q):
    """(b): pred is exactly the lowest-slot argmax of the kernel's own score, hits exactly the count from pred."""
    score, pred, hits = score.cpu(), pred.cpu(), hits.cpu()
    best = score.max(dim=3, keepdim=True).values
    first = (score == best).to(torch.int32).argmax(dim=3).to(torch.int32)                      # the first of equal maxima
    assert torch.equal(pred, first), "pred is not the lowest-slot argmax of score"
    assert torch.equal(hits, (pred == _own_slots(n, q)).sum(dim=2).to(torch.int32)), "hits is not the count from pred"


@pytest.mark.parametrize("case", spec.CASES, ids=str)
def test_case_against_the_specification(case):
    d, n, shots, q, e = case
    xs, xq, sup, qry, (s_ref, p_ref, h_ref, margin) = spec.case_data(*case)
    tol = spec.tol(d, shots[-1])
    hits, pred, score = _call(xs, xq, sup, qry, q, shots, want_pred=True, want_score=True)
    assert hits.dtype == torch.int32 and tuple(hits.shape) == (len(shots), e)
    assert pred.dtype == torch.int32 and tuple(pred.shape) == (len(shots), e, n * q)
    assert score.dtype == torch.float32 and tuple(score.shape) == (len(shots), e, n * q, n)
    # (a) the scores
    err = float((score.cpu().double() - torch.from_numpy(s_ref)).abs().max())
    print("fewshot %s: worst score error %.3e (bar %.3e)" % (case, err, tol))
    assert err <= tol
    # (b) the kernel's own consistency, with and without the optional outputs
    _check_consistency(hits, pred, score, n, q)
    assert _bits(hits, _call(xs, xq, sup, qry, q, shots))
    h2, p2 = _call(xs, xq, sup, qry, q, shots, want_pred=True)
    assert _bits(hits, h2) and _bits(pred, p2)
    # (c) the decisions, outside the band in which fp32 may flip them
    if d >= 16:
        sure = torch.from_numpy(margin > 2.0 * tol)
        assert float(sure.double().mean()) >= 0.99
        assert torch.equal(pred.cpu()[sure], torch.from_numpy(p_ref)[sure])
        unsure = (~sure).sum(dim=2).to(torch.int32)
        assert bool(((hits.cpu() - torch.from_numpy(h_ref)).abs() <= unsure).all())
    # (d) two calls give equal bits
    h3, p3, s3 = _call(xs, xq, sup, qry, q, shots, want_pred=True, want_score=True)
    assert _bits(hits, h3) and _bits(pred, p3) and _bits(score, s3)
    # (e) an episode alone has the bits it has inside the call ...
    for i in sorted({0, e // 2, e - 1}):
        h1, p1, s1 = _call(xs, xq, sup[i:i + 1], qry[i:i + 1], q, shots, want_pred=True, want_score=True)
        assert _bits(h1, hits[:, i:i + 1]) and _bits(p1, pred[:, i:i + 1]) and _bits(s1, score[:, i:i + 1]), "episode %d" % i
    # ... and so has a shot count alone
    if len(shots) > 1:
        for s, k in enumerate(shots):
            h1, p1, s1 = _call(xs, xq, sup[:, :, :k], qry, q, (k,), want_pred=True, want_score=True)
            assert _bits(h1, hits[s:s + 1]) and _bits(p1, pred[s:s + 1]) and _bits(s1, score[s:s + 1]), "shot count %d" % k


def test_more_episodes_than_one_grid_row():
    """70 000 episodes (a block each): 700 distinct ones, tiled, so that the reference stays small -- every copy of an episode
    must carry the bits of the first."""
    d, n, shots, q, e = spec.GRID_CASE
    xs, xq, sup, qry, (s_ref, p_ref, h_ref, margin) = spec.case_data(d, n, shots, q, spec.GRID_DISTINCT)
    reps = e // spec.GRID_DISTINCT
    hits, pred, score = _call(xs, xq, np.tile(sup, (reps, 1, 1)), np.tile(qry, (reps, 1, 1)), q, shots, want_pred=True,
                              want_score=True)
    tol = spec.tol(d, shots[-1])
    assert float((score[:, :spec.GRID_DISTINCT].cpu().double() - torch.from_numpy(s_ref)).abs().max()) <= tol
    _check_consistency(hits, pred, score, n, q)
    first = lambda t: t[:, :spec.GRID_DISTINCT].repeat(1, reps, *([1] * (t.dim() - 2)))        # noqa: E731
    assert _bits(hits, first(hits)) and _bits(pred, first(pred)) and _bits(score, first(score))
    sure = torch.from_numpy(margin > 2.0 * tol)
    assert torch.equal(pred[:, :spec.GRID_DISTINCT].cpu()[sure], torch.from_numpy(p_ref)[sure])
    assert _bits(hits, _call(xs, xq, np.tile(sup, (reps, 1, 1)), np.tile(qry, (reps, 1, 1)), q, shots))


def test_zero_prototypes_score_zero_and_slot_zero_wins():
    """(f): a class whose support rows are all zero scores 0 against every query; with every prototype zero all scores are 0 and
    slot 0 is the answer everywhere."""
    d, n, shots, q, e = 130, 3, (1, 4), 5, 4
    xs, xq, sup, qry, _ = spec.case_data(d, n, shots, q, e)
    xs = xs.copy()
    xs[sup[1, 2]] = 0.0                                                   # episode 1, slot 2 (other episodes may share the rows)
    s_ref, p_ref, h_ref, margin = spec.episodes_ref(xs, xq, sup, qry, shots)
    hits, pred, score = _call(xs, xq, sup, qry, q, shots, want_pred=True, want_score=True)
    assert bool((score[:, 1, :, 2] == 0).all())
    assert float((score.cpu().double() - torch.from_numpy(s_ref)).abs().max()) <= spec.tol(d, 4)
    _check_consistency(hits, pred, score, n, q)
    hits, pred, score = _call(np.zeros_like(xs), xq, sup, qry, q, shots, want_pred=True, want_score=True)
    assert bool((score == 0).all()) and bool((pred == 0).all()) and bool((hits == q).all())


def test_duplicate_indices_are_accepted():
    """(g): the same support row several times in a class (it counts as often), one row in two classes, one query in every slot."""
    d, n, shots, q, e = 40, 4, (2, 3), 3, 5
    xs, xq, sup, qry, _ = spec.case_data(d, n, shots, q, e)
    sup, qry = sup.copy(), qry.copy()
    sup[0, 1, :] = sup[0, 1, 0]
    sup[1, 2, :] = sup[1, 0, :]
    qry[2, :, :] = qry[2, 0, 0]
    sup[3] = 7
    qry[4] = 11
    s_ref, p_ref, h_ref, margin = spec.episodes_ref(xs, xq, sup, qry, shots)
    hits, pred, score = _call(xs, xq, sup, qry, q, shots, want_pred=True, want_score=True)
    tol = spec.tol(d, 3)
    assert float((score.cpu().double() - torch.from_numpy(s_ref)).abs().max()) <= tol
    _check_consistency(hits, pred, score, n, q)
    # identical prototypes tie bit for bit and the lowest slot takes the tie
    assert _bits(score[:, 1, :, 0], score[:, 1, :, 2]) and not bool((pred[:, 1] == 2).any())
    assert bool((pred[:, 3] == 0).all()) and bool((hits[:, 3] == q).all())
    sure = torch.from_numpy(margin > 2.0 * tol)
    assert torch.equal(pred.cpu()[sure], torch.from_numpy(p_ref)[sure])


def test_device_tables_and_misaligned_features():
    """Tables already on the device are taken as they are; features one element off a 16-byte boundary with an odd d give the bits
    of aligned ones (the rows are read by 4-byte loads)."""
    from cstp_amd import ops
    case = (257, 20, (16,), 16, 20)
    d, n, shots, q, e = case
    xs, xq, sup, qry, _ = spec.case_data(*case)
    base = _call(xs, xq, sup, qry, q, shots, want_pred=True, want_score=True)
    flat_s = torch.empty(xs.size + 1, dtype=torch.float32, device=DEV)
    flat_q = torch.empty(xq.size + 1, dtype=torch.float32, device=DEV)
    off_s, off_q = flat_s[1:].view(xs.shape), flat_q[1:].view(xq.shape)
    off_s.copy_(torch.from_numpy(xs))
    off_q.copy_(torch.from_numpy(xq))
    assert off_s.data_ptr() % 16 == 4
    got = ops.fewshot_episodes(off_s, off_q, torch.from_numpy(sup).to(DEV), torch.from_numpy(qry).to(DEV), q, shots, want_pred=True,
                               want_score=True)
    assert all(_bits(a, b) for a, b in zip(base, got))


# ---- guard bands ----------------------------------------------------------------------------------------------------------------
def _guarded_spec(case, shift, full):
    from cstp_amd import _lib
    lib = _lib.load()
    d, n, shots, q, e = case
    xs, xq, sup, qry, (s_ref, p_ref, h_ref, margin) = spec.case_data(*case)
    tol = spec.tol(d, shots[-1])
    sure = torch.from_numpy(margin > 2.0 * tol)
    unsure = (~sure).sum(dim=2).to(torch.int32)

    def check_score(got):
        err = float((got.double() - torch.from_numpy(s_ref)).abs().max())
        assert err <= tol, "worst score error %.3e (bar %.3e)" % (err, tol)

    def check_pred(got):
        assert bool(((got >= 0) & (got < n)).all()), "a prediction outside the class slots"
        assert torch.equal(got[sure], torch.from_numpy(p_ref)[sure]), "predictions differ outside the 2 tol band"

    def check_hits(got):
        assert bool((got >= 0).all()), "a negative count"
        assert bool(((got - torch.from_numpy(h_ref)).abs() <= unsure).all()), "hits differ by more than the decisions in the band"
    s_n = len(shots)
    outputs = {"hits": ((s_n, e), torch.int32)}
    checks = {"hits": check_hits}
    if full:
        outputs.update(pred=((s_n, e, n * q), torch.int32), score=((s_n, e, n * q, n), torch.float32))
        checks.update(pred=check_pred, score=check_score)
    s = gb.Spec("fewshot_episodes %s shift %d %s" % (case, shift, "full" if full else "hits only"),
                {"xs": torch.from_numpy(xs), "xq": torch.from_numpy(xq), "sup_idx": torch.from_numpy(sup), "qry_idx": torch.from_numpy(qry)},
                outputs, checks, ws_bytes=0, shifts={"xs": shift, "xq": shift, "sup_idx": shift, "qry_idx": shift},
                finite_as={"hits": None, "pred": None})
    stream = torch.cuda.current_stream().cuda_stream
    ks = (ctypes.c_int32 * s_n)(*shots)

    def impl(v, n_way=n, d_arg=d):
        return lib.cstp_fewshot_episodes(stream, v["xs"].data_ptr(), xs.shape[0], v["xq"].data_ptr(), xq.shape[0], d_arg,
                                         v["sup_idx"].data_ptr(), v["qry_idx"].data_ptr(), e, n_way, q, ks, s_n, v["hits"].data_ptr(),
                                         v["pred"].data_ptr() if full else None, v["score"].data_ptr() if full else None)
    return s, impl


def _checked(impl):
    from cstp_amd import _lib

    def run(v):
        _lib.check(impl(v), "the guarded call")
    return run


@pytest.mark.parametrize("full", [True, False], ids=["with pred and score", "hits only"])
@pytest.mark.parametrize("shift", [0, 4], ids=["aligned", "one element off"])
@pytest.mark.parametrize("case", [(255, 5, (1, 5), 15, 40), (257, 20, (16,), 16, 20)], ids=str)
def test_between_poisoned_guard_bands(case, shift, full):
    """(h): outputs fully written (their interior starts as 0xFF bytes: NaN scores, -1 integers, which the checks refuse), nothing
    outside them changed -- there is no workspace --, the inputs unchanged, the answer independent of what surrounds the operands."""
    s, impl = _guarded_spec(case, shift, full)
    found = gb.three_runs(s, _checked(impl), DEV, torch.cuda.synchronize)
    assert found == [], "\n".join(found)


def test_refused_calls_touch_nothing():
    s, impl = _guarded_spec((255, 5, (1, 5), 15, 40), 0, True)
    operands = gb.Operands(s, DEV)
    for kw in (dict(n_way=1), dict(n_way=21), dict(d_arg=0), dict(d_arg=8193)):
        operands.arm("nan")
        rc = impl(operands.views(), **kw)
        torch.cuda.synchronize()
        assert rc != 0, kw
        assert operands.problems() == [], kw
        for g in operands.outs.values():
            assert bool((g.buf[g.lo:g.hi] == 0xFF).all()), "%s was written by a refused call (%r)" % (g.name, kw)


# ---- the module and the driver --------------------------------------------------------------------------------------------------
def test_evaluate_features_agrees_with_the_specification():
    """(i): the accuracy of evaluate_features against the specification on the same episodes (the sampler is deterministic) and
    the rows ops.l2_normalize gives, to within the decisions that lie in the 2 tol band."""
    from cstp_amd import fewshot, ops
    d, n, shots, q, e = 255, 5, (1, 5), 15, 200
    xs, ls = spec.make_features(d, seed=d, part=0)
    xq, lq = spec.make_features(d, seed=d, part=1)
    s_feat, q_feat = torch.from_numpy(xs * 3.0).to(DEV), torch.from_numpy(xq * 0.5).to(DEV)         # not unit: it normalises
    res = fewshot.evaluate_features(s_feat, torch.from_numpy(ls), q_feat, torch.from_numpy(lq).to(DEV), n, shots, q, e, seed=5)
    assert (res["n_way"], res["shots"], res["n_query"], res["episodes"], res["seed"]) == (n, [1, 5], q, e, 5)
    assert (res["n_support"], res["n_queries"], res["feature_dim"]) == (960, 960, d)
    sup, qry, classes = fewshot.sample_episodes(ls, lq, n, 5, q, e, seed=5)
    _, _, h_ref, margin = spec.episodes_ref(ops.l2_normalize(s_feat).cpu().numpy(), ops.l2_normalize(q_feat).cpu().numpy(),
                                            sup.numpy(), qry.numpy(), shots)
    tol = spec.tol(d, 5)
    for s, k in enumerate(shots):
        want = float((h_ref[s] / float(n * q)).mean())
        slack = float((margin[s] <= 2.0 * tol).sum()) / (e * n * q)
        print("evaluate_features %d-shot: acc %.6f, spec %.6f (slack %.2e), ci95 %.4f" % (k, res["acc"][k], want, slack, res["ci95"][k]))
        assert abs(res["acc"][k] - want) <= slack + 1e-12
        assert 0.0 < res["ci95"][k] < 0.05
    assert res["acc"][5] > res["acc"][1] > 1.0 / n                          # more shots help on these features


def _run(args, timeout, **extra_env):
    env = dict(os.environ, **extra_env)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args[0], r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_fewshot_driver_on_a_fresh_checkpoint(tmp_path):
    """(j): fewshot.py in a child process on a checkpoint written from an untrained depth-1 R(2+1)D and 8 + 4 synthetic videos of
    two classes: one line per shot count, the JSON line, the result file; the options dump does not name the flags not given."""
    from cstp_amd.r21d_byol import R21DBYOL
    torch.manual_seed(0)
    model = R21DBYOL(pretrain=True, layer_sizes=(1, 1, 1, 1))
    ckpt = str(tmp_path / "fresh.pth")
    torch.save({"epoch": 1, "arch": "r21d_byol-1", "state_dict": {"module." + k: v for k, v in model.state_dict().items()}}, ckpt)
    res = str(tmp_path / "res")
    out = _run(["fewshot.py", "--dataset", "synthetic_video", "--transform_mode", "img_test", "--model_name", "r21d_byol",
                "--model_depth", "1", "--pretrained_path", ckpt, "--result_path", res, "--sample_duration", "4", "--pb_rate", "2",
                "--sample_size", "112", "--n_classes", "2", "--synthetic_len", "16", "--retrieval_gallery_len", "8",
                "--fewshot_way", "2", "--fewshot_shot", "1", "3", "--fewshot_query", "2", "--fewshot_episodes", "30"], 120)
    lines = out.split("\n")
    summary = json.loads([ln for ln in lines if ln.startswith("{")][-1])
    assert summary["task"] == "fewshot" and summary["arch"] == "r21d_byol-1"
    assert (summary["n_way"], summary["shots"], summary["n_query"], summary["episodes"], summary["seed"]) == (2, [1, 3], 2, 30, 0)
    assert (summary["n_support"], summary["n_queries"], summary["feature_dim"]) == (8, 4, 512)
    for k in ("1", "3"):
        acc, ci = summary["acc"][k], summary["ci95"][k]
        assert 0.0 <= acc <= 1.0 and 0.0 <= ci < 1.0
        assert "Few-shot 2-way %s-shot: %.4f ± %.4f (30 episodes)" % (k, acc, ci) in lines
    assert "fewshot_way=2" in out and "fewshot_seed" not in out
    saved = open(os.path.join(res, "synthetic_video", "fewshot_r21d_byol1_synthetic_video_1_4.txt")).read().split("\n")
    assert json.loads([ln for ln in saved if ln.startswith("{")][-1]) == summary

"""Weighted k-NN classification on the GPU: ops.knn_vote (csrc/retrieve.hip) against the fp64 specification of
tests/knn_spec.py, its tie order, dead and out-of-range slots behind canaries, determinism; knn.classify and knn.evaluate end to
end; the --knn_every monitor of main_byol.py and the knn.py driver chain in child processes."""
import csv
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from knn_spec import MAX_NEAR_TIE_SHARE, RTOL, vote_ref
from test_frame_folder_host import VIDEOS, write_tree

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = float("-inf")

# (nq, ng, d, classes, k, T, seed): the kernel runs one wave per query, four waves per block, lane j = slot j
CASES = [(70, 300, 24, 10, 20, 0.07, 0),        # nq not a multiple of the waves per block
         (70, 300, 24, 10, 64, 0.07, 1),        # every lane live
         (70, 300, 24, 10, 1, 0.07, 2),         # one slot, ranks 2..5 empty
         (70, 300, 24, 10, 5, 1.0, 3),          # flat weights
         (5, 3, 8, 4, 20, 0.07, 4),             # ng < k: dead slots in every row
         (130, 1000, 512, 101, 20, 0.07, 5)]    # more classes than slots


def _inv_t(t):
    return float(np.float32(1.0 / t))           # what the kernel is handed: the fp32 rounding of 1 / T


def _unit(n, d, gen):
    x = torch.randn((n, d), generator=gen)
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


def _cpu_topk(q, g, k):
    """torch.topk on the CPU, padded with (-inf, -1) to k columns: the layout sim_topk writes, made without it."""
    s = q @ g.T
    v, i = torch.topk(s, min(k, g.shape[0]), dim=1)
    val = torch.full((q.shape[0], k), NEG)
    idx = torch.full((q.shape[0], k), -1, dtype=torch.int32)
    val[:, :v.shape[1]], idx[:, :v.shape[1]] = v, i.to(torch.int32)
    return val, idx


def _check_against_spec(pred, score, val, idx, labels, t, n_top, what):
    """The rule of the spec test: (-1, 0) exactly where the spec has it; where no near tie is marked, the spec's class and its
    score within RTOL; near ties are left out and may be at most MAX_NEAR_TIE_SHARE of the (query, rank) pairs."""
    assert pred.dtype == torch.int32 and score.dtype == torch.float32 and pred.is_cuda and score.is_cuda
    assert tuple(pred.shape) == tuple(score.shape) == (val.shape[0], n_top)
    pred, score = pred.cpu().numpy().astype(np.int64), score.cpu().numpy().astype(np.float64)
    rp, rs, near = vote_ref(val.cpu().numpy(), idx.cpu().numpy(), labels.cpu().numpy(), _inv_t(t), n_top)
    share = float(near.mean())
    keep = ~near
    err = np.abs(score - rs)[keep] / np.maximum(rs[keep], 1e-300)
    print("%s: near ties %.2f %% of %d pairs, max relative score error %.3g" % (what, 100 * share, near.size,
                                                                                  err.max() if err.size else 0.0))
    assert share <= MAX_NEAR_TIE_SHARE
    empty = rp < 0
    assert ((pred < 0) == empty).all() and (pred[empty] == -1).all() and (score[empty] == 0.0).all()
    assert (pred[keep] == rp[keep]).all()
    np.testing.assert_allclose(score[keep], rs[keep], rtol=RTOL, atol=0)
    return rp


@pytest.mark.parametrize("nq,ng,d,classes,k,t,seed", CASES, ids=["-".join(map(str, c[:5])) + "-s%d" % c[6] for c in CASES])
def test_vote_meets_the_spec(nq, ng, d, classes, k, t, seed):
    from cstp_amd import ops
    gen = torch.Generator().manual_seed(seed)
    q, g = _unit(nq, d, gen), _unit(ng, d, gen)
    labels = torch.randint(0, classes, (ng,), generator=gen)
    val, idx = _cpu_topk(q, g, k)
    for lab in (labels, labels.to(torch.int32)):                                  # int64 and int32 labels: the same answer
        pred, score = ops.knn_vote(val.cuda(), idx.cuda(), lab.cuda(), t, 5)
        _check_against_spec(pred, score, val, idx, labels, t, 5, "vote %dx%d k=%d" % (nq, ng, k))
    if k == 1:
        assert bool((pred[:, 1:] == -1).all()) and bool((score[:, 0] == 1.0).all())
    for n_top in (1, 8):
        p2, s2 = ops.knn_vote(val.cuda(), idx.cuda(), labels.cuda(), t, n_top)
        m = min(n_top, 5)
        assert torch.equal(p2[:, :m], pred[:, :m]) and torch.equal(s2[:, :m], score[:, :m])     # ranks do not depend on n_top


def test_exact_ties_go_to_the_lower_class():
    from cstp_amd import ops
    gen = torch.Generator().manual_seed(11)
    nq, pairs, d = 9, 6, 16
    base = _unit(pairs, d, gen)
    g = base.repeat_interleave(2, dim=0).contiguous()                             # rows 2p and 2p + 1 are the same vector
    labels = torch.tensor([7, 3] * pairs)
    q = (base[torch.arange(nq) % pairs] + 0.05 * torch.randn((nq, d), generator=gen)).contiguous()
    s = q @ g.T
    s[:, 1::2] = s[:, 0::2]                                                       # ... and their similarities the same bits
    v, i = torch.topk(s, 2, dim=1)
    assert bool((v[:, 0] == v[:, 1]).all()) and bool((i.min(dim=1).values // 2 == i.max(dim=1).values // 2).all())
    pred, score = ops.knn_vote(v.contiguous().cuda(), i.to(torch.int32).contiguous().cuda(), labels.cuda(), 0.07, 5)
    pred, score = pred.cpu(), score.cpu()
    assert pred[:, :2].tolist() == [[3, 7]] * nq and bool((pred[:, 2:] == -1).all())
    assert torch.equal(score[:, 0].view(torch.int32), score[:, 1].view(torch.int32)) and bool((score[:, 0] == 1.0).all())
    # two slots per class, interleaved: class 3 sums slots (1, 3), class 7 slots (0, 2) -- bit-equal weights, bit-equal sums
    val = torch.tensor([[0.9, 0.9, 0.8, 0.8]]).repeat(nq, 1).contiguous()
    idx = torch.tensor([[0, 1, 2, 3]], dtype=torch.int32).repeat(nq, 1).contiguous()
    pred, score = ops.knn_vote(val.cuda(), idx.cuda(), labels.cuda(), 0.07, 2)
    assert pred.cpu().tolist() == [[3, 7]] * nq
    assert torch.equal(score[:, 0].view(torch.int32), score[:, 1].view(torch.int32))


def test_dead_and_out_of_range_slots_behind_canaries():
    """The C entry point on buffers with guard regions: an all-dead row gives all (-1, 0), a slot whose idx is >= ng (or < -1)
    is dead and forms no address, and nothing outside pred / score is written, the labels included."""
    from cstp_amd import _lib, ops
    lib = _lib.load()
    nq, ng, k, n_top, pad = 6, 10, 4, 5, 512
    labels = torch.tensor([0, 1, 2, 3, 4, 0, 1, 2, 3, 4], dtype=torch.int32)
    val = torch.tensor([[NEG] * 4,                                # all dead
                        [0.9, 0.8, 0.7, 0.6],
                        [0.9, 0.8, 0.7, 0.6],                     # as the row above with slot 1 out of range
                        [0.9, 0.8, 0.7, 0.6],                     # ... with slot 0 out of range: val_0 still anchors the weights
                        [0.9, 0.8, NEG, NEG],
                        [0.9, 0.8, 0.7, 0.6]])
    idx = torch.tensor([[-1, -1, -1, -1],
                        [0, 5, 1, 2],
                        [0, ng, 1, 2],
                        [2 ** 31 - 1, 5, 1, 2],
                        [9, 4, -1, -1],
                        [-2 ** 31, -7, ng + 1000, 3]], dtype=torch.int32)
    lab_buf = torch.full((pad + ng + pad,), 0x5A5A5A, dtype=torch.int32)
    lab_buf[pad:pad + ng] = labels
    lab_dev = lab_buf.cuda()
    pred_dev = torch.full((pad + nq * n_top + pad,), -77, dtype=torch.int32, device="cuda")
    score_dev = torch.full((pad + nq * n_top + pad,), -77.0, dtype=torch.float32, device="cuda")
    vd, idd = val.cuda(), idx.cuda()
    rc = lib.cstp_knn_vote(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), vd.data_ptr(), idd.data_ptr(),
                           lab_dev.data_ptr() + 4 * pad, nq, ng, k, _inv_t(0.1), n_top, pred_dev.data_ptr() + 4 * pad,
                           score_dev.data_ptr() + 4 * pad)
    assert rc == 0, lib.cstp_last_error()
    torch.cuda.synchronize()
    assert torch.equal(lab_dev.cpu(), lab_buf)
    pred_all, score_all = pred_dev.cpu(), score_dev.cpu()
    for buf, fill in ((pred_all, -77), (score_all, -77.0)):
        assert bool((buf[:pad] == fill).all()) and bool((buf[pad + nq * n_top:] == fill).all())
    pred = pred_all[pad:pad + nq * n_top].reshape(nq, n_top)
    score = score_all[pad:pad + nq * n_top].reshape(nq, n_top)
    rp, rs, near = vote_ref(val.numpy(), idx.numpy(), labels.numpy(), _inv_t(0.1), n_top)
    assert not near.any()
    assert pred.tolist() == rp.tolist()
    np.testing.assert_allclose(score.numpy().astype(np.float64), rs, rtol=RTOL, atol=0)
    assert pred[0].tolist() == [-1] * 5 and score[0].tolist() == [0.0] * 5
    assert pred[1].tolist() == [0, 1, 2, -1, -1]                  # classes 0 (slots 0, 1), 1, 2
    assert pred[2].tolist() == [0, 1, 2, -1, -1] and float(score[2, 0]) == 1.0        # class 0 lost slot 1
    assert pred[3].tolist() == [0, 1, 2, -1, -1] and float(score[3, 0]) < 1.0         # class 0 is slot 1 alone
    assert pred[4].tolist() == [4, -1, -1, -1, -1]                # rows 9 and 4 are both class 4
    assert pred[5].tolist() == [3, -1, -1, -1, -1]
    # the same through ops.knn_vote
    p2, s2 = ops.knn_vote(vd, idd, labels.cuda(), 0.1, n_top)
    assert torch.equal(p2.cpu(), pred) and torch.equal(s2.cpu(), score)


def test_vote_is_deterministic_and_row_wise():
    from cstp_amd import ops
    gen = torch.Generator().manual_seed(21)
    nq, ng, d, k = 203, 500, 32, 33
    q, g = _unit(nq, d, gen), _unit(ng, d, gen)
    labels = torch.randint(0, 12, (ng,), generator=gen).cuda()
    val, idx = _cpu_topk(q, g, k)
    vd, idd = val.cuda(), idx.cuda()
    p1, s1 = ops.knn_vote(vd, idd, labels, 0.07, 5)
    p2, s2 = ops.knn_vote(vd, idd, labels, 0.07, 5)
    assert torch.equal(p1, p2) and torch.equal(s1.view(torch.int32), s2.view(torch.int32))
    perm = torch.randperm(nq, generator=gen).cuda()
    p3, s3 = ops.knn_vote(vd[perm].contiguous(), idd[perm].contiguous(), labels, 0.07, 5)
    assert torch.equal(p3, p1[perm]) and torch.equal(s3.view(torch.int32), s1[perm].view(torch.int32))
    # non-contiguous inputs are taken as what they hold
    p4, s4 = ops.knn_vote(vd.T.contiguous().T, idd.T.contiguous().T, labels, 0.07, 5)
    assert torch.equal(p4, p1) and torch.equal(s4.view(torch.int32), s1.view(torch.int32))


def test_classify_end_to_end_on_clustered_features():
    from cstp_amd import knn
    gen = torch.Generator().manual_seed(31)
    classes, d, per, nq, k, t = 4, 32, 10, 16, 20, 0.07
    centres = _unit(classes, d, gen)
    g_labels = torch.arange(classes).repeat_interleave(per)
    q_labels = torch.arange(nq) % classes
    g = (3.0 * (centres[g_labels] + 0.02 * torch.randn((classes * per, d), generator=gen))).contiguous()   # not unit norm
    q = (0.5 * (centres[q_labels] + 0.02 * torch.randn((nq, d), generator=gen))).contiguous()
    # the fp64 pipeline on the CPU, and its margin: every query is classified with the runner-up at least 1e-2 (relative) behind
    qn = q.double() / q.double().norm(dim=1, keepdim=True)
    gn = g.double() / g.double().norm(dim=1, keepdim=True)
    rv, ri = torch.topk(qn @ gn.T, k, dim=1)
    rp, rs, _ = vote_ref(rv.numpy(), ri.numpy(), g_labels.numpy(), 1.0 / t, 5)
    assert (rp[:, 0] == q_labels.numpy()).all() and ((rs[:, 0] - rs[:, 1]) > 1e-2 * rs[:, 0]).all()
    pred, score, val, idx = knn.classify(q.cuda(), g.cuda(), g_labels.cuda(), k, t)
    assert tuple(pred.shape) == (nq, 5) and tuple(val.shape) == tuple(idx.shape) == (nq, k)
    assert pred[:, 0].cpu().tolist() == rp[:, 0].tolist()
    acc = knn.accuracy(pred, q_labels.cuda())
    assert acc[1] == 1.0 and acc[5] == 1.0
    assert knn.accuracy(pred.cpu(), q_labels) == acc
    _check_against_spec(pred, score, val, idx, g_labels, t, 5, "classify")
    # leave-one-out on the gallery: no row votes with its own slot, and the vote is the spec's on that list
    gd = g.cuda()
    pred, score, val, idx = knn.classify(gd, gd, g_labels.cuda(), k, t, exclude_self=True)
    assert not bool((idx.cpu() == torch.arange(classes * per).reshape(-1, 1)).any())
    _check_against_spec(pred, score, val, idx, g_labels, t, 5, "leave-one-out")
    assert knn.accuracy(pred, g_labels)[1] == 1.0
    p_in, _, _, idx_in = knn.classify(gd, gd, g_labels.cuda(), k, t)
    assert torch.equal(idx_in[:, 0].cpu().to(torch.int64), torch.arange(classes * per))       # with itself in, it comes first


def test_evaluate_on_synthetic_videos():
    """R(2+1)D depth 1, 24 gallery and 16 query videos of 4 classes, 60 x 80 pixels, clips of 8 x 112 x 112 (the shapes of
    test_retrieval_end_to_end_on_synthetic_videos).  evaluate() reports the accuracy of the vote that the spec gives on the
    extracted features' sim_topk output, and hands the model back in the mode it came in."""
    from cstp_amd import knn, ops, retrieval
    from cstp_amd.clip_ops import GpuLabelledLoader, GpuLabelledVideos
    from cstp_amd.r21d_byol import R21DBYOL
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    kw = dict(n_classes=4, height=60, width=80, sample_duration=8, sample_size=112, pb_rate=2)
    gallery = GpuLabelledLoader(GpuLabelledVideos(dev, "test", "img_test", n_videos=24, seed=2, **kw))
    queries = GpuLabelledLoader(GpuLabelledVideos(dev, "test", "img_test", n_videos=16, seed=1, **kw))
    model = R21DBYOL(pretrain=True, layer_sizes=(1, 1, 1, 1)).cuda()
    model.train()
    before = {n: b.clone() for n, b in model.named_buffers()}
    modes = {n: m.training for n, m in model.named_modules()}
    assert model.training and any(modes.values())
    k, t = 20, 0.07
    res = knn.evaluate(model, gallery, queries, k, t)
    assert model.training and {n: m.training for n, m in model.named_modules()} == modes
    assert all(torch.equal(b, before[n]) for n, b in model.named_buffers())       # eval mode: no running statistic moved
    assert res["n_query"] == 16 and res["n_gallery"] == 24 and res["feature_dim"] == 512 and res["k"] == k
    assert res["temperature"] == t and 0.0 <= res["top1"] <= res["top5"] <= 1.0
    model.eval()
    res2 = knn.evaluate(model, gallery, queries, k, t)
    assert not model.training and not any(m.training for m in model.modules())
    assert res2 == res
    # the same numbers by hand
    gf, gl = retrieval.extract_features(model, gallery)
    qf, ql = retrieval.extract_features(model, queries)
    val, idx = ops.sim_topk(ops.l2_normalize(qf), ops.l2_normalize(gf), k)
    pred, score, val2, idx2 = knn.classify(qf, gf, gl, k, t)
    assert torch.equal(val, val2) and torch.equal(idx, idx2)
    rp = _check_against_spec(pred, score, val, idx, gl, t, 5, "evaluate")
    acc = knn.accuracy(pred, ql)
    assert res["top1"] == acc[1] and res["top5"] == acc[5]
    # against the spec's own predictions the accuracy can differ by the queries with a near tie among their ranks at most
    _, _, near = vote_ref(val.cpu().numpy(), idx.cpu().numpy(), gl.cpu().numpy(), _inv_t(t), 5)
    ref = knn.accuracy(torch.from_numpy(rp), ql.cpu())
    slack = float(near.any(axis=1).sum()) / 16 + 1e-12
    print("kNN top-1 %.4f top-5 %.4f (spec %.4f / %.4f)" % (res["top1"], res["top5"], ref[1], ref[5]))
    assert abs(res["top1"] - ref[1]) <= slack and abs(res["top5"] - ref[5]) <= slack


def _run(args, timeout, **extra_env):
    env = dict(os.environ, **extra_env)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args[0], r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def _log_rows(res, dataset, name):
    with open(os.path.join(res, dataset, "loss_com", name)) as f:
        return list(csv.DictReader(f, delimiter="\t"))


def test_monitor_fills_the_acc_column_and_leaves_training_alone(tmp_path):
    """Two epochs of one step each with --knn_every 1, then with --knn_every 0: a float in [0, 1] in ``acc`` on both rows and
    the kNN lines on stdout against ``None`` / no line, and the same loss columns to the last digit.
    Both runs set CSTP_DETERMINISTIC=1 and CSTP_AUTOTUNE=0, the two documented switches that make a run repeat itself: by default
    the weight gradients are summed with float atomics, and a geometry that the committed tile table lacks (all of these small
    ones) gets the tile that wins a timing in that process.  Measured on an MI355X with this command: without the switches two
    runs with --knn_every 0 already disagree (epoch 2 loss_byol 3.9656996726989746 / 3.9656991958618164), with
    CSTP_DETERMINISTIC=1 alone four such runs gave 4.036653995513916 / 4.036653518676758 in epoch 1 and two values in epoch 2,
    with both switches thirteen runs, seven of them with --knn_every 1, agreed in every column.  Only there can the comparison
    show that the evaluation changes nothing.  Each run is a child process of about five seconds (start-up, one step and one
    evaluation of 8 + 2 short videos per epoch) under a limit of 120."""
    common = ["main_byol.py", "--dataset", "synthetic_video", "--model_name", "r21d_byol", "--model_depth", "1",
              "--sample_duration", "4", "--sample_size", "112", "--batch_size", "2", "--synthetic_len", "8",
              "--retrieval_gallery_len", "8", "--n_classes", "4", "--n_epochs", "2", "--max_steps", "1", "--task", "loss_com",
              "--loss_weight", "0.1", "1", "1", "1", "1", "--learning_rate", "0.005", "--weight_decay", "5e-4"]
    rows, outs = {}, {}
    for every in ("1", "0"):
        res = str(tmp_path / ("res" + every))
        outs[every] = _run(common + ["--result_path", res, "--knn_every", every], 120, CSTP_DETERMINISTIC="1", CSTP_AUTOTUNE="0")
        rows[every] = _log_rows(res, "synthetic_video", "synthetic_video_train_clip4modelr21d_byol1.log")
        assert [r["epoch"] for r in rows[every]] == ["1", "2"]
    for e, r in enumerate(rows["1"], 1):
        assert 0.0 <= float(r["acc"]) <= 1.0
        line = [ln for ln in outs["1"].split("\n") if ln.startswith("Epoch %d: kNN top-1 = " % e)]
        assert len(line) == 1 and float(line[0].split("=")[1]) == pytest.approx(float(r["acc"]), abs=5e-5)
        assert ("Epoch %d: kNN top-5 = " % e) in outs["1"]
    assert "kNN monitor: 8 gallery videos, 2 query videos" in outs["1"]
    assert [r["acc"] for r in rows["0"]] == ["", ""] and "kNN" not in outs["0"]        # csv writes None as the empty field
    cols = [c for c in rows["0"][0] if c != "acc"]
    assert "loss" in cols and "loss_byol" in cols and len(cols) == 8
    for a, b in zip(rows["1"], rows["0"]):
        assert [a[c] for c in cols] == [b[c] for c in cols]


def _check_result(path, out, nq, ng, k, t):
    assert os.path.isfile(path), path
    lines = [ln for ln in open(path).read().split("\n") if ln]
    summary = json.loads(lines[-1])
    assert json.loads([ln for ln in out.split("\n") if ln.startswith("{")][-1]) == summary
    assert set(summary) == {"task", "arch", "dataset", "split", "n_query", "n_gallery", "feature_dim", "k", "temperature",
                            "top1", "top5"}
    assert summary["task"] == "knn" and summary["arch"] == "r21d_byol-1" and summary["split"] == "1"
    assert summary["n_query"] == nq and summary["n_gallery"] == ng and summary["feature_dim"] == 512
    assert summary["k"] == k and summary["temperature"] == t
    assert 0.0 <= summary["top1"] <= summary["top5"] <= 1.0
    for n, key in ((1, "top1"), (5, "top5")):
        want = "kNN top-%d = %.4f" % (n, summary[key])
        assert want in lines and want in out.split("\n")


def test_knn_driver_chain(tmp_path):
    """main_byol.py (R(2+1)D depth 1 on synthetic clips; 100 one-step epochs, because the driver checkpoints every 100), then
    knn.py on that checkpoint: once on synthetic videos, once on a frame-folder tree.  Each a child process with its own time
    limit; a failing child ends the chain."""
    res = str(tmp_path / "res")
    model = ["--model_name", "r21d_byol", "--model_depth", "1", "--result_path", res]
    _run(["main_byol.py", "--dataset", "synthetic", "--sample_duration", "4", "--sample_size", "32", "--n_workers", "0",
          "--batch_size", "2", "--synthetic_len", "2", "--task", "loss_com", "--loss_weight", "0.1", "1", "1", "1", "1",
          "--n_epochs", "100", "--learning_rate", "0.005", "--weight_decay", "5e-4"] + model, 600)
    ckpt = os.path.join(res, "synthetic", "loss_com", "save_100.pth")
    assert os.path.isfile(ckpt)
    common = model + ["--pretrained_path", ckpt, "--transform_mode", "img_test", "--sample_size", "112", "--n_classes", "4"]
    out = _run(["knn.py", "--dataset", "synthetic_video", "--sample_duration", "8", "--pb_rate", "2", "--synthetic_len", "32",
                "--retrieval_gallery_len", "12", "--knn_k", "5", "--knn_t", "0.1"] + common, 300)
    _check_result(os.path.join(res, "synthetic_video", "knn_r21d_byol1_synthetic_video_1_8.txt"), out, 8, 12, 5, 0.1)
    videos = [(e, lab, n, 130, 150, g) for e, lab, n, _, _, g in VIDEOS]
    frame_dir, ann = write_tree(tmp_path / "data", videos)
    out = _run(["knn.py", "--dataset", "UcfFineTune", "--frame_dir", frame_dir, "--annotation_path", ann, "--split", "1",
                "--sample_duration", "4", "--pb_rate", "2", "--n_workers", "4"] + common, 300)      # the default k = 20 > 6 rows
    _check_result(os.path.join(res, "UcfFineTune", "knn_r21d_byol1_UcfFineTune_1_4.txt"), out, 3, 6, 20, 0.07)

"""Linear probe on cached features on the GPU: ops.probe_step and ops.probe_predict (csrc/probe.h) against the fp64 specification
of tests/probe_spec.py on its seven shapes, the first-step identity, bad labels and row indices behind canaries, determinism, the
tie order; probe.fit against the fp64 loop of the same plan (SGD to a tolerance, Adam by its predictions), separable clusters, and
the linear_probe.py driver chain in child processes."""
import ctypes
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from probe_spec import (GRAD_RTOL, LOGIT_TOL_ULPS, LOSS_RTOL, MAX_NEAR_TIE_SHARE, STEP_CASES, ULP, fit_ref, make_case, make_clusters,
                        predict_ref, step_ref)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"

# probe.fit with SGD against the fp64 loop (300 x 24, 10 classes, 5 epochs of batch 64, lr 0.1, momentum 0.9, wd 1e-4): the
# update is linear in the gradient, so rounding does not amplify.  The torch-fp32 restatement of that loop (probe_spec.fit_ref with
# dtype=float32) differed from the fp64 one by 5.7e-8 relative in the per-epoch mean loss, 2.2e-7 of max-abs in W and 1.75e-7 in b;
# the bounds are 4 x those.  probe.fit on an MI355X: 2.1e-8, 1.8e-7 and 3.7e-7.
FIT_LOSS_RTOL, FIT_W_RTOL, FIT_B_RTOL = 2.3e-7, 8.8e-7, 7.0e-7


@functools.lru_cache(maxsize=None)
def _case(i):
    """Case i of STEP_CASES as (numpy dict, device dict): made once, shared, never written."""
    case = make_case(*STEP_CASES[i])
    dev = {k: torch.from_numpy(v).to(DEV) for k, v in case.items() if isinstance(v, np.ndarray)}
    dev["rows"] = dev.get("rows")
    return case, dev


@functools.lru_cache(maxsize=None)
def _step_spec(i, standardised):
    case, _ = _case(i)
    kw = dict(mean=case["mean"], inv_std=case["inv_std"]) if standardised else {}
    return step_ref(case["x"], case["labels"], case["w"], case["b"], case["rows"], **kw)


def _std(dev, standardised):
    return (dev["mean"], dev["inv_std"]) if standardised else (None, None)


def _check_step(out, ref, m, c, d, what):
    loss, hits, dw, db = out
    assert loss.dtype == torch.float32 and hits.dtype == torch.int32 and dw.dtype == db.dtype == torch.float32
    assert all(t.is_cuda for t in out)
    assert tuple(loss.shape) == (1,) and tuple(hits.shape) == (1,) and tuple(dw.shape) == (c, d) and tuple(db.shape) == (c,)
    loss_err = abs(float(loss) - ref["loss"]) / max(abs(ref["loss"]), 1e-300)
    dw_err = np.abs(dw.cpu().numpy().astype(np.float64) - ref["dw"]).max() / max(np.abs(ref["dw"]).max(), 1e-300)
    db_err = np.abs(db.cpu().numpy().astype(np.float64) - ref["db"]).max() / max(np.abs(ref["db"]).max(), 1e-300)
    print("%s: loss rel err %.3g, dW err / max-abs %.3g, db err / max-abs %.3g, hits %d (spec %d, near-tie rows %d)"
          % (what, loss_err, dw_err, db_err, int(hits), ref["hits"], int(ref["near_top1"].sum())))
    assert loss_err <= LOSS_RTOL
    assert dw_err <= GRAD_RTOL and db_err <= GRAD_RTOL
    assert abs(int(hits) - ref["hits"]) <= int(ref["near_top1"].sum())


@pytest.mark.parametrize("standardised", [True, False])
@pytest.mark.parametrize("i", range(len(STEP_CASES)))
def test_step_matches_the_spec(i, standardised):
    from cstp_amd import ops
    m, n, d, c, _ = STEP_CASES[i]
    _, dev = _case(i)
    mean, inv_std = _std(dev, standardised)
    out = ops.probe_step(dev["x"], dev["labels"], dev["w"], dev["b"], dev["rows"], mean, inv_std)
    _check_step(out, _step_spec(i, standardised), m, c, d, "step %s std=%s" % (STEP_CASES[i], standardised))


def test_out_views_receive_the_results():
    from cstp_amd import ops
    m, n, d, c, _ = STEP_CASES[1]
    _, dev = _case(1)
    log = torch.full((3,), -7.0, device=DEV)
    hit = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    dw, db = torch.empty((c, d), device=DEV), torch.empty(c, device=DEV)
    out = ops.probe_step(dev["x"], dev["labels"], dev["w"], dev["b"], dev["rows"], dev["mean"], dev["inv_std"],
                         out=(log[1:2], hit[1:2], dw, db))
    assert out[2] is dw and out[3] is db
    _check_step(out, _step_spec(1, True), m, c, d, "out views")
    assert log[[0, 2]].tolist() == [-7.0, -7.0] and hit[[0, 2]].tolist() == [-7, -7]


def test_first_step_loss_is_ln_c():
    from cstp_amd import ops
    for i in (0, 3, 5):
        m, n, d, c, _ = STEP_CASES[i]
        case, dev = _case(i)
        w0, b0 = torch.zeros_like(dev["w"]), torch.zeros_like(dev["b"])
        loss, hits, dw, db = ops.probe_step(dev["x"], dev["labels"], w0, b0, dev["rows"], dev["mean"], dev["inv_std"])
        assert float(loss) == pytest.approx(math.log(c), rel=4 * ULP)
        y = case["labels"] if case["rows"] is None else case["labels"][case["rows"]]
        want = 1.0 / c - np.bincount(y, minlength=c) / m
        np.testing.assert_allclose(db.cpu().numpy().astype(np.float64), want, rtol=0, atol=GRAD_RTOL * np.abs(want).max())
        assert int(hits) == int((y == 0).sum())                    # all logits equal: the lowest class id is the arg-max


def _guarded(nbytes, guard=4096):
    """A canary-filled byte buffer with ``guard`` bytes after the nbytes the kernel may write -> (buffer, payload view)."""
    buf = torch.full((nbytes + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf, buf[:nbytes]


def test_bad_labels_and_rows_contribute_nothing_and_nothing_is_written_outside():
    """Values, not faults: by contract a label outside [0, c) and a row index outside [0, n) are compared and never dereferenced.
    The C entry point is called directly so that every output and the stated workspace bytes are followed by canaries."""
    from cstp_amd import _lib
    lib = _lib.load()
    m, n, d, c, _ = STEP_CASES[1]
    case, dev = _case(1)
    rows, labels = case["rows"].copy(), case["labels"].copy()
    rows[3], rows[11], rows[69] = -1, n, n + 5
    labels[rows[5]], labels[rows[20]] = -1, c
    ref = step_ref(case["x"], labels, case["w"], case["b"], rows, case["mean"], case["inv_std"])
    rows_d, labels_d = torch.from_numpy(rows).to(DEV), torch.from_numpy(labels).to(DEV)
    ws_bytes = lib.cstp_probe_workspace_bytes(m, d, c)
    assert ws_bytes > 0
    bufs = {k: _guarded(nb) for k, nb in (("loss", 4), ("hits", 4), ("dw", 4 * c * d), ("db", 4 * c), ("ws", ws_bytes))}
    rc = lib.cstp_probe_step(None, dev["x"].data_ptr(), rows_d.data_ptr(), labels_d.data_ptr(), dev["mean"].data_ptr(),
                             dev["inv_std"].data_ptr(), dev["w"].data_ptr(), dev["b"].data_ptr(), m, n, d, c,
                             bufs["loss"][0].data_ptr(), bufs["hits"][0].data_ptr(), bufs["dw"][0].data_ptr(),
                             bufs["db"][0].data_ptr(), bufs["ws"][0].data_ptr(), ws_bytes)
    assert rc == 0, lib.cstp_last_error()
    torch.cuda.synchronize()
    for k, (buf, payload) in bufs.items():
        assert bool((buf[payload.numel():] == 0xA5).all()), k
    out = (bufs["loss"][1].view(torch.float32), bufs["hits"][1].view(torch.int32), bufs["dw"][1].view(torch.float32).view(c, d),
           bufs["db"][1].view(torch.float32))
    _check_step(out, ref, m, c, d, "bad labels and rows")


def test_two_calls_give_equal_bits():
    from cstp_amd import ops
    for i in (3, 5):                                               # rows=None and gathered, the second with two row slices
        _, dev = _case(i)
        a = ops.probe_step(dev["x"], dev["labels"], dev["w"], dev["b"], dev["rows"], dev["mean"], dev["inv_std"])
        a = [t.clone() for t in a]
        b = ops.probe_step(dev["x"], dev["labels"], dev["w"], dev["b"], dev["rows"], dev["mean"], dev["inv_std"])
        assert all(torch.equal(s, t) for s, t in zip(a, b))
        p = [t.clone() for t in ops.probe_predict(dev["x"], dev["w"], dev["b"], dev["mean"], dev["inv_std"])]
        q = ops.probe_predict(dev["x"], dev["w"], dev["b"], dev["mean"], dev["inv_std"])
        assert torch.equal(p[0], q[0]) and torch.equal(p[1], q[1])


@pytest.mark.parametrize("n_top", [1, 5])
@pytest.mark.parametrize("i", range(len(STEP_CASES)))
def test_predict_matches_the_spec(i, n_top):
    from cstp_amd import ops
    m, n, d, c, _ = STEP_CASES[i]
    case, dev = _case(i)
    for standardised in (True, False):
        mean, inv_std = _std(dev, standardised)
        pred, score = ops.probe_predict(dev["x"], dev["w"], dev["b"], mean, inv_std, n_top)
        assert pred.dtype == torch.int32 and score.dtype == torch.float32 and pred.is_cuda and score.is_cuda
        assert tuple(pred.shape) == tuple(score.shape) == (n, n_top)
        kw = dict(mean=case["mean"], inv_std=case["inv_std"]) if standardised else {}
        rc, rs, near, bound = predict_ref(case["x"], case["w"], case["b"], n_top=n_top, **kw)
        pred, score = pred.cpu().numpy().astype(np.int64), score.cpu().numpy().astype(np.float64)
        k = min(n_top, c)
        assert (pred[:, k:] == -1).all() and (score[:, k:] == 0.0).all()
        assert near[:, :k].mean() <= MAX_NEAR_TIE_SHARE
        keep = ~near[:, :k]
        ulps = (np.abs(score - rs)[:, :k] / (ULP * bound[:, None]))[keep]
        print("predict %s std=%s n_top=%d: near ties %.2f %%, max logit error %.2f x 2^-24 B_r"
              % (STEP_CASES[i], standardised, n_top, 100 * near[:, :k].mean(), ulps.max()))
        assert (pred[:, :k][keep] == rc[:, :k][keep]).all()
        assert ulps.max() <= LOGIT_TOL_ULPS


def test_an_exact_tie_goes_to_the_lower_class_id():
    from cstp_amd import ops
    _, dev = _case(0)
    w, b = dev["w"].clone(), dev["b"].clone()
    w[7], b[7] = w[2], b[2]                                        # classes 2 and 7 score the same bits in every row
    w[2] *= 4.0
    w[7] *= 4.0
    pred, score = ops.probe_predict(dev["x"], w, b, dev["mean"], dev["inv_std"], 8)
    pred, score = pred.cpu().numpy(), score.cpu().numpy()
    seen = 0
    for r in range(pred.shape[0]):
        at = np.nonzero(pred[r, :7] == 2)[0]                       # class 2 with a rank behind it in the list
        if at.size:
            seen += 1
            assert pred[r, at[0] + 1] == 7 and score[r, at[0] + 1] == score[r, at[0]]
        assert 7 not in pred[r, :1]
    assert seen > 20
    pred = torch.from_numpy(pred)
    # and in the step: a row whose two best classes tie is a hit only for the lower id
    top = pred[:, 0]
    lab = torch.where(top == 2, torch.full_like(top, 7), top).to(torch.int64).to(DEV)
    _, hits, _, _ = ops.probe_step(dev["x"], lab, w, b, None, dev["mean"], dev["inv_std"])
    assert int(hits) == int((top != 2).sum()) and int((top == 2).sum()) > 0


FIT = dict(epochs=5, batch=64, weight_decay=1e-4, seed=3)


@functools.lru_cache(maxsize=None)
def _soft_clusters():
    feat, lab = make_clusters(300, 24, 10, 2.0)
    return feat, lab, feat.to(DEV), lab.to(DEV)


def _epoch_mean(loss_log, bounds, n):
    sizes = np.array([hi - lo for lo, hi in bounds], dtype=np.float64)
    return (np.asarray(loss_log, dtype=np.float64).reshape(-1, sizes.size) * sizes).sum(axis=1) / n


def test_fit_sgd_matches_the_fp64_loop():
    from cstp_amd import probe
    feat, lab, feat_d, lab_d = _soft_clusters()
    res = probe.fit(feat_d, lab_d, 10, lr=0.1, optimizer="sgd", momentum=0.9, **FIT)
    w, b, loss_log, hit_log, mean, inv_std, bounds = fit_ref(feat, lab, 10, lr=0.1, optimizer="sgd", momentum=0.9, **FIT)
    assert res.batch_bounds == bounds and res.loss_log.numel() == 25 and not res.loss_log.is_cuda
    assert torch.equal(res.mean.cpu(), mean) and torch.equal(res.inv_std.cpu(), inv_std)
    got, want = _epoch_mean(res.loss_log.numpy(), bounds, 300), _epoch_mean(loss_log, bounds, 300)
    loss_err = np.abs(got - want).max() / np.abs(want).max()
    w_err = float((res.w.cpu().double() - w).abs().max() / w.abs().max())
    b_err = float((res.b.cpu().double() - b).abs().max() / b.abs().max())
    print("fit sgd: epoch loss rel err %.3g, W err / max-abs %.3g, b err / max-abs %.3g" % (loss_err, w_err, b_err))
    assert float(res.loss_log[0]) == pytest.approx(math.log(10), rel=4 * ULP)
    assert loss_err <= FIT_LOSS_RTOL and w_err <= FIT_W_RTOL and b_err <= FIT_B_RTOL


def test_fit_adam_learns_and_predicts_as_the_fp64_loop():
    from cstp_amd import probe
    feat, lab, feat_d, lab_d = _soft_clusters()
    res = probe.fit(feat_d, lab_d, 10, lr=0.01, optimizer="adam", **FIT)
    assert bool(torch.isfinite(res.loss_log).all())
    assert _epoch_mean(res.loss_log.numpy(), res.batch_bounds, 300)[-1] < math.log(10)
    assert float(res.loss_log[0]) == pytest.approx(math.log(10), rel=4 * ULP)
    w, b, _, _, mean, inv_std, _ = fit_ref(feat, lab, 10, lr=0.01, optimizer="adam", **FIT)
    rc, _, near, _ = predict_ref(feat.numpy(), w.numpy(), b.numpy(), mean.numpy(), inv_std.numpy(), n_top=1)
    pred, _ = probe.predict(res, feat_d, 1)
    keep = ~near[:, 0]
    assert keep.mean() >= 1 - MAX_NEAR_TIE_SHARE
    assert (pred.cpu().numpy()[:, 0][keep] == rc[:, 0][keep]).all()
    # full batch, rows=None: the same protocol without the gather
    full = probe.fit(feat_d, lab_d, 10, epochs=3, batch=0, lr=0.01)
    assert full.loss_log.numel() == 3 and full.batch_bounds == [(0, 300)]
    assert float(full.loss_log[0]) == pytest.approx(math.log(10), rel=4 * ULP) and float(full.loss_log[2]) < float(full.loss_log[0])


def test_separable_clusters_are_fitted_exactly():
    from cstp_amd import knn, probe
    feat, lab = make_clusters(400, 24, 10, 6.0, seed=1)
    args = dict(epochs=20, batch=64, lr=0.1, optimizer="adam", seed=0)
    res = probe.fit(feat[:300].to(DEV), lab[:300].to(DEV), 10, **args)
    _, train_acc = probe.epoch_means(res, 300)
    assert float(train_acc[-1]) == 1.0
    w, b, _, hit_log, mean, inv_std, _ = fit_ref(feat[:300], lab[:300], 10, **args)
    assert hit_log.reshape(20, -1).sum(axis=1)[-1] == 300
    rc, _, _, _ = predict_ref(feat[300:].numpy(), w.numpy(), b.numpy(), mean.numpy(), inv_std.numpy(), n_top=1)
    pred, _ = probe.predict(res, feat[300:].to(DEV), 5)
    acc = knn.accuracy(pred, lab[300:], (1, 5))
    assert acc[1] == pytest.approx(float((rc[:, 0] == lab[300:].numpy()).mean()), abs=1e-12) and acc[5] >= acc[1] > 0.9


def _run(args, timeout):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args[0], r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_linear_probe_driver_chain(tmp_path):
    """main_byol.py (R(2+1)D depth 1 on synthetic clips; 100 one-step epochs, because the driver checkpoints every 100, as the
    knn.py chain does), then linear_probe.py on that checkpoint with synthetic videos.  Each a child process with its own time
    limit; a failing child ends the chain.  No accuracy is asserted: such an encoder promises none."""
    res = str(tmp_path / "res")
    model = ["--model_name", "r21d_byol", "--model_depth", "1", "--result_path", res]
    _run(["main_byol.py", "--dataset", "synthetic", "--sample_duration", "4", "--sample_size", "32", "--n_workers", "0",
          "--batch_size", "2", "--synthetic_len", "2", "--task", "loss_com", "--loss_weight", "0.1", "1", "1", "1", "1",
          "--n_epochs", "100", "--learning_rate", "0.005", "--weight_decay", "5e-4"] + model, 600)
    ckpt = os.path.join(res, "synthetic", "loss_com", "save_100.pth")
    assert os.path.isfile(ckpt)
    out = _run(["linear_probe.py", "--dataset", "synthetic_video", "--sample_duration", "8", "--pb_rate", "2", "--synthetic_len", "32",
                "--retrieval_gallery_len", "40", "--pretrained_path", ckpt, "--transform_mode", "img_test", "--sample_size", "112",
                "--n_classes", "4", "--n_finetune_classes", "4", "--probe_epochs", "3", "--probe_batch", "16"] + model, 300)
    path = os.path.join(res, "synthetic_video", "probe_r21d_byol1_synthetic_video_1_8.txt")
    assert os.path.isfile(path), path
    lines = [ln for ln in open(path).read().split("\n") if ln]
    summary = json.loads(lines[-1])
    assert json.loads([ln for ln in out.split("\n") if ln.startswith("{")][-1]) == summary
    assert set(summary) == {"task", "arch", "dataset", "split", "top1", "top5", "train_top1", "first_loss", "last_epoch_loss",
                            "n_query", "n_gallery", "feature_dim", "n_classes", "epochs", "batch", "lr", "weight_decay", "optimizer"}
    assert summary["task"] == "linear_probe" and summary["arch"] == "r21d_byol-1"
    assert (summary["n_query"], summary["n_gallery"], summary["feature_dim"], summary["n_classes"]) == (8, 40, 512, 4)
    assert (summary["epochs"], summary["batch"], summary["lr"], summary["weight_decay"], summary["optimizer"]) == (3, 16, 1e-3, 0.0, "adam")
    assert 0.0 <= summary["top1"] <= summary["top5"] <= 1.0 and 0.0 <= summary["train_top1"] <= 1.0
    assert summary["first_loss"] == pytest.approx(math.log(4), rel=1e-6)
    assert summary["last_epoch_loss"] < summary["first_loss"]
    for n, key in ((1, "top1"), (5, "top5")):
        want = "Linear probe top-%d = %.4f" % (n, summary[key])
        assert want in lines and want in out.split("\n")

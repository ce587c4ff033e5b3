"""The linear-probe sweep on the GPU (csrc/probe.h: cstp_probe_sweep_step / _score; cstp_amd.probe.sweep).  The contract is bit
equality with the single-head path, so the comparisons are torch.equal: every head of a sweep call against ops.probe_step on that
head alone (six shapes, with and without standardisation, bad indices included), the calls between poisoned guard bands with the
gradients as slices of one arena, every head of probe.sweep against probe.fit on the train part at that head's learning rate and
weight decay (both optimizers, mini-batches and full batch), then the selection, the refit through probe.evaluate, and the
linear_probe.py driver with a 2 x 1 grid in child processes."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import guard_bands as gb
import probe_sweep_spec as ss
from probe_spec import GRAD_RTOL, LOSS_RTOL, step_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F32, I32 = torch.float32, torch.int32


@functools.lru_cache(maxsize=None)
def _case(i):
    """Case i of SWEEP_CASES -> (numpy dict, device dict with the heads as views of one arena): made once, shared, never written."""
    from cstp_amd import ops
    case = ss.make_sweep_case(*ss.SWEEP_CASES[i])
    dev = {k: torch.from_numpy(v).to(DEV) for k, v in case.items() if isinstance(v, np.ndarray) and k not in ("w", "b")}
    dev["rows"] = dev.get("rows")
    G, c, d = case["w"].shape
    dev["arena"] = torch.from_numpy(ss.arena_of(case["w"], case["b"])).to(DEV)
    dev["w"], dev["b"] = ops.probe_head_views(dev["arena"], G, c, d)
    return case, dev


def _std(dev, standardised):
    return (dev["mean"], dev["inv_std"]) if standardised else (None, None)


@functools.lru_cache(maxsize=None)
def _alone(i, standardised):
    """ops.probe_step on every head of case i by itself (contiguous copies of W_g, b_g) -> [(loss, hits, dw, db)] on the device."""
    from cstp_amd import ops
    case, dev = _case(i)
    mean, inv_std = _std(dev, standardised)
    out = []
    for g in range(case["G"]):
        w, b = dev["w"][g].clone(), dev["b"][g].clone()
        out.append(tuple(t.clone() for t in ops.probe_step(dev["x"], dev["labels"], w, b, dev["rows"], mean, inv_std)))
    return out


def _assert_heads_equal(got, alone, grads=True):
    loss, hits = got[0], got[1]
    G = len(alone)
    assert loss.dtype == F32 and hits.dtype == I32 and tuple(loss.shape) == tuple(hits.shape) == (G,)
    for g, (l1, h1, dw1, db1) in enumerate(alone):
        assert torch.equal(loss[g:g + 1], l1) and torch.equal(hits[g:g + 1], h1), (g, float(loss[g]), float(l1), int(hits[g]), int(h1))
        if grads:
            assert torch.equal(got[2][g], dw1), "dW of head %d" % g
            assert torch.equal(got[3][g], db1), "db of head %d" % g


@pytest.mark.parametrize("standardised", [True, False])
@pytest.mark.parametrize("i", range(len(ss.SWEEP_CASES)))
def test_every_head_has_the_bits_of_the_single_head_call(i, standardised):
    from cstp_amd import ops
    G, m, n, d, c, _ = ss.SWEEP_CASES[i]
    case, dev = _case(i)
    mean, inv_std = _std(dev, standardised)
    alone = _alone(i, standardised)
    got = ops.probe_sweep_step(dev["x"], dev["labels"], dev["w"], dev["b"], dev["rows"], mean, inv_std)
    assert tuple(got[2].shape) == (G, c, d) and tuple(got[3].shape) == (G, c)
    assert G == 1 or got[2].stride(0) == got[3].stride(0) == ss.head_stride(c, d)
    _assert_heads_equal(got, alone)
    score = ops.probe_sweep_score(dev["x"], dev["labels"], dev["w"], dev["b"], dev["rows"], mean, inv_std)
    assert len(score) == 2
    _assert_heads_equal(score, alone, grads=False)
    # head 0 against the fp64 specification, at probe_spec's tolerances and near-tie rule
    kw = dict(mean=case["mean"], inv_std=case["inv_std"]) if standardised else {}
    ref = step_ref(case["x"], case["labels"], case["w"][0], case["b"][0], case["rows"], **kw)
    loss_err = abs(float(got[0][0]) - ref["loss"]) / abs(ref["loss"])
    dw_err = np.abs(got[2][0].cpu().numpy().astype(np.float64) - ref["dw"]).max() / np.abs(ref["dw"]).max()
    db_err = np.abs(got[3][0].cpu().numpy().astype(np.float64) - ref["db"]).max() / np.abs(ref["db"]).max()
    print("sweep %s std=%s head 0: loss rel err %.3g, dW %.3g, db %.3g of max-abs" % (ss.SWEEP_CASES[i], standardised, loss_err, dw_err, db_err))
    assert loss_err <= LOSS_RTOL and dw_err <= GRAD_RTOL and db_err <= GRAD_RTOL
    assert abs(int(got[1][0]) - ref["hits"]) <= int(ref["near_top1"].sum())
    assert abs(int(score[1][0]) - ref["hits"]) <= int(ref["near_top1"].sum())


def test_out_views_receive_the_results_and_the_padding_is_left_alone():
    from cstp_amd import ops
    G, m, n, d, c, _ = ss.SWEEP_CASES[1]
    _, dev = _case(1)
    log = torch.full((3, G), -7.0, device=DEV)
    hit = torch.full((3, G), -7, dtype=I32, device=DEV)
    grads = torch.full((G * ss.head_stride(c, d),), 0.25, device=DEV)
    dw, db = ops.probe_head_views(grads, G, c, d)
    out = ops.probe_sweep_step(dev["x"], dev["labels"], dev["w"], dev["b"], dev["rows"], dev["mean"], dev["inv_std"],
                               out=(log[1], hit[1], dw, db))
    assert out[2] is dw and out[3] is db
    _assert_heads_equal(out, _alone(1, True))
    assert bool((log[[0, 2]] == -7.0).all()) and bool((hit[[0, 2]] == -7).all())
    own = torch.from_numpy(ss.owned_mask(G, c, d)).to(DEV)
    assert int((~own).sum()) > 0 and bool((grads[~own] == 0.25).all())
    ops.probe_sweep_score(dev["x"], dev["labels"], dev["w"], dev["b"], dev["rows"], dev["mean"], dev["inv_std"], out=(log[2], hit[2]))
    assert torch.equal(log[2], log[1]) and torch.equal(hit[2], hit[1]) and bool((log[0] == -7.0).all())


def test_indices_outside_their_range_contribute_zeros_to_every_head():
    """Values, not faults: by contract a row index outside [0, n) and a label outside [0, c) are compared, never dereferenced."""
    from cstp_amd import ops
    G, m, n, d, c, _ = ss.SWEEP_CASES[1]
    case, dev = _case(1)
    rows, labels = case["rows"].copy(), case["labels"].copy()
    rows[3], rows[11] = -1, n
    labels[rows[5]] = c
    rows_d, labels_d = torch.from_numpy(rows).to(DEV), torch.from_numpy(labels).to(DEV)
    alone = []
    for g in range(G):
        w, b = dev["w"][g].clone(), dev["b"][g].clone()
        alone.append(tuple(t.clone() for t in ops.probe_step(dev["x"], labels_d, w, b, rows_d, dev["mean"], dev["inv_std"])))
    first = [t.clone() for t in ops.probe_sweep_step(dev["x"], labels_d, dev["w"], dev["b"], rows_d, dev["mean"], dev["inv_std"])]
    _assert_heads_equal(first, alone)
    second = ops.probe_sweep_step(dev["x"], labels_d, dev["w"], dev["b"], rows_d, dev["mean"], dev["inv_std"])
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    s1 = [t.clone() for t in ops.probe_sweep_score(dev["x"], labels_d, dev["w"], dev["b"], rows_d, dev["mean"], dev["inv_std"])]
    _assert_heads_equal(s1, alone, grads=False)
    s2 = ops.probe_sweep_score(dev["x"], labels_d, dev["w"], dev["b"], rows_d, dev["mean"], dev["inv_std"])
    assert torch.equal(s1[0], s2[0]) and torch.equal(s1[1], s2[1])
    ref = step_ref(case["x"], labels, case["w"][0], case["b"][0], rows, case["mean"], case["inv_std"])
    assert abs(float(first[0][0]) - ref["loss"]) <= LOSS_RTOL * abs(ref["loss"])
    good = step_ref(case["x"], case["labels"], case["w"][0], case["b"][0], case["rows"], case["mean"], case["inv_std"])
    assert ref["loss"] != good["loss"]                                # the three rows do count for something


# ---- guard bands ------------------------------------------------------------------------------------------------------------------
def _guard_spec(i, grads, shift):
    """The raw C-ABI call of case i between guard bands: x, rows, labels, mean, inv_std and the parameter arena are inputs; loss and
    hits are outputs; dw / db are slices of ONE guarded arena whose prior is finite and whose inter-head padding must stay as it
    was; the workspace is poisoned.  The reference of every head is the single-head call's bits."""
    from cstp_amd import _lib
    lib = _lib.load()
    G, m, n, d, c, _ = ss.SWEEP_CASES[i]
    case, dev = _case(i)
    alone = _alone(i, True)
    seg, wn = ss.head_stride(c, d), ss.pad4(c * d)
    own = torch.from_numpy(ss.owned_mask(G, c, d))
    inputs = {"x": torch.from_numpy(case["x"]), "rows": torch.from_numpy(case["rows"]), "labels": torch.from_numpy(case["labels"]),
              "mean": torch.from_numpy(case["mean"]), "inv_std": torch.from_numpy(case["inv_std"]),
              "params": torch.from_numpy(ss.arena_of(case["w"], case["b"]))}
    outputs = {"loss": ((G,), F32), "hits": ((G,), I32)}
    checks = {"loss": gb.bits_check(torch.cat([a[0] for a in alone]).cpu()), "hits": gb.bits_check(torch.cat([a[1] for a in alone]).cpu())}
    priors = {}
    if grads:
        rs = np.random.RandomState(5)
        prior = torch.from_numpy(rs.uniform(0.5, 1.5, size=G * seg).astype(np.float32))
        want = prior.clone()
        for g, a in enumerate(alone):
            want[g * seg:g * seg + c * d] = a[2].cpu().reshape(-1)
            want[g * seg + wn:g * seg + wn + c] = a[3].cpu()
        outputs["grads"] = ((G * seg,), F32)
        checks["grads"] = gb.all_checks(gb.untouched_check(prior, ~own), gb.bits_check(want, own))
        priors["grads"] = prior
    nbytes = lib.cstp_probe_sweep_workspace_bytes(G, m, d, c)
    assert nbytes > 0 and int((~own).sum()) == G * (seg - c * d - c)       # 9 floats of padding in the first case, none in the second
    spec = gb.Spec("probe_sweep_%s %s x shift %d" % ("step" if grads else "score", ss.SWEEP_CASES[i], shift), inputs, outputs, checks,
                   ws_bytes=nbytes, priors=priors, shifts={"x": shift}, finite_as={"hits": None})
    stream = torch.cuda.current_stream().cuda_stream

    def impl(v):
        p = v["params"].data_ptr()
        head = (stream, v["x"].data_ptr(), v["rows"].data_ptr(), v["labels"].data_ptr(), v["mean"].data_ptr(), v["inv_std"].data_ptr(),
                p, p + 4 * wn, seg, G, m, n, d, c, v["loss"].data_ptr(), v["hits"].data_ptr())
        if grads:
            q = v["grads"].data_ptr()
            _lib.check(lib.cstp_probe_sweep_step(*head, q, q + 4 * wn, v["ws"].data_ptr(), nbytes), "cstp_probe_sweep_step")
        else:
            _lib.check(lib.cstp_probe_sweep_score(*head, v["ws"].data_ptr(), nbytes), "cstp_probe_sweep_score")
    return spec, impl


@pytest.mark.parametrize("shift", [0, 4], ids=["x aligned", "x one element off"])
@pytest.mark.parametrize("i,grads", [(i, True) for i in ss.GUARD_STEP_CASES] + [(i, False) for i in ss.GUARD_SCORE_CASES])
def test_sweep_between_poisoned_guard_bands(i, grads, shift):
    spec, impl = _guard_spec(i, grads, shift)
    found = gb.three_runs(spec, impl, DEV, torch.cuda.synchronize)
    if spec.priors:
        found += gb.live_run(spec, impl, DEV, torch.cuda.synchronize)
    assert found == [], "\n".join(found)


# ---- the fit ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _train_data():
    t = ss.TRAIN
    feat, lab = ss.make_clusters(t["n"], t["d"], t["c"], 2.0, seed=3)
    return feat.to(DEV), lab.to(DEV)


def _step_on(feat, lab, fitted, rows):
    from cstp_amd import ops
    return ops.probe_step(feat, lab, fitted.w, fitted.b, rows, fitted.mean, fitted.inv_std)


@pytest.mark.parametrize("batch", [ss.TRAIN["batch"], 0], ids=["batch 32", "full batch"])
@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_a_head_trains_as_it_would_alone(optimizer, batch):
    from cstp_amd import probe
    t = ss.TRAIN
    feat, lab = _train_data()
    res = probe.sweep(feat, lab, t["c"], t["lrs"], t["wds"], t["val_fraction"], epochs=t["epochs"], batch=batch, optimizer=optimizer,
                      momentum=0.9, seed=t["seed"])
    train, val = ss.holdout_ref(lab.cpu().numpy(), t["val_fraction"], t["seed"])
    assert np.array_equal(res.train_idx, train) and np.array_equal(res.val_idx, val) and train.size == 71 and val.size == 25
    steps = t["epochs"] * (3 if batch else 1)
    assert res.grid == ss.grid_ref(t["lrs"], t["wds"]) and len(res.grid) == 4
    assert tuple(res.loss_log.shape) == tuple(res.hit_log.shape) == (steps, 4) and res.loss_log.is_cuda and res.hit_log.is_cuda
    assert res.loss_log.dtype == F32 and res.hit_log.dtype == I32
    assert res.val_hits.dtype == I32 and res.val_loss.dtype == F32 and not res.val_hits.is_cuda and not res.val_loss.is_cuda
    idx = torch.from_numpy(train).to(DEV).long()
    sub_feat, sub_lab = feat[idx], lab[idx]
    loss_log, hit_log = res.loss_log.cpu(), res.hit_log.cpu()
    for g, (lr, wd) in enumerate(res.grid):
        alone = probe.fit(sub_feat, sub_lab, t["c"], epochs=t["epochs"], batch=batch, lr=lr, weight_decay=wd, optimizer=optimizer,
                          momentum=0.9, seed=t["seed"])
        assert torch.equal(res.mean, alone.mean) and torch.equal(res.inv_std, alone.inv_std)
        assert torch.equal(res.w[g], alone.w), "W of head %d (%g, %g)" % (g, lr, wd)
        assert torch.equal(res.b[g], alone.b), "b of head %d (%g, %g)" % (g, lr, wd)
        assert torch.equal(loss_log[:, g], alone.loss_log) and torch.equal(hit_log[:, g], alone.hit_log), g
        # the validation score is the single-head step's loss and hit count of the held-out rows under the fitted head
        l1, h1, _, _ = _step_on(feat, lab, alone, torch.from_numpy(val).to(DEV))
        assert torch.equal(res.val_loss[g:g + 1], l1.cpu()) and torch.equal(res.val_hits[g:g + 1], h1.cpu())
    assert not torch.equal(res.w[0], res.w[1]) and not torch.equal(res.w[0], res.w[2])      # decay and rate both matter


# ---- selection and refit -------------------------------------------------------------------------------------------------------------
class _Rows(torch.nn.Module):
    """An "encoder" whose feature of a one-clip video is the clip: probe.evaluate on a feature matrix given as a loader."""

    def encode(self, clips):
        return clips


def _loader(feat, lab):
    return [(feat[i].reshape(1, 1, -1), lab[i].reshape(1)) for i in range(feat.shape[0])]


def test_the_sweep_selects_and_evaluate_refits_with_the_unchanged_fit():
    from cstp_amd import probe
    s = ss.SELECT
    feat, lab = ss.select_data()
    feat, lab = feat.to(DEV), lab.to(DEV)
    args = dict(epochs=s["epochs"], batch=s["batch"], seed=s["seed"])
    res = probe.sweep(feat, lab, s["c"], s["lrs"], val_fraction=s["val_fraction"], **args)
    best = probe.select(res)
    print("selection: validation hits %s of %d, loss %s" % (res.val_hits.tolist(), res.val_idx.size, res.val_loss.tolist()))
    assert res.grid[best] == (1e-2, 0.0) and best == ss.select_ref(res.val_hits.tolist(), res.val_loss.tolist())
    gallery, queries = _loader(feat[:600], lab[:600]), _loader(feat[600:], lab[600:])
    model = _Rows()
    swept = probe.evaluate(model, gallery, queries, s["c"], lrs=list(s["lrs"]), val_fraction=s["val_fraction"], **args)
    plain = probe.evaluate(model, gallery, queries, s["c"], lr=1e-2, **args)
    assert set(plain) == {"top1", "top5", "train_top1", "first_loss", "last_epoch_loss", "n_query", "n_gallery", "feature_dim",
                          "n_classes", "epochs", "batch", "lr", "weight_decay", "optimizer"}
    assert set(swept) == set(plain) | {"sweep", "selected_lr", "selected_wd", "val_fraction", "n_val"}
    assert (swept["selected_lr"], swept["selected_wd"], swept["val_fraction"]) == (1e-2, 0.0, s["val_fraction"])
    for key in plain:
        assert swept[key] == plain[key], key                          # top1 / top5 included: exactly equal
    assert [(p["lr"], p["wd"]) for p in swept["sweep"]] == [(1e-6, 0.0), (1e-2, 0.0)]
    n_val = ss.holdout_ref(lab[:600].cpu().numpy(), s["val_fraction"], s["seed"])[1].size
    assert swept["n_val"] == n_val and 140 <= n_val <= 160 and all(0.0 <= p["val_top1"] <= 1.0 and p["val_loss"] > 0 for p in swept["sweep"])
    assert swept["sweep"][1]["val_top1"] > swept["sweep"][0]["val_top1"]


# ---- the driver --------------------------------------------------------------------------------------------------------------------
def _run(args, timeout):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args[0], r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def _write_checkpoint(path):
    """A randomly initialised depth-1 R(2+1)D-BYOL in the layout main_byol.py saves: the driver only reads the encoder."""
    from cstp_amd.model import SingleDeviceParallel
    from cstp_amd.r21d_byol import R21DBYOL
    torch.manual_seed(0)
    model = SingleDeviceParallel(R21DBYOL(pretrain=True, layer_sizes=(1, 1, 1, 1)))
    torch.save({"epoch": 0, "arch": "r21d_byol-1", "state_dict": model.state_dict()}, path)


def test_linear_probe_driver_sweeps_on_synthetic_videos(tmp_path):
    """linear_probe.py on synthetic videos under an untrained depth-1 encoder (nothing here depends on what the encoder knows), at
    the model and clip of the existing driver chain, with a 2 x 1 grid and without one.  Each a child process with its own time
    limit; no accuracy is asserted."""
    res = str(tmp_path / "res")
    ckpt = str(tmp_path / "init.pth")
    _write_checkpoint(ckpt)
    base = ["linear_probe.py", "--dataset", "synthetic_video", "--sample_duration", "8", "--pb_rate", "2", "--synthetic_len", "32",
            "--retrieval_gallery_len", "40", "--transform_mode", "img_test", "--sample_size", "112", "--n_classes", "4",
            "--n_finetune_classes", "4", "--probe_epochs", "3", "--probe_batch", "16", "--model_name", "r21d_byol", "--model_depth", "1",
            "--result_path", res, "--pretrained_path", ckpt]
    out = _run(base + ["--probe_lrs", "1e-3", "1e-2"], 300)
    path = os.path.join(res, "synthetic_video", "probe_r21d_byol1_synthetic_video_1_8.txt")
    lines = [ln for ln in open(path).read().split("\n") if ln]
    summary = json.loads(lines[-1])
    assert json.loads([ln for ln in out.split("\n") if ln.startswith("{")][-1]) == summary
    assert {"sweep", "selected_lr", "selected_wd", "val_fraction", "n_val"} <= set(summary)
    assert [(p["lr"], p["wd"]) for p in summary["sweep"]] == [(1e-3, 0.0), (1e-2, 0.0)]
    assert summary["selected_lr"] in (1e-3, 1e-2) and summary["selected_wd"] == 0.0 and summary["lr"] == summary["selected_lr"]
    assert summary["val_fraction"] == 0.2 and summary["n_val"] == 8 and summary["n_gallery"] == 40
    sweep_lines = [ln for ln in lines if ln.startswith("Probe sweep lr = ")]
    assert len(sweep_lines) == 2 and sweep_lines[0].startswith("Probe sweep lr = 0.001, wd = 0: val top-1 = ")
    assert all(ln in out.split("\n") for ln in sweep_lines)
    want = "Probe sweep selected lr = %g, wd = 0" % summary["selected_lr"]
    assert want in lines and want in out.split("\n")
    assert lines.index(want) < lines.index("Linear probe top-1 = %.4f" % summary["top1"])
    plain = _run(base, 300)
    assert "Probe sweep" not in plain and "Probe sweep" not in open(path).read()
    keys = set(json.loads([ln for ln in plain.split("\n") if ln.startswith("{")][-1]))
    assert keys == set(summary) - {"sweep", "selected_lr", "selected_wd", "val_fraction", "n_val"}
    assert "probe_lrs" not in plain and "probe_val_fraction" not in plain          # the options dump is as it was

"""k-means clustering evaluation on the GPU: ops.kmeans_assign against the bits of ops.sim_topk and the fp64 specification of
tests/cluster_spec.py on its five shapes and on an unaligned view, the tie order; ops.kmeans_update against the spec within four
times the fp32 restatement's error, empty clusters and out-of-range assignments behind canaries; determinism and independence of
the batch of restarts; Lloyd's fixed point; cluster.fit on separable clusters; and the cluster.py driver in a child process."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cluster_spec import (CASES, MAX_NEAR_TIE_SHARE, assign_ref, make_case, restatement_error, spec_assignment, update_bound, update_ref)
from probe_spec import make_clusters
from test_cluster_host import FIT_ARGS, FIT_DATA

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"

# ops.kmeans_update against the fp64 spec, |error| of unit centroid rows over CASES.  The torch-fp32 restatement of the kernel's
# documented summation order (cluster_spec.update_restated_fp32) is within 1.13e-7 of the spec on these cases; the bound is
# 4 x that = 4.51e-7 (cluster_spec.update_bound, computed here on the CPU).  ops.kmeans_update on an MI355X: 1.13e-7, on
# (600, 96, 10, 4); 0, 5.1e-8, 2.2e-8 and 9.9e-8 on the other four -- the restatement's own figures.  Nothing was widened.


@functools.lru_cache(maxsize=None)
def _case(i):
    """Case i of CASES as (numpy dict, device dict, fp64 assignment spec): made once, shared, never written."""
    case = make_case(*CASES[i])
    dev = {k: torch.tensor(v, device=DEV) for k, v in case.items() if isinstance(v, np.ndarray)}          # a copy: the arrays are read-only
    return case, dev, assign_ref(case["x"], case["cent"])


def _check_assign(out, x, cent, prev, ref, what):
    """out of ops.kmeans_assign(x, cent, prev) on device tensors; ref = assign_ref of the same numbers."""
    from cstp_amd import ops
    assign, best, moved, score = out
    r, c, d = cent.shape
    n = x.shape[0]
    assert assign.dtype == torch.int32 and best.dtype == torch.float32 and moved.dtype == torch.int32 and score.dtype == torch.float64
    assert tuple(assign.shape) == tuple(best.shape) == (r, n) and tuple(moved.shape) == tuple(score.shape) == (r,)
    for s in range(r):
        val, idx = ops.sim_topk(x, cent[s].contiguous(), 1)
        assert torch.equal(idx[:, 0], assign[s]), "%s: restart %d: assign is not sim_topk's index" % (what, s)
        assert torch.equal(val[:, 0].view(torch.int32), best[s].view(torch.int32)), "%s: restart %d: best is not sim_topk's bits" % (what, s)
    a, b = assign.cpu().numpy(), best.cpu().numpy().astype(np.float64)
    want_moved = (a != prev.cpu().numpy()).sum(axis=1) if prev is not None else np.full(r, n)
    assert moved.cpu().tolist() == want_moved.tolist(), (what, moved.cpu().tolist(), want_moved.tolist())
    sums = b.sum(axis=1)
    rel = np.abs(score.cpu().numpy() - sums) / np.maximum(np.abs(sums), 1e-300)
    differ = a != ref["assign"]
    print("%s: score rel err %.3g, rows that differ from the fp64 spec %d (near ties %d of %d)"
          % (what, rel.max(), differ.sum(), ref["near"].sum(), differ.size))
    assert rel.max() <= 1e-12
    assert not (differ & ~ref["near"]).any(), "%s: a row whose choice is decided at fp32 precision differs from the spec" % what
    assert ref["near"].mean() <= MAX_NEAR_TIE_SHARE
    from retrieval_spec import tau_for
    assert np.abs(b - ref["best"]).max() <= tau_for(d)


@pytest.mark.parametrize("i", range(len(CASES)))
@pytest.mark.parametrize("with_prev", [False, True])
def test_assign_is_sim_topk_bit_for_bit_and_the_spec_up_to_near_ties(i, with_prev):
    from cstp_amd import ops
    case, dev, ref = _case(i)
    prev = dev["prev"] if with_prev else None
    out = ops.kmeans_assign(dev["x"], dev["cent"], prev)
    _check_assign(out, dev["x"], dev["cent"], prev, ref, "assign %s prev=%s" % (CASES[i], with_prev))
    again = ops.kmeans_assign(dev["x"], dev["cent"], prev)
    for a, b in zip(out, again):
        assert torch.equal(a, b)


def test_assign_on_views_offset_by_one_float():
    """x and cent start one float into their buffers: 4-byte aligned pointers, the scalar load path, the same bits."""
    from cstp_amd import ops
    case, dev, ref = _case(4)                                # d = 96: a multiple of 4, so only the pointers are unaligned
    n, d, c, r = CASES[4]
    xb = torch.zeros(n * d + 1, device=DEV)
    cb = torch.zeros(r * c * d + 1, device=DEV)
    xb[1:] = dev["x"].reshape(-1)
    cb[1:] = dev["cent"].reshape(-1)
    xv, cv = xb[1:].view(n, d), cb[1:].view(r, c, d)
    assert xv.data_ptr() % 16 == 4 and cv.data_ptr() % 16 == 4 and xv.is_contiguous()
    out = ops.kmeans_assign(xv, cv, dev["prev"])
    _check_assign(out, xv, cv, dev["prev"], ref, "assign on offset views")
    for a, b in zip(out, ops.kmeans_assign(dev["x"], dev["cent"], dev["prev"])):
        assert torch.equal(a, b)
    new, counts = ops.kmeans_update(xv, out[0], cv)
    new2, counts2 = ops.kmeans_update(dev["x"], out[0], dev["cent"])
    assert torch.equal(new, new2) and torch.equal(counts, counts2)


def test_assign_gives_duplicated_centroids_to_the_lowest_id():
    from cstp_amd import ops
    case, dev, _ = _case(2)                                  # 200 rows: centroids 0..99 and their copies at 100..199
    half = dev["cent"][:, :100].contiguous()
    cent = torch.cat([half, half], dim=1).contiguous()       # copies of 28..99 lie in the second centroid tile, the rest in the first
    assign, best, _, _ = ops.kmeans_assign(dev["x"], cent)
    alone, best_alone, _, _ = ops.kmeans_assign(dev["x"], half)
    assert int(assign.max()) < 100 and torch.equal(assign, alone) and torch.equal(best, best_alone)
    assert int((assign >= 28).sum()) > 0                     # some winners do have their copy in the other tile
    val, idx = ops.sim_topk(dev["x"], cent[0].contiguous(), 1)
    assert torch.equal(idx[:, 0], assign[0]) and torch.equal(val[:, 0], best[0])
    same = torch.zeros((1, 3, 7), device=DEV)               # every similarity is +0.0: id 0
    same[0, :, 0] = 1.0
    x = torch.zeros((5, 7), device=DEV)
    x[:, 1] = 1.0
    assert ops.kmeans_assign(x, same)[0].cpu().tolist() == [[0] * 5]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_update_against_the_spec(i):
    from cstp_amd import ops
    case, dev, _ = _case(i)
    a = spec_assignment(case)
    ref, ref_counts = update_ref(case["x"], a, case["cent"])
    new, counts = ops.kmeans_update(dev["x"], torch.from_numpy(a).to(DEV), dev["cent"])
    assert new.dtype == torch.float32 and counts.dtype == torch.int32 and new.data_ptr() != dev["cent"].data_ptr()
    assert counts.cpu().numpy().tolist() == ref_counts.tolist()
    err = float(np.abs(new.cpu().numpy().astype(np.float64) - ref).max())
    print("update %s: |error| %.3g (fp32 restatement over all cases %.3g, bound %.3g)" % (CASES[i], err, restatement_error(), update_bound()))
    assert err <= update_bound()
    empty = ref_counts == 0
    assert torch.equal(new.cpu()[torch.from_numpy(empty)], torch.tensor(case["cent"])[torch.from_numpy(empty)])
    new2, counts2 = ops.kmeans_update(dev["x"], torch.from_numpy(a).to(DEV), dev["cent"])
    assert torch.equal(new, new2) and torch.equal(counts, counts2)


def test_update_keeps_empty_clusters_and_never_indexes_with_a_bad_assignment():
    """The C entry point on buffers with canaries around cent_out and counts: an empty cluster and rows whose assignment lies
    outside 0..c-1 (negative, c itself, huge) -- the old centroid stays, the bad rows count nowhere, the canaries survive."""
    from cstp_amd import _lib, ops
    lib = _lib.load()
    case, dev, _ = _case(1)
    n, d, c, r = CASES[1]
    a = spec_assignment(case).copy()
    a[1, a[1] == 1] = 2                                      # cluster 1 of restart 1 is empty
    a[0, :6] = (-1, c, 1 << 30, -(1 << 31), 0x7fffffff, c + 1)
    a_dev = torch.from_numpy(a).to(DEV)
    pad = 64
    cbuf = torch.full((r * c * d + 2 * pad,), 777.0, device=DEV)
    nbuf = torch.full((r * c + 2 * pad,), -99, dtype=torch.int32, device=DEV)
    cent_out, counts = cbuf[pad:pad + r * c * d], nbuf[pad:pad + r * c]
    _lib.check(lib.cstp_kmeans_update(torch.cuda.current_stream().cuda_stream, dev["x"].data_ptr(), a_dev.data_ptr(),
                                      dev["cent"].data_ptr(), n, d, c, r, cent_out.data_ptr(), counts.data_ptr()), "cstp_kmeans_update")
    torch.cuda.synchronize()
    assert bool((cbuf[:pad] == 777.0).all()) and bool((cbuf[pad + r * c * d:] == 777.0).all())
    assert bool((nbuf[:pad] == -99).all()) and bool((nbuf[pad + r * c:] == -99).all())
    ref, ref_counts = update_ref(case["x"], a, case["cent"])
    assert counts.view(r, c).cpu().tolist() == ref_counts.tolist() and int(ref_counts[0].sum()) == n - 6 and ref_counts[1, 1] == 0
    got = cent_out.view(r, c, d).cpu()
    assert torch.equal(got[1, 1], torch.tensor(case["cent"][1, 1]))
    assert float(np.abs(got.numpy().astype(np.float64) - ref).max()) <= update_bound()
    # the aliased call is refused
    rc = lib.cstp_kmeans_update(torch.cuda.current_stream().cuda_stream, dev["x"].data_ptr(), a_dev.data_ptr(), dev["cent"].data_ptr(),
                                n, d, c, r, dev["cent"].data_ptr(), counts.data_ptr())
    assert rc != 0 and b"must not alias" in lib.cstp_last_error()
    with pytest.raises(_lib.CstpError, match="must not alias"):
        ops.kmeans_update(dev["x"], a_dev, dev["cent"], out=(dev["cent"], counts.view(r, c)))


def test_a_restart_in_a_batch_gets_the_bits_it_gets_alone():
    from cstp_amd import ops
    for i in (1, 4):
        case, dev, _ = _case(i)
        r = CASES[i][3]
        assign, best, moved, score = ops.kmeans_assign(dev["x"], dev["cent"], dev["prev"])
        new, counts = ops.kmeans_update(dev["x"], assign, dev["cent"])
        for s in range(r):
            one = ops.kmeans_assign(dev["x"], dev["cent"][s:s + 1].contiguous(), dev["prev"][s:s + 1].contiguous())
            for whole, alone in zip((assign, best, moved, score), one):
                assert torch.equal(whole[s], alone[0])
            new1, counts1 = ops.kmeans_update(dev["x"], one[0], dev["cent"][s:s + 1].contiguous())
            assert torch.equal(new[s], new1[0]) and torch.equal(counts[s], counts1[0])


@functools.lru_cache(maxsize=None)
def _fit_data():
    feat, lab = make_clusters(FIT_DATA["n"], FIT_DATA["d"], FIT_DATA["c"], FIT_DATA["sep"])
    return feat.to(DEV), lab.to(DEV)


def test_lloyd_reaches_a_fixed_point_and_stays_there():
    """assign / update by hand from fit's own seeding: once moved == 0, centroids and assignment repeat bit for bit."""
    from cstp_amd import cluster, ops
    feat, _ = _fit_data()
    x = ops.l2_normalize(feat)
    cent = cluster.init_pp(x, cluster.plan(x.shape[0], FIT_ARGS["k"], FIT_ARGS["restarts"], FIT_ARGS["seed"]))
    prev, history = None, []
    for t in range(FIT_ARGS["iters"]):
        assign, _, moved, _ = ops.kmeans_assign(x, cent, prev)
        history.append((cent, assign, moved.cpu()))
        cent, _ = ops.kmeans_update(x, assign, cent)
        prev = assign
    for s in range(FIT_ARGS["restarts"]):
        still = [t for t in range(len(history)) if int(history[t][2][s]) == 0]
        assert still and still[0] < FIT_ARGS["iters"] - 1, (s, [int(h[2][s]) for h in history])
        t0 = still[0]
        for t in range(t0, len(history)):
            assert int(history[t][2][s]) == 0
            assert torch.equal(history[t][1][s], history[t0][1][s]) and torch.equal(history[t][1][s], history[t0 - 1][1][s])
            if t > t0:
                assert torch.equal(history[t][0][s], history[t0][0][s])
        assert torch.equal(cent[s], history[t0][0][s])


def test_fit_separates_the_clusters_and_repeats_itself():
    from cstp_amd import cluster, ops
    feat, lab = _fit_data()
    res = cluster.fit(feat, **FIT_ARGS)
    k, iters, restarts = FIT_ARGS["k"], FIT_ARGS["iters"], FIT_ARGS["restarts"]
    assert tuple(res.cent.shape) == (k, FIT_DATA["d"]) and tuple(res.assign.shape) == (FIT_DATA["n"],) and res.assign.dtype == torch.int32
    assert tuple(res.score_log.shape) == tuple(res.moved_log.shape) == (iters, restarts) and tuple(res.final_scores.shape) == (restarts,)
    table = cluster.contingency(res.assign, lab, k, FIT_DATA["c"])
    assert int(table.sum()) == FIT_DATA["n"] and table.is_cuda
    assert cluster.nmi(table) == pytest.approx(1.0, abs=1e-12) and cluster.matched_accuracy(table) == 1.0
    assert 0 <= int(res.converged_at[res.restart]) < iters - 1
    assert res.moved_log[0].tolist() == [FIT_DATA["n"]] * restarts
    for s in range(restarts):
        t0 = int(res.converged_at[s])
        assert (t0 >= 0) == bool((res.moved_log[:, s] == 0).any())
        if t0 >= 0:
            assert bool((res.moved_log[t0:, s] == 0).all()) and bool((res.moved_log[:t0, s] != 0).all())
            assert bool((res.score_log[t0:, s] == res.final_scores[s]).all())           # the same centroids, the same bits
    finals = res.final_scores.tolist()
    assert res.restart == max(range(restarts), key=lambda s: (finals[s], -s)) and res.score == finals[res.restart]
    assert res.counts.tolist() == torch.bincount(res.assign.to(torch.int64), minlength=k).tolist() and int(res.counts.sum()) == FIT_DATA["n"]
    # the result describes itself: assigning the rows to res.cent gives res.assign and res.score
    x = ops.l2_normalize(feat)
    assign, _, _, score = ops.kmeans_assign(x, res.cent.unsqueeze(0).contiguous())
    assert torch.equal(assign[0], res.assign) and float(score[0]) == res.score
    assert torch.equal(cluster.predict(res, feat), res.assign)
    again = cluster.fit(feat, **FIT_ARGS)
    for a, b in zip(res, again):
        assert torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b
    other = cluster.fit(feat, **dict(FIT_ARGS, seed=FIT_ARGS["seed"] + 1))
    assert not torch.equal(other.score_log, res.score_log)


def _write_checkpoint(path):
    """A randomly initialised depth-1 R(2+1)D-BYOL in the layout main_byol.py saves: the drivers only read the encoder."""
    from cstp_amd.model import SingleDeviceParallel
    from cstp_amd.r21d_byol import R21DBYOL
    torch.manual_seed(0)
    model = SingleDeviceParallel(R21DBYOL(pretrain=True, layer_sizes=(1, 1, 1, 1)))
    torch.save({"epoch": 0, "arch": "r21d_byol-1", "state_dict": model.state_dict()}, path)


def test_cluster_driver(tmp_path):
    """cluster.py in a child process on synthetic videos with an untrained depth-1 encoder: the result file, the JSON line and
    the ranges.  No quality is asserted: such an encoder promises none."""
    res = str(tmp_path / "res")
    ckpt = str(tmp_path / "init.pth")
    _write_checkpoint(ckpt)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    args = ["cluster.py", "--dataset", "synthetic_video", "--sample_duration", "8", "--pb_rate", "2", "--synthetic_len", "32",
            "--retrieval_gallery_len", "12", "--pretrained_path", ckpt, "--transform_mode", "img_test", "--sample_size", "112",
            "--n_classes", "4", "--n_finetune_classes", "4", "--cluster_iters", "5", "--cluster_restarts", "3", "--model_name",
            "r21d_byol", "--model_depth", "1", "--result_path", res]
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    path = os.path.join(res, "synthetic_video", "cluster_r21d_byol1_synthetic_video_1_8.txt")
    assert os.path.isfile(path), path
    lines = [ln for ln in open(path).read().split("\n") if ln]
    summary = json.loads(lines[-1])
    assert json.loads([ln for ln in r.stdout.split("\n") if ln.startswith("{")][-1]) == summary
    assert summary["task"] == "cluster" and summary["arch"] == "r21d_byol-1" and summary["split"] == "1"
    assert (summary["n_query"], summary["n_gallery"], summary["feature_dim"], summary["k"]) == (8, 12, 512, 4)
    assert (summary["iters"], summary["restarts"], summary["seed"]) == (5, 3, 1) and 0 <= summary["restart"] < 3
    for part in ("train", "test"):
        for key, lo, name in (("nmi", 0.0, "NMI"), ("ari", -1.0, "ARI"), ("purity", 0.0, "purity"), ("acc", 0.0, "acc")):
            v = summary["%s_%s" % (part, key)]
            assert lo <= v <= 1.0, (part, key, v)
            want = "Cluster %s = %.4f (%s)" % (name, v, part)
            assert want in lines and want in r.stdout.split("\n")

"""Video retrieval on the GPU: ops.sim_topk (csrc/retrieve.hip) against the acceptance rule of tests/retrieval_spec.py, its tie
order, insertion extremes, exclude_self, determinism and independence of the gallery split, its memory bound; ByolBase.encode;
the retrieval pipeline end to end on synthetic videos; the driver chain in child processes."""
import argparse
import json
import os
import subprocess
import sys

import pytest
import torch

from retrieval_spec import check_topk, stable_reference, tau_for, unit_rows
from test_frame_folder_host import VIDEOS, write_tree

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSPLIT = "CSTP_SIMTOPK_NSPLIT"      # developer override of the gallery split (1 = the unsplit path)

# The kernel's tiles are 64 queries x 128 gallery rows x 32 features; the gallery is split over
# min(32, 256 / query tiles, gallery tiles / 4) blocks per query tile.  The first eight shapes are the issue's; of those
# (1500, 1300, ...) splits in two under this rule (24 query tiles, 11 gallery tiles) -- the unsplit path at many query tiles is
# pinned through the override in test_split_does_not_change_the_answer.  The rest sit one below / on / one above each edge:
# query tile 63 / 64 / 65, gallery tile 127 / 128 / 129, feature chunk 31 / 32 / 33 and feature counts that are no multiple of 4
# (the scalar staging path); the split thresholds 7 -> 8 gallery tiles (896 / 897 rows: 1 -> 2 blocks) and 128 -> 129 query tiles
# (8192 / 8193 queries: 2 -> 1 blocks); (7, 20000) sits at the cap of 32.
SHAPES = [(1, 1, 8, 1), (3, 5, 7, 5), (2, 3, 16, 5), (64, 128, 128, 1), (65, 257, 512, 50), (7, 20000, 512, 64),
          (1500, 1300, 1024, 20), (33, 4097, 2048, 10),
          (63, 127, 31, 3), (64, 129, 33, 7), (65, 128, 32, 64), (5, 896, 30, 8), (5, 897, 36, 8), (8192, 1024, 8, 1),
          (8193, 1024, 8, 2)]


def _dev(t):
    return t.cuda()


@pytest.mark.parametrize("nq,ng,d,k", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_sim_topk_meets_the_acceptance_rule(nq, ng, d, k):
    from cstp_amd import ops
    q, g = unit_rows(nq, d, 100 + nq), unit_rows(ng, d, 200 + ng)
    val, idx = ops.sim_topk(_dev(q), _dev(g), k)
    assert val.dtype == torch.float32 and idx.dtype == torch.int32 and val.is_cuda and idx.is_cuda
    check_topk(val, idx, q, g, k, False, tau_for(d))


def test_ties_are_ordered_by_gallery_index():
    from cstp_amd import ops
    nq, d, k = 9, 96, 40
    base = unit_rows(50, d, 5)
    # every row appears four times, far apart and across gallery tiles: rows j, j + 50, j + 100, j + 150 are the same vector
    g = torch.cat([base, base, base, base])
    q = unit_rows(nq, d, 6)
    val, idx = ops.sim_topk(_dev(q), _dev(g), k)
    check_topk(val, idx, q, g, k, False, tau_for(d))
    val, idx = val.cpu(), idx.cpu().to(torch.int64)
    grp = idx.reshape(nq, k // 4, 4)
    assert bool((grp[:, :, 1:] == grp[:, :, :1] + torch.tensor([50, 100, 150])).all())      # exactly j, j+50, j+100, j+150
    assert bool((grp[:, :, 0] < 50).all())
    v = val.reshape(nq, k // 4, 4).contiguous().view(torch.int32)
    assert bool((v == v[:, :, :1]).all())                                                  # the same vector, the same bits
    # the same across the split: 30 000 copies of one row, any k of them tie and the first k rows win
    one = unit_rows(1, d, 7)
    val, idx = ops.sim_topk(_dev(q), _dev(one.expand(30000, d).contiguous()), 64)
    assert torch.equal(idx.cpu(), torch.arange(64, dtype=torch.int32).expand(nq, 64))
    assert bool((val.cpu().view(torch.int32) == val.cpu().view(torch.int32)[:, :1]).all())
    val, idx = ops.sim_topk(_dev(q), _dev(one.expand(100, d).contiguous()), 17)
    assert torch.equal(idx.cpu(), torch.arange(17, dtype=torch.int32).expand(nq, 17))


@pytest.mark.parametrize("ng", [700, 5000], ids=["unsplit", "split"])
def test_insertion_extremes(ng):
    """A gallery whose similarities ascend along j: every candidate displaces one.  Descending: none does after the first k."""
    from cstp_amd import ops
    d, k = 24, 33
    e0, e1 = torch.zeros(d), torch.zeros(d)
    e0[0], e1[1] = 1.0, 1.0
    ang = torch.linspace(1.5, 0.1, ng, dtype=torch.float64).reshape(-1, 1)              # cos ascends along j
    up = (torch.cos(ang) * e0.double() + torch.sin(ang) * e1.double()).float().contiguous()
    q = e0.reshape(1, d).repeat(3, 1).contiguous()
    q[1] = -q[1]                                                                         # for this query the order is reversed
    q[2] = e1
    for g in (up, up.flip(0).contiguous()):
        val, idx = ops.sim_topk(_dev(q), _dev(g), k)
        check_topk(val, idx, q, g, k, False, tau_for(d))
        rv, ri = stable_reference(q, g, k)
        assert torch.equal(idx.cpu(), ri)                                                # spacing is far above tau: one answer


def test_exclude_self():
    from cstp_amd import ops
    for n, d, k in ((300, 64, 10), (5, 12, 8), (2000, 40, 3)):
        x = unit_rows(n, d, 40 + n)
        xd = _dev(x)
        val, idx = ops.sim_topk(xd, xd, k, exclude_self=True)
        check_topk(val, idx, x, x, k, True, tau_for(d))
        assert not bool((idx.cpu() == torch.arange(n).reshape(-1, 1)).any())
        val, idx = ops.sim_topk(xd, xd, k)
        check_topk(val, idx, x, x, k, False, tau_for(d))
        assert torch.equal(idx[:, 0].cpu().to(torch.int64), torch.arange(n))             # a unit row is its own best match


def test_split_does_not_change_the_answer(monkeypatch):
    """Two calls give the same bits; the (7, 20000) answer (32 blocks along the gallery) equals, bit for bit, rows 0..6 of a
    1 500-query call on the unsplit path, of the same call under its natural split (10), and the 7-query call under any split."""
    from cstp_amd import ops
    monkeypatch.delenv(NSPLIT, raising=False)
    d, k = 512, 64
    q7, g = unit_rows(7, d, 107), unit_rows(20000, d, 20200)
    big = torch.cat([q7, unit_rows(1493, d, 9)]).contiguous()
    q7d, gd, bigd = _dev(q7), _dev(g), _dev(big)
    val, idx = ops.sim_topk(q7d, gd, k)
    val2, idx2 = ops.sim_topk(q7d, gd, k)
    assert torch.equal(val.view(torch.int32), val2.view(torch.int32)) and torch.equal(idx, idx2)
    bv, bi = ops.sim_topk(bigd, gd, k)
    assert torch.equal(bv[:7].view(torch.int32), val.view(torch.int32)) and torch.equal(bi[:7], idx)
    monkeypatch.setenv(NSPLIT, "1")
    uv, ui = ops.sim_topk(bigd, gd, k)
    assert torch.equal(uv.view(torch.int32), bv.view(torch.int32)) and torch.equal(ui, bi)
    assert torch.equal(uv[:7].view(torch.int32), val.view(torch.int32)) and torch.equal(ui[:7], idx)
    for ns in ("1", "2", "3", "31"):
        monkeypatch.setenv(NSPLIT, ns)
        sv, si = ops.sim_topk(q7d, gd, k)
        assert torch.equal(sv.view(torch.int32), val.view(torch.int32)) and torch.equal(si, idx), ns
    monkeypatch.delenv(NSPLIT)
    check_topk(val, idx, q7, g, k, False, tau_for(d))


def test_memory_grows_with_queries_times_k():
    from cstp_amd import _lib, ops
    nq, ng, d, k = 4096, 65536, 128, 50
    gen = torch.Generator(device="cuda").manual_seed(3)
    q = torch.nn.functional.normalize(torch.randn((nq, d), device="cuda", generator=gen), dim=1)
    g = torch.nn.functional.normalize(torch.randn((ng, d), device="cuda", generator=gen), dim=1)
    ws = _lib.load().cstp_simtopk_workspace_bytes(nq, ng, d, k)
    assert ws < 0.01 * nq * ng * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    val, idx = ops.sim_topk(q, g, k)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print("sim_topk %dx%dx%d k=%d: peak growth %d B, outputs %d B, workspace %d B" % (nq, ng, d, k, grown, nq * k * 8, ws))
    assert grown <= nq * k * 8 + ws + (1 << 20)
    # and the answer is right where it can be checked cheaply: the first 64 queries
    check_topk(val[:64], idx[:64], q[:64].cpu(), g.cpu(), k, False, tau_for(d))


def _r3d_opts(depth, t, hw, k):
    return argparse.Namespace(model_depth=depth, sample_size=hw, sample_duration=t, sc_type="B", n_classes=k)


def test_encode_is_the_feature_the_heads_read():
    from cstp_amd import ops
    from cstp_amd.i3d_byol import I3DBYOL
    from cstp_amd.r21d_byol import R21DBYOL
    from cstp_amd.r3d_byol import R3DBYOL
    torch.manual_seed(0)
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand((3, 3, 4, 32, 32), device="cuda", generator=gen) * 2 - 1
    with torch.no_grad():
        m = R21DBYOL(pretrain=False, num_classes=5, cls_bn=True, layer_sizes=(1, 1, 1, 1)).cuda().eval()
        f = m.encode(x)
        assert tuple(f.shape) == (3, 512) and f.dtype == torch.float32
        assert torch.equal(m.classify(m.cls_bn(ops.l2_normalize(f))), m(x, o_type="test"))
        m = R3DBYOL(pretrain=False, cls_bn=True, opts=_r3d_opts(10, 8, 64, 5)).cuda().eval()
        x3 = torch.rand((2, 3, 8, 64, 64), device="cuda", generator=gen) * 2 - 1
        f = m.encode(x3)
        assert tuple(f.shape) == (2, 512)
        assert torch.equal(m.classify(m.classify_bn(ops.l2_normalize(f))), m(x3, o_type="test"))
        m = I3DBYOL(pretrain=True, opts=None).cuda().eval()
        f = m.encode(torch.rand((2, 3, 8, 64, 64), device="cuda", generator=gen) * 2 - 1)
        assert tuple(f.shape) == (2, 1024)
        assert float((f.double().norm(dim=1) - 1).abs().max()) < 1e-5                  # the encoder ends in its Normalize(2)
        # the pre-training wrapper of R(2+1)D returns (feature, projection): encode is the feature
        m = R21DBYOL(pretrain=True, layer_sizes=(1, 1, 1, 1)).cuda().eval()
        out = m.online_net(x)
        assert isinstance(out, tuple) and torch.equal(m.encode(x), out[0])


def test_retrieval_end_to_end_on_synthetic_videos():
    """R(2+1)D depth 1, 24 gallery and 16 query videos of 4 classes, 60 x 80 pixels; clips of 8 x 112 x 112, because the video
    test's ClipScale serves the sample sizes 112 and 224 only (sampler.short_side).  retrieve() passes the acceptance rule on the extracted features, and
    its R@k differs from the R@k of the fp64 stable answer by at most (queries whose top-k set differs) / nq, which is at most
    the number of queries with another similarity within tau of the k-th."""
    from cstp_amd import retrieval
    from cstp_amd.clip_ops import GpuLabelledLoader, GpuLabelledVideos
    from cstp_amd.r21d_byol import R21DBYOL
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    kw = dict(n_classes=4, height=60, width=80, sample_duration=8, sample_size=112, pb_rate=2)
    gallery = GpuLabelledVideos(dev, "test", "img_test", n_videos=24, seed=2, **kw)
    queries = GpuLabelledVideos(dev, "test", "img_test", n_videos=16, seed=1, **kw)
    model = R21DBYOL(pretrain=True, layer_sizes=(1, 1, 1, 1)).cuda()
    gf, gl = retrieval.extract_features(model, GpuLabelledLoader(gallery))
    qf, ql = retrieval.extract_features(model, GpuLabelledLoader(queries))
    assert tuple(gf.shape) == (24, 512) and tuple(qf.shape) == (16, 512) and gf.dtype == torch.float32 and gf.is_cuda
    assert gl.cpu().tolist() == gallery.labels and ql.cpu().tolist() == queries.labels
    assert not model.training
    # a video's feature is the mean over its test-plan clips
    clips, _ = gallery.video(2)
    with torch.no_grad():
        assert torch.equal(gf[2], model.encode(clips).mean(dim=0))
    ks = [5, 1, 10, 20]
    recall, val, idx, qn, gn = retrieval.retrieve(qf, ql, gf, gl, ks)
    kmax, tau = max(ks), tau_for(512)
    assert float((qn.double().norm(dim=1) - 1).abs().max()) < 1e-5
    check_topk(val, idx, qn, gn, kmax, False, tau)
    s = qn.double().cpu() @ gn.double().cpu().T
    ref = torch.sort(s, dim=1, descending=True, stable=True).indices[:, :kmax]
    ref_recall = retrieval.recall_at_k(ref, ql.cpu(), gl.cpu(), ks)
    srt = torch.sort(s, dim=1, descending=True).values
    got = idx.cpu().to(torch.int64)
    for k in ks:
        differ = sum(set(got[i, :k].tolist()) != set(ref[i, :k].tolist()) for i in range(16))
        close = int(((srt[:, k - 1:k] - srt[:, k:k + 1]).abs() <= tau).sum()) if k < 24 else 0
        print("R@%d = %.4f (fp64 stable answer %.4f): %d queries with another top-%d set, %d with a similarity within tau of the "
              "k-th" % (k, recall[k], ref_recall[k], differ, k, close))
        assert differ <= close
        assert abs(recall[k] - ref_recall[k]) <= differ / 16 + 1e-12
    assert [recall[k] for k in sorted(ks)] == sorted(recall.values()) and 0.0 <= min(recall.values()) and recall[20] <= 1.0


def _run(args, timeout):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args[0], r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def _check_result(path, out, ks, nq, ng):
    assert os.path.isfile(path), path
    lines = [ln for ln in open(path).read().split("\n") if ln]
    summary = json.loads(lines[-1])
    assert json.loads([ln for ln in out.split("\n") if ln.startswith("{")][-1]) == summary
    assert summary["n_query"] == nq and summary["n_gallery"] == ng and summary["feature_dim"] == 512
    r = [summary["recall"][str(k)] for k in ks]
    assert all(0.0 <= v <= 1.0 for v in r) and r == sorted(r)
    for k in ks:
        assert any(ln.startswith("R@%d = " % k) for ln in lines) and ("R@%d = " % k) in out


def test_retrieval_driver_chain(tmp_path):
    """main_byol.py (R(2+1)D depth 1 on synthetic clips; 100 one-step epochs, because the driver checkpoints every 100), then
    retrieval.py on that checkpoint: once on synthetic videos, once on a frame-folder tree.  Each a child process with its own
    time limit; a failing child ends the chain."""
    res = str(tmp_path / "res")
    model = ["--model_name", "r21d_byol", "--model_depth", "1", "--result_path", res]
    _run(["main_byol.py", "--dataset", "synthetic", "--sample_duration", "4", "--sample_size", "32", "--n_workers", "0",
          "--batch_size", "2", "--synthetic_len", "2", "--task", "loss_com", "--loss_weight", "0.1", "1", "1", "1", "1",
          "--n_epochs", "100", "--learning_rate", "0.005", "--weight_decay", "5e-4"] + model, 600)
    ckpt = os.path.join(res, "synthetic", "loss_com", "save_100.pth")
    assert os.path.isfile(ckpt)
    ks = [1, 5, 10]
    common = model + ["--pretrained_path", ckpt, "--transform_mode", "img_test", "--sample_size", "112", "--n_classes", "4",
                      "--retrieval_k", "10", "1", "5"]
    out = _run(["retrieval.py", "--dataset", "synthetic_video", "--sample_duration", "8", "--pb_rate", "2", "--synthetic_len", "32",
                "--retrieval_gallery_len", "12"] + common, 300)
    _check_result(os.path.join(res, "synthetic_video", "retrieval_r21d_byol1_synthetic_video_1_8.txt"), out, ks, 8, 12)
    videos = [(e, lab, n, 130, 150, g) for e, lab, n, _, _, g in VIDEOS]
    frame_dir, ann = write_tree(tmp_path / "data", videos)
    common[-3:] = ["5", "1", "2"]
    out = _run(["retrieval.py", "--dataset", "UcfFineTune", "--frame_dir", frame_dir, "--annotation_path", ann, "--split", "1",
                "--sample_duration", "4", "--pb_rate", "2", "--n_workers", "4"] + common, 300)
    _check_result(os.path.join(res, "UcfFineTune", "retrieval_r21d_byol1_UcfFineTune_1_4.txt"), out, [1, 2, 5], 3, 6)

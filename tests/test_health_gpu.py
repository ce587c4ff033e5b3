"""Label-free collapse metrics on the GPU: ops.feat_gram and ops.pair_potential (csrc/health.h) against fp64 on the fp32-rounded
input, symmetry and determinism in bits, the segment / split paths of pair_potential, no [n, n] tensor, both kernels between
poisoned guard bands; health.metrics end to end against tests/health_spec.py; health.evaluate on a model, the --health_every
monitor of main_byol.py in child processes.

THE BARS are not fixed in advance.  For every case the CPU fp32 ATen composition (x.T @ x; x @ x.T -> exp -> fp64 row sums) is
measured against the same fp64 truth and the bar is max(1e-6, 4 x that deviation): the project's 1e-6 op bar with the S3D-G / I3D
widening rule.  Every test prints the HIP error beside the fp32 one."""
import functools
import json
import math
import os
import re
import subprocess
import sys

import pytest
import torch

import guard_bands as gb
import health_spec as spec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
T = 2.0

# (n, d): the tiles are 64 rows x 128 gallery rows x 32 features (pair_potential) and 64 x 128 features x slabs of 32 rows
# (feat_gram); the shapes sit at their edges.  The last one spans 66 row slabs with a ragged last one (20 rows) and three parts
# of the column sums (1024 + 1024 + 52 rows).
SHAPES = [(1, 1), (2, 5), (63, 32), (64, 33), (65, 5), (129, 100), (200, 33), (300, 512), (2100, 40)]
# 34 gallery tiles -> 17 segments of 2 tiles; 67 row tiles -> by default 3 blocks per row tile, each walking 6 (the last 5) segments:
# several tiles per segment, several segments per block, several blocks per row tile, and the fold of 17 partials
SPLIT_SHAPE = (4229, 8)


def _bar(dev32):
    return max(1e-6, 4.0 * dev32)


@functools.lru_cache(maxsize=None)
def _raw(n, d):
    return spec.make_features(n, d, max(1, min(4, d)), 0.1, seed=1000 * n + d)


@functools.lru_cache(maxsize=None)
def _unit(n, d):
    """Rows normalised in fp64, rounded to fp32: the input of pair_potential, and what its truth is computed on."""
    return spec.normalize_ref(_raw(n, d)).to(torch.float32).contiguous()


def _rel(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _row_rel(got, ref):
    return float(((got.double() - ref).abs() / ref.abs().clamp_min(1e-30)).max())


def _rowsum32(x, t):
    """The fp32 ATen composition on the CPU: x @ x.T -> exp -> fp64 row sums without the diagonal."""
    e = torch.exp(2.0 * t * (x @ x.T - 1.0))
    e.fill_diagonal_(0.0)
    return e.double().sum(dim=1)


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- feat_gram ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", SHAPES)
def test_feat_gram_against_fp64(n, d):
    from cstp_amd import ops
    x = _raw(n, d)
    g_ref, s_ref = spec.gram_ref(x)
    dev_g, dev_s = _rel(x.T @ x, g_ref), _rel(x.sum(dim=0), s_ref)
    xd = x.to(DEV)
    gram, colsum = ops.feat_gram(xd)
    assert gram.dtype == torch.float64 and tuple(gram.shape) == (d, d) and colsum.dtype == torch.float64 and tuple(colsum.shape) == (d,)
    err_g, err_s = _rel(gram.cpu(), g_ref), _rel(colsum.cpu(), s_ref)
    print("feat_gram %dx%d: G rel_err HIP %.3e, fp32 ATen %.3e (bar %.1e); colsum HIP %.3e, fp32 ATen %.3e (bar %.1e)"
          % (n, d, err_g, dev_g, _bar(dev_g), err_s, dev_s, _bar(dev_s)))
    assert err_g < _bar(dev_g) and err_s < _bar(dev_s)
    assert _bits(gram, gram.T.contiguous()), "G differs from its transpose"
    gram2, colsum2 = ops.feat_gram(xd)
    assert _bits(gram, gram2) and _bits(colsum, colsum2)


def test_feat_gram_does_not_depend_on_alignment():
    """The scalar-load variant (x one element off a 16-byte boundary, d a multiple of 4) gives the bits of the vector one."""
    from cstp_amd import ops
    n, d = 129, 100
    x = _raw(n, d)
    flat = torch.empty(n * d + 1, dtype=torch.float32, device=DEV)
    off = flat[1:].view(n, d)
    off.copy_(x)
    assert off.data_ptr() % 16 == 4
    g0, s0 = ops.feat_gram(x.to(DEV))
    g1, s1 = ops.feat_gram(off)
    assert _bits(g0, g1) and _bits(s0, s1)
    r0, r1 = ops.pair_potential(x.to(DEV), T), ops.pair_potential(off, T)
    assert _bits(r0, r1)


# ---- pair_potential -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", SHAPES + [SPLIT_SHAPE])
def test_pair_potential_against_fp64(n, d):
    from cstp_amd import ops
    x = _unit(n, d)
    ref = spec.pair_potential_ref(x, T)
    dev32 = _row_rel(_rowsum32(x, T), ref)
    xd = x.to(DEV)
    rowsum = ops.pair_potential(xd, T)
    assert rowsum.dtype == torch.float64 and tuple(rowsum.shape) == (n,)
    err = _row_rel(rowsum.cpu(), ref)
    print("pair_potential %dx%d: worst row rel_err HIP %.3e, fp32 ATen %.3e (bar %.1e)" % (n, d, err, dev32, _bar(dev32)))
    assert err < _bar(dev32)
    assert _bits(rowsum, ops.pair_potential(xd, T))
    if n == 1:
        assert float(rowsum[0]) == 0.0                    # the only pair is the diagonal one


def _plan(n, override=None):
    """csrc/health.h pairpot_plan restated: (tiles per segment, segments, segments per block, blocks per row tile)."""
    gtiles = -(-n // 128)
    per = -(-gtiles // 32)
    nseg = -(-gtiles // per)
    ns = override if override is not None else 256 // -(-n // 64)
    ns = max(1, min(ns, nseg))
    spb = -(-nseg // ns)
    return per, nseg, spb, -(-nseg // spb)


def test_pair_potential_segments_and_splits_change_no_bit(monkeypatch):
    """SPLIT_SHAPE takes every path the implementation has: segments of several tiles, blocks that walk several segments, several
    blocks per row tile, the fold of the segment partials.  The workspace size proves the segment count; the grid split
    (CSTP_PAIRPOT_NSPLIT: one block per row tile, the default three, one block per segment) changes no bit."""
    from cstp_amd import _lib, ops
    n, d = SPLIT_SHAPE
    per, nseg, spb, nsplit = _plan(n)
    assert (per, nseg, spb, nsplit) == (2, 17, 6, 3)
    lib = _lib.load()
    assert lib.cstp_pair_potential_workspace_bytes(n, d) == nseg * n * 8 + 256          # the library's own segment count
    monkeypatch.delenv("CSTP_PAIRPOT_NSPLIT", raising=False)
    xd = _unit(n, d).to(DEV)
    base = ops.pair_potential(xd, T)
    for ns in (1, 2, 32):
        assert _plan(n, ns)[3] == {1: 1, 2: 2, 32: 17}[ns]
        monkeypatch.setenv("CSTP_PAIRPOT_NSPLIT", str(ns))
        assert _bits(base, ops.pair_potential(xd, T)), "the answer depends on the grid split %d" % ns
    monkeypatch.delenv("CSTP_PAIRPOT_NSPLIT")
    # segments of one tile (17 of them, by default dealt to 6 blocks per row tile) against one block per row tile
    n2, d2 = 2100, 40
    assert _plan(n2) == (1, 17, 3, 6) and _plan(n2, 1)[3] == 1
    x2 = _unit(n2, d2).to(DEV)
    split = ops.pair_potential(x2, T)
    monkeypatch.setenv("CSTP_PAIRPOT_NSPLIT", "1")
    assert _bits(split, ops.pair_potential(x2, T))


def test_pair_potential_special_rows():
    from cstp_amd import ops
    # two identical rows whose similarity is exactly 1: both sums are exp(0)
    two = torch.zeros(2, 8)
    two[:, :4] = 0.5
    assert ops.pair_potential(two.to(DEV), T).tolist() == [1.0, 1.0]
    # the diagonal is left out by index, not by value: a duplicate of row i counts for row i
    x = _unit(65, 33).clone()
    x[9] = x[4]
    x[:, 7] = 0.0                                         # a zero feature column
    x[3] = 0.0                                            # an all-zero row: s = 0 with every row
    ref = spec.pair_potential_ref(x, T)
    got = ops.pair_potential(x.to(DEV), T).cpu()
    dev32 = _row_rel(_rowsum32(x, T), ref)
    err = _row_rel(got, ref)
    print("pair_potential special rows: HIP %.3e, fp32 ATen %.3e" % (err, dev32))
    assert bool(torch.isfinite(got).all()) and err < _bar(dev32)
    assert float(got[3]) == pytest.approx(64 * math.exp(-2.0 * T), rel=1e-6)
    gram, colsum = ops.feat_gram(x.to(DEV))
    assert bool((gram[7] == 0).all()) and bool((gram[:, 7] == 0).all()) and float(colsum[7]) == 0.0
    # other temperatures
    for t in (0.5, 7.0):
        r = spec.pair_potential_ref(x, t)
        assert _row_rel(ops.pair_potential(x.to(DEV), t).cpu(), r) < _bar(_row_rel(_rowsum32(x, t), r))


def test_pair_potential_builds_no_n_by_n_tensor():
    from cstp_amd import ops
    n, d = 8192, 64
    x = _unit(n, d).to(DEV)
    ops.pair_potential(x[:256].contiguous(), T)           # the library is loaded and warm
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    rowsum = ops.pair_potential(x, T)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print("pair_potential %dx%d: peak rise %.2f MB (the matrix would be %.0f MB)" % (n, d, rise / 1e6, n * n * 4 / 1e6))
    assert rise < 32e6 and bool(torch.isfinite(rowsum).all())


# ---- guard bands ----------------------------------------------------------------------------------------------------------------
def _gram_spec(n, d, shift):
    from cstp_amd import _lib
    lib = _lib.load()
    x = _raw(n, d)
    g_ref, s_ref = spec.gram_ref(x)
    nbytes = lib.cstp_feat_gram_workspace_bytes(n, d)
    s = gb.Spec("feat_gram %dx%d shift %d" % (n, d, shift), {"x": x}, {"gram": ((d, d), torch.float64), "colsum": ((d,), torch.float64)},
                {"gram": gb.rel_check(g_ref, _bar(_rel(x.T @ x, g_ref))), "colsum": gb.rel_check(s_ref, _bar(_rel(x.sum(dim=0), s_ref)))},
                ws_bytes=nbytes, shifts={"x": shift})
    stream = torch.cuda.current_stream().cuda_stream

    def impl(v, n_arg=n, ws_bytes=nbytes):
        return lib.cstp_feat_gram(stream, v["x"].data_ptr(), n_arg, d, v["gram"].data_ptr(), v["colsum"].data_ptr(),
                                  v["ws"].data_ptr(), ws_bytes)
    return s, impl


def _pair_spec(n, d, shift):
    from cstp_amd import _lib
    lib = _lib.load()
    x = _unit(n, d)
    ref = spec.pair_potential_ref(x, T)
    bar = _bar(_row_rel(_rowsum32(x, T), ref))
    nbytes = lib.cstp_pair_potential_workspace_bytes(n, d)

    def check(got):
        err = _row_rel(got, ref)
        assert err < bar, "worst row relative error %.3e (bar %.1e)" % (err, bar)
    s = gb.Spec("pair_potential %dx%d shift %d" % (n, d, shift), {"x": x}, {"rowsum": ((n,), torch.float64)}, {"rowsum": check},
                ws_bytes=nbytes, shifts={"x": shift})
    stream = torch.cuda.current_stream().cuda_stream

    def impl(v, t=T, ws_bytes=nbytes):
        return lib.cstp_pair_potential(stream, v["x"].data_ptr(), n, d, t, v["rowsum"].data_ptr(), v["ws"].data_ptr(), ws_bytes)
    return s, impl


def _checked(impl):
    from cstp_amd import _lib

    def run(v):
        _lib.check(impl(v), "the guarded call")
    return run


@pytest.mark.parametrize("shift", [0, 4], ids=["x aligned", "x one element off"])
@pytest.mark.parametrize("n,d", [(65, 33), (129, 100)])
@pytest.mark.parametrize("make", [_gram_spec, _pair_spec], ids=["feat_gram", "pair_potential"])
def test_between_poisoned_guard_bands(make, n, d, shift):
    """Outputs fully written (their interior starts as NaN), nothing outside the outputs and the declared workspace bytes
    changed, the input unchanged, the answer independent of what surrounds the operands."""
    s, impl = make(n, d, shift)
    found = gb.three_runs(s, _checked(impl), DEV, torch.cuda.synchronize)
    assert found == [], "\n".join(found)


@pytest.mark.parametrize("make", [_gram_spec, _pair_spec], ids=["feat_gram", "pair_potential"])
def test_refused_calls_touch_nothing(make):
    s, impl = make(65, 33, 0)
    operands = gb.Operands(s, DEV)
    bad = [dict(ws_bytes=s.ws_bytes - 1)] + ([dict(n_arg=0)] if make is _gram_spec else [dict(t=0.0), dict(t=float("nan"))])
    for kw in bad:
        operands.arm("nan")
        rc = impl(operands.views(), **kw)
        torch.cuda.synchronize()
        assert rc != 0, kw
        assert operands.problems() == [], kw
        for g in list(operands.outs.values()) + [operands.ws]:
            assert bool((g.buf[g.lo:g.hi] == 0xFF).all()), "%s was written by a refused call (%r)" % (g.name, kw)


# ---- metrics end to end ---------------------------------------------------------------------------------------------------------
def _fp32_composition(feat, t):
    """The six figures from fp32 ATen sums on the CPU (fp32 normalisation, x.T @ x, x.sum(0), x @ x.T -> exp -> fp64 row sums,
    the best other cosine from the fp32 matrix), through the spec's fp64 host arithmetic."""
    n, d = feat.shape
    x = feat / feat.norm(dim=1, keepdim=True).clamp_min(1e-12)
    s = x @ x.T
    s.fill_diagonal_(float("-inf"))
    return spec.metrics_from_sums_ref((x.T @ x).double(), x.sum(dim=0).double(), _rowsum32(x, t), s.max(dim=1).values.double(), n, d, t)


@pytest.mark.parametrize("n,d,rank,noise", [(200, 33, 5, 0.05), (1100, 100, 12, 0.1), (129, 512, 40, 0.2), (64, 2048, 30, 0.3)])
def test_metrics_against_the_specification(n, d, rank, noise):
    from cstp_amd import health, ops
    feat = spec.make_features(n, d, rank, noise, seed=n + d)
    want = spec.metrics_ref(feat, T)
    comp = _fp32_composition(feat, T)
    res = health.metrics(feat.to(DEV), T)
    assert (res["n"], res["d"], res["t"]) == (n, d, T) and set(res) == set(health.KEYS) | {"n", "d", "t"}
    for key in health.KEYS:
        rel = lambda v: abs(v - want[key]) / max(abs(want[key]), 1e-30)      # noqa: E731
        err, dev32 = rel(res[key]), rel(comp[key])
        print("metrics %dx%d %-10s = %+.9f (spec %+.9f): rel_err HIP %.3e, fp32 ATen %.3e (bar %.1e)"
              % (n, d, key, res[key], want[key], err, dev32, _bar(dev32)))
        assert math.isfinite(res[key])
        if key == "rankme" and n < d:                    # ill-conditioned there (cstp_amd/health.py): finite and in range only
            assert 1.0 <= res[key] <= min(n, d) + 1
        else:
            assert err < _bar(dev32), key
    val, _ = ops.sim_topk(ops.l2_normalize(feat.to(DEV)), ops.l2_normalize(feat.to(DEV)), 1, True)
    assert res["nn_sim"] == float(val[:, 0].to("cpu", torch.float64).mean())


def test_metrics_known_answers_through_the_kernels():
    from cstp_amd import health
    res = health.metrics(spec.one_hot_rows().to(DEV), T)
    p = torch.tensor([0.125 + 1e-7] * 8 + [1e-7] * 32, dtype=torch.float64)
    exact = {"erank": 7.0, "top1_share": 1.0 / 7.0, "rankme": math.exp(-float((p * p.log()).sum())),
             "std_ratio": math.sqrt(40) * 8 * math.sqrt(7.0 / 64.0) / 40, "nn_sim": 1.0,
             "uniformity": math.log((11 + 84 * math.exp(-4.0)) / 95)}
    for key, want in exact.items():
        assert res[key] == pytest.approx(want, abs=1e-6), key
        if key in spec.ONE_HOT_ANSWERS:
            assert want == pytest.approx(spec.ONE_HOT_ANSWERS[key], abs=5e-5)
    res = health.metrics(spec.collapsed_rows().to(DEV), T)
    for key, want in spec.COLLAPSED_ANSWERS.items():
        assert res[key] == pytest.approx(want, abs=1e-6), key
    assert res["rankme"] == pytest.approx(1.0, abs=1e-4) and res["nn_sim"] == pytest.approx(1.0, abs=1e-6)
    with pytest.raises(ValueError, match="at least 2 rows"):
        health.metrics(torch.ones(1, 4, device=DEV))


# ---- model level ----------------------------------------------------------------------------------------------------------------
def test_evaluate_on_synthetic_videos():
    """R(2+1)D depth 1 on 10 short synthetic videos (the clip of test_knn_gpu.py's monitor test): finite figures, an effective
    rank between 1 and min(n - 1, d), the model handed back in the mode it came in, labels ignored."""
    from cstp_amd import health, retrieval
    from cstp_amd.clip_ops import GpuLabelledLoader, GpuLabelledVideos
    from cstp_amd.r21d_byol import R21DBYOL
    torch.manual_seed(0)
    kw = dict(n_classes=4, height=60, width=80, sample_duration=4, sample_size=112, pb_rate=2)
    loader = GpuLabelledLoader(GpuLabelledVideos(DEV, "test", "img_test", n_videos=10, seed=1, **kw))
    model = R21DBYOL(pretrain=True, layer_sizes=(1, 1, 1, 1)).cuda()
    model.train()
    modes = {n: m.training for n, m in model.named_modules()}
    before = {n: b.clone() for n, b in model.named_buffers()}
    res = health.evaluate(model, loader, T)
    assert {n: m.training for n, m in model.named_modules()} == modes
    assert all(torch.equal(b, before[n]) for n, b in model.named_buffers())
    assert res["n"] == 10 and res["d"] == 512 and res["t"] == T
    assert all(math.isfinite(res[k]) for k in health.KEYS), res
    assert 1.0 <= res["erank"] <= min(res["n"] - 1, res["d"])
    assert 0.0 <= res["top1_share"] <= 1.0 and res["uniformity"] <= 1e-6 and -1.0 <= res["nn_sim"] <= 1.0 + 1e-6
    feat, _ = retrieval.extract_features(model, loader)
    model.train()
    assert health.metrics(feat, T) == res
    print("health.evaluate: " + health.format_line(res))


def _run(args, timeout, **extra_env):
    env = dict(os.environ, **extra_env)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args[0], r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_monitor_prints_writes_and_leaves_the_run_alone(tmp_path):
    """One epoch of two steps with --health_every 1, then without the flag, each in a fresh child process of a few seconds
    (CSTP_DETERMINISTIC=1 and CSTP_AUTOTUNE=0 make the two runs repeat each other, as in test_knn_gpu.py): the ``Health epoch``
    line and one JSON line in health.jsonl against no such line and no file, and every other output line the same -- the
    options dump included, but for the path of the result folder and the timing columns."""
    common = ["main_byol.py", "--dataset", "synthetic_video", "--model_name", "r21d_byol", "--model_depth", "1",
              "--sample_duration", "4", "--sample_size", "112", "--batch_size", "2", "--synthetic_len", "8",
              "--retrieval_gallery_len", "8", "--n_classes", "4", "--n_epochs", "1", "--max_steps", "2", "--task", "loss_com",
              "--loss_weight", "0.1", "1", "1", "1", "1", "--learning_rate", "0.005", "--weight_decay", "5e-4"]
    outs, logs = {}, {}
    for tag, extra in (("on", ["--health_every", "1"]), ("off", [])):
        res = str(tmp_path / "res")
        outs[tag] = _run(common + ["--result_path", res] + extra, 120, CSTP_DETERMINISTIC="1", CSTP_AUTOTUNE="0")
        folder = os.path.join(res, "synthetic_video", "loss_com")
        logs[tag] = open(os.path.join(folder, "synthetic_video_train_clip4modelr21d_byol1.log")).read()
        path = os.path.join(folder, "health.jsonl")
        if tag == "on":
            lines = [ln for ln in open(path).read().split("\n") if ln]
            assert len(lines) == 1
            rec = json.loads(lines[0])
            assert rec["epoch"] == 1 and rec["n"] == 2 and rec["d"] == 512 and rec["t"] == 2.0
            assert all(math.isfinite(rec[k]) for k in ("std_ratio", "erank", "rankme", "top1_share", "uniformity", "nn_sim"))
            shown = [ln for ln in outs[tag].split("\n") if ln.startswith("Health epoch 1: std_ratio = ")]
            assert len(shown) == 1 and "erank = %.4f" % rec["erank"] in shown[0] and "nn_sim = %.4f" % rec["nn_sim"] in shown[0]
            assert "Health monitor: 2 videos, t = 2.0" in outs[tag]
            os.remove(path)
        else:
            assert not os.path.exists(path) and "Health" not in outs[tag]

    def stable(out):
        keep = []
        for ln in out.split("\n"):
            if ln.startswith("Health"):
                continue
            if ln.startswith("Epoch: ["):                # Time / Data columns are wall-clock readings
                ln = "\t".join(c for c in ln.split("\t") if not c.startswith(("Time ", "Data ")))
            keep.append(ln)
        return keep
    dump = re.sub(r"(, )?health_every=1(, )?", lambda m: ", " if m.group(1) and m.group(2) else "", outs["on"])
    assert stable(dump) == stable(outs["off"])
    assert "health_every" not in outs["off"] and "health_t" not in outs["off"]
    assert logs["on"] == logs["off"]                     # the epoch log: the same columns and the same values


def test_health_driver_on_a_fresh_checkpoint(tmp_path):
    """health.py in a child process on a checkpoint written from an untrained depth-1 R(2+1)D (no training run: the driver only
    needs the encoder's tensors): the two ``Health`` lines, the JSON line, the result file."""
    from cstp_amd.r21d_byol import R21DBYOL
    torch.manual_seed(0)
    model = R21DBYOL(pretrain=True, layer_sizes=(1, 1, 1, 1))
    ckpt = str(tmp_path / "fresh.pth")
    torch.save({"epoch": 1, "arch": "r21d_byol-1", "state_dict": {"module." + k: v for k, v in model.state_dict().items()}}, ckpt)
    res = str(tmp_path / "res")
    out = _run(["health.py", "--dataset", "synthetic_video", "--transform_mode", "img_test", "--model_name", "r21d_byol",
                "--model_depth", "1", "--pretrained_path", ckpt, "--result_path", res, "--sample_duration", "4", "--pb_rate", "2",
                "--sample_size", "112", "--n_classes", "4", "--synthetic_len", "16", "--retrieval_gallery_len", "6",
                "--health_t", "1.5"], 120)
    lines = out.split("\n")
    summary = json.loads([ln for ln in lines if ln.startswith("{")][-1])
    assert summary["task"] == "health" and summary["arch"] == "r21d_byol-1" and summary["t"] == 1.5
    for part, n in (("train", 6), ("test", 4)):
        rec = summary[part]
        assert rec["n"] == n and rec["d"] == 512 and rec["t"] == 1.5
        assert all(math.isfinite(rec[k]) for k in ("std_ratio", "erank", "rankme", "top1_share", "uniformity", "nn_sim"))
        shown = [ln for ln in lines if ln.startswith("Health %s: std_ratio = %.4f" % (part, rec["std_ratio"]))]
        assert len(shown) == 1 and "erank = %.4f" % rec["erank"] in shown[0]
    saved = open(os.path.join(res, "synthetic_video", "health_r21d_byol1_synthetic_video_1_4.txt")).read().split("\n")
    assert json.loads([ln for ln in saved if ln.startswith("{")][-1]) == summary

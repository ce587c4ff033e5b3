"""k-means clustering evaluation, the parts that need no GPU: the three flags, cluster.plan and cluster.init_pp, the metrics on the
contingency table (hand-computed answers, invariances, brute force, scipy / scikit-learn where installed), the near-tie share and
the restatement error of every GPU case from tests/cluster_spec.py alone, the fp64 spec on the separable data of the GPU fit
test, the refusals of the driver, of ops.kmeans_assign / ops.kmeans_update and of the C ABI (declared, bound, exported, refusing
bad arguments before any HIP call), and the workspace formula."""
import ctypes
import itertools
import math
import os

import numpy as np
import pytest
import torch

from cluster_spec import (CASES, MAX_NEAR_TIE_SHARE, assign_ref, fit_ref, make_case, restatement_error, spec_assignment, update_bound,
                          update_ref, update_restated_fp32)
from probe_spec import make_clusters
from test_abi import header_symbols

# tests/test_cluster_gpu.py fits these: 300 x 24 features in 10 classes whose centres lie 12 standard deviations apart
FIT_DATA = dict(n=300, d=24, c=10, sep=12.0)
FIT_ARGS = dict(k=10, iters=12, restarts=4, seed=3)


def test_opts_carry_the_cluster_flags():
    from cstp_amd import opts as opts_mod
    from cstp_amd.opts import parse_opts
    d = parse_opts([])
    assert (d.cluster_k, d.cluster_iters, d.cluster_restarts) == (0, 50, 10)
    o = parse_opts(["--cluster_k", "7", "--cluster_iters", "1", "--cluster_restarts", "32"])
    assert (o.cluster_k, o.cluster_iters, o.cluster_restarts) == (7, 1, 32)
    for bad in (["--cluster_k", "-1"], ["--cluster_k", "x"], ["--cluster_iters", "0"], ["--cluster_iters", "-3"],
                ["--cluster_restarts", "0"], ["--cluster_restarts", "33"], ["--cluster_restarts", "2.5"]):
        with pytest.raises(SystemExit):
            parse_opts(bad)
    for flag in ("--cluster_k", "--cluster_iters", "--cluster_restarts"):
        assert flag in opts_mod.__doc__
    helps = {a.dest: a.help for a in opts_mod.build_parser()._actions}
    assert "not tuned on real data" in helps["cluster_iters"] and "not tuned on real data" in helps["cluster_restarts"]


def test_plan_is_a_pure_function_of_its_arguments():
    from cstp_amd.cluster import plan
    torch.manual_seed(5)
    u = plan(300, 10, 4, 3)
    torch.manual_seed(6)                                     # the global generator plays no part
    assert torch.equal(u, plan(300, 10, 4, 3))
    assert u.dtype == torch.float64 and tuple(u.shape) == (4, 10) and u.device.type == "cpu"
    assert float(u.min()) >= 0.0 and float(u.max()) < 1.0
    assert not torch.equal(u, plan(300, 10, 4, 4)) and not torch.equal(u[0], u[1])
    assert torch.equal(plan(300, 10, 2, 3), u[:2])           # restart s is seeded by (seed, s) alone
    for bad in ((0, 1, 1), (5, 6, 1), (5, 0, 1), (5, 2, 0), (5, 2, 33)):
        with pytest.raises(ValueError):
            plan(bad[0], bad[1], bad[2], 0)


def test_init_pp_picks_rows_of_x_spread_over_the_clusters():
    from cstp_amd.cluster import init_pp, plan
    feat, lab = make_clusters(FIT_DATA["n"], FIT_DATA["d"], FIT_DATA["c"], FIT_DATA["sep"])
    x = torch.nn.functional.normalize(feat, dim=1)
    u = plan(300, 10, 4, 3)
    state = torch.random.get_rng_state()
    cent = init_pp(x, u)
    assert torch.equal(torch.random.get_rng_state(), state)  # no draw from the global generator
    assert torch.equal(cent, init_pp(x, u)) and tuple(cent.shape) == (4, 10, 24) and cent.dtype == torch.float32
    for s in range(4):
        rows = [int((x == cent[s, j]).all(dim=1).nonzero()[0, 0]) for j in range(10)]        # every centre is a row of x
        assert rows[0] == min(int(float(u[s, 0]) * 300), 299)
        assert len(set(rows)) == 10
    # a row that coincides with a centre has weight 0 and is never drawn again, even with u = 0 and u -> 1
    edge = init_pp(x[:7], torch.tensor([[0.0] * 7, [1.0 - 2.0 ** -53] * 7], dtype=torch.float64))
    for s in range(2):
        assert len({tuple(row.tolist()) for row in edge[s]}) == 7


# ---- the metrics ------------------------------------------------------------------------------------------------------------
def test_metrics_known_answers():
    from cstp_amd import cluster
    same = np.diag([4, 3, 5])                               # identical partitions
    for fn in (cluster.nmi, cluster.ari, cluster.purity, cluster.matched_accuracy):
        assert fn(same) == pytest.approx(1.0, abs=1e-15)
    indep = np.array([[2, 4], [3, 6]])                      # n_ij = a_i b_j / n: independent
    assert cluster.nmi(indep) == pytest.approx(0.0, abs=1e-15)
    # ARI by hand: sum C(n_ij, 2) = 1 + 6 + 3 + 15 = 25, rows C(6,2) + C(9,2) = 51, cols C(5,2) + C(10,2) = 55, all C(15,2) = 105
    assert cluster.ari(indep) == pytest.approx((25 - 51 * 55 / 105) / (0.5 * (51 + 55) - 51 * 55 / 105), rel=1e-14)
    assert cluster.purity(indep) == pytest.approx(10 / 15) and cluster.matched_accuracy(indep) == pytest.approx(8 / 15)
    # the worked example: clusters x classes, n = 17 (Manning, Raghavan & Schuetze, Introduction to IR, fig. 16.4)
    t = np.array([[5, 1, 0], [1, 4, 1], [2, 0, 3]])
    assert cluster.purity(t) == pytest.approx(12 / 17)
    assert cluster.matched_accuracy(t) == pytest.approx(12 / 17)
    n = 17.0
    a, b = t.sum(axis=1), t.sum(axis=0)
    mi = sum(t[i, j] / n * math.log(n * t[i, j] / (a[i] * b[j])) for i in range(3) for j in range(3) if t[i, j])
    h = lambda v: -sum(p / n * math.log(p / n) for p in v)
    assert cluster.nmi(t) == pytest.approx(mi / (0.5 * (h(a) + h(b))), rel=1e-13)
    assert cluster.nmi(t) == pytest.approx(0.36, abs=0.005)                       # the book's figure
    # pairs: TP = 20 (same cluster, same class), TP + FP = 40, TP + FN = C(8,2) + C(5,2) + C(4,2) = 44, all = 136
    assert cluster.ari(t) == pytest.approx((20 - 40 * 44 / 136) / (0.5 * (40 + 44) - 40 * 44 / 136), rel=1e-14)
    one = np.array([[9]])                                   # both partitions a single cluster
    assert cluster.nmi(one) == 1.0 and cluster.ari(one) == 1.0 and cluster.purity(one) == 1.0
    assert cluster.nmi(np.array([[3, 3]])) == 0.0           # one cluster against two classes: no information
    for bad in (np.zeros((0, 3)), np.array([1, 2]), np.array([[1, -1]])):
        with pytest.raises(ValueError):
            cluster.nmi(bad)


def test_metrics_do_not_depend_on_the_cluster_ids():
    from cstp_amd import cluster
    rs = np.random.RandomState(0)
    t = rs.randint(0, 9, size=(6, 4))
    for fn in (cluster.nmi, cluster.ari, cluster.purity, cluster.matched_accuracy):
        base = fn(t)
        for _ in range(5):
            assert fn(t[rs.permutation(6)]) == pytest.approx(base, rel=1e-13, abs=1e-15)
        assert fn(t[:, rs.permutation(4)]) == pytest.approx(base, rel=1e-13, abs=1e-15)
    assert cluster.nmi(t.T) == pytest.approx(cluster.nmi(t), rel=1e-13) and cluster.ari(t.T) == pytest.approx(cluster.ari(t), rel=1e-13)
    assert cluster.nmi(torch.from_numpy(t)) == cluster.nmi(t)


def _brute(cost):
    n, m = cost.shape
    if n > m:
        return _brute(cost.T)
    return min(sum(cost[i, p[i]] for i in range(n)) for p in itertools.permutations(range(m), n))


def test_hungarian_against_brute_force():
    from cstp_amd.cluster import hungarian
    rs = np.random.RandomState(1)
    shapes = [(k, k) for k in range(1, 7)] + [(2, 5), (5, 2), (1, 6), (6, 1), (3, 6), (6, 4)]
    for n, m in shapes:
        for trial in range(6):
            cost = rs.randint(-6, 7, size=(n, m)).astype(np.float64) if trial % 2 else rs.standard_normal((n, m))
            rows, cols = hungarian(cost)
            assert rows.tolist() == sorted(rows.tolist()) and len(rows) == min(n, m)
            assert len(set(rows.tolist())) == len(rows) and len(set(cols.tolist())) == len(cols)
            assert 0 <= rows.min() and rows.max() < n and 0 <= cols.min() and cols.max() < m
            assert cost[rows, cols].sum() == pytest.approx(_brute(cost), rel=1e-12, abs=1e-12)
    for bad in (np.zeros((0, 2)), np.zeros(3), np.array([[np.nan]])):
        with pytest.raises(ValueError):
            hungarian(bad)


def test_metrics_against_scipy_and_sklearn():
    opt = pytest.importorskip("scipy.optimize")
    metrics = pytest.importorskip("sklearn.metrics")
    from cstp_amd import cluster
    rs = np.random.RandomState(2)
    for n, m in [(5, 5), (12, 12), (30, 30), (7, 11), (11, 7), (101, 101)]:
        cost = rs.standard_normal((n, m))
        rows, cols = cluster.hungarian(cost)
        r2, c2 = opt.linear_sum_assignment(cost)
        assert cost[rows, cols].sum() == pytest.approx(cost[r2, c2].sum(), rel=1e-12)
    for k, classes, n in [(3, 3, 50), (10, 7, 400), (4, 9, 123), (1, 5, 40), (6, 1, 40)]:
        pred, lab = rs.randint(0, k, size=n), rs.randint(0, classes, size=n)
        t = cluster.contingency(torch.from_numpy(pred), torch.from_numpy(lab), k, classes)
        assert cluster.nmi(t) == pytest.approx(metrics.normalized_mutual_info_score(lab, pred), rel=1e-10, abs=1e-12)
        assert cluster.ari(t) == pytest.approx(metrics.adjusted_rand_score(lab, pred), rel=1e-10, abs=1e-12)


def test_contingency_counts_exactly_and_drops_out_of_range_rows():
    from cstp_amd.cluster import contingency
    pred = torch.tensor([0, 2, 2, 1, 5, -1, 2], dtype=torch.int32)
    lab = torch.tensor([1, 0, 0, 3, 0, 0, 4], dtype=torch.int64)
    t = contingency(pred, lab, 3, 4)
    assert t.dtype == torch.int64 and t.tolist() == [[0, 1, 0, 0], [0, 0, 0, 1], [2, 0, 0, 0]]
    with pytest.raises(ValueError):
        contingency(pred, lab[:3], 3, 4)


# ---- the GPU cases, from the spec alone -------------------------------------------------------------------------------------
def test_near_tie_share_of_every_gpu_case_is_under_the_cap():
    for shape in CASES:
        case = make_case(*shape)
        ref = assign_ref(case["x"], case["cent"])
        assert ref["near"].mean() <= MAX_NEAR_TIE_SHARE, (shape, ref["near"].mean())
        assert (ref["assign"] >= 0).all() and (ref["assign"] < shape[2]).all()
        assert ((case["prev"] != ref["assign"]).sum(axis=1) == -(-shape[0] // 3)).all()


def test_update_restatement_error_sets_the_gpu_bound():
    """The fp32 restatement of the kernel's documented order against the fp64 spec on the GPU cases: its largest error is what
    tests/test_cluster_gpu.py multiplies by 4.  Unit rows summed in fp32: the error must sit at a few ulps of 1."""
    err = restatement_error()
    print("update restatement error %.3g, GPU bound %.3g" % (err, update_bound()))
    assert 2.0 ** -26 < err < 64 * 2.0 ** -24 and update_bound() == 4 * err
    case = make_case(*CASES[1])
    a = spec_assignment(case).copy()
    a[0, :5] = (-1, 3, 1 << 20, -7, 3)                      # out-of-range values belong to no cluster, in both statements
    ref, counts = update_ref(case["x"], a, case["cent"])
    assert counts[0].sum() == 60 and counts[1].sum() == 65
    assert np.abs(update_restated_fp32(case["x"], a, case["cent"]).astype(np.float64) - ref).max() <= err
    a[1, :] = 2                                             # clusters 0 and 1 of restart 1 are empty: they keep their centroid
    ref, counts = update_ref(case["x"], a, case["cent"])
    assert counts[1].tolist() == [0, 0, 65] and np.array_equal(ref[1, :2], case["cent"][1, :2].astype(np.float64))


def test_spec_separates_the_fit_data_with_the_gpu_tests_seeds():
    """The data and the seeds of the GPU fit test: the fp64 spec, seeded by init_pp on the CPU, reaches NMI = accuracy = 1 and
    a fixed point well before the last iteration."""
    from cstp_amd import cluster
    feat, lab = make_clusters(FIT_DATA["n"], FIT_DATA["d"], FIT_DATA["c"], FIT_DATA["sep"])
    x = torch.nn.functional.normalize(feat, dim=1)
    init = cluster.init_pp(x, cluster.plan(300, FIT_ARGS["k"], FIT_ARGS["restarts"], FIT_ARGS["seed"]))
    ref = fit_ref(x.numpy(), init.numpy(), FIT_ARGS["iters"])
    t = cluster.contingency(torch.from_numpy(ref["assign"][ref["win"]]), lab, 10, 10)
    assert cluster.nmi(t) == pytest.approx(1.0, abs=1e-12) and cluster.matched_accuracy(t) == 1.0
    assert cluster.ari(t) == pytest.approx(1.0, abs=1e-12) and cluster.purity(t) == 1.0
    first = int(np.argmax(ref["moved"][:, ref["win"]] == 0))
    assert ref["moved"][first, ref["win"]] == 0 and first < FIT_ARGS["iters"] - 2
    assert (ref["moved"][FIT_ARGS["iters"] - 3:] == 0).all()                      # every restart, not only the winner
    # far from a near tie: the winner's rows choose their centroid by a margin the fp32 kernels cannot flip
    last = assign_ref(x.numpy(), ref["cent"][ref["win"]][None])
    assert last["gap"].min() > 1e-3


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_cluster_driver_names_its_datasets():
    import cluster as driver
    from cstp_amd.opts import parse_opts
    for name in ("Kin400RepreLMDB", "synthetic", "UcfRepreBYOLSpPre"):
        with pytest.raises(NotImplementedError, match="synthetic_video and UcfFineTune"):
            driver.run(parse_opts(["--dataset", name, "--transform_mode", "img_test"]))
    with pytest.raises(ValueError, match="img_test"):
        driver.run(parse_opts(["--dataset", "synthetic_video", "--transform_mode", "img"]))
    with pytest.raises(ValueError, match="img_test"):
        driver.build_sets(parse_opts(["--dataset", "UcfFineTune", "--transform_mode", "img"]))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            driver.run(parse_opts(["--dataset", "synthetic_video", "--transform_mode", "img_test"]))


def test_fit_refuses_bad_arguments_before_any_device_work():
    from cstp_amd import cluster
    feat = torch.zeros(8, 4)
    for kw in (dict(k=0), dict(k=9), dict(k=2, iters=0), dict(k=2, restarts=0), dict(k=2, restarts=33)):
        with pytest.raises(ValueError):
            cluster.fit(feat, **kw)
    with pytest.raises(ValueError):
        cluster.fit(feat[0], 2)


def test_kmeans_ops_refusals_on_cpu_tensors():
    from cstp_amd import ops
    from cstp_amd._lib import CstpError
    x, cent = torch.zeros(6, 4), torch.zeros(2, 3, 4)
    a = torch.zeros(2, 6, dtype=torch.int32)
    for call in (lambda **kw: ops.kmeans_assign(kw.pop("x", x), kw.pop("cent", cent), **kw),
                 lambda **kw: ops.kmeans_update(kw.pop("x", x), kw.pop("assign", a), kw.pop("cent", cent))):
        with pytest.raises(CstpError, match="HIP device"):
            call()
        with pytest.raises(CstpError, match="x must be float32"):
            call(x=x.double())
        with pytest.raises(CstpError, match="cent must be float32"):
            call(cent=cent.double())
        with pytest.raises(CstpError, match="x must be"):
            call(x=x[0])
        with pytest.raises(CstpError, match="cent must be"):
            call(cent=cent[0])
        with pytest.raises(CstpError, match="cent must be"):
            call(cent=torch.zeros(2, 3, 5))
        with pytest.raises(CstpError, match="empty"):
            call(x=x[:0])
        with pytest.raises(CstpError, match="empty"):
            call(cent=cent[:, :0])
        with pytest.raises(CstpError, match="must not exceed the rows"):
            call(cent=torch.zeros(2, 7, 4))
        with pytest.raises(CstpError, match="restarts are served"):
            call(cent=torch.zeros(33, 3, 4))
        with pytest.raises(CstpError, match="features"):
            call(x=torch.zeros(6, 4097), cent=torch.zeros(2, 3, 4097))
    with pytest.raises(CstpError, match="prev must be int32"):
        ops.kmeans_assign(x, cent, a.to(torch.int64))
    with pytest.raises(CstpError, match="prev must be \\[2, 6\\]"):
        ops.kmeans_assign(x, cent, a[:1])
    with pytest.raises(CstpError, match="assign must be int32"):
        ops.kmeans_update(x, a.to(torch.int64), cent)
    with pytest.raises(CstpError, match="assign must be \\[2, 6\\]"):
        ops.kmeans_update(x, a[:, :5], cent)


KMEANS_SYMBOLS = ("cstp_kmeans_workspace_bytes", "cstp_kmeans_assign", "cstp_kmeans_update")


def test_kmeans_entry_points_are_declared_bound_and_exported():
    from cstp_amd import _lib
    for name in KMEANS_SYMBOLS:
        assert name in header_symbols() and name in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 18                       # pure additions
    assert "#define CSTP_ABI_VERSION 18" in open(os.path.join(os.path.dirname(_lib._HERE), "include", "cstp_hip.h")).read()
    lib = _lib.load()
    for name in KMEANS_SYMBOLS:
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert lib.cstp_abi_version() == 18


def test_kmeans_workspace_bytes_follows_the_documented_formula():
    from cstp_amd import _lib
    lib = _lib.load()
    r16 = lambda v: -(-v // 16) * 16
    for n, d, c, r in CASES + [(9537, 512, 101, 10), (65536, 512, 400, 4), (1 << 24, 4096, 4096, 32), (64, 1, 64, 3), (129, 5, 1, 1)]:
        parts = r * -(-n // 64)
        assert lib.cstp_kmeans_workspace_bytes(n, d, c, r) == r16(8 * parts) + r16(4 * parts), (n, d, c, r)
    for bad in [(0, 8, 1, 1), (-1, 8, 1, 1), ((1 << 24) + 1, 8, 2, 1), (8, 0, 2, 1), (8, 4097, 2, 1), (8, 8, 0, 1), (8, 8, 9, 1),
                (5000, 8, 4097, 1), (8, 8, 2, 0), (8, 8, 2, 33)]:
        assert lib.cstp_kmeans_workspace_bytes(*bad) == 0, bad


def test_kmeans_entry_points_refuse_bad_arguments_before_any_hip_call():
    from cstp_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p                                              # never dereferenced: the checks fail first
    names = ("stream", "x", "cent", "prev", "n", "d", "c", "r", "assign", "best", "moved", "score", "ws", "ws_bytes")
    need = lib.cstp_kmeans_workspace_bytes(100, 16, 10, 2)
    good = [None, P(1 << 20), P(2 << 20), None, 100, 16, 10, 2, P(3 << 20), P(4 << 20), P(5 << 20), P(6 << 20), P(1 << 30), need]

    def assign(**kw):
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        return lib.cstp_kmeans_assign(*args), lib.cstp_last_error()

    cases = [(dict(x=None), b"null argument"), (dict(cent=None), b"null argument"), (dict(assign=None), b"null argument"),
             (dict(best=None), b"null argument"), (dict(moved=None), b"null argument"), (dict(score=None), b"null argument"),
             (dict(ws=None), b"null argument"),
             (dict(n=0), b"n must be in"), (dict(n=-5), b"n must be in"), (dict(n=(1 << 24) + 1), b"n must be in"),
             (dict(c=101), b"c must not exceed n"), (dict(c=0), b"c must be in"), (dict(c=4097, n=5000), b"c must be in"),
             (dict(r=33), b"r must be in 1..32"), (dict(r=0), b"r must be in 1..32"),
             (dict(d=4097), b"d must be in 1..4096"), (dict(d=0), b"d must be in 1..4096"),
             (dict(prev=P(3 << 20)), b"must not alias"), (dict(prev=P((3 << 20) + 796)), b"must not alias"),
             (dict(ws=P((1 << 30) + 8)), b"16-byte aligned"),
             (dict(ws_bytes=need - 1), b"workspace too small"), (dict(ws_bytes=0), b"workspace too small"),
             (dict(n=200), b"workspace too small")]
    for kw, needle in cases:
        rc, msg = assign(**kw)
        assert rc != 0 and needle in msg and b"line" in msg, (kw, rc, msg)

    unames = ("stream", "x", "assign", "cent_in", "n", "d", "c", "r", "cent_out", "counts")
    ugood = [None, P(1 << 20), P(2 << 20), P(3 << 20), 100, 16, 10, 2, P(4 << 20), P(5 << 20)]

    def update(**kw):
        args = list(ugood)
        for k, v in kw.items():
            args[unames.index(k)] = v
        return lib.cstp_kmeans_update(*args), lib.cstp_last_error()

    cb = 2 * 10 * 16 * 4
    ucases = [(dict(x=None), b"null argument"), (dict(assign=None), b"null argument"), (dict(cent_in=None), b"null argument"),
              (dict(cent_out=None), b"null argument"), (dict(counts=None), b"null argument"),
              (dict(n=0), b"n must be in"), (dict(c=101), b"c must not exceed n"), (dict(r=33), b"r must be in 1..32"),
              (dict(d=4097), b"d must be in 1..4096"), (dict(c=0), b"c must be in"),
              (dict(cent_out=P(3 << 20)), b"must not alias"), (dict(cent_out=P((3 << 20) + cb - 4)), b"must not alias"),
              (dict(cent_out=P((3 << 20) - cb + 4)), b"must not alias")]
    for kw, needle in ucases:
        rc, msg = update(**kw)
        assert rc != 0 and needle in msg and b"line" in msg, (kw, rc, msg)

"""Weighted k-NN classification, the parts that need no GPU: the fp64 specification tests/knn_spec.vote_ref on hand-computed rows,
knn.accuracy on hand-made predictions, the three new flags, the refusals of the --knn_every monitor and of the knn.py driver before
any device work, the refusals of ops.knn_vote, and the C ABI of the vote (declared, bound, exported, refusing bad arguments
before any HIP call)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from knn_spec import RTOL, vote_ref
from test_abi import header_symbols

NEG = float("-inf")


def test_vote_ref_on_hand_computed_rows():
    # k = 3, labels (2, 2, 5), values (0.9, 0.8, 0.85) at T = 0.1: w = (1, e^-1, e^-0.5)
    g_labels = [2, 9, 2, 5]
    pred, score, near = vote_ref([[0.9, 0.8, 0.85]], [[0, 2, 3]], g_labels, 10.0, 5)
    assert pred.tolist() == [[2, 5, -1, -1, -1]]
    assert score[0, 0] == pytest.approx(1.0 + math.exp(-1.0), rel=1e-12, abs=0)
    assert score[0, 1] == pytest.approx(math.exp(-0.5), rel=1e-12, abs=0)
    assert score[0, 2:].tolist() == [0.0, 0.0, 0.0] and not near.any()
    # n_top cuts the list; the answer is the head of the longer one
    p1, s1, _ = vote_ref([[0.9, 0.8, 0.85]], [[0, 2, 3]], g_labels, 10.0, 1)
    assert p1.tolist() == [[2]] and s1[0, 0] == score[0, 0]
    # the all-dead row, and dead slots beside live ones: -1 and an index >= ng weigh nothing
    pred, score, near = vote_ref([[NEG, NEG, NEG], [0.5, 0.4, NEG]], [[-1, -1, -1], [1, 4, -1]], g_labels, 10.0, 3)
    assert pred.tolist() == [[-1, -1, -1], [9, -1, -1]] and score.tolist() == [[0.0] * 3, [1.0, 0.0, 0.0]] and not near.any()
    # the one-class row: every slot votes for class 2
    pred, score, near = vote_ref([[0.7, 0.6]], [[2, 0]], g_labels, 1.0, 2)
    assert pred.tolist() == [[2, -1]] and score[0, 0] == pytest.approx(1.0 + math.exp(-0.1), rel=1e-12, abs=0)
    # equal scores: the lower class id first, and both ranks are marked near ties; a third class far away is not
    pred, score, near = vote_ref([[0.5, 0.5, 0.1]], [[3, 1, 0]], g_labels, 10.0, 3)
    assert pred.tolist() == [[5, 9, 2]] and score[0, 0] == score[0, 1] == 1.0
    assert near.tolist() == [[True, True, False]]
    # a near tie with the first rank that is cut off still marks the last rank kept
    _, _, near = vote_ref([[0.5, 0.5 - 1e-6]], [[3, 1]], g_labels, 1.0, 1)
    assert near.tolist() == [[True]]
    # no overflow at a temperature that would overflow exp(val / T): the largest weight is 1
    pred, score, _ = vote_ref([[30.0, 29.0]], [[0, 1]], g_labels, 1000.0, 2)
    assert pred.tolist() == [[2, 9]] and score[0, 0] == 1.0 and score[0, 1] == pytest.approx(math.exp(-1000.0), abs=1e-300)
    assert RTOL == 1e-4


def test_accuracy_on_hand_made_predictions():
    from cstp_amd.knn import accuracy
    q_labels = torch.tensor([4, 0, 7, 2, 3])
    pred = torch.tensor([[4, 1, 2, 3, 0],               # rank 1
                         [1, 2, 0, -1, -1],             # rank 3
                         [1, 2, 3, 4, 5],               # never
                         [0, 1, 3, 4, 2],               # rank 5
                         [-1, -1, -1, -1, -1]], dtype=torch.int32)   # no neighbour at all: never
    acc = accuracy(pred, q_labels)
    assert list(acc) == [1, 5] and acc[1] == pytest.approx(1 / 5) and acc[5] == pytest.approx(3 / 5)
    acc = accuracy(pred, q_labels, (3, 1, 2))
    assert list(acc) == [3, 1, 2] and acc[3] == pytest.approx(2 / 5) and acc[2] == pytest.approx(1 / 5)
    # -1 is no class: a (nonsensical) label of -1 must not match the padding
    assert accuracy(torch.tensor([[-1, -1]]), torch.tensor([-1]), (1, 2)) == {1: 0.0, 2: 0.0}
    assert accuracy(pred.to(torch.int64), q_labels.to(torch.int32), (1,))[1] == pytest.approx(1 / 5)
    with pytest.raises(ValueError):
        accuracy(pred, q_labels, (6,))
    with pytest.raises(ValueError):
        accuracy(pred, q_labels, (0,))
    with pytest.raises(ValueError):
        accuracy(pred, q_labels[:3])


def test_opts_carry_the_knn_flags():
    from cstp_amd import opts as opts_mod
    from cstp_amd.opts import parse_opts
    d = parse_opts([])
    assert d.knn_k == 20 and d.knn_t == 0.07 and d.knn_every == 0
    o = parse_opts(["--knn_k", "64", "--knn_t", "0.5", "--knn_every", "3"])
    assert o.knn_k == 64 and o.knn_t == 0.5 and o.knn_every == 3
    assert parse_opts(["--knn_k", "1"]).knn_k == 1
    for bad in (["--knn_k", "0"], ["--knn_k", "65"], ["--knn_t", "0"], ["--knn_t", "-0.1"], ["--knn_t", "nan"]):
        with pytest.raises(SystemExit):
            parse_opts(bad)
    for flag in ("--knn_k", "--knn_t", "--knn_every"):
        assert flag in opts_mod.__doc__


def test_monitor_refuses_before_any_device_work():
    """main() checks the monitor's flags first: the refusals below are ValueErrors also where no device exists (there, a run
    that passed the check ends in main()'s NotImplementedError)."""
    import main_byol
    from cstp_amd.opts import parse_opts
    with pytest.raises(ValueError, match="labelled"):
        main_byol.main(parse_opts(["--knn_every", "1", "--dataset", "synthetic"]))
    for size in ("32", "128"):
        with pytest.raises(ValueError, match="112 and 224"):
            main_byol.main(parse_opts(["--knn_every", "1", "--dataset", "synthetic_video", "--sample_size", size]))
        with pytest.raises(ValueError, match="112 and 224"):
            main_byol.main(parse_opts(["--knn_every", "2", "--dataset", "UcfRepreBYOLSpPre", "--sample_size", size]))
    with pytest.raises(ValueError, match="knn_every"):
        main_byol.main(parse_opts(["--knn_every", "-1", "--dataset", "synthetic_video"]))
    # off: nothing is checked, whatever the data set and the size
    main_byol.check_knn_opts(parse_opts(["--dataset", "synthetic", "--sample_size", "32"]))
    for size in ("112", "224"):
        main_byol.check_knn_opts(parse_opts(["--knn_every", "1", "--dataset", "synthetic_video", "--sample_size", size]))
        main_byol.check_knn_opts(parse_opts(["--knn_every", "1", "--dataset", "UcfRepreBYOLSpPre", "--sample_size", size]))


def test_knn_driver_names_its_datasets():
    import knn as driver
    from cstp_amd.opts import parse_opts
    for name in ("Kin400RepreLMDB", "synthetic", "UcfRepreBYOLSpPre"):
        with pytest.raises(NotImplementedError, match="synthetic_video and UcfFineTune"):
            driver.run(parse_opts(["--dataset", name, "--transform_mode", "img_test"]))
    with pytest.raises(ValueError, match="img_test"):
        driver.build_sets(parse_opts(["--dataset", "synthetic_video", "--transform_mode", "img"]))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            driver.run(parse_opts(["--dataset", "synthetic_video", "--transform_mode", "img_test"]))


def test_build_video_sets_is_what_the_retrieval_driver_builds():
    import retrieval as driver
    from cstp_amd import retrieval
    from cstp_amd.opts import parse_opts
    o = parse_opts(["--dataset", "Kin400RepreLMDB", "--transform_mode", "img_test"])
    with pytest.raises(NotImplementedError):
        retrieval.build_video_sets(o)
    with pytest.raises(NotImplementedError):
        driver.build_sets(o)
    with pytest.raises(NotImplementedError):
        retrieval.build_video_sets(o, "UcfRepreBYOLSpPre")          # the monitor maps it to UcfFineTune itself
    with pytest.raises(ValueError, match="img_test"):
        retrieval.build_video_sets(parse_opts(["--dataset", "synthetic_video"]))


def test_knn_vote_refusals_on_cpu_tensors():
    from cstp_amd import ops
    from cstp_amd._lib import CstpError
    val, idx, lab = torch.zeros(3, 4), torch.zeros(3, 4, dtype=torch.int32), torch.zeros(9, dtype=torch.int64)
    with pytest.raises(CstpError, match="HIP device"):
        ops.knn_vote(val, idx, lab, 0.07)
    with pytest.raises(CstpError, match="float32"):
        ops.knn_vote(val.double(), idx, lab, 0.07)
    with pytest.raises(CstpError, match="int32"):
        ops.knn_vote(val, idx.to(torch.int64), lab, 0.07)
    with pytest.raises(CstpError, match="int64 or int32"):
        ops.knn_vote(val, idx, lab.float(), 0.07)
    with pytest.raises(CstpError, match="one shape"):
        ops.knn_vote(val, idx[:, :3], lab, 0.07)
    with pytest.raises(CstpError, match="one shape"):
        ops.knn_vote(val[0], idx[0], lab, 0.07)
    with pytest.raises(CstpError, match="gallery labels"):
        ops.knn_vote(val, idx, lab.reshape(3, 3), 0.07)
    with pytest.raises(CstpError, match="k must be"):
        ops.knn_vote(torch.zeros(3, 65), torch.zeros(3, 65, dtype=torch.int32), lab, 0.07)
    with pytest.raises(CstpError, match="empty"):
        ops.knn_vote(val, idx, lab[:0], 0.07)
    for n_top in (0, 9, 2.0, True):
        with pytest.raises(CstpError, match="n_top"):
            ops.knn_vote(val, idx, lab, 0.07, n_top)
    for t in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(CstpError, match="temperature"):
            ops.knn_vote(val, idx, lab, t)


def test_knn_vote_is_declared_bound_and_exported():
    from cstp_amd import _lib
    assert "cstp_knn_vote" in header_symbols() and "cstp_knn_vote" in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 18                       # a pure addition, as the LARS and mixing entry points were
    assert "#define CSTP_ABI_VERSION 18" in open(os.path.join(os.path.dirname(_lib._HERE), "include", "cstp_hip.h")).read()
    lib = _lib.load()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "cstp_knn_vote")
    assert lib.cstp_abi_version() == 18


def test_knn_vote_refuses_bad_arguments_before_any_hip_call():
    from cstp_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)                           # never dereferenced: the checks fail first
    good = [None, one, one, one, 8, 100, 20, 1.0 / 0.07, 5, one, one]

    def call(**kw):
        names = ("stream", "val", "idx", "g_labels", "nq", "ng", "k", "inv_t", "n_top", "pred", "score")
        args = list(good)
        for n, v in kw.items():
            args[names.index(n)] = v
        rc = lib.cstp_knn_vote(*args)
        return rc, lib.cstp_last_error()

    cases = [(dict(val=None), b"null argument"), (dict(idx=None), b"null argument"), (dict(g_labels=None), b"null argument"),
             (dict(pred=None), b"null argument"), (dict(score=None), b"null argument"),
             (dict(k=65), b"k must be in 1..64"), (dict(k=0), b"k must be in 1..64"),
             (dict(n_top=9), b"n_top must be in 1..8"), (dict(n_top=0), b"n_top must be in 1..8"),
             (dict(inv_t=0.0), b"inv_t"), (dict(inv_t=-1.0), b"inv_t"), (dict(inv_t=float("inf")), b"inv_t"),
             (dict(inv_t=float("nan")), b"inv_t"),
             (dict(nq=0), b"bad shape"), (dict(nq=-3), b"bad shape"), (dict(ng=0), b"bad shape")]
    for kw, needle in cases:
        rc, msg = call(**kw)
        assert rc != 0 and needle in msg and b"line" in msg, (kw, rc, msg)


def test_vote_ref_agrees_with_a_dense_fp64_formulation():
    """The spec's per-slot loop against the textbook one-hot formulation (weights scattered into [nq, classes], then a stable
    sort): the same classes and scores wherever no near tie is marked."""
    rs = np.random.RandomState(0)
    nq, ng, k, classes, n_top = 40, 200, 20, 7, 5
    labels = rs.randint(0, classes, size=ng)
    sims = rs.uniform(-1, 1, size=(nq, ng))
    idx = np.argsort(-sims, axis=1, kind="stable")[:, :k]
    val = np.take_along_axis(sims, idx, axis=1)
    pred, score, near = vote_ref(val, idx, labels, 1.0 / 0.07, n_top)
    table = np.zeros((nq, classes))
    w = np.exp((val - val[:, :1]) / 0.07)
    for i in range(nq):
        np.add.at(table[i], labels[idx[i]], w[i])
    order = np.argsort(-table, axis=1, kind="stable")[:, :n_top]
    dense = np.take_along_axis(table, order, axis=1)
    order = np.where(dense > 0, order, -1)
    keep = ~near
    assert keep.mean() > 0.9
    assert (pred[keep] == order[keep]).all()
    np.testing.assert_allclose(score[keep], dense[keep], rtol=1e-12, atol=0)

"""Few-shot episodic evaluation, the parts that need no GPU: the episode sampler, the specification against its own definition,
the margin condition that the GPU test's decision check rests on, the acc / ci95 arithmetic, the five flags, the C ABI of
cstp_fewshot_episodes (declared, bound, exported, refusing every limit before any HIP call) and the checks of the op wrapper as
far as they run without a device."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import fewshot_spec as spec
from test_abi import header_symbols

NAME = "cstp_fewshot_episodes"


# ---- the sampler ----------------------------------------------------------------------------------------------------------------
def _labels(seed=0, n_classes=12, lo=3, hi=30):
    """Two lists with class sizes between lo and hi, shuffled."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        sizes = rng.integers(lo, hi + 1, n_classes)
        out.append(torch.from_numpy(rng.permutation(np.repeat(np.arange(n_classes) * 7 + 3, sizes))))
    return out


def test_sampler_is_deterministic_and_private():
    from cstp_amd import fewshot
    s_lab, q_lab = _labels()
    state = np.random.get_state()[1].copy()
    torch_state = torch.get_rng_state().clone()
    a = fewshot.sample_episodes(s_lab, q_lab, 5, 3, 3, 50, seed=7)
    b = fewshot.sample_episodes(s_lab, q_lab, 5, 3, 3, 50, seed=7)
    c = fewshot.sample_episodes(s_lab, q_lab, 5, 3, 3, 50, seed=8)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], c[0])
    assert bool((np.random.get_state()[1] == state).all()) and torch.equal(torch.get_rng_state(), torch_state)
    for t, shape in zip(a, ((50, 5, 3), (50, 5, 3), (50, 5))):
        assert t.dtype == torch.int32 and tuple(t.shape) == shape and t.device.type == "cpu" and t.is_contiguous()


def test_sampler_draws_without_replacement_from_the_right_rows(capsys):
    from cstp_amd import fewshot
    s_lab, q_lab = _labels(seed=3)
    n_way, kmax, n_query, episodes = 4, 5, 6, 300
    sup, qry, classes = fewshot.sample_episodes(s_lab, q_lab, n_way, kmax, n_query, episodes, seed=1)
    shown = capsys.readouterr().out
    every = sorted(set(s_lab.tolist()) | set(q_lab.tolist()))
    eligible = {c for c in every if int((s_lab == c).sum()) >= kmax and int((q_lab == c).sum()) >= n_query}
    assert 0 < len(eligible) < len(every)                                  # the lists were chosen so that some classes drop out
    lines = [ln for ln in shown.split("\n") if ln.startswith("Few-shot sampler: dropped")]
    assert len(lines) == 1 and "dropped %d of %d classes" % (len(every) - len(eligible), len(every)) in lines[0]
    for e in range(episodes):
        cls = classes[e].tolist()
        assert len(set(cls)) == n_way and set(cls) <= eligible             # no class twice, no ineligible class
        for slot, c in enumerate(cls):
            rows_s, rows_q = sup[e, slot].tolist(), qry[e, slot].tolist()
            assert len(set(rows_s)) == kmax and len(set(rows_q)) == n_query   # no video twice within a class
            assert all(int(s_lab[r]) == c for r in rows_s) and all(int(q_lab[r]) == c for r in rows_q)
    assert set(classes.flatten().tolist()) == eligible                     # 300 episodes reach every eligible class
    # every support video of an eligible class is reachable
    c0 = sorted(eligible)[0]
    assert set(sup[classes == c0].flatten().tolist()) == set((s_lab == c0).nonzero().flatten().tolist())


def test_sampler_without_dropped_classes_prints_nothing(capsys):
    from cstp_amd import fewshot
    lab = torch.arange(6).repeat_interleave(4)
    fewshot.sample_episodes(lab, lab, 3, 4, 4, 5, seed=0)
    assert capsys.readouterr().out == ""


def test_sampler_refuses_too_few_eligible_classes():
    from cstp_amd import fewshot
    s_lab, q_lab = _labels(seed=3)
    with pytest.raises(ValueError, match=r"5-way episodes need 5 eligible classes, \d+ of 12 have at least 31 support and 2 query"):
        fewshot.sample_episodes(s_lab, q_lab, 5, 31, 2, 4, seed=0)
    with pytest.raises(ValueError, match="at least 1"):
        fewshot.sample_episodes(s_lab, q_lab, 5, 0, 2, 4, seed=0)


# ---- the specification ----------------------------------------------------------------------------------------------------------
def test_specification_against_the_definition():
    xs, ls = spec.make_features(7, seed=1, part=0, n_classes=5, per_class=6)
    xq, lq = spec.make_features(7, seed=1, part=1, n_classes=5, per_class=6)
    sup, qry = spec.make_tables(ls, lq, 3, 4, 2, 3, seed=0)
    xs[sup[1, 2]] = 0.0                                                     # a zero prototype: score 0 for that slot
    score, pred, hits, margin = spec.episodes_ref(xs, xq, sup, qry, (1, 2, 4))
    score2, pred2, hits2 = spec.episodes_loops(xs, xq, sup, qry, (1, 2, 4))
    assert np.allclose(score, score2, rtol=0, atol=1e-14) and (pred == pred2).all() and (hits == hits2).all()
    assert (score[:, 1, :, 2] == 0).all() and (margin >= 0).all()
    # all prototypes zero: every score 0, slot 0 wins, the hits are the queries of slot 0
    zero = np.zeros_like(xs)
    _, pred0, hits0, _ = spec.episodes_ref(zero, xq, sup, qry, (4,))
    assert (pred0 == 0).all() and (hits0 == 2).all()


@pytest.mark.parametrize("case", [c for c in spec.CASES if c[0] >= 16], ids=str)
def test_margin_condition_of_the_gpu_cases(case):
    """What check (c) of the GPU test rests on: at most 1 % of the (episode, query) decisions of a case lie within 2 tol of a
    flip, so comparing predictions outside that band compares at least 99 % of them; and the decisions are not trivial."""
    d, n, shots, q, e = case
    _, _, _, _, (score, pred, hits, margin) = spec.case_data(*case)
    close = float((margin <= 2.0 * spec.tol(d, shots[-1])).mean())
    acc = float(hits.sum()) / (len(shots) * e * n * q)
    print("case %s: %.3f %% of the decisions within 2 tol = %.2e of a flip, spec accuracy %.3f" % (case, 100 * close,
                                                                                              2 * spec.tol(d, shots[-1]), acc))
    assert close <= 0.01
    assert 1.5 / n < acc < 0.98                                            # well above chance, well below certainty


def test_tolerance_formula():
    assert spec.tol(512, 5) == 2 * (1024 + 5 + 8) * 2.0 ** -24


# ---- acc / ci95 -----------------------------------------------------------------------------------------------------------------
def test_accuracy_and_confidence_interval_arithmetic():
    from cstp_amd import fewshot
    hits = torch.tensor([[10, 20, 30, 40], [75, 75, 75, 75]], dtype=torch.int32)
    acc, ci = fewshot.accuracy_from_hits(hits, 75)
    a = np.array([10, 20, 30, 40]) / 75.0
    assert acc[0] == pytest.approx(a.mean(), rel=1e-15) and acc[1] == 1.0
    assert ci[0] == pytest.approx(1.96 * a.std() / math.sqrt(4), rel=1e-14) and ci[1] == 0.0
    with pytest.raises(ValueError, match="shot counts, episodes"):
        fewshot.accuracy_from_hits(torch.zeros(4), 75)
    res = {"n_way": 5, "episodes": 4, "acc": {1: acc[0]}, "ci95": {1: ci[0]}}
    assert fewshot.format_line(res, 1) == "Few-shot 5-way 1-shot: %.4f ± %.4f (4 episodes)" % (acc[0], ci[0])


# ---- flags ----------------------------------------------------------------------------------------------------------------------
def test_opts_carry_the_fewshot_flags_and_the_dump_is_unchanged():
    from cstp_amd import opts as opts_mod
    from cstp_amd.opts import fewshot_opts, parse_opts
    d = parse_opts([])
    assert fewshot_opts(d) == (5, (1, 5), 15, 10000, 0)
    assert not [k for k in vars(d) if k.startswith("fewshot")]             # the options dump of every driver is unchanged
    assert "fewshot" not in str(d)
    o = parse_opts("--fewshot_way 20 --fewshot_shot 1 5 16 --fewshot_query 16 --fewshot_episodes 2000 --fewshot_seed 3".split())
    assert fewshot_opts(o) == (20, (1, 5, 16), 16, 2000, 3)
    assert fewshot_opts(parse_opts(["--fewshot_shot", "3"])) == (5, (3,), 15, 10000, 0)
    bad = [["--fewshot_way", "1"], ["--fewshot_way", "21"], ["--fewshot_query", "0"], ["--fewshot_query", "33"],
           ["--fewshot_way", "20", "--fewshot_query", "17"], ["--fewshot_shot", "0"], ["--fewshot_shot", "17"],
           ["--fewshot_shot", "5", "1"], ["--fewshot_shot", "1", "1"], ["--fewshot_shot", "1", "2", "3", "4", "5"],
           ["--fewshot_episodes", "0"], ["--fewshot_episodes", str((1 << 20) + 1)], ["--fewshot_seed", "-1"], ["--fewshot_way", "x"]]
    for argv in bad:
        with pytest.raises(SystemExit):
            parse_opts(argv)
    for flag in ("--fewshot_way", "--fewshot_shot", "--fewshot_query", "--fewshot_episodes", "--fewshot_seed"):
        assert flag in opts_mod.__doc__
    assert "not tuned" in opts_mod.__doc__


def test_driver_names_its_datasets_and_says_what_was_not_measured():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mod_spec = importlib.util.spec_from_file_location("fewshot_driver", os.path.join(root, "fewshot.py"))
    driver = importlib.util.module_from_spec(mod_spec)
    mod_spec.loader.exec_module(driver)
    from cstp_amd import fewshot
    from cstp_amd.opts import parse_opts
    for name in ("Kin400RepreLMDB", "synthetic", "UcfRepreBYOLSpPre"):
        with pytest.raises(NotImplementedError, match="synthetic_video and UcfFineTune"):
            driver.run(parse_opts(["--dataset", name, "--transform_mode", "img_test"]))
    with pytest.raises(ValueError, match="img_test"):
        driver.build_sets(parse_opts(["--dataset", "synthetic_video", "--transform_mode", "img"]))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            driver.run(parse_opts(["--dataset", "synthetic_video", "--transform_mode", "img_test"]))
    for doc in (driver.__doc__, fewshot.__doc__):
        assert "not tuned" in doc and "no few-shot accuracy of a trained encoder" in doc


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_bound_and_exported():
    from cstp_amd import _lib
    assert NAME in header_symbols() and NAME in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 18                       # a pure addition
    lib = _lib.load()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME) and lib.cstp_abi_version() == 18


def test_entry_point_refuses_every_limit_before_any_hip_call():
    """Dummy non-null pointers that are never dereferenced: each limit gives its own message with the line, rc != 0, and no
    launch is attempted (a launch on these pointers would fault on a device and fail without one)."""
    from cstp_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(64)
    names = ("stream", "xs", "ns", "xq", "nq", "d", "sup_idx", "qry_idx", "episodes", "n_way", "n_query", "shots", "n_shots", "hits",
             "pred", "score")

    def shots(*ks):
        return (ctypes.c_int32 * len(ks))(*ks)
    good = [None, one, 100, one, 100, 512, one, one, 10, 5, 15, shots(1, 5), 2, one, None, None]
    cases = [(dict(xs=None), b"null argument"), (dict(xq=None), b"null argument"), (dict(sup_idx=None), b"null argument"),
             (dict(qry_idx=None), b"null argument"), (dict(hits=None), b"null argument"), (dict(shots=None), b"null argument"),
             (dict(ns=0), b"ns and nq"), (dict(nq=-1), b"ns and nq"), (dict(d=0), b"d must be in 1..8192"),
             (dict(d=8193), b"d must be in 1..8192"), (dict(episodes=0), b"episodes must be in 1..2^20"),
             (dict(episodes=(1 << 20) + 1), b"episodes must be in 1..2^20"), (dict(n_way=1), b"n_way must be in 2..20"),
             (dict(n_way=21), b"n_way must be in 2..20"), (dict(n_query=0), b"n_query must be in 1..32"),
             (dict(n_query=33), b"n_query must be in 1..32"), (dict(n_way=20, n_query=17), b"at most 320"),
             (dict(n_shots=0), b"n_shots must be in 1..4"), (dict(n_shots=5, shots=shots(1, 2, 3, 4, 5)), b"n_shots must be in 1..4"),
             (dict(shots=shots(0, 5)), b"shots must lie in 1..16"), (dict(shots=shots(1, 17)), b"shots must lie in 1..16"),
             (dict(shots=shots(5, 1)), b"strictly ascending"), (dict(shots=shots(5, 5)), b"strictly ascending")]
    for kw, needle in cases:
        args = list(good)
        for n, v in kw.items():
            args[names.index(n)] = v
        rc = lib.cstp_fewshot_episodes(*args)
        msg = lib.cstp_last_error()
        assert rc != 0 and needle in msg and b"(line " in msg, (kw, rc, msg)


# ---- the op wrapper -------------------------------------------------------------------------------------------------------------
def test_op_checks_that_run_without_a_device():
    from cstp_amd import ops
    from cstp_amd._lib import CstpError
    xs, xq = torch.zeros(50, 8), torch.zeros(40, 8)
    sup = torch.zeros(3, 5, 5, dtype=torch.int32)
    qry = torch.zeros(3, 5, 4, dtype=torch.int32)

    def call(xs=xs, xq=xq, sup=sup, qry=qry, n_query=4, shots=(1, 5), **kw):
        return ops.fewshot_episodes(xs, xq, sup, qry, n_query, shots, **kw)
    for shots in ((), (0,), (17,), (5, 1), (1, 1), (1, 2, 3, 4, 5), (1.0, 5), (True, 5), 5):
        with pytest.raises(CstpError, match="shots must be"):
            call(shots=shots)
    with pytest.raises(CstpError, match="float32"):
        call(xs=xs.double())
    with pytest.raises(CstpError, match=r"\[rows, features\]"):
        call(xq=xq[0])
    with pytest.raises(CstpError, match="xs has 8 features, xq 9"):
        call(xq=torch.zeros(40, 9))
    with pytest.raises(CstpError, match="empty"):
        call(xs=xs[:0])
    with pytest.raises(CstpError, match="at most 8192 features"):
        call(xs=torch.zeros(2, 8193), xq=torch.zeros(2, 8193))
    with pytest.raises(CstpError, match="int32"):
        call(sup=sup.long())
    with pytest.raises(CstpError, match="int32"):
        call(qry=qry.long())
    with pytest.raises(CstpError, match=r"\[episodes, ways, shots\]"):
        call(sup=sup[0])
    with pytest.raises(CstpError, match="qry_idx must be"):
        call(qry=torch.zeros(3, 4, 4, dtype=torch.int32))
    with pytest.raises(CstpError, match="qry_idx must be"):
        call(n_query=3)
    with pytest.raises(CstpError, match="n_query must be"):
        call(n_query=33)
    with pytest.raises(CstpError, match="5 support columns, the largest shot count is 4"):
        call(shots=(1, 4))
    with pytest.raises(CstpError, match="2..20 ways"):
        call(sup=torch.zeros(3, 1, 5, dtype=torch.int32), qry=torch.zeros(3, 1, 4, dtype=torch.int32))
    with pytest.raises(CstpError, match="at most 320 query slots"):
        call(sup=torch.zeros(3, 20, 5, dtype=torch.int32), qry=torch.zeros(3, 20, 17, dtype=torch.int32), n_query=17)
    with pytest.raises(CstpError, match="contiguous"):
        call(sup=torch.zeros(3, 5, 10, dtype=torch.int32)[:, :, ::2])
    # the range check of host tables: before any upload, against the rows of the side the table indexes
    for name, table, rows in (("sup_idx", "sup", 50), ("qry_idx", "qry", 40)):
        for bad in (-1, rows):
            t = (sup if table == "sup" else qry).clone()
            t[2, 4, 3] = bad
            with pytest.raises(CstpError, match=r"%s holds rows .* the features have rows 0\.\.%d" % (name, rows - 1)):
                call(**{table: t})
    t = qry.clone()
    t[0, 0, 0] = 39                                                         # the last valid row passes the range check ...
    with pytest.raises(CstpError, match="HIP device"):                      # ... and the CPU features are what is refused
        call(qry=t)
    assert "TAKEN\n    AS VALID" in ops.fewshot_episodes.__doc__ or "TAKEN AS VALID" in " ".join(ops.fewshot_episodes.__doc__.split())

"""Label-free collapse metrics, the parts that need no GPU: the two flags, the C ABI of cstp_feat_gram / cstp_pair_potential
(declared, bound, exported, refusing bad arguments before any HIP call, workspace caps), the refusals of the two ops on CPU
tensors, the host half of health.metrics on sums computed on the CPU (known answers and the fp64 specification), and the
refusals of the --health_every monitor and of the health.py driver before any device work."""
import ctypes
import math
import os

import pytest
import torch

import health_spec as spec
from test_abi import header_symbols

NAMES = ("cstp_feat_gram_workspace_bytes", "cstp_feat_gram", "cstp_pair_potential_workspace_bytes", "cstp_pair_potential")


def test_opts_carry_the_health_flags_and_default_to_off():
    from cstp_amd import opts as opts_mod
    from cstp_amd.opts import health_opts, parse_opts
    d = parse_opts([])
    assert health_opts(d) == (0, 2.0)
    assert "health_every" not in vars(d) and "health_t" not in vars(d)          # the options dump of every driver is unchanged
    o = parse_opts(["--health_every", "3", "--health_t", "0.5"])
    assert health_opts(o) == (3, 0.5)
    for bad in (["--health_t", "0"], ["--health_t", "-1"], ["--health_t", "nan"], ["--health_t", "inf"], ["--health_every", "x"]):
        with pytest.raises(SystemExit):
            parse_opts(bad)
    for flag in ("--health_every", "--health_t"):
        assert flag in opts_mod.__doc__


def test_the_four_symbols_are_declared_bound_and_exported():
    from cstp_amd import _lib
    for name in NAMES:
        assert name in header_symbols() and name in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 18                       # a pure addition
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, name) for name in NAMES)
    assert lib.cstp_abi_version() == 18


def _refusals(fn_name, names, good, cases):
    from cstp_amd import _lib
    lib = _lib.load()
    for kw, needle in cases:
        args = list(good)
        for n, v in kw.items():
            args[names.index(n)] = v
        rc = getattr(lib, fn_name)(*args)
        msg = lib.cstp_last_error()
        assert rc != 0 and needle in msg and b"line" in msg, (fn_name, kw, rc, msg)


def test_feat_gram_refuses_bad_arguments_before_any_hip_call():
    one = ctypes.c_void_p(64)                           # never dereferenced: the checks fail first
    names = ("stream", "x", "n", "d", "gram", "colsum", "ws", "ws_bytes")
    good = [None, one, 100, 33, one, one, one, 1 << 30]
    _refusals("cstp_feat_gram", names, good, [
        (dict(x=None), b"null argument"), (dict(gram=None), b"null argument"), (dict(colsum=None), b"null argument"),
        (dict(ws=None), b"null argument"), (dict(n=0), b"n must be"), (dict(n=-5), b"n must be"), (dict(d=0), b"d must be"),
        (dict(d=4097), b"d must be"), (dict(n=1 << 20, d=2048), b"2^31"), (dict(ws_bytes=0), b"workspace too small"),
        (dict(ws_bytes=33 * 8), b"workspace too small"), (dict(gram=ctypes.c_void_p(68)), b"8-byte aligned"),
        (dict(colsum=ctypes.c_void_p(66)), b"8-byte aligned"), (dict(ws=ctypes.c_void_p(65)), b"8-byte aligned")])


def test_pair_potential_refuses_bad_arguments_before_any_hip_call():
    one = ctypes.c_void_p(64)
    names = ("stream", "x", "n", "d", "t", "rowsum", "ws", "ws_bytes")
    good = [None, one, 100, 33, 2.0, one, one, 1 << 30]
    _refusals("cstp_pair_potential", names, good, [
        (dict(x=None), b"null argument"), (dict(rowsum=None), b"null argument"), (dict(ws=None), b"null argument"),
        (dict(n=0), b"n must be"), (dict(d=0), b"d must be"), (dict(d=5000), b"d must be"), (dict(n=1 << 20, d=2048), b"2^31"),
        (dict(t=0.0), b"t must be"), (dict(t=-2.0), b"t must be"), (dict(t=float("inf")), b"t must be"),
        (dict(t=float("nan")), b"t must be"), (dict(t=3e38), b"t must be"), (dict(ws_bytes=100 * 8), b"workspace too small"),
        (dict(rowsum=ctypes.c_void_p(68)), b"8-byte aligned"), (dict(ws=ctypes.c_void_p(70)), b"8-byte aligned")])


@pytest.mark.parametrize("n", [1, 64, 9537, 65536])
def test_workspace_caps(n):
    """pair_potential: at most SQ_MAX_SPLIT = 32 doubles per row; feat_gram: one double per feature and 1024 rows.  Both
    are pure host functions and 0 on a bad shape."""
    from cstp_amd import _lib
    lib = _lib.load()
    for d in (1, 512, 2048):
        pp = lib.cstp_pair_potential_workspace_bytes(n, d)
        assert 8 * n <= pp <= 32 * 8 * n + 4096, (n, d, pp)
        assert pp == lib.cstp_pair_potential_workspace_bytes(n, 1)         # a function of n alone
        fg = lib.cstp_feat_gram_workspace_bytes(n, d)
        assert fg == (n + 1023) // 1024 * d * 8 + 256, (n, d, fg)
    assert lib.cstp_pair_potential_workspace_bytes(0, 8) == 0 and lib.cstp_pair_potential_workspace_bytes(8, 4097) == 0
    assert lib.cstp_feat_gram_workspace_bytes(-1, 8) == 0 and lib.cstp_feat_gram_workspace_bytes(1 << 20, 2048) == 0


def test_ops_refuse_cpu_tensors_and_bad_operands():
    from cstp_amd import ops
    from cstp_amd._lib import CstpError
    x = torch.zeros(5, 8)
    for fn in (ops.feat_gram, ops.pair_potential):
        with pytest.raises(CstpError, match="HIP device"):
            fn(x)
        with pytest.raises(CstpError, match="float32"):
            fn(x.double())
        with pytest.raises(CstpError, match=r"\[rows, features\]"):
            fn(x[0])
        with pytest.raises(CstpError, match="empty"):
            fn(x[:0])
        with pytest.raises(CstpError, match="at most 4096 features"):
            fn(torch.zeros(2, 4097))
    for t in (0.0, -1.0, float("inf"), float("nan"), True, "2"):
        with pytest.raises(CstpError, match="t must be"):
            ops.pair_potential(x, t)


def _cpu_parts(feat, t=2.0):
    """The four device results computed on the CPU in fp64 from fp64-normalised rows."""
    x = spec.normalize_ref(feat)
    gram, colsum = spec.gram_ref(x)
    return gram, colsum, spec.pair_potential_ref(x, t), spec.nn_sim_ref(x)


def test_host_half_on_one_hot_rows():
    from cstp_amd import health
    x = spec.one_hot_rows()
    res = health.metrics_from_parts(*_cpu_parts(x), 96, 40, 2.0)
    assert res["erank"] == pytest.approx(7.0, abs=1e-9)
    assert res["top1_share"] == pytest.approx(1.0 / 7.0, abs=1e-12)
    assert res["rankme"] == pytest.approx(8.0004, abs=5e-5)              # the 1e-7 offset on 40 values lifts it above 8
    p = torch.tensor([0.125 + 1e-7] * 8 + [1e-7] * 32, dtype=torch.float64)
    assert res["rankme"] == pytest.approx(math.exp(-float((p * p.log()).sum())), rel=1e-12)
    assert res["std_ratio"] == pytest.approx(0.41833, abs=5e-6)
    assert res["std_ratio"] == pytest.approx(math.sqrt(40) * 8 * math.sqrt(7.0 / 64.0) / 40, rel=1e-12)
    assert res["nn_sim"] == 1.0
    # 11 of a row's 95 partners are its copies (exp(0)), 84 are orthogonal (exp(-2 t))
    assert res["uniformity"] == pytest.approx(math.log((11 + 84 * math.exp(-4.0)) / 95), rel=1e-12)
    assert (res["n"], res["d"], res["t"]) == (96, 40, 2.0)
    assert set(res) == set(health.KEYS) | {"n", "d", "t"}


def test_host_half_on_collapsed_rows():
    from cstp_amd import health
    x = spec.collapsed_rows()
    res = health.metrics_from_parts(*_cpu_parts(x), 50, 16, 2.0)
    for key, want in spec.COLLAPSED_ANSWERS.items():
        assert res[key] == want, (key, res[key])
    assert res["rankme"] == pytest.approx(1.0, abs=1e-4) and res["nn_sim"] == 1.0


@pytest.mark.parametrize("shape", [(200, 33, 5, 0.05), (129, 512, 40, 0.2)])
def test_host_half_is_the_specification(shape):
    """health.metrics_from_parts and tests/health_spec.py are written independently; on the same fp64 sums they agree to
    rounding.  rankme where n < d (zero eigenvalues of G under the square root) only to the conditioning the docstring states."""
    from cstp_amd import health
    n, d, rank, noise = shape
    feat = spec.make_features(n, d, rank, noise, seed=n + d)
    want = spec.metrics_ref(feat, 2.0)
    res = health.metrics_from_parts(*_cpu_parts(feat), n, d, 2.0)
    for key in health.KEYS:
        tol = 1e-12 if key != "rankme" or n >= d else 1e-6
        assert res[key] == pytest.approx(want[key], rel=tol, abs=tol), key
    assert 1.0 <= res["erank"] <= min(n - 1, d) and 0.0 < res["std_ratio"] < 1.5 and res["uniformity"] < 0.0
    assert "ill-conditioned" in health.__doc__.lower()


def test_fewer_than_two_rows_raise():
    from cstp_amd import health
    one = torch.ones(1, 4)
    with pytest.raises(ValueError, match="at least 2 rows"):
        health.metrics(one)
    with pytest.raises(ValueError, match="at least 2 rows"):
        health.metrics_from_parts(torch.ones(4, 4), torch.ones(4), torch.ones(1), torch.ones(1), 1, 4)
    with pytest.raises(ValueError, match="rows, features"):
        health.metrics(torch.ones(4))


def test_monitor_refuses_before_any_device_work():
    """main() checks the monitor's flags first: what check_knn_opts refuses for --knn_every, with the monitor's own message."""
    import main_byol
    from cstp_amd.opts import parse_opts
    for name in ("synthetic", "Kin400RepreLMDB"):
        with pytest.raises(ValueError, match="health monitor"):
            main_byol.main(parse_opts(["--health_every", "1", "--dataset", name]))
    for size in ("32", "128"):
        with pytest.raises(ValueError, match="112 and 224"):
            main_byol.main(parse_opts(["--health_every", "1", "--dataset", "synthetic_video", "--sample_size", size]))
    with pytest.raises(ValueError, match="health_every"):
        main_byol.main(parse_opts(["--health_every", "-1", "--dataset", "synthetic_video"]))
    # off: nothing is checked, whatever the data set and the size
    main_byol.check_health_opts(parse_opts(["--dataset", "synthetic", "--sample_size", "32"]))
    main_byol.check_health_opts(parse_opts(["--health_every", "0", "--dataset", "synthetic", "--sample_size", "32"]))
    for size in ("112", "224"):
        main_byol.check_health_opts(parse_opts(["--health_every", "2", "--dataset", "synthetic_video", "--sample_size", size]))
        main_byol.check_health_opts(parse_opts(["--health_every", "2", "--dataset", "UcfRepreBYOLSpPre", "--sample_size", size]))
    assert "--knn_every" in main_byol.HealthMonitor.__doc__ or "KnnMonitor" in main_byol.HealthMonitor.__doc__


def test_health_driver_names_its_datasets():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mod_spec = importlib.util.spec_from_file_location("health_driver", os.path.join(root, "health.py"))
    driver = importlib.util.module_from_spec(mod_spec)
    mod_spec.loader.exec_module(driver)
    from cstp_amd.opts import parse_opts
    for name in ("Kin400RepreLMDB", "synthetic", "UcfRepreBYOLSpPre"):
        with pytest.raises(NotImplementedError, match="synthetic_video and UcfFineTune"):
            driver.run(parse_opts(["--dataset", name, "--transform_mode", "img_test"]))
    with pytest.raises(ValueError, match="img_test"):
        driver.build_sets(parse_opts(["--dataset", "synthetic_video", "--transform_mode", "img"]))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            driver.run(parse_opts(["--dataset", "synthetic_video", "--transform_mode", "img_test"]))

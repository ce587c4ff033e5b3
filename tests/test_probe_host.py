"""Linear probe on cached features, the parts that need no GPU: the fp64 specification tests/probe_spec.py against
torch.nn.functional.cross_entropy + autograd, its treatment of bad labels and row indices, the near-tie share of every GPU case,
probe.plan and probe.standardize, the five flags, the refusals of the driver, of ops.probe_step / ops.probe_predict and of the
C ABI (declared, bound, exported, refusing bad arguments before any HIP call), and the workspace formula."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from probe_spec import LOGIT_TOL_ULPS, MAX_NEAR_TIE_SHARE, STEP_CASES, make_case, predict_ref, step_ref
from test_abi import header_symbols


def _torch_ref(case, rows, standardised):
    x = torch.from_numpy(case["x"]).double()
    if standardised:
        x = (x - torch.from_numpy(case["mean"]).double()) * torch.from_numpy(case["inv_std"]).double()
    idx = torch.arange(case["n"]) if rows is None else torch.from_numpy(rows).long()
    w = torch.from_numpy(case["w"]).double().requires_grad_()
    b = torch.from_numpy(case["b"]).double().requires_grad_()
    loss = torch.nn.functional.cross_entropy(x[idx] @ w.T + b, torch.from_numpy(case["labels"])[idx])
    loss.backward()
    return float(loss), w.grad.numpy(), b.grad.numpy()


@pytest.mark.parametrize("standardised", [True, False])
def test_step_ref_is_cross_entropy_with_autograd(standardised):
    for m, n, d, c, rows in STEP_CASES[:3] + STEP_CASES[6:]:
        case = make_case(m, n, d, c, rows)
        kw = dict(mean=case["mean"], inv_std=case["inv_std"]) if standardised else {}
        ref = step_ref(case["x"], case["labels"], case["w"], case["b"], case["rows"], **kw)
        loss, dw, db = _torch_ref(case, case["rows"], standardised)
        assert (case["rows"] is None) == (not rows)
        assert ref["loss"] == pytest.approx(loss, rel=1e-12)
        np.testing.assert_allclose(ref["dw"], dw, rtol=0, atol=1e-13 * max(1.0, np.abs(dw).max()))
        np.testing.assert_allclose(ref["db"], db, rtol=0, atol=1e-13)
        assert 0 <= ref["hits"] <= m and ref["bound"].shape == (m,)


def test_step_ref_drops_bad_labels_and_bad_rows():
    case = make_case(70, 300, 23, 3, True)
    rows, labels = case["rows"].copy(), case["labels"].copy()
    rows[3], rows[11] = -1, 300
    labels[rows[5]], labels[rows[20]] = -1, 3
    bad = step_ref(case["x"], labels, case["w"], case["b"], rows, case["mean"], case["inv_std"])
    # the same batch with those four rows taken out, rescaled from its own mean to the mean over all 70
    keep = np.ones(70, dtype=bool)
    keep[[3, 11, 5, 20]] = False
    good = step_ref(case["x"], case["labels"], case["w"], case["b"], rows[keep], case["mean"], case["inv_std"])
    f = keep.sum() / 70.0
    assert bad["loss"] == pytest.approx(good["loss"] * f, rel=1e-12)
    np.testing.assert_allclose(bad["dw"], good["dw"] * f, rtol=0, atol=1e-14)
    np.testing.assert_allclose(bad["db"], good["db"] * f, rtol=0, atol=1e-14)
    assert bad["hits"] == good["hits"]


def test_near_tie_share_of_every_gpu_case_is_under_the_cap():
    """From the spec alone, on exactly the inputs of tests/test_probe_gpu.py: the (row, rank) pairs among the top five that a
    near tie touches, and the rows whose top-1 is one."""
    for m, n, d, c, rows in STEP_CASES:
        case = make_case(m, n, d, c, rows)
        for kw in (dict(mean=case["mean"], inv_std=case["inv_std"]), {}):
            for n_top in (1, 5):
                _, _, near, _ = predict_ref(case["x"], case["w"], case["b"], n_top=n_top, **kw)
                assert near[:, :min(n_top, c)].mean() <= MAX_NEAR_TIE_SHARE, (m, n, d, c, n_top, near.mean())
            ref = step_ref(case["x"], case["labels"], case["w"], case["b"], case["rows"], **kw)
            assert ref["near_top1"].sum() <= max(1, MAX_NEAR_TIE_SHARE * m), (m, n, d, c)
    assert LOGIT_TOL_ULPS <= 64


def test_predict_ref_orders_ties_by_class_and_pads():
    x = np.array([[1.0, 0.0], [0.0, 1.0]], dtype=np.float32)
    w = np.array([[1.0, 0.0], [1.0, 0.0], [0.0, 2.0]], dtype=np.float32)
    b = np.zeros(3, dtype=np.float32)
    cls, val, near, _ = predict_ref(x, w, b, n_top=5)
    assert cls.tolist() == [[0, 1, 2, -1, -1], [2, 0, 1, -1, -1]]
    assert val.tolist() == [[1.0, 1.0, 0.0, 0.0, 0.0], [2.0, 0.0, 0.0, 0.0, 0.0]]
    assert near.tolist() == [[True, True, False, False, False], [False, True, True, False, False]]


def test_plan_is_a_pure_function_of_its_arguments():
    from cstp_amd.probe import plan
    perm, lrs, bounds = plan(300, 5, 64, 0.1, 3)
    perm2, lrs2, bounds2 = plan(300, 5, 64, 0.1, 3)
    assert torch.equal(perm, perm2) and torch.equal(lrs, lrs2) and bounds == bounds2
    assert perm.dtype == torch.int32 and tuple(perm.shape) == (5, 300) and lrs.dtype == torch.float32
    for e in range(5):
        assert sorted(perm[e].tolist()) == list(range(300))
    assert not torch.equal(perm[0], perm[1]) and not torch.equal(perm, plan(300, 5, 64, 0.1, 4)[0])
    assert bounds == [(0, 64), (64, 128), (128, 192), (192, 256), (256, 300)]
    steps = 25
    assert lrs.numel() == steps and float(lrs[0]) == pytest.approx(0.1, rel=1e-7)
    assert float(lrs[-1]) == pytest.approx(0.1 * 0.5 * (1 + math.cos(math.pi * (steps - 1) / steps)), rel=1e-6)
    assert all(float(lrs[i]) > float(lrs[i + 1]) for i in range(steps - 1))
    assert plan(300, 2, 0, 0.1, 0)[2] == [(0, 300)] and plan(300, 2, 0, 0.1, 0)[1].numel() == 2
    assert plan(10, 1, 64, 0.1, 0)[2] == [(0, 10)]
    for bad in ((0, 1, 1), (5, 0, 1), (5, 1, -1)):
        with pytest.raises(ValueError):
            plan(bad[0], bad[1], bad[2], 0.1, 0)


def test_standardize_drops_a_constant_column():
    from cstp_amd.probe import standardize
    g = torch.Generator().manual_seed(0)
    feat = torch.randn((50, 6), generator=g) * 3 + 2
    feat[:, 4] = 1.25
    mean, inv_std = standardize(feat)
    assert mean.dtype == inv_std.dtype == torch.float32
    assert float(inv_std[4]) == 0.0 and float(mean[4]) == 1.25
    z = (feat.double() - mean.double()) * inv_std.double()
    keep = [0, 1, 2, 3, 5]
    assert torch.allclose(z[:, keep].mean(dim=0), torch.zeros(5, dtype=torch.float64), atol=1e-6)
    assert torch.allclose((z[:, keep] ** 2).mean(dim=0), torch.ones(5, dtype=torch.float64), atol=1e-5)
    assert float(z[:, 4].abs().max()) == 0.0


def test_opts_carry_the_probe_flags():
    from cstp_amd import opts as opts_mod
    from cstp_amd.opts import parse_opts
    d = parse_opts([])
    assert (d.probe_epochs, d.probe_batch, d.probe_lr, d.probe_wd, d.probe_optimizer) == (100, 1024, 1e-3, 0.0, "adam")
    o = parse_opts(["--probe_epochs", "3", "--probe_batch", "0", "--probe_lr", "0.5", "--probe_wd", "1e-4", "--probe_optimizer", "sgd"])
    assert (o.probe_epochs, o.probe_batch, o.probe_lr, o.probe_wd, o.probe_optimizer) == (3, 0, 0.5, 1e-4, "sgd")
    for bad in (["--probe_epochs", "0"], ["--probe_batch", "-1"], ["--probe_lr", "0"], ["--probe_lr", "-1e-3"],
                ["--probe_lr", "nan"], ["--probe_lr", "inf"], ["--probe_wd", "-1"], ["--probe_optimizer", "lars"]):
        with pytest.raises(SystemExit):
            parse_opts(bad)
    for flag in ("--probe_epochs", "--probe_batch", "--probe_lr", "--probe_wd", "--probe_optimizer"):
        assert flag in opts_mod.__doc__


def test_probe_driver_names_its_datasets():
    import linear_probe as driver
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
    from cstp_amd import probe
    feat, labels = torch.zeros(8, 4), torch.zeros(8, dtype=torch.int64)
    with pytest.raises(ValueError, match="optimizer"):
        probe.fit(feat, labels, 3, optimizer="lars")
    for kw in (dict(lr=0.0), dict(lr=float("nan")), dict(weight_decay=-1.0), dict(epochs=0), dict(batch=-2)):
        with pytest.raises(ValueError):
            probe.fit(feat, labels, 3, **kw)


def test_probe_ops_refusals_on_cpu_tensors():
    from cstp_amd import ops
    from cstp_amd._lib import CstpError
    x, lab = torch.zeros(6, 4), torch.zeros(6, dtype=torch.int64)
    w, b = torch.zeros(3, 4), torch.zeros(3)
    rows = torch.zeros(5, dtype=torch.int32)
    mean = torch.zeros(4)
    for call in (lambda **kw: ops.probe_step(kw.pop("x", x), kw.pop("labels", lab), kw.pop("w", w), kw.pop("b", b), **kw),
                 lambda **kw: (kw.pop("labels", None), ops.probe_predict(kw.pop("x", x), kw.pop("w", w), kw.pop("b", b), **kw))[1]):
        with pytest.raises(CstpError, match="HIP device"):
            call()
        with pytest.raises(CstpError, match="x must be float32"):
            call(x=x.double())
        with pytest.raises(CstpError, match="w must be float32"):
            call(w=w.double())
        with pytest.raises(CstpError, match="x must be"):
            call(x=x[0])
        with pytest.raises(CstpError, match="w must be"):
            call(w=torch.zeros(3, 5))
        with pytest.raises(CstpError, match="b must be"):
            call(b=torch.zeros(4))
        with pytest.raises(CstpError, match="mean must be"):
            call(mean=torch.zeros(5))
        with pytest.raises(CstpError, match="inv_std must be float32"):
            call(inv_std=mean.double())
        with pytest.raises(CstpError, match="classes c"):
            call(w=torch.zeros(1, 4), b=torch.zeros(1))
        with pytest.raises(CstpError, match="classes c"):
            call(w=torch.zeros(1025, 4), b=torch.zeros(1025))
        with pytest.raises(CstpError, match="empty"):
            call(x=x[:0], labels=lab[:0])
    with pytest.raises(CstpError, match="labels must be \\[6\\]"):
        ops.probe_step(x, lab[:5], w, b)
    with pytest.raises(CstpError, match="labels must be int64"):
        ops.probe_step(x, lab.to(torch.int32), w, b)
    with pytest.raises(CstpError, match="rows must be int32"):
        ops.probe_step(x, lab, w, b, rows.to(torch.int64))
    with pytest.raises(CstpError, match="rows must be"):
        ops.probe_step(x, lab, w, b, rows[:0])
    with pytest.raises(CstpError, match="out must be"):
        ops.probe_step(x, lab, w, b, out=(torch.zeros(1),))
    with pytest.raises(CstpError, match="out hits"):
        ops.probe_step(x, lab, w, b, out=(torch.zeros(1), torch.zeros(1), torch.zeros(3, 4), torch.zeros(3)))
    with pytest.raises(CstpError, match="out dw"):
        ops.probe_step(x, lab, w, b, out=(torch.zeros(1), torch.zeros(1, dtype=torch.int32), torch.zeros(4, 3), torch.zeros(3)))
    for n_top in (0, 9, 2.0, True):
        with pytest.raises(CstpError, match="n_top"):
            ops.probe_predict(x, w, b, n_top=n_top)


PROBE_SYMBOLS = ("cstp_probe_workspace_bytes", "cstp_probe_step", "cstp_probe_predict")


def test_probe_entry_points_are_declared_bound_and_exported():
    from cstp_amd import _lib
    for name in PROBE_SYMBOLS:
        assert name in header_symbols() and name in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 18                       # pure additions
    assert "#define CSTP_ABI_VERSION 18" in open(os.path.join(os.path.dirname(_lib._HERE), "include", "cstp_hip.h")).read()
    lib = _lib.load()
    for name in PROBE_SYMBOLS:
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert lib.cstp_abi_version() == 18


def test_probe_workspace_bytes_follows_the_documented_formula():
    from cstp_amd import _lib
    lib = _lib.load()

    def formula(m, d, c):
        cpad = 4 * ((c + 3) // 4)
        s = max(1, min(32, -(-m // 64), 512 // ((-(-d // 64)) * (-(-c // 64)))))
        r16 = lambda v: -(-v // 16) * 16
        return 4 * m * cpad + r16(8 * m) + r16(4 * s * c) + (4 * s * c * d if s > 1 else 0)

    for m, d, c in [(1, 8, 2), (70, 23, 3), (64, 4, 65), (1024, 512, 101), (1024, 2048, 101), (9537, 512, 101), (1024, 1024, 400),
                    (257, 100, 400), (33, 2048, 101), (5, 2048, 1024)]:
        assert lib.cstp_probe_workspace_bytes(m, d, c) == formula(m, d, c), (m, d, c)
    for bad in [(0, 8, 2), (-1, 8, 2), (8, 0, 2), (8, 8, 1), (8, 8, 1025), (8, 1 << 22, 1024)]:
        assert lib.cstp_probe_workspace_bytes(*bad) == 0, bad
    for d, c in [(512, 101), (23, 3), (2048, 1024)]:
        sizes = [lib.cstp_probe_workspace_bytes(m, d, c) for m in range(1, 3000, 7)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0


def test_probe_entry_points_refuse_bad_arguments_before_any_hip_call():
    from cstp_amd import _lib
    lib = _lib.load()
    one, two = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 30)        # never dereferenced: the checks fail first
    big = 1 << 28
    names = ("stream", "x", "rows", "labels", "mean", "inv_std", "w", "b", "m", "n", "d", "c", "loss", "hits", "dw", "db", "ws",
             "ws_bytes")
    good = [None, one, None, one, None, None, ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20), 8, 100, 16, 10, one, one,
            ctypes.c_void_p(3 << 20), ctypes.c_void_p(4 << 20), two, big]

    def step(**kw):
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        return lib.cstp_probe_step(*args), lib.cstp_last_error()

    cases = [(dict(x=None), b"null argument"), (dict(labels=None), b"null argument"), (dict(w=None), b"null argument"),
             (dict(b=None), b"null argument"), (dict(loss=None), b"null argument"), (dict(hits=None), b"null argument"),
             (dict(dw=None), b"null argument"), (dict(db=None), b"null argument"), (dict(ws=None), b"null argument"),
             (dict(c=1), b"c must be in 2..1024"), (dict(c=1025), b"c must be in 2..1024"),
             (dict(m=0), b"bad shape"), (dict(n=0), b"bad shape"), (dict(d=0), b"bad shape"), (dict(m=-4), b"bad shape"),
             (dict(m=101), b"m must not exceed n"),
             (dict(dw=ctypes.c_void_p(1 << 20)), b"must not alias"), (dict(dw=ctypes.c_void_p((1 << 20) + 16)), b"must not alias"),
             (dict(db=ctypes.c_void_p(2 << 20)), b"must not alias"), (dict(db=ctypes.c_void_p((1 << 20) + 8)), b"must not alias"),
             (dict(dw=ctypes.c_void_p((2 << 20) - 64)), b"must not alias"),
             (dict(ws=ctypes.c_void_p((1 << 30) + 4)), b"16-byte aligned"),
             (dict(ws_bytes=lib.cstp_probe_workspace_bytes(8, 16, 10) - 1), b"workspace too small"), (dict(ws_bytes=0), b"workspace too small")]
    for kw, needle in cases:
        rc, msg = step(**kw)
        assert rc != 0 and needle in msg and b"line" in msg, (kw, rc, msg)

    pnames = ("stream", "x", "mean", "inv_std", "w", "b", "n", "d", "c", "n_top", "pred", "score")
    pgood = [None, one, None, None, one, one, 100, 16, 10, 5, one, one]

    def predict(**kw):
        args = list(pgood)
        for k, v in kw.items():
            args[pnames.index(k)] = v
        return lib.cstp_probe_predict(*args), lib.cstp_last_error()

    pcases = [(dict(x=None), b"null argument"), (dict(w=None), b"null argument"), (dict(b=None), b"null argument"),
              (dict(pred=None), b"null argument"), (dict(score=None), b"null argument"),
              (dict(c=1), b"c must be in 2..1024"), (dict(c=1025), b"c must be in 2..1024"),
              (dict(n_top=0), b"n_top must be in 1..8"), (dict(n_top=9), b"n_top must be in 1..8"),
              (dict(n=0), b"bad shape"), (dict(d=0), b"bad shape"), (dict(d=-1), b"bad shape")]
    for kw, needle in pcases:
        rc, msg = predict(**kw)
        assert rc != 0 and needle in msg and b"line" in msg, (kw, rc, msg)

"""The linear-probe sweep, the parts that need no GPU: probe.holdout_split, the grid order and probe.select against the
restatements of tests/probe_sweep_spec.py, the per-step hyper table against plan()'s schedule (exactly), the three flags and the
driver's refusals, the three entry points (declared, bound, exported, ABI 18), the workspace formula, every refusal of the C ABI
and of ops.probe_sweep_*, and two conditions on the inputs of tests/test_probe_sweep_gpu.py asserted from the fp64 spec alone:
the near-tie share of head 0 of every case, and the margin by which the selection test's two grid points differ."""
import ctypes
import os

import numpy as np
import pytest
import torch

import probe_sweep_spec as ss
from probe_spec import MAX_NEAR_TIE_SHARE, step_ref
from test_abi import header_symbols


def _labels_with_small_classes():
    """Class 0: one row, class 1: two rows, class 2: 57 rows, classes 3..6: 7-13 rows, scattered."""
    rs = np.random.RandomState(11)
    lab = np.concatenate([[0], [1, 1], np.full(57, 2), np.full(7, 3), np.full(10, 4), np.full(13, 5), np.full(8, 6)])
    return rs.permutation(lab).astype(np.int64)


@pytest.mark.parametrize("fraction", [0.2, 0.5])
def test_holdout_split_matches_the_spec(fraction):
    from cstp_amd.probe import holdout_split
    lab = _labels_with_small_classes()
    for seed in (0, 7):
        train, val = holdout_split(torch.from_numpy(lab), fraction, seed)
        want_train, want_val = ss.holdout_ref(lab, fraction, seed)
        assert train.dtype == val.dtype == np.int32
        assert np.array_equal(train, want_train) and np.array_equal(val, want_val)
        again = holdout_split(lab, fraction, seed)                    # a numpy vector serves as well; same draws
        assert np.array_equal(again[0], train) and np.array_equal(again[1], val)
        assert np.all(np.diff(train) > 0) and np.all(np.diff(val) > 0)
        assert not set(train.tolist()) & set(val.tolist())
        assert sorted(train.tolist() + val.tolist()) == list(range(lab.size))
        counts = np.bincount(lab[val], minlength=7)
        sizes = np.bincount(lab, minlength=7)
        assert counts[0] == 0 and counts[1] == 1                       # a one-row class stays in training; of two rows one is held out
        for cls in range(2, 7):
            assert counts[cls] == max(1, int(np.floor(fraction * sizes[cls] + 0.5))), (cls, counts[cls], sizes[cls])
        assert np.all(np.bincount(lab[train], minlength=7) >= 1)
    assert not np.array_equal(holdout_split(lab, fraction, 0)[1], holdout_split(lab, fraction, 7)[1])
    for bad in (0.0, 0.51, -0.1, float("nan")):
        with pytest.raises(ValueError, match="fraction"):
            holdout_split(lab, bad, 0)


def test_grid_is_lr_major_and_refuses_bad_grids():
    from cstp_amd.probe import grid_points
    lrs, wds = (3e-2, 1e-3, 0.5), (0.0, 1e-2)
    assert grid_points(lrs, wds) == ss.grid_ref(lrs, wds) == [(3e-2, 0.0), (3e-2, 1e-2), (1e-3, 0.0), (1e-3, 1e-2), (0.5, 0.0), (0.5, 1e-2)]
    assert len(grid_points([float(i + 1) for i in range(8)], [0.0, 0.1, 0.2, 0.3])) == 32
    for bad_lrs, bad_wds in (([], [0.0]), ([1e-3], []), ([0.0], [0.0]), ([float("nan")], [0.0]), ([float("inf")], [0.0]), ([1e-3], [-1.0]),
                             ([1e-3, 1e-3], [0.0]), ([1e-3], [0.1, 0.1]), ([float(i + 1) for i in range(11)], [0.0, 0.1, 0.2])):
        with pytest.raises(ValueError, match="probe sweep"):
            grid_points(bad_lrs, bad_wds)


def _result(hits, loss):
    from cstp_amd.probe import SweepResult
    fields = dict.fromkeys(SweepResult._fields)
    fields.update(val_hits=torch.tensor(hits, dtype=torch.int32), val_loss=torch.tensor(loss, dtype=torch.float32))
    return SweepResult(**fields)


def test_select_orders_by_hits_then_loss_then_index():
    from cstp_amd.probe import select
    cases = [([3, 9, 5], [0.1, 0.9, 0.2], 1),                        # hits decide, whatever the loss
             ([9, 9, 5], [0.5, 0.25, 0.0], 1),                        # equal hits: the lower loss
             ([5, 9, 9, 9], [0.0, 0.5, 0.5, 0.75], 1),                # equal hits and loss: the lower index
             ([7, 7], [float("nan"), 2.0], 1),                        # a NaN loss loses to a number
             ([7], [1.0], 0)]
    for hits, loss, want in cases:
        assert select(_result(hits, loss)) == want, (hits, loss)
        if not any(v != v for v in loss):
            assert ss.select_ref(hits, loss) == want


@pytest.mark.parametrize("batch", [32, 0])
def test_hyper_table_holds_each_heads_own_schedule_exactly(batch):
    """Row t of the table is what the optimizer launch of step t reads: scale = the fp32 rate plan() gives head g at step t (the
    base rate is 1.0, and 1.0f * s == s), decay = wd_g on W_g and 0 on b_g; the chunk table covers every head's padded extents."""
    from cstp_amd import ops
    from cstp_amd.probe import grid_points, plan, sweep_tables
    t = ss.TRAIN
    grid = grid_points(t["lrs"], t["wds"])
    n_train, c, d = 71, t["c"], t["d"]      # the train part of tests/test_probe_sweep_gpu.py
    _, lrs0, bounds = plan(n_train, t["epochs"], batch, grid[0][0], t["seed"])
    steps = t["epochs"] * len(bounds)
    assert steps == (9 if batch else 3) and lrs0.numel() == steps
    chunks, hyper = sweep_tables(grid, c, d, steps)
    assert hyper.dtype == torch.float32 and tuple(hyper.shape) == (steps, 2 * len(grid), 2) and hyper.is_contiguous()
    want = ss.schedule_ref(grid, n_train, t["epochs"], batch, t["seed"])
    for g, (lr, wd) in enumerate(grid):
        for seg in (2 * g, 2 * g + 1):
            assert np.array_equal(hyper[:, seg, 0].numpy(), want[:, g]), (g, seg)        # bits, not a tolerance
        assert np.array_equal(hyper[:, 2 * g, 1].numpy(), np.full(steps, np.float32(wd)))
        assert np.array_equal(hyper[:, 2 * g + 1, 1].numpy(), np.zeros(steps, dtype=np.float32))
        assert np.float32(1.0) * hyper[0, 2 * g, 0].numpy() == np.float32(lr)
    seg = ss.head_stride(c, d)
    covered = np.zeros(len(grid) * seg, dtype=bool)
    for s, off, length in chunks:
        assert off % 4 == 0 and length % 4 == 0 and 0 < length <= ops.LARS_CHUNK and 0 <= s < 2 * len(grid)
        assert off // seg == s // 2 and not covered[off:off + length].any()
        covered[off:off + length] = True
    assert covered[ss.owned_mask(len(grid), c, d)].all()


def test_opts_carry_the_sweep_flags():
    from cstp_amd import opts as opts_mod
    from cstp_amd.opts import parse_opts, probe_grid
    d = parse_opts([])
    assert probe_grid(d) is None and opts_mod.PROBE_VAL_FRACTION == 0.2
    assert not any(k in vars(d) for k in ("probe_lrs", "probe_wds", "probe_val_fraction"))    # the options dump is unchanged
    assert probe_grid(parse_opts(["--probe_lrs", "1e-3"])) == ([1e-3], [0.0], 0.2)
    assert probe_grid(parse_opts(["--probe_lrs", "1e-3", "3e-2", "--probe_wd", "0.5"])) == ([1e-3, 3e-2], [0.5], 0.2)
    o = parse_opts(["--probe_lrs", "3e-2", "1e-3", "--probe_wds", "0", "1e-2", "--probe_val_fraction", "0.5"])
    assert probe_grid(o) == ([3e-2, 1e-3], [0.0, 1e-2], 0.5)
    for bad in (["--probe_lrs"], ["--probe_lrs", "0"], ["--probe_lrs", "-1"], ["--probe_lrs", "nan"], ["--probe_lrs", "inf"],
                ["--probe_lrs", "1e-3", "1e-3"], ["--probe_lrs", "1e-3", "--probe_wds", "-1"],
                ["--probe_lrs", "1e-3", "--probe_wds", "inf"], ["--probe_lrs", "1e-3", "--probe_wds", "0.1", "0.1"],
                ["--probe_lrs", "1e-3", "--probe_val_fraction", "0"], ["--probe_lrs", "1e-3", "--probe_val_fraction", "0.6"],
                ["--probe_lrs", "1e-3", "--probe_val_fraction", "nan"], ["--probe_wds", "0.1"], ["--probe_val_fraction", "0.2"],
                ["--probe_lrs"] + [str(i + 1) for i in range(33)],
                ["--probe_lrs"] + [str(i + 1) for i in range(11)] + ["--probe_wds", "0", "0.1", "0.2"]):
        with pytest.raises(SystemExit):
            parse_opts(bad)
    assert len(probe_grid(parse_opts(["--probe_lrs"] + [str(i + 1) for i in range(32)]))[0]) == 32
    doc = opts_mod.__doc__
    for flag in ("--probe_lrs", "--probe_wds", "--probe_val_fraction"):
        assert flag in doc
    assert "untuned" in doc and "no linear-probe accuracy of a trained encoder" in doc


def test_driver_and_evaluate_refuse_a_bad_grid_before_device_work():
    import linear_probe as driver
    from cstp_amd import probe
    from cstp_amd.opts import parse_opts
    base = ["--dataset", "synthetic_video", "--transform_mode", "img_test"]
    o = parse_opts(base + ["--probe_lrs", "1e-3"])
    o.probe_lrs = [1e-3, 1e-3]                                         # a namespace built by hand gets the same refusals
    with pytest.raises(ValueError, match="duplicate"):
        driver.run(o)
    o.probe_lrs, o.probe_wds = [float(i + 1) for i in range(11)], [0.0, 0.1, 0.2]
    with pytest.raises(ValueError, match="at most 32"):
        driver.run(o)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            driver.run(parse_opts(base + ["--probe_lrs", "1e-3", "1e-2"]))
    with pytest.raises(ValueError, match="without lrs"):
        probe.evaluate(None, None, None, 4, wds=[0.0])
    with pytest.raises(ValueError, match="without lrs"):
        probe.evaluate(None, None, None, 4, val_fraction=0.2)
    with pytest.raises(ValueError, match="duplicate"):
        probe.evaluate(None, None, None, 4, lrs=[1e-3, 1e-3])
    feat, labels = torch.zeros(8, 4), torch.zeros(8, dtype=torch.int64)
    with pytest.raises(ValueError, match="optimizer"):
        probe.sweep(feat, labels, 3, [1e-3], optimizer="lars")
    with pytest.raises(ValueError, match="fraction"):
        probe.sweep(feat, labels, 3, [1e-3], val_fraction=0.75)
    with pytest.raises(ValueError, match="nothing can be held out"):
        probe.sweep(feat, torch.arange(8), 8, [1e-3])


SWEEP_SYMBOLS = ("cstp_probe_sweep_workspace_bytes", "cstp_probe_sweep_step", "cstp_probe_sweep_score")


def test_sweep_entry_points_are_declared_bound_and_exported():
    from cstp_amd import _lib
    for name in SWEEP_SYMBOLS:
        assert name in header_symbols() and name in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 18                       # pure additions
    assert "#define CSTP_ABI_VERSION 18" in open(os.path.join(os.path.dirname(_lib._HERE), "include", "cstp_hip.h")).read()
    lib = _lib.load()
    for name in SWEEP_SYMBOLS:
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert lib.cstp_abi_version() == 18


def test_sweep_workspace_bytes_is_heads_times_the_rounded_single_head_size():
    from cstp_amd import _lib
    lib = _lib.load()
    r16 = lambda v: -(-v // 16) * 16
    for m, d, c in [(1, 8, 2), (70, 23, 3), (64, 4, 65), (1024, 512, 101), (1024, 2048, 101), (9537, 512, 101), (1024, 1024, 400),
                    (257, 100, 400), (33, 2048, 101), (5, 2048, 1024)]:
        single = lib.cstp_probe_workspace_bytes(m, d, c)
        assert single > 0
        for heads in (1, 3, 32):
            assert lib.cstp_probe_sweep_workspace_bytes(heads, m, d, c) == heads * r16(single), (heads, m, d, c)
    for bad in [(0, 8, 8, 2), (-1, 8, 8, 2), (33, 8, 8, 2), (2, 0, 8, 2), (2, -1, 8, 2), (2, 8, 0, 2), (2, 8, 8, 1), (2, 8, 8, 1025),
                (2, 8, 1 << 22, 1024)]:
        assert lib.cstp_probe_sweep_workspace_bytes(*bad) == 0, bad


def test_sweep_entry_points_refuse_bad_arguments_before_any_hip_call():
    from cstp_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    one, two = P(4096), P(1 << 30)                                     # never dereferenced: the checks fail first
    m, n, d, c, heads = 8, 100, 16, 10, 3
    stride = ss.head_stride(c, d)                                      # 172 floats = 688 bytes
    w, b, dw, db = 1 << 20, (1 << 20) + 4 * ss.pad4(c * d), 3 << 20, (3 << 20) + 4 * ss.pad4(c * d)
    need = lib.cstp_probe_sweep_workspace_bytes(heads, m, d, c)
    names = ("stream", "x", "rows", "labels", "mean", "inv_std", "w", "b", "head_stride", "heads", "m", "n", "d", "c", "loss", "hits",
             "dw", "db", "ws", "ws_bytes")
    good = [None, one, None, one, None, None, P(w), P(b), stride, heads, m, n, d, c, one, one, P(dw), P(db), two, 1 << 28]

    def call(score, **kw):
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        if score:
            del args[names.index("dw"):names.index("db") + 1]
            return lib.cstp_probe_sweep_score(*args), lib.cstp_last_error()
        return lib.cstp_probe_sweep_step(*args), lib.cstp_last_error()

    shared = [(dict(x=None), b"null argument"), (dict(labels=None), b"null argument"), (dict(w=None), b"null argument"),
              (dict(b=None), b"null argument"), (dict(loss=None), b"null argument"), (dict(hits=None), b"null argument"),
              (dict(ws=None), b"null argument"),
              (dict(heads=0), b"heads must be in 1..32"), (dict(heads=33), b"heads must be in 1..32"), (dict(heads=-1), b"heads must be"),
              (dict(c=1), b"c must be in 2..1024"), (dict(c=1025), b"c must be in 2..1024"),
              (dict(m=0), b"bad shape"), (dict(n=0), b"bad shape"), (dict(d=0), b"bad shape"), (dict(m=-4), b"bad shape"),
              (dict(m=101), b"m must not exceed n"),
              (dict(head_stride=stride + 2), b"head stride"), (dict(head_stride=stride - 4), b"head stride"),
              (dict(head_stride=ss.pad4(c * d) + 8), b"head stride"), (dict(head_stride=0), b"head stride"),
              (dict(head_stride=-stride), b"head stride"),
              (dict(ws=P((1 << 30) + 4)), b"16-byte aligned"),
              (dict(ws_bytes=need - 1), b"workspace too small"), (dict(ws_bytes=0), b"workspace too small"),
              (dict(ws_bytes=lib.cstp_probe_workspace_bytes(m, d, c)), b"workspace too small")]
    step_only = [(dict(dw=None), b"null argument"), (dict(db=None), b"null argument"),
                 (dict(dw=P(w)), b"must not alias"), (dict(db=P(b)), b"must not alias"),
                 (dict(dw=P(w + 4 * stride)), b"must not alias"),                   # dW_0 on W_1
                 (dict(dw=P(w + 8 * stride - 4 * c * d + 16)), b"must not alias"),  # the tail of dW_0 on the head of W_2
                 (dict(db=P(b + 8 * stride)), b"must not alias"),                   # db_0 on b_2
                 (dict(dw=P(w - 8 * stride)), b"must not alias"),                   # dW_2 on W_0
                 (dict(db=P(w - 4 * stride + 4 * c * d - 4)), b"must not alias")]   # db_1's first float on W_0's last
    for score in (False, True):
        for kw, needle in shared + ([] if score else step_only):
            rc, msg = call(score, **kw)
            assert rc != 0 and needle in msg and b"line" in msg, (score, kw, rc, msg)
    # stride pad4(c d) + c exactly is accepted by the stride check (c a multiple of 4): the next refusal in line answers
    rc, msg = call(False, c=12, head_stride=ss.pad4(12 * d) + 12, ws_bytes=0)
    assert rc != 0 and b"workspace too small" in msg


def test_probe_sweep_ops_refusals_on_cpu_tensors():
    from cstp_amd import ops
    from cstp_amd._lib import CstpError
    G, c, d = 3, 3, 4
    x, lab = torch.zeros(6, d), torch.zeros(6, dtype=torch.int64)
    arena = torch.zeros(G * ss.head_stride(c, d))
    w, b = ops.probe_head_views(arena, G, c, d)
    assert w.stride() == (16, 4, 1) and b.stride() == (16, 1) and b.storage_offset() == 12
    rows, mean = torch.zeros(5, dtype=torch.int32), torch.zeros(d)
    with pytest.raises(CstpError, match="arena"):
        ops.probe_head_views(arena, G + 1, c, d)
    for fn in (ops.probe_sweep_step, ops.probe_sweep_score):
        def call(**kw):
            return fn(kw.pop("x", x), kw.pop("labels", lab), kw.pop("w", w), kw.pop("b", b), **kw)
        with pytest.raises(CstpError, match="HIP device"):
            call()
        with pytest.raises(CstpError, match="x must be float32"):
            call(x=x.double())
        with pytest.raises(CstpError, match="must be float32"):
            call(w=w.double())
        with pytest.raises(CstpError, match="x must be"):
            call(x=x[0])
        with pytest.raises(CstpError, match="heads, classes, features"):
            call(w=w[0])
        with pytest.raises(CstpError, match="heads, classes, features"):
            call(b=torch.zeros(G + 1, c))
        with pytest.raises(CstpError, match="w must be"):
            call(x=torch.zeros(6, d + 1))
        with pytest.raises(CstpError, match="b must be"):
            call(b=torch.zeros(48).as_strided((G, c + 1), (16, 1)))
        with pytest.raises(CstpError, match="heads must be in 1..32"):
            call(w=torch.zeros(33, c, d), b=torch.zeros(33, c))
        with pytest.raises(CstpError, match="disagree on the head stride"):
            call(b=torch.zeros(G, c))
        with pytest.raises(CstpError, match="head stride"):
            call(w=torch.zeros(G, c, d), b=torch.zeros(G * c * d).as_strided((G, c), (c * d, 1)))     # no room for b between the heads
        with pytest.raises(CstpError, match="head stride"):
            call(w=torch.zeros(G * 18).as_strided((G, c, d), (18, d, 1)), b=torch.zeros(G * 18).as_strided((G, c), (18, 1)))
        with pytest.raises(CstpError, match="contiguous"):
            call(w=torch.zeros(G, d, c).transpose(1, 2), b=b)
        with pytest.raises(CstpError, match="mean must be"):
            call(mean=torch.zeros(d + 1))
        with pytest.raises(CstpError, match="inv_std must be float32"):
            call(inv_std=mean.double())
        with pytest.raises(CstpError, match="classes c"):
            call(w=torch.zeros(16).as_strided((2, 1, d), (8, d, 1)), b=torch.zeros(16).as_strided((2, 1), (8, 1)))
        with pytest.raises(CstpError, match="empty"):
            call(x=x[:0], labels=lab[:0])
        with pytest.raises(CstpError, match="labels must be \\[6\\]"):
            call(labels=lab[:5])
        with pytest.raises(CstpError, match="labels must be int64"):
            call(labels=lab.to(torch.int32))
        with pytest.raises(CstpError, match="rows must be int32"):
            call(rows=rows.to(torch.int64))
        with pytest.raises(CstpError, match="rows must be"):
            call(rows=rows[:0])
        with pytest.raises(CstpError, match="out must be"):
            call(out=(torch.zeros(G),))
        with pytest.raises(CstpError, match="out hits"):
            call(out=(torch.zeros(G), torch.zeros(G)) + ((w.clone(), b.clone()) if fn is ops.probe_sweep_step else ()))
        with pytest.raises(CstpError, match="out loss"):
            call(out=(torch.zeros(1), torch.zeros(G, dtype=torch.int32)) + ((w.clone(), b.clone()) if fn is ops.probe_sweep_step else ()))
    ok = (torch.zeros(G), torch.zeros(G, dtype=torch.int32))
    with pytest.raises(CstpError, match="out dw / db must have the shapes"):
        ops.probe_sweep_step(x, lab, w, b, out=ok + (torch.zeros(G, d, c), torch.zeros(G, c)))
    with pytest.raises(CstpError, match="out dw / db"):
        ops.probe_sweep_step(x, lab, w, b, out=ok + (torch.zeros(G, c, d), torch.zeros(G, c)))       # contiguous: another stride


def test_near_tie_share_of_head_zero_of_every_sweep_case_is_under_the_cap():
    """From the spec alone, on exactly the inputs of tests/test_probe_sweep_gpu.py (head 0 is probe_spec.make_case's own head)."""
    for G, m, n, d, c, rows in ss.SWEEP_CASES:
        case = ss.make_sweep_case(G, m, n, d, c, rows)
        assert case["w"].shape == (G, c, d) and case["b"].shape == (G, c)
        assert G == 1 or not np.array_equal(case["w"][0], case["w"][1])
        for kw in (dict(mean=case["mean"], inv_std=case["inv_std"]), {}):
            ref = step_ref(case["x"], case["labels"], case["w"][0], case["b"][0], case["rows"], **kw)
            assert ref["near_top1"].sum() <= max(1, MAX_NEAR_TIE_SHARE * m), (G, m, n, d, c)


def test_the_selection_inputs_separate_the_two_grid_points_by_a_quarter_of_the_validation_rows():
    """A condition on the inputs of the GPU selection test, from fit_ref (fp64) alone: the hit counts of lr = 1e-6 and lr = 1e-2
    on the held-out rows differ by at least a quarter of those rows, so no rounding difference can change the winner."""
    hits, n_val = ss.select_val_hits_fp64()
    print("selection inputs: validation hits %s of %d" % (hits, n_val))
    assert ss.SELECT["lrs"] == (1e-6, 1e-2)
    assert hits[1] - hits[0] >= 0.25 * n_val

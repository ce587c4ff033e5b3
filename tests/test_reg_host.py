"""Dropout / stochastic depth, the parts that need no GPU: Philox4x32-10 (the restatement and the library's own host evaluation)
against its known answers, the plan (cstp_amd.regularize) against known answers and as a pure function, the flag rules, the
restated forwards against the functional oracles, and the C ABI of the three entry points."""
import argparse
import ctypes
import os

import numpy as np
import pytest
import torch

import reg_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (counter, key) -> output; the first two are the known-answer vectors of the Random123 distribution, the third its pi-digits one
PHILOX_VECTORS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
PLAN_ANSWERS = [      # seed 1, batch 4, n_blocks 4, dropout 0.5, drop_path 0.3
    ((0, 0, 0), 0x15b7fa397883287b, [[1, 1, 1, 1], [1, 1, 0, 1], [1, 1, 1, 1], [0, 0, 1, 1]]),
    ((2, 5, 1), 0xce3ae104d723a7ad, [[1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1], [1, 0, 1, 1]]),
]


@pytest.mark.parametrize("ctr,key,want", PHILOX_VECTORS)
def test_philox_known_answers(ctr, key, want):
    assert [int(v) for v in reg_spec.philox4x32_10(ctr, key)] == list(want)
    # ... and the function the dropout kernel is compiled from, evaluated on the host by the library
    from cstp_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_uint32 * 4)()
    assert lib.cstp_philox4x32_10((ctypes.c_uint32 * 4)(*ctr), (ctypes.c_uint32 * 2)(*key), out) == 0
    assert list(out) == list(want)


def test_philox_restatement_is_vectorised_consistently():
    q = np.arange(0, 37, dtype=np.uint64)
    many = reg_spec.philox4x32_10((q, 0, 7, 1), (3, 9))
    for i in (0, 1, 36):
        assert np.array_equal(many[i], reg_spec.philox4x32_10((int(q[i]), 0, 7, 1), (3, 9)))
    keep = reg_spec.dropout_keep(4001, 0.3, 0x15b7fa397883287b)
    assert keep.shape == (4001,) and abs(keep.mean() - 0.7) < 0.03
    assert np.array_equal(keep[:407], reg_spec.dropout_keep(407, 0.3, 0x15b7fa397883287b))       # a prefix: the mask is per element
    assert not np.array_equal(keep, reg_spec.dropout_keep(4001, 0.3, 0x15b7fa397883287b, offset=1))


@pytest.mark.parametrize("pos,key,keep", PLAN_ANSWERS)
def test_plan_known_answers(pos, key, keep):
    from cstp_amd.regularize import Regularizer
    plan = Regularizer(0.5, 0.3, seed=1).plan(4, 4, *pos)
    assert plan.key == key
    assert plan.keep.astype(int).tolist() == keep
    assert plan.p == pytest.approx([0.0, 0.1, 0.2, 0.3])
    assert plan.scale.dtype == np.float32 and plan.scale.shape == (4, 4)
    want = np.array(keep, dtype=np.float64) / (1.0 - np.array(plan.p)[:, None])
    assert np.array_equal(plan.scale, want.astype(np.float32))


def test_plan_is_a_pure_function_of_its_arguments():
    from cstp_amd.regularize import Regularizer
    reg = Regularizer(0.5, 0.3, seed=1)
    state = (np.random.get_state()[1].copy(), torch.get_rng_state().clone())
    a = reg.plan(8, 8, 3, 4, 1)
    b = Regularizer(0.5, 0.3, seed=1).plan(8, 8, 3, 4, 1)
    assert a.key == b.key and np.array_equal(a.keep, b.keep) and np.array_equal(a.scale, b.scale)
    assert np.array_equal(np.random.get_state()[1], state[0]) and torch.equal(torch.get_rng_state(), state[1])   # global streams untouched
    for other in ((4, 4, 1), (3, 5, 1), (3, 4, 0)):                      # epoch, step and rank each change the plan
        c = reg.plan(8, 8, *other)
        assert c.key != a.key and not np.array_equal(c.keep, a.keep)
    assert Regularizer(0.5, 0.3, seed=2).plan(8, 8, 3, 4, 1).key != a.key
    # a flag at 0 makes no draw: dropout only has no table, drop-path only has no key and reads the stream from its start
    only_d, only_p = Regularizer(0.5, 0.0, seed=1).plan(8, 8, 3, 4, 1), Regularizer(0.0, 0.3, seed=1).plan(8, 8, 3, 4, 1)
    assert only_d.key == a.key and only_d.keep is None and only_d.scale is None
    assert only_p.key is None and only_p.keep.shape == (8, 8)
    with pytest.raises(ValueError):
        reg.plan(0, 8, 0, 0, 0)
    with pytest.raises(ValueError):
        reg.plan(8, 8, -1, 0, 0)


def test_drop_rates_follow_the_linear_rule():
    from cstp_amd.regularize import Regularizer, block_probabilities
    reg = Regularizer(0.0, 0.2, seed=1)
    p = np.array(block_probabilities(0.2, 8))
    assert p[0] == 0.0 and p[-1] == pytest.approx(0.2) and np.allclose(np.diff(p), 0.2 / 7)
    kept = np.zeros(8)
    for step in range(200):
        plan = reg.plan(16, 8, 0, step, 0)
        assert plan.keep[0].all()                                         # the first block is never dropped
        kept += plan.keep.mean(axis=1)
    dev = np.abs(kept / 200 - (1.0 - p))
    print("kept share per block:", kept / 200, "largest deviation %.4f" % dev.max())
    assert dev.max() < 0.02
    assert block_probabilities(0.3, 1) == [0.0] and block_probabilities(0.3, 0) == []


def _opts(**kw):
    base = dict(dropout=0.0, drop_path=0.0, manual_seed=1, model_name="r21d_byol", task="ft_all")
    base.update(kw)
    return argparse.Namespace(**base)


def test_flag_rules():
    from cstp_amd.opts import parse_opts
    from cstp_amd.regularize import Regularizer, build_regularizer
    o = parse_opts([])
    assert o.dropout == 0.0 and o.drop_path == 0.0
    o = parse_opts(["--dropout", "0.5", "--drop_path", "0.1"])
    assert o.dropout == 0.5 and o.drop_path == 0.1
    assert build_regularizer(_opts()) is None                             # 0 / 0: the step is exactly today's
    reg = build_regularizer(_opts(dropout=0.5, drop_path=0.1, manual_seed=7))
    assert isinstance(reg, Regularizer) and (reg.dropout, reg.drop_path, reg.seed) == (0.5, 0.1, 7)
    for flag in ("dropout", "drop_path"):
        for bad in (-0.1, 1.0, 1.5, float("nan")):
            with pytest.raises(ValueError, match="--" + flag):
                build_regularizer(_opts(**{flag: bad}))
    for kw in (dict(task="ft_fc"), dict(model_name="s3d_byol"), dict(model_name="i3d_byol")):
        with pytest.raises(ValueError, match="--drop_path"):
            build_regularizer(_opts(drop_path=0.1, **kw))
        assert build_regularizer(_opts(dropout=0.5, **kw)).dropout == 0.5  # dropout serves every backbone, ft_fc and ft_all
    assert build_regularizer(_opts(drop_path=0.1, model_name="r3d_byol")).drop_path == 0.1
    with pytest.raises(ValueError):
        Regularizer(0.5, 0.1, seed=-1)


def test_only_the_fine_tune_driver_regularises():
    for name in ("test.py", "retrieval.py", "knn.py", "main_byol.py", os.path.join("cstp_amd", "retrieval.py"),
                 os.path.join("cstp_amd", "knn.py")):
        src = open(os.path.join(ROOT, name)).read()
        assert "regulariz" not in src and "drop_path" not in src, name
    src = open(os.path.join(ROOT, "main_ft_mp.py")).read()
    assert "build_regularizer(opts)" in src and "regularizer=regularizer" in src
    val = src[src.index("def validation("):src.index("def main_worker(")]
    assert "regulariz" not in val


def test_restated_forwards_equal_the_oracles_bit_for_bit():
    """Dropout off and every block's scale 1: the restatement IS oracle.ft_forward; it also equals it with no scales at all."""
    from oracle import r21d_byol_oracle as orc
    from oracle import r21d_ft_oracle as fto
    from oracle import r3d_byol_oracle as r3d
    x, _, _ = orc.closed_form_clips(2, 4, 32, torch.float32)
    ones = [torch.ones(2)] * 4
    with torch.no_grad():
        sd = fto.closed_form_state((1, 1, 1, 1), 7, torch.float32)
        clone = lambda: {k: v.clone() for k, v in sd.items()}
        want = fto.ft_forward(clone(), x, (1, 1, 1, 1), True)
        assert torch.equal(reg_spec.r21d_ft_forward(clone(), x, (1, 1, 1, 1), ones, None), want)
        assert torch.equal(reg_spec.r21d_ft_forward(clone(), x, (1, 1, 1, 1)), want)
        assert torch.equal(reg_spec.r21d_ft_forward(clone(), x, (1, 1, 1, 1), ones, (0.0, 5)), want)
        assert torch.equal(reg_spec.r21d_ft_forward(clone(), x, (1, 1, 1, 1), None, (0.5, 5), training=False),
                           fto.ft_forward(clone(), x, (1, 1, 1, 1), False))
        layers = r3d.for_depth(10)
        sd = r3d.closed_form_state(r3d.ft_spec(layers, 7), torch.float32)
        want = r3d.ft_forward(clone(), x, layers, True)
        assert torch.equal(reg_spec.r3d_ft_forward(clone(), x, layers, ones, None), want)
        assert torch.equal(reg_spec.r3d_ft_forward(clone(), x, layers), want)
        # and the operations do something when they are on
        assert not torch.equal(reg_spec.r3d_ft_forward(clone(), x, layers, [None, torch.tensor([0.0, 2.0])] + ones[2:], None), want)
        assert not torch.equal(reg_spec.r3d_ft_forward(clone(), x, layers, None, (0.5, 5)), want)


def test_restated_operations():
    x = np.linspace(-2, 2, 407, dtype=np.float32)
    y = reg_spec.dropout_fp32(x, 0.5, 9, 3)
    keep = reg_spec.dropout_keep(407, 0.5, 9, 3)
    assert np.array_equal(y[keep], x[keep] * np.float32(2.0)) and not y[~keep].any()
    t = torch.from_numpy(x).double().requires_grad_(True)
    reg_spec.dropout_torch(t, 0.5, 9, 3).sum().backward()
    assert np.array_equal(t.grad.numpy(), np.where(keep, 2.0, 0.0))        # the backward is the same mask and scale
    z, r = torch.tensor([[1.0, -3.0], [2.0, -1.0]], dtype=torch.float64), torch.tensor([[0.5, 1.0], [-1.0, 0.25]], dtype=torch.float64)
    assert reg_spec.drop_path_add_relu(z, r, [0.0, 1.25]).tolist() == [[0.5, 1.0], [1.5, 0.0]]


def test_residual_blocks_are_numbered_in_forward_order():
    from cstp_amd.r21d_byol import R21DBYOL
    from cstp_amd.r3d_byol import R3DBYOL
    m = R21DBYOL(pretrain=False, num_classes=3, cls_bn=True, layer_sizes=(2, 1, 1, 1))
    names = {id(mod): n for n, mod in m.named_modules()}
    assert [names[id(b)] for b in m.residual_blocks()] == ["online_net.conv2.block1", "online_net.conv2.blocks.0",
                                                           "online_net.conv3.block1", "online_net.conv4.block1",
                                                           "online_net.conv5.block1"]
    keys = list(m.state_dict().keys())
    with m.regularized((0.5, 7), [None] + [torch.ones(2)] * 4) as inner:
        assert inner._dropout == (0.5, 7) and m.residual_blocks()[1]._drop_scale is not None
        assert m.residual_blocks()[0]._drop_scale is None
    assert m._dropout is None and all(b._drop_scale is None for b in m.residual_blocks())          # nothing outlives the forward
    assert list(m.state_dict().keys()) == keys
    with pytest.raises(ValueError):
        with m.regularized(None, [None]):
            pass
    opts = argparse.Namespace(model_depth=50, sample_size=32, sample_duration=4, sc_type="B", n_classes=3)
    r = R3DBYOL(pretrain=False, cls_bn=True, opts=opts)
    assert len(r.residual_blocks()) == 16 and type(r.residual_blocks()[0]).__name__ == "Bottleneck"


def test_step_refuses_drop_path_where_nothing_can_be_dropped():
    from cstp_amd.regularize import Regularizer
    from cstp_amd.s3dg_byol import S3DGBYOL
    from cstp_amd.train import FineTuneStep
    s3d = S3DGBYOL(pretrain=False, gating=True, slow=False, num_classes=3)
    assert s3d.residual_blocks() == []
    with pytest.raises(ValueError, match="--drop_path"):
        FineTuneStep(s3d, None, "ft_all", regularizer=Regularizer(0.0, 0.1, seed=1))
    FineTuneStep(s3d, None, "ft_all", regularizer=Regularizer(0.5, 0.0, seed=1))                   # dropout alone is served


def test_abi_declared_bound_exported_and_refusing():
    from cstp_amd import _lib
    from test_abi import header_symbols
    names = ("cstp_philox4x32_10", "cstp_dropout", "cstp_droppath_add_relu_forward", "cstp_droppath_add_relu_backward")
    syms = header_symbols()
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert n in syms and n in _lib.SIGNATURES and hasattr(raw, n), n
    assert lib.cstp_abi_version() == 18 and _lib.ABI_VERSION == 18
    one = ctypes.c_void_p(16)
    f = ctypes.c_float
    calls = [
        ("cstp_dropout", (None, None, one, 16, f(0.5), 1, 0), b"null argument"),
        ("cstp_dropout", (None, one, None, 16, f(0.5), 1, 0), b"null argument"),
        ("cstp_dropout", (None, one, one, 0, f(0.5), 1, 0), b"bad size"),
        ("cstp_dropout", (None, one, one, -4, f(0.5), 1, 0), b"bad size"),
        ("cstp_dropout", (None, one, one, 16, f(1.0), 1, 0), b"outside [0, 1)"),
        ("cstp_dropout", (None, one, one, 16, f(-0.25), 1, 0), b"outside [0, 1)"),
        ("cstp_dropout", (None, one, one, 16, f(float("nan")), 1, 0), b"outside [0, 1)"),
        ("cstp_droppath_add_relu_forward", (None, None, one, one, one, 16, 8, 0, None), b"null argument"),
        ("cstp_droppath_add_relu_forward", (None, one, one, None, one, 16, 8, 0, None), b"null argument"),
        ("cstp_droppath_add_relu_forward", (None, one, one, one, one, 0, 8, 0, None), b"bad size"),
        ("cstp_droppath_add_relu_forward", (None, one, one, one, one, 16, 0, 0, None), b"bad size"),
        ("cstp_droppath_add_relu_forward", (None, one, one, one, one, 17, 8, 0, None), b"bad size"),
        ("cstp_droppath_add_relu_forward", (None, one, one, one, one, 16, 8, 1, one), b"fp32 only"),
        ("cstp_droppath_add_relu_backward", (None, None, one, one, one, one, 16, 8, 0), b"null argument"),
        ("cstp_droppath_add_relu_backward", (None, one, one, one, None, None, 16, 8, 0), b"null argument"),
        ("cstp_droppath_add_relu_backward", (None, one, one, one, one, None, -16, 8, 0), b"bad size"),
    ]
    for name, args, needle in calls:
        rc = getattr(lib, name)(*args)
        msg = lib.cstp_last_error()
        assert rc != 0 and needle in msg and b"line" in msg, (name, args, rc, msg)
    assert lib.cstp_philox4x32_10(None, None, None) != 0


def test_ops_refuse_cpu_tensors():
    from cstp_amd import _lib, ops
    x = torch.zeros(2, 3, 2, 4, 4)
    with pytest.raises(_lib.CstpError):
        ops.dropout(x, 0.5, 1)
    with pytest.raises(_lib.CstpError):
        ops.dropout(x, 0.0, 1)                     # even where it would return its input
    with pytest.raises(_lib.CstpError):
        ops.drop_path_add_relu(x, x, torch.ones(2))

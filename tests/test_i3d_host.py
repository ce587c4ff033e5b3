"""I3D-BYOL (cstp_amd/i3d_byol.py) host-side checks, no GPU needed: the state-dict key list and order of the reference (701 keys /
356 parameters for the pre-training wrapper, 343 keys for the fine-tune wrapper), the initialisation RNG stream under
torch.manual_seed(1) (per-tensor checksums captured from the reference, tests/golden/i3d_init.npz), the closed-form spec of the
parity tests, the fine-tune parameter plan, the TensorFlow-SAME pooling geometry against ATen, the refusals and the factory."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import i3d_spec

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _init():
    return np.load(os.path.join(GOLD, "i3d_init.npz"), allow_pickle=False)


def _opts(**kw):
    kw.setdefault("n_classes", 11)
    return types.SimpleNamespace(**kw)


def _checksums(sd):
    return np.stack([np.array([float(v.double().sum()), float(v.double().abs().sum())]) for v in sd.values()])


def _assert_same_tensors(ours, ref):
    """Per-tensor (sum, abs-sum) in fp64: the values are the reference's bit for bit, but the fp64 sums of the checksums are
    reduced in an order that follows the CPU thread count, so they may differ in the last bits (~1e-16 relative).  A different
    draw moves a checksum by O(1) relative to its abs-sum."""
    scale = np.maximum(np.abs(ref[:, 1:2]), 1e-30)
    assert ours.shape == ref.shape
    assert float((np.abs(ours - ref) / scale).max()) < 1e-12


def test_state_dict_keys_match_reference():
    from cstp_amd.i3d_byol import I3DBYOL
    g = _init()
    ref_keys = [str(k) for k in g["state_keys"]]
    assert len(ref_keys) == 701
    m = I3DBYOL(pretrain=True, opts=None)
    assert list(m.state_dict().keys()) == ref_keys
    assert [k for k, _, _ in i3d_spec.model_spec()] == ref_keys
    assert [tuple(v.shape) for v in m.state_dict().values()] == [tuple(s) for _, s, _ in i3d_spec.model_spec()]
    assert len(list(m.parameters())) == int(g["n_params"]) == 356
    assert sum(p.numel() for p in m.online_net.parameters()) == 12287264
    assert "online_net.mixed_3b.branch_1.0.conv3d.weight" in ref_keys
    assert "target_net.mixed_5c.branch_3.1.batch3d.running_mean" in ref_keys
    assert tuple(m.overlap_spa.weight.shape) == (5, 2048) and tuple(m.rot_cls.weight.shape) == (4, 1024)
    assert not hasattr(m, "rotate_cls") and not hasattr(m, "classify")
    ft = I3DBYOL(pretrain=False, opts=_opts())
    ft_keys = list(ft.state_dict().keys())
    assert ft_keys == [str(k) for k in g["ft.state_keys"]] == [k for k, _, _ in i3d_spec.ft_spec(11)]
    assert len(ft_keys) == 343 and ft_keys[-1] == "online_net.conv3d_0c_1x1_custom.conv3d.weight"
    assert tuple(ft.online_net.conv3d_0c_1x1_custom.conv3d.weight.shape) == (11, 1024, 7, 1, 1)
    assert len(list(ft.parameters())) == int(g["ft.n_params"])
    assert not hasattr(ft, "classify") and not hasattr(ft, "cls_bn")


def test_init_stream_matches_reference_checksums():
    """Default nn.Conv3d / nn.Linear draws in construction order, target_net deep-copied BEFORE the Glorot pass over modules(),
    which then re-draws online and target independently."""
    from cstp_amd.i3d_byol import I3DBYOL
    g = _init()
    torch.manual_seed(1)
    m = I3DBYOL(pretrain=True, opts=None)
    _assert_same_tensors(_checksums(m.state_dict()), g["state_cs"])
    sd = m.state_dict()
    assert not torch.equal(sd["online_net.conv3d_2b_1x1.conv3d.weight"], sd["target_net.conv3d_2b_1x1.conv3d.weight"])
    assert not torch.equal(sd["online_net.mixed_4d.branch_0.batch3d.weight"], sd["target_net.mixed_4d.branch_0.batch3d.weight"])
    assert all(not p.requires_grad for p in m.target_net.parameters())
    torch.manual_seed(1)
    ft = I3DBYOL(pretrain=False, opts=_opts())
    _assert_same_tensors(_checksums(ft.state_dict()), g["ft.state_cs"])


def test_closed_form_state_loads_strict():
    from cstp_amd.i3d_byol import I3DBYOL
    for model, spec in ((I3DBYOL(pretrain=True, opts=None), i3d_spec.model_spec()),
                        (I3DBYOL(pretrain=False, opts=_opts()), i3d_spec.ft_spec(11))):
        sd = i3d_spec.closed_form(spec)
        res = model.load_state_dict(sd, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        assert all(torch.equal(v, sd[k]) for k, v in model.state_dict().items())


def test_fine_tuning_parameter_plan_matches_reference():
    """ft_begin_index 5 matches names containing 'fc' only: no I3D parameter has one, everything is frozen with lr 0."""
    from cstp_amd.i3d_byol import I3DBYOL, get_fine_tuning_parameters
    g = _init()
    ft = I3DBYOL(pretrain=False, opts=_opts())
    groups = get_fine_tuning_parameters(ft, 5)
    trainable = [n for n, p in ft.named_parameters() if p.requires_grad]
    assert trainable == [str(k) for k in g["ft_fc.trainable"]] == []
    assert [gr.get("lr", -1.0) for gr in groups] == [float(v) for v in g["ft_fc.group_lrs"]]
    assert len(groups) == 172 and all(gr["lr"] == 0.0 for gr in groups)
    ft2 = I3DBYOL(pretrain=False, opts=_opts())
    assert list(get_fine_tuning_parameters(ft2, 0)) == list(ft2.parameters())


SAME_CASES = [(n, k, s) for n in range(1, 18) for k, s in ((1, 1), (2, 2), (3, 1), (3, 2))]


def test_same_pool_geometry_matches_aten():
    """pad split and output length of every (n, k, s) against F.max_pool3d(F.pad(...), ceil_mode=True); the library's own
    cstp_maxpool3d_same_out agrees."""
    from cstp_amd import _lib, ops
    lib = _lib.load()
    assert len(SAME_CASES) == 68
    for n, k, s in SAME_CASES:
        front, back, out = ops.same_pool_geometry(n, k, s)
        assert front + back == max(k - s, 0) and front == max(k - s, 0) // 2
        x = torch.zeros(1, 1, n, 1, 1)
        y = F.max_pool3d(F.pad(x, (0, 0, 0, 0, front, back)), (k, 1, 1), (s, 1, 1), ceil_mode=True)
        assert y.shape[2] == out, (n, k, s, out, tuple(y.shape))
        assert lib.cstp_maxpool3d_same_out(n, k, s) == out
    with pytest.raises(ValueError):
        ops.same_pool_geometry(0, 3, 1)


def test_same_padding_zero_is_a_candidate_in_the_reference_semantics():
    """What the kernel has to reproduce: an all-negative input through the padded 3x3x3 / stride 1 pool has maximum 0 (a padding
    zero wins at the border) and the border windows drop their gradient."""
    from cstp_amd.i3d_byol import MaxPool3dTFPadding, get_padding_shape
    assert get_padding_shape((3, 3, 3), (1, 1, 1)) == (1, 1, 1, 1, 1, 1)
    assert get_padding_shape((1, 3, 3), (1, 2, 2)) == (0, 1, 0, 1, 0, 0)
    assert get_padding_shape((7, 7, 7), (2, 2, 2)) == (2, 3, 2, 3, 2, 3)
    assert get_padding_shape((2, 2, 2), (2, 2, 2)) == (0, 0, 0, 0, 0, 0)
    pool = MaxPool3dTFPadding((3, 3, 3), (1, 1, 1))
    x = (-torch.rand(1, 1, 3, 3, 3) - 0.5).requires_grad_(True)
    y = F.max_pool3d(F.pad(x, pool.padding_shape), pool.kernel_size, pool.stride, ceil_mode=True)
    assert float(y.detach().max()) == 0.0 and tuple(y.shape) == (1, 1) + pool.out_size((3, 3, 3))
    y.sum().backward()
    assert int((x.grad != 0).sum()) == 1          # only the centre window has no padding in it


def test_final_map_and_clip_checks():
    from cstp_amd.i3d_byol import I3D
    enc = I3D(with_classifier=False)
    assert enc.final_map((16, 112, 112)) == (2, 4, 4)
    assert enc.final_map((16, 224, 224)) == (2, 7, 7)
    assert enc.final_map((8, 64, 64)) == (1, 2, 2)
    enc.check_clip((2, 3, 8, 64, 64))
    with pytest.raises(ValueError, match="too small"):
        enc.check_clip((2, 3, 1, 64, 64))
    with pytest.raises(ValueError, match="3"):
        enc.check_clip((2, 4, 16, 64, 64))
    cls = I3D(num_classes=5, with_classifier=True)
    cls.check_clip((2, 3, 16, 224, 224))
    cls.check_clip((2, 3, 10, 194, 194))       # the smallest clip that still ends in a 2 x 7 x 7 map
    assert cls.final_map((10, 194, 194)) == (2, 7, 7) and cls.final_map((9, 193, 193)) == (1, 6, 6)
    for shape in ((2, 3, 9, 224, 224), (2, 3, 16, 193, 193), (2, 3, 16, 112, 112)):
        with pytest.raises(ValueError, match="too small for the I3D classifier"):
            cls.check_clip(shape)
    with pytest.raises(ValueError, match="7x7"):
        cls.check_clip((2, 3, 16, 256, 256))


def test_refusals():
    from cstp_amd import ops
    from cstp_amd._lib import CstpError
    from cstp_amd.i3d_byol import I3D, I3DBYOL, Unit3Dpy
    with pytest.raises(ValueError, match="fp32"):
        I3DBYOL(pretrain=True, opts=_opts(act_dtype="bf16"))
    m = I3DBYOL(pretrain=True, opts=None)
    z = torch.zeros(1, 3, 16, 112, 112)
    with pytest.raises(NotImplementedError, match="shuffle_bn"):
        m(z, z, o_type="r_byol")
    with pytest.raises(AttributeError, match="classify"):
        m(z, o_type="scratch")
    with pytest.raises(AttributeError, match="pretrain=False"):
        m(z, o_type="ft_all")
    ft = I3DBYOL(pretrain=False, opts=_opts())
    with pytest.raises(AttributeError, match="pretrain=True"):
        ft(z, z, o_type="loss_com")
    with pytest.raises(AttributeError, match="classify"):
        ft(z, o_type="scratch")
    with pytest.raises(ValueError, match="too small for the I3D classifier"):
        ft(z, o_type="ft_all")
    with pytest.raises(NotImplementedError):
        I3D(modality="flow")
    with pytest.raises(ValueError):
        Unit3Dpy(3, 4, padding="FULL")
    x = torch.zeros(2, 4, 2, 3, 3)
    bn = (torch.ones(4), torch.zeros(4), torch.zeros(4), torch.ones(4))
    with pytest.raises(CstpError, match="fp32"):
        ops.bn_relu_concat([x.bfloat16()], [bn])
    with pytest.raises(CstpError, match="HIP device"):
        ops.bn_relu_concat([x], [bn])
    with pytest.raises(CstpError, match="branches"):
        ops.bn_relu_concat([x] * 5, [bn] * 5)
    with pytest.raises(CstpError, match="HIP device"):
        ops.bn_relu_concat_eval([x], [bn])
    with pytest.raises(CstpError, match="fp32"):
        ops.max_pool3d_same(x.bfloat16(), 3, 1)
    with pytest.raises(CstpError, match="HIP device"):
        ops.max_pool3d_same(x, 3, 1)
    with pytest.raises(CstpError, match="HIP device"):
        ops.avg_pool3d_window(x, (1, 2, 2))
    with pytest.raises(CstpError, match="does not fit"):
        ops.avg_pool3d_window(x, (3, 2, 2))


def test_factory_builds_i3d_byol():
    """generate_model(model_name='i3d_byol') is served: without a GPU it stops at the device check (RuntimeError), not at the
    backbone check (ValueError); ft_fc and scratch are refused with the reason; c3d_byol stays refused."""
    from cstp_amd.model import generate_model
    from cstp_amd.opts import parse_opts
    with pytest.raises(ValueError, match="nothing to train"):
        generate_model(parse_opts(["--model_name", "i3d_byol", "--task", "ft_fc"]))
    with pytest.raises(ValueError, match="scratch"):
        generate_model(parse_opts(["--model_name", "i3d_byol", "--task", "scratch"]))
    with pytest.raises(ValueError, match="i3d_byol"):
        generate_model(parse_opts(["--model_name", "c3d_byol", "--task", "loss_com"]))
    o = parse_opts(["--model_name", "i3d_byol", "--task", "loss_com", "--act_dtype", "bf16"])
    if not torch.cuda.is_available():
        for task in ("loss_com", "ft_all", "test", "resume"):
            with pytest.raises(RuntimeError, match="HIP device"):
                generate_model(parse_opts(["--model_name", "i3d_byol", "--task", task]))
        with pytest.raises(RuntimeError, match="HIP device"):
            generate_model(o)
    else:
        with pytest.raises(ValueError, match="fp32"):
            generate_model(o)

"""S3D-G-BYOL (cstp_amd/s3dg_byol.py) host-side checks, no GPU needed: the state-dict key list and order of the reference (2 199
keys with the stage Sequentials' aliases), the initialisation RNG stream under torch.manual_seed(1) (per-tensor checksums captured
from the reference, tests/golden/s3dg_init.npz), the closed-form spec of the parity tests, the fine-tune parameter plan, and the
refusals."""
import os

import numpy as np
import pytest
import torch

import s3dg_spec

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _init():
    return np.load(os.path.join(GOLD, "s3dg_init.npz"), allow_pickle=False)


def _checksums(sd):
    return np.stack([np.array([float(v.double().sum()), float(v.double().abs().sum())]) for v in sd.values()])


def _assert_same_tensors(ours, ref):
    """Per-tensor (sum, abs-sum) in fp64: the values are the reference's bit for bit, but the fp64 sums of the checksums are
    reduced in an order that follows the CPU thread count, so they may differ in the last bits (~1e-16 relative).  A different
    draw moves a checksum by O(1) relative to its abs-sum."""
    scale = np.maximum(np.abs(ref[:, 1:2]), 1e-30)
    assert ours.shape == ref.shape
    assert float((np.abs(ours - ref) / scale).max()) < 1e-12


def test_state_dict_keys_match_reference_with_aliases():
    from cstp_amd.s3dg_byol import S3DGBYOL
    g = _init()
    ref_keys = [str(k) for k in g["state_keys"]]
    assert len(ref_keys) == 2199
    m = S3DGBYOL(pretrain=True, gating=True, slow=False, num_classes=101)
    assert list(m.state_dict().keys()) == ref_keys
    assert [k for k, _, _ in s3dg_spec.model_spec()] == ref_keys
    assert len(list(m.parameters())) == int(g["n_params"]) == 648
    # the aliases are the same objects, not copies
    assert m.online_net.block1[0] is m.online_net.Conv_1a and m.online_net.block3[1] is m.online_net.Mixed_3b
    ft = S3DGBYOL(pretrain=False, gating=True, slow=False, num_classes=11)
    assert list(ft.state_dict().keys()) == [str(k) for k in g["ft.state_keys"]] == [k for k, _, _ in s3dg_spec.ft_spec(11)]


def test_init_stream_matches_reference_checksums():
    """N(0, 0.01) conv draws after the default init, then the Glorot pass over the de-duplicated modules(); target_net built
    on its own (its weights differ from online_net's)."""
    from cstp_amd.s3dg_byol import S3DGBYOL
    g = _init()
    torch.manual_seed(1)
    m = S3DGBYOL(pretrain=True, gating=True, slow=False, num_classes=101)
    _assert_same_tensors(_checksums(m.state_dict()), g["state_cs"])
    sd = m.state_dict()
    assert not torch.equal(sd["online_net.Conv_2b.conv.weight"], sd["target_net.Conv_2b.conv.weight"])
    torch.manual_seed(1)
    ft = S3DGBYOL(pretrain=False, gating=True, slow=False, num_classes=11)
    _assert_same_tensors(_checksums(ft.state_dict()), g["ft.state_cs"])


def test_closed_form_aliases_share_values_and_load():
    from cstp_amd.s3dg_byol import S3DGBYOL
    spec = s3dg_spec.model_spec()
    sd = s3dg_spec.closed_form(spec)
    assert s3dg_spec.canonical("target_net.block4.3.branch1.1.conv2.weight") == "target_net.Mixed_4d.branch1.1.conv2.weight"
    assert torch.equal(sd["online_net.block1.0.conv1.weight"], sd["online_net.Conv_1a.conv1.weight"])
    assert torch.equal(sd["online_net.block5.2.gating_b3.fc.bias"], sd["online_net.Mixed_5c.gating_b3.fc.bias"])
    m = S3DGBYOL(pretrain=True, gating=True, slow=False, num_classes=101)
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())


def test_fine_tuning_parameter_plan_matches_reference():
    """ft_fc (ft_begin_index 5): the substring match of s3dg.py:11-36 keeps classify_bn trainable too."""
    from cstp_amd.s3dg_byol import S3DGBYOL, get_fine_tuning_parameters
    g = _init()
    ft = S3DGBYOL(pretrain=False, gating=True, slow=False, num_classes=11)
    groups = get_fine_tuning_parameters(ft, 5)
    trainable = [n for n, p in ft.named_parameters() if p.requires_grad]
    assert trainable == [str(k) for k in g["ft_fc.trainable"]]
    assert "classify_bn.weight" in trainable and "classify_bn.bias" in trainable
    assert [gr.get("lr", -1.0) for gr in groups] == [float(v) for v in g["ft_fc.group_lrs"]]
    ft2 = S3DGBYOL(pretrain=False, gating=True, slow=False, num_classes=11)
    assert list(get_fine_tuning_parameters(ft2, 0)) == list(ft2.parameters())


def test_refusals():
    from cstp_amd import ops
    from cstp_amd._lib import CstpError
    from cstp_amd.s3dg_byol import S3D, S3DGBYOL
    with pytest.raises(ValueError, match="fp32"):
        S3DGBYOL(pretrain=True, gating=True, slow=False, num_classes=101, act_dtype="bf16")
    m = S3DGBYOL(pretrain=True, gating=True, slow=False, num_classes=101)
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 3, 16, 112, 112), torch.zeros(1, 3, 16, 112, 112), o_type="r_byol")
    net = S3D(gating=True)
    net.check_clip((2, 3, 16, 112, 112))
    net.check_clip((2, 3, 5, 17, 17))
    for shape in ((2, 3, 4, 112, 112), (2, 3, 16, 16, 16)):
        with pytest.raises(ValueError, match="too small"):
            net.check_clip(shape)
    with pytest.raises(NotImplementedError):
        S3D(gating=False)
    x = torch.zeros(2, 4, 2, 3, 3)
    w, b = torch.zeros(4, 4), torch.zeros(4)
    with pytest.raises(CstpError, match="fp32"):
        ops.gate_concat([x.bfloat16()], [(w, b)])
    with pytest.raises(CstpError, match="HIP device"):
        ops.gate_concat([x], [(w, b)])
    with pytest.raises(CstpError, match="branches"):
        ops.gate_concat([x] * 5, [(w, b)] * 5)


def test_factory_builds_s3d_byol():
    """generate_model(model_name='s3d_byol') is served: without a GPU it stops at the device check (RuntimeError), not at the
    backbone check (ValueError); test_colorjit stays refused."""
    from cstp_amd.model import generate_model
    from cstp_amd.opts import parse_opts
    o = parse_opts(["--model_name", "s3d_byol", "--task", "test_colorjit"])
    with pytest.raises(ValueError):
        generate_model(o)
    o = parse_opts(["--model_name", "s3d_byol", "--task", "loss_com", "--act_dtype", "bf16"])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            generate_model(o)
        o = parse_opts(["--model_name", "s3d_byol", "--task", "loss_com"])
        with pytest.raises(RuntimeError, match="HIP device"):
            generate_model(o)
    else:
        with pytest.raises(ValueError, match="fp32"):
            generate_model(o)

"""State-dict spec of the I3D-BYOL wrappers (models/BE/i3d_byol.py as models/model.py:66-71 builds them for i3d_byol) as
(key, shape, kind) triples in the reference's state_dict() order, for the closed-form weights of the parity tests
(oracle.r3d_byol_oracle.closed_form_state).  Needs neither the reference nor a GPU.  No key is aliased here.
"""
from collections import OrderedDict

# (in_channels, [b0, b1a, b1b, b2a, b2b, b3b]) per Mixed block, i3d_byol.py:272-290
MIXED = OrderedDict([
    ("mixed_3b", (192, [64, 96, 128, 16, 32, 32])),
    ("mixed_3c", (256, [128, 128, 192, 32, 96, 64])),
    ("mixed_4b", (480, [192, 96, 208, 16, 48, 64])),
    ("mixed_4c", (512, [160, 112, 224, 24, 64, 64])),
    ("mixed_4d", (512, [128, 128, 256, 24, 64, 64])),
    ("mixed_4e", (512, [112, 144, 288, 32, 64, 64])),
    ("mixed_4f", (528, [256, 160, 320, 32, 128, 128])),
    ("mixed_5b", (832, [256, 160, 320, 32, 128, 128])),
    ("mixed_5c", (832, [384, 192, 384, 48, 128, 128])),
])


def _bn(prefix, c):
    return [(prefix + ".weight", (c,), "bn_w"), (prefix + ".bias", (c,), "bn_b"), (prefix + ".running_mean", (c,), "buf_mean"),
            (prefix + ".running_var", (c,), "buf_var"), (prefix + ".num_batches_tracked", (), "buf_nbt")]


def _unit(prefix, cin, cout, k):
    return [(prefix + ".conv3d.weight", (cout, cin) + tuple(k), "conv_w")] + _bn(prefix + ".batch3d", cout)


def _mixed(prefix, cin, planes):
    b0, b1a, b1b, b2a, b2b, b3b = planes
    spec = _unit(prefix + ".branch_0", cin, b0, (1, 1, 1))
    spec += _unit(prefix + ".branch_1.0", cin, b1a, (1, 1, 1)) + _unit(prefix + ".branch_1.1", b1a, b1b, (3, 3, 3))
    spec += _unit(prefix + ".branch_2.0", cin, b2a, (1, 1, 1)) + _unit(prefix + ".branch_2.1", b2a, b2b, (3, 3, 3))
    spec += _unit(prefix + ".branch_3.1", cin, b3b, (1, 1, 1))
    return spec


def _mlp(prefix, din, dhid, dout):
    return ([(prefix + ".0.weight", (dhid, din), "lin_w"), (prefix + ".0.bias", (dhid,), "lin_b")] + _bn(prefix + ".1", dhid)
            + [(prefix + ".3.weight", (dout, dhid), "lin_w"), (prefix + ".3.bias", (dout,), "lin_b")])


def encoder_spec(prefix, num_classes=None):
    spec = _unit("conv3d_1a_7x7", 3, 64, (7, 7, 7)) + _unit("conv3d_2b_1x1", 64, 64, (1, 1, 1))
    spec += _unit("conv3d_2c_3x3", 64, 192, (3, 3, 3))
    for name, (cin, planes) in MIXED.items():
        spec += _mixed(name, cin, planes)
    if num_classes is not None:
        spec += [("conv3d_0c_1x1_custom.conv3d.weight", (num_classes, 1024, 7, 1, 1), "conv_w")]
    return [(prefix + "." + k, shape, kind) for k, shape, kind in spec]


def model_spec():
    spec = encoder_spec("online_net") + encoder_spec("target_net")
    spec += _mlp("predictor.net", 1024, 4096, 1024)
    for name, din, dout in (("overlap_spa", 2048, 5), ("overlap_tem", 2048, 5), ("pb_cls", 1024, 4), ("rot_cls", 1024, 4)):
        spec += [(name + ".weight", (dout, din), "lin_w"), (name + ".bias", (dout,), "lin_b")]
    return spec


def ft_spec(num_classes):
    return encoder_spec("online_net", num_classes)


def closed_form(spec, dtype=None):
    """OrderedDict key -> tensor for every key of ``spec`` (oracle.r3d_byol_oracle.closed_form_state)."""
    import torch
    from oracle import r3d_byol_oracle as r3d
    return r3d.closed_form_state(list(spec), dtype or torch.float32)

"""State-dict spec of the S3D-G-BYOL wrapper (models/coclr/s3dg.py as models/model.py builds it for s3d_byol: gating=True,
slow=False) as (key, shape, kind) triples in the reference's state_dict() order, for the closed-form weights of the parity tests
(oracle.r3d_byol_oracle.closed_form_state).  Needs neither the reference nor a GPU.

S3D registers its stage Sequentials over the same module objects (``block1 = nn.Sequential(self.Conv_1a)``, ``block3 =
nn.Sequential(self.MaxPool_3a, self.Mixed_3b, self.Mixed_3c)``, ...), so every tensor of those modules appears twice in the state
dict.  ``canonical(key)`` maps the second (alias) name to the first; ``closed_form(spec)`` draws each tensor under its canonical name
and copies it to the alias, so both names hold the same values and ``load_state_dict`` keeps them whichever it writes last.
"""
from collections import OrderedDict

import torch

# (in_planes, [b0, b1a, b1b, b2a, b2b, b3b]) per SepInception, s3dg.py:197-240
INCEPTIONS = OrderedDict([
    ("Mixed_3b", (192, [64, 96, 128, 16, 32, 32])),
    ("Mixed_3c", (256, [128, 128, 192, 32, 96, 64])),
    ("Mixed_4b", (480, [192, 96, 208, 16, 48, 64])),
    ("Mixed_4c", (512, [160, 112, 224, 24, 64, 64])),
    ("Mixed_4d", (512, [128, 128, 256, 24, 64, 64])),
    ("Mixed_4e", (512, [112, 144, 288, 32, 64, 64])),
    ("Mixed_4f", (528, [256, 160, 320, 32, 128, 128])),
    ("Mixed_5b", (832, [256, 160, 320, 32, 128, 128])),
    ("Mixed_5c", (832, [384, 192, 384, 48, 128, 128])),
])
# alias prefix -> canonical prefix (inside one S3D)
ALIASES = OrderedDict([("block1.0", "Conv_1a"), ("block2.1", "Conv_2b"), ("block2.2", "Conv_2c"),
                       ("block3.1", "Mixed_3b"), ("block3.2", "Mixed_3c"),
                       ("block4.1", "Mixed_4b"), ("block4.2", "Mixed_4c"), ("block4.3", "Mixed_4d"), ("block4.4", "Mixed_4e"),
                       ("block4.5", "Mixed_4f"), ("block5.1", "Mixed_5b"), ("block5.2", "Mixed_5c")])
# which named modules each stage Sequential repeats, in the order S3D.__init__ registers them
STAGES = [("Conv_1a",), ("Conv_2b", "Conv_2c"), ("Mixed_3b", "Mixed_3c"),
          ("Mixed_4b", "Mixed_4c", "Mixed_4d", "Mixed_4e", "Mixed_4f"), ("Mixed_5b", "Mixed_5c")]


def _bn(prefix, c):
    return [(prefix + ".weight", (c,), "bn_w"), (prefix + ".bias", (c,), "bn_b"), (prefix + ".running_mean", (c,), "buf_mean"),
            (prefix + ".running_var", (c,), "buf_var"), (prefix + ".num_batches_tracked", (), "buf_nbt")]


def _basic(prefix, cin, cout):
    return [(prefix + ".conv.weight", (cout, cin, 1, 1, 1), "conv_w")] + _bn(prefix + ".bn", cout)


def _stconv(prefix, cin, cout, k):
    return ([(prefix + ".conv1.weight", (cout, cin, 1, k, k), "conv_w"), (prefix + ".conv2.weight", (cout, cout, k, 1, 1), "conv_w")]
            + _bn(prefix + ".bn1", cout) + _bn(prefix + ".bn2", cout))


def _inception(prefix, cin, planes):
    b0, b1a, b1b, b2a, b2b, b3b = planes
    spec = _basic(prefix + ".branch0.0", cin, b0)
    spec += _basic(prefix + ".branch1.0", cin, b1a) + _stconv(prefix + ".branch1.1", b1a, b1b, 3)
    spec += _basic(prefix + ".branch2.0", cin, b2a) + _stconv(prefix + ".branch2.1", b2a, b2b, 3)
    spec += _basic(prefix + ".branch3.1", cin, b3b)
    for i, c in enumerate((b0, b1b, b2b, b3b)):
        spec += [("%s.gating_b%d.fc.weight" % (prefix, i), (c, c), "lin_w"), ("%s.gating_b%d.fc.bias" % (prefix, i), (c,), "lin_b")]
    return spec


def _mlp(prefix, din, dhid, dout):
    return ([(prefix + ".0.weight", (dhid, din), "lin_w"), (prefix + ".0.bias", (dhid,), "lin_b")] + _bn(prefix + ".1", dhid)
            + [(prefix + ".3.weight", (dout, dhid), "lin_w"), (prefix + ".3.bias", (dout,), "lin_b")])


def encoder_spec(prefix, proj):
    named = OrderedDict()
    named["Conv_1a"] = _stconv("Conv_1a", 3, 64, 7)
    named["Conv_2b"] = _basic("Conv_2b", 64, 64)
    named["Conv_2c"] = _stconv("Conv_2c", 64, 192, 3)
    for name, (cin, planes) in INCEPTIONS.items():
        named[name] = _inception(name, cin, planes)
    spec = []
    for si, members in enumerate(STAGES):
        for name in members:
            spec += named[name]
        for j, name in enumerate(members):
            idx = j if si == 0 else j + 1                   # block2..5 start with their MaxPool (index 0, no state)
            spec += [("block%d.%d%s" % (si + 1, idx, k[len(name):]), shape, kind) for k, shape, kind in named[name]]
    if proj:
        spec += _mlp("project.net", 1024, 1024, 1024)
    return [(prefix + "." + k, shape, kind) for k, shape, kind in spec]


def model_spec():
    spec = encoder_spec("online_net", True) + encoder_spec("target_net", True)
    spec += _mlp("predictor.net", 1024, 4096, 1024)
    for name, din in (("overlap_spa", 2048), ("overlap_tem", 2048), ("pb_cls", 1024), ("rotate_cls", 1024)):
        spec += _mlp(name, din, din, 5)
    return spec


def ft_spec(num_classes):
    return (encoder_spec("online_net", False) + [("classify.weight", (num_classes, 1024), "lin_w"),
                                                 ("classify.bias", (num_classes,), "lin_b")] + _bn("classify_bn", 1024))


def canonical(key):
    """The first name under which S3D registers the tensor ``key`` names."""
    for net in ("online_net.", "target_net.", ""):
        if key.startswith(net):
            rest = key[len(net):]
            for alias, canon in ALIASES.items():
                if rest.startswith(alias + "."):
                    return net + canon + rest[len(alias):]
            break
    return key


def closed_form(spec, dtype=torch.float32):
    """OrderedDict key -> tensor for every key of ``spec``: canonical keys drawn by oracle.r3d_byol_oracle.closed_form_state,
    alias keys copies of their canonical tensor."""
    from oracle import r3d_byol_oracle as r3d
    canon = r3d.closed_form_state([e for e in spec if canonical(e[0]) == e[0]], dtype)
    return OrderedDict((k, canon[canonical(k)].clone()) for k, _, _ in spec)

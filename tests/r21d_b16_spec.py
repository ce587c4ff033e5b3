"""TEST INFRASTRUCTURE ONLY -- the bf16-storage spec of R(2+1)D-BYOL (``R21DBYOL(act_dtype="bf16")``), restated on the CPU.

The structure is oracle/r21d_byol_oracle.py's (st_conv / res_block / encoder_forward, the same state dict and clips); the
rounding points are oracle/r3d_byol_oracle.py's (``_RoundBoth`` where a tensor is written, ``_RoundGrad`` where a consumer's
backward writes its gradient, ``_RoundValue`` for the weights at use), imported, not copied.  They are those of the 3D-ResNet
 plus one: the bf16 path materialises the mid-channel BatchNorm+ReLU output of every (2+1)D convolution (spatial
conv -> BN+ReLU -> temporal conv), so the spec rounds it too.  The residual joins follow the product's ops.GradJoin: each of the
two gradients is rounded where its consumer writes it and their sum once more (autograd's bf16 add).

``storage("bf16")`` swaps this encoder into the oracle for the duration of a ``with`` block, so that the oracle's own
model_forward / train_step (losses, heads, EMA, clipping, SGD in the state's dtype) run on it unchanged; ``storage(None)``
runs the restated encoder without any rounding, which must be the oracle itself.
"""
from __future__ import annotations

import contextlib

import torch
import torch.nn.functional as F

from oracle import r21d_byol_oracle as orc
from oracle import r3d_byol_oracle as r3d

_bn = orc._bn
_conv, _in, _out = r3d._conv, r3d._in, r3d._out


def st_conv(sd, prefix, x, k, stride, pad, training=True):
    """spatial 1xkxk conv -> BN -> ReLU (bf16: materialised, rounded once) -> temporal tx1x1 conv."""
    x = _conv(x, sd[prefix + ".spatial_conv.weight"], (1, stride[1], stride[2]), (0, pad[1], pad[2]))
    x = _out(F.relu(_bn(sd, prefix + ".bn", _in(x), training)))
    return _conv(x, sd[prefix + ".temporal_conv.weight"], (stride[0], 1, 1), (pad[0], 0, 0))


def res_block(sd, prefix, x, downsample, training=True):
    s = (2, 2, 2) if downsample else (1, 1, 1)
    res = st_conv(sd, prefix + ".conv1", x, (3, 3, 3), s, (1, 1, 1), training)
    res = _out(F.relu(_bn(sd, prefix + ".bn1", _in(res), training)))
    res = st_conv(sd, prefix + ".conv2", res, (3, 3, 3), (1, 1, 1), (1, 1, 1), training)
    res = _bn(sd, prefix + ".bn2", _in(res), training)
    if downsample:
        x = st_conv(sd, prefix + ".downsampleconv", x, (1, 1, 1), (2, 2, 2), (0, 0, 0), training)
        x = _out(_bn(sd, prefix + ".downsamplebn", _in(x), training))
    return _out(F.relu(_in(x) + res))              # BN + residual + ReLU is ONE kernel: rounded once, behind the activation


def encoder_forward(sd, prefix, x, layer_sizes, training=True, proj=True):
    if r3d._storage["kind"] == "bf16":
        x = r3d._bf(x)                             # the clip is rounded once
    x = st_conv(sd, prefix + ".conv1", x, (3, 7, 7), (1, 2, 2), (1, 3, 3), training)
    x = _out(F.relu(_bn(sd, prefix + ".bn1", _in(x), training)))
    for li, n in enumerate(layer_sizes):
        lp = "%s.conv%d" % (prefix, li + 2)
        x = res_block(sd, lp + ".block1", x, li > 0, training)
        for bi in range(n - 1):
            x = res_block(sd, "%s.blocks.%d" % (lp, bi), x, False, training)
    feat = _in(x).mean(dim=(2, 3, 4)).view(-1, 512)   # pooled features are fp32 (their gradient is written in bf16)
    if not proj:
        return feat
    return feat, orc.mlp(sd, prefix + ".project.net", feat, training)


@contextlib.contextmanager
def storage(kind):
    """Run the oracle (orc.model_forward / orc.train_step) on this encoder with ``kind`` storage (None / "fp32" / "bf16")."""
    saved = orc.encoder_forward
    r3d.set_storage(kind)
    orc.encoder_forward = encoder_forward
    try:
        yield
    finally:
        orc.encoder_forward = saved
        r3d.set_storage(None)


def ft_forward(sd, x, layer_sizes, training=True):
    """The fine-tune / test wrapper (o_type 'ft_all' / 'test'): encoder -> F.normalize -> cls_bn -> classify."""
    f = encoder_forward(sd, "online_net", x, layer_sizes, training, proj=False)
    f = _bn(sd, "cls_bn", F.normalize(f, p=2, dim=1), training)
    return F.linear(f, sd["classify.weight"], sd["classify.bias"])


def train_step(sd, x1, x2, labels, layer_sizes, kind, lr=0.05, wd=5e-4, loss_weight=(0.1, 1.0, 1.0, 1.0, 1.0)):
    """One oracle optimisation step (SGD momentum 0.9, clipping on) with ``kind`` storage; ``sd`` is copied, not mutated."""
    sd = {k: v.clone() for k, v in sd.items()}
    with storage(kind):
        return orc.train_step(sd, {}, x1, x2, labels, layer_sizes, lr, 0.9, wd, loss_weight, True)


def to64(sd):
    return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}


def rel(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))

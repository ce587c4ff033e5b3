"""TEST INFRASTRUCTURE ONLY -- restatements of the fine-tuning regularisers in numpy / stock PyTorch:
Philox4x32-10 and the dropout mask of cstp_dropout, the stochastic-depth join in fp64, and the R3D / R(2+1)D fine-tune forwards
with both operations inserted.  The model forwards are assembled from the functional oracles' own pieces (convolutions,
BatchNorm, the (2+1)D convolution), which this module imports and never modifies; with dropout off and every scale 1 they
compute the oracles' ft_forward bit for bit (tests/test_reg_host.py).  Nothing in cstp_amd imports this file."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import r21d_byol_oracle as base
from oracle import r3d_byol_oracle as r3d

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)


def philox4x32_10(ctr, key):
    """ctr: four arrays (or ints) of 32-bit words, key: two ints -> uint32 array [..., 4] (Salmon et al., SC'11)."""
    c = [np.asarray(v, dtype=np.uint64) & M32 for v in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = np.uint64(key[0]) & M32, np.uint64(key[1]) & M32
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c[0], PHILOX_M1 * c[2]          # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return np.stack(c, axis=-1).astype(np.uint32)


def dropout_keep(n, p, seed, offset=0):
    """bool [n]: element e is kept iff u >= p, u = (w >> 8) * 2^-24, w = Philox((e >> 2, offset), seed)[e & 3]; p as fp32."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    w = philox4x32_10((q & M32, q >> np.uint64(32), offset & 0xFFFFFFFF, (offset >> 32) & 0xFFFFFFFF),
                      (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).reshape(-1)[:n]
    u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u >= np.float32(p)


def inv_keep(p):
    """The kernel's scale of a kept element: the fp32 quotient 1 / (1 - p)."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def dropout_fp32(x, p, seed, offset=0):
    """cstp_dropout on a flat fp32 numpy array, bit for bit."""
    x = np.asarray(x, dtype=np.float32)
    return np.where(dropout_keep(x.size, p, seed, offset).reshape(x.shape), x * inv_keep(p), np.float32(0.0)).astype(np.float32)


def dropout_torch(x, p, seed, offset=0):
    """The same on a torch tensor of any float dtype, differentiable (the fp32 scale promoted to x's dtype)."""
    if p == 0:
        return x
    keep = torch.from_numpy(dropout_keep(x.numel(), p, seed, offset)).view(x.shape)
    return torch.where(keep, x * float(inv_keep(p)), torch.zeros((), dtype=x.dtype))


def drop_path_add_relu(z, res, scale):
    """relu(scale[b] * z[b] + res[b]) in the dtype of z (the tests call it in fp64); scale: [B]."""
    s = torch.as_tensor(scale, dtype=z.dtype).view((-1,) + (1,) * (z.dim() - 1))
    return F.relu(s * z + res)


def _join(z, res, scale):
    return F.relu(res + z) if scale is None else drop_path_add_relu(z, res, scale)


# ---- R(2+1)D fine-tune forward (oracle.r21d_ft_oracle.ft_forward with the two operations) -------------------------------------------
def r21d_res_block(sd, prefix, x, downsample, scale, training=True):
    s = (2, 2, 2) if downsample else (1, 1, 1)
    res = base.st_conv(sd, prefix + ".conv1", x, (3, 3, 3), s, (1, 1, 1), training)
    res = F.relu(base._bn(sd, prefix + ".bn1", res, training))
    res = base.st_conv(sd, prefix + ".conv2", res, (3, 3, 3), (1, 1, 1), (1, 1, 1), training)
    res = base._bn(sd, prefix + ".bn2", res, training)
    if downsample:
        x = base.st_conv(sd, prefix + ".downsampleconv", x, (1, 1, 1), (2, 2, 2), (0, 0, 0), training)
        x = base._bn(sd, prefix + ".downsamplebn", x, training)
    return _join(res, x, scale)


def r21d_ft_forward(sd, x, layer_sizes, scales=None, dropout=None, training=True):
    """scales: per residual block in forward order, [B] or None (the block is never dropped); dropout: (p, key) or None."""
    scales = list(scales) if scales is not None else [None] * sum(layer_sizes)
    x = base.st_conv(sd, "online_net.conv1", x, (3, 7, 7), (1, 2, 2), (1, 3, 3), training)
    x = F.relu(base._bn(sd, "online_net.bn1", x, training))
    l = 0
    for li, n in enumerate(layer_sizes):
        lp = "online_net.conv%d" % (li + 2)
        for bi in range(n):
            name = lp + ".block1" if bi == 0 else "%s.blocks.%d" % (lp, bi - 1)
            x = r21d_res_block(sd, name, x, li > 0 and bi == 0, scales[l], training)
            l += 1
    feat = x.mean(dim=(2, 3, 4)).view(-1, 512)
    feat = F.normalize(feat, p=2, dim=1)
    feat = base._bn(sd, "cls_bn", feat, training)
    if dropout is not None and training:
        feat = dropout_torch(feat, dropout[0], dropout[1], 0)
    return F.linear(feat, sd["classify.weight"], sd["classify.bias"])


# ---- 3D-ResNet fine-tune forward (oracle.r3d_byol_oracle.ft_forward with the two operations; BasicBlock depths) -------------------
def r3d_basic_block(sd, prefix, x, stride, scale, training=True):
    out = r3d._conv(x, sd[prefix + ".conv1.weight"], stride, 1)
    out = r3d._out(F.relu(base._bn(sd, prefix + ".bn1", r3d._in(out), training)))
    out = r3d._conv(out, sd[prefix + ".conv2.weight"], 1, 1)
    out = base._bn(sd, prefix + ".bn2", r3d._in(out), training)
    residual = x
    if (prefix + ".downsample.0.weight") in sd:
        residual = r3d._conv(x, sd[prefix + ".downsample.0.weight"], stride, 0)
        residual = r3d._out(base._bn(sd, prefix + ".downsample.1", r3d._in(residual), training))
    if scale is None:
        return r3d._out(F.relu(out + r3d._in(residual)))
    return r3d._out(drop_path_add_relu(r3d._in(r3d._out(out)), r3d._in(residual), scale))     # bn2's output is a tensor of its own


def r3d_ft_forward(sd, x, layers, scales=None, dropout=None, training=True):
    scales = list(scales) if scales is not None else [None] * sum(layers)
    if r3d._storage["kind"] == "bf16":
        x = r3d._bf(x)                              # the clip is rounded once
    x = r3d._conv(x, sd["online_net.conv1.weight"], (1, 2, 2), (3, 3, 3))
    x = r3d._out(F.relu(base._bn(sd, "online_net.bn1", r3d._in(x), training)))
    x = r3d._out(F.max_pool3d(r3d._in(x), 3, 2, 1))
    l = 0
    for li, n in enumerate(layers):
        for bi in range(n):
            x = r3d_basic_block(sd, "online_net.layer%d.%d" % (li + 1, bi), x, 2 if (bi == 0 and li > 0) else 1, scales[l], training)
            l += 1
    feat = r3d._in(x).mean(dim=(2, 3, 4)).flatten(1)
    feat = F.normalize(feat, p=2, dim=1)
    feat = base._bn(sd, "classify_bn", feat, training)
    if dropout is not None and training:
        feat = dropout_torch(feat, dropout[0], dropout[1], 0)
    return F.linear(feat, sd["classify.weight"], sd["classify.bias"])


def plan_scales(plan):
    """The per-block scale rows the step installs for ``plan`` (cstp_amd.regularize.RegPlan): None where p_l is 0."""
    if plan.scale is None:
        return None
    return [torch.from_numpy(plan.scale[l].copy()) if plan.p[l] > 0.0 else None for l in range(len(plan.p))]

"""S3D-G-BYOL for MI355X -- host-side mirror of /root/reference/models/coclr/s3dg.py as models/model.py:54-59 builds it for
``--model_name s3d_byol``: ``S3DGBYOL(pretrain=..., gating=True, slow=False, num_classes=...)``.

Mirrors (same class names, attribute names, state-dict keys, argument meaning and initialisation RNG stream):
  get_fine_tuning_parameters :11-36, BasicConv3d :39-59, STConv3d :62-99 (1xkxk spatial -> BN -> ReLU -> kx1x1 temporal -> BN -> ReLU),
  SelfGating :100-110, SepInception :113-163, S3D :166-262 (the stage Sequentials block1..block5 ALIAS the named modules -- Conv_1a
  is also block1.0, Mixed_3b is also block3.1, ... -- so the state dict lists each of those tensors under two names: 2 199 keys for
  the pre-training wrapper, 648 distinct parameters), Projector / Predictor :251-276, S3DGBYOL :336-538 (o_type 'loss_com'
  :487-511, 'ft_fc' / 'ft_all' / 'test' :526-534, 'scratch' :535-538).
Differences from the R(2+1)D wrapper that the reference makes and this file keeps: target_net is built on its own (NOT a deepcopy:
its initial weights differ from the online network's until the first EMA), every conv weight is drawn N(0, 0.01) after the default
init and then overwritten by the Glorot pass over the de-duplicated modules(), the overlap heads are 2048 -> 2048 -> 5 and the
playback / rotation heads 1024 -> 1024 -> 5 MLPs called once per view, the fine-tune BatchNorm is ``classify_bn`` and 'scratch'
skips the normalisation and that BatchNorm.

All arithmetic runs in the HIP kernels of libcstp_hip.so through cstp_amd.ops.  The four SelfGating modules of an inception block
and the torch.cat behind them are one fused op (ops.gate_concat: two launches forward, three backward, y written straight into
the concat tensor); ``CSTP_S3D_GATE=0`` composes them from the existing ops plus ATen (mean, sigmoid, mul, cat) instead, for a
same-box comparison.  fp32 activations only: ``--act_dtype bf16`` is refused.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from . import ops
from .r21d_byol import (BatchNorm1d, BatchNorm3d, ByolBase, Conv3d, Linear, Predictor, Projector, ReLU,
                        _MLP)

# A/B switch: 0 = self-gating and the inception concat composed from ops.linear + ATen mean / sigmoid / mul / cat
FUSED_GATE = os.environ.get("CSTP_S3D_GATE", "1") != "0"


def get_fine_tuning_parameters(model, ft_begin_index):
    """s3dg.py:11-36.  ft_begin_index 0: every parameter.  Otherwise only parameters whose NAME contains 'layer<i>'
    (i = ft_begin_index..4) or 'classify' stay trainable -- a substring match, so ``classify_bn.*`` is trainable too (S3D has no
    'layer' stages: every non-zero index leaves the classifier and its BatchNorm).  Every other parameter is frozen and listed
    with lr 0.0, one param group per tensor."""
    if ft_begin_index == 0:
        return model.parameters()
    ft_module_names = []
    if ft_begin_index <= 4:
        for i in range(ft_begin_index, 5):
            ft_module_names.append("layer{}".format(i))
        ft_module_names.append("classify")
    else:
        ft_module_names.append("classify")
    print("Modules to finetune : ", ft_module_names)
    parameters = []
    for k, v in model.named_parameters():
        for ft_module in ft_module_names:
            if ft_module in k:
                print("Layers to finetune : ", k)
                parameters.append({"params": v})
                break
        else:
            v.requires_grad = False
            parameters.append({"params": v, "lr": 0.0})
    return parameters


class MaxPool3d(nn.Module):
    """nn.MaxPool3d stand-in (no state): keeps the reference's Sequential indices (block2.0, block3.0, ...)."""

    def __init__(self, kernel_size, stride, padding=0):
        super().__init__()
        self.kernel_size, self.stride, self.padding = kernel_size, stride, padding

    def forward(self, x):
        return ops.max_pool3d(x, self.kernel_size, self.stride, self.padding)


class AdaptiveAvgPool3d(nn.Module):
    """nn.AdaptiveAvgPool3d((1, 1, 1)) + view(-1, C) (no state)."""

    def forward(self, x):
        return ops.global_avg_pool(x)


class BasicConv3d(nn.Module):
    def __init__(self, in_planes, out_planes, kernel_size, stride, padding=0):
        super().__init__()
        self.conv = Conv3d(in_planes, out_planes, kernel_size=kernel_size, stride=stride, padding=padding, bias=False)
        self.bn = BatchNorm3d(out_planes)
        self.relu = ReLU()
        with torch.no_grad():     # :52-54 -- the draw consumes the CPU RNG stream; the Glorot pass overwrites it later
            self.conv.weight.normal_(mean=0, std=0.01)
            self.bn.weight.fill_(1)
            self.bn.bias.zero_()

    def forward(self, x, groups=1):
        return self.bn(self.conv(x), relu=True, groups=groups)


class STConv3d(nn.Module):
    def __init__(self, in_planes, out_planes, kernel_size, stride, padding=0):
        super().__init__()
        if isinstance(stride, tuple):
            t_stride, stride = stride[0], stride[-1]
        else:
            t_stride = stride
        self.conv1 = Conv3d(in_planes, out_planes, kernel_size=(1, kernel_size, kernel_size), stride=(1, stride, stride),
                            padding=(0, padding, padding), bias=False)
        self.conv2 = Conv3d(out_planes, out_planes, kernel_size=(kernel_size, 1, 1), stride=(t_stride, 1, 1),
                            padding=(padding, 0, 0), bias=False)
        self.bn1 = BatchNorm3d(out_planes)
        self.bn2 = BatchNorm3d(out_planes)
        self.relu = ReLU()
        with torch.no_grad():     # :83-90
            self.conv1.weight.normal_(mean=0, std=0.01)
            self.conv2.weight.normal_(mean=0, std=0.01)
            for bn in (self.bn1, self.bn2):
                bn.weight.fill_(1)
                bn.bias.zero_()

    def forward(self, x, groups=1):
        x = self.bn1(self.conv1(x), relu=True, groups=groups)
        return self.bn2(self.conv2(x), relu=True, groups=groups)


class SelfGating(nn.Module):
    def __init__(self, input_dim):
        super().__init__()
        self.fc = Linear(input_dim, input_dim)

    def forward(self, x):
        """The composed form (CSTP_S3D_GATE=0): mean over (D, H, W), fc, sigmoid, broadcast multiply (:106-110)."""
        w = torch.sigmoid(self.fc(x.mean(dim=[2, 3, 4])))
        return w[:, :, None, None, None] * x


class _Branch(nn.Sequential):
    def forward(self, x, groups=1):
        for m in self:
            x = m(x) if isinstance(m, MaxPool3d) else m(x, groups)
        return x


class SepInception(nn.Module):
    def __init__(self, in_planes, out_planes, gating=False):
        super().__init__()
        assert len(out_planes) == 6
        assert isinstance(out_planes, list)
        n0, n1a, n1b, n2a, n2b, n3b = out_planes
        self.branch0 = _Branch(BasicConv3d(in_planes, n0, kernel_size=1, stride=1))
        self.branch1 = _Branch(BasicConv3d(in_planes, n1a, kernel_size=1, stride=1),
                               STConv3d(n1a, n1b, kernel_size=3, stride=1, padding=1))
        self.branch2 = _Branch(BasicConv3d(in_planes, n2a, kernel_size=1, stride=1),
                               STConv3d(n2a, n2b, kernel_size=3, stride=1, padding=1))
        self.branch3 = _Branch(MaxPool3d(kernel_size=(3, 3, 3), stride=1, padding=1),
                               BasicConv3d(in_planes, n3b, kernel_size=1, stride=1))
        self.out_channels = n0 + n1b + n2b + n3b
        self.gating = gating
        if gating:
            self.gating_b0 = SelfGating(n0)
            self.gating_b1 = SelfGating(n1b)
            self.gating_b2 = SelfGating(n2b)
            self.gating_b3 = SelfGating(n3b)

    def forward(self, x, groups=1):
        xs = [self.branch0(x, groups), self.branch1(x, groups), self.branch2(x, groups), self.branch3(x, groups)]
        gates = (self.gating_b0, self.gating_b1, self.gating_b2, self.gating_b3)
        if FUSED_GATE:
            return ops.gate_concat(xs, [(gt.fc.weight, gt.fc.bias) for gt in gates])
        return torch.cat([gt(xi) for gt, xi in zip(gates, xs)], 1)


def _pool_out(size, k, s, p):
    return tuple((n + 2 * pp - kk) // ss + 1 for n, kk, ss, pp in zip(size, k, s, p))


class S3D(nn.Module):
    def __init__(self, input_channel=3, gating=False, slow=False, proj_flag=False):
        super().__init__()
        if not gating:
            raise NotImplementedError("cstp_amd serves S3D-G (gating=True, what models/model.py:54-59 builds for s3d_byol); the "
                                      "ungated S3D of s3d_classify is out of scope")
        self.gating = gating
        self.slow = slow
        if slow:
            self.Conv_1a = STConv3d(input_channel, 64, kernel_size=7, stride=(1, 2, 2), padding=3)
        else:
            self.Conv_1a = STConv3d(input_channel, 64, kernel_size=7, stride=2, padding=3)
        self.block1 = nn.Sequential(self.Conv_1a)
        self.MaxPool_2a = MaxPool3d(kernel_size=(1, 3, 3), stride=(1, 2, 2), padding=(0, 1, 1))
        self.Conv_2b = BasicConv3d(64, 64, kernel_size=1, stride=1)
        self.Conv_2c = STConv3d(64, 192, kernel_size=3, stride=1, padding=1)
        self.block2 = nn.Sequential(self.MaxPool_2a, self.Conv_2b, self.Conv_2c)
        self.MaxPool_3a = MaxPool3d(kernel_size=(1, 3, 3), stride=(1, 2, 2), padding=(0, 1, 1))
        self.Mixed_3b = SepInception(in_planes=192, out_planes=[64, 96, 128, 16, 32, 32], gating=gating)
        self.Mixed_3c = SepInception(in_planes=256, out_planes=[128, 128, 192, 32, 96, 64], gating=gating)
        self.block3 = nn.Sequential(self.MaxPool_3a, self.Mixed_3b, self.Mixed_3c)
        self.MaxPool_4a = MaxPool3d(kernel_size=(3, 3, 3), stride=(2, 2, 2), padding=(1, 1, 1))
        self.Mixed_4b = SepInception(in_planes=480, out_planes=[192, 96, 208, 16, 48, 64], gating=gating)
        self.Mixed_4c = SepInception(in_planes=512, out_planes=[160, 112, 224, 24, 64, 64], gating=gating)
        self.Mixed_4d = SepInception(in_planes=512, out_planes=[128, 128, 256, 24, 64, 64], gating=gating)
        self.Mixed_4e = SepInception(in_planes=512, out_planes=[112, 144, 288, 32, 64, 64], gating=gating)
        self.Mixed_4f = SepInception(in_planes=528, out_planes=[256, 160, 320, 32, 128, 128], gating=gating)
        self.block4 = nn.Sequential(self.MaxPool_4a, self.Mixed_4b, self.Mixed_4c, self.Mixed_4d, self.Mixed_4e, self.Mixed_4f)
        self.MaxPool_5a = MaxPool3d(kernel_size=(2, 2, 2), stride=(2, 2, 2), padding=(0, 0, 0))
        self.Mixed_5b = SepInception(in_planes=832, out_planes=[256, 160, 320, 32, 128, 128], gating=gating)
        self.Mixed_5c = SepInception(in_planes=832, out_planes=[384, 192, 384, 48, 128, 128], gating=gating)
        self.block5 = nn.Sequential(self.MaxPool_5a, self.Mixed_5b, self.Mixed_5c)
        self.avgpooling = AdaptiveAvgPool3d()
        self.proj_flag = proj_flag
        if self.proj_flag:
            self.project = Projector(dim=1024, projection_size=1024, projection_hidden_size=1024)

    def check_clip(self, shape):
        """The five down-sampling stages must leave at least one position: raise a clear error instead of a kernel failure."""
        dhw = tuple(shape[2:])
        c1, c2 = self.Conv_1a.conv1, self.Conv_1a.conv2
        stages = [(c1.kernel_size, c1.stride, c1.padding), (c2.kernel_size, c2.stride, c2.padding)]
        stages += [(p.kernel_size, p.stride, p.padding) for p in (self.MaxPool_2a, self.MaxPool_3a, self.MaxPool_4a, self.MaxPool_5a)]
        for k, s, p in stages:
            t3 = lambda v: (v, v, v) if isinstance(v, int) else tuple(v)  # noqa: E731
            dhw = _pool_out(dhw, t3(k), t3(s), t3(p))
            if min(dhw) < 1:
                raise ValueError("clip %s is too small for S3D-G: its stem and four max-poolings reduce it to nothing "
                                 "(needs at least 5 frames of 17x17 pixels)" % (tuple(shape[1:]),))

    def forward(self, x, groups=1, after_early_stage=None):
        """``groups`` > 1: x holds that many independent forward calls back to back along the batch axis (per-call BN
        statistics).  ``after_early_stage``: called once block2 is enqueued (S3DGBYOL starts the target network's stream there)."""
        self.check_clip(x.shape)
        x = self.Conv_1a(x, groups)
        x = self.Conv_2c(self.Conv_2b(self.MaxPool_2a(x), groups), groups)
        if after_early_stage is not None:
            after_early_stage()
        x = self.MaxPool_3a(x)
        for m in (self.Mixed_3b, self.Mixed_3c):
            x = m(x, groups)
        x = self.MaxPool_4a(x)
        for m in (self.Mixed_4b, self.Mixed_4c, self.Mixed_4d, self.Mixed_4e, self.Mixed_4f):
            x = m(x, groups)
        x = self.MaxPool_5a(x)
        for m in (self.Mixed_5b, self.Mixed_5c):
            x = m(x, groups)
        x = self.avgpooling(x)
        if self.proj_flag:
            return x, self.project(x, groups)
        return x


class S3DGBYOL(ByolBase):
    """forward(x1, x2, o_type='loss_com') -> (loss_byol, (pred_spa, pred_tem, pred_pb_1, pred_pb_2, pred_rot_1, pred_rot_2)),
    every logit [B, 5] (s3dg.py:487-511)."""

    def __init__(self, momentum=0.996, pretrain=True, classify_bn=True, shuffle_bn=False, act_dtype="fp32", **kwargs):
        super().__init__()
        act = act_dtype or "fp32"
        if act != "fp32":
            raise ValueError("--act_dtype %r: s3d_byol runs fp32 activations only (bf16 storage is served for r21d_byol / r3d_byol)"
                             % (act_dtype,))
        self.pretrain = bool(pretrain)
        gating, slow = kwargs.get("gating", True), kwargs.get("slow", False)
        if pretrain:
            self.momentum = momentum
            self.online_net = S3D(gating=gating, slow=slow, proj_flag=True)
            self.target_net = S3D(gating=gating, slow=slow, proj_flag=True)      # built, not copied (:341)
            self.predictor = Predictor(dim=1024, prediction_size=1024, prediction_hidden_size=4096)
            self._set_grad(self.target_net, False)
            self.overlap_spa = _MLP(2048, 2048, 5)
            self.overlap_tem = _MLP(2048, 2048, 5)
            self.pb_cls = _MLP(1024, 1024, 5)
            self.rotate_cls = _MLP(1024, 1024, 5)
        else:
            self.online_net = S3D(gating=gating, slow=slow, proj_flag=False)
            self.classify = Linear(1024, kwargs["num_classes"])
            if classify_bn:
                print("classify_bn is true, Feature norm and Batch norm on final features")
                self.classify_bn = BatchNorm1d(1024)
                self.l2_norm = True
            else:
                self.l2_norm = False
        self._glorot_all((Linear, Conv3d, BatchNorm1d, BatchNorm3d))      # :370-380 over the de-duplicated modules()
        self._arenas = None

    def _head_bn_calls(self):
        # forward() calls per step: predictor x2, overlap_spa x1, overlap_tem x1, pb_cls x2, rotate_cls x2 (the projector is
        # inside online_net / target_net and counted with them)
        return [(self.predictor, 2), (self.overlap_spa, 1), (self.overlap_tem, 1), (self.pb_cls, 2), (self.rotate_cls, 2)]

    def forward(self, x1, x2=None, o_type="r_byol"):
        if o_type == "loss_com":
            return self._two_view_step(x1, x2)
        if o_type == "r_byol":
            raise NotImplementedError("o_type='r_byol' is shape-broken in the reference (the predictor is fed the (feature, "
                                      "projection) tuple, s3dg.py:514-518); use o_type='loss_com'")
        if o_type in ["ft_fc", "ft_all", "test", "scratch"]:
            if self.pretrain:
                raise AttributeError("S3DGBYOL(pretrain=True) has no classify: o_type=%r needs pretrain=False" % o_type)
            return self._normed_classify(self.online_net(x1), o_type, self.l2_norm)     # :526-534 vs :535-538
        return None     # the reference falls off the end of forward for any other o_type

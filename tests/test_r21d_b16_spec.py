"""The bf16-storage spec of R(2+1)D-BYOL (tests/r21d_b16_spec.py) on the CPU: with rounding off it IS the oracle; with rounding
on, its distance from the reference's fp64 goldens is the price of bf16 storage itself -- measured and printed here, and the
basis of the bars of tests/test_r21d_b16_gpu.py's golden test.  CPU only."""
import os

import numpy as np
import pytest
import torch

import r21d_b16_spec as spec
from oracle import r21d_byol_oracle as orc

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_spec_without_rounding_is_the_oracle():
    g = np.load(os.path.join(GOLD, "r18_small.npz"), allow_pickle=False)
    depth, b, t, hw, _ = [int(v) for v in g["meta"]]
    ls = orc.layer_sizes_for_depth(depth)
    sd = orc.closed_form_state(ls, torch.float32)
    x1, x2, labels = orc.closed_form_clips(b, t, hw, torch.float32)
    want = orc.train_step({k: v.clone() for k, v in sd.items()}, {}, x1, x2, labels, ls, 0.05, 0.9, 5e-4, (0.1, 1.0, 1.0, 1.0, 1.0), True)
    got = spec.train_step(sd, x1, x2, labels, ls, None)
    assert orc.encoder_forward is not spec.encoder_forward           # the swap is undone
    for k in ("loss_byol", "loss_total", "grad_norm"):
        assert torch.equal(got[k], want[k]), k
    assert all(torch.equal(a, c) for a, c in zip(got["logits"], want["logits"]))
    assert all(torch.equal(got["grads"][k], want["grads"][k]) for k in want["grads"])


def test_spec_with_rounding_rounds_the_mid_tensor():
    """bf16 storage changes the result, and every stored 5-D activation of the restated encoder is a bf16 value -- the
    mid-channel BatchNorm+ReLU output included."""
    ls = (1, 1, 1, 1)
    sd = orc.closed_form_state(ls, torch.float64)
    x1, _, _ = orc.closed_form_clips(2, 4, 32, torch.float64)
    seen = []
    real = spec._out

    def spy(x):
        y = real(x)
        seen.append(y)
        return y
    spec._out = spy
    try:
        with spec.storage("bf16"):
            f16, _ = spec.encoder_forward(spec.to64(sd), "online_net", x1, ls)
    finally:
        spec._out = real
    # stem: mid + bn1; per block: conv1 mid, bn1, conv2 mid, out (+ the downsample's mid and BN in stages 3..5)
    assert len(seen) == 2 + 4 + 3 * 6
    assert all(torch.equal(y, y.to(torch.bfloat16).double()) for y in seen)
    with spec.storage(None):
        f64, _ = spec.encoder_forward(spec.to64(sd), "online_net", x1, ls)
    e = spec.rel(f16, f64)
    assert 1e-5 < e < 0.25, e          # (two clips per BatchNorm group: train-mode statistics amplify every flip)


# measured (this file, fp64 between the rounding points): losses <= 2.1e-3, gradient norm 3.5e-3 / 2.0e-2 / 3.6e-3, logits
# 2.5e-2 / 8.3e-2 / 2.8e-1 for d1 / r18 / r34 -- the logits pass BatchNorm1d heads over four samples, which amplify every flip
LOGITS_PRICE = {"d1_small": 2.5e-2, "r18_small": 8.3e-2, "r34_small": 2.8e-1}


@pytest.mark.parametrize("name", ["d1_small", "r18_small", "r34_small"])
def test_spec_distance_to_the_reference_goldens(name):
    """The spec in fp64 between its rounding points against the reference (fp64, no rounding).  Printed: these numbers set the
    GPU golden test's bars (tests/test_r21d_b16_gpu.py).  Asserted at the measured values plus a quarter: the rounding is
    deterministic, so a change here is a change of the spec."""
    g = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    depth, b, t, hw, _ = [int(v) for v in g["meta"]]
    ls = orc.layer_sizes_for_depth(depth)
    sd = spec.to64(orc.closed_form_state(ls, torch.float32))
    x1, x2, labels = orc.closed_form_clips(b, t, hw, torch.float64)
    info = spec.train_step(sd, x1, x2, labels, ls, "bf16", float(g["lr"]), float(g["wd"]), tuple(g["loss_weight"]))
    e = {"loss_byol": spec.rel(info["loss_byol"], g["s1.loss_byol"]), "loss_total": spec.rel(info["loss_total"], g["s1.loss_total"]),
         "logits": spec.rel(torch.stack(info["logits"]), g["s1.logits"]), "grad_norm": spec.rel(info["grad_norm"], g["s1.grad_norm"])}
    print("%s: bf16-storage spec (fp64 between roundings) vs the reference fp64 golden: %s" % (name, e))
    assert e["loss_byol"] < 2.5e-3 and e["loss_total"] < 2.5e-3 and e["grad_norm"] < 2.5e-2, e
    assert e["logits"] < 1.25 * LOGITS_PRICE[name], e


def test_r21dbyol_act_dtype_argument():
    from cstp_amd.r21d_byol import R21DBYOL
    m = R21DBYOL(pretrain=True, layer_sizes=(1, 1, 1, 1), act_dtype="bf16")
    assert m.act_bf16
    assert not R21DBYOL(pretrain=True, layer_sizes=(1, 1, 1, 1)).act_bf16
    ft = R21DBYOL(pretrain=False, num_classes=11, cls_bn=True, layer_sizes=(1, 1, 1, 1), act_dtype="bf16")
    assert ft.act_bf16
    with pytest.raises(ValueError):
        R21DBYOL(pretrain=True, layer_sizes=(1, 1, 1, 1), act_dtype="fp16")

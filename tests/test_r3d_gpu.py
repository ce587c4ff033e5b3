"""3D-ResNet-BYOL on a real MI355X (HIP kernels through the C ABI): MaxPool3d against PyTorch CPU fp64, the pre-training step
and the fine-tune / test forwards against golden vectors captured from the reference in fp64 (tests/golden/r3d_*.npz), and the
factory + training step end to end.  The loop reads like main_byol.py:60-91."""
import argparse

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from test_oracle_golden import STATE_TOLS, TOLS, cs_err, rel
from test_r3d_oracle_golden import GRAD_SCALE, OUT_SCALE, load

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape,k,s,p", [((2, 5, 6, 9, 11), 3, 2, 1), ((1, 3, 4, 8, 8), 3, 2, 1), ((2, 4, 5, 7, 6), (1, 3, 3), (1, 2, 2), (0, 1, 1)),
                                         ((1, 2, 3, 5, 5), 2, 2, 0), ((2, 3, 7, 7, 7), 3, 1, 1)])
def test_max_pool3d_fwd_bwd(shape, k, s, p):
    from cstp_amd import ops
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1).requires_grad_(True)
    y = F.max_pool3d(x, k, s, p)
    dy = torch.rand(y.shape, generator=g, dtype=torch.float64) * 2 - 1
    y.backward(dy)
    xg = x.detach().float().cuda().requires_grad_(True)
    yg = ops.max_pool3d(xg, k, s, p)
    yg.backward(dy.float().cuda())
    assert tuple(yg.shape) == tuple(y.shape)
    assert rel_err(yg, y) < 1e-6 and rel_err(xg.grad, x.grad) < 1e-6
    # ties: the first maximum in (d, h, w) scan order takes the gradient, as in aten
    xt = torch.zeros((1, 1, 4, 4, 4), dtype=torch.float64, requires_grad=True)
    yt = F.max_pool3d(xt, 3, 2, 1)
    yt.backward(torch.ones_like(yt))
    xtg = torch.zeros((1, 1, 4, 4, 4), device="cuda", requires_grad=True)
    ops.max_pool3d(xtg, 3, 2, 1).backward(torch.ones((1, 1, 2, 2, 2), device="cuda"))
    assert torch.equal(xtg.grad.cpu().double(), xt.grad)


def _opts(depth, t, hw, k=101):
    return argparse.Namespace(model_depth=depth, sample_size=hw, sample_duration=t, sc_type="B", n_classes=k)


# the smallest case also runs with the target forward on the main stream (ByolBase._two_view_step's serial branch); the ids of
# the existing cases are unchanged
GOLDEN_CASES = ["r3d_10_small", "r3d_18_small", "r3d_34_small"]
@pytest.mark.parametrize("name,overlap", [pytest.param(n, True if n == "r3d_10_small" else None, id=n) for n in GOLDEN_CASES]
                         + [pytest.param("r3d_10_small", False, id="r3d_10_small-serial")])
def test_r3d_hip_matches_reference_golden(name, overlap, monkeypatch):
    if overlap is not None:
        from cstp_amd import r21d_byol
        monkeypatch.setattr(r21d_byol, "OVERLAP_TARGET_FORWARD", overlap)
    from cstp_amd import ops
    from cstp_amd.optim import FlatSGD
    from cstp_amd.r3d_byol import R3DBYOL
    from cstp_amd.train import PretrainStep
    from oracle import r21d_byol_oracle as orc
    from oracle import r3d_byol_oracle as r3d
    g = load(name)
    depth, b, t, hw, steps = [int(v) for v in g["meta"]]
    layers = r3d.for_depth(depth)
    sd = r3d.closed_form_state(r3d.model_spec(layers), torch.float32)
    x1, x2, _ = orc.closed_form_clips(b, t, hw, torch.float32)
    lab = {k: v.cuda() for k, v in r3d.closed_form_labels(b).items()}
    keys = [str(k) for k in g["state_keys"]]
    pkeys = [str(k) for k in g["param_keys"]]

    def build():
        m = R3DBYOL(pretrain=True, opts=_opts(depth, t, hw))
        res = m.load_state_dict(sd, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        m.cuda()
        m.flatten_parameters()
        return m.train()

    # forward internals (r3d_byol.py:382-395)
    model = build()
    x1d, x2d = x1.cuda(), x2.cuda()
    tol1 = TOLS[1][0] * OUT_SCALE.get(name, 1.0)
    with torch.no_grad():
        f1, f2 = model.online_net(x1d), model.online_net(x2d)
        p1, p2 = model.predictor(f1), model.predictor(f2)
        model._update_target_net()
        t1, t2 = model.target_net(x1d), model.target_net(x2d)
    for k, v in (("feat_1", f1), ("feat_2", f2), ("pred_1", p1), ("pred_2", p2), ("tfeat_1", t1), ("tfeat_2", t2)):
        assert rel(v.cpu().numpy(), g["fwd." + k]) < tol1, k

    # optimisation steps through the product's own step object (main_byol.py:60-91)
    model = build()
    opt = FlatSGD(model.parameters(), lr=float(g["lr"]), momentum=0.9, weight_decay=float(g["wd"]), arenas=model.flatten_parameters())
    step = PretrainStep(model, opt, tuple(g["loss_weight"]), clip_grad_norm=True)
    for s in range(1, steps + 1):
        tol, gtol = TOLS[s]
        tol *= OUT_SCALE.get(name, 1.0)
        gtol *= GRAD_SCALE.get(name, 1.0)
        pre = "s%d." % s
        out = step(x1d, x2d, lab["spa"], lab["tem"], lab["pb"], lab["rot1"], lab["rot2"])
        assert rel(float(out.loss_byol), g[pre + "loss_byol"]) < tol
        assert rel(float(out.loss_total), g[pre + "loss_total"]) < tol
        assert rel([float(c) for c in out.ce], g[pre + "ce"]) < tol
        assert rel(torch.stack([l.cpu() for l in out.logits[:2]]).numpy(), g[pre + "logits_5"]) < tol
        assert rel(torch.stack([l.cpu() for l in out.logits[2:]]).numpy(), g[pre + "logits_4"]) < tol
        assert rel(float(out.grad_norm), g[pre + "grad_norm"]) < gtol
        st = model.state_dict()
        cs = np.array([[float(st[k].double().sum()), float(st[k].double().abs().sum())] for k in keys])
        assert cs_err(cs, g[pre + "state_cs"]) < STATE_TOLS[s]
        osd = opt.state_dict()["state"]
        # state indices are torch.optim.SGD(model.parameters())'s: the frozen target tensors keep their rows (no state)
        mcs = np.array([[float(osd[i]["momentum_buffer"].double().sum()), float(osd[i]["momentum_buffer"].double().abs().sum())]
                        if i in osd else [0.0, 0.0] for i in range(len(pkeys))])
        assert cs_err(mcs, g[pre + "mom_cs"]) < gtol
    msd = model.state_dict()
    assert int(msd["online_net.bn1.num_batches_tracked"]) == 2 * steps
    assert int(msd["target_net.layer4.0.downsample.1.num_batches_tracked"]) == 2 * steps
    assert int(msd["predictor.net.1.num_batches_tracked"]) == 2 * steps

    # fine-tune / test wrapper: train-mode and eval-mode logits (r3d_byol.py:420-428)
    fsd = r3d.closed_form_state(r3d.ft_spec(layers, 11), torch.float32)
    ft = R3DBYOL(pretrain=False, cls_bn=True, opts=_opts(depth, t, hw, 11))
    res = ft.load_state_dict(fsd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    ft.cuda().train()
    with torch.no_grad():
        assert rel(ft(x1d, o_type="ft_all").cpu().numpy(), g["ft.train_logits"]) < tol1
        ft.eval()
        assert rel(ft(x2d, o_type="test").cpu().numpy(), g["ft.eval_logits"]) < 2e-3
        # 'scratch' skips normalize + classify_bn: on this un-trained net (running statistics 0 / 1, Glorot-drawn BN gammas) the
        # eval-mode features shrink layer by layer and every row becomes the classifier bias plus a cancelling remainder, so two
        # fp32 evaluations (HIP vs stock CPU) agree to ~2e-3 only; the check guards the branch, not the arithmetic
        assert rel(ft(x2d, o_type="scratch").cpu().numpy(), r3d.ft_forward(fsd, x2, layers, False, "scratch").numpy()) < 1e-2


@pytest.mark.parametrize("act_dtype", ["fp32", "bf16"])
def test_r3d_factory_and_pretrain_driver(tmp_path, act_dtype):
    """generate_model(model_name='r3d_byol') + the pre-training driver for two epochs on synthetic clips; ``--act_dtype bf16``:
    the same command line with bf16 activation storage (BASELINE configs[4])."""
    import importlib.util
    import os
    from cstp_amd.opts import parse_opts
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("cstp_script_main_byol_r3d", os.path.join(root, "main_byol.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    opts = parse_opts(["--dataset", "synthetic", "--batch_size", "4", "--sample_duration", "8", "--sample_size", "56",
                       "--model_name", "r3d_byol", "--model_depth", "10", "--n_workers", "0", "--synthetic_len", "8",
                       "--result_path", str(tmp_path), "--task", "loss_com", "--loss_weight", "0.1", "1", "1", "1", "1",
                       "--n_epochs", "2", "--learning_rate", "0.01", "--weight_decay", "5e-4", "--act_dtype", act_dtype])
    mod.main(opts)
    rows = open(str(tmp_path / "synthetic" / "loss_com" / "synthetic_train_clip8modelr3d_byol10.log")).read().strip().split("\n")
    assert len(rows) == 3 and all(np.isfinite(float(r.split("\t")[1])) for r in rows[1:])


def test_r3d_finetune_and_test_drivers(tmp_path, capsys):
    """main_ft_mp.py --task scratch and test.py with --model_name r3d_byol: train, validate under model.eval(), keep the best
    checkpoint, load it strictly for the video-level test."""
    import importlib.util
    import os
    from cstp_amd.opts import parse_opts
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def load(name):
        spec = importlib.util.spec_from_file_location("cstp_script_%s_r3d" % name, os.path.join(root, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    common = ["--dataset", "synthetic", "--n_classes", "4", "--batch_size", "8", "--sample_duration", "8", "--sample_size", "56",
              "--model_name", "r3d_byol", "--model_depth", "10", "--n_workers", "0", "--synthetic_len", "32",
              "--result_path", str(tmp_path), "--weight_decay", "1e-4"]
    opts = parse_opts(common + ["--task", "scratch", "--learning_rate", "0.02", "--n_epochs", "3"])
    opts.highest_val = {"name": 0}
    load("main_ft_mp").main(opts)
    d = tmp_path / "synthetic" / "scratch"
    best = [f for f in os.listdir(d) if f.endswith("_max.pth")]
    assert len(best) == 1
    md = torch.load(str(d / best[0]), map_location="cpu")
    assert md["arch"] == "r3d_byol-10" and "module.classify_bn.running_mean" in md["state_dict"]
    opts = parse_opts(common + ["--task", "test", "--t_ft_task", "scratch"])
    acc = load("test").run(opts)
    assert 0.0 <= acc <= 1.0 and "Video accuracy" in capsys.readouterr().out


@pytest.mark.parametrize("fixture", ["r3d_50_backbone", "r3d_50_backbone_224"])
def test_r3d_50_bottleneck_backbone_matches_reference_modules_and_corrected_wrapper_matches_oracle(fixture):
    """``r3d_50_backbone_224``: the same at BASELINE configs[4]'s TRUE clip shape, 3x16x224x224 (B = 2: fp64 memory).
    BASELINE configs[4] names 3D-ResNet-50.  (1) The Bottleneck BACKBONE on the HIP kernels against the reference's own layers
    driven up to the average pool in fp64 (tests/golden/r3d_50_backbone.npz): pooled 2048-d features of two clip batches, the
    per-tensor gradient norms of sum(features * c), the BN running statistics, and the eval-mode features.  (2) The WRAPPER at
    this depth follows the corrected spec of cstp_amd/r3d_byol.py (the reference's is shape-broken, r3d_byol.py:204) and is
    parity-UNPINNED: one optimisation step of the product's PretrainStep is put against the CPU oracle of the same spec."""
    from cstp_amd.optim import FlatSGD
    from cstp_amd.r3d_byol import R3DBYOL
    from cstp_amd.train import PretrainStep
    from oracle import r21d_byol_oracle as orc
    from oracle import r3d_byol_oracle as r3d
    g = load(fixture)
    depth, b, t, hw, _ = [int(v) for v in g["meta"]]
    layers = r3d.for_depth(depth)
    try:
        esd = r3d.closed_form_state(r3d.encoder_spec("online_net", layers), torch.float32)
        net = R3DBYOL(pretrain=False, cls_bn=True, opts=_opts(depth, t, hw, 11)).online_net
        res = net.load_state_dict({k[len("online_net."):]: v for k, v in esd.items()}, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        net.cuda().train()
        x1, x2, _ = orc.closed_form_clips(b, t, hw, torch.float32)
        x1d, x2d = x1.cuda(), x2.cuda()
        f1 = net(x1d)
        assert tuple(f1.shape) == (b, 2048)
        c = orc.hash_uniform(f1.numel(), 4242).reshape(f1.shape).float().cuda()
        (f1 * c).sum().backward()
        assert rel(f1.detach().cpu().numpy(), g["feat_1"]) < 3e-4          # 53 conv + BN layers: the R34-class output bar
        gn = np.array([float(p.grad.norm()) for _, p in net.named_parameters()])
        assert [k for k, _ in net.named_parameters()] == [str(k) for k in g["param_keys"]]
        assert rel(gn, g["grad_norms"]) < 3e-2
        msd = net.state_dict()
        cs = np.array([[float(msd[str(k)].double().sum()), float(msd[str(k)].double().abs().sum())] for k in g["state_keys"]])
        assert cs_err(cs, g["state_cs_after_fwd"]) < 1e-4
        with torch.no_grad():
            assert rel(net(x2d).cpu().numpy(), g["feat_2"]) < 3e-4
            net.eval()
            assert rel(net(x1d).cpu().numpy(), g["feat_eval"]) < 2e-3

        # ---- the corrected wrapper (F = 2048), one full step vs the oracle of the same spec, on a smaller clip
        bb, tt, hh = 4, 4, 32
        sd = r3d.closed_form_state(r3d.model_spec(layers), torch.float32)
        y1, y2, _ = orc.closed_form_clips(bb, tt, hh, torch.float32)
        labels = r3d.closed_form_labels(bb)
        w = (0.1, 1.0, 1.0, 1.0, 1.0)
        osd = {k: v.clone() for k, v in sd.items()}
        info = r3d.train_step(osd, {}, y1, y2, labels, layers, 0.05, 0.9, 5e-4, w, True)
        model = R3DBYOL(pretrain=True, opts=_opts(depth, tt, hh))
        res = model.load_state_dict(sd, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        model.cuda()
        arenas = model.flatten_parameters()
        model.train()
        opt = FlatSGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4, arenas=arenas)
        step = PretrainStep(model, opt, w, clip_grad_norm=True)
        lab = {k: v.cuda() for k, v in labels.items()}
        out = step(y1.cuda(), y2.cuda(), lab["spa"], lab["tem"], lab["pb"], lab["rot1"], lab["rot2"])
        assert tuple(out.logits[0].shape) == (bb, 5) and tuple(out.logits[2].shape) == (bb, 4)     # B rows, not 4B
        assert rel(float(out.loss_byol), float(info["loss_byol"])) < 5e-4
        assert rel(float(out.loss_total), float(info["loss_total"])) < 5e-4
        assert rel(torch.stack([l.cpu() for l in out.logits[:2]]).numpy(), torch.stack(info["logits"][:2]).numpy()) < 2e-3
        assert rel(float(out.grad_norm), float(info["grad_norm"])) < 3e-2
        msd = model.state_dict()
        for k in ("online_net.layer4.2.bn3.running_var", "target_net.layer1.0.conv3.weight", "predictor.net.3.weight",
                  "overlap_spa.weight"):
            assert rel(msd[k].cpu().numpy(), osd[k].detach().numpy()) < 2e-3, k
    finally:
        r3d.for_depth(18)


def test_full_size_properties_r3d50_cfg5_share():
    """BASELINE configs[4] at its full per-GPU share -- 3D-ResNet-50 (corrected wrapper), 4 clip pairs of 3x16x224x224 (B = 32
    over 8 GPUs), fp32 storage -- one optimisation step of the product's PretrainStep, checked through properties that need
    no oracle run (the Bottleneck backbone itself is pinned at this clip shape by ``r3d_50_backbone_224``)."""
    from cstp_amd.optim import FlatSGD
    from cstp_amd.r3d_byol import R3DBYOL
    from cstp_amd.synthetic import device_batch
    from cstp_amd.train import PretrainStep
    torch.manual_seed(1)
    model = R3DBYOL(pretrain=True, opts=_opts(50, 16, 224)).cuda()
    a = model.flatten_parameters()
    model.train()
    lr, wd = 0.01, 5e-4
    opt = FlatSGD(model.parameters(), lr=lr, momentum=0.9, weight_decay=wd, arenas=a)
    step = PretrainStep(model, opt, (0.1, 1.0, 1.0, 1.0, 1.0), clip_grad_norm=True)
    x1, x2, lab = device_batch(4, 16, 224, torch.device("cuda"), seed=1)
    t_before, q_before, p_before = a["target"].clone(), a["param"][:a["n_encoder"]].clone(), a["param"].clone()
    out = step(x1, x2, lab["spa"], lab["tem"], lab["pb"], lab["rot1"], lab["rot2"])
    torch.cuda.synchronize()
    # (1) shapes of the corrected wrapper (B rows, 5/5/4/4-way heads), everything finite, BYOL loss in [0, 8]
    assert [tuple(l.shape) for l in out.logits] == [(4, 5), (4, 5), (4, 4), (4, 4), (4, 4), (4, 4)]
    assert np.isfinite(float(out.loss_total)) and 0.0 <= float(out.loss_byol) <= 8.0
    assert bool(torch.isfinite(a["grad"]).all()) and bool(torch.isfinite(a["param"]).all())
    # (2) the EMA is linear in the PRE-step online weights (it runs before the optimiser step, r3d_byol.py:392-395)
    expect = t_before * 0.996 + q_before * (1.0 - 0.996)
    assert rel_err(a["target"], expect) < 1e-6
    # (3) first SGD step: p_new = p - lr * (clip * g + wd * p); .grad holds the clipped gradient
    gnorm = float(out.grad_norm)
    coef = min(1.0, 18.0 / (gnorm + 1e-6))
    total_norm = float(a["grad"].double().norm())
    assert abs(total_norm - gnorm * coef) / (gnorm * coef) < 1e-4
    assert rel_err(a["param"], p_before - lr * (a["grad"] + wd * p_before)) < 1e-5
    # (4) BN counters and running statistics moved: two forwards per network per step
    msd = model.state_dict()
    assert int(msd["online_net.bn1.num_batches_tracked"]) == 2 and int(msd["target_net.bn1.num_batches_tracked"]) == 2
    assert bool(torch.isfinite(a["buffers"]).all()) and float(a["buffers"].abs().sum()) > 0

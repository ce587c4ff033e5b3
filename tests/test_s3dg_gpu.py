"""S3D-G-BYOL on a real MI355X: the fused self-gating + concat op (ops.gate_concat) against fp64 PyTorch over every (channels, s)
of the model, its absmax by-product, determinism and launch count; the pre-training step and the fine-tune / eval / test forwards
against golden vectors captured from the reference in fp64 (tests/golden/s3dg_*.npz); the drivers end to end; one full-size step."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import s3dg_spec
from conftest import rel_err
from test_oracle_golden import STATE_TOLS, TOLS, cs_err, rel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
# (branch channels, spatial) of every SepInception in the model at 16x112x112
BLOCKS = [([p[0], p[2], p[4], p[5]], (8, 14, 14) if name.startswith("Mixed_3") else (4, 7, 7) if name.startswith("Mixed_4")
           else (2, 3, 3)) for name, (_, p) in s3dg_spec.INCEPTIONS.items()]


def load(name):
    return np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)


def _gate_case(cs, spatial, n, seed):
    g = torch.Generator().manual_seed(seed)
    xs = [torch.rand((n, c) + spatial, generator=g, dtype=torch.float64) * 2 for c in cs]     # ReLU outputs: >= 0
    for x in xs:
        x[x < 0.5] = 0.0
    ws = [(torch.rand((c, c), generator=g, dtype=torch.float64) * 2 - 1) / c ** 0.5 for c in cs]
    bs = [torch.rand((c,), generator=g, dtype=torch.float64) * 2 - 1 for c in cs]
    dy = torch.rand((n, sum(cs)) + spatial, generator=g, dtype=torch.float64) * 2 - 1
    return xs, ws, bs, dy


def _gate_ref(xs, ws, bs):
    outs = []
    for x, w, b in zip(xs, ws, bs):
        gate = torch.sigmoid(torch.nn.functional.linear(x.mean(dim=[2, 3, 4]), w, b))
        outs.append(gate[:, :, None, None, None] * x)
    return torch.cat(outs, 1)


def _gate_hip(xs, ws, bs, dy):
    from cstp_amd import ops
    xg = [x.float().cuda().requires_grad_(True) for x in xs]
    wg = [w.float().cuda().requires_grad_(True) for w in ws]
    bg = [b.float().cuda().requires_grad_(True) for b in bs]
    y = ops.gate_concat(xg, list(zip(wg, bg)))
    cell = ops._absmax_of(y)
    y.backward(dy.float().cuda())
    torch.cuda.synchronize()
    return y.detach(), cell, [t.grad for t in xg], [t.grad for t in wg], [t.grad for t in bg]


@pytest.mark.parametrize("cs,spatial", BLOCKS + [([24, 7, 130], (3, 5, 3)), ([16], (1, 1, 1))])
def test_gate_concat_matches_fp64(cs, spatial):
    n = 6
    xs, ws, bs, dy = _gate_case(cs, spatial, n, 11 + sum(cs))
    xr = [x.clone().requires_grad_(True) for x in xs]
    wr = [w.clone().requires_grad_(True) for w in ws]
    br = [b.clone().requires_grad_(True) for b in bs]
    yr = _gate_ref(xr, wr, br)
    yr.backward(dy)
    y, cell, dxs, dws, dbs = _gate_hip(xs, ws, bs, dy)
    assert tuple(y.shape) == tuple(yr.shape)
    assert rel_err(y, yr) <= 1e-6
    for a, r in zip(dxs + dws + dbs, [t.grad for t in xr + wr + br]):
        assert rel_err(a, r) <= 1e-5
    # the absmax cell: max |y| as fp32 bits, exactly the value the tensor holds
    assert cell is not None and torch.equal(cell.view(torch.float32).cpu()[0], y.abs().max().cpu())
    # fixed-order reductions, no float atomics: a second run is bit-identical
    y2, cell2, dxs2, dws2, dbs2 = _gate_hip(xs, ws, bs, dy)
    assert torch.equal(y, y2) and torch.equal(cell, cell2)
    assert all(torch.equal(a, b) for a, b in zip(dxs + dws + dbs, dxs2 + dws2 + dbs2))


def test_gate_concat_rejects_mismatched_shapes_and_skips_saving_without_grad():
    from cstp_amd import ops
    from cstp_amd._lib import CstpError
    x = torch.rand(2, 4, 2, 3, 3, device="cuda")
    w, b = torch.rand(4, 4, device="cuda"), torch.rand(4, device="cuda")
    with pytest.raises(CstpError, match="one N, D, H, W"):
        ops.gate_concat([x, torch.rand(2, 4, 2, 3, 4, device="cuda")], [(w, b), (w, b)])
    with pytest.raises(CstpError, match="weight"):
        ops.gate_concat([x], [(torch.rand(4, 5, device="cuda"), b)])
    with torch.no_grad():
        y = ops.gate_concat([x, x], [(w, b), (w, b)])
    assert y.grad_fn is None and tuple(y.shape) == (2, 8, 2, 3, 3)


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_gate_concat_launches_per_block():
    """At most 2 kernel launches forward and 3 backward for all four branches of a block (the composed path needs ~20 / ~30)."""
    from cstp_amd import ops
    cs, spatial = BLOCKS[2]
    xs, ws, bs, dy = _gate_case(cs, spatial, 4, 5)
    xg = [x.float().cuda().requires_grad_(True) for x in xs]
    gates = [(w.float().cuda().requires_grad_(True), b.float().cuda().requires_grad_(True)) for w, b in zip(ws, bs)]
    dyg = dy.float().cuda()
    ops.gate_concat(xg, gates).backward(dyg)          # warm-up (library load, workspace)
    out = {}

    def fwd():
        out["y"] = ops.gate_concat(xg, gates)

    fw = _kernel_names(fwd)
    bw = _kernel_names(lambda: torch.autograd.backward(out["y"], dyg))
    print("forward kernels:", fw, "backward kernels:", bw)
    assert len([k for k in fw if "gate_" in k]) == 2 and len(fw) <= 2
    assert len([k for k in bw if "gate_" in k]) == 3
    # what else the backward pass launches is autograd's gradient accumulation into the 12 fresh .grad tensors, not the op
    assert len([k for k in bw if "gate_" not in k]) <= 12


def _build_pretrain(sd):
    from cstp_amd.s3dg_byol import S3DGBYOL
    m = S3DGBYOL(pretrain=True, gating=True, slow=False, num_classes=101)
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    m.cuda()
    m.flatten_parameters()
    return m.train()


# S3D-G's last inception blocks normalise over very few values per channel (s = 1 at 8x32x32, 18 at 16x112x112), which amplifies
# rounding: the reference's own fp32 run sits 1e-4 .. 6e-4 from the fp64 truth on the forward tensors and up to 0.25 on the grad
# norm of an ill-conditioned second step (recorded per fixture as fp32.fwd / fp32.dev by make_golden_s3dg.py).  A quantity passes
# under the usual bar, or within this factor of what stock fp32 leaves against the same truth -- a broken kernel is off by 10x+.
HIP_VS_FP32 = 4.0


def _tol(base, dev):
    return max(base, HIP_VS_FP32 * float(dev))


# the smallest case also runs with the target forward on the main stream (ByolBase._two_view_step's serial branch); the ids of
# the existing cases are unchanged
GOLDEN_CASES = ["s3dg_small", "s3dg_112"]
@pytest.mark.parametrize("name,overlap", [pytest.param(n, True if n == "s3dg_small" else None, id=n) for n in GOLDEN_CASES]
                         + [pytest.param("s3dg_small", False, id="s3dg_small-serial")])
def test_s3dg_pretrain_matches_reference_golden(name, overlap, monkeypatch):
    if overlap is not None:
        from cstp_amd import r21d_byol
        monkeypatch.setattr(r21d_byol, "OVERLAP_TARGET_FORWARD", overlap)
    from cstp_amd.optim import FlatSGD
    from cstp_amd.train import PretrainStep
    from oracle import r21d_byol_oracle as orc
    from oracle import r3d_byol_oracle as r3d
    g = load(name)
    b, t, hw, steps = [int(v) for v in g["meta"]]
    dev = g["fp32.dev"]
    sd = s3dg_spec.closed_form(s3dg_spec.model_spec(), torch.float32)
    keys = list(sd.keys())
    x1, x2, _ = orc.closed_form_clips(b, t, hw, torch.float32)
    x1d, x2d = x1.cuda(), x2.cuda()
    lab = {k: v.cuda() for k, v in r3d.closed_form_labels(b).items()}
    model = _build_pretrain(sd)
    with torch.no_grad():
        f1, q1 = model.online_net(x1d)
        f2, q2 = model.online_net(x2d)
        p1, p2 = model.predictor(q1), model.predictor(q2)
        model._update_target_net()
        _, t1 = model.target_net(x1d)
        _, t2 = model.target_net(x2d)
    for i, (k, v) in enumerate((("feat_1", f1), ("feat_2", f2), ("proj_1", q1), ("proj_2", q2), ("pred_1", p1), ("pred_2", p2),
                                ("tproj_1", t1), ("tproj_2", t2))):
        e = rel(v.cpu().numpy(), g["fwd." + k])
        print("%s fwd.%s: HIP %.3g, reference fp32 %.3g" % (name, k, e, g["fp32.fwd"][i]))
        assert e < _tol(TOLS[1][0], g["fp32.fwd"][i]), k

    model = _build_pretrain(sd)
    opt = FlatSGD(model.parameters(), lr=float(g["lr"]), momentum=0.9, weight_decay=float(g["wd"]),
                  arenas=model.flatten_parameters())
    step = PretrainStep(model, opt, tuple(g["loss_weight"]), clip_grad_norm=True)
    pkeys = [str(k) for k in g["param_keys"]]
    for s in range(1, steps + 1):
        pre = "s%d." % s
        tol = _tol(TOLS[s][0], dev[s - 1][2])
        gtol = _tol(TOLS[s][1], dev[s - 1][3])
        out = step(x1d, x2d, lab["spa"], lab["tem"], lab["pb"], lab["rot1"], lab["rot2"])
        print("%s step %d: logits HIP %.3g (reference fp32 %.3g), grad_norm HIP %.3g (reference fp32 %.3g)"
              % (name, s, rel(torch.stack([l.cpu() for l in out.logits]).numpy(), g[pre + "logits"]), dev[s - 1][2],
                 rel(float(out.grad_norm), g[pre + "grad_norm"]), dev[s - 1][3]))
        assert rel(float(out.loss_byol), g[pre + "loss_byol"]) < tol
        assert rel(float(out.loss_total), g[pre + "loss_total"]) < tol
        assert rel([float(c) for c in out.ce], g[pre + "ce"]) < tol
        assert rel(torch.stack([l.cpu() for l in out.logits]).numpy(), g[pre + "logits"]) < tol
        assert rel(float(out.grad_norm), g[pre + "grad_norm"]) < gtol
        # .grad holds the CLIPPED gradient after the fused optimizer pass: undo the coefficient (clip_grad_norm_, main_byol.py:89)
        coef = min(1.0, 18.0 / (float(out.grad_norm) + 1e-6))
        gn = {k: float(p.grad.norm()) / coef for k, p in model.named_parameters() if p.requires_grad}
        gn = np.array([gn.get(k, -1.0) for k in pkeys])
        ref_gn = g[pre + "grad_norms"]
        per = np.abs(gn - ref_gn) / np.maximum(np.abs(ref_gn), 1e-3 * np.abs(ref_gn).max())
        worst = [(pkeys[i], float(gn[i]), float(ref_gn[i])) for i in np.argsort(-per)[:5]]
        print("%s step %d: grad_norms HIP %.3g (reference fp32 %.3g), worst tensors %s" % (name, s, rel(gn, ref_gn), dev[s - 1][4], worst))
        assert rel(gn, ref_gn) < _tol(TOLS[s][1], dev[s - 1][4]), worst
        st = model.state_dict()
        cs = np.array([[float(st[k].double().sum()), float(st[k].double().abs().sum())] for k in keys])
        osd = opt.state_dict()["state"]
        mcs = np.array([[float(osd[i]["momentum_buffer"].double().sum()), float(osd[i]["momentum_buffer"].double().abs().sum())]
                        if i in osd else [0.0, 0.0] for i in range(len(pkeys))])
        me = np.abs(mcs - g[pre + "mom_cs"]).max(axis=1) / np.maximum(np.abs(g[pre + "mom_cs"][:, 1]), 1e-12)
        print("%s step %d: state_cs HIP %.3g (reference fp32 %.3g), mom_cs HIP %.3g (reference fp32 %.3g), worst %s"
              % (name, s, cs_err(cs, g[pre + "state_cs"]), dev[s - 1][5], cs_err(mcs, g[pre + "mom_cs"]), dev[s - 1][6],
                 [(pkeys[i], float(me[i])) for i in np.argsort(-me)[:5]]))
        assert cs_err(cs, g[pre + "state_cs"]) < _tol(STATE_TOLS[s], dev[s - 1][5])
        assert cs_err(mcs, g[pre + "mom_cs"]) < _tol(gtol, dev[s - 1][6])
    msd = model.state_dict()
    assert int(msd["online_net.Conv_1a.bn1.num_batches_tracked"]) == 2 * steps
    assert int(msd["online_net.block1.0.bn1.num_batches_tracked"]) == 2 * steps
    assert int(msd["target_net.Mixed_5c.branch3.1.bn.num_batches_tracked"]) == 2 * steps
    assert int(msd["online_net.project.net.1.num_batches_tracked"]) == 2 * steps
    assert int(msd["predictor.net.1.num_batches_tracked"]) == 2 * steps
    assert int(msd["overlap_spa.1.num_batches_tracked"]) == steps
    assert int(msd["rotate_cls.1.num_batches_tracked"]) == 2 * steps


@pytest.mark.parametrize("name", ["s3dg_ft_all", "s3dg_ft_fc"])
def test_s3dg_finetune_eval_test_match_reference_golden(name):
    from cstp_amd.s3dg_byol import S3DGBYOL, get_fine_tuning_parameters
    from oracle import r21d_ft_oracle as ftorc
    g = load(name)
    b, t, hw, k, steps = [int(v) for v in g["meta"]]
    task = str(g["task"])
    sd = s3dg_spec.closed_form(s3dg_spec.ft_spec(k), torch.float32)
    model = S3DGBYOL(pretrain=False, gating=True, slow=False, num_classes=k)
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    model.cuda()
    params = get_fine_tuning_parameters(model, 0 if task == "ft_all" else 5)
    opt = torch.optim.SGD(params, lr=float(g["lr"]), momentum=0.9, weight_decay=float(g["wd"]))
    x_train, x_val, labels = ftorc.closed_form_batch(b, t, hw, k, dtype=torch.float32)
    xt, xv, lab = x_train.cuda(), x_val.cuda(), labels.cuda()
    assert np.array_equal([p.requires_grad for p in model.parameters()], g["requires_grad"])
    names = [n for n, _ in model.named_parameters()]
    for s in range(1, steps + 1):
        pre = "s%d." % s
        tol = TOLS[s][0]
        model.train()
        outputs = model(xt, o_type=task)
        loss = torch.nn.functional.cross_entropy(outputs, lab)
        opt.zero_grad()
        loss.backward()
        gn = np.array([float(p.grad.norm()) if p.grad is not None else -1.0 for p in model.parameters()])
        opt.step()
        dv = g["fp32.dev"][s - 1]        # the reference's own fp32 run: [loss, logits, grad_norms, val_logits, video_mean]
        e = {"loss": rel(float(loss), g[pre + "loss"]), "logits": rel(outputs.detach().cpu().numpy(), g[pre + "logits"])}
        ref_gn = g[pre + "grad_norms"]
        assert np.array_equal(gn < 0, ref_gn < 0), [n for n, a, r in zip(names, gn, ref_gn) if (a < 0) != (r < 0)]
        live = ref_gn >= 0
        e["grad_norms"] = rel(gn[live], ref_gn[live])
        model.eval()
        with torch.no_grad():
            e["val_logits"] = rel(model(xv, o_type=task).cpu().numpy(), g[pre + "val_logits"])
            vid = model(xv, None, o_type="test").mean(dim=0, keepdim=True)
            e["video_mean"] = rel(vid.cpu().numpy(), g[pre + "video_mean"])
        print("%s step %d: (HIP, reference fp32) %s" % (name, s, {k: (v, float(d)) for (k, v), d in zip(e.items(), dv)}))
        assert e["loss"] < _tol(tol, dv[0]) and e["logits"] < _tol(tol, dv[1])
        assert e["grad_norms"] < _tol(TOLS[s][1], dv[2])
        assert e["val_logits"] < _tol(2e-3, dv[3]) and e["video_mean"] < _tol(2e-3, dv[4])


def _run(args, timeout):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args[0], r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_s3dg_driver_chain(tmp_path):
    """main_byol.py --model_name s3d_byol on synthetic clips (100 one-step epochs: the driver checkpoints every 100), its
    checkpoint fine-tuned by main_ft_mp.py --task ft_fc, the best fine-tune checkpoint tested by test.py -- each a child process
    with a time limit.  No model-specific code in any driver."""
    res = str(tmp_path)
    common = ["--dataset", "synthetic", "--sample_duration", "8", "--sample_size", "32", "--model_name", "s3d_byol",
              "--model_depth", "1", "--n_workers", "0", "--result_path", res]
    _run(["main_byol.py"] + common + ["--batch_size", "4", "--synthetic_len", "4", "--task", "loss_com", "--loss_weight", "0.1",
                                      "1", "1", "1", "1", "--n_epochs", "100", "--learning_rate", "0.005", "--weight_decay", "5e-4"],
         900)
    ckpt = os.path.join(res, "synthetic", "loss_com", "save_100.pth")
    md = torch.load(ckpt, map_location="cpu")
    keys = list(md["state_dict"].keys())
    assert md["arch"] == "s3d_byol-1"
    assert [k[len("module."):] for k in keys] == [k for k, _, _ in s3dg_spec.model_spec()]
    assert all(torch.isfinite(v.float()).all() for v in md["state_dict"].values())
    ft = common + ["--n_classes", "4", "--batch_size", "8", "--synthetic_len", "16", "--weight_decay", "1e-4"]
    _run(["main_ft_mp.py"] + ft + ["--task", "ft_fc", "--pretrained_path", ckpt, "--learning_rate", "0.05", "--n_epochs", "2"], 600)
    d = os.path.join(res, "synthetic", "ft_fc")
    best = [f for f in os.listdir(d) if f.endswith("_max.pth")]
    assert len(best) == 1
    fmd = torch.load(os.path.join(d, best[0]), map_location="cpu")
    assert [k[len("module."):] for k in fmd["state_dict"]] == [k for k, _, _ in s3dg_spec.ft_spec(4)]
    # ft_fc trains the classifier (and, by the substring match, classify_bn) only: the encoder keeps the pre-trained weights
    assert torch.equal(fmd["state_dict"]["module.online_net.Conv_2b.conv.weight"], md["state_dict"]["module.online_net.Conv_2b.conv.weight"])
    out = _run(["test.py"] + ft + ["--task", "test", "--t_ft_task", "ft_fc"], 600)
    assert "Video accuracy" in out


def test_s3dg_full_size_step():
    """BASELINE-size step: 16 clip pairs of 3x16x112x112 through PretrainStep; finite loss and gradients, peak memory reported."""
    from cstp_amd.optim import FlatSGD
    from cstp_amd.s3dg_byol import S3DGBYOL
    from cstp_amd.train import PretrainStep
    torch.manual_seed(0)
    model = S3DGBYOL(pretrain=True, gating=True, slow=False, num_classes=101).cuda()
    arenas = model.flatten_parameters()
    model.train()
    opt = FlatSGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=5e-4, arenas=arenas)
    step = PretrainStep(model, opt, (0.1, 1.0, 1.0, 1.0, 1.0), clip_grad_norm=True)
    b = 16
    g = torch.Generator(device="cuda").manual_seed(0)
    x1 = torch.rand((b, 3, 16, 112, 112), device="cuda", generator=g) * 2 - 1
    x2 = torch.rand((b, 3, 16, 112, 112), device="cuda", generator=g) * 2 - 1
    lab = [torch.randint(0, 5, (b,), device="cuda", generator=g) for _ in range(5)]
    torch.cuda.reset_peak_memory_stats()
    out = step(x1, x2, *lab)
    torch.cuda.synchronize()
    print("s3d_byol B=16 pairs 3x16x112x112: loss_total %.4f grad_norm %.3f peak memory %.2f GiB"
          % (float(out.loss_total), float(out.grad_norm), torch.cuda.max_memory_allocated() / 2 ** 30))
    assert np.isfinite(float(out.loss_total)) and np.isfinite(float(out.grad_norm))
    assert bool(torch.isfinite(arenas["grad"]).all()) and bool(torch.isfinite(arenas["param"]).all())


def test_composed_gate_path_agrees(monkeypatch):
    """CSTP_S3D_GATE=0 (ops.linear + ATen mean / sigmoid / mul / cat) computes what the fused op does: one inception block
    (Mixed_3c's channels), forward and every gradient."""
    from cstp_amd import s3dg_byol
    torch.manual_seed(3)
    blk = s3dg_byol.SepInception(256, [128, 128, 192, 32, 96, 64], gating=True).cuda().train()
    x = (torch.rand(4, 256, 4, 14, 14, device="cuda") * 2 - 1).requires_grad_(True)
    dy = torch.rand(4, 480, 4, 14, 14, device="cuda") * 2 - 1
    outs = []
    for fused in (True, False):
        monkeypatch.setattr(s3dg_byol, "FUSED_GATE", fused)
        params = [p for p in blk.parameters()]
        y = blk(x, 2)
        grads = torch.autograd.grad(y, [x] + params, dy)
        outs.append([y.detach()] + list(grads))
    for a, b in zip(*outs):
        assert rel_err(a, b) < 1e-5

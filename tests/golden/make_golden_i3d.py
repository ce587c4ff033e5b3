#!/usr/bin/env python3
"""Golden vectors for the I3D-BYOL wrappers from the REFERENCE implementation (CPU, fp64 truth).

Runs only in the build container: it imports /root/reference/models/BE/i3d_byol.py (read-only) and refuses to run without it.
Nothing of the reference is copied -- the outputs are data (tests/golden/i3d_*.npz).  The pre-training sequence is the one of
main_byol.py:60-91 (6x CrossEntropy, loss_weight sum, zero_grad, backward, clip_grad_norm_(18), SGD) and the fine-tune sequence the
one of main_ft_mp.py / test.py (see make_golden_ft.py), restated because the drivers themselves need CUDA + torchvision.
Closed-form weights: tests/i3d_spec.py.  Besides the fp64 truth every config
records how far the reference's own fp32 run lands from it (``fp32.*``), the yardstick for any widened bar.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_i3d.py [config ...]
"""
import os
import sys
import time

import numpy as np
import torch

REF = "/root/reference"
if not os.path.isdir(REF):
    raise SystemExit("make_golden_i3d.py needs the reference at /root/reference (build container only)")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

from models.BE import i3d_byol as ref_model  # noqa: E402  (reference)

import i3d_spec as spec  # noqa: E402
from oracle import r21d_byol_oracle as orc  # noqa: E402  (closed-form fills only)
from oracle import r21d_ft_oracle as ftorc  # noqa: E402  (closed-form fills only)
from oracle import r3d_byol_oracle as r3d  # noqa: E402  (closed-form labels only)

CONFIGS = {
    # name: (B, T, HW, steps, lr, wd)
    "i3d_small": (4, 8, 64, 2, 0.005, 5e-4),      # final map 1 x 2 x 2
    "i3d_112": (2, 16, 112, 1, 0.05, 5e-4),       # final map 2 x 4 x 4
}
FT_CONFIGS = {
    # name: (task, B, T, HW, classes, steps, lr, wd)
    "i3d_ft_all": ("ft_all", 2, 16, 224, 11, 2, 0.01, 5e-4),      # the classifier needs the 2 x 7 x 7 map of a 16 x 224 x 224 clip
}
LOSS_WEIGHT = (0.1, 1.0, 1.0, 1.0, 1.0)


def checksums(items):
    return np.stack([np.array([float(v.detach().double().sum()), float(v.detach().double().abs().sum())]) for _, v in items])


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def cs_err(ours, ref):
    scale = np.maximum(np.abs(ref[:, 1]), 1e-12)
    return float((np.abs(ours - ref).max(axis=1) / scale).max())


def build(dtype):
    m = ref_model.I3DBYOL(pretrain=True, opts=None)
    sd = spec.closed_form(spec.model_spec(), torch.float64)
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert list(m.state_dict().keys()) == list(sd.keys()), "state-dict order differs from tests/i3d_spec.py"
    return m.to(dtype).train()


def pretrain_steps(b, t, hw, steps, lr, wd, dtype, out=None, name=""):
    model = build(dtype)
    x1, x2, _ = orc.closed_form_clips(b, t, hw, dtype=dtype)
    labels = r3d.closed_form_labels(b)
    crit = torch.nn.CrossEntropyLoss()
    opt = torch.optim.SGD(model.parameters(), lr=lr, momentum=0.9, weight_decay=wd)
    names = [k for k, _ in model.named_parameters()]
    res = []
    for step in range(1, steps + 1):
        t0 = time.time()
        loss_byol, logits = model(x1, x2, o_type="loss_com")
        ce = [crit(logits[0], labels["spa"]), crit(logits[1], labels["tem"]), crit(logits[2], labels["pb"]),
              crit(logits[3], labels["pb"]), crit(logits[4], labels["rot1"]), crit(logits[5], labels["rot2"])]
        w = LOSS_WEIGHT
        total = w[0] * loss_byol + w[1] * ce[0] + w[2] * ce[1] + w[3] * ce[2] + w[3] * ce[3] + w[4] * ce[4] + w[4] * ce[5]
        opt.zero_grad()
        total.backward()
        gn = {k: float(p.grad.detach().norm()) for k, p in model.named_parameters() if p.grad is not None}
        gnorm = torch.nn.utils.clip_grad_norm_(model.parameters(), 18)
        opt.step()
        lg = np.concatenate([l.detach().double().numpy() for l in logits], axis=1)     # [B, 5 + 5 + 4 x 4]
        res.append((float(loss_byol), float(total), lg, float(gnorm)))
        if out is None:
            continue
        pre = "s%d." % step
        out[pre + "loss_byol"] = np.array(float(loss_byol.detach()))
        out[pre + "loss_total"] = np.array(float(total.detach()))
        out[pre + "ce"] = np.array([float(c.detach()) for c in ce])
        out[pre + "grad_norm"] = np.array(float(gnorm))
        out[pre + "logits"] = lg.astype(np.float32)
        out[pre + "grad_norms"] = np.array([gn.get(k, -1.0) for k in names])
        out[pre + "state_cs"] = checksums(model.state_dict().items())
        mcs = []
        for p in model.parameters():
            buf = opt.state.get(p, {}).get("momentum_buffer")
            mcs.append([float(buf.double().sum()), float(buf.double().abs().sum())] if buf is not None else [0.0, 0.0])
        out[pre + "mom_cs"] = np.array(mcs)
        print("  [%s] step %d: byol %.6f total %.6f gnorm %.4f (%.1fs)" % (name, step, float(loss_byol), float(total), float(gnorm),
                                                                            time.time() - t0), flush=True)
    if out is not None:
        out["param_keys"] = np.array(names)
    return res


def run_config(name):
    b, t, hw, steps, lr, wd = CONFIGS[name]
    out = {"meta": np.array([b, t, hw, steps], dtype=np.int64), "lr": np.array(lr), "wd": np.array(wd),
           "loss_weight": np.array(LOSS_WEIGHT)}
    r64 = pretrain_steps(b, t, hw, steps, lr, wd, torch.float64, out, name)
    # forward internals from the closed-form state: features, predictions, target features after one EMA
    model = build(torch.float64)
    x1, x2, _ = orc.closed_form_clips(b, t, hw, dtype=torch.float64)
    with torch.no_grad():
        f1 = model.online_net(x1)
        f2 = model.online_net(x2)
        p1, p2 = model.predictor(f1), model.predictor(f2)
        model._update_target_net()
        t1 = model.target_net(x1)
        t2 = model.target_net(x2)
    fwd = (("feat_1", f1), ("feat_2", f2), ("pred_1", p1), ("pred_2", p2), ("tfeat_1", t1), ("tfeat_2", t2))
    for k, v in fwd:
        out["fwd." + k] = v.numpy().astype(np.float32)
    # ... and the reference's own fp32 forward of the same: its deviation per tensor
    m32 = build(torch.float32)
    y1, y2, _ = orc.closed_form_clips(b, t, hw, dtype=torch.float32)
    with torch.no_grad():
        g1 = m32.online_net(y1)
        g2 = m32.online_net(y2)
        s1, s2 = m32.predictor(g1), m32.predictor(g2)
        m32._update_target_net()
        u1 = m32.target_net(y1)
        u2 = m32.target_net(y2)
    out["fp32.fwd"] = np.array([rel(v.numpy(), ref.numpy()) for v, (_, ref) in zip((g1, g2, s1, s2, u1, u2), fwd)])
    # the reference's own fp32 run against the fp64 truth: [step][loss_byol, loss_total, logits, grad_norm, grad_norms (per tensor),
    # state checksums, momentum checksums] -- the latter three as the tests measure them (rel / cs_err)
    o32 = {}
    r32 = pretrain_steps(b, t, hw, steps, lr, wd, torch.float32, o32, name + " fp32")
    out["fp32.dev"] = np.array([[rel(a[0], c[0]), rel(a[1], c[1]), rel(a[2], c[2]), rel(a[3], c[3]),
                                 rel(o32["s%d.grad_norms" % s], out["s%d.grad_norms" % s]),
                                 cs_err(o32["s%d.state_cs" % s], out["s%d.state_cs" % s]),
                                 cs_err(o32["s%d.mom_cs" % s], out["s%d.mom_cs" % s])]
                                for s, (a, c) in enumerate(zip(r32, r64), 1)])
    print("  [%s] reference fp32 vs fp64: %s" % (name, out["fp32.dev"].tolist()))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name)


class _Opts:
    def __init__(self, n_classes):
        self.n_classes = n_classes


def build_ft(k, dtype):
    m = ref_model.I3DBYOL(pretrain=False, opts=_Opts(k))
    sd = spec.closed_form(spec.ft_spec(k), torch.float64)
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys and list(m.state_dict().keys()) == list(sd.keys())
    return m.to(dtype).train()


def run_ft(name):
    task, b, t, hw, k, steps, lr, wd = FT_CONFIGS[name]
    model = build_ft(k, torch.float64)
    x_train, x_val, labels = ftorc.closed_form_batch(b, t, hw, k, dtype=torch.float64)
    crit = torch.nn.CrossEntropyLoss()
    params = ref_model.get_fine_tuning_parameters(model, 0 if task == "ft_all" else 5)
    opt = torch.optim.SGD(params, lr=lr, momentum=0.9, weight_decay=wd)
    names = [n for n, _ in model.named_parameters()]
    out = {"meta": np.array([b, t, hw, k, steps], dtype=np.int64), "task": np.array(task), "lr": np.array(lr),
           "wd": np.array(wd), "labels": labels.numpy()}
    for step in range(1, steps + 1):
        model.train()
        outputs = model(x_train, o_type=task)
        loss = crit(outputs, labels)
        opt.zero_grad()
        loss.backward()
        gn = {n: (float(p.grad.detach().norm()) if p.grad is not None else -1.0) for n, p in model.named_parameters()}
        opt.step()
        pre = "s%d." % step
        out[pre + "loss"] = np.array(float(loss))
        out[pre + "logits"] = outputs.detach().numpy().astype(np.float32)
        out[pre + "grad_norms"] = np.array([gn[n] for n in names])
        out[pre + "state_cs"] = checksums(model.state_dict().items())
        model.eval()
        with torch.no_grad():
            out[pre + "val_logits"] = model(x_val, o_type=task).numpy().astype(np.float32)
            vid = model(x_val, None, o_type="test")            # test.py: the clips of ONE video, averaged
        out[pre + "video_mean"] = vid.mean(dim=0, keepdim=True).numpy().astype(np.float32)
        print("  [%s] step %d: loss %.6f" % (name, step, float(loss)), flush=True)
    out["state_keys"] = np.array(list(model.state_dict().keys()))
    out["param_keys"] = np.array(names)
    out["requires_grad"] = np.array([p.requires_grad for p in model.parameters()])
    out["group_lrs"] = np.array([g["lr"] for g in opt.param_groups])
    m32 = build_ft(k, torch.float32)
    a_train, a_val, a_lab = ftorc.closed_form_batch(b, t, hw, k, dtype=torch.float32)
    # the same steps in fp32: [step][loss, logits, grad_norms, val_logits, video_mean, state checksums] deviation from the fp64 truth
    opt32 = torch.optim.SGD(ref_model.get_fine_tuning_parameters(m32, 0 if task == "ft_all" else 5), lr=lr, momentum=0.9,
                            weight_decay=wd)
    dev = []
    for step in range(1, steps + 1):
        pre = "s%d." % step
        m32.train()
        o = m32(a_train, o_type=task)
        if step == 1:
            out["fp32.logits"] = o.detach().numpy()
        loss = crit(o, a_lab)
        opt32.zero_grad()
        loss.backward()
        gn = np.array([float(p.grad.norm()) if p.grad is not None else -1.0 for p in m32.parameters()])
        opt32.step()
        state_dev = cs_err(checksums(m32.state_dict().items()), out[pre + "state_cs"])      # after the update, before the eval forwards
        m32.eval()
        with torch.no_grad():
            v = m32(a_val, o_type=task)
            vid = m32(a_val, None, o_type="test").mean(dim=0, keepdim=True)
        dev.append([rel(float(loss), out[pre + "loss"]), rel(o.detach().numpy(), out[pre + "logits"]),
                    rel(gn, out[pre + "grad_norms"]), rel(v.numpy(), out[pre + "val_logits"]),
                    rel(vid.numpy(), out[pre + "video_mean"]), state_dev])
    out["fp32.dev"] = np.array(dev)
    print("  [%s] reference fp32 vs fp64: %s" % (name, out["fp32.dev"].tolist()))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name)


def run_init(name="i3d_init"):
    """The reference's own initialisation under torch.manual_seed(1): key lists and per-tensor checksums (pre-training and
    fine-tune wrappers), and the fine-tune parameter groups of ft_begin_index 5 (ft_fc: no I3D parameter stays trainable)."""
    out = {}
    torch.manual_seed(1)
    m = ref_model.I3DBYOL(pretrain=True, opts=None)
    out["state_keys"] = np.array(list(m.state_dict().keys()))
    out["state_cs"] = checksums(m.state_dict().items())
    out["n_params"] = np.array(len(list(m.parameters())))
    torch.manual_seed(1)
    f = ref_model.I3DBYOL(pretrain=False, opts=_Opts(11))
    out["ft.n_params"] = np.array(len(list(f.parameters())))
    out["ft.state_keys"] = np.array(list(f.state_dict().keys()))
    out["ft.state_cs"] = checksums(f.state_dict().items())
    groups = ref_model.get_fine_tuning_parameters(f, 5)
    out["ft_fc.trainable"] = np.array([n for n, p in f.named_parameters() if p.requires_grad])
    out["ft_fc.group_lrs"] = np.array([g.get("lr", -1.0) for g in groups])
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name)


if __name__ == "__main__":
    torch.set_num_threads(8)
    for c in (sys.argv[1:] or list(CONFIGS) + list(FT_CONFIGS) + ["i3d_init"]):
        if c == "i3d_init":
            run_init()
        elif c in FT_CONFIGS:
            run_ft(c)
        else:
            run_config(c)

#!/usr/bin/env python3
"""What dropout and stochastic depth cost next to a fine-tune step on one MI355X, and the kernels against the ATen compositions
they stand in for (CSTP_REG_FUSED=0 runs those inside the step).

    python tools/bench_reg.py --windows 5 --steps 10 [--out profiles/r16/bench_reg.jsonl] [--only steps|kernels]

One process, the cases alternating window by window (so a drift of the box lands on all of them alike).
  Steps (host clock around `steps` calls that end in a device synchronise):
    r21d18_fp32_off / _on   R(2+1)D-18 ft_all, 16 clips of 3x16x112x112, fp32; without a regulariser / with --dropout 0.5 --drop_path 0.1
    r3d50_bf16_off / _on    3D-ResNet-50 ft_all, 4 clips of 3x16x224x224, bf16 activation storage; likewise
  Kernels (device events around `kernel_steps` back-to-back calls into preallocated outputs; no autograd, no allocation):
    join_fwd / join_bwd     cstp_droppath_add_relu_* vs relu(s * z + r) / (g = dy * (y > 0); s * g) from ATen, at the first- and
                            last-stage block shapes of the two models
    dropout                 cstp_dropout vs x * mask * inv with a precomputed mask (ATen's share of a dropout that stores its mask)
  Bytes: what the operation has to move (join forward: read z and res, write y; backward: read y and dy, write dz and dres;
  dropout: read x, write y; the ATen dropout also reads its mask), over the kernel time, and that rate as a share of the 8 TB/s
  HBM peak -- the operations are bandwidth-bound.  The last-stage tensors are a few MB and stay in the last-level cache: their
  rates are not HBM rates.  One JSON line per case."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cstp_amd import _lib, ops  # noqa: E402
from cstp_amd.optim import FlatSGD  # noqa: E402
from cstp_amd.r21d_byol import R21DBYOL, layer_sizes_for_depth  # noqa: E402
from cstp_amd.r3d_byol import R3DBYOL  # noqa: E402
from cstp_amd.regularize import Regularizer  # noqa: E402
from cstp_amd.train import FineTuneStep  # noqa: E402

HBM_PEAK = 8.0e12


def host_window(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def event_window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def make_step(kind, dev, regularizer, classes):
    torch.manual_seed(1)
    if kind == "r21d18_fp32":
        model = R21DBYOL(pretrain=False, num_classes=classes, cls_bn=True, layer_sizes=layer_sizes_for_depth(18)).to(dev)
    else:
        opts = argparse.Namespace(model_depth=50, sample_size=224, sample_duration=16, sc_type="B", n_classes=classes, act_dtype="bf16")
        model = R3DBYOL(pretrain=False, cls_bn=True, opts=opts).to(dev)
    arenas = model.flatten_parameters()
    opt = FlatSGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=5e-4, arenas=arenas)
    model.train()
    return FineTuneStep(model, opt, "ft_all", regularizer=regularizer)


def join_cases(name, shape, dtype, dev, lib):
    """[(case, fn, bytes)] of the join forward and backward at one block shape, kernel and ATen composition."""
    b16 = dtype == torch.bfloat16
    z, r, dy = [(torch.rand(shape, device=dev) * 2 - 1).to(dtype) for _ in range(3)]
    s = torch.tensor([0.0 if i % 4 == 1 else 1.25 for i in range(shape[0])], device=dev)
    sv = s.view(-1, 1, 1, 1, 1)
    y, dz, dres = torch.empty_like(z), torch.empty_like(z), torch.empty_like(z)
    n, row, st = z.numel(), z.numel() // shape[0], torch.cuda.current_stream().cuda_stream
    ops.drop_path_add_relu(z, r, s)          # (argument checks once, outside the windows)
    y.copy_(torch.relu(sv * z.float() + r.float()).to(dtype))
    nbytes = 3 * n * z.element_size()

    def fwd_hip():
        lib.cstp_droppath_add_relu_forward(st, z.data_ptr(), r.data_ptr(), s.data_ptr(), y.data_ptr(), n, row, 1 if b16 else 0, None)

    def bwd_hip():
        lib.cstp_droppath_add_relu_backward(st, y.data_ptr(), dy.data_ptr(), s.data_ptr(), dz.data_ptr(), dres.data_ptr(), n, row,
                                            1 if b16 else 0)

    def fwd_aten():
        if b16:
            return torch.relu(sv * z.float() + r.float()).to(dtype)
        return torch.relu(sv * z + r)

    def bwd_aten():
        g = dy * (y > 0)
        return sv.to(dtype) * g, g

    tag = "%s %s %s" % (name, "x".join(str(v) for v in shape), "bf16" if b16 else "fp32")
    return [("join_fwd_hip " + tag, fwd_hip, nbytes), ("join_fwd_aten " + tag, fwd_aten, nbytes),
            ("join_bwd_hip " + tag, bwd_hip, nbytes + n * z.element_size()), ("join_bwd_aten " + tag, bwd_aten, nbytes + n * z.element_size())]


def dropout_cases(shape, dev, lib):
    x = torch.rand(shape, device=dev) * 2 - 1
    y = torch.empty_like(x)
    mask = (torch.rand(shape, device=dev) >= 0.5).float()
    n, st = x.numel(), torch.cuda.current_stream().cuda_stream
    tag = "x".join(str(v) for v in shape)
    return [("dropout_hip " + tag, lambda: lib.cstp_dropout(st, x.data_ptr(), y.data_ptr(), n, 0.5, 0x15b7fa397883287b, 0), 8 * n),
            ("dropout_aten " + tag, lambda: x * mask * 2.0, 12 * n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, default=101)
    ap.add_argument("--steps", type=int, default=10, help="calls per window of a step case")
    ap.add_argument("--kernel_steps", type=int, default=50, help="calls per window of a kernel case")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="steps | kernels (default: both)")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_reg.py needs a HIP device: nothing is timed without one")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    cases = []       # (name, fn, calls per window, window function, bytes or None, workload)
    if a.only in ("", "steps"):
        for kind, b, t, hw in (("r21d18_fp32", 16, 16, 112), ("r3d50_bf16", 4, 16, 224)):
            torch.manual_seed(1)
            x = torch.rand((b, 3, t, hw, hw), device=dev) * 2 - 1
            lab = torch.randint(0, a.classes, (b,), device=dev)
            workload = "%s ft_all, B=%d, 3x%dx%dx%d, %d classes" % (kind, b, t, hw, hw, a.classes)
            for tag, reg in (("off", None), ("on", Regularizer(0.5, 0.1, seed=1))):
                step = make_step(kind, dev, reg, a.classes)
                cases.append(("%s_%s" % (kind, tag), (lambda step=step, x=x, lab=lab: step(x, lab)), a.steps, host_window, None, workload))
    if a.only in ("", "kernels"):
        for name, shape, dtype in (("r21d18 conv2", (16, 64, 16, 56, 56), torch.float32), ("r21d18 conv5", (16, 512, 2, 7, 7), torch.float32),
                                   ("r3d50 layer1", (4, 256, 8, 56, 56), torch.bfloat16), ("r3d50 layer4", (4, 2048, 1, 7, 7), torch.bfloat16)):
            for case, fn, nbytes in join_cases(name, shape, dtype, dev, lib):
                cases.append((case, fn, a.kernel_steps, event_window, nbytes, "block output of " + name))
        for shape in ((16, 512), (4, 2048)):
            for case, fn, nbytes in dropout_cases(shape, dev, lib):
                cases.append((case, fn, a.kernel_steps, event_window, nbytes, "classifier input"))
    for _, fn, _, _, _, _ in cases:
        for _ in range(a.warmup):
            fn()
    times = {c[0]: [] for c in cases}
    for _ in range(a.windows):
        for name, fn, calls, win, _, _ in cases:
            times[name].append(win(fn, calls))
    lines = []
    for name, _, calls, win, nbytes, workload in cases:
        t = times[name]
        rec = {"case": name, "workload": workload, "ms_per_call_median": round(statistics.median(t), 5), "ms_min": round(min(t), 5),
               "ms_max": round(max(t), 5), "windows": len(t), "calls_per_window": calls,
               "clock": "host, synchronised" if win is host_window else "device events"}
        if nbytes is not None:
            rate = nbytes / (statistics.median(t) * 1e-3)
            rec.update({"bytes": nbytes, "GB_per_s": round(rate / 1e9, 1), "share_of_8TBs_peak": round(rate / HBM_PEAK, 4)})
        lines.append(json.dumps(rec))
    for line in lines:
        print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

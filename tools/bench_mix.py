#!/usr/bin/env python3
"""What label smoothing / mixup / CutMix cost next to a fine-tune step on one MI355X, and the two kernels against the ATen
compositions they stand in for.

    python tools/bench_mix.py --windows 5 --steps 10 [--out profiles/r14/bench_mix.jsonl]

One process, the sides alternating window by window (so a drift of the box lands on all of them alike):
  step_off        R(2+1)D-18 ft_all step, 16 clips of 3x16x112x112, FineTuneStep(mixer=None)
  step_on         the same step with a Mixer (smoothing 0.1, mixup 0.8, CutMix 1.0, prob 1): plan, blend, soft-target loss
  mixup_hip/aten  ops.clip_mix (mode 1)           vs  lam*x + (1-lam)*x[perm]
  cutmix_hip/aten ops.clip_mix (mode 2)           vs  torch.where(mask, x[perm], x)
  loss_hip/aten   ops.soft_cross_entropy fwd+bwd  vs  F.cross_entropy(logits, q) fwd+bwd (q built from one_hot each call)
Every window is `steps` calls between two device synchronisations, timed with the host clock; the figure of a case is the median
of its windows (min / max kept).  One JSON line per case.  The kernels are microseconds: their windows time launch and
allocation as much as the kernel, which is how they run inside the step."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cstp_amd import ops  # noqa: E402
from cstp_amd.mix import Mixer  # noqa: E402
from cstp_amd.optim import FlatSGD  # noqa: E402
from cstp_amd.r21d_byol import R21DBYOL, get_fine_tuning_parameters, layer_sizes_for_depth  # noqa: E402
from cstp_amd.train import FineTuneStep  # noqa: E402


def window(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def make_step(a, dev, mixer):
    torch.manual_seed(1)
    model = R21DBYOL(pretrain=False, num_classes=a.classes, cls_bn=True, layer_sizes=layer_sizes_for_depth(a.depth)).to(dev)
    arenas = model.flatten_parameters()
    opt = FlatSGD(get_fine_tuning_parameters(model, 0), lr=0.01, momentum=0.9, weight_decay=5e-4, arenas=arenas)
    model.train()
    return FineTuneStep(model, opt, "ft_all", mixer=mixer)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=18)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=112)
    ap.add_argument("--classes", type=int, default=101)
    ap.add_argument("--steps", type=int, default=10, help="calls per window of a step case")
    ap.add_argument("--kernel_steps", type=int, default=200, help="calls per window of a kernel case")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mix.py needs a HIP device: nothing is timed without one")
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    b, k, s = a.batch, a.classes, a.size
    x = torch.rand((b, 3, a.frames, s, s), device=dev) * 2 - 1
    y = torch.randint(0, k, (b,), device=dev)
    logits = (torch.rand((b, k), device=dev) * 6 - 3).requires_grad_(True)
    perm_list = [(i + 1) % b for i in range(b)]
    perm = torch.tensor(perm_list, device=dev)
    tb = y[perm]
    lam, eps = 0.3, 0.1
    lam_t = torch.full((b,), lam, device=dev)
    box = (s // 4, s // 4 + s // 2, s // 4 + 1, s // 4 + 1 + s // 2)          # x0 off the 16-byte groups
    mask = torch.zeros((1, 1, 1, s, s), dtype=torch.bool, device=dev)
    mask[..., box[0]:box[1], box[2]:box[3]] = True
    step_off = make_step(a, dev, None)
    step_on = make_step(a, dev, Mixer(eps, 0.8, 1.0, 1.0, 0.5, seed=1))

    def loss_hip():
        logits.grad = None
        ops.soft_cross_entropy(logits, y, tb, lam_t, eps).backward()

    def loss_aten():
        logits.grad = None
        q = (1 - eps) * (lam_t[:, None] * F.one_hot(y, k) + (1 - lam_t)[:, None] * F.one_hot(tb, k)) + eps / k
        F.cross_entropy(logits, q).backward()

    cases = [
        ("step_off", lambda: step_off(x, y), a.steps),
        ("step_on", lambda: step_on(x, y), a.steps),
        ("mixup_hip", lambda: ops.clip_mix(x, perm_list, 1, lam), a.kernel_steps),
        ("mixup_aten", lambda: lam * x + (1 - lam) * x[perm], a.kernel_steps),
        ("cutmix_hip", lambda: ops.clip_mix(x, perm_list, 2, lam, box), a.kernel_steps),
        ("cutmix_aten", lambda: torch.where(mask, x[perm], x), a.kernel_steps),
        ("loss_hip", loss_hip, a.kernel_steps),
        ("loss_aten", loss_aten, a.kernel_steps),
    ]
    for _, fn, _ in cases:
        for _ in range(a.warmup):
            fn()
    times = {name: [] for name, _, _ in cases}
    for _ in range(a.windows):
        for name, fn, steps in cases:
            times[name].append(window(fn, steps))
    workload = "R(2+1)D-%d ft_all, B=%d, 3x%dx%dx%d, %d classes" % (a.depth, b, a.frames, s, s, k)
    lines = []
    for name, _, steps in cases:
        t = times[name]
        lines.append(json.dumps({"case": name, "workload": workload, "ms_per_call_median": round(statistics.median(t), 4),
                                 "ms_min": round(min(t), 4), "ms_max": round(max(t), 4), "windows": len(t),
                                 "calls_per_window": steps}))
    for line in lines:
        print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Label smoothing, mixup and CutMix for fine-tuning: the host side (no device work here).

``Mixer.plan`` decides, once per batch (the "batch" mode of the usual Mixup implementation: one draw serves every sample),
whether and how the clips of a batch are blended; ``ops.clip_mix`` executes the plan on the device in one launch and
``ops.soft_cross_entropy`` computes the loss against the two weighted, smoothed targets.

The plan is a pure function of ``(seed, epoch, step, rank)`` and the batch geometry: it draws from a private
``numpy.random.Generator`` seeded from exactly those four numbers and never touches the global ``torch`` / ``numpy`` /
``random`` streams, so a resumed run that starts at its epoch reproduces the plans of the uninterrupted one, ranks draw
different plans without communicating, and a test can re-derive the plan a step used.

Order of the draws (fixed; a draw whose outcome is already decided is not made):
  1. u ~ U[0, 1): the batch is mixed iff u < prob                       (skipped when both alphas are 0: never mixed)
  2. u ~ U[0, 1): CutMix iff u < switch_prob, mixup otherwise           (only when both alphas are positive)
  3. lam ~ Beta(alpha, alpha) with the chosen mode's alpha
  4. a permutation of the batch: sample i is blended with sample partner[i]
  5. CutMix only: the box centre, cy ~ U{0..h-1} then cx ~ U{0..w-1}
CutMix geometry: cut ratio r = sqrt(1 - lam), box sides int(h*r) x int(w*r), the box placed with its centre at (cy, cx)
(y0 = cy - side//2, y1 = y0 + side), clipped to the frame, the same in every frame of the clip; lam is then replaced by
1 - box_area / (h*w), the share of the sample that survives.  A plan that would change nothing (not mixed, or lam == 1: an
empty box) is the identity: mode 0, lam 1, partner[i] = i.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

MODE_COPY, MODE_MIXUP, MODE_CUTMIX = 0, 1, 2


class MixPlan(NamedTuple):
    mode: int                         # MODE_COPY | MODE_MIXUP | MODE_CUTMIX, the same for every sample of the batch
    lam: float                        # weight of a sample's own target (and, under mixup, of its own pixels)
    partner: List[int]                # a permutation of range(batch); the identity permutation for an identity plan
    box: Tuple[int, int, int, int]    # (y0, y1, x0, x1), half-open; (0, 0, 0, 0) unless CutMix
    applied: bool                     # outcome of draw 1 (a mixed batch may still come out as the identity: empty box)

    @property
    def identity(self) -> bool:
        return self.mode == MODE_COPY


def _check(name, value, lo, hi, closed_hi):
    v = float(value)
    ok = lo <= v <= hi if closed_hi else lo <= v < hi
    if not ok or math.isnan(v):
        raise ValueError("--%s must lie in [%g, %g%s, got %r" % (name, lo, hi, "]" if closed_hi else ")", value))
    return v


class Mixer:
    """Per-batch mixup / CutMix plans and the label-smoothing weight of the loss.  Refuses negative alphas, smoothing outside
    [0, 1) and probabilities outside [0, 1] with a ValueError naming the command-line flag."""

    def __init__(self, label_smoothing=0.0, mixup_alpha=0.0, cutmix_alpha=0.0, prob=1.0, switch_prob=0.5, seed=0):
        self.label_smoothing = _check("label_smoothing", label_smoothing, 0.0, 1.0, False)
        self.mixup_alpha = _check("mixup_alpha", mixup_alpha, 0.0, math.inf, False)
        self.cutmix_alpha = _check("cutmix_alpha", cutmix_alpha, 0.0, math.inf, False)
        self.prob = _check("mix_prob", prob, 0.0, 1.0, True)
        self.switch_prob = _check("mix_switch_prob", switch_prob, 0.0, 1.0, True)
        self.seed = int(seed)
        if self.seed < 0:
            raise ValueError("the mixer's seed must not be negative, got %r" % (seed,))

    @property
    def mixes(self) -> bool:
        """False for a smoothing-only mixer: every plan is the identity."""
        return self.mixup_alpha > 0.0 or self.cutmix_alpha > 0.0

    def plan(self, batch: int, h: int, w: int, epoch: int, step: int, rank: int = 0) -> MixPlan:
        if batch <= 0 or h <= 0 or w <= 0:
            raise ValueError("plan needs a positive batch and frame size, got batch %r, %r x %r" % (batch, h, w))
        if epoch < 0 or step < 0 or rank < 0:
            raise ValueError("plan needs non-negative epoch, step and rank, got %r, %r, %r" % (epoch, step, rank))
        ident = MixPlan(MODE_COPY, 1.0, list(range(batch)), (0, 0, 0, 0), False)
        if not self.mixes:
            return ident
        rng = np.random.default_rng([self.seed, int(epoch), int(step), int(rank)])
        if not rng.random() < self.prob:                                               # 1
            return ident
        if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
            cutmix = bool(rng.random() < self.switch_prob)                             # 2
        else:
            cutmix = self.cutmix_alpha > 0.0
        alpha = self.cutmix_alpha if cutmix else self.mixup_alpha
        lam = min(max(float(rng.beta(alpha, alpha)), 0.0), 1.0)                        # 3
        partner = [int(p) for p in rng.permutation(batch)]                             # 4
        box = (0, 0, 0, 0)
        if cutmix:
            r = math.sqrt(1.0 - lam)
            ch, cw = int(h * r), int(w * r)
            cy, cx = int(rng.integers(h)), int(rng.integers(w))                        # 5
            y0, x0 = cy - ch // 2, cx - cw // 2
            y1, x1 = min(max(y0 + ch, 0), h), min(max(x0 + cw, 0), w)
            y0, x0 = min(max(y0, 0), h), min(max(x0, 0), w)
            box = (y0, y1, x0, x1)
            lam = 1.0 - ((y1 - y0) * (x1 - x0)) / float(h * w)
        if lam == 1.0:
            return ident._replace(applied=True)
        return MixPlan(MODE_CUTMIX if cutmix else MODE_MIXUP, lam, partner, box, True)


def target_distribution(ta, tb, lam, eps, k):
    """q [rows][k] in float64 (numpy) as ops.soft_cross_entropy defines it: (1-eps)*(lam*onehot(ta) + (1-lam)*onehot(tb)) +
    eps/k; a target outside [0, k) adds no one-hot mass.  A restatement for tests and documentation, not used by the step."""
    ta, tb = np.asarray(ta, dtype=np.int64), np.asarray(tb, dtype=np.int64)
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), ta.shape)
    q = np.full((ta.shape[0], k), float(eps) / k, dtype=np.float64)
    for r in range(ta.shape[0]):
        if 0 <= ta[r] < k:
            q[r, ta[r]] += (1.0 - eps) * lam[r]
        if 0 <= tb[r] < k:
            q[r, tb[r]] += (1.0 - eps) * (1.0 - lam[r])
    return q


def build_mixer(opts) -> Optional[Mixer]:
    """The Mixer of --label_smoothing / --mixup_alpha / --cutmix_alpha / --mix_prob / --mix_switch_prob (seeded with
    --manual_seed), or None when the first three are all 0: the step then runs exactly as it does without these flags."""
    mixer = Mixer(opts.label_smoothing, opts.mixup_alpha, opts.cutmix_alpha, opts.mix_prob, opts.mix_switch_prob,
                  seed=opts.manual_seed)
    if mixer.label_smoothing == 0.0 and not mixer.mixes:
        return None
    return mixer

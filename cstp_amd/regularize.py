"""Dropout and stochastic depth (drop-path) for fine-tuning: the host side (no device work here).

``Regularizer.plan`` decides, once per step, the key of the dropout mask in front of the classifier and which residual blocks
each sample skips; ``ops.dropout`` and ``ops.drop_path_add_relu`` execute it on the device (cstp_dropout,
cstp_droppath_add_relu_*).  As with cstp_amd.mix, the plan is a pure function of ``(seed, epoch, step, rank)`` and the geometry:
it draws from a private ``numpy.random.Generator`` seeded from exactly those numbers (and a constant that keeps its stream apart
from the mixer's) and never touches the global ``torch`` / ``numpy`` / ``random`` streams, so a resumed run that starts at its
epoch reproduces the plans of the uninterrupted one, ranks draw different plans without communicating, and a test can re-derive
the plan a step used.

Order of the draws (fixed; a draw whose flag is 0 is not made):
  1. dropout > 0:    key = one uint64; the mask itself is Philox4x32-10 of (key, call-site offset, element index) on the device
  2. drop_path > 0:  u ~ U[0, 1) of shape [n_blocks][batch]; block l keeps sample b iff u[l][b] >= p_l
Stochastic depth follows the linear rule of Huang et al. (2016): block l of L, in forward order across the stages, is dropped
with p_l = drop_path * l / (L - 1) -- the first block never, the last with the flag's value -- and a kept sample's branch is
scaled by 1 / (1 - p_l), so the expectation of the block's output is that of the unregularised block.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional

import numpy as np

from .mix import _check

STREAM = 0x5EED          # fifth seed word: the regulariser's generator is not the mixer's

DROP_PATH_MODELS = ("r21d_byol", "r3d_byol")       # the backbones with residual blocks


class RegPlan(NamedTuple):
    key: Optional[int]                # seed of the dropout mask (uint64), None when dropout is off
    keep: Optional[np.ndarray]        # bool [n_blocks][batch]: block l runs its branch for sample b; None when drop-path is off
    scale: Optional[np.ndarray]       # fp32 [n_blocks][batch]: keep / (1 - p_l), what the device multiplies the branch by
    p: List[float]                    # p_l per block (all 0 when drop-path is off)


def block_probabilities(drop_path: float, n_blocks: int) -> List[float]:
    """p_l = drop_path * l / (L - 1) for l = 0 .. L - 1 (a single block is block 0: never dropped)."""
    if n_blocks <= 1:
        return [0.0] * max(n_blocks, 0)
    return [float(drop_path) * l / (n_blocks - 1) for l in range(n_blocks)]


class Regularizer:
    """Per-step dropout keys and drop-path tables.  Refuses probabilities outside [0, 1) with a ValueError naming the flag."""

    def __init__(self, dropout=0.0, drop_path=0.0, seed=0):
        self.dropout = _check("dropout", dropout, 0.0, 1.0, False)
        self.drop_path = _check("drop_path", drop_path, 0.0, 1.0, False)
        self.seed = int(seed)
        if self.seed < 0:
            raise ValueError("the regulariser's seed must not be negative, got %r" % (seed,))

    @property
    def active(self) -> bool:
        return self.dropout > 0.0 or self.drop_path > 0.0

    def plan(self, batch: int, n_blocks: int, epoch: int, step: int, rank: int = 0) -> RegPlan:
        if batch <= 0 or n_blocks < 0:
            raise ValueError("plan needs a positive batch and a block count, got batch %r, %r blocks" % (batch, n_blocks))
        if epoch < 0 or step < 0 or rank < 0:
            raise ValueError("plan needs non-negative epoch, step and rank, got %r, %r, %r" % (epoch, step, rank))
        rng = np.random.default_rng([self.seed, int(epoch), int(step), int(rank), STREAM])
        key = None
        if self.dropout > 0.0:
            key = int(rng.integers(0, 2 ** 64, dtype=np.uint64))                        # 1
        p = block_probabilities(self.drop_path, n_blocks)
        keep = scale = None
        if self.drop_path > 0.0 and n_blocks > 0:
            u = rng.random((n_blocks, batch))                                           # 2
            pl = np.asarray(p, dtype=np.float64)[:, None]
            keep = u >= pl
            scale = (keep / (1.0 - pl)).astype(np.float32)
        return RegPlan(key, keep, scale, p)


def check_flags(dropout, drop_path, model_name, task):
    """The flag rules of --dropout / --drop_path: ranges as cstp_amd.mix refuses them; --drop_path needs a backbone with residual
    blocks and a task that trains them."""
    _check("dropout", dropout, 0.0, 1.0, False)
    if _check("drop_path", drop_path, 0.0, 1.0, False) > 0.0:
        if model_name not in DROP_PATH_MODELS:
            raise ValueError("--drop_path needs residual blocks: --model_name %s have them, %r has no residual branch to drop"
                             % (" | ".join(DROP_PATH_MODELS), model_name))
        if task == "ft_fc":
            raise ValueError("--drop_path with --task ft_fc: nothing inside a dropped branch is trained (the encoder is frozen); "
                             "use --task ft_all")


def build_regularizer(opts) -> Optional[Regularizer]:
    """The Regularizer of --dropout / --drop_path (seeded with --manual_seed), or None when both are 0: the step then runs exactly
    as it does without these flags."""
    dropout, drop_path = getattr(opts, "dropout", 0.0), getattr(opts, "drop_path", 0.0)
    check_flags(dropout, drop_path, getattr(opts, "model_name", None), getattr(opts, "task", None))
    reg = Regularizer(dropout, drop_path, seed=opts.manual_seed)
    return reg if reg.active else None

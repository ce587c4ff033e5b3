"""The optimisation half of the fine-tuning recipe (main_ft_mp.py): layer-wise learning-rate decay, no weight decay on biases
and BatchNorm parameters, an exponential moving average of the weights, and a per-iteration warm-up + cosine schedule.  Host side
only; the device work is optim.TableSGD / TableAdam (csrc/optim_table.h: one launch per step whatever the grouping, the EMA in the
same pass) and ops.ema_update_.

  --layer_decay D     tensor of layer l of L trains at lr * D ** (L - l): the stem is layer 0, residual block b (1-based, forward
                      order) is layer b, the classifier head is layer L = blocks + 1 (layer_ids)
  --wd_skip_1d 1      tensors with dim() <= 1 (biases, BatchNorm gamma / beta) get weight decay 0
  --model_ema M       shadow <- m * shadow + (1 - m) * weights after every step, m = min(M, (1 + t) / (10 + t)) at update t;
                      validation, the plateau metric and the best checkpoint use the shadow (ema_applied); the checkpoint gains
                      ``state_dict_ema`` next to the unchanged ``state_dict``
  --lr_schedule cosine  WarmupCosine stepped once per iteration in place of ReduceLROnPlateau (--warmup_epochs, --min_lr)
Everything is off by default: build_optimizer / build_scheduler then return exactly what the driver built before these flags.
"""
from __future__ import annotations

import contextlib
import math
from typing import NamedTuple

import torch

from . import optim
from .mix import _check
from .scheduler import ReduceLROnPlateau

LAYER_DECAY_MODELS = ("r21d_byol", "r3d_byol")       # the backbones with residual blocks to number
LAYER_DECAY_TASKS = ("ft_all", "scratch", "resume")
HEAD_MODULES = ("classify", "cls_bn", "classify_bn")  # the classifier and the BatchNorm1d in front of it (either spelling)


class Recipe(NamedTuple):
    layer_decay: float
    wd_skip_1d: bool
    model_ema: float
    lr_schedule: str
    warmup_epochs: int
    min_lr: float

    @property
    def table(self) -> bool:
        """Whether the step needs the table optimisers (per-tensor hyper-parameters or the fused EMA)."""
        return self.layer_decay != 1.0 or self.wd_skip_1d or self.model_ema > 0.0


def _flag01(name, value):
    if value not in (0, 1, False, True):
        raise ValueError("--%s is 0 or 1, got %r" % (name, value))
    return bool(value)


def check_flags(opts) -> Recipe:
    """The rules of --layer_decay / --wd_skip_1d / --model_ema / --lr_schedule / --warmup_epochs / --min_lr / --test_ema, each
    refusal naming its flag; reads only ``opts``, so it runs before any data or model is built."""
    layer_decay = float(getattr(opts, "layer_decay", 1.0))
    if not (0.0 < layer_decay <= 1.0):
        raise ValueError("--layer_decay must lie in (0, 1], got %r" % (getattr(opts, "layer_decay"),))
    wd_skip_1d = _flag01("wd_skip_1d", getattr(opts, "wd_skip_1d", 0))
    model_ema = _check("model_ema", getattr(opts, "model_ema", 0.0), 0.0, 1.0, False)
    _flag01("test_ema", getattr(opts, "test_ema", 0))
    model_name, task = getattr(opts, "model_name", None), getattr(opts, "task", None)
    if layer_decay != 1.0:
        if model_name not in LAYER_DECAY_MODELS:
            raise ValueError("--layer_decay numbers residual blocks: --model_name %s have them, %r is not served"
                             % (" | ".join(LAYER_DECAY_MODELS), model_name))
        if task not in LAYER_DECAY_TASKS:
            raise ValueError("--layer_decay with --task %s: the encoder is not trained (only %s train it)"
                             % (task, " / ".join(LAYER_DECAY_TASKS)))
    optimizer = getattr(opts, "optimizer", "sgd")
    if optimizer == "lars":
        if layer_decay != 1.0:
            raise ValueError("--layer_decay with --optimizer lars: LARS sets each tensor's step by its own trust ratio")
        if wd_skip_1d:
            raise ValueError("--wd_skip_1d with --optimizer lars: LARS already exempts tensors with dim() <= 1 from weight decay")
    lr_schedule = getattr(opts, "lr_schedule", "plateau")
    if lr_schedule not in ("plateau", "cosine"):
        raise ValueError("--lr_schedule is plateau or cosine, got %r" % (lr_schedule,))
    warmup_epochs = getattr(opts, "warmup_epochs", 0)
    if int(warmup_epochs) != warmup_epochs or warmup_epochs < 0:
        raise ValueError("--warmup_epochs must be an integer >= 0, got %r" % (warmup_epochs,))
    if lr_schedule == "cosine" and not warmup_epochs < getattr(opts, "n_epochs", 1):
        raise ValueError("--warmup_epochs %d must be fewer than --n_epochs %d" % (warmup_epochs, getattr(opts, "n_epochs", 1)))
    min_lr = float(getattr(opts, "min_lr", 0.0))
    if not (0.0 <= min_lr < float("inf")):
        raise ValueError("--min_lr must be finite and >= 0, got %r" % (getattr(opts, "min_lr"),))
    return Recipe(layer_decay, wd_skip_1d, model_ema, lr_schedule, int(warmup_epochs), min_lr)


# ---- parameter groups ------------------------------------------------------------------------------------------------------------
def layer_ids(inner):
    """{parameter name: layer} over every parameter of a fine-tune model with residual blocks (r21d_byol, r3d_byol; BasicBlock and
    Bottleneck): the stem (online_net.conv1, online_net.bn1) is layer 0, residual block b of ``inner.residual_blocks()`` (1-based,
    forward order) is layer b, the head (classify and the BatchNorm1d in front of it) is layer L = blocks + 1.  An encoder
    parameter in none of these is an error, not a guess."""
    blocks = inner.residual_blocks() if hasattr(inner, "residual_blocks") and hasattr(inner, "online_net") else []
    if not blocks:
        raise ValueError("--layer_decay numbers residual blocks and %s has none (served: %s)"
                         % (type(inner).__name__, " | ".join(LAYER_DECAY_MODELS)))
    owner = {}
    for name in ("conv1", "bn1"):
        for p in getattr(inner.online_net, name).parameters():
            owner[id(p)] = 0
    for b, block in enumerate(blocks, 1):
        for p in block.parameters():
            owner[id(p)] = b
    head = len(blocks) + 1
    ids = {}
    for name, p in inner.named_parameters():
        if id(p) in owner:
            ids[name] = owner[id(p)]
        elif name.split(".")[0] in HEAD_MODULES:
            ids[name] = head
        else:
            raise ValueError("--layer_decay: parameter %r of %s is neither the stem, a residual block nor the classifier head"
                             % (name, type(inner).__name__))
    return ids


def param_groups(inner, parameters, layer_decay=1.0, wd=0.0, wd_skip_1d=False):
    """One group per tensor for TableSGD / TableAdam, in the order of ``parameters`` (``model.parameters()`` or the per-tensor list
    of get_fine_tuning_parameters) and with its conventions: a frozen tensor (requires_grad False) is listed at ``lr 0.0``.
      lr_scale     = layer_decay ** (L - layer)        (1 for every tensor at layer_decay 1; layer_ids is then not consulted)
      weight_decay = 0 for dim() <= 1 tensors when wd_skip_1d, else wd"""
    names = {id(p): n for n, p in inner.named_parameters()}
    ids = layer_ids(inner) if layer_decay != 1.0 else None
    top = max(ids.values()) if ids else 0
    groups = []
    for entry in parameters:
        given = dict(entry) if isinstance(entry, dict) else {"params": entry}
        p = given["params"]
        if not isinstance(p, torch.Tensor):
            raise ValueError("param_groups takes one tensor per group, as get_fine_tuning_parameters lists them")
        if id(p) not in names:
            raise ValueError("a parameter of shape %s is not one of the model's" % (tuple(p.shape),))
        group = {"params": p,
                 "lr_scale": 1.0 if ids is None else float(layer_decay) ** (top - ids[names[id(p)]]),
                 "weight_decay": 0.0 if (wd_skip_1d and p.dim() <= 1) else float(wd)}
        if not p.requires_grad or given.get("lr") == 0.0:
            group["lr"] = 0.0
        groups.append(group)
    return groups


def build_optimizer(opts, inner, parameters, arenas):
    """optim.build_optimizer when none of --layer_decay / --wd_skip_1d / --model_ema is set (exactly today's object); otherwise
    TableSGD / TableAdam on param_groups -- or FlatLARS, which takes --model_ema alone.  The EMA itself is switched on by the
    driver (``optimizer.enable_ema``) after the checkpoint has been loaded."""
    recipe = check_flags(opts)
    if not recipe.table or opts.optimizer == "lars":
        return optim.build_optimizer(opts, parameters, arenas)
    groups = param_groups(inner, parameters, recipe.layer_decay, opts.weight_decay, recipe.wd_skip_1d)
    if opts.optimizer == "sgd":
        return optim.TableSGD(groups, lr=opts.learning_rate, momentum=opts.momentum, weight_decay=opts.weight_decay, arenas=arenas)
    if opts.optimizer == "adamw":
        return optim.TableAdam(groups, lr=opts.learning_rate, betas=(0.9, 0.99), weight_decay=opts.weight_decay, decoupled=True,
                               arenas=arenas)
    if opts.optimizer == "adam":
        return optim.TableAdam(groups, lr=opts.learning_rate, weight_decay=opts.weight_decay, arenas=arenas)
    raise ValueError("unknown --optimizer %r (sgd / adam / adamw / lars)" % (opts.optimizer,))


# ---- schedule --------------------------------------------------------------------------------------------------------------------
def warmup_cosine(i, base, total, warmup=0, min_lr=0.0):
    """The learning rate of global iteration i (0-based) of ``total``: base * (i + 1) / warmup below ``warmup``, then the half
    cosine min_lr + (base - min_lr) * (1 + cos(pi * (i - warmup) / (total - warmup))) / 2, which reaches min_lr at i = total."""
    if not 0 <= warmup < total:
        raise ValueError("warm-up of %r iterations in a schedule of %r" % (warmup, total))
    i = min(max(int(i), 0), total)
    if i < warmup:
        return base * (i + 1) / warmup
    return min_lr + (base - min_lr) * (1.0 + math.cos(math.pi * (i - warmup) / (total - warmup))) / 2.0


class WarmupCosine:
    """Per-iteration warm-up + cosine: step() sets every group's lr to warmup_cosine(i) * lr_scale (a group at lr 0.0, the frozen
    convention, stays there) and moves on to the next iteration.  A pure function of the global iteration, so there is nothing to
    checkpoint: a resumed run passes ``start`` = (begin_epoch - 1) * iterations per epoch."""

    def __init__(self, optimizer, base_lr, total_iters, warmup_iters=0, min_lr=0.0, start=0):
        if not 0 <= warmup_iters < total_iters:
            raise ValueError("warm-up of %r iterations in a schedule of %r" % (warmup_iters, total_iters))
        self.optimizer, self.base_lr, self.min_lr = optimizer, float(base_lr), float(min_lr)
        self.total_iters, self.warmup_iters = int(total_iters), int(warmup_iters)
        self.iteration = int(start)
        self._frozen = [float(g["lr"]) == 0.0 for g in optimizer.param_groups]

    def value(self, i=None):
        return warmup_cosine(self.iteration if i is None else i, self.base_lr, self.total_iters, self.warmup_iters, self.min_lr)

    def step(self):
        lr = self.value()
        for g, frozen in zip(self.optimizer.param_groups, self._frozen):
            g["lr"] = 0.0 if frozen else lr * float(g.get("lr_scale", 1.0))
        self.iteration += 1
        return lr


def build_scheduler(opts, optimizer, iters_per_epoch, begin_epoch=1):
    """--lr_schedule plateau: today's ReduceLROnPlateau(optimizer, 'min', patience=--lr_patience), stepped per epoch with the
    validation loss.  cosine: WarmupCosine over n_epochs * iters_per_epoch iterations, positioned at ``begin_epoch``."""
    recipe = check_flags(opts)
    if recipe.lr_schedule == "plateau":
        return ReduceLROnPlateau(optimizer, "min", patience=opts.lr_patience)
    if iters_per_epoch < 1:
        raise ValueError("--lr_schedule cosine needs at least one iteration per epoch, got %r" % (iters_per_epoch,))
    return WarmupCosine(optimizer, opts.learning_rate, opts.n_epochs * iters_per_epoch, recipe.warmup_epochs * iters_per_epoch,
                        recipe.min_lr, start=(begin_epoch - 1) * iters_per_epoch)


# ---- the EMA weights -------------------------------------------------------------------------------------------------------------
def _swap(a, b):
    tmp = a.clone()
    a.copy_(b)
    b.copy_(tmp)


@contextlib.contextmanager
def ema_applied(inner, optimizer):
    """Within the context the model holds the EMA weights and EMA BatchNorm statistics (and the optimizer's shadows hold the raw
    ones); on exit both are swapped back, bit for bit.  Plain copies through a scratch buffer: this runs once per epoch.
    ``inner`` is the unwrapped model whose flatten_parameters() built the optimizer's arenas."""
    if getattr(optimizer, "_ema", None) is None:
        raise ValueError("ema_applied needs optimizer.enable_ema(momentum) first (--model_ema)")
    arenas = inner.flatten_parameters()
    if arenas["param"].data_ptr() != optimizer._p.data_ptr():
        raise ValueError("ema_applied: the optimizer was not built on this model's arenas")
    pairs = [(arenas["param"], optimizer._ema)]
    if optimizer._ema_buffers is not None:
        pairs.append((arenas["buffers"], optimizer._ema_buffers))
    with torch.no_grad():
        for a, b in pairs:
            _swap(a, b)
    try:
        yield
    finally:
        with torch.no_grad():
            for a, b in pairs:
                _swap(a, b)


def ema_state_dict(model, inner, optimizer):
    """``model.state_dict()`` with the EMA weights and EMA BatchNorm statistics in place of the raw ones: same keys, cloned."""
    with ema_applied(inner, optimizer):
        return {k: v.clone() for k, v in model.state_dict().items()}


def load_ema_state_dict(model, inner, optimizer, state_dict_ema):
    """Restores the shadows from a checkpoint's ``state_dict_ema`` (--task resume); the model's own weights, statistics and
    counters are left as they are."""
    counters = inner.flatten_parameters()["nbt_all"].clone()
    with ema_applied(inner, optimizer):
        model.load_state_dict(state_dict_ema)
    with torch.no_grad():
        inner.flatten_parameters()["nbt_all"].copy_(counters)

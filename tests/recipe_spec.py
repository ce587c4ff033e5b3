"""Restatement of the fine-tuning recipe's arithmetic, from the formulas in include/cstp_hip.h (cstp_tab_sgd_step,
cstp_tab_adam_step, cstp_ema_update) and cstp_amd/recipe.py's docstring -- not the code under test.  Everything runs in the dtype of
its tensor arguments (fp64 for the reference, fp32 to show what fp32 arithmetic alone costs); scalars are Python floats."""
import math


def sgd_step(p, g, buf, c, lr, scale, momentum, wd, first_step):
    """One tensor of the table SGD step -> (p, written-back g, buf)."""
    g = c * g
    d = g + wd * p
    buf = d if first_step else momentum * buf + d
    return p - (lr * scale) * buf, g, buf


def adam_step(p, g, m, v, lr, scale, b1, b2, eps, wd, decoupled, step):
    """One tensor of the table Adam (decoupled False) / AdamW (True) step, ``step`` counted from 1 -> (p, m, v)."""
    l = lr * scale
    if decoupled:
        p = p * (1.0 - l * wd)
    else:
        g = g + wd * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    p = p - l / (1.0 - b1 ** step) * (m / (v.sqrt() / math.sqrt(1.0 - b2 ** step) + eps))
    return p, m, v


def ema_momentum(momentum, t):
    """Momentum of shadow update t (counted from 1)."""
    return min(momentum, (1.0 + t) / (10.0 + t))


def ema_update(ema, p, momentum, t):
    m = ema_momentum(momentum, t)
    return m * ema + (1.0 - m) * p


def warmup_cosine(i, base, total, warmup, min_lr):
    """Learning rate of global iteration i (0-based) of ``total`` with ``warmup`` warm-up iterations."""
    if i < warmup:
        return base * (i + 1) / warmup
    return min_lr + (base - min_lr) * (1 + math.cos(math.pi * (i - warmup) / (total - warmup))) / 2

"""The training loss, TULIP(loss="l1" | "l2" | "berhu") -- the host definition of what csrc/loss.hip computes on the device.

The reference's forward_loss is L1 (tulip.py:690-700), and that stays the default.  The alternative it imports and leaves unused
(tulip.py:11, util/evaluation.py:177-180, inverse_huber_loss) is berHu, the usual depth-regression loss; L2 is its other half.
With d = pred - target and n = pred.numel():

    l1      loss = mean |d|                                   gradient  sign(d) / n
    l2      loss = mean d^2                                   gradient  2 d / n
    berhu   C = 0.2 * max |d|                                 (read with .item() in the reference: a constant under autograd)
            value_i = |d_i| where |d_i| < C, else (d_i^2 + C^2) / (2 C)
            loss = mean value_i                               (the reference function returns the elementwise tensor; the mean is
                                                               how forward_loss would use it)
            gradient  sign(d_i) / n where |d_i| < C, else d_i / (C n)           -- nothing flows through C

One departure from the reference: C == 0 (pred equals target everywhere) makes its formula 0/0 = NaN; here loss and gradient are 0,
so that a perfect prediction is not a non-finite step.  A NaN or an infinity anywhere in pred or target makes the loss non-finite
and at least the affected gradient elements with it (numpy's max keeps a NaN; the device's max is written to do the same), so the
non-finite guard and train_one_epoch's abort still see it.  `pixel_loss`, the second value the model returns, keeps its meaning for
every kind: the L1 metric, mean |expm1(pred) - expm1(target)| with log_transform and mean |pred - target| without.

The functions below are that table in numpy float64 (the device works in float32: C there is the float32 product
float32(0.2) * float32(max |d|), `berhu_c32`).  With world > 1 and with accum_iter > 1 C is per rank and per micro-batch, as in the
reference, where every rank computes its own loss on its own batch.
"""
from __future__ import annotations

import numpy as np

KINDS = ("l1", "l2", "berhu")
BERHU_FRACTION = 0.2


def check_loss(name) -> str:
    """The loss of TULIP(loss=...): "l1", "l2" or "berhu" (ValueError for anything else)."""
    if not isinstance(name, str) or name not in KINDS:
        raise ValueError(f"loss must be one of {KINDS}, got {name!r}")
    return name


def _diff(pred, target):
    pred, target = np.asarray(pred, dtype=np.float64), np.asarray(target, dtype=np.float64)
    with np.errstate(all="ignore"):
        return pred - target


def berhu_c(pred, target) -> np.float64:
    """C = 0.2 * max |pred - target| in float64 (NaN when any difference is NaN)."""
    with np.errstate(all="ignore"):
        return np.float64(BERHU_FRACTION) * np.max(np.abs(_diff(pred, target)))


def berhu_c32(pred, target) -> np.float32:
    """The device's C: float32(0.2) * float32(max |d|), d formed in float32 -- one float32 product."""
    with np.errstate(all="ignore"):
        d = np.asarray(pred, dtype=np.float32) - np.asarray(target, dtype=np.float32)
        return np.float32(BERHU_FRACTION) * np.float32(np.max(np.abs(d)))


def berhu_values(pred, target, c=None) -> np.ndarray:
    """The elementwise berHu values (what inverse_huber_loss returns) for the threshold c (default: berhu_c)."""
    d = _diff(pred, target)
    c = berhu_c(pred, target) if c is None else np.float64(c)
    if c == 0.0:
        return np.zeros_like(d)
    a = np.abs(d)
    with np.errstate(all="ignore"):
        return np.where(a < c, a, (a * a + c * c) / (2.0 * c))


def loss_value(kind: str, pred, target) -> np.float64:
    """The scalar training loss of `kind` in float64."""
    kind = check_loss(kind)
    d = _diff(pred, target)
    with np.errstate(all="ignore"):
        if kind == "l1":
            return np.mean(np.abs(d))
        if kind == "l2":
            return np.mean(d * d)
        return np.mean(berhu_values(pred, target))


def loss_grad(kind: str, pred, target, gscale: float = 1.0) -> np.ndarray:
    """gscale * d(loss_value) / d(pred) in float64, the shape of pred."""
    kind = check_loss(kind)
    d = _diff(pred, target)
    n = d.size
    with np.errstate(all="ignore"):
        if kind == "l1":
            g = np.sign(d) / n
        elif kind == "l2":
            g = 2.0 * d / n
        else:
            c = berhu_c(pred, target)
            g = np.zeros_like(d) if c == 0.0 else np.where(np.abs(d) < c, np.sign(d) / n, d / (c * n))
        return np.float64(gscale) * g


def pixel_loss(pred, target, log_transform: bool) -> np.float64:
    """The logged L1 metric, the same for every kind (tulip.py:695-698)."""
    pred, target = np.asarray(pred, dtype=np.float64), np.asarray(target, dtype=np.float64)
    with np.errstate(all="ignore"):
        if log_transform:
            return np.mean(np.abs(np.expm1(pred) - np.expm1(target)))
        return np.mean(np.abs(pred - target))


def torch_loss(kind: str, pred, target):
    """The same definition on torch tensors, differentiable in pred (C detached, as the reference's .item() leaves it): what a
    test or a CPU experiment back-propagates through an autograd model."""
    import torch
    kind = check_loss(kind)
    d = pred - target
    if kind == "l1":
        return d.abs().mean()
    if kind == "l2":
        return (d * d).mean()
    a = d.abs()
    c = (BERHU_FRACTION * a.detach().max()).item()
    if c == 0.0:
        return (a * 0.0).mean()
    return torch.where(a < c, a, (a * a + c * c) / (2.0 * c)).mean()

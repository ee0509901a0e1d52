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

The valid-pixel mask, TULIP(loss_valid_min=v) -- `valid_min=v` below.  A range image has pixels with no return, written as 0
(util/datasets.py:143-150; log1p keeps them 0).  With target of shape (B, C, ...), pixel (b, y, x) is valid iff
target[b, 0, y, x] > v: the rule reads channel 0, the range (a hole has no intensity either, while a valid return may have
intensity 0), and the comparison is false for a NaN.  All C elements of a valid pixel count, n_v = C * (valid pixels), and every
row of the table above is that loss over the valid elements with n_v in place of n (berHu's C: the max over the valid |d|);
pixel_loss likewise.  The gradient at an invalid element is +0.  n_v == 0 gives loss 0, pixel_loss 0, C 0 and all gradients 0
(a second departure from 0/0).  Whatever pred or any channel of target holds at an invalid pixel -- a NaN, an infinity -- changes
nothing; a non-finite value at a valid element propagates as above.  n_v and C are per call.  valid_min=None (the default): every
element counts, and each function returns what it returns without the keyword, bit for bit.
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


def check_valid_min(v):
    """The threshold of TULIP(loss_valid_min=...): None (no mask) or a finite float, returned as a Python float (ValueError for a
    bool, a NaN, an infinity or any other type -- an int among them: the value is in the target's units, write 0.0)."""
    if v is None:
        return None
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (float, np.floating)) or not np.isfinite(v):
        raise ValueError(f"loss_valid_min must be None or a finite float, got {v!r}")
    return float(v)


def valid_mask(target, valid_min) -> np.ndarray:
    """The valid elements of target (B, C, ...) as a bool array of its shape: target[b, 0, ...] > valid_min, broadcast over the
    channels (false for a NaN); all true for valid_min=None."""
    target = np.asarray(target)
    valid_min = check_valid_min(valid_min)
    if valid_min is None:
        return np.ones(target.shape, dtype=bool)
    if target.ndim < 2:
        raise ValueError(f"valid_mask needs a target of shape (B, C, ...), got {target.shape}")
    with np.errstate(all="ignore"):
        return np.broadcast_to(target[:, :1] > valid_min, target.shape).copy()


def _valid(pred, target, valid_min):
    """(pred, target) compressed to the valid elements, and the mask"""
    m = valid_mask(target, valid_min)
    return np.asarray(pred)[m], np.asarray(target)[m], m


def _diff(pred, target):
    pred, target = np.asarray(pred, dtype=np.float64), np.asarray(target, dtype=np.float64)
    with np.errstate(all="ignore"):
        return pred - target


def berhu_c(pred, target, valid_min=None) -> np.float64:
    """C = 0.2 * max |pred - target| in float64 (NaN when any difference is NaN); over the valid elements with valid_min (0 when
    there is none)."""
    if valid_min is not None:
        p, t, _ = _valid(pred, target, valid_min)
        return np.float64(0.0) if p.size == 0 else berhu_c(p, t)
    with np.errstate(all="ignore"):
        return np.float64(BERHU_FRACTION) * np.max(np.abs(_diff(pred, target)))


def berhu_c32(pred, target, valid_min=None) -> np.float32:
    """The device's C: float32(0.2) * float32(max |d|), d formed in float32 -- one float32 product."""
    if valid_min is not None:
        p, t, _ = _valid(pred, target, valid_min)
        return np.float32(0.0) if p.size == 0 else berhu_c32(p, t)
    with np.errstate(all="ignore"):
        d = np.asarray(pred, dtype=np.float32) - np.asarray(target, dtype=np.float32)
        return np.float32(BERHU_FRACTION) * np.float32(np.max(np.abs(d)))


def berhu_values(pred, target, c=None, valid_min=None) -> np.ndarray:
    """The elementwise berHu values (what inverse_huber_loss returns) for the threshold c (default: berhu_c); with valid_min the
    values of the valid elements (c's default: the masked berhu_c) and 0 at the others."""
    if valid_min is not None:
        p, t, m = _valid(pred, target, valid_min)
        out = np.zeros(m.shape, dtype=np.float64)
        if p.size:
            out[m] = berhu_values(p, t, c)
        return out
    d = _diff(pred, target)
    c = berhu_c(pred, target) if c is None else np.float64(c)
    if c == 0.0:
        return np.zeros_like(d)
    a = np.abs(d)
    with np.errstate(all="ignore"):
        return np.where(a < c, a, (a * a + c * c) / (2.0 * c))


def loss_value(kind: str, pred, target, valid_min=None) -> np.float64:
    """The scalar training loss of `kind` in float64; over the valid elements with valid_min (0 when there is none)."""
    kind = check_loss(kind)
    if valid_min is not None:
        p, t, _ = _valid(pred, target, valid_min)
        return np.float64(0.0) if p.size == 0 else loss_value(kind, p, t)
    d = _diff(pred, target)
    with np.errstate(all="ignore"):
        if kind == "l1":
            return np.mean(np.abs(d))
        if kind == "l2":
            return np.mean(d * d)
        return np.mean(berhu_values(pred, target))


def loss_grad(kind: str, pred, target, gscale: float = 1.0, valid_min=None) -> np.ndarray:
    """gscale * d(loss_value) / d(pred) in float64, the shape of pred; +0 at the invalid elements with valid_min."""
    kind = check_loss(kind)
    if valid_min is not None:
        p, t, m = _valid(pred, target, valid_min)
        out = np.zeros(m.shape, dtype=np.float64)
        if p.size:
            out[m] = loss_grad(kind, p, t, gscale)
        return out
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


def pixel_loss(pred, target, log_transform: bool, valid_min=None) -> np.float64:
    """The logged L1 metric, the same for every kind (tulip.py:695-698); over the valid elements with valid_min (0 when there is
    none)."""
    if valid_min is not None:
        p, t, _ = _valid(pred, target, valid_min)
        return np.float64(0.0) if p.size == 0 else pixel_loss(p, t, log_transform)
    pred, target = np.asarray(pred, dtype=np.float64), np.asarray(target, dtype=np.float64)
    with np.errstate(all="ignore"):
        if log_transform:
            return np.mean(np.abs(np.expm1(pred) - np.expm1(target)))
        return np.mean(np.abs(pred - target))


def torch_loss(kind: str, pred, target, valid_min=None):
    """The same definition on torch tensors, differentiable in pred (C detached, as the reference's .item() leaves it): what a
    test or a CPU experiment back-propagates through an autograd model.  With valid_min: over the valid elements (indexing, not
    a product with the mask: a NaN at an invalid pixel reaches neither the value nor the gradient)."""
    import torch
    kind = check_loss(kind)
    d = pred - target
    if check_valid_min(valid_min) is not None:
        d = d[(target[:, :1] > valid_min).expand_as(target)]
        if d.numel() == 0:
            return d.sum()                               # no valid pixel: 0, with a zero gradient
    if kind == "l1":
        return d.abs().mean()
    if kind == "l2":
        return (d * d).mean()
    a = d.abs()
    c = (BERHU_FRACTION * a.detach().max()).item()
    if c == 0.0:
        return (a * 0.0).mean()
    return torch.where(a < c, a, (a * a + c * c) / (2.0 * c)).mean()

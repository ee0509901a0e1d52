"""Gradient clipping by global norm -- the host definition of what tulip_grad_clip (csrc/elementwise.hip) computes on the device.

The reference's loop clips between backward() and optimizer.step() (util/misc.py:294-303: `scaler.unscale_`, then
`torch.nn.utils.clip_grad_norm_(parameters, clip_grad)`).  `Trainer(clip_grad=...)` does not rewrite the gradients: the coefficient
goes into the gradient scale every AdamW launch reads from device memory (hyper[7] of the 8-float hyper block, 1/world as the host
uploads it), so the optimizer steps on g * fl32(base * coef):

    norm   = (float)(sqrt(sum g[i]^2) * (double)base)      the PRE-clip norm of the mean gradient: what clip_grad_norm_ returns
    c      = max_norm / (norm + 1e-6f)                     fp32, two separately rounded operations
    coef   = 1.0f if c > 1.0f else c                       a NaN norm gives a NaN coef (torch.clamp), an infinite norm gives 0
    scale  = fl32(base * coef)                             coef == 1.0f: base keeps its bits, the step is the unclipped step

The functions below are that table in numpy float32, operation for operation; the kernel's result has their bits.
"""
from __future__ import annotations

import math

import numpy as np

ONE = np.float32(1.0)
EPS = np.float32(1e-6)          # clip_grad_norm_'s constant


def check_clip_grad(max_norm) -> float:
    """The max_norm of Trainer(clip_grad=...): a float >= 0 (ValueError for a negative value or NaN)."""
    x = float(max_norm)
    if math.isnan(x) or x < 0.0:
        raise ValueError(f"clip_grad must be None or a float >= 0, got {max_norm!r}")
    return x


def clip_coef_host(norm32, max_norm):
    """(coef, c): the clipping coefficient for the float32 pre-clip norm `norm32` and `max_norm` (rounded to float32, as the
    device float is), and the quotient it was clamped from."""
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.float32(norm32) + EPS)
    coef = ONE if c > ONE else c
    return np.float32(coef), np.float32(c)


def clipped_grad_scale_host(base32, coef32):
    """fl32(base * coef): the gradient scale the AdamW launches behind the clip read."""
    with np.errstate(all="ignore"):
        return np.float32(np.float32(base32) * np.float32(coef32))

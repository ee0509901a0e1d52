"""Non-finite step guard -- the host definition of what tulip_step_guard (csrc/elementwise.hip) decides on the device.

The reference's loop ends in `GradScaler.step(optimizer)` (util/misc.py:288-308), which does not call `optimizer.step()` when the
unscaled gradients hold an Inf or a NaN.  `Trainer(skip_nonfinite=True)` takes the same decision from the gradient norm the step
has already computed (a single non-finite gradient makes the norm non-finite), on the device, inside the captured graphs:

    skip = norm is NaN or +-Inf                                  (the float32 norm of tulip_grad_norm / tulip_grad_clip)
    skip:      skipped_total += 1;  skipped_consecutive += 1;  applied and the bias corrections stay
    no skip:   applied += 1;  skipped_consecutive = 0;  bias_corr_k = float32(1 - beta_k ** applied),  k = 1, 2

A skipped step does not advance the optimizer's step count (torch: `optimizer.step()` is not called).  The power is formed by
binary exponentiation in float64 in a fixed order, one rounding per multiplication and no transcendental function, so that the
device reproduces it bit for bit; the functions below are that definition in numpy, operation for operation.
"""
from __future__ import annotations

import numpy as np

_M64 = (1 << 64) - 1


def check_skip_nonfinite(value) -> bool:
    """The skip_nonfinite of Trainer(...): a bool (ValueError for anything else, 0 and 1 included)."""
    if not isinstance(value, (bool, np.bool_)):
        raise ValueError(f"skip_nonfinite must be a bool, got {value!r}")
    return bool(value)


def found_nonfinite_host(norm32) -> bool:
    """True when the float32 norm is NaN or +-Inf: every exponent bit set."""
    bits = int(np.float32(norm32).view(np.uint32))
    return (bits & 0x7F800000) == 0x7F800000


def bias_corr_host(beta, t) -> np.float32:
    """float32(1.0 - beta ** t), the power by binary exponentiation in float64 (np.float64 products: one rounding each, nothing
    contracted):  r = 1; x = beta; while t: (if t & 1: r = r * x); t >>= 1; (if t: x = x * x)."""
    t = int(t)
    if t < 0:
        raise ValueError("bias_corr_host: t must be >= 0")
    r, x = np.float64(1.0), np.float64(beta)
    with np.errstate(under="ignore"):
        while t:
            if t & 1:
                r = r * x
            t >>= 1
            if t:
                x = x * x
    return np.float32(np.float64(1.0) - r)


def guard_step_host(state, norm32, betas):
    """One decision: state = (applied, skipped_total, skipped_consecutive) BEFORE the step (64-bit counters), the float32 norm and
    (beta1, beta2) -> (state', skip, bc1, bc2).  On a skipped step bc1 and bc2 are None: the device leaves its two words alone."""
    applied, total, consecutive = (int(s) & _M64 for s in state)
    if found_nonfinite_host(norm32):
        return (applied, (total + 1) & _M64, (consecutive + 1) & _M64), True, None, None
    applied = (applied + 1) & _M64
    return (applied, total, 0), False, bias_corr_host(betas[0], applied), bias_corr_host(betas[1], applied)

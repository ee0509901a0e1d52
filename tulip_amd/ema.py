"""Exponential moving average (EMA) of the weights: the object the reference's training loop calls as `ema.update()` after every
optimizer call (engine_upsampling.py:51, 94-95 -- no arguments: torch_ema's `ExponentialMovingAverage` interface), kept as a
second flat fp32 buffer with the layout of the parameters and advanced by one launch pair (tulip_ema_update, csrc/elementwise.hip).

The definition -- what the kernel reproduces bit for bit and what `ema_update_host` is -- of one update of the shadow `s` of the
parameters `p`:

    1. num_updates += 1                                           (64-bit counter, starts at 0)
    2. d = min(decay, (1 + num_updates) / (10 + num_updates))     (float64; without warm-up, use_num_updates=False: d = decay)
    3. omd = float32(1.0 - d)                                      (float64 subtraction, rounded once)
    4. per element, float32, three separately rounded operations, no fused multiply-add:  t = s - p;  t = omd * t;  s = s - t

CAVEAT: torch_ema is neither installed beside this package nor part of the reference tree; the four steps restate its `update()`
from memory and are not pinned by any test against torch_ema itself.  They are the contract here.
"""
from __future__ import annotations

import contextlib
import math
import numbers

import numpy as np

_M64 = (1 << 64) - 1


def check_decay(decay) -> float:
    """A real number in [0, 1] as a Python float; anything else (bool, NaN, a string, out of range) raises ValueError."""
    if isinstance(decay, bool) or not isinstance(decay, numbers.Real):
        raise ValueError(f"EMA decay must be a float in [0, 1], got {decay!r}")
    d = float(decay)
    if math.isnan(d) or d < 0.0 or d > 1.0:
        raise ValueError(f"EMA decay must be in [0, 1], got {decay!r}")
    return d


def one_minus_decay(decay: float, num_updates) -> np.float32:
    """Steps 2 and 3 for the counter value AFTER its increment (None: no warm-up)."""
    d = float(decay)
    if num_updates is not None:
        n = int(num_updates)
        d = min(d, (1 + n) / (10 + n))
    return np.float32(1.0 - d)


def ema_update_host(shadow, params, decay, num_updates):
    """One update on the host: float32 numpy arrays `shadow`, `params` and the counter BEFORE the update (an int; None: no
    warm-up and no counter, d = decay) -> (new_shadow, new_num_updates).  The inputs are left unchanged."""
    decay = check_decay(decay)
    s, p = np.asarray(shadow), np.asarray(params)
    if s.dtype != np.float32 or p.dtype != np.float32 or s.shape != p.shape:
        raise TypeError("ema_update_host: shadow and params must be float32 arrays of one shape")
    n = None if num_updates is None else (int(num_updates) + 1) & _M64
    omd = one_minus_decay(decay, n)
    t = s - p
    t = omd * t
    s = s - t
    return s, n


class ParamEMA:
    """EMA of a TULIP model's parameters on the HIP path.  Bound to the model's FlatParams: `shadow` is a float32 buffer with
    the layout of the flat master (`W.total` elements; the padding between tensors stays exactly 0), the counter and the
    coefficient slot are device words, `update()` is one tulip_ema_update launch pair on the current stream (capturable: a
    replayed graph advances the counter and the warm-up schedule on the device).  The method names are torch_ema's.

    decay: float in [0, 1] (ValueError otherwise).  use_num_updates=False: no warm-up, no counter (`num_updates` is None).
    If the engine re-flattens the parameters after construction (`model.to(...)` does) or the master is partial
    (Trainer(exchange="sharded") before gather_state()), every method that touches the parameters raises RuntimeError."""

    def __init__(self, model, decay, use_num_updates: bool = True, device=None):
        import torch
        self.decay = check_decay(decay)
        self.model = model
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        eng = model.engine()
        eng.bind(self.device)
        self._W = eng.params
        W = self._params()
        self.shadow = W.flat.clone()
        self.counter = torch.zeros(1, dtype=torch.int64, device=self.device) if use_num_updates else None
        self._omd = torch.zeros(1, dtype=torch.float32, device=self.device)
        # the non-finite guard's device flag (set by the Trainer(skip_nonfinite=True) that owns this average; None: no guard): an
        # update behind a skipped optimizer step changes neither the counter nor the shadow (tulip_ema_update_g)
        self.skip_flag = None
        self._stash = None         # the parameters put aside by store()
        self._stored = False
        self._inside = False        # average_parameters() is not re-entrant

    def _params(self):
        W = self.model.engine().params
        if W is not self._W:
            raise RuntimeError("tulip_amd.ParamEMA: the engine re-flattened the model's parameters since this average was built "
                               "(model.to(...) / .cuda() / a replaced parameter): build a new ParamEMA and load this one's state_dict()")
        if W.master_partial:
            raise RuntimeError("tulip_amd.ParamEMA: the fp32 master weights are partial (Trainer(exchange='sharded')); call "
                               "Trainer.gather_state() on every rank first")
        return W

    @property
    def num_updates(self):
        """The counter read back (one host sync); None without warm-up."""
        return None if self.counter is None else int(self.counter.item())

    # ------------------------------------------------------------------ the update
    def update(self) -> None:
        from . import ops
        W = self._params()
        ops.ema_update(W.flat, self.shadow, W.total, self.decay, self.counter, self._omd, skip=self.skip_flag)

    # ------------------------------------------------------------------ evaluating with the averaged weights
    def store(self) -> None:
        """Put the current parameters aside (restore() brings them back)."""
        W = self._params()
        if self._stash is None:
            self._stash = W.flat.clone()
        else:
            self._stash.copy_(W.flat)
        self._stored = True

    def copy_to(self) -> None:
        """Write the average into the model's parameters (the views of the flat buffer: module forward, GraphedForward, evaluate,
        MCdrop and state_dict() all see it); the bf16 operands are re-derived before the next forward."""
        W = self._params()
        W.flat.copy_(self.shadow)
        W.shadow_dirty = True

    def restore(self) -> None:
        W = self._params()
        if not self._stored:
            raise RuntimeError("tulip_amd.ParamEMA.restore(): nothing stored (call store() first)")
        W.flat.copy_(self._stash)
        W.shadow_dirty = True
        self._stored = False

    @contextlib.contextmanager
    def average_parameters(self):
        """with ema.average_parameters(): ...  -- the model holds the averaged weights inside and its own again afterwards."""
        if self._inside:
            raise RuntimeError("tulip_amd.ParamEMA.average_parameters() is not re-entrant")
        self.store()
        self._inside = True
        try:
            self.copy_to()
            yield self
        finally:
            self._inside = False
            self.restore()

    # ------------------------------------------------------------------ checkpoint (keyed by name, like Trainer.state_dict()'s moments)
    def state_dict(self) -> dict:
        W = self._W
        cut = lambda n: self.shadow[W.offset[n]:W.offset[n] + W.numel[n]].view(W.shape[n]).clone()
        return {"decay": self.decay, "num_updates": self.num_updates, "shadow_params": {n: cut(n) for n in W.names}}

    def load_state_dict(self, sd: dict) -> None:
        W = self._W
        missing = [n for n in W.names if n not in sd["shadow_params"]]
        if missing:
            raise KeyError(f"EMA state lacks {len(missing)} parameters, e.g. {missing[:3]}")
        if (sd["num_updates"] is None) != (self.counter is None):
            raise ValueError("EMA state was saved with use_num_updates="
                             f"{sd['num_updates'] is not None}, this ParamEMA was built with {self.counter is not None}")
        self.decay = check_decay(sd["decay"])
        for n in W.names:
            self.shadow[W.offset[n]:W.offset[n] + W.numel[n]].copy_(sd["shadow_params"][n].reshape(-1).to(self.shadow.dtype))
        if self.counter is not None:
            self.counter.fill_(int(sd["num_updates"]))

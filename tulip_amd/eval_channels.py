"""Host (numpy) definition of the multi-channel evaluation -- what tulip_eval_postprocess_c and tulip_mc_aggregate_c compute
(include/tulip_hip.h; csrc/evalpost.hip).  Used by the tests; nothing on the hot path calls it.  The reference evaluates one channel
only (its evaluate() reshapes an (H, W, 2) array into H*W and fails), so the definition is this project's; it continues two rules:
channel 0 is exactly the single-channel chain, and "a hole has no intensity either" (prep_channels.py, the masked loss).

pred, hi are (C, H, W) and lo is (C, h, w), float32 in the model's value space; f = H // h; rows are restored iff w == W.

    channel 0   p0, t0, l0 = expm1 of all three if log_transform;  p0 = (gmin <= p0 <= gmax) ? p0 : 0;  |p0 - t0| -> mae[0];
                rows 0::f: |p0 - l0| -> mae_low[0], then p0 = l0;  keep_close > 0: p0, t0 above it become 0:
                tulip_eval_postprocess and nothing else
    hole        pixel (i, j) is a prediction hole iff p0 == 0.0 after the gate, before the rows are restored and before keep_close
                (true for -0.0; a NaN fails the gate, so it is a hole)
    valid       pixel (i, j) is a valid target pixel iff t0 > 0 after the expm1, before keep_close (false for a NaN): the rule of
                TULIP(loss_valid_min=0.0)
    channel c   pc = expm1(pred_c) if channel_log[c-1] else pred_c;  pc = hole ? +0.0 : pc  (a select: a NaN or an infinity in a
                hole yields +0.0);  tc = the same inverse of hi_c and nothing else (RangePrep has zeroed the target's holes);
                |pc - tc| -> mae[c];  rows 0::f when restored: lc = the inverse of lo_c, |pc - lc| -> mae_low[c], then pc = lc;
                keep_close > 0: where the final p0 > keep_close all C channels of the prediction's pixel become 0, where
                t0 > keep_close all C channels of the target's
    mae_valid   for every c, 0 included: the sum of |pc - tc| over the valid target pixels / n_valid, before the restore;
                n_valid == 0 gives 0

Sums are float64 sums of the float32 |differences|; a result is float32(sum * inv) with inv = 1/(H*W), 1/(h*W) (0 when no row is
restored) and 1/n_valid.

MC-dropout aggregate of preds (T, C, n), T >= 2: per channel the float64 mean rounded to float32; the drop decision is channel 0's,
float32(sd0) > thr * float32(mean0) with the unbiased std (the single-channel expression); a dropped pixel is 0 in all C channels.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np

F32 = np.float32


class ChannelEval(NamedTuple):
    pred_img: np.ndarray      # (C, H, W) float32
    hi_img: np.ndarray        # (C, H, W) float32
    mae: np.ndarray           # (C,) float32
    mae_low: np.ndarray       # (C,) float32
    mae_valid: np.ndarray     # (C,) float32
    n_valid: int
    hole: np.ndarray          # (H, W) bool
    valid: np.ndarray         # (H, W) bool


def _flags(C: int, channel_log: Optional[Sequence[bool]]):
    lg = [False] * (C - 1) if channel_log is None else [bool(v) for v in channel_log]
    if len(lg) != C - 1:
        raise ValueError(f"{C} channels take {C - 1} log flags")
    return lg


def _mean(abs_diff: np.ndarray, inv: float) -> np.float32:
    return F32(abs_diff.astype(np.float64).sum() * inv)


def eval_channels(pred, hi, lo, log_transform: bool, channel_log: Optional[Sequence[bool]], gate: Tuple[float, float],
                  keep_close: float = 0.0) -> ChannelEval:
    pred, hi, lo = (np.asarray(a) for a in (pred, hi, lo))
    if any(a.dtype != np.float32 or a.ndim != 3 for a in (pred, hi, lo)) or pred.shape != hi.shape or lo.shape[0] != pred.shape[0]:
        raise ValueError("pred, hi must be (C, H, W) and lo (C, h, w) float32 arrays")
    C, H, W = pred.shape
    h, w = lo.shape[1:]
    if not 2 <= C <= 4 or h <= 0 or H % h:
        raise ValueError("C must be 2..4 and H a multiple of h")
    lg = [bool(log_transform)] + _flags(C, channel_log)
    f, restore = H // h, w == W
    gmin, gmax, kc = F32(gate[0]), F32(gate[1]), F32(keep_close)
    inv_all, inv_low = 1.0 / (float(H) * W), (1.0 / (float(h) * W) if restore else 0.0)
    zero = F32(0.0)
    with np.errstate(all="ignore"):
        inv_c = lambda a, c: np.expm1(a) if lg[c] else a.copy()
        p = [inv_c(pred[c], c) for c in range(C)]
        t = [inv_c(hi[c], c) for c in range(C)]
        p[0] = np.where((p[0] >= gmin) & (p[0] <= gmax), p[0], zero)
        hole, valid = p[0] == zero, t[0] > zero
        n_valid = int(valid.sum())
        inv_val = 1.0 / n_valid if n_valid else 0.0
        mae, mae_low, mae_valid = (np.zeros(C, dtype=np.float32) for _ in range(3))
        for c in range(C):
            if c:
                p[c] = np.where(hole, zero, p[c])
            d = np.abs(p[c] - t[c])
            mae[c], mae_valid[c] = _mean(d, inv_all), _mean(d[valid], inv_val)
            if restore:
                l = inv_c(lo[c], c)
                mae_low[c] = _mean(np.abs(p[c][0::f] - l), inv_low)
                p[c][0::f] = l
        if kc > 0:
            far_p, far_t = p[0] > kc, t[0] > kc
            for c in range(C):
                p[c][far_p] = zero
                t[c][far_t] = zero
    return ChannelEval(np.stack(p).astype(np.float32, copy=False), np.stack(t).astype(np.float32, copy=False), mae, mae_low,
                       mae_valid, n_valid, hole, valid)


def mc_aggregate_channels(preds, noise_threshold: float) -> np.ndarray:
    """preds (T, C, ...) float32, T >= 2 -> (C, ...) float32"""
    preds = np.asarray(preds)
    if preds.dtype != np.float32 or preds.ndim < 3 or preds.shape[0] < 2:
        raise ValueError("preds must be a (T >= 2, C, ...) float32 array")
    T = preds.shape[0]
    p64 = preds.astype(np.float64)
    s = p64[0].copy()
    for k in range(1, T):           # the kernel's order of additions
        s += p64[k]
    mean = s / T
    q = np.zeros_like(mean[0])
    for k in range(T):
        d = p64[k, 0] - mean[0]
        q += d * d
    out = mean.astype(np.float32)
    sd0 = np.sqrt(q / (T - 1)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        drop = sd0 > F32(noise_threshold) * out[0]
    out[:, drop] = F32(0.0)
    return out

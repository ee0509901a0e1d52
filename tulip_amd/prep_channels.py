"""Host (numpy) definition of the multi-channel input batches -- what tulip_range_prep_c computes (include/tulip_hip.h;
csrc/prep.hip), and with `augment.apply` on top what tulip_range_prep_aug_c computes.  Used by the tests; nothing on the hot path
calls it.

raw[b, i, j, c] is float32 with Cr >= C raw channels; s_c and log_c are the scale and the log flag of channel c >= 1.

    channel 0   v0 = raw0 * scale;  v0 = (gmin <= v0 <= gmax) ? v0 : 0 when the dataset has a gate;  log1p(v0) if log_transform:
                the single-channel chain and nothing else
    hole        pixel (b, i, j) is a hole iff v0 == 0.0 after scale and gate, before the log (true for -0.0, false for a NaN)
    channel c   u = raw_c * s_c (one float32 multiply);  u = hole ? +0.0 : u  (a select, not a multiply: a NaN, infinite or
                negative intensity in a hole yields +0.0);  u = log1p(u) if log_c

Geometry is shared: the high-res output is (B, C, H, W), the low-res one its rows row_phase::f and columns col_phase::fw, both
rolled by roll_shift along W.  Under RangePrep(augment=...) output channel c is `augment.apply` of plain channel c (apply indexes a
(B, C, H, W) array; a dropped low-res pixel is +0.0 in all C channels; the draws do not depend on C; the target is never dropped).
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np


def holes(raw0: np.ndarray, scale: float, gate: Optional[Tuple[float, float]]) -> Tuple[np.ndarray, np.ndarray]:
    """(v0 after scale and gate, before the log; the hole mask v0 == 0.0) of the channel-0 array raw0"""
    v0 = np.asarray(raw0, dtype=np.float32) * np.float32(scale)
    if gate is not None:
        with np.errstate(invalid="ignore"):
            v0 = np.where((v0 >= np.float32(gate[0])) & (v0 <= np.float32(gate[1])), v0, np.float32(0.0))
    return v0, v0 == np.float32(0.0)


def prep_channels(raw, scale: float, gate: Optional[Tuple[float, float]], log_transform: bool, in_chans: int,
                  channel_scale: Optional[Sequence[float]] = None, channel_log: Optional[Sequence[bool]] = None, f: int = 1,
                  fw: int = 1, row_phase: int = 0, col_phase: int = 0, roll_shift: int = 0):
    """raw (B, H, W, Cr >= in_chans) float32 -> (low_res (B, C, H//f, W//fw), high_res (B, C, H, W)), float32"""
    raw = np.asarray(raw)
    if raw.dtype != np.float32 or raw.ndim != 4 or raw.shape[3] < in_chans:
        raise ValueError(f"raw must be a (B, H, W, Cr >= {in_chans}) float32 array")
    C = int(in_chans)
    s = [1.0] * (C - 1) if channel_scale is None else list(channel_scale)
    lg = [False] * (C - 1) if channel_log is None else list(channel_log)
    if len(s) != C - 1 or len(lg) != C - 1:
        raise ValueError(f"{C} channels take {C - 1} scales and log flags")
    v0, hole = holes(raw[..., 0], scale, gate)
    with np.errstate(all="ignore"):
        planes = [np.log1p(v0) if log_transform else v0]
        for c in range(1, C):
            u = raw[..., c] * np.float32(s[c - 1])
            u = np.where(hole, np.float32(0.0), u)
            planes.append(np.log1p(u) if lg[c - 1] else u)
    hi = np.stack(planes, axis=1).astype(np.float32, copy=False)
    lo = hi[:, :, row_phase::f, col_phase::fw]
    if roll_shift:
        lo, hi = np.roll(lo, roll_shift, axis=-1), np.roll(hi, roll_shift, axis=-1)
    return np.ascontiguousarray(lo), np.ascontiguousarray(hi)

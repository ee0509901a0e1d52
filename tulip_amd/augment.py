"""Host (numpy) definition of the per-sample range-image augmentation -- bit for bit what tulip_range_prep_aug draws and
gathers (include/tulip_hip.h; csrc/prep.hip).  Used by the tests; nothing on the hot path calls it.

    DOMAIN       0x52414E4745415547
    K(seed, id)  mix64((seed mod 2^64) ^ DOMAIN ^ mix64(id mod 2^64))              (dropout.mix64)
    draw(K, n)   mix64((K + n) mod 2^64)
    shift  s     ((draw(K,0) >> 32) * W) >> 32           in [0, W)      (0 when roll is off)
    flip         draw(K,1) >> 63                          0 | 1          (0 when flip is off)
    row phase p  ((draw(K,2) >> 32) * f) >> 32            in [0, f)      (the fixed row phase when off)
    beam il dropped      iff (draw(K, 2^20 + il)          >> 40) < thr(beam_drop)
    point il,jl dropped  iff (draw(K, 2^32 + il*Wl + jl) >> 40) < thr(point_drop)
    thr(p)       rint(float32(p) * 2^24)                                 (dropout.threshold)

W, f: high-res width and row factor H // h; Wl = W // fw; (il, jl): coordinates in the augmented low-res image.  The scan is
mirrored, then rotated, and the pair is derived from it afterwards.  With hi0 the plain high-res output (no roll),
c = (j - s) mod W and src(j) = W-1-c under a flip, else c:

    hi[b,0,i,j]   = hi0[b,0,i,src_b(j)]
    lo[b,0,il,jl] = +0.0 if beam il or point (il,jl) is dropped, else hi0[b,0, p_b + f*il, src_b(cp + fw*jl)]

A sample's augmentation depends on (seed, sample id) alone: not on the batch it is drawn in, its position, the rank or the
world size.  The target is never dropped.
"""
from __future__ import annotations

import math
import numbers
from dataclasses import dataclass

import numpy as np

from .dropout import mix64, threshold

DOMAIN = 0x52414E4745415547
BEAM_BASE, POINT_BASE = 1 << 20, 1 << 32
_M64 = (1 << 64) - 1


def _u64(v) -> np.ndarray:
    """integers (Python ints of any size, or an integer array) mod 2^64"""
    a = np.asarray(v)
    if a.dtype == np.uint64:
        return a
    if a.dtype == object or a.dtype.kind not in "iu":
        return np.array([int(x) & _M64 for x in np.asarray(v, dtype=object).reshape(-1)], dtype=np.uint64).reshape(a.shape)
    return a.astype(np.int64).view(np.uint64)


def key(seed: int, ids) -> np.ndarray:
    """K(seed, id) for every id: uint64, the shape of ids"""
    return mix64(np.uint64((int(seed) & _M64) ^ DOMAIN) ^ mix64(_u64(ids)))


def draw(K, n) -> np.ndarray:
    with np.errstate(over="ignore"):
        return mix64(np.asarray(K, dtype=np.uint64) + _u64(n))


def params(seed: int, ids, W: int, f: int, roll: bool = True, flip: bool = True, row_phase=True) -> np.ndarray:
    """(B,3) int64 rows (s, flip, p).  row_phase: True draws p; an int (or False: 0) is the fixed row phase of every sample."""
    K = key(seed, np.asarray(_u64(ids)).reshape(-1))
    out = np.zeros((K.shape[0], 3), dtype=np.int64)
    if roll:
        out[:, 0] = ((draw(K, 0) >> np.uint64(32)) * np.uint64(W)) >> np.uint64(32)
    if flip:
        out[:, 1] = draw(K, 1) >> np.uint64(63)
    if row_phase is True:
        out[:, 2] = ((draw(K, 2) >> np.uint64(32)) * np.uint64(f)) >> np.uint64(32)
    else:
        out[:, 2] = int(row_phase)
    return out


def beam_mask(seed: int, ids, Hl: int, beam_drop: float) -> np.ndarray:
    """(B,Hl) bool: True where low-res row il of the sample is dropped"""
    K = key(seed, np.asarray(_u64(ids)).reshape(-1))[:, None]
    n = np.uint64(BEAM_BASE) + np.arange(Hl, dtype=np.uint64)[None, :]
    return (draw(K, n) >> np.uint64(40)) < np.uint64(threshold(beam_drop))


def point_mask(seed: int, ids, Hl: int, Wl: int, point_drop: float) -> np.ndarray:
    """(B,Hl,Wl) bool: True where low-res pixel (il, jl) of the sample is dropped"""
    K = key(seed, np.asarray(_u64(ids)).reshape(-1))[:, None, None]
    n = np.uint64(POINT_BASE) + np.arange(Hl * Wl, dtype=np.uint64).reshape(1, Hl, Wl)
    return (draw(K, n) >> np.uint64(40)) < np.uint64(threshold(point_drop))


def source_columns(par: np.ndarray, W: int) -> np.ndarray:
    """(B,W) int64: src_b(j) for the (s, flip, p) rows of `params`"""
    c = (np.arange(W, dtype=np.int64)[None, :] - par[:, 0:1]) % W
    return np.where(par[:, 1:2] != 0, W - 1 - c, c)


def apply(hi0, seed: int, ids, f: int, fw: int = 1, col_phase: int = 0, roll: bool = True, flip: bool = True, row_phase=True,
          beam_drop: float = 0.0, point_drop: float = 0.0):
    """hi0: the plain (B,1,H,W) high-res output (no roll).  Returns (lo (B,1,H//f,W//fw), hi (B,1,H,W)), numpy, by indexing."""
    hi0 = np.asarray(hi0)
    B, C, H, W = hi0.shape
    Hl, Wl = H // f, W // fw
    par = params(seed, ids, W, f, roll, flip, row_phase)
    if par.shape[0] != B:
        raise ValueError(f"{par.shape[0]} sample ids for a batch of {B}")
    src = source_columns(par, W)
    hi = np.take_along_axis(hi0, np.broadcast_to(src[:, None, None, :], hi0.shape), axis=3)
    rows = par[:, 2:3] + f * np.arange(Hl, dtype=np.int64)[None, :]                     # (B,Hl)
    cols = col_phase + fw * np.arange(Wl, dtype=np.int64)                               # (Wl,)
    b = np.arange(B)[:, None, None]
    lo = hi[b, :, rows[:, :, None], cols[None, None, :]]                                # (B,Hl,Wl,C)
    lo = np.ascontiguousarray(np.moveaxis(lo, 3, 1))
    dropped = beam_mask(seed, ids, Hl, beam_drop)[:, :, None] | point_mask(seed, ids, Hl, Wl, point_drop)
    lo[np.broadcast_to(dropped[:, None], lo.shape)] = 0
    return lo, hi


def _probability(name: str, v) -> float:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Real):
        raise ValueError(f"{name} must be a real number in [0, 1), got {v!r}")
    v = float(v)
    if math.isnan(v) or not 0.0 <= v < 1.0:
        raise ValueError(f"{name} must be a real number in [0, 1), got {v!r}")
    return v


@dataclass(frozen=True)
class RangeAugment:
    """What RangePrep(augment=...) draws per sample: a rotation about the sensor axis, a mirror, the start row of the beam
    subsampling, and the probabilities of a low-res beam / a low-res point losing its return."""
    seed: int = 0
    roll: bool = True
    flip: bool = True
    row_phase: bool = True
    beam_drop: float = 0.0
    point_drop: float = 0.0

    def __post_init__(self):
        if isinstance(self.seed, (bool, np.bool_)) or not isinstance(self.seed, numbers.Integral):
            raise ValueError(f"seed must be an int, got {self.seed!r}")
        object.__setattr__(self, "seed", int(self.seed))
        for n in ("roll", "flip", "row_phase"):
            if not isinstance(getattr(self, n), (bool, np.bool_)):
                raise ValueError(f"{n} must be a bool, got {getattr(self, n)!r}")
            object.__setattr__(self, n, bool(getattr(self, n)))
        object.__setattr__(self, "beam_drop", _probability("beam_drop", self.beam_drop))
        object.__setattr__(self, "point_drop", _probability("point_drop", self.point_drop))

    @property
    def flags(self) -> int:
        """the TULIP_AUG_* bits"""
        return (1 if self.roll else 0) | (2 if self.flip else 0) | (4 if self.row_phase else 0)

    @property
    def thresholds(self):
        """(beam, point) thresholds of the kernel's 24-bit draws"""
        return threshold(self.beam_drop), threshold(self.point_drop)

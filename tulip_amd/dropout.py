"""Host (numpy) definition of the element-dropout keep mask -- bit for bit what the kernels draw (include/tulip_hip.h,
"Element dropout").  Used by the tests and by the fixture generator; nothing on the hot path calls it.

    mix64(z)    splitmix64 finaliser
    key         mix64(seed ^ mix64(counter * 2^20 + site))
    u(index)    mix64(key + index) >> 40                       (top 24 bits)
    kept        u >= rint(p * 2^24)                             (p as fp32)
    scale       float32(1) / (float32(1) - float32(p))

Sites: 0 pos_drop; block i of TulipEngine.blocks: 1 + 4 i + {0 attn_drop, 1 proj_drop, 2 mlp.drop1, 3 mlp.drop2}.
"""
from __future__ import annotations

import numpy as np

ATTN, PROJ, DROP1, DROP2 = range(4)
_M64 = (1 << 64) - 1


def site(block: int, kind: int) -> int:
    return 1 + 4 * block + kind


def mix64(z: np.ndarray) -> np.ndarray:
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def key(seed: int, counter: int, site_id: int) -> np.uint64:
    inner = np.uint64(((int(counter) << 20) + int(site_id)) & _M64)
    return mix64(np.uint64(int(seed) & _M64) ^ mix64(inner))


def threshold(p: float) -> int:
    return int(np.rint(np.float32(p) * np.float32(1 << 24)))


def scale(p: float) -> np.float32:
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep(seed: int, counter: int, site_id: int, p: float, index) -> np.ndarray:
    """bool keep mask at the given flat element indices (any integer array)"""
    idx = np.asarray(index, dtype=np.uint64)
    with np.errstate(over="ignore"):
        u = mix64(key(seed, counter, site_id) + idx) >> np.uint64(40)
    return u >= np.uint64(threshold(p))


def multiplier(seed: int, counter: int, site_id: int, p: float, index) -> np.ndarray:
    """fp32 per-element multiplier: scale where kept, 0 elsewhere (what tulip_dropout_mask reads out)"""
    return np.where(keep(seed, counter, site_id, p, index), scale(p), np.float32(0.0)).astype(np.float32)


def attn_index(B: int, H: int, W: int, nh: int, win) -> np.ndarray:
    """[B * nW, nh, L, L] (L = wh * ww) -> flat index of the reference's attention-probability tensor (its own
    flattening): ((window * nh + head) * L + q) * L + k"""
    wh, ww = win
    n = B * (H // wh) * (W // ww) * nh * (wh * ww) ** 2
    return np.arange(n, dtype=np.uint64).reshape(B * (H // wh) * (W // ww), nh, wh * ww, wh * ww)


def window_rows(B: int, H: int, W: int, win, shift) -> np.ndarray:
    """[B * nW, wh * ww] natural token row of every in-window slot (roll by -shift, window partition), the layout of the
    reference's proj_drop input"""
    wh, ww = win
    sh, sw = shift
    nWy, nWx = H // wh, W // ww
    b, wy, wx, i, j = np.meshgrid(np.arange(B), np.arange(nWy), np.arange(nWx), np.arange(wh), np.arange(ww), indexing="ij")
    h = (wy * wh + i + sh) % H
    w = (wx * ww + j + sw) % W
    return ((b * H + h) * W + w).reshape(B * nWy * nWx, wh * ww)

"""Seeded inputs of the multi-channel evaluation tests (tests/test_eval_channels_cpu.py, tests/test_eval_channels_gpu.py) and the
comparisons they share.  tulip_amd/eval_channels.py is the definition under test; nothing here restates it."""
import numpy as np

from oracle.eval_oracle import synthetic_eval_case

F32 = np.float32
GATE = (2 / 80, 1.0)        # CARLA / KITTI `evaluate`
KEEP_CLOSE = 0.25
MARGIN = 1e-6               # no channel-0 value of a case lies this close to a threshold of a decision
NUDGE = 1e-4


def _inv(a, log):
    with np.errstate(all="ignore"):
        return np.expm1(a) if log else a


def _clear_of(v, thresholds):
    """move every value within 2*MARGIN of a threshold away from it (deterministic; asserted again by margins_hold)"""
    for th in thresholds:
        v = np.where(np.abs(v - F32(th)) <= 2 * MARGIN, v + F32(NUDGE), v)
    return v.astype(np.float32)


def post_case(C, H, W, h, w, log_transform, channel_log, seed, inject, gate=GATE):
    """(pred (C,H,W), hi (C,H,W), lo (C,h,w)) float32 in the model's value space.  Metric-space values lie in [0, 1] (channel 0 of the
    prediction also holds negatives, values below gmin and above gmax); a logged channel stores log1p of them.  15% of the target's
    pixels are holes (0 in every channel, as RangePrep leaves them).  inject: NaN, +-Inf, -0.0 and negative values at fixed pixels.  gate: the (gmin, gmax) the case keeps its margins from."""
    rng = np.random.default_rng(seed)
    f, fw = H // h, W // w
    logs = [bool(log_transform)] + [bool(v) for v in channel_log]
    t = rng.uniform(0.03, 0.98, size=(C, H, W)).astype(np.float32)
    t[:, rng.random((H, W)) < 0.15] = 0
    p = t + F32(0.02) * rng.standard_normal((C, H, W)).astype(np.float32)
    u = rng.random((H, W))
    p[0] = np.where(u < 0.04, -p[0], p[0])
    p[0] = np.where((u >= 0.04) & (u < 0.08), p[0] + F32(1.0), p[0])
    p[0] = np.where((u >= 0.08) & (u < 0.16), p[0] * F32(0.02), p[0])          # below gmin: prediction holes
    p[1:] = np.clip(p[1:], 0.0, 1.0)
    p[1:] = np.where(rng.random((C - 1, H, W)) < 0.5, p[1:], rng.uniform(0, 1, size=(C - 1, H, W)))   # intensity inside holes too
    p, t = p.astype(np.float32), t.astype(np.float32)
    th = (0.0, gate[0], gate[1], KEEP_CLOSE)
    p[0], t[0] = _clear_of(p[0], th), _clear_of(t[0], (KEEP_CLOSE,))
    with np.errstate(all="ignore"):
        pred = np.stack([np.log1p(np.maximum(p[c], F32(-0.5))) if logs[c] else p[c] for c in range(C)]).astype(np.float32)
        hi = np.stack([np.log1p(t[c]) if logs[c] else t[c] for c in range(C)]).astype(np.float32)
    if inject:
        px = [(r % H, (7 * r + 3) % W) for r in range(1, 12)]
        pred[0][px[0]] = np.nan
        pred[0][px[1]] = np.inf
        pred[0][px[2]] = -np.inf
        pred[0][px[3]] = -0.0
        for c in range(1, C):                   # intensity of every kind inside prediction holes ...
            pred[c][px[0]], pred[c][px[1]], pred[c][px[2]], pred[c][px[3]] = np.nan, np.inf, -np.inf, -1.0
            pred[c][px[4]] = -0.0               # ... and a -0.0 wherever it falls
        hi[0][px[5]] = np.nan
        hi[0][px[6]] = -0.0
        hi[0][px[7]] = -np.inf
        hi[C - 1][px[8]] = -0.0
        pred[0][px[9]] = -0.0                   # a hole under a NaN intensity of the target's last channel
        hi[C - 1][px[9]] = np.nan
    return np.ascontiguousarray(pred), np.ascontiguousarray(hi), np.ascontiguousarray(hi[:, 0::f, 0::fw])


def margins_hold(pred, hi, lo, log_transform, keep_close, gate=GATE):
    """no channel-0 value (after the expm1) lies within MARGIN of a threshold that a decision compares it with: the prediction against
    0, gmin and gmax; with keep_close all three images against it.  Returns the number of pixels that do (the tests assert 0)."""
    p0, t0, l0 = (_inv(a[0].astype(np.float64), log_transform) for a in (pred, hi, lo))
    with np.errstate(invalid="ignore"):
        bad = 0
        for th in (0.0, gate[0], gate[1]):
            near = np.abs(p0 - th) <= MARGIN
            if th == 0.0:
                near &= p0 != 0.0               # an exact (signed) zero is a hole on both sides
            bad += int(near.sum())
        if keep_close > 0:
            bad += sum(int((np.abs(a - keep_close) <= MARGIN).sum()) for a in (p0, t0, l0))
    return bad


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def close(got, want, rel, absolute=0.0):
    """|got - want| <= absolute + rel*|want|; two NaNs and two equal infinities agree"""
    got, want = float(got), float(want)
    if np.isnan(want) or np.isnan(got):
        return bool(np.isnan(want) and np.isnan(got))
    if np.isinf(want) or np.isinf(got):
        return got == want
    return abs(got - want) <= absolute + rel * abs(want)


def planes_agree(dev, host, logged, tol=3e-7):
    """one (H,W) plane of the device against the host definition: bit-identical when no expm1 produced it, else the same zeros and
    NaNs and |difference| <= tol"""
    if not logged:
        return same_bits(dev, host)
    if not (np.array_equal(np.isnan(dev), np.isnan(host)) and np.array_equal(dev == 0, host == 0)):
        return False
    fin = np.isfinite(host)
    return bool(np.array_equal(dev[~fin & ~np.isnan(host)], host[~fin & ~np.isnan(host)]) and
                (np.abs(dev[fin] - host[fin]).max(initial=0.0) <= tol))


def mc_case(T, C, n, seed):
    """(preds (T,C,n) float32 in [2^-10, 2), threshold): float64 sums of T such values are exact.  Channel 0: a third of the pixels have
    identical passes, a third a relative spread of at most 0.5% (kept at threshold 0.03), a third alternate by 10-30% (dropped)."""
    rng = np.random.default_rng(seed)
    thr = 0.03
    base = rng.uniform(0.01, 1.5, size=n)
    kind = rng.integers(0, 3, size=n)
    sign = np.where(np.arange(T) % 2 == 0, 1.0, -1.0)[:, None]
    eps = np.where(kind == 0, 0.0, np.where(kind == 1, rng.uniform(-0.005, 0.005, size=(T, n)),
                                            sign * rng.uniform(0.1, 0.3, size=(T, n))))
    preds = np.empty((T, C, n), dtype=np.float32)
    preds[:, 0] = (base * (1.0 + eps)).astype(np.float32)
    preds[:, 1:] = rng.uniform(2.0 ** -10, 1.999, size=(T, C - 1, n)).astype(np.float32)
    assert preds.min() >= 2.0 ** -10 and preds.max() < 2.0
    return preds, thr


def mc_margin(preds, thr):
    """pixels whose channel-0 std lies within 1e-6 relative of thr * mean (float64); the tests assert 0"""
    p = preds[:, 0].astype(np.float64)
    sd, mean = p.std(axis=0, ddof=1), p.mean(axis=0)
    return int((np.abs(sd - thr * mean) <= 1e-6 * np.maximum(sd, thr * mean)).sum())


def stack_case(ds, C, H, W, h, w, seed, log_transform):
    """channel 0: the oracle's synthetic case; channels 1..C-1: seeded values in [0, 1], zero where the target's range is"""
    pred, hi, lo = synthetic_eval_case(ds, H, W, h, w, seed=seed, log_transform=log_transform)
    rng = np.random.default_rng(seed)
    tc = rng.uniform(0, 1, size=(C - 1, H, W)).astype(np.float32) * (hi[0, 0].numpy() != 0)
    pc = np.clip(tc + 0.05 * rng.standard_normal((C - 1, H, W)), 0, 1).astype(np.float32)
    P = np.concatenate([pred[0].numpy(), pc])
    T = np.concatenate([hi[0].numpy(), tc])
    return (pred, hi, lo), (P, T, np.ascontiguousarray(T[:, 0::H // h, 0::max(1, W // w)]))

"""CPU: the host definition of the weight EMA (tulip_amd/ema.py: ema_update_host) against an independent float64 restatement,
its warm-up schedule in closed form, and the argument checks that need no library."""
import numpy as np
import pytest

from tulip_amd import ema as E


def value_set(n=4096, seed=7):
    """(shadow, params): n float32 values each, magnitudes log-uniform over 1e-8 .. 1e4, both signs, with exact zeros (either
    side, both sides) and runs where p == s."""
    rng = np.random.default_rng(seed)
    mk = lambda: (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-8.0, 4.0, n)).astype(np.float32)
    s, p = mk(), mk()
    s[0:64] = 0.0                   # s == 0
    p[32:96] = 0.0                  # both zero on 32..63, p == 0 on 64..95
    p[128:256] = s[128:256]         # p == s
    s[256], p[256] = np.float32(1e-8), np.float32(-1e4)
    s[257], p[257] = np.float32(1e4), np.float32(1e-8)
    return s, p


def restated(s, p, decay, n):
    """One update restated in float64 with a rounding to float32 behind each of the three operations; n: the counter BEFORE the
    update, None without warm-up."""
    if n is None:
        d, n1 = np.float64(decay), None
    else:
        n1 = n + 1
        d = min(np.float64(decay), np.float64(1 + n1) / np.float64(10 + n1))
    omd = np.float32(np.float64(1.0) - d).astype(np.float64)
    s64, p64 = s.astype(np.float64), p.astype(np.float64)
    # (a float64 result rounded to float32 is the correctly rounded float32 result for + - *: 53 >= 2 * 24 + 2 bits)
    t = (s64 - p64).astype(np.float32).astype(np.float64)
    t = (omd * t).astype(np.float32).astype(np.float64)
    return (s64 - t).astype(np.float32), n1


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def test_host_definition_matches_the_float64_restatement_with_warmup():
    s, p = value_set()
    rng = np.random.default_rng(11)
    a, b, n, m = s.copy(), s.copy(), 0, 0
    took_warm, took_decay = [], []
    for k in range(12):
        pk = (p * np.float32(1.0 + 0.01 * k)).astype(np.float32) if k else p       # the parameters move between updates
        if k == 5:
            pk = rng.permutation(pk)
        a_in, a_keep, pk_keep = a, a.copy(), pk.copy()
        a, n = E.ema_update_host(a_in, pk, 0.5, n)
        b, m = restated(b, pk, 0.5, m)
        assert a.dtype == np.float32 and n == m == k + 1
        assert np.array_equal(bits(a), bits(b)), f"update {k + 1}"
        assert np.array_equal(bits(a_in), bits(a_keep)) and np.array_equal(bits(pk), bits(pk_keep))    # the inputs are not written
        warm = (1 + n) / (10 + n)
        (took_warm if warm < 0.5 else took_decay).append(n)
    # (1 + n) / (10 + n) crosses 0.5 at update 8: both branches of the min were taken
    assert took_warm == [1, 2, 3, 4, 5, 6, 7] and took_decay == [8, 9, 10, 11, 12]
    assert (1 + 7) / (10 + 7) < 0.5 <= (1 + 8) / (10 + 8)


def test_host_definition_without_warmup():
    s, p = value_set(seed=8)
    a, b = s.copy(), s.copy()
    for k in range(12):
        pk = (p * np.float32(1.0 - 0.02 * k)).astype(np.float32)
        a, n = E.ema_update_host(a, pk, 0.999, None)
        b, _ = restated(b, pk, 0.999, None)
        assert n is None
        assert np.array_equal(bits(a), bits(b)), f"update {k + 1}"
    assert E.one_minus_decay(0.999, None) == np.float32(1.0 - 0.999)


def test_closed_form_warmup_and_padding():
    """decay 0.9, warm-up on: d = 2/11, 3/12, 4/13 for the first three updates; zeros (the padding between tensors) stay +0.0."""
    s = np.array([1.0, -2.0, 0.0, 0.0, 3.5, 0.0, 0.0, 0.0], dtype=np.float32)
    p = np.array([0.0, 4.0, 0.0, 0.0, 3.5, 1.0, 0.0, 0.0], dtype=np.float32)
    pad = [2, 3, 6, 7]
    n = 0
    for want in (2.0 / 11.0, 3.0 / 12.0, 4.0 / 13.0):
        omd = np.float32(1.0 - want)
        assert want < 0.9 and E.one_minus_decay(0.9, n + 1) == omd
        expect = (s - (omd * (s - p)).astype(np.float32)).astype(np.float32)
        s, n = E.ema_update_host(s, p, 0.9, n)
        assert np.array_equal(bits(s), bits(expect))
        assert np.all(bits(s[pad]) == 0)                     # +0.0, not -0.0
    assert n == 3
    # element 0 in exact arithmetic: 1 -> 2/11 -> (2/11)(3/12) -> ...(4/13); float32 follows to a few ulps
    assert abs(float(s[0]) - (2 / 11) * (3 / 12) * (4 / 13)) < 1e-7
    assert s[4] == np.float32(3.5)                           # p == s: unchanged
    # far into the run the bound no longer binds
    assert E.one_minus_decay(0.9, 10 ** 6) == np.float32(1.0 - 0.9)
    # decay 1.0 never moves the shadow, decay 0.0 without warm-up copies the parameters
    keep, _ = E.ema_update_host(s, p, 1.0, None)
    assert np.array_equal(bits(keep), bits(s))
    copy, _ = E.ema_update_host(s, p, 0.0, None)
    assert np.array_equal(copy, p)


@pytest.mark.parametrize("bad", [-1e-9, 1.0000001, float("nan"), float("inf"), -1.0, 2, "0.9", None, True, [0.9]])
def test_decay_outside_the_unit_interval_raises(bad):
    z = np.zeros(4, dtype=np.float32)
    with pytest.raises(ValueError):
        E.check_decay(bad)
    with pytest.raises(ValueError):
        E.ema_update_host(z, z, bad, 0)


def test_decay_bounds_are_accepted_and_arrays_are_checked():
    assert E.check_decay(0.0) == 0.0 and E.check_decay(1.0) == 1.0 and E.check_decay(np.float64(0.25)) == 0.25
    z = np.zeros(4, dtype=np.float32)
    with pytest.raises(TypeError):
        E.ema_update_host(z.astype(np.float64), z, 0.5, 0)
    with pytest.raises(TypeError):
        E.ema_update_host(z, np.zeros(8, dtype=np.float32), 0.5, 0)


def test_trainer_refuses_bad_arguments_before_touching_the_gpu():
    """Trainer's own checks of ema_decay come first in its constructor: no model, no device needed."""
    from tulip_amd.trainer import Trainer
    with pytest.raises(ValueError):
        Trainer(None, 1, ema_decay=1.5)
    with pytest.raises(ValueError, match="sharded"):
        Trainer(None, 1, ema_decay=0.9, exchange="sharded")

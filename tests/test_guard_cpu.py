"""The non-finite step guard without a GPU: the host definition (tulip_amd/guard.py) -- the bias corrections by binary exponentiation
against float32(1 - beta ** t), the decision, the state machine --, the four new symbols in the header, both libraries and the
bindings, the refusals that come back before any launch, and the constructor's refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

from tulip_amd import _lib
from tulip_amd.guard import bias_corr_host, check_skip_nonfinite, found_nonfinite_host, guard_step_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"tulip_step_guard": 7, "tulip_adamw_g": 12, "tulip_adamw_blocks_g": 13, "tulip_ema_update_g": 8}


def bits(x) -> int:
    return int(np.float32(x).view(np.uint32))


# ---------------------------------------------------------------------------------------------------- 1. bias corrections
@pytest.mark.parametrize("beta", [0.9, 0.95, 0.99, 0.999])
def test_bias_corrections_are_the_hosts_power(beta):
    """bias_corr_host(b, t) has the bits of float32(1.0 - b ** t) -- what Trainer._set_hyper uploads without the guard -- for every
    t from 1 until both are exactly 1.0f, which every one of the four betas reaches before t = 20000."""
    one, t, differ = bits(1.0), 0, []
    while True:
        t += 1
        assert t <= 20000, f"beta {beta}: 1 - beta**t has not rounded to 1.0f by t = 20000"
        got, want = bias_corr_host(beta, t), np.float32(1.0 - beta ** t)
        assert got.dtype == np.float32
        if bits(got) != bits(want):
            differ.append((t, float(got), float(want)))
        if bits(got) == one and bits(want) == one:
            break
    assert differ == [], differ[:5]
    assert t > 100                                                     # (the loop did run over the whole warm-up of the correction)
    assert bits(bias_corr_host(beta, 10 ** 9)) == one and bits(bias_corr_host(beta, 0)) == bits(0.0)


def test_power_is_binary_exponentiation_with_one_rounding_per_product():
    """The fixed order, restated with exact rational arithmetic rounded to float64 after every product."""
    from fractions import Fraction
    for beta, t in ((0.9, 13), (0.95, 200), (0.999, 777), (0.99, 1)):
        r, x, k = Fraction(1), Fraction(beta), t
        while k:
            if k & 1:
                r = Fraction(float(r * x))
            k >>= 1
            if k:
                x = Fraction(float(x * x))
        want = np.float32(np.float64(1.0) - np.float64(float(r)))    # (the difference rounds once to float64, then once to float32)
        assert bits(bias_corr_host(beta, t)) == bits(want), (beta, t)
    with pytest.raises(ValueError):
        bias_corr_host(0.9, -1)


# ---------------------------------------------------------------------------------------------------- 2. decision and state
def test_found_nonfinite():
    for x in (float("nan"), float("inf"), -float("inf"), np.uint32(0xFFC00001).view(np.float32)):
        assert found_nonfinite_host(np.float32(x)) is True
    for x in (0.0, -0.0, 1e-45, 3.4028235e38, -3.4028235e38, 1.0):
        assert found_nonfinite_host(np.float32(x)) is False


def test_state_machine():
    betas = (0.9, 0.95)
    nan, inf = np.float32("nan"), np.float32("inf")
    seq = [np.float32(1.5), nan, inf, np.float32(0.0), np.float32(2.0), -inf, np.float32(1e30)]
    want = [((1, 0, 0), False), ((1, 1, 1), True), ((1, 2, 2), True), ((2, 2, 0), False), ((3, 2, 0), False), ((3, 3, 1), True),
            ((4, 3, 0), False)]
    state = (0, 0, 0)
    for norm, (st, skip) in zip(seq, want):
        before = state
        state, got_skip, bc1, bc2 = guard_step_host(state, norm, betas)
        assert state == st and got_skip is skip, (float(norm), state, st)
        if skip:
            assert bc1 is None and bc2 is None and state[0] == before[0]                 # applied and the corrections stay
        else:
            assert state[0] == before[0] + 1 and state[1] == before[1]
            assert bits(bc1) == bits(bias_corr_host(0.9, state[0])) == bits(np.float32(1.0 - 0.9 ** state[0]))
            assert bits(bc2) == bits(bias_corr_host(0.95, state[0])) == bits(np.float32(1.0 - 0.95 ** state[0]))
    # resumed counters, 64-bit wrap of the skip counters
    s, skip, _, _ = guard_step_host((41, (1 << 64) - 1, 7), nan, betas)
    assert s == (41, 0, 8) and skip
    s, skip, bc1, _ = guard_step_host((41, 5, 7), np.float32(1.0), betas)
    assert s == (42, 5, 0) and not skip and bits(bc1) == bits(np.float32(1.0 - 0.9 ** 42))


def test_check_skip_nonfinite():
    assert check_skip_nonfinite(True) is True and check_skip_nonfinite(False) is False
    assert check_skip_nonfinite(np.bool_(True)) is True
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(ValueError, match="skip_nonfinite"):
            check_skip_nonfinite(bad)


# ---------------------------------------------------------------------------------------------------- 3. library, bindings
def test_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "tulip_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, f"{name} is not declared in include/tulip_hip.h"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs == len(_lib.SIGNATURES[name]), name
        assert args[-1].startswith("hipStream_t")
        if name != "tulip_step_guard":
            assert args[-2].startswith("const uint32_t*") and args[-2].endswith("skip"), (name, args[-2])
    assert _lib.SIGNATURES["tulip_step_guard"] == [_lib.P, _lib.P, _lib.P, _lib.P, _lib.D, _lib.D, _lib.P]
    assert _lib.SIGNATURES["tulip_adamw_g"] == _lib.SIGNATURES["tulip_adamw_s"][:-1] + [_lib.P, _lib.P]
    assert _lib.SIGNATURES["tulip_adamw_blocks_g"] == _lib.SIGNATURES["tulip_adamw_blocks_s"][:-1] + [_lib.P, _lib.P]
    assert _lib.SIGNATURES["tulip_ema_update_g"] == _lib.SIGNATURES["tulip_ema_update"][:-1] + [_lib.P, _lib.P]
    from tulip_amd.csrc.build import build
    build(force=False, verbose=False)
    lib = _lib.load()
    assert lib.tulip_abi_version() == 6 == _lib.ABI_VERSION                           # additive: the ABI version stays
    with _lib.dev_library() as dev:
        assert dev is not lib
        for name in NEW:
            assert hasattr(lib, name) and hasattr(dev, name), name
    from tulip_amd import ops
    assert callable(ops.step_guard)


def test_bad_arguments_are_refused_on_the_host():
    """TULIP_ERR_ARG comes back before any launch: these calls need no GPU."""
    lib = _lib.load()
    buf = (ctypes.c_float * 32)()
    a = (ctypes.addressof(buf) + 15) & ~15
    ok = dict(norm=a, state=a, flag=a, hyper=a)
    for name, bad in (("norm NULL", dict(norm=None)), ("state NULL", dict(state=None)), ("flag NULL", dict(flag=None)),
                      ("hyper NULL", dict(hyper=None)), ("state misaligned", dict(state=a + 4))):
        k = dict(ok, **bad)
        assert lib.tulip_step_guard(k["norm"], k["state"], k["flag"], k["hyper"], 0.9, 0.95, None) == -1, name
    assert not any(buf)                                                                # nothing was written
    # the gated forms keep the refusals of the entries they extend
    assert lib.tulip_adamw_g(a, a, a, a, None, 6, a, None, None, 0, a, None) == -1                     # n % 4
    assert lib.tulip_adamw_g(a, a, a, a, None, 8, a, None, a, 0, a, None) == -1                        # a table without a mask
    assert lib.tulip_adamw_blocks_g(a, a, a, a, None, None, 1, a, None, None, 0, a, None) == -1       # blocks NULL
    assert lib.tulip_ema_update_g(a, a, 6, 0.5, None, a, a, None) == -1                                # n % 4
    assert lib.tulip_ema_update_g(a, a, 8, 1.5, None, a, a, None) == -1                                # decay out of range
    assert lib.tulip_ema_update_g(a, a + 4, 8, 0.5, None, a, a, None) == -1                            # misaligned shadow


def test_constructor_refuses_before_it_touches_the_device():
    from tulip_amd.trainer import Trainer
    for bad in (1, 0, None, "on"):
        with pytest.raises(ValueError, match="skip_nonfinite"):
            Trainer(None, 4, skip_nonfinite=bad)
    with pytest.raises(ValueError, match="sharded"):
        Trainer(None, 4, exchange="sharded", skip_nonfinite=True)

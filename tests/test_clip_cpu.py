"""Gradient clipping without a GPU: the host definition (tulip_amd/clip.py) against torch.nn.utils.clip_grad_norm_, the new
symbol in the header, both libraries and the bindings, the constructor's refusals, and the conditions that make the fixture
tests/golden/g18_clip.npz able to tell a clipped run from an unclipped one."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tulip_amd import _lib
from tulip_amd.clip import check_clip_grad, clip_coef_host, clipped_grad_scale_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(48, 4), (48,), (3, 5, 7), (1,), (144, 48), (2, 2)]


def grads(seed, scale=1.0):
    """Random fp32 gradients as parameters with .grad; the first element is exactly 1.0, so that the element after clipping IS
    the coefficient torch multiplied by (no rounding of a product, none of a quotient)."""
    g = torch.Generator().manual_seed(seed)
    ps = []
    for s in SHAPES:
        p = torch.nn.Parameter(torch.zeros(s))
        p.grad = torch.randn(s, generator=g) * scale
        ps.append(p)
    ps[0].grad.view(-1)[0] = 1.0
    return ps


def ulp_distance(a, b) -> int:
    ia, ib = (int(np.float32(x).view(np.int32)) for x in (a, b))
    return abs(ia - ib)


def clip_with_torch(ps, max_norm):
    before = [p.grad.clone() for p in ps]
    norm = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    return before, np.float32(norm.item()), np.float32(ps[0].grad.view(-1)[0].item())


# ---------------------------------------------------------------------------------------------------- 1. the host definition
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("scale", [1e-3, 1.0, 37.0])
def test_coefficient_is_torchs_when_it_clips(seed, scale):
    """norm well above max_norm: torch forms reciprocal(norm + 1e-6) * max_norm, one rounding more than the definition's single
    division -- 1.5 ulp from the exact quotient against 0.5: within 2 ulp of each other."""
    ps = grads(seed, scale)
    total = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in ps))
    for max_norm in (total / 1.5, total / 10.0, total / 1000.0):
        ps = grads(seed, scale)
        before, norm32, coef_torch = clip_with_torch(ps, max_norm)
        assert abs(float(norm32) - total) <= 1e-5 * total
        coef, c = clip_coef_host(norm32, max_norm)
        assert coef.dtype == np.float32 and coef == c and coef < 0.8
        assert ulp_distance(coef, coef_torch) <= 2, (float(coef), float(coef_torch))
        # ... and every element is its gradient times that coefficient
        for p, b in zip(ps, before):
            assert torch.equal(p.grad, b * torch.tensor(coef_torch))


@pytest.mark.parametrize("seed", [0, 1])
def test_coefficient_is_exactly_one_when_torch_does_not_clip(seed):
    ps = grads(seed)
    total = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in ps))
    for max_norm in (total * 1.5, total * 100.0, 1e9):
        ps = grads(seed)
        before, norm32, coef_torch = clip_with_torch(ps, max_norm)
        coef, c = clip_coef_host(norm32, max_norm)
        assert coef_torch == np.float32(1.0) and all(torch.equal(p.grad, b) for p, b in zip(ps, before))
        assert coef.view(np.uint32) == np.float32(1.0).view(np.uint32) and c > 1.0
        for base in (np.float32(1.0), np.float32(0.25), np.float32(1.0 / 3.0)):            # base keeps its bits
            assert clipped_grad_scale_host(base, coef).view(np.uint32) == base.view(np.uint32)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_norm_equal_to_max_norm(seed):
    """max_norm = the float32 norm itself: c = n / (n + 1e-6f) <= 1, never clamped; torch's value within 2 ulp."""
    ps = grads(seed, 10.0 ** (seed - 2))
    n32 = np.float32(torch.nn.utils.clip_grad_norm_(ps, 1e30).item())
    ps = grads(seed, 10.0 ** (seed - 2))
    _, norm32, coef_torch = clip_with_torch(ps, float(n32))
    assert norm32 == n32
    coef, c = clip_coef_host(norm32, float(n32))
    assert coef == c and coef <= np.float32(1.0)
    assert ulp_distance(coef, coef_torch) <= 2, (float(coef), float(coef_torch))


def test_zero_nan_and_infinite_gradients():
    zero = [torch.nn.Parameter(torch.zeros(s)) for s in SHAPES]
    for p in zero:
        p.grad = torch.zeros_like(p)
    n = torch.nn.utils.clip_grad_norm_(zero, 1.0)
    coef, _ = clip_coef_host(np.float32(n.item()), 1.0)
    assert n.item() == 0.0 and coef == np.float32(1.0) and all(not p.grad.any() for p in zero)
    # NaN propagates (error_if_nonfinite=False): a NaN norm, a NaN coefficient, NaN gradients
    ps = grads(0)
    ps[2].grad.view(-1)[3] = float("nan")
    _, norm32, coef_torch = clip_with_torch(ps, 1.0)
    coef, _ = clip_coef_host(norm32, 1.0)
    assert np.isnan(norm32) and np.isnan(coef) and np.isnan(coef_torch)
    assert np.isnan(clipped_grad_scale_host(np.float32(1.0), coef))
    # an infinite norm gives 0: every finite gradient becomes 0
    ps = grads(0)
    ps[2].grad.view(-1)[3] = float("inf")
    _, norm32, coef_torch = clip_with_torch(ps, 1.0)
    coef, _ = clip_coef_host(norm32, 1.0)
    assert np.isinf(norm32) and coef == np.float32(0.0) and coef_torch == np.float32(0.0)
    assert not ps[1].grad.any() and clipped_grad_scale_host(np.float32(0.5), coef) == np.float32(0.0)


def test_definition_rounds_once_per_operation():
    """float32 throughout: the sum norm + 1e-6f and the quotient are rounded separately."""
    norm32, mx = np.float32(2.1848207), 0.25
    s = np.float32(np.float64(norm32) + np.float64(np.float32(1e-6)))
    want = np.float32(np.float64(np.float32(mx)) / np.float64(s))
    coef, _ = clip_coef_host(norm32, mx)
    assert coef.view(np.uint32) == want.view(np.uint32)
    assert clipped_grad_scale_host(0.25, coef) == np.float32(np.float64(np.float32(0.25)) * np.float64(coef))
    assert clip_coef_host(np.float32(3.0), 0.0)[0] == np.float32(0.0)                  # max_norm 0: every step is wd only
    with pytest.raises(ValueError):
        check_clip_grad(-1e-9)
    with pytest.raises(ValueError):
        check_clip_grad(float("nan"))
    assert check_clip_grad(0) == 0.0 and check_clip_grad(np.float32(2.5)) == 2.5


# ---------------------------------------------------------------------------------------------------- 2. symbol, constructor
def test_symbol_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "tulip_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+tulip_grad_clip\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m, "tulip_grad_clip is not declared in include/tulip_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 7 == len(_lib.SIGNATURES["tulip_grad_clip"])
    assert args[0].startswith("const float*") and args[1].startswith("int64_t") and args[2].startswith("double*")
    assert args[3].startswith("float*") and args[4].startswith("const float*") and args[6].startswith("hipStream_t")
    assert _lib.SIGNATURES["tulip_grad_clip"] == [_lib.P, _lib.L, _lib.P, _lib.P, _lib.P, _lib.P, _lib.P]
    from tulip_amd.csrc.build import build
    build(force=False, verbose=False)
    lib = _lib.load()
    assert hasattr(lib, "tulip_grad_clip") and lib.tulip_abi_version() == 6           # additive: the ABI version stays
    with _lib.dev_library() as dev:
        assert hasattr(dev, "tulip_grad_clip") and dev is not lib
    from tulip_amd import ops
    assert callable(ops.grad_clip)


def test_bad_arguments_are_refused_on_the_host():
    """TULIP_ERR_ARG comes back before any launch: these calls need no GPU."""
    import ctypes
    lib = _lib.load()
    buf = (ctypes.c_float * 16)()
    a = (ctypes.addressof(buf) + 15) & ~15
    ok = dict(g=a, n=4, partials=a, grad_scale=a, max_norm=a, out=a)
    for name, bad in (("n == 0", dict(n=0)), ("n < 0", dict(n=-4)), ("partials NULL", dict(partials=None)),
                      ("grad_scale NULL", dict(grad_scale=None)), ("max_norm NULL", dict(max_norm=None)),
                      ("out NULL", dict(out=None)), ("g NULL", dict(g=None)), ("g misaligned", dict(g=a + 4))):
        k = dict(ok, **bad)
        assert lib.tulip_grad_clip(k["g"], k["n"], k["partials"], k["grad_scale"], k["max_norm"], k["out"], None) == -1, name


def test_constructor_refuses_before_it_touches_the_device():
    from tulip_amd.trainer import Trainer
    for bad in (-1, -1e-9, float("nan")):
        with pytest.raises(ValueError, match="clip_grad"):
            Trainer(None, 4, clip_grad=bad)
    with pytest.raises(ValueError, match="sharded"):
        Trainer(None, 4, exchange="sharded", clip_grad=1.0)


# ---------------------------------------------------------------------------------------------------- 3. the fixture
def test_fixture_can_tell_clipping_from_none(golden_dir):
    z = np.load(os.path.join(golden_dir, "g18_clip.npz"))
    clip = float(z["clip_grad"])
    assert int(z["steps"]) == 4 == len(z["loss"]) == len(z["grad_norm"]) == len(z["m_norm"]) == len(z["v_norm"])
    assert np.all(z["grad_norm"] > 1.25 * clip), (z["grad_norm"], clip)               # active at every step, coef < 0.8
    for key, rtol in (("m_norm", 2e-2), ("v_norm", 4e-2)):                            # 5 x the GPU test's tolerances apart
        a, b = z[key + "_unclipped"], z[key]
        assert np.all(np.abs(a - b) > 5.0 * rtol * np.abs(b)), key
    # the same start: the first loss and the first norm do not know about the clip
    assert z["loss"][0] == z["loss_unclipped"][0] and abs(z["grad_norm"][0] - z["grad_norm_unclipped"][0]) <= 1e-6 * z["grad_norm"][0]
    # the first step's moments are the definition: exp_avg = 0.1 g coef
    coef, _ = clip_coef_host(np.float32(z["grad_norm"][0]), clip)
    assert abs(z["m_norm"][0] - 0.1 * z["grad_norm"][0] * float(coef)) <= 1e-5 * z["m_norm"][0]

"""The selectable training loss without a GPU: the host definition (tulip_amd/loss.py) against the reference's berHu function as
recorded in tests/golden/g19_loss.npz, the C == 0 departure, NaN propagation, the names check_loss accepts, the constructor
keyword, and the new symbols in the header, both libraries and the bindings with their refusals before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tulip_amd import _lib
from tulip_amd import loss as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "g19_loss.npz")
NEW = {"tulip_loss_blocks": 1, "tulip_loss_stats": 6, "tulip_loss_bwd": 10, "tulip_loss_value": 6, "tulip_loss_final": 7}


def rel_l2(a, b) -> float:
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


# ---------------------------------------------------------------------------------------------------- 1. the definition
@pytest.mark.parametrize("case", [0, 1])
def test_berhu_matches_the_reference_function(case):
    """Value, C and gradient against the reference's inverse_huber_loss and its autograd, float64 on both sides."""
    g = np.load(GOLD)
    assert int(g["n_cases"]) == 2
    pred, target = g[f"pred{case}"], g[f"target{case}"]
    assert pred.dtype == np.float32 and pred.shape == ((2, 1, 16, 64), (2, 2, 8, 32))[case]
    np.testing.assert_allclose(L.berhu_c(pred, target), g[f"c{case}"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(L.berhu_values(pred, target), g[f"values{case}"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(L.loss_value("berhu", pred, target), g[f"mean{case}"], rtol=1e-12, atol=0)
    grad = L.loss_grad("berhu", pred, target)
    assert grad.dtype == np.float64 and grad.shape == pred.shape
    np.testing.assert_allclose(grad, g[f"grad{case}"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(L.loss_grad("berhu", pred, target, gscale=0.25), 0.25 * g[f"grad{case}"], rtol=1e-12, atol=0)
    # the fixture's two conditions, re-asserted: both branches are exercised, and berHu is not L1
    d = pred.astype(np.float64) - target.astype(np.float64)
    share = float(np.mean(np.abs(d) >= g[f"c{case}"]))
    assert share == float(g[f"share{case}"]) and 0.1 <= share <= 0.9
    assert rel_l2(g[f"grad{case}"], L.loss_grad("l1", pred, target)) > 0.10
    # the torch form of the definition (what the GPU test back-propagates through the oracle) is the same function
    p = torch.from_numpy(pred).double().requires_grad_(True)
    v = L.torch_loss("berhu", p, torch.from_numpy(target).double())
    v.backward()
    np.testing.assert_allclose(v.item(), g[f"mean{case}"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(p.grad.numpy(), g[f"grad{case}"], rtol=1e-12, atol=0)


def test_l1_and_l2_definitions():
    rng = np.random.default_rng(5)
    pred, target = rng.standard_normal((3, 7)).astype(np.float32), rng.standard_normal((3, 7)).astype(np.float32)
    d = pred.astype(np.float64) - target.astype(np.float64)
    assert L.loss_value("l2", pred, target) == np.mean(d * d) and L.loss_value("l1", pred, target) == np.mean(np.abs(d))
    np.testing.assert_array_equal(L.loss_grad("l2", pred, target), 2.0 * d / d.size)
    np.testing.assert_array_equal(L.loss_grad("l1", pred, target), np.sign(d) / d.size)
    for kind in ("l1", "l2"):
        p = torch.from_numpy(pred).double().requires_grad_(True)
        v = L.torch_loss(kind, p, torch.from_numpy(target).double())
        v.backward()
        np.testing.assert_allclose(v.item(), L.loss_value(kind, pred, target), rtol=1e-14)
        np.testing.assert_allclose(p.grad.numpy(), L.loss_grad(kind, pred, target), rtol=1e-14, atol=0)
    # pixel_loss is the L1 metric whatever the kind: of expm1 with log_transform, of the values without
    assert L.pixel_loss(pred, target, False) == np.mean(np.abs(d))
    assert L.pixel_loss(pred, target, True) == np.mean(np.abs(np.expm1(pred.astype(np.float64)) - np.expm1(target.astype(np.float64))))
    # the device's C is one float32 product
    c32 = L.berhu_c32(pred, target)
    assert c32.dtype == np.float32 and c32 == np.float32(0.2) * np.max(np.abs(pred - target))


def test_c_zero_gives_zero_loss_and_zero_gradient():
    """pred == target everywhere: the reference's formula is 0/0; here loss and gradient are 0 (the documented departure)."""
    x = np.random.default_rng(0).standard_normal((2, 1, 4, 8)).astype(np.float32)
    assert L.berhu_c(x, x) == 0.0
    assert L.loss_value("berhu", x, x) == 0.0
    g = L.loss_grad("berhu", x, x)
    assert g.shape == x.shape and not g.any()
    assert not L.berhu_values(x, x).any()
    p = torch.from_numpy(x).requires_grad_(True)
    v = L.torch_loss("berhu", p, torch.from_numpy(x))
    v.backward()
    assert v.item() == 0.0 and not p.grad.numpy().any()


@pytest.mark.parametrize("kind", ["l1", "l2", "berhu"])
def test_nonfinite_inputs_give_a_nonfinite_loss(kind):
    rng = np.random.default_rng(1)
    pred, target = rng.standard_normal(257).astype(np.float32), rng.standard_normal(257).astype(np.float32)
    bad = target.copy()
    bad[-1] = np.nan
    assert np.isnan(L.loss_value(kind, pred, bad))
    if kind != "l1":
        assert np.isnan(L.loss_grad(kind, pred, bad)[-1])
    if kind == "berhu":
        assert np.isnan(L.berhu_c(pred, bad)) and np.isnan(L.berhu_c32(pred, bad))
    bad[-1] = np.inf
    assert not np.isfinite(L.loss_value(kind, pred, bad))


def test_check_loss():
    for name in ("l1", "l2", "berhu"):
        assert L.check_loss(name) == name
    for bad in ("huber", "L1", "", None, 1, "smooth_l1"):
        with pytest.raises(ValueError, match="loss"):
            L.check_loss(bad)
    with pytest.raises(ValueError):
        L.loss_value("huber", np.zeros(2), np.zeros(2))


# ---------------------------------------------------------------------------------------------------- 2. the constructor
def test_constructor_keyword():
    from functools import partial
    import torch.nn as nn
    from oracle import tulip_oracle as O
    from tulip_amd.model import tulip as T
    cfg = O.tiny_config()
    with pytest.raises(ValueError, match="loss"):
        T.TULIP(loss="huber")
    with pytest.raises(ValueError, match="loss"):
        T.tulip_base(loss="huber")
    # positional construction in the reference's argument order (tulip.py:531-535) still works, and `loss` trails it
    m = T.TULIP(cfg.img_size, cfg.target_img_size, cfg.patch_size, 1, cfg.embed_dim, [2, 8], cfg.depths, cfg.num_heads, 4.0, True,
                0.0, 0.0, 0.0, partial(nn.LayerNorm, eps=1e-6), True, True, True, False, True, True)
    assert m.loss == "l1" and m.pixel_shuffle and m.circular_padding and m.log_transform and m.patch_unmerging
    kw = dict(img_size=cfg.img_size, target_img_size=cfg.target_img_size, patch_size=cfg.patch_size, embed_dim=cfg.embed_dim,
              window_size=[2, 8], depths=cfg.depths, num_heads=cfg.num_heads, pixel_shuffle=True, circular_padding=True,
              log_transform=True, patch_unmerging=True)
    b = T.TULIP(loss="berhu", **kw)
    assert b.loss == "berhu" and T.TULIP(loss="l2", **kw).loss == "l2" and T.TULIP(**kw).loss == "l1"
    assert list(b.state_dict().keys()) == list(m.state_dict().keys())                 # the choice is not state
    with pytest.raises(AttributeError):
        b.loss = "l1"                                                                  # fixed at construction


def test_default_state_dict_keys_are_unchanged():
    from tulip_amd.model import tulip as T
    keys = list(T.TULIP().state_dict().keys())
    assert keys == list(T.TULIP(loss="berhu").state_dict().keys())
    assert len(keys) == len(set(keys)) and not any("loss" in k for k in keys)
    assert list(T.tulip_base(loss="l2").state_dict().keys()) == list(T.tulip_base().state_dict().keys())     # through **kwargs


def test_trainer_refuses_sharded_before_it_touches_the_device():
    from tulip_amd.trainer import Trainer

    class M:
        loss = "berhu"
    with pytest.raises(ValueError, match="sharded"):
        Trainer(M(), 2, exchange="sharded")
    M.loss = "huber"
    with pytest.raises(ValueError, match="loss"):
        Trainer(M(), 2)


# ---------------------------------------------------------------------------------------------------- 3. library, bindings
def test_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "tulip_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, f"{name} is not declared in include/tulip_hip.h"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs == len(_lib.SIGNATURES[name]), name
        if name != "tulip_loss_blocks":
            assert args[-1].startswith("hipStream_t")
    for k, v in (("TULIP_LOSS_L1", _lib.LOSS_L1), ("TULIP_LOSS_L2", _lib.LOSS_L2), ("TULIP_LOSS_BERHU", _lib.LOSS_BERHU),
                 ("TULIP_LOSS_BLOCKS_MAX", _lib.LOSS_BLOCKS_MAX)):
        assert re.search(r"#define\s+" + k + r"\s+" + str(v) + r"\b", hdr), k
    from tulip_amd.csrc.build import SOURCES, build
    assert "loss.hip" in SOURCES
    build(force=False, verbose=False)
    lib = _lib.load()
    assert lib.tulip_abi_version() == 6 == _lib.ABI_VERSION                           # additive: the ABI version stays
    with _lib.dev_library() as dev:
        assert dev is not lib
        for name in NEW:
            assert hasattr(lib, name) and hasattr(dev, name), name
    from tulip_amd import ops
    assert all(callable(getattr(ops, f)) for f in ("loss_stats", "loss_bwd", "loss_value", "loss_final", "loss_blocks"))
    assert ops.LOSS_KINDS == {"l1": 0, "l2": 1, "berhu": 2} and set(ops.LOSS_KINDS) == set(L.KINDS)


def test_grid_is_at_most_1024_workgroups():
    lib = _lib.load()
    for n, want in ((1, 1), (3, 1), (255, 1), (257, 1), (1024, 1), (1025, 2), (1024 * 256 + 5, 257), (1 << 20, 1024),
                    ((1 << 20) + 1, 1024), (1 << 33, 1024), (0, 0), (-4, 0)):
        assert lib.tulip_loss_blocks(n) == want, n


def test_bad_arguments_are_refused_on_the_host():
    """TULIP_ERR_ARG comes back before any launch: these calls need no GPU."""
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    a = (ctypes.addressof(buf) + 15) & ~15
    for kind in (-1, 3, 99):
        assert lib.tulip_loss_bwd(kind, a, a, a, None, 1.0, a, a, 8, None) == -1
        assert lib.tulip_loss_final(kind, a, a, a, 8, 0, None) == -1
    for n in (0, -1):
        assert lib.tulip_loss_stats(a, a, a, n, 0, None) == -1
        assert lib.tulip_loss_bwd(_lib.LOSS_L2, a, a, None, None, 1.0, a, None, n, None) == -1
        assert lib.tulip_loss_value(a, a, a, a, n, None) == -1
        assert lib.tulip_loss_final(_lib.LOSS_L2, a, None, a, n, 0, None) == -1
    assert lib.tulip_loss_stats(None, a, a, 8, 0, None) == -1 and lib.tulip_loss_stats(a, None, a, 8, 0, None) == -1
    assert lib.tulip_loss_stats(a, a, None, 8, 0, None) == -1 and lib.tulip_loss_stats(a, a, a + 4, 8, 0, None) == -1
    assert lib.tulip_loss_bwd(_lib.LOSS_L2, None, a, None, None, 1.0, a, None, 8, None) == -1
    assert lib.tulip_loss_bwd(_lib.LOSS_L2, a, None, None, None, 1.0, a, None, 8, None) == -1
    assert lib.tulip_loss_bwd(_lib.LOSS_L2, a, a, None, None, 1.0, None, None, 8, None) == -1
    assert lib.tulip_loss_bwd(_lib.LOSS_BERHU, a, a, None, None, 1.0, a, a, 8, None) == -1          # berHu reads the maxima
    assert lib.tulip_loss_bwd(_lib.LOSS_BERHU, a, a, a, None, 1.0, a, None, 8, None) == -1          # ... and writes C
    assert lib.tulip_loss_value(a, a, None, a, 8, None) == -1 and lib.tulip_loss_value(a, a, a, None, 8, None) == -1
    assert lib.tulip_loss_final(_lib.LOSS_BERHU, a, None, a, 8, 0, None) == -1
    assert lib.tulip_loss_final(_lib.LOSS_L2, None, None, a, 8, 0, None) == -1
    assert lib.tulip_loss_final(_lib.LOSS_L2, a, None, None, 8, 0, None) == -1
    assert not any(buf)                                                                # nothing was written

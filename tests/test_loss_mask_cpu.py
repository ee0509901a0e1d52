"""The masked training loss without a GPU, TULIP(loss_valid_min=...): the host definition (tulip_amd/loss.py) against the unmasked
functions on the compressed valid elements, the channel-0 rule, the edge values, the constructor keyword, the four new symbols in
the header, both libraries and the bindings with their refusals before any launch, and the engine's launch sequence read off the
dry-run launch log (tests/dry_run.py)."""
import ctypes
import functools
import os
import re
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn as nn

from dry_run import dry_run
from oracle import tulip_oracle as O
from tulip_amd import _lib
from tulip_amd import loss as L
from tulip_amd.engine import TulipEngine
from tulip_amd.model import tulip as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"tulip_loss_stats_m": 10, "tulip_loss_bwd_m": 15, "tulip_loss_value_m": 10, "tulip_loss_final_m": 9}
NAN, INF = float("nan"), float("inf")


def data(shape=(2, 2, 5, 7), seed=0):
    """seeded float32 (pred, target): about half the pixels have target channel 0 <= 0"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)


def torch_grad(kind, pred, target, valid_min):
    p = torch.from_numpy(np.asarray(pred)).double().requires_grad_(True)
    v = L.torch_loss(kind, p, torch.from_numpy(np.asarray(target)).double(), valid_min=valid_min)
    v.backward()
    return v.item(), p.grad.numpy()


# ---------------------------------------------------------------------------------------------------- 1. the definition
@pytest.mark.parametrize("kind", L.KINDS)
def test_masked_functions_are_the_unmasked_ones_on_the_valid_elements(kind):
    pred, target = data()
    v = 0.0
    m = L.valid_mask(target, v)
    assert m.shape == target.shape and m.dtype == bool and np.array_equal(m, np.broadcast_to(target[:, :1] > v, target.shape))
    nv = int(m.sum())
    assert 0 < nv < m.size and nv == 2 * int((target[:, 0] > v).sum())
    pv, tv = pred[m], target[m]                                            # the compressed valid elements: n_v of them
    np.testing.assert_allclose(L.loss_value(kind, pred, target, valid_min=v), L.loss_value(kind, pv, tv), rtol=1e-12, atol=0)
    for lt in (False, True):
        np.testing.assert_allclose(L.pixel_loss(pred, target, lt, valid_min=v), L.pixel_loss(pv, tv, lt), rtol=1e-12, atol=0)
    np.testing.assert_allclose(L.berhu_c(pred, target, valid_min=v), L.berhu_c(pv, tv), rtol=1e-12, atol=0)
    assert L.berhu_c32(pred, target, valid_min=v) == L.berhu_c32(pv, tv)
    for gs in (1.0, 0.25):
        g = L.loss_grad(kind, pred, target, gs, valid_min=v)
        assert g.shape == pred.shape and g.dtype == np.float64
        np.testing.assert_allclose(g[m], L.loss_grad(kind, pv, tv, gs), rtol=1e-12, atol=0)
        assert not g[~m].any() and not np.signbit(g[~m]).any()              # exactly +0 at the invalid elements
    vals = L.berhu_values(pred, target, valid_min=v)
    np.testing.assert_allclose(vals[m], L.berhu_values(pv, tv), rtol=1e-12, atol=0)
    assert not vals[~m].any()
    # the masked loss is not the unmasked one on this data
    assert abs(L.loss_value(kind, pred, target, valid_min=v) - L.loss_value(kind, pred, target)) > 1e-3
    # the torch form of the definition: the same value, and its autograd is loss_grad
    tv_, tg = torch_grad(kind, pred, target, v)
    np.testing.assert_allclose(tv_, L.loss_value(kind, pred, target, valid_min=v), rtol=1e-12, atol=0)
    np.testing.assert_allclose(tg, L.loss_grad(kind, pred, target, valid_min=v), rtol=1e-12, atol=0)
    assert not tg[~m].any()


@pytest.mark.parametrize("kind", L.KINDS)
def test_valid_min_none_returns_the_bits_of_the_call_without_the_keyword(kind):
    pred, target = data(seed=1)
    same = lambda a, b: np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))
    assert same(L.loss_value(kind, pred, target, valid_min=None), L.loss_value(kind, pred, target))
    assert same(L.loss_grad(kind, pred, target, 0.5, valid_min=None), L.loss_grad(kind, pred, target, 0.5))
    assert same(L.pixel_loss(pred, target, True, valid_min=None), L.pixel_loss(pred, target, True))
    assert same(L.berhu_c(pred, target, valid_min=None), L.berhu_c(pred, target))
    assert L.berhu_c32(pred, target, valid_min=None).view(np.uint32) == L.berhu_c32(pred, target).view(np.uint32)
    assert same(L.berhu_values(pred, target, valid_min=None), L.berhu_values(pred, target))
    p = torch.from_numpy(pred).double()
    t = torch.from_numpy(target).double()
    assert torch.equal(L.torch_loss(kind, p, t, valid_min=None), L.torch_loss(kind, p, t))
    assert L.valid_mask(target, None).all() and L.valid_mask(target, None).shape == target.shape
    # a threshold below every target value: every element counts, the unmasked values
    np.testing.assert_allclose(L.loss_value(kind, pred, target, valid_min=-100.0), L.loss_value(kind, pred, target), rtol=1e-14)
    np.testing.assert_allclose(L.loss_grad(kind, pred, target, valid_min=-100.0), L.loss_grad(kind, pred, target), rtol=1e-14)


# ---------------------------------------------------------------------------------------------------- 2. the channel-0 rule
@pytest.mark.parametrize("kind", L.KINDS)
def test_channel_0_decides_for_every_channel(kind):
    """in_chans == 2: a zero in channel 1 (intensity) of a valid pixel counts; a non-zero channel 1 of an invalid pixel does not."""
    pred, target = data((2, 2, 4, 6), seed=2)
    target[:, 0] = np.abs(target[:, 0]) + 0.5                     # every pixel valid ...
    target[0, 0, 1, 2] = 0.0                                      # ... but this hole,
    target[0, 1, 1, 2] = 3.0                                      # whose intensity is not zero,
    target[1, 1, 3, 5] = 0.0                                      # and a valid return of intensity 0
    m = L.valid_mask(target, 0.0)
    assert not m[0, 0, 1, 2] and not m[0, 1, 1, 2] and m[1, 0, 3, 5] and m[1, 1, 3, 5]
    assert int(m.sum()) == target.size - 2
    g = L.loss_grad(kind, pred, target, valid_min=0.0)
    assert g[0, 0, 1, 2] == 0.0 and g[0, 1, 1, 2] == 0.0 and g[1, 1, 3, 5] != 0.0
    base = L.loss_value(kind, pred, target, valid_min=0.0)
    moved = target.copy()
    moved[0, 1, 1, 2] = -50.0                                     # the invalid pixel's intensity: nothing changes
    assert L.loss_value(kind, pred, moved, valid_min=0.0) == base
    assert np.array_equal(L.loss_grad(kind, pred, moved, valid_min=0.0), g)
    moved = target.copy()
    moved[1, 1, 3, 5] = 0.25                                      # the valid pixel's intensity: the loss follows
    assert L.loss_value(kind, pred, moved, valid_min=0.0) != base
    # channel 1 alone never makes a pixel valid or invalid
    flipped = target.copy()
    flipped[:, 1] = -np.abs(flipped[:, 1])
    assert np.array_equal(L.valid_mask(flipped, 0.0), m)


# ---------------------------------------------------------------------------------------------------- 3. edge values
@pytest.mark.parametrize("kind", L.KINDS)
def test_edge_values(kind):
    pred, target = data((2, 2, 4, 6), seed=3)
    # no valid pixel: zeros, not 0/0
    none = target.copy()
    none[:, 0] = -np.abs(none[:, 0])
    assert L.loss_value(kind, pred, none, valid_min=0.0) == 0.0 and L.pixel_loss(pred, none, True, valid_min=0.0) == 0.0
    assert L.berhu_c(pred, none, valid_min=0.0) == 0.0 and L.berhu_c32(pred, none, valid_min=0.0) == 0.0
    g = L.loss_grad(kind, pred, none, valid_min=0.0)
    assert g.shape == pred.shape and not g.any() and not L.berhu_values(pred, none, valid_min=0.0).any()
    v, tg = torch_grad(kind, pred, none, 0.0)
    assert v == 0.0 and not tg.any()
    # NaN / inf at invalid pixels, in pred and in every channel of target, are ignored; a NaN in target[:, 0] is invalid
    target[0, 0, 0, 0], target[1, 0, 2, 3] = -1.0, -2.0                       # two invalid pixels
    target[0, 0, 1, 1], target[0, 0, 3, 5] = 1.5, 0.5                         # two valid ones (below)
    want = L.loss_value(kind, pred, target, valid_min=0.0)
    want_g, want_c = L.loss_grad(kind, pred, target, valid_min=0.0), L.berhu_c(pred, target, valid_min=0.0)
    want_p = L.pixel_loss(pred, target, True, valid_min=0.0)
    bad_p, bad_t = pred.copy(), target.copy()
    bad_p[0, :, 0, 0] = (NAN, INF)
    bad_t[0, 1, 0, 0] = NAN
    bad_p[1, 1, 2, 3], bad_t[1, 1, 2, 3] = -INF, INF
    assert L.loss_value(kind, bad_p, bad_t, valid_min=0.0) == want and L.pixel_loss(bad_p, bad_t, True, valid_min=0.0) == want_p
    assert np.array_equal(L.loss_grad(kind, bad_p, bad_t, valid_min=0.0), want_g)
    assert L.berhu_c(bad_p, bad_t, valid_min=0.0) == want_c
    v, tg = torch_grad(kind, bad_p, bad_t, 0.0)
    np.testing.assert_allclose(v, want, rtol=1e-12)
    np.testing.assert_allclose(tg, want_g, rtol=1e-12, atol=0)
    nan0 = target.copy()
    nan0[0, 0, 1, 1] = NAN                                                    # a valid pixel becomes invalid: finite, one pixel fewer
    m = L.valid_mask(nan0, 0.0)
    assert not m[0, :, 1, 1].any() and int(m.sum()) == int(L.valid_mask(target, 0.0).sum()) - 2
    assert np.isfinite(L.loss_value(kind, pred, nan0, valid_min=0.0))
    assert np.isfinite(L.loss_grad(kind, pred, nan0, valid_min=0.0)).all()
    # a NaN at a valid element propagates as it does without the mask
    bad_p = pred.copy()
    bad_p[0, 1, 3, 5] = NAN
    assert np.isnan(L.loss_value(kind, bad_p, target, valid_min=0.0))
    bad_t = target.copy()
    bad_t[0, 1, 3, 5] = INF                                                   # (channel 1 of a valid pixel)
    assert not np.isfinite(L.loss_value(kind, pred, bad_t, valid_min=0.0))
    if kind == "berhu":
        assert np.isnan(L.berhu_c(bad_p, target, valid_min=0.0)) and np.isnan(L.berhu_c32(bad_p, target, valid_min=0.0))


def test_berhu_threshold_is_the_maximum_over_the_valid_elements():
    pred, target = data((1, 1, 8, 16), seed=4)
    target[0, 0, 2, 3] = -1.0
    pred[0, 0, 2, 3] = 11.0                                                  # the largest |d|, at an invalid pixel
    assert L.berhu_c(pred, target) == 0.2 * 12.0
    d = np.abs(pred.astype(np.float64) - target)[L.valid_mask(target, 0.0)]
    assert L.berhu_c(pred, target, valid_min=0.0) == 0.2 * d.max() < 0.2 * 12.0
    assert L.berhu_c32(pred, target, valid_min=0.0) == np.float32(0.2) * np.float32(np.abs(pred - target)[target > 0].max())


# ---------------------------------------------------------------------------------------------------- 4. the constructor keyword
def test_check_valid_min():
    assert L.check_valid_min(None) is None
    for v in (0.0, -1.0, 0.5, np.float32(0.25), np.float64(1e-3)):
        got = L.check_valid_min(v)
        assert type(got) is float and got == float(v)
    for bad in (True, False, np.bool_(True), NAN, INF, -INF, np.float32("nan"), "0.0", 0, 1, [0.0], (0.0,), torch.zeros(())):
        with pytest.raises(ValueError, match="loss_valid_min"):
            L.check_valid_min(bad)
    with pytest.raises(ValueError):
        L.loss_value("l1", np.zeros((1, 1, 2)), np.zeros((1, 1, 2)), valid_min=NAN)
    with pytest.raises(ValueError):
        L.valid_mask(np.zeros(4), 0.0)                                        # no channel axis


def tiny(**kw):
    cfg = O.tiny_config()
    return T.TULIP(img_size=cfg.img_size, target_img_size=cfg.target_img_size, patch_size=cfg.patch_size, embed_dim=cfg.embed_dim,
                   window_size=[2, 8], depths=cfg.depths, num_heads=cfg.num_heads, norm_layer=partial(nn.LayerNorm, eps=1e-6),
                   **dict(dict(pixel_shuffle=True, circular_padding=True, log_transform=True, patch_unmerging=True), **kw))


def test_constructor_keyword():
    cfg = O.tiny_config()
    for bad in (True, NAN, INF, "0", 0):
        with pytest.raises(ValueError, match="loss_valid_min"):
            T.TULIP(loss_valid_min=bad)
        with pytest.raises(ValueError, match="loss_valid_min"):
            T.tulip_base(loss_valid_min=bad)
    plain = tiny()
    assert plain.loss_valid_min is None and tiny(loss_valid_min=None).loss_valid_min is None
    m = tiny(loss="berhu", loss_valid_min=0.0)
    assert m.loss == "berhu" and m.loss_valid_min == 0.0 and type(m.loss_valid_min) is float
    assert tiny(loss_valid_min=-0.5).loss == "l1" and tiny(loss_valid_min=-0.5).loss_valid_min == -0.5
    assert list(m.state_dict().keys()) == list(plain.state_dict().keys())                       # the setting is not state
    assert not any("valid" in k for k in m.state_dict())
    with pytest.raises(AttributeError):
        m.loss_valid_min = 1.0                                                                  # fixed at construction
    # the keyword trails `loss` behind the reference's positional arguments (tulip.py:531-535)
    pos = T.TULIP(cfg.img_size, cfg.target_img_size, cfg.patch_size, 1, cfg.embed_dim, [2, 8], cfg.depths, cfg.num_heads, 4.0, True,
                  0.0, 0.0, 0.0, partial(nn.LayerNorm, eps=1e-6), True, True, True, False, True, True, "l2", 0.25)
    assert pos.loss == "l2" and pos.loss_valid_min == 0.25
    # through **kwargs
    b = T.tulip_base(loss="l2", loss_valid_min=0.0)
    assert b.loss_valid_min == 0.0 and list(b.state_dict().keys()) == list(T.tulip_base().state_dict().keys())
    assert T.tulip_large(loss_valid_min=0.5).loss_valid_min == 0.5
    assert TulipEngine(m).loss_valid_min == 0.0 and TulipEngine(plain).loss_valid_min is None


def test_trainer_refuses_sharded_before_it_touches_the_device():
    from tulip_amd.trainer import Trainer

    class M:
        loss = "l1"
        loss_valid_min = 0.0
    with pytest.raises(ValueError, match="sharded.*loss_valid_min|loss_valid_min.*sharded"):
        Trainer(M(), 2, exchange="sharded")
    M.loss_valid_min = NAN
    with pytest.raises(ValueError, match="loss_valid_min"):
        Trainer(M(), 2)


# ---------------------------------------------------------------------------------------------------- 5. library, bindings
def test_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "tulip_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, f"{name} is not declared in include/tulip_hip.h"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs == len(_lib.SIGNATURES[name]), name
        assert args[-1].startswith("hipStream_t")
        for want in ("uint32_t* counts",) + (("int chans", "int64_t chan_stride", "float valid_min") if "final" not in name else ()) + (
                ("int64_t* n_valid",) if name in ("tulip_loss_bwd_m", "tulip_loss_final_m") else ()):
            assert any(a.endswith(want) for a in args), (name, want)
    assert re.search(r"#define\s+TULIP_ABI_VERSION\s+6\b", hdr)
    from tulip_amd.csrc.build import build
    build(force=False, verbose=False)
    lib = _lib.load()
    assert lib.tulip_abi_version() == 6 == _lib.ABI_VERSION                           # additive: the ABI version stays
    with _lib.dev_library() as dev:
        assert dev is not lib
        for name in NEW:
            assert hasattr(lib, name) and hasattr(dev, name), name
    from tulip_amd import ops
    assert all(callable(getattr(ops, f)) for f in ("loss_stats_m", "loss_bwd_m", "loss_value_m", "loss_final_m"))


def test_bad_arguments_are_refused_on_the_host():
    """TULIP_ERR_ARG comes back before any launch: these calls need no GPU."""
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    a = (ctypes.addressof(buf) + 15) & ~15
    stats = lambda *x, pred=a, target=a, st=a, n=8, c=1, hw=8, v=0.0, cnt=a: lib.tulip_loss_stats_m(pred, target, st, n, 0, c, hw, v, cnt, None)
    bwd = lambda kind=_lib.LOSS_L2, pred=a, target=a, st=a, dp=a, lc=a, n=8, c=1, hw=8, v=0.0, cnt=a, nv=a: lib.tulip_loss_bwd_m(
        kind, pred, target, st, None, 1.0, dp, lc, n, c, hw, v, cnt, nv, None)
    value = lambda pred=a, target=a, st=a, vp=a, n=8, c=1, hw=8, v=0.0, cnt=a: lib.tulip_loss_value_m(pred, target, st, vp, n, c, hw, v, cnt, None)
    final = lambda kind=_lib.LOSS_L2, st=a, vp=a, lo=a, n=8, cnt=a, nv=a: lib.tulip_loss_final_m(kind, st, vp, lo, n, 0, cnt, nv, None)
    for kind in (-1, 3, 99):
        assert bwd(kind=kind) == -1 and final(kind=kind) == -1
    for n in (0, -1):
        assert stats(n=n) == -1 and bwd(n=n) == -1 and value(n=n) == -1 and final(n=n) == -1
    # the arguments of the unmasked entry points
    assert stats(pred=None) == -1 and stats(target=None) == -1 and stats(st=None) == -1 and stats(st=a + 4) == -1
    assert bwd(pred=None) == -1 and bwd(target=None) == -1 and bwd(dp=None) == -1
    assert bwd(kind=_lib.LOSS_BERHU, st=None) == -1 and bwd(kind=_lib.LOSS_BERHU, lc=None) == -1
    assert value(pred=None) == -1 and value(target=None) == -1 and value(st=None) == -1 and value(vp=None) == -1
    assert final(st=None) == -1 and final(lo=None) == -1 and final(kind=_lib.LOSS_BERHU, vp=None) == -1
    # the mask's own
    for f in (stats, bwd, value):
        assert f(c=0) == -1 and f(c=-1) == -1 and f(hw=0) == -1 and f(hw=-8) == -1
        assert f(c=3, hw=8) == -1 and f(c=1, hw=3) == -1 and f(c=2, hw=8) == -1      # n = 8 is no multiple of chans * chan_stride
        assert f(v=NAN) == -1 and f(v=INF) == -1 and f(v=-INF) == -1
        assert f(cnt=None) == -1 and f(cnt=a + 2) == -1
    assert final(cnt=None) == -1 and final(cnt=a + 1) == -1
    assert bwd(nv=None) == -1 and bwd(nv=a + 4) == -1 and final(nv=None) == -1 and final(nv=a + 4) == -1
    assert stats(n=1 << 41, hw=1 << 41) == -1                                         # a workgroup's count would not fit its uint32
    assert not any(buf)                                                                # nothing was written


# ---------------------------------------------------------------------------------------------------- 6. the launch log
HEADS = {"pixel_shuffle": dict(), "final_expanding": dict(pixel_shuffle=False, patch_unmerging=False)}
MASKED = ("tulip_loss_stats_m", "tulip_loss_bwd_m", "tulip_loss_value_m", "tulip_loss_final_m")


@functools.lru_cache(maxsize=None)
def launch_log(head, **kw):
    """forward + backward of the tiny model on a CPU-bound engine: (the log, the index of the backward's first entry)"""
    torch.manual_seed(0)
    model = tiny(**dict(HEADS[head], **kw)).train()
    eng = TulipEngine(model)
    eng.bind(torch.device("cpu"))
    g = torch.zeros(eng.params.total, dtype=torch.float32)
    with dry_run(eng, gflat=g) as dry:
        P = eng.plan(2)
        eng.run_forward(P, with_loss=True, defer_loss_final=True)
        bwd0 = len(dry.log)
        eng.run_backward(P, g, overwrite=True)
    return tuple(dry.log), bwd0, frozenset(P.bufs)


def launches(log):
    return [e for e in log if e[0] == "launch"]


@pytest.mark.parametrize("head", list(HEADS))
def test_mask_off_is_the_launch_sequence_of_a_model_without_the_keyword(head):
    for kind in L.KINDS:
        plain, b0, bufs = launch_log(head, loss=kind)
        off, b1, bufs_off = launch_log(head, loss=kind, loss_valid_min=None)
        assert b0 == b1 and len(plain) == len(off) and all(x == y for x, y in zip(plain, off))
        assert bufs == bufs_off and not {"loss_counts", "loss_valid"} & bufs                    # no new buffer
        assert not any(e[1].endswith("_m") and e[1].startswith("tulip_loss_") for e in launches(plain))
    # ... and without arguments at all
    bare, b2, _ = launch_log(head)
    l1, b3, _ = launch_log(head, loss="l1", loss_valid_min=None)
    assert b2 == b3 and bare == l1 and any(e[1].startswith("tulip_l1_loss_") or ("partials", 0) in e[3] for e in launches(bare))


@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("head", list(HEADS))
def test_masked_launch_sequence(head, kind):
    plain, pb0, _ = launch_log(head)                                   # unmasked L1: where target / partials ride in the head kernels
    log, b0, bufs = launch_log(head, loss=kind, loss_valid_min=0.0)
    L_ = launches(log)
    assert {"loss_counts", "loss_valid", "loss_stats", "loss_vpart", "loss_c"} <= bufs
    assert not any(e[1].startswith("tulip_l1_loss_") for e in L_)
    assert not any(e[1] in ("tulip_loss_stats", "tulip_loss_bwd", "tulip_loss_value", "tulip_loss_final") for e in L_)
    # the masked symbols in the order stats, bwd, (value for berHu), final
    want = [s for s in MASKED if kind == "berhu" or s != "tulip_loss_value_m"]
    assert [e[1] for e in L_ if e[1] in MASKED] == want
    at = {e[1]: i for i, e in enumerate(log) if e[0] == "launch" and e[1] in MASKED}
    assert at["tulip_loss_stats_m"] < b0 <= at["tulip_loss_bwd_m"]        # behind the head's forward / in front of its backward
    by = {e[1]: e for e in L_ if e[1] in MASKED}
    assert by["tulip_loss_stats_m"][2] == by["tulip_loss_bwd_m"][2] == "chain"
    hw = 32 * 256
    st, bw, fi = by["tulip_loss_stats_m"][3], by["tulip_loss_bwd_m"][3], by["tulip_loss_final_m"][3]
    assert st == (("pred", 0), ("target", 0), ("loss_stats", 0), 2 * hw, 1, 1, hw, 0.0, ("loss_counts", 0))
    assert bw[:4] == (_lib.LOSS_L1 + L.KINDS.index(kind), ("pred", 0), ("target", 0), ("loss_stats", 0))
    assert bw[6:] == (("dpred", 0), ("loss_c", 0), 2 * hw, 1, hw, 0.0, ("loss_counts", 0), ("loss_valid", 0))
    assert fi == (_lib.LOSS_L1 + L.KINDS.index(kind), ("loss_stats", 0), ("loss_vpart", 0), ("losses", 0), 2 * hw, 1, ("loss_counts", 0),
                  ("loss_valid", 0))
    if kind == "berhu":
        assert by["tulip_loss_value_m"][3] == (("pred", 0), ("target", 0), ("loss_stats", 0), ("loss_vpart", 0), 2 * hw, 1, hw, 0.0,
                                               ("loss_counts", 0))
    # the head kernels: where the unmasked L1 model passes target (and the forward its partials), the masked one passes NULL
    fwd_pos, bwd_pos = {}, {}
    for i, e in enumerate(plain):
        if e[0] == "launch" and not e[1].startswith("tulip_l1_loss_"):
            pos = tuple(k for k, v in enumerate(e[3]) if v in (("target", 0), ("partials", 0)))
            if pos:
                (fwd_pos if i < pb0 else bwd_pos).setdefault(e[1], pos)
    if head == "pixel_shuffle":
        assert len(fwd_pos) == 1 and len(next(iter(fwd_pos.values()))) == 2 and len(bwd_pos) >= 2     # tail forward; dgrad and wgrad
    else:
        assert not fwd_pos and not bwd_pos                                     # this head's L1 is tulip_l1_loss_fwd / _bwd
    seen = set()
    for i, e in enumerate(log):
        if e[0] != "launch":
            continue
        pos = (fwd_pos if i < b0 else bwd_pos).get(e[1])
        if pos:
            seen.add(e[1])
            assert all(e[3][k] is None for k in pos), (e[1], pos)
        if e[1] not in MASKED:
            assert ("target", 0) not in e[3] and ("partials", 0) not in e[3], e[1]
    assert seen == set(fwd_pos) | set(bwd_pos)
    if head == "pixel_shuffle":
        # ... and the backward's head kernels read dpred where they read pred
        for sym in bwd_pos:
            e_plain = next(e for e in plain[pb0:] if e[0] == "launch" and e[1] == sym)
            e_mask = next(e for e in log[b0:] if e[0] == "launch" and e[1] == sym)
            k = e_plain[3].index(("pred", 0))
            assert e_mask[3][k] == ("dpred", 0) and ("pred", 0) not in e_mask[3]

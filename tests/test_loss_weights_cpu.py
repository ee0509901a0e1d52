"""The channel weights of the training loss without a GPU, TULIP(loss_channel_weights=...): the constructor keyword and its
validation, the host definition (tulip_amd/loss.py) against autograd of torch_loss, the identities the definition promises (one
channel alone, all ones, selection, no counted element), the float32 restatements, the Trainer's checks that need no device, and
the new symbols in the header, both libraries and the bindings."""
import os
import re
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import tulip_oracle as O
from tulip_amd import _lib
from tulip_amd import loss as L
from tulip_amd.engine import TulipEngine
from tulip_amd.model import tulip as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
KINDS = ("l1", "l2", "berhu")
SHAPES = ((2, 3, 5, 7), (1, 2, 4, 4))
WEIGHTS = {3: (0.5, 0.0, 1.5), 2: (1.0, 0.25)}
NEW = {"tulip_loss_stats_w": 12, "tulip_loss_bwd_w": 17, "tulip_loss_value_w": 12, "tulip_loss_final_w": 8,
       "tulip_loss_edge_stats_w": 11, "tulip_loss_edge_bwd_w": 15, "tulip_loss_edge_final_w": 9}
same = lambda a, b: np.asarray(a).tobytes() == np.asarray(b).tobytes()


def data(shape, seed=0, holes=True):
    """seeded float64 (pred, target); channel 0 of target positive at the valid pixels and 0 or negative at about 30 % of them"""
    rng = np.random.default_rng(seed + int(np.prod(shape)))
    pred, target = rng.standard_normal(shape), rng.standard_normal(shape)
    ch0 = np.abs(target[:, 0]) + 0.25
    if holes:
        hole = rng.random(ch0.shape) < 0.3
        hole[0, 0, 0] = False
        ch0[hole] = np.where(rng.random(int(hole.sum())) < 0.5, 0.0, -1.5)
    target[:, 0] = ch0
    return pred, target


def tiny(**kw):
    cfg = O.tiny_config()
    return T.TULIP(img_size=cfg.img_size, target_img_size=cfg.target_img_size, patch_size=cfg.patch_size, embed_dim=cfg.embed_dim,
                   window_size=[2, 8], depths=cfg.depths, num_heads=cfg.num_heads, norm_layer=partial(nn.LayerNorm, eps=1e-6),
                   **dict(dict(pixel_shuffle=True, circular_padding=True, log_transform=True, patch_unmerging=True), **kw))


# ---------------------------------------------------------------------------------------------------- 1. the keyword
def test_constructor_keyword():
    m = T.TULIP(in_chans=2, loss_channel_weights=(1.0, 0.25))
    assert m.loss_channel_weights == (1.0, 0.25) and all(type(w) is float for w in m.loss_channel_weights)
    assert T.TULIP(in_chans=2).loss_channel_weights is None
    plain = tiny(in_chans=2)
    w = tiny(in_chans=2, loss="berhu", loss_valid_min=0.0, loss_edge_weight=0.5, loss_channel_weights=[np.float32(0.5), 0.0])
    assert w.loss_channel_weights == (0.5, 0.0) and w.loss == "berhu" and w.loss_valid_min == 0.0 and w.loss_edge_weight == 0.5
    assert list(w.state_dict().keys()) == list(plain.state_dict().keys())                        # the setting is not state
    with pytest.raises(AttributeError):
        w.loss_channel_weights = (1.0, 1.0)                                                       # fixed at construction
    assert tiny(loss_channel_weights=(2.0,)).loss_channel_weights == (2.0,)                       # in_chans 1: a plain scale
    for bad in ((1.0,), (1.0, 1.0, 1.0), (True, 1.0), (1, 1.0), (1.0, NAN), (INF, 1.0), (1.0, -0.5), (0.0, 0.0), 1.0, "11",
                np.ones(2), (1.0, "1")):
        with pytest.raises(ValueError, match="loss_channel_weights"):
            T.TULIP(in_chans=2, loss_channel_weights=bad)
        with pytest.raises(ValueError, match="loss_channel_weights"):
            T.tulip_base(in_chans=2, loss_channel_weights=bad)
    assert T.tulip_base(in_chans=2, loss_channel_weights=(0.0, 1.0)).loss_channel_weights == (0.0, 1.0)
    import dropin.model.tulip as D
    assert D.TULIP is T.TULIP and D.tulip_large(in_chans=3, loss_channel_weights=(1.0, 0.0, 0.5)).loss_channel_weights == (1.0, 0.0, 0.5)
    assert TulipEngine(w).loss_channel_weights == (0.5, 0.0) and TulipEngine(plain).loss_channel_weights is None

    class Foreign:                                                                                # a model object without the attribute
        pass
    eng = TulipEngine.__new__(TulipEngine)
    eng.model = Foreign()
    assert eng.loss_channel_weights is None


def test_check_channel_weights():
    assert L.check_channel_weights(None, 3) is None
    got = L.check_channel_weights([np.float64(1.0), np.float32(0.25), 0.0], 3)
    assert got == (1.0, 0.25, 0.0) and type(got) is tuple and all(type(v) is float for v in got)
    assert L.check_channel_weights((3.0,), 1) == (3.0,)
    for bad, c in (((1.0, 1.0), 3), ((), 0), ((False, 1.0), 2), ((np.bool_(True), 1.0), 2), ((2, 1.0), 2), ((NAN, 1.0), 2),
                   ((1.0, -INF), 2), ((1.0, INF), 2), ((-0.25, 1.0), 2), ((0.0, 0.0, 0.0), 3), (0.5, 1), ({0: 1.0}, 1),
                   ((None, 1.0), 2)):
        with pytest.raises(ValueError, match="loss_channel_weights"):
            L.check_channel_weights(bad, c)


# ---------------------------------------------------------------------------------------------------- 2. the definition
@pytest.mark.parametrize("edge", [0.0, 0.5])
@pytest.mark.parametrize("valid_min", [None, 0.0], ids=["unmasked", "masked"])
@pytest.mark.parametrize("kind", KINDS)
def test_definition_is_autograd_of_torch_loss(kind, valid_min, edge):
    """value and gradient in float64: (1/n_S) sum_S w_c f(d) + w_e (1/n_S) sum_S w_c (|e_h| + |e_v|) against torch_loss, the
    gradient w_c f' / n_S + w_e w_c k / n_S against its autograd.  Both are float64 evaluations of one formula: 1e-12."""
    for shape in SHAPES:
        pred, target = data(shape)
        w = WEIGHTS[shape[1]]
        S = L.counted_mask(target, valid_min, w)
        ns = int(S.sum())
        assert 0 < ns < S.size or (valid_min is None and all(v > 0 for v in w))
        expect = (S.size if valid_min is None else int(L.valid_mask(target, valid_min).sum())) // shape[1] * sum(v > 0 for v in w)
        assert ns == expect                                                                       # (n / C) * #{c: w_c > 0} without a mask
        p = torch.from_numpy(pred).requires_grad_(True)
        loss = L.torch_loss(kind, p, torch.from_numpy(target), valid_min, edge, w)
        loss.backward()
        value = L.loss_value(kind, pred, target, valid_min, w) + edge * L.edge_value(pred, target, valid_min, w)
        grad = L.loss_grad(kind, pred, target, 1.0, valid_min, w)
        grad = grad + edge * L._weights_like(target, w) * L.edge_grad_int(pred, target, valid_min, w) / ns
        np.testing.assert_allclose(loss.item(), value, rtol=1e-12, atol=0)
        np.testing.assert_allclose(p.grad.numpy(), grad, rtol=1e-10, atol=1e-15)
        assert not p.grad.numpy()[~S].any() and not grad[~S].any() and not np.signbit(grad[~S]).any()


@pytest.mark.parametrize("valid_min", [None, 0.0], ids=["unmasked", "masked"])
@pytest.mark.parametrize("kind", KINDS)
def test_one_channel_alone_all_ones_and_none(kind, valid_min):
    for shape in SHAPES:
        pred, target = data(shape, seed=1)
        C = shape[1]
        # (1, 0, ...): the single-channel loss of channel 0 -- value, gradient, pixel_loss, C, the edge term
        e0 = (1.0,) + (0.0,) * (C - 1)
        p0, t0 = pred[:, :1], target[:, :1]
        assert same(L.loss_value(kind, pred, target, valid_min, e0), L.loss_value(kind, p0, t0, valid_min))
        assert same(L.pixel_loss(pred, target, True, valid_min, e0), L.pixel_loss(p0, t0, True, valid_min))
        assert same(L.berhu_c(pred, target, valid_min, e0), L.berhu_c(p0, t0, valid_min))
        assert same(L.edge_value(pred, target, valid_min, e0), L.edge_value(p0, t0, valid_min))
        g = L.loss_grad(kind, pred, target, 0.5, valid_min, e0)
        assert same(g[:, :1], L.loss_grad(kind, p0, t0, 0.5, valid_min)) and not g[:, 1:].any()
        k = L.edge_grad_int(pred, target, valid_min, e0)
        assert np.array_equal(k[:, :1], L.edge_grad_int(p0, t0, valid_min)) and not k[:, 1:].any()
        # all ones: the call without the keyword, bit for bit; so is None
        ones = (1.0,) * C
        p32, t32 = pred.astype(np.float32), target.astype(np.float32)
        base32 = L.loss_grad32(kind, p32, t32, 0.5, valid_min)
        for cw in (ones, None):
            assert same(L.loss_value(kind, pred, target, valid_min, cw), L.loss_value(kind, pred, target, valid_min))
            assert same(L.loss_grad(kind, pred, target, 0.5, valid_min, cw), L.loss_grad(kind, pred, target, 0.5, valid_min))
            assert same(L.pixel_loss(pred, target, True, valid_min, cw), L.pixel_loss(pred, target, True, valid_min))
            assert same(L.berhu_c(pred, target, valid_min, cw), L.berhu_c(pred, target, valid_min))
            assert same(L.berhu_c32(pred, target, valid_min, cw), L.berhu_c32(pred, target, valid_min))
            assert same(L.berhu_values(pred, target, None, valid_min, cw), L.berhu_values(pred, target, None, valid_min))
            assert same(L.edge_value(pred, target, valid_min, cw), L.edge_value(pred, target, valid_min))
            assert same(L.edge_grad32(p32, t32, base32, 0.5, 0.5, valid_min, cw), L.edge_grad32(p32, t32, base32, 0.5, 0.5, valid_min))
            assert same(L.edge_total32(p32, t32, 1.25, 0.5, valid_min, cw), L.edge_total32(p32, t32, 1.25, 0.5, valid_min))
            assert same(base32, L.loss_grad32(kind, p32, t32, 0.5, valid_min, cw))
            assert same(L.loss_values32(kind, p32, t32, True, valid_min, cw), L.loss_values32(kind, p32, t32, True, valid_min))
        pt, tt = torch.from_numpy(pred), torch.from_numpy(target)
        assert same(L.torch_loss(kind, pt, tt, valid_min, 0.5, None).numpy(), L.torch_loss(kind, pt, tt, valid_min, 0.5).numpy())
        # (torch_loss sums the weighted terms in another order than the mean of the call without: the same value, not the same bits)
        np.testing.assert_allclose(L.torch_loss(kind, pt, tt, valid_min, 0.5, ones).item(), L.torch_loss(kind, pt, tt, valid_min, 0.5).item(),
                                   rtol=1e-13)


@pytest.mark.parametrize("valid_min", [None, 0.0], ids=["unmasked", "masked"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_weightless_channel_is_removed_by_selection(kind, valid_min):
    """a NaN and an infinity in pred, and in target's channels >= 1, of a w_c == 0 channel: no value and no gradient moves -- while
    channel 0 of target still decides validity with w_0 == 0"""
    pred, target = data((2, 3, 5, 7), seed=2)
    w = (0.0, 0.0, 2.0) if valid_min is not None else (0.5, 0.0, 1.5)
    off = [c for c, v in enumerate(w) if v == 0.0]
    pb, tb = pred.copy(), target.copy()
    for c in off:
        pb[:, c, ::2] = NAN
        pb[0, c, 1, 1] = INF
        if c >= 1:
            tb[:, c, :, ::3] = NAN
            tb[1, c, 1, 1] = -INF

    def everything(p, t):
        pt = torch.from_numpy(p).requires_grad_(True)
        loss = L.torch_loss(kind, pt, torch.from_numpy(t), valid_min, 0.5, w)
        loss.backward()
        p32, t32 = p.astype(np.float32), t.astype(np.float32)
        b32 = L.loss_grad32(kind, p32, t32, 1.0, valid_min, w)
        return (L.loss_value(kind, p, t, valid_min, w), L.loss_grad(kind, p, t, 1.0, valid_min, w), L.pixel_loss(p, t, True, valid_min, w),
                L.berhu_c(p, t, valid_min, w), L.edge_value(p, t, valid_min, w), L.edge_grad_int(p, t, valid_min, w), b32,
                L.edge_grad32(p32, t32, b32, 0.5, 1.0, valid_min, w), L.edge_total32(p32, t32, 1.0, 0.5, valid_min, w),
                L.loss_values32(kind, p32, t32, True, valid_min, w), loss.item(), pt.grad.numpy())
    clean, bad = everything(pred, target), everything(pb, tb)
    assert all(same(a, b) for a, b in zip(clean, bad)) and all(np.isfinite(np.asarray(a, dtype=np.float64)).all() for a in bad)
    if valid_min is not None:
        # w_0 == 0, and channel 0 of target still punches the holes: n_S = (valid pixels) * 1
        assert int(L.counted_mask(target, valid_min, w).sum()) == int(L.valid_mask(target, valid_min)[:, 0].sum())
        assert 0 < int(L.valid_mask(target, valid_min)[:, 0].sum()) < 2 * 5 * 7
    # a NaN in a counted element reaches the loss
    pn = pred.copy()
    pn.reshape(-1)[np.flatnonzero(L.counted_mask(target, valid_min, w))[0]] = NAN
    assert np.isnan(L.loss_value(kind, pn, target, valid_min, w)) and np.isnan(L.loss_values32(kind, pn, target, False, valid_min, w)[0])


@pytest.mark.parametrize("kind", KINDS)
def test_no_counted_element_gives_zeros(kind):
    pred, target = data((1, 2, 4, 4), seed=3)
    target[:, 0] = -1.0
    w = (1.0, 0.25)
    pt = torch.from_numpy(pred).requires_grad_(True)
    loss = L.torch_loss(kind, pt, torch.from_numpy(target), 0.0, 0.5, w)
    loss.backward()
    assert loss.item() == 0.0 and not pt.grad.numpy().any()
    p32, t32 = pred.astype(np.float32), target.astype(np.float32)
    zeros = (L.loss_value(kind, pred, target, 0.0, w), L.loss_grad(kind, pred, target, 1.0, 0.0, w), L.pixel_loss(pred, target, True, 0.0, w),
             L.berhu_c(pred, target, 0.0, w), L.berhu_c32(pred, target, 0.0, w), L.edge_value(pred, target, 0.0, w),
             L.edge_grad_int(pred, target, 0.0, w), L.loss_grad32(kind, p32, t32, 1.0, 0.0, w), L.loss_values32(kind, p32, t32, True, 0.0, w),
             L.edge_grad32(p32, t32, np.zeros_like(p32), 0.5, 1.0, 0.0, w), L.edge_total32(p32, t32, 0.0, 0.5, 0.0, w))
    for z in zeros:
        z = np.asarray(z, dtype=np.float64)
        assert not z.any() and not np.signbit(z).any()


@pytest.mark.parametrize("edge", [0.0, 0.5])
@pytest.mark.parametrize("valid_min", [None, 0.0], ids=["unmasked", "masked"])
@pytest.mark.parametrize("kind", KINDS)
def test_float32_restatements_agree_with_float64(kind, valid_min, edge):
    """the project's tolerances (tests/test_loss_gpu.py): rtol 1e-6 for the base gradient -- float32 inputs, so d is one rounding, then
    g, g_c, and at most four more in berHu's branch (C's product, d / C, the product with g_c; l2: 2 d is exact): seven in all,
    7 * 2^-24 = 4.2e-7 -- and 1e-5 for the losses.  The edge gradient is an integer times ge_c (four roundings) beside the base."""
    for shape in SHAPES:
        pred, target = (a.astype(np.float32) for a in data(shape, seed=4))
        w = WEIGHTS[shape[1]]
        g32 = L.loss_grad32(kind, pred, target, 0.75, valid_min, w)
        g64 = L.loss_grad(kind, pred, target, 0.75, valid_min, w)
        assert g32.dtype == np.float32
        np.testing.assert_allclose(g32, g64, rtol=1e-6, atol=0)
        S = L.counted_mask(target, valid_min, w)
        assert not g32[~S].view(np.int32).any()
        l32, pix32 = L.loss_values32(kind, pred, target, True, valid_min, w)
        np.testing.assert_allclose(l32, L.loss_value(kind, pred, target, valid_min, w), rtol=1e-5, atol=0)
        np.testing.assert_allclose(pix32, L.pixel_loss(pred, target, True, valid_min, w), rtol=1e-5, atol=0)
        if edge:
            ns = int(S.sum())
            k = L.edge_grad_int(pred, target, valid_min, w)
            assert np.array_equal(k, L._edge_k(*L._edge_diff(pred, target, valid_min, np.float32, w), L._responses))
            e32 = L.edge_grad32(pred, target, np.zeros_like(pred), edge, 0.75, valid_min, w)
            np.testing.assert_allclose(e32, 0.75 * edge * L._weights_like(target, w) * k / ns, rtol=1e-6, atol=0)
            edge32, total32 = L.edge_total32(pred, target, l32, edge, valid_min, w)
            np.testing.assert_allclose(edge32, L.edge_value(pred, target, valid_min, w), rtol=1e-5, atol=0)
            np.testing.assert_allclose(total32, L.loss_value(kind, pred, target, valid_min, w) + edge * L.edge_value(pred, target, valid_min, w),
                                       rtol=1e-5, atol=0)


# ---------------------------------------------------------------------------------------------------- 3. the Trainer, without a device
def test_trainer_refuses_sharded_before_it_touches_the_device():
    from tulip_amd.trainer import Trainer

    class M:
        loss = "l1"
        loss_valid_min = None
        loss_edge_weight = 0.0
        in_chans = 2
        loss_channel_weights = (1.0, 0.25)
    with pytest.raises(ValueError, match="sharded.*loss_channel_weights|loss_channel_weights.*sharded"):
        Trainer(M(), 2, exchange="sharded")
    M.loss_channel_weights = (1.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="loss_channel_weights"):
        Trainer(M(), 2)


def test_trainer_reports_a_state_saved_under_other_weights(capsys):
    """load_state_dict's check alone, on a stand-in (the rest of it needs the device): the key missing counts as None"""
    from tulip_amd.trainer import Trainer

    class Stand:
        _loss_channel_weights = (1.0, 0.25)
    assert not Trainer._report_saved_channel_weights(Stand(), {"loss_channel_weights": (1.0, 0.25)}) and capsys.readouterr().err == ""
    assert not Trainer._report_saved_channel_weights(Stand(), {"loss_channel_weights": [1.0, 0.25]})
    assert Trainer._report_saved_channel_weights(Stand(), {"loss_channel_weights": (1.0, 0.5)})
    err = capsys.readouterr().err
    assert "loss_channel_weights=(1.0, 0.5)" in err and "(1.0, 0.25)" in err
    assert Trainer._report_saved_channel_weights(Stand(), {})                                     # saved before the keyword existed
    assert "loss_channel_weights=None" in capsys.readouterr().err
    Stand._loss_channel_weights = None
    assert not Trainer._report_saved_channel_weights(Stand(), {}) and capsys.readouterr().err == ""
    assert Trainer._report_saved_channel_weights(Stand(), {"loss_channel_weights": (1.0, 0.5)})
    import inspect
    assert "_report_saved_channel_weights(sd)" in inspect.getsource(Trainer.load_state_dict)


# ---------------------------------------------------------------------------------------------------- 4. library, bindings
def test_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "tulip_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, f"{name} is not declared in include/tulip_hip.h"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs == len(_lib.SIGNATURES[name]), name
        assert args[-1].startswith("hipStream_t")
        if "final" not in name:                                                                    # the weights travel by value: a host array
            assert all(any(a.endswith(w) for a in args) for w in ("int chans", "const float* weights", "int masked", "float valid_min")), name
        if name not in ("tulip_loss_stats_w", "tulip_loss_edge_stats_w"):
            assert any(a.endswith("const uint32_t* counts") for a in args), name
    from tulip_amd.csrc.build import build
    build(force=False, verbose=False)
    lib = _lib.load()
    with _lib.dev_library() as dev:
        assert dev is not lib
        for name in NEW:
            assert getattr(lib, name) is not None and getattr(dev, name) is not None
    from tulip_amd import ops
    for name in NEW:
        assert callable(getattr(ops, name[len("tulip_"):]))

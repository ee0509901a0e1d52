"""The channel weights of the training loss on the GPU, TULIP(loss_channel_weights=...): the _w entry points of csrc/loss.hip against
the host definition (tulip_amd/loss.py) -- dpred, C and n_S bit for bit against the float32 restatement, the losses at the sums'
tolerance and bit for bit where every sum is exact; all-ones weights against the unweighted entry points, bit for bit; selection (a
non-finite value in a w_c == 0 channel moves no bit); plane isolation; the argument checks; the model's loss and gradients against
the oracle's autograd of the same definition; and the Trainer's step forms.  Tolerances are those of tests/test_loss_gpu.py."""
import math

import numpy as np
import pytest
import torch

import test_loss_edge_gpu as E
import test_loss_gpu as G
import test_loss_mask_gpu as M
from oracle import tulip_oracle as O
from tulip_amd import _lib, ops
from tulip_amd import loss as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN, INF = float("nan"), float("inf")
KINDS = ("l1", "l2", "berhu")
VMIN = 0.0
EDGE = 0.5
bits = G.bits
# (B, C, H, W).  One pixel per channel; chan_stride 35: the scalar route, a channel boundary inside a thread's four elements; two
# float4 shapes (chan_stride % 4 == 0); three workgroups and a column past the 128-wide edge tile; a second tile row and column;
# 1025 groups of 1024 elements: the grid capped at TULIP_LOSS_BLOCKS_MAX, the stride loop across the channel boundary
SHAPES = ((1, 2, 1, 1), (2, 3, 5, 7), (1, 2, 4, 4), (2, 4, 3, 8), (1, 2, 8, 130), (1, 3, 9, 129), (1, 2, 16, 32800))
# every weight a power of two, one channel switched off in all but the first.  (The four-channel tuple is this file's: the feature's
# description names weights for two and three channels only.)
WEIGHTS = {2: ((1.0, 0.25), (0.0, 2.0)), 3: ((0.5, 0.0, 1.0),), 4: ((1.0, 0.0, 0.5, 2.0),)}
CASES = [(s, w) for s in SHAPES for w in WEIGHTS[s[1]]]
ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def make(shape, what, masked, weights=None, seed=0):
    """(pred, target) in float32.  randn: seeded normal values; int: integer-valued with d = pred - target in [-3, 3] and one d = 5 at
    the first counted element, so that berHu's C = fl32(fl32(0.2) * 5) is 1.0 exactly and every value, (a^2 + 1) / 2, a multiple of
    one half.  masked: channel 0 of target is positive at the valid pixels and 0 or negative at about 30 % of them."""
    rng = np.random.default_rng(100 * seed + int(np.prod(shape)) + shape[-1])
    if what == "int":
        target = rng.integers(-2, 3, shape).astype(np.float32)
        d = rng.integers(-3, 4, shape).astype(np.float32)
    else:
        target, d = rng.standard_normal(shape).astype(np.float32), None
    if masked:
        hole = rng.random((shape[0],) + shape[2:]) < 0.3
        hole[0, 0, 0] = False
        ch0 = np.abs(target[:, 0]) + np.float32(1.0 if what == "int" else 0.25)
        ch0[hole] = np.where(rng.random(int(hole.sum())) < 0.5, 0.0, -1.5).astype(np.float32)
        target[:, 0] = ch0
    if what == "int":
        if weights is not None:
            first = np.flatnonzero(L.counted_mask(target, VMIN if masked else None, weights))[0]
            d.reshape(-1)[first] = 5.0
        pred = target + d
    else:
        pred = rng.standard_normal(shape).astype(np.float32)
    return pred, target


def bufs():
    z = lambda n: torch.zeros(n, dtype=torch.float32, device=DEV)
    return dict(stats=z(4 * _lib.LOSS_BLOCKS_MAX), vpart=z(_lib.LOSS_BLOCKS_MAX), c=z(1), losses=z(2),
                counts=torch.full((_lib.LOSS_BLOCKS_MAX,), 12345, dtype=torch.int32, device=DEV),
                nv_bwd=torch.full((1,), -7, dtype=torch.int64, device=DEV), nv_fin=torch.full((1,), -7, dtype=torch.int64, device=DEV),
                epart=z(_lib.LOSS_BLOCKS_MAX), edge=z(1))


def run_w(kind, p_h, t_h, weights, valid_min=None, edge=0.0, log_transform=0, gscale_dev=None, gscale=1.0):
    """the step's launch order through the _w entry points: stats -> bwd (-> edge bwd) -> value (berhu) -> final (-> edge stats ->
    edge final); (dpred, losses, C, n_S of bwd, n_S of final, edge term) on the host"""
    B, C, H, W = p_h.shape
    n = p_h.size
    pred, target = torch.from_numpy(p_h).to(DEV), torch.from_numpy(t_h).to(DEV)
    dpred = torch.full_like(pred, 7.0)
    b = bufs()
    a = (C, H * W, weights, valid_min)
    ops.loss_stats_w(pred, target, b["stats"], n, log_transform, *a, b["counts"])
    ops.loss_bwd_w(kind, pred, target, b["stats"], gscale_dev, gscale, dpred, b["c"], n, *a, b["counts"], b["nv_bwd"])
    if edge:
        ops.loss_edge_bwd_w(pred, target, gscale_dev, gscale, edge, dpred, B * C, H, W, C, weights, valid_min, b["counts"])
    if kind == "berhu":
        ops.loss_value_w(pred, target, b["stats"], b["vpart"], n, *a, b["counts"])
    ops.loss_final_w(kind, b["stats"], b["vpart"], b["losses"], n, b["counts"], b["nv_fin"])
    if edge:
        ops.loss_edge_stats_w(pred, target, b["epart"], B * C, H, W, C, weights, valid_min)
        ops.loss_edge_final_w(b["epart"], b["edge"], b["losses"], edge, B * C, H, W, b["counts"])
    torch.cuda.synchronize()
    return (dpred.cpu().numpy(), b["losses"].cpu().numpy(), b["c"].cpu().numpy()[0], int(b["nv_bwd"].item()), int(b["nv_fin"].item()),
            b["edge"].cpu().numpy()[0])


def run_plain(kind, p_h, t_h, valid_min=None, edge=0.0, log_transform=0, gscale=1.0):
    """the same through the entry points without weights (unmasked, or _m)"""
    B, C, H, W = p_h.shape
    n = p_h.size
    pred, target = torch.from_numpy(p_h).to(DEV), torch.from_numpy(t_h).to(DEV)
    dpred = torch.full_like(pred, 7.0)
    b = bufs()
    if valid_min is None:
        ekw = {}
        ops.loss_stats(pred, target, b["stats"], n, log_transform)
        ops.loss_bwd(kind, pred, target, b["stats"], None, gscale, dpred, b["c"], n)
    else:
        mask = (C, H * W, valid_min)
        ekw = dict(mask=(C, valid_min), counts=b["counts"])
        ops.loss_stats_m(pred, target, b["stats"], n, log_transform, *mask, b["counts"])
        ops.loss_bwd_m(kind, pred, target, b["stats"], None, gscale, dpred, b["c"], n, *mask, b["counts"], b["nv_bwd"])
    if edge:
        ops.loss_edge_bwd(pred, target, None, gscale, edge, dpred, B * C, H, W, **ekw)
    if valid_min is None:
        if kind == "berhu":
            ops.loss_value(pred, target, b["stats"], b["vpart"], n)
        ops.loss_final(kind, b["stats"], b["vpart"], b["losses"], n, log_transform)
    else:
        if kind == "berhu":
            ops.loss_value_m(pred, target, b["stats"], b["vpart"], n, *mask, b["counts"])
        ops.loss_final_m(kind, b["stats"], b["vpart"], b["losses"], n, log_transform, b["counts"], b["nv_fin"])
    if edge:
        ops.loss_edge_stats(pred, target, b["epart"], B * C, H, W, **ekw)
        ops.loss_edge_final(b["epart"], b["edge"], b["losses"], edge, B * C, H, W, **ekw)
    torch.cuda.synchronize()
    return dpred.cpu().numpy(), b["losses"].cpu().numpy(), b["c"].cpu().numpy()[0], b["edge"].cpu().numpy()[0]


def want_dpred(kind, p_h, t_h, weights, vm, edge, gscale=1.0):
    base = L.loss_grad32(kind, p_h, t_h, gscale, vm, weights)
    return L.edge_grad32(p_h, t_h, base, edge, gscale, vm, weights) if edge else base


# ---------------------------------------------------------------------------------------------------- 1. kernels vs the definition
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("shape,weights", CASES, ids=ids)
def test_kernels_match_the_host_definition(shape, weights, masked):
    """every kind, edge term off and on.  dpred, C: the float32 restatement's bits; n_valid: n_S; the losses at rtol 1e-5 on randn
    input (the sums' tolerance of tests/test_loss_gpu.py) and the restatement's bits on integer input, where every weight is a power
    of two and every sum exact."""
    vm = VMIN if masked else None
    for what in ("randn", "int"):
        p_h, t_h = make(shape, what, masked, weights)
        S = L.counted_mask(t_h, vm, weights)
        ns = int(S.sum())
        assert 0 < ns <= S.size
        for kind in KINDS:
            for edge in (0.0, EDGE):
                dpred, losses, c, nv_b, nv_f, e = run_w(kind, p_h, t_h, weights, vm, edge)
                tag = f"{shape} {weights} masked={masked} {what} {kind} edge={edge}"
                print(f"{tag}: losses {losses.tolist()} C {c!r} n_S {nv_b} of {S.size} edge {e!r}")
                assert nv_b == nv_f == ns, tag
                assert np.array_equal(bits(dpred), bits(want_dpred(kind, p_h, t_h, weights, vm, edge))), tag
                assert not bits(dpred[~S]).any(), tag                                     # +0.0 off S
                if kind == "berhu":
                    assert bits(c) == bits(L.berhu_c32(p_h, t_h, vm, weights)), tag
                l32, pix32 = L.loss_values32(kind, p_h, t_h, False, vm, weights)
                if what == "int":
                    assert kind != "berhu" or c == 1.0
                    want_e, want_t = L.edge_total32(p_h, t_h, l32, edge, vm, weights) if edge else (np.float32(0.0), l32)
                    assert bits(losses[0]) == bits(want_t) and bits(losses[1]) == bits(pix32) and bits(e) == bits(want_e), tag
                else:
                    ev = L.edge_value(p_h, t_h, vm, weights) if edge else 0.0
                    np.testing.assert_allclose(losses[0], L.loss_value(kind, p_h, t_h, vm, weights) + edge * ev, rtol=1e-5, atol=0)
                    np.testing.assert_allclose(losses[1], L.pixel_loss(p_h, t_h, False, vm, weights), rtol=1e-5, atol=0)
                    np.testing.assert_allclose(e, ev, rtol=1e-5, atol=0)
    # log_transform moves losses[1] only; gscale from device memory and as an argument: the host's bits
    p_h, t_h = make(shape, "randn", masked, weights)
    ref = run_w("berhu", p_h, t_h, weights, vm, EDGE)
    gl = run_w("berhu", p_h, t_h, weights, vm, EDGE, log_transform=1)
    np.testing.assert_allclose(gl[1][1], L.pixel_loss(p_h, t_h, True, vm, weights), rtol=1e-5, atol=0)
    assert np.array_equal(bits(gl[0]), bits(ref[0])) and bits(gl[1][0]) == bits(ref[1][0]) and bits(gl[2]) == bits(ref[2])
    gdev = torch.full((1,), 0.3, dtype=torch.float32, device=DEV)
    ga, gb = run_w("l2", p_h, t_h, weights, vm, EDGE, gscale_dev=gdev, gscale=9.0), run_w("l2", p_h, t_h, weights, vm, EDGE, gscale=0.3)
    assert np.array_equal(bits(ga[0]), bits(gb[0])) and np.array_equal(bits(ga[0]), bits(want_dpred("l2", p_h, t_h, weights, vm, EDGE, 0.3)))


# ---------------------------------------------------------------------------------------------------- 2. all ones: the kernels without
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_all_ones_are_the_unweighted_entry_points_bits(shape, masked):
    """randn input, every kind, with the edge term: dpred, both losses, C and the edge value of the _w entry points with every weight
    1.0 are those of the entry points without weights (unmasked: tulip_loss_*, masked: the _m forms), bit for bit -- every product
    with 1.0 is exact and every thread sums the elements it sums there."""
    vm = VMIN if masked else None
    p_h, t_h = make(shape, "randn", masked)
    ones = (1.0,) * shape[1]
    for kind in KINDS:
        for lt in (0, 1):
            dpred, losses, c, nv_b, _, e = run_w(kind, p_h, t_h, ones, vm, EDGE, log_transform=lt)
            d0, l0, c0, e0 = run_plain(kind, p_h, t_h, vm, EDGE, log_transform=lt)
            tag = f"{shape} masked={masked} {kind} log_transform={lt}: losses {losses.tolist()} / {l0.tolist()} edge {e!r} / {e0!r}"
            print(tag)
            assert nv_b == int(L.valid_mask(t_h, vm).sum())
            assert np.array_equal(bits(dpred), bits(d0)), tag
            assert np.array_equal(bits(losses), bits(l0)) and bits(c) == bits(c0) and bits(e) == bits(e0), tag


# ---------------------------------------------------------------------------------------------------- 3. selection
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("shape,weights", [((1, 2, 8, 130), (0.0, 2.0)), ((2, 3, 5, 7), (0.5, 0.0, 1.0)), ((2, 4, 3, 8), (1.0, 0.0, 0.5, 2.0))],
                         ids=ids)
def test_a_nonfinite_value_in_a_weightless_channel_moves_no_bit(shape, weights, masked):
    """NaNs and infinities in pred of every w_c == 0 channel and in target of those with c >= 1 (channel 0 of target decides validity
    whatever w_0 is): every output is the clean run's, bit for bit.  A NaN in a counted element reaches losses[0]."""
    vm = VMIN if masked else None
    p_h, t_h = make(shape, "randn", masked, weights)
    off = [c for c, w in enumerate(weights) if w == 0.0]
    p_b, t_b = p_h.copy(), t_h.copy()
    for c in off:
        p_b[:, c].reshape(-1)[::3] = NAN
        p_b[-1, c, -1, -1] = INF
        p_b[0, c, 0, 0] = -INF
        if c >= 1:
            t_b[:, c].reshape(-1)[1::2] = NAN
            t_b[0, c, -1, 0] = INF
    assert not np.isfinite(p_b).all()
    S = L.counted_mask(t_h, vm, weights)
    assert np.array_equal(S, L.counted_mask(t_b, vm, weights))
    for kind in KINDS:
        clean, bad = run_w(kind, p_h, t_h, weights, vm, EDGE), run_w(kind, p_b, t_b, weights, vm, EDGE)
        assert np.isfinite(bad[0]).all() and np.isfinite(bad[1]).all()
        assert E.same((clean[0], clean[1], clean[2], clean[5]), (bad[0], bad[1], bad[2], bad[5])) and clean[3:5] == bad[3:5], kind
        p_n = p_h.copy()
        p_n.reshape(-1)[np.flatnonzero(S)[-1]] = NAN
        got = run_w(kind, p_n, t_h, weights, vm, EDGE)
        assert math.isnan(got[1][0]) and math.isnan(got[1][1]), kind


# ---------------------------------------------------------------------------------------------------- 4. plane isolation
@pytest.mark.parametrize("plane", [(0, 0), (0, 2), (1, 0)])
def test_an_impulse_stays_in_its_plane(plane):
    """d = one 1 at the last pixel of plane (b, c) of a (2, 3, 9, 129) batch with weights (0.5, 0.0, 1.0): dpred is 0 in every other
    plane and sample, and +0.0 -- the sign bit clear -- in the w_c == 0 planes, which an impulse of their own does not change."""
    shape, weights = (2, 3, 9, 129), (0.5, 0.0, 1.0)
    b, c = plane
    t_h = np.zeros(shape, dtype=np.float32)
    p_h = t_h.copy()
    p_h[b, c, -1, -1] = 1.0
    p_h[:, 1, -1, -1] = -1.0                                                                      # ... in the weightless planes
    for kind in KINDS:
        dpred, losses, _, nv, _, e = run_w(kind, p_h, t_h, weights, None, EDGE)
        assert nv == 2 * 2 * 9 * 129
        assert np.array_equal(bits(dpred), bits(want_dpred(kind, p_h, t_h, weights, None, EDGE)))
        others = np.ones(shape, dtype=bool)
        others[b, c] = False
        assert not dpred[others].any() and dpred[b, c].any()
        assert not bits(dpred[:, 1]).any()
        # three neighbours respond with |e_h| + |e_v| = 2 each, times the plane's weight
        assert bits(e) == bits(np.float32(np.float64(np.float32(weights[c]) * 6.0) * (1.0 / nv)))


# ---------------------------------------------------------------------------------------------------- 5. the argument checks
def test_bad_arguments_return_err_arg():
    x = torch.zeros(4096, dtype=torch.float32, device=DEV)
    cnt = torch.zeros(_lib.LOSS_BLOCKS_MAX, dtype=torch.int32, device=DEV)
    nv = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = torch.full((4096,), 3.0, dtype=torch.float32, device=DEV)
    good = (2, 16, (1.0, 0.25), None)
    bad = [(0, 16, (), None), (5, 4, (1.0,) * 5, None), (2, 16, None, None), (2, 16, (1.0, -0.5), None), (2, 16, (1.0, NAN), None),
           (2, 16, (INF, 1.0), None), (2, 16, (0.0, 0.0), None), (2, 15, (1.0, 0.25), None), (2, 16, (1.0, 0.25), NAN)]
    for a in bad:
        with pytest.raises(_lib.TulipHipError, match="TULIP_ERR_ARG"):
            ops.loss_stats_w(x, x, out, 32, 0, *a, cnt)
        with pytest.raises(_lib.TulipHipError, match="TULIP_ERR_ARG"):
            ops.loss_bwd_w("l2", x, x, x, None, 1.0, out, x, 32, *a, cnt, nv)
        with pytest.raises(_lib.TulipHipError, match="TULIP_ERR_ARG"):
            ops.loss_value_w(x, x, x, out, 32, *a, cnt)
        if a[0] * a[1] == 32:
            with pytest.raises(_lib.TulipHipError, match="TULIP_ERR_ARG"):
                ops.loss_edge_stats_w(x, x, out, 2, 4, 4, a[0], a[2], a[3])
            with pytest.raises(_lib.TulipHipError, match="TULIP_ERR_ARG"):
                ops.loss_edge_bwd_w(x, x, None, 1.0, 0.5, out, 2, 4, 4, a[0], a[2], a[3], cnt)
    for call in (lambda: ops.loss_bwd_w(7, x, x, x, None, 1.0, out, x, 32, *good, cnt, nv),               # the cases of the _m forms
                 lambda: ops.loss_stats_w(x, x, out, 0, 0, *good, cnt),
                 lambda: ops.loss_stats_w(x, x, out, 32, 0, *good, None),
                 lambda: ops.loss_stats_w(None, x, out, 32, 0, *good, cnt),
                 lambda: ops.loss_bwd_w("l2", x, x, x, None, 1.0, out, x, 32, *good, cnt, None),
                 lambda: ops.loss_final_w("l2", x, x, out, 32, None, nv),
                 lambda: ops.loss_final_w("l2", x, x, out, 32, cnt, None),
                 lambda: ops.loss_edge_bwd_w(x, x, None, 1.0, -0.5, out, 2, 4, 4, 2, (1.0, 0.25), None, cnt),
                 lambda: ops.loss_edge_bwd_w(x, x, None, 1.0, 0.5, out, 2, 4, 4, 2, (1.0, 0.25), None, None),
                 lambda: ops.loss_edge_bwd_w(x, x, None, 1.0, 0.5, out, 3, 4, 4, 2, (1.0, 0.25), None, cnt),
                 lambda: ops.loss_edge_final_w(x, out, out, 0.5, 2, 4, 4, None)):
        with pytest.raises(_lib.TulipHipError, match="TULIP_ERR_ARG"):
            call()
    torch.cuda.synchronize()
    assert (out == 3.0).all().item() and not cnt.any().item() and not nv.any().item() and not x.any().item()


# ---------------------------------------------------------------------------------------------------- 6. model vs the oracle
CASE, CW = "in_chans2", (1.0, 0.25)
MODEL = [("l1", False, 0.0), ("berhu", True, EDGE)]
_oracle_cache = {}


def oracle_grads(kind, masked, edge, lowp):
    """(loss, {name: grad}) of the oracle's forward with torch_loss(..., channel_weights=) by autograd; computed once"""
    key = (kind, masked, edge, lowp)
    if key not in _oracle_cache:
        cfg, sd, lo, hi = E.case_data(CASE, masked)
        leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
        full = dict(sd)
        full.update(leaves)
        pred = O.tulip_forward(full, cfg, lo, None, lowp=lowp)
        loss = L.torch_loss(kind, pred, hi, valid_min=VMIN if masked else None, edge_weight=edge, channel_weights=CW)
        loss.backward()
        _oracle_cache[key] = (loss.item(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()})
    return _oracle_cache[key]


def model_kw(masked, edge, weights=CW):
    kw = dict(loss_channel_weights=weights) if weights != "absent" else {}
    if masked:
        kw["loss_valid_min"] = VMIN
    if edge:
        kw["loss_edge_weight"] = edge
    return kw


def device_grads(kind, masked, edge):
    cfg, sd, lo, hi = E.case_data(CASE, masked)
    m = M.build(cfg, sd, kind, **model_kw(masked, edge))
    pred, loss, pix = m(lo.to(DEV), hi.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    P = m.engine().plan(lo.shape[0])
    return m, P, pred.detach().cpu(), loss.item(), pix.item(), {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("kind,masked,edge", MODEL, ids=lambda v: str(v))
def test_model_loss_and_gradients_vs_oracle(kind, masked, edge):
    """model(lo, hi) and loss.backward() with loss_channel_weights=(1.0, 0.25) on the two-channel model against the oracle's autograd
    of torch_loss(..., channel_weights=), at the tolerances of tests/test_loss_edge_gpu.py's test of the same name: loss 1e-3
    relative; gradient rel_l2 1e-2 against the low-precision oracle and 1.5e-2 against the fp32 one -- with the edge term, twice the
    recorded OWN_LOWP figure of this case there (bias tables 5e-2 and 1e-1).  The read-outs are the host values for the device's own
    pred; the no-grad forward returns the same total."""
    rel_l2 = G.rel_l2
    ol, og = oracle_grads(kind, masked, edge, False)
    _, olp = oracle_grads(kind, masked, edge, True)
    m, P, pred, loss, pix, g = device_grads(kind, masked, edge)
    cfg, sd, lo, hi = E.case_data(CASE, masked)
    vm = VMIN if masked else None
    worst = max((rel_l2(g[n], og[n]), n) for n in g if not n.endswith("relative_position_bias_table"))
    worst_lp = max((rel_l2(g[n], olp[n]), n) for n in g if not n.endswith("relative_position_bias_table"))
    print(f"{kind} masked={masked} edge={edge}: loss {loss!r} oracle {ol!r} (rel {abs(loss - ol) / ol:.2e}); worst rel_l2 vs fp32 {worst}, "
          f"vs lowp {worst_lp}")
    assert abs(loss - ol) <= 1e-3 * ol
    p_h, t_h = pred.numpy(), hi.numpy()
    np.testing.assert_allclose(pix, L.pixel_loss(p_h, t_h, cfg.log_transform, vm, CW), rtol=1e-5)
    ev = L.edge_value(p_h, t_h, vm, CW) if edge else 0.0
    np.testing.assert_allclose(loss, L.loss_value(kind, p_h, t_h, vm, CW) + edge * ev, rtol=2e-5)
    assert int(P.loss_valid.item()) == int(L.counted_mask(t_h, vm, CW).sum())
    if edge:
        np.testing.assert_allclose(P.loss_edge.item(), ev, rtol=1e-5)
    if kind == "berhu":
        assert bits(P.loss_c.cpu().numpy()[0]) == bits(L.berhu_c32(p_h, t_h, vm, CW))
    bound = 2 * E.OWN_LOWP[CASE, kind, masked] if edge else 1.5e-2
    for n in g:
        table = n.endswith("relative_position_bias_table")
        assert rel_l2(g[n], og[n]) <= (1e-1 if table else bound), n
        assert rel_l2(g[n], olp[n]) <= (5e-2 if table else 1.0e-2), n
    with torch.no_grad():
        _, loss_n, pix_n = m(lo.to(DEV), hi.to(DEV))
    assert bits(loss_n.item()) == bits(loss) and bits(pix_n.item()) == bits(pix)
    # the weights do something: another loss than the model without them returns for the same input
    m0 = M.build(cfg, sd, kind, **model_kw(masked, edge, "absent"))
    with torch.no_grad():
        _, loss_0, _ = m0(lo.to(DEV), hi.to(DEV))
    assert abs(loss_0.item() - loss) > 1e-2 * loss


# ---------------------------------------------------------------------------------------------------- 7. Trainer
def trainer_run(loss, steps=3, batch=2, model_kw={}, **kw):
    from tulip_amd.trainer import Trainer
    cfg = O.tiny_config(drop_path_rate=0.0, in_chans=2)
    sd = O.key_seeded_state_dict(cfg, seed=3)
    m = M.build(cfg, sd, loss, train=True, **model_kw)
    tr = Trainer(m, batch, lr=5e-4, **kw)
    lo, hi = (t.to(DEV) for t in O.synthetic_batch(cfg, batch, seed=77))
    tr.load_batch(lo, hi)
    losses = [tr.step().clone() for _ in range(steps)]
    torch.cuda.synchronize()
    return tr, torch.stack(losses).cpu().numpy(), tr.eng.params.flat.clone().cpu().numpy(), (lo, hi)


@pytest.mark.parametrize("kind,masked,edge", MODEL, ids=lambda v: str(v))
def test_trainer_graph_and_eager_steps_are_bit_identical(kind, masked, edge):
    mk = model_kw(masked, edge)
    tr_g, lg, pg, (lo, hi) = trainer_run(kind, model_kw=mk, use_graph=True)
    tr_e, le, pe, _ = trainer_run(kind, model_kw=mk, use_graph=False)
    print(f"{kind} masked={masked} edge={edge} weighted trainer losses", lg.tolist())
    assert np.isfinite(lg).all() and lg[-1, 0] < lg[0, 0]
    assert np.array_equal(bits(lg), bits(le)) and np.array_equal(bits(pg), bits(pe))
    vm = VMIN if masked else None
    pred, target = tr_g.P.pred.cpu().numpy(), hi.cpu().numpy()
    ev = L.edge_value(pred, target, vm, CW) if edge else 0.0
    np.testing.assert_allclose(lg[-1, 0], L.loss_value(kind, pred, target, vm, CW) + edge * ev, rtol=2e-5)
    assert int(tr_g.loss_valid.item()) == int(L.counted_mask(target, vm, CW).sum())
    assert tr_g.loss_channel_weights == CW and tr_g.eng.loss_channel_weights == CW and tr_g.state_dict()["loss_channel_weights"] == CW
    # another trajectory than without the weights
    _, l0, p0, _ = trainer_run(kind, model_kw=model_kw(masked, edge, "absent"), use_graph=True)
    assert not np.array_equal(bits(l0[:, 0]), bits(lg[:, 0])) and not np.array_equal(bits(p0), bits(pg))


def test_trainer_accumulation_runs():
    for use_graph in (True, False):
        tr, la, pa, _ = trainer_run("l1", steps=4, accum_iter=2, use_graph=use_graph, model_kw=model_kw(False, EDGE))
        assert np.isfinite(la).all() and np.isfinite(pa).all()
        assert bits(la[0, 0]) == bits(la[1, 0]) and la[2, 0] < la[0, 0]


@pytest.mark.parametrize("kind", ["l1", "berhu"])
def test_none_is_the_step_without_the_keyword_and_all_ones_its_parameters(kind):
    tr_a, la, pa, _ = trainer_run(kind, steps=2, model_kw=dict(loss_channel_weights=None), use_graph=True)
    tr_b, lb, pb, _ = trainer_run(kind, steps=2, use_graph=True)
    assert np.array_equal(bits(la), bits(lb)) and np.array_equal(bits(pa), bits(pb))
    assert set(tr_a.P.bufs) == set(tr_b.P.bufs) and "loss_channel_weights" not in tr_a.state_dict()
    assert tr_a.loss_channel_weights is None and tr_a.eng.loss_channel_weights is None
    # (1.0, 1.0): every product with a weight is exact, so the gradient -- for "l1" formed in front of the head instead of inside
    # it -- and with it the parameters after two steps are those of the step without the keyword
    tr_1, l1, p1, _ = trainer_run(kind, steps=2, model_kw=dict(loss_channel_weights=(1.0, 1.0)), use_graph=True)
    print(kind, "all ones", l1.tolist(), "without", lb.tolist(), "parameters differ at", int((bits(p1) != bits(pb)).sum()))
    assert np.array_equal(bits(p1), bits(pb))
    np.testing.assert_allclose(l1, lb, rtol=1e-5)
    if kind == "berhu":
        assert np.array_equal(bits(l1), bits(lb))                                                 # the same kernels' reduction orders
    assert "loss_counts" in tr_1.P.bufs and "loss_counts" not in tr_b.P.bufs


def test_trainer_state_dict_round_trip_and_report(capsys):
    tr, _, p, _ = trainer_run("l2", steps=1, model_kw=dict(loss_channel_weights=CW), use_graph=False)
    sd = tr.state_dict()
    assert sd["loss_channel_weights"] == CW
    tr2, _, _, _ = trainer_run("l2", steps=1, model_kw=dict(loss_channel_weights=CW), use_graph=False)
    capsys.readouterr()
    tr2.load_state_dict(sd)
    assert "loss_channel_weights" not in capsys.readouterr().err and tr2.state_dict()["loss_channel_weights"] == CW
    other, _, _, _ = trainer_run("l2", steps=1, model_kw=dict(loss_channel_weights=(0.0, 1.0)), use_graph=False)
    other.load_state_dict(sd)
    err = capsys.readouterr().err
    assert "loss_channel_weights=(1.0, 0.25)" in err and "(0.0, 1.0)" in err and other.loss_channel_weights == (0.0, 1.0)
    plain, _, _, _ = trainer_run("l2", steps=1, use_graph=False)
    plain.load_state_dict(sd)
    assert "loss_channel_weights=(1.0, 0.25)" in capsys.readouterr().err and plain.loss_channel_weights is None
    from tulip_amd.trainer import Trainer
    with pytest.raises(ValueError, match="sharded"):
        Trainer(tr.model, 2, exchange="sharded")


@pytest.mark.parametrize("use_graph", [True, False])
def test_trainer_skips_a_nan_in_a_counted_target_only(use_graph):
    """skip_nonfinite with weights (1.0, 0.0): a NaN in channel 1 of the target -- not counted -- costs no step; one in channel 0 --
    every pixel is valid, so it is counted -- reaches the loss and the norm, and the step is dropped."""
    tr, _, _, (lo, hi) = trainer_run("l2", steps=2, use_graph=use_graph, skip_nonfinite=True, model_kw=dict(loss_channel_weights=(1.0, 0.0)))
    assert int(tr.last_step_skipped.item()) == 0 and tr.applied_steps == 2
    before = tr.eng.params.flat.clone()
    aux = hi.clone()
    aux[1, 1, 5, 9] = NAN
    aux[0, 1, 0, 0] = INF
    losses = tr.step(lo, aux).clone()
    torch.cuda.synchronize()
    assert int(tr.last_step_skipped.item()) == 0 and tr.applied_steps == 3 and math.isfinite(losses[0].item())
    assert not torch.equal(tr.eng.params.flat.view(torch.int32), before.view(torch.int32))
    before = tr.eng.params.flat.clone()
    bad = hi.clone()
    bad[1, 0, 5, 9] = NAN
    losses = tr.step(lo, bad).clone()
    torch.cuda.synchronize()
    assert int(tr.last_step_skipped.item()) != 0 and tr.applied_steps == 3 and tr.skipped_steps == 1
    assert math.isnan(losses[0].item())
    assert torch.equal(tr.eng.params.flat.view(torch.int32), before.view(torch.int32))
    losses = tr.step(lo, hi).clone()
    torch.cuda.synchronize()
    assert int(tr.last_step_skipped.item()) == 0 and tr.applied_steps == 4 and math.isfinite(losses[0].item())
    assert torch.isfinite(tr.eng.params.flat).all().item()

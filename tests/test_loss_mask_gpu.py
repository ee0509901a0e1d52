"""The masked training loss on the GPU, TULIP(loss_valid_min=...): the four _m kernels of csrc/loss.hip against the host definition
(tulip_amd/loss.py) on flat (B, C, HW) buffers, the model's loss and parameter gradients against the oracle's autograd of the same
definition, that invalid pixels carry nothing, the Trainer's step forms, and that the mask switched off is today's step.
Everything on the tiny model (8x256 -> 32x256, depths (2, 2), embed_dim 48).  Tolerances are those of tests/test_loss_gpu.py."""
import math

import numpy as np
import pytest
import torch

import test_loss_gpu as G
from oracle import tulip_oracle as O
from tulip_amd import _lib, ops
from tulip_amd import loss as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN, INF = float("nan"), float("inf")
KINDS = ("l1", "l2", "berhu")
VMIN = 0.0
PEAK = G.PEAK                    # 12.0: above every |randn - randn| difference of these sizes
# (B, C, HW): one element; a tail with no float4 group; one short of / one past a workgroup's 256 lanes; HW % 4 != 0 at C > 1 (the
# scalar route); float4 groups whose channel-0 look-ups cross channels and samples; more than 1024 workgroups' worth of float4
# groups (grid-stride) plus a tail
SHAPES = ((1, 1, 1), (1, 1, 3), (1, 1, 255), (1, 1, 257), (1, 2, 257), (2, 3, 260), (1, 1, 1024 * 256 * 4 + 260))
VARIANT_SHAPES = ((2, 3, 260), (1, 1, 257))
bits = G.bits


def bufs():
    z = lambda n: torch.zeros(n, dtype=torch.float32, device=DEV)
    return dict(stats=z(4 * _lib.LOSS_BLOCKS_MAX), vpart=z(_lib.LOSS_BLOCKS_MAX), c=z(1), losses=z(2),
                counts=torch.full((_lib.LOSS_BLOCKS_MAX,), 12345, dtype=torch.int32, device=DEV),
                nv_bwd=torch.full((1,), -7, dtype=torch.int64, device=DEV), nv_fin=torch.full((1,), -7, dtype=torch.int64, device=DEV))


def inputs(shape, variant="seeded", seed=0):
    """seeded fp32 randn (pred, target) of shape (B, C, HW).  Channel 0 of target decides: |randn| + 0.25 at the valid pixels, 0 or
    a negative value at the invalid ones (about 30 % of them, seeded).  The variants:
        all_valid / none_valid / last_only   every pixel / no pixel / only the last pixel of the last sample valid
        peak_invalid                          the largest |d| (PEAK) planted at an invalid pixel, in the last channel
        nonfinite_invalid                     a NaN in pred and in target channels >= 1 at invalid pixels (an infinity too), and a NaN in
                                              target channel 0 (which makes that pixel invalid)"""
    B, C, HW = shape
    rng = np.random.default_rng(1000 * seed + B * C * HW + 7 * C)
    pred, target = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    hole = rng.random((B, HW)) < 0.3
    if variant == "all_valid":
        hole[:] = False
    elif variant == "none_valid":
        hole[:] = True
    elif variant == "last_only":
        hole[:] = True
        hole[-1, -1] = False
    elif variant in ("peak_invalid", "nonfinite_invalid"):
        hole[0, HW // 2] = True
        hole[-1, HW - 1] = True
        hole[0, 0] = False
    ch0 = np.abs(target[:, 0]) + np.float32(0.25)
    ch0[hole] = np.where(rng.random(int(hole.sum())) < 0.5, 0.0, -1.5).astype(np.float32)
    target[:, 0] = ch0
    if variant == "peak_invalid":
        pred[0, C - 1, HW // 2] = target[0, C - 1, HW // 2] + np.float32(PEAK)
        assert int(np.argmax(np.abs(pred - target))) == np.ravel_multi_index((0, C - 1, HW // 2), shape)
    if variant == "nonfinite_invalid":
        pred[0, :, HW // 2] = NAN
        pred[-1, 0, HW - 1] = INF
        if C > 1:
            target[0, 1:, HW // 2] = NAN
            target[-1, C - 1, HW - 1] = -INF
        target[0, 0, 0] = NAN                                   # was valid: a NaN range is no return
        pred[0, C - 1, 0] = NAN                                 # ... so this one is ignored as well
    return pred, target


def run(kind, pred, target, log_transform=0, gscale_dev=None, gscale=1.0, b=None, dpred=None):
    """the step's launch order: stats -> bwd -> value (berhu) -> final; (dpred, losses, C, n_v of bwd, n_v of final) on the host"""
    b = b or bufs()
    B, C, HW = target.shape
    n = pred.numel()
    dpred = torch.full_like(pred, 7.0) if dpred is None else dpred
    mask = (C, HW, VMIN)
    ops.loss_stats_m(pred, target, b["stats"], n, log_transform, *mask, b["counts"])
    ops.loss_bwd_m(kind, pred, target, b["stats"], gscale_dev, gscale, dpred, b["c"], n, *mask, b["counts"], b["nv_bwd"])
    if kind == "berhu":
        ops.loss_value_m(pred, target, b["stats"], b["vpart"], n, *mask, b["counts"])
    ops.loss_final_m(kind, b["stats"], b["vpart"], b["losses"], n, log_transform, b["counts"], b["nv_fin"])
    torch.cuda.synchronize()
    return dpred.cpu().numpy(), b["losses"].cpu().numpy(), b["c"].cpu().numpy()[0], int(b["nv_bwd"].item()), int(b["nv_fin"].item())


def check_against_definition(kind, p_h, t_h, got, log_transform=False, gscale=1.0):
    """dpred elementwise at rtol 1e-6 (exact zeros where the definition has them), +0 bits at the invalid elements, both losses at
    rtol 1e-5, C the float32 product's bits, n_v exact"""
    dpred, losses, c, nv_b, nv_f = got
    m = L.valid_mask(t_h, VMIN)
    want_g = L.loss_grad(kind, p_h, t_h, gscale, valid_min=VMIN)
    np.testing.assert_allclose(dpred, want_g, rtol=1e-6, atol=0)
    assert not bits(dpred[~m]).any()                                           # +0.0, not -0.0
    np.testing.assert_allclose(losses[0], L.loss_value(kind, p_h, t_h, valid_min=VMIN), rtol=1e-5, atol=0)
    np.testing.assert_allclose(losses[1], L.pixel_loss(p_h, t_h, log_transform, valid_min=VMIN), rtol=1e-5, atol=0)
    assert nv_b == nv_f == int(m.sum())
    if kind == "berhu":
        assert bits(c) == bits(L.berhu_c32(p_h, t_h, valid_min=VMIN)), (c, L.berhu_c32(p_h, t_h, valid_min=VMIN))
    return m


# ---------------------------------------------------------------------------------------------------- 1. kernels vs the definition
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_kernels_match_the_host_definition(kind, shape):
    p_h, t_h = inputs(shape)
    pred, target = torch.from_numpy(p_h).to(DEV), torch.from_numpy(t_h).to(DEV)
    got = run(kind, pred, target)
    dpred, losses, c, nv, _ = got
    print(f"{kind} {shape}: losses {losses.tolist()} C {c!r} n_v {nv} of {p_h.size}")
    m = check_against_definition(kind, p_h, t_h, got)
    assert shape[2] < 255 or 0 < nv < p_h.size
    # gscale from device memory and as an argument, 0.25 (a power of two: the same roundings, a quarter of the value)
    gdev = torch.full((1,), 0.25, dtype=torch.float32, device=DEV)
    for kw in (dict(gscale_dev=gdev, gscale=123.0), dict(gscale=0.25)):
        gq = run(kind, pred, target, **kw)
        check_against_definition(kind, p_h, t_h, gq, gscale=0.25)
        assert np.array_equal(bits(gq[0]), bits(np.float32(0.25) * dpred)) and np.array_equal(bits(gq[1]), bits(losses))
    # log_transform changes losses[1] only
    gl = run(kind, pred, target, log_transform=1)
    check_against_definition(kind, p_h, t_h, gl, log_transform=True)
    assert np.array_equal(bits(gl[0]), bits(dpred)) and bits(gl[1][0]) == bits(losses[0]) and bits(gl[2]) == bits(c)
    # the same bits run to run
    g2 = run(kind, pred, target)
    assert np.array_equal(bits(g2[0]), bits(dpred)) and np.array_equal(bits(g2[1]), bits(losses)) and bits(g2[2]) == bits(c)
    assert g2[3:] == got[3:]


@pytest.mark.parametrize("variant", ["all_valid", "none_valid", "last_only", "peak_invalid", "nonfinite_invalid"])
@pytest.mark.parametrize("shape", VARIANT_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_mask_variants(kind, shape, variant):
    p_h, t_h = inputs(shape, variant, seed=2)
    pred, target = torch.from_numpy(p_h).to(DEV), torch.from_numpy(t_h).to(DEV)
    n = p_h.size
    got = run(kind, pred, target, log_transform=1)
    dpred, losses, c, nv, _ = got
    print(f"{kind} {shape} {variant}: losses {losses.tolist()} C {c!r} n_v {nv} of {n}")
    check_against_definition(kind, p_h, t_h, got, log_transform=True)
    assert np.isfinite(dpred).all() and np.isfinite(losses).all() and math.isfinite(c)
    if variant == "all_valid":
        # every element counts: dpred and C are the unmasked entry points' bits
        b = bufs()
        want_d = torch.full_like(pred, 7.0)
        ops.loss_stats(pred, target, b["stats"], n, 1)
        ops.loss_bwd(kind, pred, target, b["stats"], None, 1.0, want_d, b["c"], n)
        if kind == "berhu":
            ops.loss_value(pred, target, b["stats"], b["vpart"], n)
        ops.loss_final(kind, b["stats"], b["vpart"], b["losses"], n, 1)
        torch.cuda.synchronize()
        assert nv == n
        assert np.array_equal(bits(dpred), bits(want_d.cpu().numpy())) and bits(c) == bits(b["c"].cpu().numpy()[0])
        np.testing.assert_allclose(losses, b["losses"].cpu().numpy(), rtol=1e-5, atol=0)
    elif variant == "none_valid":
        assert nv == 0 and not bits(dpred).any() and not bits(losses).any() and bits(c) == 0
    elif variant == "last_only":
        assert nv == shape[1] and dpred.reshape(shape)[-1, :, -1].all() and np.count_nonzero(dpred) == shape[1]
    elif variant == "peak_invalid":
        # the maximum is masked: the unmasked call's C is 0.2f * PEAK, the masked one 0.2f * the valid maximum
        b = bufs()
        ops.loss_stats(pred, target, b["stats"], n, 0)
        ops.loss_bwd("berhu", pred, target, b["stats"], None, 1.0, torch.empty_like(pred), b["c"], n)
        torch.cuda.synchronize()
        assert bits(b["c"].cpu().numpy()[0]) == bits(np.float32(0.2) * np.float32(PEAK))
        valid_max = np.abs(p_h - t_h)[L.valid_mask(t_h, VMIN)].max()
        assert valid_max < 10.0
        if kind == "berhu":
            assert bits(c) == bits(np.float32(0.2) * np.float32(valid_max)) and c < 2.0
    else:
        # the same inputs with finite values at those places: the same bits
        q_h, u_h = p_h.copy(), t_h.copy()
        m = L.valid_mask(t_h, VMIN)
        q_h[~m] = 0.5
        keep0 = u_h[:, 0].copy()
        u_h[~m] = -0.75
        u_h[:, 0] = np.where(np.isnan(keep0), -1.0, keep0)
        assert np.isfinite(q_h).all() and np.isfinite(u_h).all() and np.array_equal(L.valid_mask(u_h, VMIN), m)
        clean = run(kind, torch.from_numpy(q_h).to(DEV), torch.from_numpy(u_h).to(DEV), log_transform=1)
        assert np.array_equal(bits(clean[0]), bits(dpred)) and np.array_equal(bits(clean[1]), bits(losses))
        assert bits(clean[2]) == bits(c) and clean[3:] == got[3:]


@pytest.mark.parametrize("shape", VARIANT_SHAPES + ((1, 2, 1028),), ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_unaligned_pointers_take_the_scalar_route(kind, shape):
    """pred / target / dpred one float past a 16-byte boundary: no float4 access, the same dpred bits as the aligned call, nothing
    written outside dpred."""
    p_h, t_h = inputs(shape, seed=3)
    n = p_h.size
    pred, target = torch.from_numpy(p_h).to(DEV), torch.from_numpy(t_h).to(DEV)
    want = run(kind, pred, target, log_transform=1)
    check_against_definition(kind, p_h, t_h, want, log_transform=True)
    hold = [torch.zeros(n + 8, dtype=torch.float32, device=DEV) for _ in range(3)]
    po, to, do = (h[1:1 + n].view(shape) for h in hold)
    assert po.data_ptr() % 16 == 4 and to.data_ptr() % 16 == 4 and do.data_ptr() % 16 == 4
    po.copy_(pred)
    to.copy_(target)
    got = run(kind, po, to, log_transform=1, dpred=do)
    check_against_definition(kind, p_h, t_h, got, log_transform=True)          # (another partition of the sums)
    assert np.array_equal(bits(got[0]), bits(want[0])) and bits(got[2]) == bits(want[2]) and got[3:] == want[3:]
    assert hold[2][0].item() == 0.0 and not hold[2][1 + n:].any().item()       # nothing written outside dpred


# ---------------------------------------------------------------------------------------------------- 2. model vs the oracle
SECTOR = 64                      # columns [0, SECTOR) of every row have no return: a blind sector


def masked_case(case):
    cfg, sd, lo, hi = G.model_case(case)
    hi = hi.clone()
    hi[:, 0, :, :SECTOR] = 0.0
    return cfg, sd, lo, hi


_oracle_cache = {}


def oracle_grads(case, kind, lowp, valid_min):
    """(loss, {name: grad}, pixel_loss) of the oracle's forward with torch_loss(..., valid_min=) by autograd; computed once"""
    key = (case, kind, lowp, valid_min)
    if key not in _oracle_cache:
        cfg, sd, lo, hi = masked_case(case)
        leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
        full = dict(sd)
        full.update(leaves)
        pred = O.tulip_forward(full, cfg, lo, None, lowp=lowp)
        loss = L.torch_loss(kind, pred, hi, valid_min=valid_min)
        loss.backward()
        _oracle_cache[key] = (loss.item(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()},
                              L.pixel_loss(pred.detach().numpy(), hi.numpy(), cfg.log_transform, valid_min=valid_min))
    return _oracle_cache[key]


def build(cfg, sd, loss, train=False, **mask):
    from functools import partial
    import torch.nn as nn
    from tulip_amd.model import tulip as T
    kw = {} if loss is None else dict(loss=loss)
    m = T.TULIP(img_size=cfg.img_size, target_img_size=cfg.target_img_size, patch_size=cfg.patch_size, in_chans=cfg.in_chans,
                embed_dim=cfg.embed_dim, window_size=list(cfg.window_size), depths=cfg.depths, num_heads=cfg.num_heads,
                mlp_ratio=cfg.mlp_ratio, drop_path_rate=cfg.drop_path_rate, norm_layer=partial(nn.LayerNorm, eps=cfg.ln_eps),
                pixel_shuffle=cfg.pixel_shuffle, circular_padding=cfg.circular_padding, log_transform=cfg.log_transform,
                patch_unmerging=cfg.patch_unmerging, **kw, **mask)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    m.train(train)
    return m


def device_grads(cfg, sd, lo, hi, kind, valid_min=VMIN):
    m = build(cfg, sd, kind, loss_valid_min=valid_min)
    pred, loss, pix = m(lo.to(DEV), hi.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    P = m.engine().plan(lo.shape[0])
    return (P, pred.detach().cpu(), loss.detach().cpu().numpy(), pix.detach().cpu().numpy(),
            {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()})


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", list(G.MODEL_CASES))
def test_model_loss_and_gradients_vs_oracle(case, kind):
    """model(lo, hi) and loss.backward() with loss_valid_min=0.0 against the oracle's autograd of torch_loss(..., valid_min=0.0), at
    the tolerances of tests/test_loss_gpu.py: loss and pixel_loss 1e-3 relative, gradient rel_l2 1.5e-2 against the fp32 oracle and
    1e-2 against the low-precision one (bias tables 1e-1 and 5e-2); loss_valid is the host count.  The oracle alone tells masked
    from unmasked by more than three times the tolerance applied, in the loss and in decoder_pred.weight's gradient."""
    rel_l2 = G.rel_l2
    ol, og, opix = oracle_grads(case, kind, False, VMIN)
    _, olp, _ = oracle_grads(case, kind, True, VMIN)
    ul, ug, _ = oracle_grads(case, kind, False, None)
    sep_loss, sep_grad = abs(ul - ol) / ol, rel_l2(ug["decoder_pred.weight"], og["decoder_pred.weight"])
    cfg, sd, lo, hi = masked_case(case)
    P, pred, loss, pix, g = device_grads(cfg, sd, lo, hi, kind)
    loss, pix = float(loss), float(pix)
    worst = max((rel_l2(g[n], og[n]), n) for n in g if not n.endswith("relative_position_bias_table"))
    worst_lp = max((rel_l2(g[n], olp[n]), n) for n in g if not n.endswith("relative_position_bias_table"))
    print(f"{case} {kind}: loss {loss!r} oracle {ol!r} (rel {abs(loss - ol) / ol:.2e}); pixel {pix!r} oracle {opix!r}; worst rel_l2 vs "
          f"fp32 {worst}, vs lowp {worst_lp}; masked vs unmasked oracle: loss {sep_loss:.3f}, decoder_pred.weight {sep_grad:.3f}")
    assert sep_loss > 3 * 1e-3 and sep_grad > 3 * 1.5e-2
    assert abs(loss - ol) <= 1e-3 * ol
    assert abs(pix - opix) <= 1e-3 * opix
    for n in g:
        table = n.endswith("relative_position_bias_table")
        assert rel_l2(g[n], og[n]) <= (1e-1 if table else 1.5e-2), n
        assert rel_l2(g[n], olp[n]) <= (5e-2 if table else 1.0e-2), n
    m_h = L.valid_mask(hi.numpy(), VMIN)
    assert int(P.loss_valid.item()) == int(m_h.sum()) < hi.numel() * (1 - SECTOR / 256)
    if kind == "berhu":                                  # C as the backward formed it from this forward's pred, on the device
        assert bits(P.loss_c.cpu().numpy()[0]) == bits(L.berhu_c32(pred.numpy(), hi.numpy(), valid_min=VMIN))


def test_no_grad_forward_returns_the_masked_loss():
    """model(x, target) under no_grad (the evaluation call): the losses of the differentiable call, and n_v from the final fold"""
    case, kind = "in_chans2", "berhu"
    cfg, sd, lo, hi = masked_case(case)
    m = build(cfg, sd, kind, loss_valid_min=VMIN)
    with torch.no_grad():
        _, loss, pix = m(lo.to(DEV), hi.to(DEV))
    torch.cuda.synchronize()
    assert int(m.engine().plan(lo.shape[0]).loss_valid.item()) == int(L.valid_mask(hi.numpy(), VMIN).sum())
    _, _, loss_g, pix_g, _ = device_grads(cfg, sd, lo, hi, kind)
    assert bits(loss.item()) == bits(loss_g) and bits(pix.item()) == bits(pix_g)
    ol, _, _ = oracle_grads(case, kind, False, VMIN)
    assert abs(loss.item() - ol) <= 1e-3 * ol


# ---------------------------------------------------------------------------------------------------- 3. invalid pixels carry nothing
@pytest.mark.parametrize("kind", KINDS)
def test_invalid_pixels_carry_nothing(kind):
    """in_chans == 2: whatever channel 1 of the target holds at the invalid pixels -- other finite values, a NaN -- the loss and
    every parameter gradient keep their bits."""
    cfg, sd, lo, hi = masked_case("in_chans2")
    hole = ~(hi[:, 0] > VMIN)
    assert 0.25 < hole.float().mean().item() < 0.5 and (hi[:, 1][hole] != 0).any()
    _, _, loss, pix, g = device_grads(cfg, sd, lo, hi, kind)
    assert math.isfinite(float(loss))
    for fill in (3.5, -2.0, NAN, INF):
        other = hi.clone()
        other[:, 1][hole] = fill
        P, _, loss2, pix2, g2 = device_grads(cfg, sd, lo, other, kind)
        assert bits(loss2) == bits(loss) and bits(pix2) == bits(pix), fill
        for n in g:
            assert torch.equal(g[n].view(torch.int32), g2[n].view(torch.int32)), (fill, n)
        dp = P.dpred.view(torch.int32).cpu()
        assert not dp[:, 0][hole].any().item() and not dp[:, 1][hole].any().item() and dp[:, 1][~hole].any().item()


# ---------------------------------------------------------------------------------------------------- 4. Trainer
def trainer_run(loss, steps=3, batch=2, mask=(), cfg_kw={}, **kw):
    """mask: () -- the model built without the keyword; (v,) -- built with loss_valid_min=v"""
    from tulip_amd.trainer import Trainer
    cfg = O.tiny_config(drop_path_rate=0.0, **cfg_kw)
    sd = O.key_seeded_state_dict(cfg, seed=3)
    m = build(cfg, sd, loss, train=True, **(dict(loss_valid_min=mask[0]) if mask else {}))
    tr = Trainer(m, batch, lr=5e-4, **kw)
    lo, hi = (t.to(DEV) for t in O.synthetic_batch(cfg, batch, seed=77))
    tr.load_batch(lo, hi)
    losses = [tr.step().clone() for _ in range(steps)]
    torch.cuda.synchronize()
    return tr, torch.stack(losses).cpu().numpy(), tr.eng.params.flat.clone().cpu().numpy(), (lo, hi)


@pytest.mark.parametrize("kind", ["l1", "berhu"])
def test_trainer_graph_and_eager_steps_are_bit_identical(kind):
    tr_g, lg, pg, (lo, hi) = trainer_run(kind, mask=(VMIN,), use_graph=True)
    tr_e, le, pe, _ = trainer_run(kind, mask=(VMIN,), use_graph=False)
    print(f"masked {kind} trainer losses", lg.tolist(), "n_v", tr_g.loss_valid.item())
    assert np.isfinite(lg).all() and lg[-1, 0] < lg[0, 0]
    assert np.array_equal(bits(lg), bits(le)) and np.array_equal(bits(pg), bits(pe))
    want_nv = int((hi[:, 0] > VMIN).sum().item()) * hi.shape[1]
    assert tr_g.loss_valid.dtype == torch.int64 and tr_g.loss_valid.item() == tr_e.loss_valid.item() == want_nv < hi.numel()
    if kind == "berhu":
        assert bits(tr_g.loss_c.item()) == bits(tr_e.loss_c.item()) and tr_g.loss_c.item() > 0.0
    else:
        with pytest.raises(AttributeError):
            tr_g.loss_c
    # ... and the masked loss is not the unmasked one
    tr_u, lu, pu, _ = trainer_run(kind, use_graph=True)
    assert not np.array_equal(bits(lu[:, 0]), bits(lg[:, 0])) and not np.array_equal(bits(pu), bits(pg))
    with pytest.raises(AttributeError):
        tr_u.loss_valid
    assert not any("valid" in str(k) for k in tr_g.state_dict())           # the setting is the model's, not the Trainer's state


def test_trainer_final_expanding_head_two_channels():
    """The other head (its masked read-out goes beside the chain too) at in_chans == 2: the step forms agree bit for bit, and the first
    step's losses are the module path's for the same weights and batch."""
    cfg_kw = dict(pixel_shuffle=False, in_chans=2)
    tr_g, lg, pg, (lo, hi) = trainer_run("l2", mask=(VMIN,), cfg_kw=cfg_kw, use_graph=True)
    tr_e, le, pe, _ = trainer_run("l2", mask=(VMIN,), cfg_kw=cfg_kw, use_graph=False)
    assert np.isfinite(lg).all() and lg[-1, 0] < lg[0, 0]
    assert np.array_equal(bits(lg), bits(le)) and np.array_equal(bits(pg), bits(pe))
    assert tr_g.loss_valid.item() == tr_e.loss_valid.item() == 2 * int((hi[:, 0] > VMIN).sum().item()) < hi.numel()
    cfg = O.tiny_config(drop_path_rate=0.0, **cfg_kw)
    m = build(cfg, O.key_seeded_state_dict(cfg, seed=3), "l2", train=True, loss_valid_min=VMIN)
    _, loss, pix = m(lo, hi)
    assert bits(loss.item()) == bits(lg[0, 0]) and bits(pix.item()) == bits(lg[0, 1])


@pytest.mark.parametrize("use_graph", [True, False])
def test_trainer_accumulation_clipping_and_ema_run(use_graph):
    for kind in ("l1", "berhu"):
        tr, la, pa, _ = trainer_run(kind, steps=4, mask=(VMIN,), accum_iter=2, use_graph=use_graph)
        assert np.isfinite(la).all() and np.isfinite(pa).all()
        # the resident batch twice per optimizer step: both micro-steps of the first window report the same loss
        assert bits(la[0, 0]) == bits(la[1, 0]) and la[2, 0] < la[0, 0]
    tr, lc, pc, _ = trainer_run("l2", mask=(VMIN,), clip_grad=0.05, ema_decay=0.9, use_graph=use_graph)
    _, ln, pn, _ = trainer_run("l2", mask=(VMIN,), use_graph=use_graph)
    assert np.isfinite(lc).all() and np.isfinite(pc).all() and lc[-1, 0] < lc[0, 0]
    assert np.array_equal(bits(lc[0]), bits(ln[0]))                         # the first step's losses: the same forward


@pytest.mark.parametrize("use_graph", [True, False])
def test_a_nan_in_a_target_pixel_costs_no_step(use_graph):
    """skip_nonfinite with a masked berHu loss: the NaN in target[1, 0, 5, 9] is not a valid pixel, so the step is taken -- where the
    unmasked berHu model skips it (tests/test_loss_gpu.py::test_trainer_skips_a_nonfinite_target)."""
    tr, _, _, (lo, hi) = trainer_run("berhu", steps=2, mask=(VMIN,), use_graph=use_graph, skip_nonfinite=True)
    assert hi[1, 0, 5, 9].item() > VMIN                                    # a valid pixel of the clean batch
    nv = int(tr.loss_valid.item())
    assert int(tr.last_step_skipped.item()) == 0 and tr.applied_steps == 2
    before = tr.eng.params.flat.clone()
    bad = hi.clone()
    bad[1, 0, 5, 9] = NAN
    losses = tr.step(lo, bad).clone()
    torch.cuda.synchronize()
    assert int(tr.last_step_skipped.item()) == 0 and tr.applied_steps == 3 and tr.skipped_steps == 0
    assert math.isfinite(losses[0].item()) and math.isfinite(losses[1].item()) and math.isfinite(tr.loss_c.item())
    assert int(tr.loss_valid.item()) == nv - 1
    assert not torch.equal(tr.eng.params.flat.view(torch.int32), before.view(torch.int32))
    assert torch.isfinite(tr.eng.params.flat).all().item()
    # the same batch on the unmasked berHu model is skipped
    tu, _, _, _ = trainer_run("berhu", steps=1, use_graph=use_graph, skip_nonfinite=True)
    before = tu.eng.params.flat.clone()
    losses = tu.step(lo, bad).clone()
    torch.cuda.synchronize()
    assert int(tu.last_step_skipped.item()) != 0 and math.isnan(losses[0].item())
    assert torch.equal(tu.eng.params.flat.view(torch.int32), before.view(torch.int32))


# ---------------------------------------------------------------------------------------------------- 5. off is off
@pytest.mark.parametrize("kind", KINDS)
def test_off_is_off(kind):
    _, la, pa, (lo, hi) = trainer_run(kind, use_graph=True)
    _, lb, pb, _ = trainer_run(kind, mask=(None,), use_graph=True)
    assert np.array_equal(bits(la), bits(lb)) and np.array_equal(bits(pa), bits(pb))
    if kind != "l1":
        # a threshold below every target value: the masked kernels with every element valid step to the unmasked parameters
        assert hi.min().item() > -1.0
        tr, lc, pc, _ = trainer_run(kind, mask=(-1.0,), use_graph=True)
        assert np.array_equal(bits(pa), bits(pc))
        np.testing.assert_allclose(lc, la, rtol=1e-5)
        assert tr.loss_valid.item() == hi.numel()

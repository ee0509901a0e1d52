"""GPU: upscale_factor 8 -- 16-pixel patches (2, 8) and (4, 4).

  1. the head family at r = 8 against fp32 autograd of O.ps_head_and_pred: the shapes, checks and tolerances of
     test_inchans_gpu.test_head_family_multichannel / test_head_with_norm_up_and_loss_multichannel, at in_chans 1, 2, 4;
  2. the r-carrying entry points at r = 4 against the old symbols, bit for bit;
  3. FinalPatchExpanding at P = 8 through the engine against the oracle, and expand_norm at P = 8 (bands of
     test_inchans_gpu.test_expand_norm_multichannel);
  4. the model against the reference fixture g17_upscale (bands of test_windows_gpu.test_model_vs_reference_fixture);
  5. KITTI tulip_base at patch_size (2, 8), batch 8, against the fp32 oracle (bands of
     test_model_gpu.test_kitti_base_full_size_gradients_vs_oracle);
  6. bit-identity: two Trainers from one state (captured against eager, accum_iter 2, dropout 0.1), GraphedForward against the
     module forward;
  7. TULIP() with the constructor defaults at full size through the module path.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from oracle import tulip_oracle as O
from tulip_amd import _lib, ops
from tests import upscale_cases as UC

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
R8 = 8


def bf(t):
    return t.to(torch.bfloat16).contiguous()


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def close(a, b, rtol, atol_scale, what=""):
    a, b = a.float(), b.float()
    scale = b.abs().max().item() + 1e-30
    err = (a - b).abs()
    bad = err > rtol * b.abs() + atol_scale * scale
    assert not bad.any(), (f"{what}: {bad.sum().item()}/{bad.numel()} out of tolerance; max err "
                           f"{err.max().item():.4e} (scale {scale:.3e})")


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def head_cfg(B, H, W, E, nch, **kw):
    """a config whose upscale_factor is 8 on an H x W token grid of (2, 8) patches"""
    cfg = O.TulipConfig(img_size=(2 * H, 8 * W), target_img_size=(8 * H, 8 * W), patch_size=(2, 8), embed_dim=E, in_chans=nch, **kw)
    assert cfg.upscale_factor == 8 and cfg.grid == (H, W)
    return cfg


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("nch", [1, 2, 4])
@pytest.mark.parametrize("B,H,W,E", [(2, 8, 64, 48), (1, 3, 24, 96), (3, 16, 64, 96)])
@pytest.mark.parametrize("l1", [False, True])
def test_head_family_r8(nch, B, H, W, E, l1):
    """tail_fwd / tail_bwd / tail_bwd_dgrad / tail_wgrad at r = 8 against autograd of ps_head_and_pred; every output buffer is
    pre-filled with NaN, so an unwritten pixel, row or slab element fails"""
    M, NE = B * H * W, 64 * E
    cfg = head_cfg(B, H, W, E, nch)
    xn = bf(rnd(M, E))
    We, be, wd = bf(rnd(NE, E, scale=0.1, seed=1)), rnd(NE, scale=0.1, seed=2), rnd(nch, E, scale=0.2, seed=3)
    sd = {"ps_head.conv_expand.0.weight": We.float().reshape(NE, E, 1, 1).requires_grad_(True),
          "ps_head.conv_expand.0.bias": be.clone().requires_grad_(True),
          "decoder_pred.weight": wd.reshape(nch, E, 1, 1).clone().requires_grad_(True)}
    xr = xn.float().reshape(B, H, W, E).requires_grad_(True)
    ref = O.ps_head_and_pred(O._Prec(False), sd, cfg, xr)
    assert tuple(ref.shape) == (B, nch, 8 * H, 8 * W)
    pred = torch.full((B, nch, 8 * H, 8 * W), float("nan"), device=DEV)
    ops.tail_fwd(xn, We, be, wd, pred, B, H, W, E, in_chans=nch, r=R8)
    close(pred, ref, 1e-4, 2e-5, "tail fwd")
    if l1:
        target = rnd(B, nch, 8 * H, 8 * W, seed=8)
        (3.0 * (ref - target).abs().mean()).backward()
        kw = dict(target=target, gscale=3.0, in_chans=nch, r=R8)
        dsrc = pred
    else:
        dsrc = rnd(B, nch, 8 * H, 8 * W, seed=4)
        ref.backward(dsrc)
        kw = dict(in_chans=nch, r=R8)
    R = (M + 31) // 32
    dxn = torch.full((M, E), float("nan"), dtype=torch.bfloat16, device=DEV)
    dpart = torch.full((R, nch * 128), float("nan"), device=DEV)
    ops.tail_bwd_dgrad(xn, We, be, wd, dsrc, dxn, dpart, B, H, W, E, **kw)
    sp = ops.tail_wgrad_splits(B, H, W, E, nch, R8)
    assert sp >= 1
    sw = torch.full((sp, NE * E), float("nan"), device=DEV)
    sb = torch.full((sp, NE), float("nan"), device=DEV)
    ops.tail_wgrad(xn, We, be, wd, dsrc, sw, sb, B, H, W, E, **kw)
    dwd = torch.zeros(nch, E, device=DEV)
    for k in range(nch):
        ops.reduce_rows2(dpart[:, 128 * k:], nch * 128, dwd[k], E, None, 0, None, 0, R)
    dWe, dbe = torch.zeros(NE * E, device=DEV), torch.zeros(NE, device=DEV)
    ops.reduce_rows_multi([ops.reduce_region(sw, NE * E, dWe, NE * E, sp), ops.reduce_region(sb, NE, dbe, NE, sp)])
    torch.cuda.synchronize()
    gwd = sd["decoder_pred.weight"].grad.reshape(nch, E)
    close(dwd, gwd, 1e-3, 1e-4 * max(1.0, float(dwd.abs().max())), "tail dwd")
    for got, want, what in [(dxn.float(), xr.grad.reshape(M, E), "dxn"),
                            (dWe.reshape(NE, E), sd["ps_head.conv_expand.0.weight"].grad.reshape(NE, E), "dWe"),
                            (dbe, sd["ps_head.conv_expand.0.bias"].grad, "dbe")]:
        assert torch.isfinite(got).all(), what
        err = (got - want).abs().max().item() / max(want.abs().max().item(), 1e-30)
        rl2 = ((got - want).norm() / want.norm()).item()
        print(f"r8 head nch {nch} {(B, H, W, E)} l1 {l1} {what}: max {err:.3e} rel-L2 {rl2:.3e}")
        assert err <= 1e-2 and rl2 <= 6e-3, (what, err, rl2)
    # the dz-materialising form: the same decoder_pred partial rows, dz through its consumers
    dz = torch.full((M, NE), float("nan"), dtype=torch.bfloat16, device=DEV)
    dpart2 = torch.full_like(dpart, float("nan"))
    ops.tail_bwd(xn, We, be, wd, dsrc, dz, dpart2, B, H, W, E, **kw)
    torch.cuda.synchronize()
    assert (dpart2 - dpart).abs().max().item() <= 2e-6 * max(dpart2.abs().max().item(), 1e-30)
    dzf = dz.float()
    assert torch.isfinite(dzf).all()
    close(dzf.sum(0), sd["ps_head.conv_expand.0.bias"].grad, 2e-2, 4e-3, "tail_bwd dbe (colsum dz)")
    close(dzf @ We.float(), xr.grad.reshape(M, E), 2e-2, 4e-3, "tail_bwd dxn (dz.We)")


@pytest.mark.parametrize("nch", [1, 2, 4])
@pytest.mark.parametrize("log_transform", [True, False])
def test_head_with_norm_up_and_loss_r8(nch, log_transform):
    """tail_fwd_ln (loss partials) and tail_bwd_dgrad_ln at r = 8 against the oracle"""
    B, H, W, E = 2, 8, 64, 96
    M, R, NE = B * H * W, (B * H * W + 31) // 32, 64 * E
    cfg = head_cfg(B, H, W, E, nch, log_transform=log_transform)
    x = rnd(M, E, seed=11)
    gam, bet = 1.0 + 0.1 * rnd(E, seed=12), 0.1 * rnd(E, seed=13)
    We, be, wd = bf(rnd(NE, E, scale=0.1, seed=1)), rnd(NE, scale=0.1, seed=2), rnd(nch, E, scale=0.2, seed=3)
    target = 0.3 * rnd(B, nch, 8 * H, 8 * W, seed=8)
    eps = 1e-6
    xn = torch.full((M, E), float("nan"), dtype=torch.bfloat16, device=DEV)
    mean, rstd = torch.full((M,), float("nan"), device=DEV), torch.full((M,), float("nan"), device=DEV)
    pred = torch.full((B, nch, 8 * H, 8 * W), float("nan"), device=DEV)
    parts, losses = torch.full((2 * R,), float("nan"), device=DEV), torch.empty(2, device=DEV)
    ops.tail_fwd_ln(x, gam, bet, eps, xn, mean, rstd, We, be, wd, pred, B, H, W, E, target=target, loss_partials=parts,
                    log_transform=log_transform, in_chans=nch, r=R8)
    ops.l1_loss_final(parts, losses, R, pred.numel(), log_transform)
    sd = {"ps_head.conv_expand.0.weight": We.float().reshape(NE, E, 1, 1).requires_grad_(True),
          "ps_head.conv_expand.0.bias": be.clone().requires_grad_(True),
          "decoder_pred.weight": wd.reshape(nch, E, 1, 1).clone().requires_grad_(True)}
    xr = x.clone().requires_grad_(True)
    g_, b_ = gam.clone().requires_grad_(True), bet.clone().requires_grad_(True)
    pr = O._Prec(True)
    ref = O.ps_head_and_pred(pr, sd, cfg, pr.r(O.layer_norm(xr, g_, b_, eps)).reshape(B, H, W, E))
    loss, pix = O.forward_loss(cfg, ref, target)
    torch.cuda.synchronize()
    assert torch.isfinite(xn.float()).all() and torch.isfinite(mean).all() and torch.isfinite(rstd).all()
    close(pred, ref, 2e-3, 2e-3, "pred")
    assert abs(losses[0].item() - loss.item()) <= 1e-3 * abs(loss.item())
    assert abs(losses[1].item() - pix.item()) <= 2e-3 * abs(pix.item())
    (2.0 * loss).backward()
    dx = torch.full((M, E), float("nan"), device=DEV)
    dpart, lnp = torch.full((R, nch * 128), float("nan"), device=DEV), torch.full((R, 2 * E), float("nan"), device=DEV)
    ops.tail_bwd_dgrad_ln(xn, We, be, wd, pred, dpart, B, H, W, E, x, mean, rstd, gam, dx, lnp, target=target, gscale=2.0,
                          in_chans=nch, r=R8)
    dgb = torch.zeros(2 * E, device=DEV)
    ops.reduce_rows_multi([ops.reduce_region(lnp, 2 * E, dgb, 2 * E, R)])
    dwd = torch.zeros(nch, E, device=DEV)
    for k in range(nch):
        ops.reduce_rows2(dpart[:, 128 * k:], nch * 128, dwd[k], E, None, 0, None, 0, R)
    torch.cuda.synchronize()
    assert rel_l2(dx, xr.grad) <= 1.5e-2
    assert rel_l2(dgb[:E], g_.grad) <= 1.5e-2 and rel_l2(dgb[E:], b_.grad) <= 1.5e-2
    assert rel_l2(dwd, sd["decoder_pred.weight"].grad.reshape(nch, E)) <= 1.5e-2


@pytest.mark.parametrize("nch", [1, 2])
def test_r_entry_points_at_r4_equal_the_old_symbols_bitwise(nch):
    """r = 4 is untouched: the _r forms with r = 4 launch what the _c forms launch"""
    lib = _lib.load()
    B, H, W, E = 2, 8, 64, 96
    M, NE, R = B * H * W, 16 * E, (B * H * W + 31) // 32
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = rnd(M, E, seed=11)
    gam, bet = 1.0 + 0.1 * rnd(E, seed=12), 0.1 * rnd(E, seed=13)
    We, be, wd = bf(rnd(NE, E, scale=0.1, seed=1)), rnd(NE, scale=0.1, seed=2), rnd(nch, E, scale=0.2, seed=3)
    target = 0.3 * rnd(B, nch, 4 * H, 4 * W, seed=8)
    sp = lib.tulip_tail_wgrad_splits(B, H, W, E)
    assert sp == lib.tulip_tail_wgrad_splits_r(B, H, W, E, nch, 4)
    outs = []
    for new in (False, True):
        tail = (nch, 4) if new else (nch,)
        f = lambda name: getattr(lib, name + ("_r" if new else "_c"))
        nan = lambda *s, dt=torch.float32: torch.full(s, float("nan"), dtype=dt, device=DEV)
        xn, mean, rstd = nan(M, E, dt=torch.bfloat16), nan(M), nan(M)
        pred, pred2, parts = nan(B, nch, 4 * H, 4 * W), nan(B, nch, 4 * H, 4 * W), nan(2 * R)
        assert f("tulip_tail_fwd_ln")(p(x), p(gam), p(bet), 1e-6, p(xn), p(mean), p(rstd), p(We), p(be), p(wd), p(pred), p(target),
                                      p(parts), 1, B, H, W, E, st, *tail) == 0
        assert f("tulip_tail_fwd")(p(xn), p(We), p(be), p(wd), p(pred2), B, H, W, E, st, *tail) == 0
        dxn, dpart, dz, dpart2 = nan(M, E, dt=torch.bfloat16), nan(R, nch * 128), nan(M, NE, dt=torch.bfloat16), nan(R, nch * 128)
        assert f("tulip_tail_bwd_dgrad")(p(xn), p(We), p(be), p(wd), p(pred), p(dxn), p(dpart), B, H, W, E, p(target), None, 2.0,
                                         st, *tail) == 0
        assert f("tulip_tail_bwd")(p(xn), p(We), p(be), p(wd), p(pred), p(dz), p(dpart2), B, H, W, E, p(target), None, 2.0, st,
                                   *tail) == 0
        dx, dpart3, lnp = nan(M, E), nan(R, nch * 128), nan(R, 2 * E)
        assert f("tulip_tail_bwd_dgrad_ln")(p(xn), p(We), p(be), p(wd), p(pred), p(dpart3), B, H, W, E, p(target), None, 2.0, p(x),
                                            p(mean), p(rstd), p(gam), p(dx), None, None, 1, p(lnp), st, *tail) == 0
        sw, sb = nan(sp, NE * E), nan(sp, NE)
        assert f("tulip_tail_wgrad")(p(xn), p(We), p(be), p(wd), p(pred), p(sw), p(sb), B, H, W, E, p(target), None, 2.0, st,
                                     *tail) == 0
        torch.cuda.synchronize()
        outs.append([xn, mean, rstd, pred, pred2, parts, dxn, dpart, dz, dpart2, dx, dpart3, lnp, sw, sb])
    for i, (a, b) in enumerate(zip(*outs)):
        assert torch.isfinite(a.float()).all(), i
        assert torch.equal(a, b), i


def test_expand_norm_p8():
    """FinalPatchExpanding's rearrange + LayerNorm + decoder_pred at P = 8 and its backward (in_chans 1 and 2)"""
    for nch in (1, 2):
        B, H, W, P, Cn = 2, 4, 16, 8, 48
        M, eps = B * H * W, 1e-6
        y = rnd(M, P * P * Cn, seed=1)
        gam, bet = 1 + 0.1 * rnd(Cn, seed=2), 0.1 * rnd(Cn, seed=3)
        dotw = rnd(nch, Cn, scale=0.2, seed=4)
        mean, rstd = torch.empty(M * P * P, device=DEV), torch.empty(M * P * P, device=DEV)
        pred = torch.full((B, nch, H * P, W * P), float("nan"), device=DEV)
        ops.expand_norm_fwd(y, gam, bet, mean, rstd, B, H, W, P, Cn, eps, dotw=dotw, pred=pred, in_chans=nch)
        yr, gr, br, wr = (t.clone().requires_grad_(True) for t in (y, gam, bet, dotw))
        fine = yr.reshape(B, H, W, P, P, Cn).permute(0, 1, 3, 2, 4, 5).reshape(B, H * P, W * P, Cn)
        ln = O._BF16Round.apply(O.layer_norm(fine, gr, br, eps))
        ref = torch.einsum("bhwc,kc->bkhw", ln, wr)
        torch.cuda.synchronize()
        close(pred, ref, 1e-3, 1e-4, "expand_norm pred")
        dpred = rnd(B, nch, H * P, W * P, seed=5)
        ref.backward(dpred)
        R = ops.expand_norm_bwd_partial_rows(B, H, W, P)
        part = torch.full((R, (2 + nch) * Cn), float("nan"), device=DEV)
        dy = torch.full((M, P * P * Cn), float("nan"), dtype=torch.bfloat16, device=DEV)
        ops.expand_norm_bwd(y, mean, rstd, gam, dy, part, B, H, W, P, Cn, dpred=dpred, dotw=dotw, beta=bet, in_chans=nch)
        tot = torch.zeros((2 + nch) * Cn, device=DEV)
        ops.reduce_rows_multi([ops.reduce_region(part, (2 + nch) * Cn, tot, (2 + nch) * Cn, R)])
        torch.cuda.synchronize()
        assert rel_l2(dy.float(), yr.grad) <= 1e-2
        assert rel_l2(tot[:Cn], gr.grad) <= 1e-3 and rel_l2(tot[Cn:2 * Cn], br.grad) <= 1e-3
        assert rel_l2(tot[2 * Cn:].reshape(nch, Cn), wr.grad) <= 1e-3


# ------------------------------------------------------------------ model
def build(cfg: O.TulipConfig, sd=None, train=True, **kw):
    from tulip_amd.model import tulip as T
    m = T.TULIP(**UC.model_kwargs(cfg), **kw)
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    return m.to(DEV).train(train)


def engine_step(m, lo, hi, B):
    eng = m.engine()
    eng.bind(torch.device(DEV, torch.cuda.current_device()))
    P = eng.plan(B)
    eng.check_target(B, hi)
    P.x_in.copy_(lo.to(DEV)); P.target.copy_(hi.to(DEV))
    eng.draw_drop_scales(P, False)
    eng.run_forward(P)
    g = torch.zeros(eng.params.total, device=DEV)
    eng.run_backward(P, g)
    torch.cuda.synchronize()
    W_ = eng.params
    grads = {n: g[W_.offset[n]:W_.offset[n] + W_.numel[n]].view(W_.shape[n]).cpu() for n in W_.names}
    return P, grads


@pytest.mark.parametrize("name", UC.NAMES)
def test_model_vs_reference_fixture(name):
    z = np.load(os.path.join(GOLD, "g17_upscale.npz"), allow_pickle=False)
    with open(os.path.join(GOLD, "g17_upscale.json")) as f:
        meta = json.load(f)
    cfg = O.TulipConfig(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in meta["configs"][name]["cfg"].items()})
    sd = O.key_seeded_state_dict(cfg, seed=meta["seed"])
    lo, hi = UC.batch(cfg, meta["batch"], seed=1234 + meta["seed"])
    P, grads = engine_step(build(cfg, sd), lo, hi, meta["batch"])
    assert tuple(P.pred.shape) == tuple(z[f"{name}::pred_shape"].tolist())
    loss, pix = float(z[f"{name}::loss"]), float(z[f"{name}::pixel_loss"])
    assert abs(P.losses[0].item() - loss) <= 1e-3 * loss, (P.losses[0].item(), loss)
    assert abs(P.losses[1].item() - pix) <= 2e-3 * pix, (P.losses[1].item(), pix)
    pred = P.pred.reshape(-1)[torch.from_numpy(z[f"{name}::pred_index"]).to(DEV)].cpu()
    assert rel_l2(pred, z[f"{name}::pred"]) <= 1e-2
    assert all(torch.isfinite(g).all() for g in grads.values())
    for k in meta["configs"][name]["grad_keys"]:
        e = rel_l2(grads[k], z[f"{name}::grad::{k}"])
        assert e <= 1.5e-2, (k, e)
    for k, step in meta["configs"][name]["grad_rows"].items():
        e = rel_l2(grads[k][::step], z[f"{name}::grad_rows::{k}"])
        assert e <= 1.5e-2, (k, e)
    for k, l2 in zip(z[f"{name}::grad_keys"].tolist(), z[f"{name}::grad_l2"]):
        got = grads[k].double().norm().item()
        tol = 1e-1 if k.endswith("relative_position_bias_table") else 1.5e-2
        assert abs(got - l2) <= tol * l2 + 1e-9, (k, got, l2)


@pytest.mark.parametrize("pixel_shuffle", [True, False])
def test_final_heads_fwd_bwd_vs_oracle_lowp(pixel_shuffle):
    """the engine's head sequence at r = 8 (pixel shuffle / FinalPatchExpanding with the E -> 64E Linear through the GEMM) against
    the oracle in the engine's own precision: prediction, loss and the head's gradients"""
    name = "ps8_p2x8" if pixel_shuffle else "fe8_p2x8"
    cfg = UC.config(name)
    sd = O.key_seeded_state_dict(cfg, seed=3)
    lo, hi = UC.batch(cfg, 2, seed=99)
    P, grads = engine_step(build(cfg, sd), lo, hi, 2)
    with torch.no_grad():
        op, ol, _ = O.tulip_forward(sd, cfg, lo, hi, lowp=True)
    assert rel_l2(P.pred, op) <= 1e-2                       # (the prediction band of test_model_vs_reference_fixture)
    assert abs(P.losses[0].item() - ol.item()) <= 1e-3 * ol.item()
    _, _, _, og = O.tulip_loss_and_grads(sd, cfg, lo, hi)
    for k in [UC.expand_key(cfg), "decoder_pred.weight", "norm_up.weight"] + ([] if pixel_shuffle else ["final_patch_expanding.norm.weight"]):
        e = rel_l2(grads[k], og[k])
        assert e <= 1.5e-2, (k, e)


def _kitti_2x8(seed=0, **kw):
    from tulip_amd.model.tulip import tulip_base
    torch.manual_seed(seed)
    args = dict(img_size=(16, 1024), target_img_size=(64, 1024), patch_size=(2, 8), window_size=(2, 8), pixel_shuffle=True,
                circular_padding=True, log_transform=True, patch_unmerging=True)
    if kw:         # tulip_base pins drop_rate / attn_drop_rate to 0: the same network with the rates given
        from functools import partial
        import torch.nn as nn
        from tulip_amd.model.tulip import TULIP
        return TULIP(depths=(2, 2, 2, 2), embed_dim=96, num_heads=(3, 6, 12, 24), qkv_bias=True, mlp_ratio=4, drop_path_rate=0.1,
                     norm_layer=partial(nn.LayerNorm, eps=1e-6), **args, **kw).to(DEV)
    return tulip_base(**args).to(DEV)


def _kitti_batch(B=8, nch=1):
    g = torch.Generator().manual_seed(1234)
    r = torch.rand(B, nch, 64, 1024, generator=g)
    r[torch.rand(B, nch, 64, 1024, generator=g) < 0.1] = 0
    hi = torch.log1p(r)
    return hi[:, :, 0::4, :].contiguous().to(DEV), hi.to(DEV)


def test_kitti_base_2x8_batch8_step_vs_oracle():
    cfg = O.tulip_base_config(patch_size=(2, 8), drop_path_rate=0.0)
    assert cfg.upscale_factor == 8
    sd = O.key_seeded_state_dict(cfg, seed=11)
    lo, hi = UC.batch(cfg, 8, seed=21)
    P, grads = engine_step(build(cfg, sd), lo, hi, 8)
    _, oloss, _, og = O.tulip_loss_and_grads(sd, cfg, lo, hi)
    assert abs(P.losses[0].item() - oloss.item()) <= 1e-3 * oloss.item()
    for n, g in grads.items():
        e = rel_l2(g, og[n])
        assert e <= (1e-1 if n.endswith("relative_position_bias_table") else 2e-2), (n, e)


@pytest.mark.parametrize("accum,drop", [(1, 0.0), (2, 0.0), (1, 0.1)])
def test_trainer_steps_are_bit_identical_r8(accum, drop):
    """two Trainers from one state: the captured step equals the eager step bit for bit, and so does the next one"""
    from tulip_amd.trainer import Trainer
    lo, hi = _kitti_batch()
    kw = dict(drop_rate=drop, attn_drop_rate=drop) if drop else {}
    ma = _kitti_2x8(**kw).train()
    mb = _kitti_2x8(**kw).train()
    mb.load_state_dict(ma.state_dict())
    ta = Trainer(ma, 8, use_graph=True, accum_iter=accum)
    tb = Trainer(mb, 8, use_graph=False, accum_iter=accum)
    for _ in range(2):
        la = ta.step(lo, hi).clone()
        lb = tb.step(lo, hi).clone()
        torch.cuda.synchronize()
        assert torch.isfinite(la).all()
        assert torch.equal(la, lb), (la, lb)
        assert torch.equal(ta.eng.params.flat, tb.eng.params.flat)
    with pytest.raises(ValueError, match="output shape"):
        ta.step(lo, hi[:, :, ::2])


def test_graphed_forward_equals_module_forward_r8():
    from tulip_amd.infer import GraphedForward
    lo, hi = _kitti_batch()
    m = _kitti_2x8().eval()
    gf = GraphedForward(m, 8)
    with torch.no_grad():
        ref = m(lo, hi, mc_drop=True)
    assert tuple(ref.shape) == (8, 1, 64, 1024)
    for _ in range(2):
        a = gf(lo)
        torch.cuda.synchronize()
        assert tuple(a.shape) == (8, 1, 64, 1024)
        assert torch.isfinite(a).all() and torch.equal(a, ref)


def test_constructor_defaults_full_size_module_path():
    """TULIP() exactly as the reference constructs it by default -- (4, 4) patches, window 4, FinalPatchExpanding, DropPath 0.1
    (eval mode here so that the oracle sees the same network) -- on a 32x2048 input with the (B, 1, 64, 4096) target"""
    from tulip_amd.model import tulip as T
    B = 2
    cfg = O.TulipConfig(img_size=(32, 2048), target_img_size=(128, 2048), patch_size=(4, 4), window_size=(4, 4), depths=(2, 2, 6, 2),
                        ln_eps=1e-5, pixel_shuffle=False, circular_padding=False, log_transform=False, patch_unmerging=False)
    assert cfg.upscale_factor == 8 and UC.output_size(cfg) == (64, 4096)
    sd = O.key_seeded_state_dict(cfg, seed=5)
    m = T.TULIP()
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    lo, hi = UC.batch(cfg, B, seed=77)
    with pytest.raises(ValueError, match="output shape"):
        m(lo.to(DEV), torch.zeros(B, 1, 128, 2048, device=DEV))
    pred, loss, pix = m(lo.to(DEV), hi.to(DEV))
    assert tuple(pred.shape) == (B, 1, 64, 4096)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max().item() > 0, n
    _, oloss, _, og = O.tulip_loss_and_grads(sd, cfg, lo, hi)
    assert abs(loss.item() - oloss.item()) <= 1e-3 * oloss.item()
    grads = dict(m.named_parameters())
    for n in ("patch_embed.proj.weight", "final_patch_expanding.expand.weight", "layers.2.blocks.5.mlp.fc1.weight"):
        got, want = grads[n].grad.double().norm().item(), og[n].double().norm().item()
        assert abs(got - want) <= 2e-2 * want, (n, got, want)

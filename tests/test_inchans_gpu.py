"""GPU: multi-channel images (in_chans 2 to 4).

  1. the kernels against fp32 autograd of the oracle with the tolerances of test_ops_gpu: the patch embedding at Cin 2
     and 4 (circular and not, partial rows folded), the fused head family and expand_norm at NCH 2 and 4, with and
     without a target;
  2. the model against the reference fixture g16_inchans, and a KITTI tulip_base batch-8 step at in_chans 2 against the
     fp32 oracle (bands of test_model_gpu.test_kitti_base_full_size_gradients_vs_oracle);
  3. bit-identity at in_chans 2: two Trainer steps from one state (captured against eager, accum_iter 2), GraphedForward
     against the module forward with mc_drop;
  4. evaluate refuses a multi-channel model.
"""
import json
import os
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import tulip_oracle as O
from tulip_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


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


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("cin", [2, 4])
@pytest.mark.parametrize("circular", [True, False])
@pytest.mark.parametrize("E,Hin,Win", [(96, 16, 1024), (48, 3, 20)])
def test_patch_embed_multichannel(cin, circular, E, Hin, Win):
    B = 2
    cfg = O.TulipConfig(img_size=(Hin, Win), embed_dim=E, circular_padding=circular, in_chans=cin)
    kw = 8 if circular else 4
    img = torch.rand(B, cin, Hin, Win, device=DEV)
    sd = {"patch_embed.proj.weight": rnd(E, cin, 1, kw, scale=0.3), "patch_embed.proj.bias": rnd(E, scale=0.1, seed=1),
          "patch_embed.norm.weight": 1 + 0.1 * rnd(E, seed=2), "patch_embed.norm.bias": 0.1 * rnd(E, seed=3)}
    sdr = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref = O.patch_embed(O._Prec(False), sdr, cfg, img)
    out = torch.empty(B, Hin, Win // 4, E, device=DEV)
    ops.patch_embed_fwd(img, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], sd["patch_embed.norm.weight"],
                        sd["patch_embed.norm.bias"], out, B, cin, Hin, Win, E, 1, 4, kw, circular, 1e-6)
    close(out, ref, 1e-4, 2e-5, "patch embed fwd")
    dout = rnd(B, Hin, Win // 4, E, seed=5)
    ref.backward(dout)
    # partial-row mode (the engine's): rows laid out [w | b | gamma | beta], folded by reduce_rows2
    T = cin * kw
    ntok = B * Hin * (Win // 4)
    nb, stride = ops.patch_embed_bwd_blocks(ntok), E * T + 3 * E
    part = torch.full((nb, stride), float("nan"), device=DEV)
    base = part.data_ptr()
    ops.patch_embed_bwd(img, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], sd["patch_embed.norm.weight"],
                        dout, base, base + 4 * E * T, base + 4 * (E * T + E), base + 4 * (E * T + 2 * E), B, cin, Hin,
                        Win, E, 1, 4, kw, circular, 1e-6, partial_stride=stride)
    tot = torch.zeros(stride, device=DEV)
    ops.reduce_rows2(part, stride, tot, stride, None, 0, None, 0, nb)
    torch.cuda.synchronize()
    close(tot[:E * T].reshape(E, cin, 1, kw), sdr["patch_embed.proj.weight"].grad, 2e-3, 2e-4, "embed dw (partial)")
    close(tot[E * T:E * T + E], sdr["patch_embed.proj.bias"].grad, 2e-3, 2e-4, "embed db (partial)")
    close(tot[E * T + E:E * T + 2 * E], sdr["patch_embed.norm.weight"].grad, 2e-3, 2e-4, "embed dgamma (partial)")
    close(tot[E * T + 2 * E:], sdr["patch_embed.norm.bias"].grad, 2e-3, 2e-4, "embed dbeta (partial)")


@pytest.mark.parametrize("nch", [2, 4])
@pytest.mark.parametrize("B,H,W,E", [(2, 8, 64, 48), (1, 3, 24, 96), (3, 16, 64, 96)])
@pytest.mark.parametrize("l1", [False, True])
def test_head_family_multichannel(nch, B, H, W, E, l1):
    """tail_fwd / tail_bwd / tail_bwd_dgrad / tail_wgrad at NCH output channels against autograd of ps_head_and_pred"""
    M = B * H * W
    cfg = O.TulipConfig(img_size=(H, W * 4), target_img_size=(4 * H, 4 * W), embed_dim=E, in_chans=nch)
    xn = bf(rnd(M, E))
    We, be, wd = bf(rnd(16 * E, E, scale=0.1, seed=1)), rnd(16 * E, scale=0.1, seed=2), rnd(nch, E, scale=0.2, seed=3)
    sd = {"ps_head.conv_expand.0.weight": We.float().reshape(16 * E, E, 1, 1).requires_grad_(True),
          "ps_head.conv_expand.0.bias": be.clone().requires_grad_(True),
          "decoder_pred.weight": wd.reshape(nch, E, 1, 1).clone().requires_grad_(True)}
    xr = xn.float().reshape(B, H, W, E).requires_grad_(True)
    ref = O.ps_head_and_pred(O._Prec(False), sd, cfg, xr)
    pred = torch.empty(B, nch, 4 * H, 4 * W, device=DEV)
    ops.tail_fwd(xn, We, be, wd, pred, B, H, W, E, in_chans=nch)
    close(pred, ref, 1e-4, 2e-5, "tail fwd")
    if l1:
        target = rnd(B, nch, 4 * H, 4 * W, seed=8)
        (3.0 * (ref - target).abs().mean()).backward()
        kw = dict(target=target, gscale=3.0, in_chans=nch)
        dsrc = pred
    else:
        dsrc = rnd(B, nch, 4 * H, 4 * W, seed=4)
        ref.backward(dsrc)
        kw = dict(in_chans=nch)
    R = (M + 31) // 32
    dxn = torch.full((M, E), float("nan"), dtype=torch.bfloat16, device=DEV)
    dpart = torch.full((R, nch * 128), float("nan"), device=DEV)
    ops.tail_bwd_dgrad(xn, We, be, wd, dsrc, dxn, dpart, B, H, W, E, **kw)
    sp = ops.tail_wgrad_splits(B, H, W, E)
    sw = torch.full((sp, 16 * E * E), float("nan"), device=DEV)
    sb = torch.full((sp, 16 * E), float("nan"), device=DEV)
    ops.tail_wgrad(xn, We, be, wd, dsrc, sw, sb, B, H, W, E, **kw)
    dwd = torch.zeros(nch, E, device=DEV)
    for k in range(nch):
        ops.reduce_rows2(dpart[:, 128 * k:], nch * 128, dwd[k], E, None, 0, None, 0, R)
    dWe, dbe = torch.zeros(16 * E * E, device=DEV), torch.zeros(16 * E, device=DEV)
    ops.reduce_rows_multi([ops.reduce_region(sw, 16 * E * E, dWe, 16 * E * E, sp), ops.reduce_region(sb, 16 * E, dbe, 16 * E, sp)])
    torch.cuda.synchronize()
    gwd = sd["decoder_pred.weight"].grad.reshape(nch, E)
    close(dwd, gwd, 1e-3, 1e-4 * max(1.0, float(dwd.abs().max())), "tail dwd")
    for got, want, what in [(dxn.float(), xr.grad.reshape(M, E), "dxn"),
                            (dWe.reshape(16 * E, E), sd["ps_head.conv_expand.0.weight"].grad.reshape(16 * E, E), "dWe"),
                            (dbe, sd["ps_head.conv_expand.0.bias"].grad, "dbe")]:
        assert torch.isfinite(got).all(), what
        err = (got - want).abs().max().item() / max(want.abs().max().item(), 1e-30)
        rl2 = ((got - want).norm() / want.norm()).item()
        assert err <= 1e-2 and rl2 <= 6e-3, (what, err, rl2)
    # the dz-materialising form: the same decoder_pred partial rows, dz through its consumers
    dz = torch.empty(M, 16 * E, dtype=torch.bfloat16, device=DEV)
    dpart2 = torch.full_like(dpart, float("nan"))
    ops.tail_bwd(xn, We, be, wd, dsrc, dz, dpart2, B, H, W, E, **kw)
    torch.cuda.synchronize()
    assert (dpart2 - dpart).abs().max().item() <= 2e-6 * max(dpart2.abs().max().item(), 1e-30)
    dzf = dz.float()
    close(dzf.sum(0), sd["ps_head.conv_expand.0.bias"].grad, 2e-2, 4e-3, "tail_bwd dbe (colsum dz)")
    close(dzf @ We.float(), xr.grad.reshape(M, E), 2e-2, 4e-3, "tail_bwd dxn (dz.We)")


@pytest.mark.parametrize("nch", [2, 4])
@pytest.mark.parametrize("log_transform", [True, False])
def test_head_with_norm_up_and_loss_multichannel(nch, log_transform):
    """tail_fwd_ln (loss partials summed over every channel) and tail_bwd_dgrad_ln at NCH channels against the oracle"""
    B, H, W, E = 2, 8, 64, 96
    M, R = B * H * W, (B * H * W + 31) // 32
    cfg = O.TulipConfig(img_size=(H, W * 4), target_img_size=(4 * H, 4 * W), embed_dim=E, log_transform=log_transform,
                        in_chans=nch)
    x = rnd(M, E, seed=11)
    gam, bet = 1.0 + 0.1 * rnd(E, seed=12), 0.1 * rnd(E, seed=13)
    We, be, wd = bf(rnd(16 * E, E, scale=0.1, seed=1)), rnd(16 * E, scale=0.1, seed=2), rnd(nch, E, scale=0.2, seed=3)
    target = 0.3 * rnd(B, nch, 4 * H, 4 * W, seed=8)
    eps = 1e-6
    xn, mean, rstd = torch.empty(M, E, dtype=torch.bfloat16, device=DEV), torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    pred = torch.empty(B, nch, 4 * H, 4 * W, device=DEV)
    parts, losses = torch.full((2 * R,), float("nan"), device=DEV), torch.empty(2, device=DEV)
    ops.tail_fwd_ln(x, gam, bet, eps, xn, mean, rstd, We, be, wd, pred, B, H, W, E, target=target, loss_partials=parts,
                    log_transform=log_transform, in_chans=nch)
    ops.l1_loss_final(parts, losses, R, pred.numel(), log_transform)
    sd = {"ps_head.conv_expand.0.weight": We.float().reshape(16 * E, E, 1, 1).requires_grad_(True),
          "ps_head.conv_expand.0.bias": be.clone().requires_grad_(True),
          "decoder_pred.weight": wd.reshape(nch, E, 1, 1).clone().requires_grad_(True)}
    xr = x.clone().requires_grad_(True)
    g_, b_ = gam.clone().requires_grad_(True), bet.clone().requires_grad_(True)
    pr = O._Prec(True)
    ref = O.ps_head_and_pred(pr, sd, cfg, pr.r(O.layer_norm(xr, g_, b_, eps)).reshape(B, H, W, E))
    loss, pix = O.forward_loss(cfg, ref, target)
    torch.cuda.synchronize()
    close(pred, ref, 2e-3, 2e-3, "pred")
    assert abs(losses[0].item() - loss.item()) <= 1e-3 * abs(loss.item())
    assert abs(losses[1].item() - pix.item()) <= 2e-3 * abs(pix.item())
    (2.0 * loss).backward()
    dx = torch.full((M, E), float("nan"), device=DEV)
    dpart, lnp = torch.full((R, nch * 128), float("nan"), device=DEV), torch.full((R, 2 * E), float("nan"), device=DEV)
    ops.tail_bwd_dgrad_ln(xn, We, be, wd, pred, dpart, B, H, W, E, x, mean, rstd, gam, dx, lnp, target=target, gscale=2.0,
                          in_chans=nch)
    dgb = torch.zeros(2 * E, device=DEV)
    ops.reduce_rows_multi([ops.reduce_region(lnp, 2 * E, dgb, 2 * E, R)])
    dwd = torch.zeros(nch, E, device=DEV)
    for k in range(nch):
        ops.reduce_rows2(dpart[:, 128 * k:], nch * 128, dwd[k], E, None, 0, None, 0, R)
    torch.cuda.synchronize()
    assert rel_l2(dx, xr.grad) <= 1.5e-2
    assert rel_l2(dgb[:E], g_.grad) <= 1.5e-2 and rel_l2(dgb[E:], b_.grad) <= 1.5e-2
    assert rel_l2(dwd, sd["decoder_pred.weight"].grad.reshape(nch, E)) <= 1.5e-2


@pytest.mark.parametrize("nch", [2, 4])
def test_expand_norm_multichannel(nch):
    """FinalPatchExpanding's rearrange + LayerNorm + decoder_pred (nch dot products per fine token) and its backward"""
    B, H, W, P, Cn = 2, 4, 16, 4, 48
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
    dy = torch.empty(M, P * P * Cn, dtype=torch.bfloat16, device=DEV)
    ops.expand_norm_bwd(y, mean, rstd, gam, dy, part, B, H, W, P, Cn, dpred=dpred, dotw=dotw, beta=bet, in_chans=nch)
    tot = torch.zeros((2 + nch) * Cn, device=DEV)
    ops.reduce_rows_multi([ops.reduce_region(part, (2 + nch) * Cn, tot, (2 + nch) * Cn, R)])
    torch.cuda.synchronize()
    assert rel_l2(dy.float(), yr.grad) <= 1e-2
    assert rel_l2(tot[:Cn], gr.grad) <= 1e-3 and rel_l2(tot[Cn:2 * Cn], br.grad) <= 1e-3
    assert rel_l2(tot[2 * Cn:].reshape(nch, Cn), wr.grad) <= 1e-3


# ------------------------------------------------------------------ model
def build(cfg: O.TulipConfig, sd=None, train=True):
    from tulip_amd.model import tulip as T
    m = T.TULIP(img_size=cfg.img_size, target_img_size=cfg.target_img_size, patch_size=cfg.patch_size,
                in_chans=cfg.in_chans, embed_dim=cfg.embed_dim, window_size=list(cfg.window_size), depths=cfg.depths,
                num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio, drop_path_rate=cfg.drop_path_rate,
                norm_layer=partial(nn.LayerNorm, eps=cfg.ln_eps), pixel_shuffle=cfg.pixel_shuffle,
                circular_padding=cfg.circular_padding, log_transform=cfg.log_transform,
                patch_unmerging=cfg.patch_unmerging)
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    return m.to(DEV).train(train)


def engine_step(m, lo, hi, B):
    eng = m.engine()
    eng.bind(torch.device(DEV, torch.cuda.current_device()))
    P = eng.plan(B)
    P.x_in.copy_(lo.to(DEV)); P.target.copy_(hi.to(DEV))
    eng.draw_drop_scales(P, False)
    eng.run_forward(P)
    g = torch.zeros(eng.params.total, device=DEV)
    eng.run_backward(P, g)
    torch.cuda.synchronize()
    W_ = eng.params
    grads = {n: g[W_.offset[n]:W_.offset[n] + W_.numel[n]].view(W_.shape[n]).cpu() for n in W_.names}
    return P, grads


@pytest.mark.parametrize("name", ["c2", "c3", "c4"])
def test_model_vs_reference_fixture(name):
    z = np.load(os.path.join(GOLD, "g16_inchans.npz"), allow_pickle=False)
    with open(os.path.join(GOLD, "g16_inchans.json")) as f:
        meta = json.load(f)
    cfg = O.TulipConfig(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in meta["configs"][name]["cfg"].items()})
    sd = O.key_seeded_state_dict(cfg, seed=meta["seed"])
    lo, hi = O.synthetic_batch(cfg, meta["batch"], seed=1234 + meta["seed"])
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


def test_kitti_base_batch8_step_vs_oracle_in_chans_2():
    cfg = O.tulip_base_config(in_chans=2, drop_path_rate=0.0)
    sd = O.key_seeded_state_dict(cfg, seed=11)
    lo, hi = O.synthetic_batch(cfg, 8, seed=21)
    P, grads = engine_step(build(cfg, sd), lo, hi, 8)
    _, oloss, _, og = O.tulip_loss_and_grads(sd, cfg, lo, hi)
    assert abs(P.losses[0].item() - oloss.item()) <= 1e-3 * oloss.item()
    for n, g in grads.items():
        e = rel_l2(g, og[n])
        assert e <= (1e-1 if n.endswith("relative_position_bias_table") else 2e-2), (n, e)


def _kitti2(seed=0):
    from tulip_amd.model.tulip import tulip_base
    torch.manual_seed(seed)
    return tulip_base(img_size=(16, 1024), target_img_size=(64, 1024), patch_size=(1, 4), window_size=(2, 8),
                      pixel_shuffle=True, circular_padding=True, log_transform=True, patch_unmerging=True,
                      in_chans=2).to(DEV)


def _kitti2_batch(B=8):
    g = torch.Generator().manual_seed(1234)
    r = torch.rand(B, 2, 64, 1024, generator=g)
    r[torch.rand(B, 2, 64, 1024, generator=g) < 0.1] = 0
    hi = torch.log1p(r)
    return hi[:, :, 0::4, :].contiguous().to(DEV), hi.to(DEV)


@pytest.mark.parametrize("accum", [1, 2])
def test_trainer_steps_are_bit_identical_in_chans_2(accum):
    """two Trainers from one state: the captured step equals the eager step bit for bit, and so does the next one"""
    from tulip_amd.trainer import Trainer
    lo, hi = _kitti2_batch()
    ma = _kitti2().train()
    mb = _kitti2().train()
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


def test_graphed_forward_equals_module_forward_in_chans_2():
    from tulip_amd.infer import GraphedForward
    lo, hi = _kitti2_batch()
    m = _kitti2().eval()
    gf = GraphedForward(m, 8)
    with torch.no_grad():
        ref = m(lo, hi, mc_drop=True)
    assert tuple(ref.shape) == (8, 2, 64, 1024)
    for _ in range(2):
        a = gf(lo)
        torch.cuda.synchronize()
        assert tuple(a.shape) == (8, 2, 64, 1024)
        assert torch.isfinite(a).all() and torch.equal(a, ref)


def test_evaluate_refuses_in_chans_2():
    from tulip_amd import evaluation as EV
    m = _kitti2().eval()
    with pytest.raises(ValueError, match="in_chans"):
        EV.evaluate([], m, torch.device(DEV), args=None)

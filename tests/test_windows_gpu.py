"""GPU: attention windows of 32 and 64 tokens (window_size 4x8, 2x16, 8x8, 4x16, 2x32 and the (1, L) backup windows).

  1. the kernels, every window shape shifted and not, head dim 16 and 32: forward, dqkv and the folded d(table) against
     autograd of the same fp32 reference with the tolerances of test_ops_gpu.test_window_attention_fwd_bwd;
  2. the attn_drop forms at L = 32 / 64: the mask the kernel applied, read back through the output, equals the host mask
     bit for bit, and forward / gradients stay in the band against the reference with that mask;
  3. the model against the reference fixture g15_windows, and a KITTI tulip_base batch-8 step at (4, 8) and (2, 16)
     against the fp32 oracle (bands of test_model_gpu.test_kitti_base_full_size_gradients_vs_oracle);
  4. bit-identity: two Trainer steps from one state, the captured step against the eager one, GraphedForward against the
     module forward;
  5. refusals: a 24-token window, fp8 scores at a 32-token window.
"""
import json
import os
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import tulip_oracle as O
from tulip_amd import dropout as D
from tulip_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
WINDOWS = [(4, 8), (2, 16), (1, 32), (8, 8), (4, 16), (2, 32), (1, 64)]


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


def attn_reference(qkv, table, rel_index, B, H, W, C, nh, win, sft, drop_mult=None):
    """tulip.py:289-323 minus the Linears, natural-order tokens, fp32 (P rounded to bf16); drop_mult: the attn_drop
    multiplier [B * nW, nh, L, L] on the probabilities"""
    L, P = win[0] * win[1], C // nh
    idx = torch.from_numpy(O.window_token_index(H, W, win, sft)).to(qkv.device)
    nW = idx.shape[0]
    t = qkv.reshape(B, H * W, 3 * C)[:, idx.reshape(-1)].reshape(B * nW, L, 3, nh, P).permute(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]
    attn = (q @ k.transpose(-2, -1)) * P ** -0.5
    attn = attn + table[rel_index.reshape(-1).long()].reshape(L, L, nh).permute(2, 0, 1)[None]
    if sft != (0, 0):
        mask = torch.from_numpy(O.shift_attention_mask(H, W, win, sft)).to(qkv.device)
        attn = (attn.reshape(B, nW, nh, L, L) + mask[None, :, None]).reshape(B * nW, nh, L, L)
    p = torch.softmax(attn, -1)
    if drop_mult is not None:
        p = p * drop_mult
    p = O._BF16Round.apply(p)
    o = (p @ v).permute(0, 2, 1, 3).reshape(B, nW * L, C)
    out = torch.zeros(B, H * W, C, device=qkv.device, dtype=o.dtype)
    out[:, idx.reshape(-1)] = o
    return out.reshape(B * H * W, C)


def geometry(win, odd):
    """(B, H, W): two windows down and four across, or an odd window count (3 samples x 1 x 3: the last group of a
    32-token launch holds one window)"""
    wh, ww = win
    return (3, wh, 3 * ww) if odd else (2, 2 * wh, 4 * ww)


def fold_table(part, R, nh, LL, rel32, ntab):
    dtab = torch.zeros(ntab, nh, device=DEV)
    ops.reduce_rows_multi([ops.reduce_region(part, nh * LL, dtab, nh * LL, R, scatter_index=rel32, scatter_nh=nh,
                                             scatter_len=LL)])
    return dtab


@pytest.mark.parametrize("win", WINDOWS)
@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("C,nh,odd", [(96, 3, False), (48, 3, True), (384, 12, False)])
def test_window_attention_fwd_bwd(win, shift, C, nh, odd):
    B, H, W = geometry(win, odd)
    L, LL = win[0] * win[1], (win[0] * win[1]) ** 2
    sft = (win[0] // 2, win[1] // 2) if shift else (0, 0)
    M = B * H * W
    qkv = bf(rnd(M, 3 * C, scale=1.5))
    ntab = (2 * win[0] - 1) * (2 * win[1] - 1)
    table = rnd(ntab, nh, scale=0.5, seed=1)
    rel = torch.from_numpy(O.relative_position_index(*win)).to(DEV)
    rel32 = rel.to(torch.int32).contiguous()
    out = torch.full((M, C), float("nan"), dtype=torch.bfloat16, device=DEV)
    ops.window_attn_fwd(qkv, table, rel32, out, B, H, W, C, nh, win, sft, int(shift))
    qr = qkv.float().requires_grad_(True)
    tr = table.clone().requires_grad_(True)
    ref = attn_reference(qr, tr, rel, B, H, W, C, nh, win, sft)
    close(out, ref, 2 ** -7, 3e-3, "attn fwd")
    dout = bf(rnd(M, C, seed=3))
    ref.backward(dout.float())
    dqkv = torch.full_like(qkv, float("nan"))
    R = ops.window_attn_bwd_partial_rows(B, H, W, nh, win)
    part = torch.full((R * nh, LL), float("nan"), device=DEV)
    ops.window_attn_bwd(qkv, dout, table, rel32, dqkv, part, B, H, W, C, nh, win, sft, int(shift))
    close(dqkv, qr.grad, 2 ** -5, 6e-3, "attn dqkv")
    assert torch.isfinite(part).all()
    dtab = fold_table(part, R, nh, LL, rel32, ntab)
    close(dtab, tr.grad, 2e-2, 5e-3, "attn dtable")
    assert torch.equal(dtab, fold_table(part, R, nh, LL, rel32, ntab))        # the scatter is deterministic
    # the launch is deterministic too
    dqkv2, part2 = torch.empty_like(qkv), torch.empty_like(part)
    ops.window_attn_bwd(qkv, dout, table, rel32, dqkv2, part2, B, H, W, C, nh, win, sft, int(shift))
    assert torch.equal(dqkv, dqkv2) and torch.equal(part, part2)


def _mask_tensor(seed, counter, site, p, B, H, W, nh, win):
    return torch.from_numpy(D.multiplier(seed, counter, site, p, D.attn_index(B, H, W, nh, win))).to(DEV)


@pytest.mark.parametrize("win", [(4, 8), (2, 16), (1, 32), (8, 8), (1, 64)])
def test_attn_drop_mask_readout_is_exact(win):
    """q = k = 0 and a zero table make every probability exactly 1/L; V[key][d] = 1 + (key >= 32) where d == key % 32 puts
    the dropped probabilities of keys d and d + 32 into output column d as m0 + 2 m1 (times bf16(1/(1-p)) / L)."""
    B, H, W = 2, 2 * win[0], 4 * win[1]
    C, nh, L = 96, 3, win[0] * win[1]
    seed, counter, site, p = 0x0DDBA11, 9, D.site(2, D.ATTN), 0.3
    M = B * H * W
    idx = O.window_token_index(H, W, win, (0, 0))                 # [nW, L] natural token of each slot
    nW = idx.shape[0]
    qkv = torch.zeros(M, 3 * C)
    slot = np.zeros(H * W, dtype=np.int64)
    slot[idx.reshape(-1)] = np.tile(np.arange(L), nW)
    vcol = torch.zeros(H * W, 32)
    vcol[torch.arange(H * W), torch.from_numpy(slot % 32)] = torch.from_numpy(1.0 + (slot >= 32)).float()
    for h in range(nh):
        qkv.view(B, H * W, 3 * C)[:, :, 2 * C + 32 * h:2 * C + 32 * h + 32] = vcol
    qkv = bf(qkv.to(DEV))
    table = torch.zeros((2 * win[0] - 1) * (2 * win[1] - 1), nh, device=DEV)
    rel32 = torch.from_numpy(O.relative_position_index(*win)).to(DEV).to(torch.int32).contiguous()
    key = torch.tensor([counter], dtype=torch.int64, device=DEV)
    out = torch.empty(M, C, dtype=torch.bfloat16, device=DEV)
    ops.window_attn_fwd_drop(qkv, table, rel32, out, B, H, W, C, nh, win, (0, 0), 0, key, seed, site, p)
    unit = float(torch.tensor(float(D.scale(p)) / L).to(torch.bfloat16).float())
    o = out.float().cpu().view(B, H * W, nh, 32)[:, torch.from_numpy(idx.reshape(-1))].view(B * nW, L, nh, 32)
    code = torch.round(o / unit).to(torch.int64).permute(0, 2, 1, 3)         # [B nW, nh, query, d]
    keep = torch.from_numpy(D.keep(seed, counter, site, p, D.attn_index(B, H, W, nh, win)).astype(np.int64))
    want = keep[..., :32].clone()
    if L == 64:
        want += 2 * keep[..., 32:]
    assert torch.equal(code, want)


@pytest.mark.parametrize("win", [(4, 8), (2, 16), (8, 8), (1, 64)])
@pytest.mark.parametrize("C,nh", [(96, 3), (48, 3)])
def test_attn_drop_forms_in_band(win, C, nh):
    B, H, W = 2, 2 * win[0], 4 * win[1]
    L, LL = win[0] * win[1], (win[0] * win[1]) ** 2
    sft = (win[0] // 2, win[1] // 2)
    seed, counter, site, p = 0x5EED, 3, D.site(1, D.ATTN), 0.2
    M = B * H * W
    qkv = bf(rnd(M, 3 * C, scale=1.5))
    ntab = (2 * win[0] - 1) * (2 * win[1] - 1)
    table = rnd(ntab, nh, scale=0.5, seed=1)
    rel = torch.from_numpy(O.relative_position_index(*win)).to(DEV)
    rel32 = rel.to(torch.int32).contiguous()
    key = torch.tensor([counter], dtype=torch.int64, device=DEV)
    mult = _mask_tensor(seed, counter, site, p, B, H, W, nh, win)
    out = torch.empty(M, C, dtype=torch.bfloat16, device=DEV)
    ops.window_attn_fwd_drop(qkv, table, rel32, out, B, H, W, C, nh, win, sft, 1, key, seed, site, p)
    qr = qkv.float().requires_grad_(True)
    tr = table.clone().requires_grad_(True)
    ref = attn_reference(qr, tr, rel, B, H, W, C, nh, win, sft, drop_mult=mult)
    close(out, ref, 2 ** -7, 3e-3, "attn_drop fwd")
    dout = bf(rnd(M, C, seed=3))
    ref.backward(dout.float())
    dqkv = torch.empty_like(qkv)
    R = ops.window_attn_bwd_partial_rows(B, H, W, nh, win)
    part = torch.full((R * nh, LL), float("nan"), device=DEV)
    ops.window_attn_bwd_drop(qkv, dout, table, rel32, dqkv, part, B, H, W, C, nh, win, sft, 1, key, seed, site, p)
    close(dqkv, qr.grad, 2 ** -5, 6e-3, "attn_drop dqkv")
    close(fold_table(part, R, nh, LL, rel32, ntab), tr.grad, 2e-2, 5e-3, "attn_drop dtable")


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


@pytest.mark.parametrize("name", ["w4x8", "w2x16", "w8x8"])
def test_model_vs_reference_fixture(name):
    z = np.load(os.path.join(GOLD, "g15_windows.npz"), allow_pickle=False)
    with open(os.path.join(GOLD, "g15_windows.json")) as f:
        meta = json.load(f)
    cfg = O.TulipConfig(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in meta["configs"][name]["cfg"].items()})
    sd = O.key_seeded_state_dict(cfg, seed=meta["seed"])
    lo, hi = O.synthetic_batch(cfg, meta["batch"], seed=1234 + meta["seed"])
    P, grads = engine_step(build(cfg, sd), lo, hi, meta["batch"])
    loss = float(z[f"{name}::loss"])
    assert abs(P.losses[0].item() - loss) <= 1e-3 * loss, (P.losses[0].item(), loss)
    pred = P.pred.reshape(-1)[torch.from_numpy(z[f"{name}::pred_index"]).to(DEV)].cpu()
    assert rel_l2(pred, z[f"{name}::pred"]) <= 1e-2
    assert all(torch.isfinite(g).all() for g in grads.values())
    for k in meta["configs"][name]["grad_keys"]:
        e = rel_l2(grads[k], z[f"{name}::grad::{k}"])
        assert e <= (1e-1 if k.endswith("relative_position_bias_table") else 1.5e-2), (k, e)
    for k, step in meta["configs"][name]["grad_rows"].items():     # the last encoder block's qkv weight: the band of
        e = rel_l2(grads[k][::step], z[f"{name}::grad_rows::{k}"])    # the full-size gradient test (w4x8 measured 1.6e-2)
        assert e <= 2e-2, (k, e)
    for k, l2 in zip(z[f"{name}::grad_keys"].tolist(), z[f"{name}::grad_l2"]):
        tol = 1e-1 if k.endswith("relative_position_bias_table") else 1.5e-2
        assert abs(grads[k].double().norm().item() - l2) <= tol * l2 + 1e-9, (k, grads[k].double().norm().item(), l2)


@pytest.mark.parametrize("win", [(4, 8), (2, 16)])
def test_kitti_base_batch8_step_vs_oracle(win):
    cfg = O.tulip_base_config(window_size=win, drop_path_rate=0.0)
    sd = O.key_seeded_state_dict(cfg, seed=11)
    lo, hi = O.synthetic_batch(cfg, 8, seed=21)
    P, grads = engine_step(build(cfg, sd), lo, hi, 8)
    _, oloss, _, og = O.tulip_loss_and_grads(sd, cfg, lo, hi)
    assert abs(P.losses[0].item() - oloss.item()) <= 1e-3 * oloss.item()
    for n, g in grads.items():
        e = rel_l2(g, og[n])
        assert e <= (1e-1 if n.endswith("relative_position_bias_table") else 2e-2), (n, e)


def _kitti(win, seed=0):
    from tulip_amd.model import tulip as T
    torch.manual_seed(seed)
    return T.TULIP(img_size=(16, 1024), target_img_size=(64, 1024), patch_size=(1, 4), in_chans=1, window_size=list(win),
                   depths=(2, 2, 2, 2), embed_dim=96, num_heads=(3, 6, 12, 24), qkv_bias=True, mlp_ratio=4,
                   drop_path_rate=0.1, norm_layer=partial(nn.LayerNorm, eps=1e-6), pixel_shuffle=True,
                   circular_padding=True, log_transform=True, patch_unmerging=True).to(DEV)


def _kitti_batch(B=8):
    g = torch.Generator().manual_seed(1234)
    r = torch.rand(B, 1, 64, 1024, generator=g)
    r[torch.rand(B, 1, 64, 1024, generator=g) < 0.1] = 0
    hi = torch.log1p(r)
    return hi[:, :, 0::4, :].contiguous().to(DEV), hi.to(DEV)


@pytest.mark.parametrize("win", [(4, 8), (2, 16)])       # (8, 8) does not tile the 2x32 grid of stage 3 (the reference asserts)
def test_trainer_steps_are_bit_identical(win):
    """two Trainers from one state: the captured step equals the eager step bit for bit, and so does the next one"""
    from tulip_amd.trainer import Trainer
    lo, hi = _kitti_batch()
    ma = _kitti(win).train()
    mb = _kitti(win).train()
    mb.load_state_dict(ma.state_dict())
    ta = Trainer(ma, 8, use_graph=True)
    tb = Trainer(mb, 8, use_graph=False)
    for _ in range(2):
        la = ta.step(lo, hi).clone()
        lb = tb.step(lo, hi).clone()
        torch.cuda.synchronize()
        assert torch.isfinite(la).all()
        assert torch.equal(la, lb), (la, lb)
        assert torch.equal(ta.eng.params.flat, tb.eng.params.flat)


def test_trainer_accum_and_dropout_at_4x8():
    """accum_iter and drop_rate / attn_drop_rate run at a 32-token window: finite, and the captured step equals the eager one"""
    from tulip_amd.model import tulip as T
    from tulip_amd.trainer import Trainer

    def mk():
        torch.manual_seed(0)
        return T.TULIP(img_size=(16, 1024), target_img_size=(64, 1024), patch_size=(1, 4), in_chans=1, window_size=[4, 8],
                       depths=(2, 2, 2, 2), embed_dim=96, num_heads=(3, 6, 12, 24), qkv_bias=True, mlp_ratio=4,
                       drop_path_rate=0.1, drop_rate=0.1, attn_drop_rate=0.1, norm_layer=partial(nn.LayerNorm, eps=1e-6),
                       pixel_shuffle=True, circular_padding=True, log_transform=True, patch_unmerging=True).to(DEV).train()
    lo, hi = _kitti_batch()
    ma, mb = mk(), mk()
    ta = Trainer(ma, 8, use_graph=True, accum_iter=2)
    tb = Trainer(mb, 8, use_graph=False, accum_iter=2)
    for _ in range(2):
        la = ta.step(lo, hi).clone()
        lb = tb.step(lo, hi).clone()
        torch.cuda.synchronize()
        assert torch.isfinite(la).all() and torch.equal(la, lb), (la, lb)
    assert torch.equal(ta.eng.params.flat, tb.eng.params.flat)


def test_graphed_forward_equals_module_forward():
    from tulip_amd.infer import GraphedForward
    lo, hi = _kitti_batch()
    m = _kitti((4, 8)).eval()
    gf = GraphedForward(m, 8)
    with torch.no_grad():
        ref = m(lo, hi, mc_drop=True)
    for _ in range(2):
        a = gf(lo)
        torch.cuda.synchronize()
        assert torch.isfinite(a).all() and torch.equal(a, ref)


def test_refusals():
    from tulip_amd.model import tulip as T
    from tulip_amd.trainer import Trainer
    m = T.TULIP(img_size=(12, 384), target_img_size=(48, 384), patch_size=(1, 4), window_size=[3, 8], depths=(2, 2),
                embed_dim=48, num_heads=(3, 6), norm_layer=partial(nn.LayerNorm, eps=1e-6), pixel_shuffle=True,
                circular_padding=True, log_transform=True, patch_unmerging=True).to(DEV)
    with pytest.raises(NotImplementedError, match="16, 32 or 64"):
        m.engine()
    with pytest.raises(NotImplementedError, match="16-token windows only"):
        Trainer(_kitti((4, 8)).train(), 8, attn_fp8=True)
    fake = 4096
    from tulip_amd import _lib
    lib = _lib.load()
    assert lib.tulip_window_attn_fwd(fake, fake, fake, fake, 1, 3, 64, 96, 3, 3, 8, 0, 0, 0, None) == -1      # L = 24
    assert lib.tulip_window_attn_fwd(fake, fake, fake, fake, 1, 4, 64, 96, 3, 4, 8, 0, 0, 2, None) == -1      # fp8, L = 32

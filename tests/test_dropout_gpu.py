"""GPU: element dropout (drop_rate / attn_drop_rate; nn.Dropout at tulip.py:190-192, 315, 319, 705) on the HIP path.

  1. the mask kernels draw exactly the host definition (tulip_amd/dropout.py), keep 1-p of the elements and scale the kept
     ones by exactly fp32(1/(1-p));
  2. the tiny fixture g14_tiny_dropout (the reference with every nn.Dropout replaced by that mask at a fixed (seed, counter),
     DropPath on with injected draws): loss and gradients inside the bands of test_model_gpu.test_tiny_gradients_vs_reference;
  3. KITTI tulip_base with drop_rate = attn_drop_rate = 0.1, batch 8: the captured Trainer step equals the eager one bit for
     bit, every step draws new masks, and eval() takes the fused path (bit-identical to a p = 0 model);
  4. MC dropout: eval() + enable_dropout -> graph replays and the 8 tiles of one batch differ; eval() alone -> identical.
"""
import json
import os
import time
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
_T0 = time.time()


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_mask_kernels_match_host_definition(p):
    seed, counter = 0x0123456789ABCDEF, 41
    key = torch.tensor([counter], dtype=torch.int64, device=DEV)
    for site in (0, D.site(0, D.ATTN), D.site(3, D.PROJ), D.site(5, D.DROP1), D.site(7, D.DROP2)):
        n = (1 << 22) if site == 0 else (1 << 16)
        out = torch.empty(n, dtype=torch.float32, device=DEV)
        ops.dropout_mask(key, seed, site, p, n, out)
        got = out.cpu().numpy()
        want = D.multiplier(seed, counter, site, p, np.arange(n))
        assert np.array_equal(got, want), (site, p, int((got != want).sum()))
        if site == 0:
            k = (got != 0).mean()
            assert abs(k - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / n), (k, p)
    # in place on fp32 / bf16 rows with a pitch: kept values are exactly x * fp32(1/(1-p)), dropped ones 0
    rows, cols, ld = 1000, 96, 192
    x = torch.randn(rows, ld, device=DEV)
    y = x.clone()
    ops.dropout_scale(y, False, rows, cols, key, seed, 5, p, ld=ld)
    mult = torch.from_numpy(D.multiplier(seed, counter, 5, p, np.arange(rows * cols)).reshape(rows, cols))
    xc, yc = x.cpu(), y.cpu()
    assert torch.equal(yc[:, :cols], xc[:, :cols] * mult) and torch.equal(yc[:, cols:], xc[:, cols:])
    assert torch.equal(yc[:, :cols][mult != 0], xc[:, :cols][mult != 0] * torch.tensor(float(D.scale(p))))
    xb = x.to(torch.bfloat16)
    yb = xb.clone()
    ops.dropout_scale(yb, True, rows, cols, key, seed, 5, p, ld=ld)
    assert torch.equal(yb.cpu()[:, :cols], (xb.cpu().float()[:, :cols] * mult).to(torch.bfloat16))
    # the backward cast with a per-sample scale: bf16(dx * rowscale * mask)
    rs = torch.tensor([0.5, 2.0], device=DEV)
    dyb = torch.empty(rows, cols, dtype=torch.bfloat16, device=DEV)
    dx = x[:, :cols].contiguous()
    ops.dropout_cast(dx, dyb, rows, cols, rs, rows // 2, key, seed, 5, p)
    want = (dx.cpu() * rs.cpu().repeat_interleave(rows // 2)[:, None] * mult).to(torch.bfloat16)
    assert torch.equal(dyb.cpu(), want)


def _tiny_model(cfg, sd, p):
    from tulip_amd.model import tulip as T
    m = T.TULIP(img_size=cfg.img_size, target_img_size=cfg.target_img_size, patch_size=cfg.patch_size,
                in_chans=cfg.in_chans, embed_dim=cfg.embed_dim, window_size=list(cfg.window_size), depths=cfg.depths,
                num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio, drop_path_rate=cfg.drop_path_rate, drop_rate=p,
                attn_drop_rate=p, norm_layer=partial(nn.LayerNorm, eps=cfg.ln_eps), pixel_shuffle=cfg.pixel_shuffle,
                circular_padding=cfg.circular_padding, log_transform=cfg.log_transform, patch_unmerging=cfg.patch_unmerging)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).train()


def test_tiny_dropout_vs_reference_fixture():
    z = np.load(os.path.join(HERE, "golden", "g14_tiny_dropout.npz"), allow_pickle=False)
    with open(os.path.join(HERE, "golden", "g14_tiny_dropout.json")) as f:
        meta = json.load(f)
    cfg = O.TulipConfig(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in meta["cfg"].items()})
    sd = O.key_seeded_state_dict(cfg, seed=meta["seed"])
    lo, hi = O.synthetic_batch(cfg, meta["batch"], seed=1234 + meta["seed"])
    m = _tiny_model(cfg, sd, meta["drop_rate"])
    eng = m.engine()
    eng.bind(torch.device(DEV, torch.cuda.current_device()))
    eng._drop_seed = meta["mask_seed"]
    eng._drop_counter.fill_(meta["mask_counter"])
    P = eng.plan(meta["batch"])
    P.x_in.copy_(lo.to(DEV)); P.target.copy_(hi.to(DEV))
    eng.draw_drop_scales(P, True, torch.from_numpy(z["drop_u"]).to(DEV))
    eng.run_forward(P)
    torch.cuda.synchronize()
    assert int(P.drop_key.item()) == meta["mask_counter"] and int(eng._drop_counter.item()) == meta["mask_counter"] + 1
    assert abs(P.losses[0].item() - float(z["loss"])) <= 1e-3 * float(z["loss"]), (P.losses[0].item(), float(z["loss"]))
    gflat = torch.zeros(eng.params.total, device=DEV)
    eng.run_backward(P, gflat)
    torch.cuda.synchronize()
    W_ = eng.params
    grads = {n: gflat[W_.offset[n]:W_.offset[n] + W_.numel[n]].view(W_.shape[n]).cpu() for n in W_.names}
    assert all(torch.isfinite(g).all() for g in grads.values())
    checked = 0
    for k in z.files:
        if not k.startswith("grad::"):
            continue
        n = k[len("grad::"):]
        e = rel_l2(grads[n], torch.from_numpy(z[k]))
        assert e <= (1e-1 if n.endswith("relative_position_bias_table") else 1.5e-2), (n, e)
        checked += 1
    assert checked >= 40
    for n, l2 in zip(z["grad_keys"].tolist(), z["grad_l2"]):
        tol = 1e-1 if n.endswith("relative_position_bias_table") else 1.5e-2
        assert abs(grads[n].double().norm().item() - l2) <= tol * l2 + 1e-9, (n, grads[n].double().norm().item(), l2)


def _kitti(p, seed=0):
    from tulip_amd.model import tulip as T
    torch.manual_seed(seed)
    return T.TULIP(img_size=(16, 1024), target_img_size=(64, 1024), patch_size=(1, 4), in_chans=1, window_size=[2, 8],
                   depths=(2, 2, 2, 2), embed_dim=96, num_heads=(3, 6, 12, 24), qkv_bias=True, mlp_ratio=4,
                   drop_path_rate=0.1, drop_rate=p, attn_drop_rate=p, norm_layer=partial(nn.LayerNorm, eps=1e-6),
                   pixel_shuffle=True, circular_padding=True, log_transform=True, patch_unmerging=True).to(DEV)


def _kitti_batch(B=8):
    g = torch.Generator().manual_seed(1234)
    r = torch.rand(B, 1, 64, 1024, generator=g)
    r[torch.rand(B, 1, 64, 1024, generator=g) < 0.1] = 0
    hi = torch.log1p(r)
    return hi[:, :, 0::4, :].contiguous().to(DEV), hi.to(DEV)


def test_kitti_captured_step_with_dropout():
    from tulip_amd.trainer import Trainer
    lo, hi = _kitti_batch()
    ma, mb = _kitti(0.1).train(), _kitti(0.1).train()
    ta = Trainer(ma, 8, use_graph=True)
    tb = Trainer(mb, 8, use_graph=False)
    assert ta.eng._drop_seed == tb.eng._drop_seed and int(ta.eng._drop_counter.item()) == int(tb.eng._drop_counter.item())
    la = ta.step(lo, hi).clone()
    lb = tb.step(lo, hi).clone()
    torch.cuda.synchronize()
    assert torch.equal(la, lb), (la, lb)
    assert torch.equal(ta.eng.params.flat, tb.eng.params.flat)
    c0 = int(ta.eng._drop_counter.item())
    # learning rate 0: the weights stay, only the masks (and DropPath draws) of the next step change
    l1 = ta.step(lr=0.0).clone()
    l2 = ta.step(lr=0.0).clone()
    torch.cuda.synchronize()
    assert int(ta.eng._drop_counter.item()) == c0 + 2
    assert torch.isfinite(l1).all() and torch.isfinite(l2).all() and l1[0].item() != l2[0].item()
    # eval(): no dropout site is active -> the fused blocks run, bit-identical to the same weights without dropout
    m0 = _kitti(0.0)
    m0.load_state_dict(ma.state_dict())
    ma.eval(); m0.eval()
    with torch.no_grad():
        pa, la_, _ = ma(lo, hi)
        p0, l0_, _ = m0(lo, hi)
    assert torch.equal(pa, p0) and torch.equal(la_, l0_)


def test_mc_dropout_replays_draw_new_masks():
    from tulip_amd.evaluation import enable_dropout
    from tulip_amd.infer import GraphedForward
    lo, hi = _kitti_batch(1)
    m = _kitti(0.1).eval()
    gf = GraphedForward(m, 8)
    x = lo[:1].tile(8, 1, 1, 1)
    a = gf(x).clone()
    b = gf(x).clone()
    assert torch.equal(a, b) and all(torch.equal(a[0], a[i]) for i in range(1, 8))      # eval(): deterministic
    enable_dropout(m)
    c = gf(x).clone()
    d = gf(x).clone()
    assert not torch.equal(c, d)                                                          # each replay: new masks
    assert not any(torch.equal(c[0], c[i]) for i in range(1, 8))                         # the 8 tiles differ
    with torch.no_grad():
        preds = torch.cat([m(x, hi, mc_drop=True) for _ in range(2)])
    assert preds.std(0).max().item() > 0 and torch.isfinite(preds).all()
    m.eval()
    e = gf(x).clone()
    assert torch.equal(e, a)                                                              # back to the captured p = 0 form
    print(f"test_dropout_gpu wall time so far: {time.time() - _T0:.1f} s")

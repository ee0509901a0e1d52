"""CPU: attention windows of 32 and 64 tokens (window_size 4x8, 2x16, 8x8 and their (1, L) backup windows).

  1. the oracle reproduces the reference fixture g15_windows (tests/golden/make_golden_windows.py) for the three windows;
  2. the drop-in TULIP constructs at these windows with the reference's state_dict shapes, and its engine plans the
     backup window where the token grid is lower than the window;
  3. the host attn_drop index at L = 32 / 64;
  4. what is not built is refused before anything launches: other window lengths, fp8 scores at L != 16 (engine and C ABI).
"""
import json
import os
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import tulip_oracle as O
from tulip_amd import _lib
from tulip_amd import dropout as D

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
NAMES = ("w4x8", "w2x16", "w8x8")


def fixture():
    z = np.load(os.path.join(GOLD, "g15_windows.npz"), allow_pickle=False)
    with open(os.path.join(GOLD, "g15_windows.json")) as f:
        return z, json.load(f)


def fixture_config(meta, name) -> O.TulipConfig:
    return O.TulipConfig(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in meta["configs"][name]["cfg"].items()})


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def make_model(cfg: O.TulipConfig, **kw):
    from tulip_amd.model import tulip as T
    return T.TULIP(img_size=cfg.img_size, target_img_size=cfg.target_img_size, patch_size=cfg.patch_size,
                   in_chans=cfg.in_chans, embed_dim=cfg.embed_dim, window_size=list(cfg.window_size), depths=cfg.depths,
                   num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio, drop_path_rate=cfg.drop_path_rate,
                   norm_layer=partial(nn.LayerNorm, eps=cfg.ln_eps), pixel_shuffle=cfg.pixel_shuffle,
                   circular_padding=cfg.circular_padding, log_transform=cfg.log_transform,
                   patch_unmerging=cfg.patch_unmerging, **kw)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_reference_fixture(name):
    z, meta = fixture()
    cfg = fixture_config(meta, name)
    sd = O.key_seeded_state_dict(cfg, seed=meta["seed"])
    lo, hi = O.synthetic_batch(cfg, meta["batch"], seed=1234 + meta["seed"])
    pred, loss, pix, grads = O.tulip_loss_and_grads(sd, cfg, lo, hi)
    assert abs(loss.item() - float(z[f"{name}::loss"])) <= 1e-5 * float(z[f"{name}::loss"])
    assert abs(pix.item() - float(z[f"{name}::pixel_loss"])) <= 1e-5 * float(z[f"{name}::pixel_loss"])
    got = pred.reshape(-1)[torch.from_numpy(z[f"{name}::pred_index"])].numpy()
    assert np.abs(got - z[f"{name}::pred"]).max() <= 1e-5
    for k in meta["configs"][name]["grad_keys"]:
        assert rel_l2(grads[k], z[f"{name}::grad::{k}"]) <= 1e-4, k
    for k, step in meta["configs"][name]["grad_rows"].items():
        assert rel_l2(grads[k][::step], z[f"{name}::grad_rows::{k}"]) <= 1e-4, k
    for k, l2 in zip(z[f"{name}::grad_keys"].tolist(), z[f"{name}::grad_l2"]):
        assert abs(grads[k].double().norm().item() - l2) <= 1e-4 * l2 + 1e-12, k


@pytest.mark.parametrize("name", NAMES)
def test_tulip_constructs_with_reference_shapes(name):
    _, meta = fixture()
    cfg = fixture_config(meta, name)
    m = make_model(cfg)
    wh, ww = cfg.window_size
    L = wh * ww
    spec = O.state_dict_spec(cfg)
    sd = m.state_dict()
    assert list(sd.keys()) == list(spec.keys())
    for k, (shape, _) in spec.items():
        assert tuple(sd[k].shape) == tuple(shape), k
    blk = m.layers[0].blocks[0].attn
    assert tuple(blk.relative_position_bias_table.shape) == ((2 * wh - 1) * (2 * ww - 1), cfg.num_heads[0])
    assert tuple(blk.relative_position_index.shape) == (L, L)
    m.load_state_dict(O.key_seeded_state_dict(cfg, seed=meta["seed"]), strict=True)
    eng = m.engine()
    assert eng.win_len == L
    for sp in eng.blocks:
        win, sft = O.effective_window(sp.H, cfg.window_size, sp.shift)
        assert tuple(sp.win) == tuple(win) and tuple(sp.sft) == tuple(sft), sp.prefix
    if name != "w2x16":            # the last stage's grid is lower than the window: the (1, L) backup window
        assert any(tuple(sp.win) == (1, L) for sp in eng.blocks)
    # none of the fused block kernels take these windows: every block runs the unfused sequence
    assert all(eng._unfused(sp, meta["batch"]) for sp in eng.blocks)


@pytest.mark.parametrize("win", [(4, 8), (2, 16), (1, 32), (8, 8), (4, 16), (1, 64)])
def test_attn_drop_index_at_wide_windows(win):
    L = win[0] * win[1]
    B, H, W, nh = 2, 8, 128, 3
    idx = D.attn_index(B, H, W, nh, win)
    nW = (H // win[0]) * (W // win[1])
    assert idx.shape == (B * nW, nh, L, L)
    for w, h, q, k in [(0, 0, 0, 0), (B * nW - 1, 2, L - 1, L - 1), (5, 1, 7, L // 2 + 3)]:
        assert idx[w, h, q, k] == ((w * nh + h) * L + q) * L + k


def test_other_window_lengths_refused():
    cfg = O.tiny_config(window_size=(3, 8), img_size=(6, 384), target_img_size=(24, 384))
    m = make_model(cfg)
    with pytest.raises(NotImplementedError, match="16, 32 or 64"):
        m.engine()


def test_token_grid_not_divisible_still_refused():
    cfg = O.tiny_config(window_size=(4, 8), img_size=(8, 240), target_img_size=(32, 240), depths=(2, 2), num_heads=(3, 6))
    with pytest.raises(NotImplementedError, match="not divisible"):
        make_model(cfg).engine()


def test_fp8_scores_refused_at_wide_windows(monkeypatch):
    _, meta = fixture()
    eng = make_model(fixture_config(meta, "w4x8")).engine()
    eng.check_attn_fp8()                       # off: nothing to refuse
    eng.attn_fp8 = True
    with pytest.raises(NotImplementedError, match="16-token windows only"):
        eng.check_attn_fp8()
    with pytest.raises(NotImplementedError, match="16-token windows only"):
        eng.run_forward(None)                  # refused before the plan is touched


def test_abi_refuses_unbuilt_windows_before_launching():
    """argument checks run on the host before any launch: no GPU needed"""
    lib = _lib.load()
    assert lib.tulip_abi_version() == 6
    fake = 4096
    # (B, H, W, C, nh, wh, ww, sh, sw, masked): L = 24 is not built, fp8 scores (masked bit 1) only at L = 16
    for geo in [(1, 3, 64, 96, 3, 3, 8, 0, 0, 0), (1, 4, 64, 96, 3, 4, 8, 0, 0, 2), (1, 8, 64, 96, 3, 8, 8, 0, 0, 2),
                (1, 4, 64, 96, 3, 4, 6, 0, 0, 0)]:
        assert lib.tulip_window_attn_fwd(fake, fake, fake, fake, *geo, None) == -1, geo
        assert lib.tulip_window_attn_bwd(fake, fake, fake, fake, fake, fake, *geo, None) == -1, geo
        assert lib.tulip_window_attn_fwd_drop(fake, fake, fake, fake, *geo, fake, 1, 1, 0.1, None) == -1, geo
        assert lib.tulip_window_attn_bwd_drop(fake, fake, fake, fake, fake, fake, *geo, fake, 1, 1, 0.1, None) == -1, geo
    # head dims other than 16 / 32 and grids the window does not tile stay refused at L = 32 / 64
    assert lib.tulip_window_attn_fwd(fake, fake, fake, fake, 1, 4, 64, 192, 3, 4, 8, 0, 0, 0, None) == -1
    assert lib.tulip_window_attn_fwd(fake, fake, fake, fake, 1, 4, 60, 96, 3, 4, 8, 0, 0, 0, None) == -1
    # empty batches are accepted (no launch) at the new lengths
    assert lib.tulip_window_attn_fwd(fake, fake, fake, fake, 0, 4, 64, 96, 3, 4, 8, 0, 0, 1, None) == 0
    assert lib.tulip_window_attn_bwd(fake, fake, fake, fake, fake, fake, 0, 8, 64, 96, 6, 8, 8, 4, 4, 1, None) == 0


def test_bias_partial_rows_bound():
    lib = _lib.load()
    assert lib.tulip_window_attn_bwd_partial_rows(8, 16, 256, 3, 2, 8) >= 1      # the 16-token sizing is unchanged
    for (B, H, W, nh, wh, ww) in [(8, 16, 256, 3, 4, 8), (8, 16, 256, 3, 2, 16), (8, 16, 256, 3, 8, 8), (1, 1, 32, 48, 1, 32),
                                  (64, 4, 64, 24, 1, 64), (1, 8, 8, 1, 8, 8)]:
        L = wh * ww
        R = lib.tulip_window_attn_bwd_partial_rows(B, H, W, nh, wh, ww)
        windows = B * (H // wh) * (W // ww)
        assert 1 <= R <= max(1, 512 // nh), (B, H, W, nh, wh, ww)
        assert R <= (windows + 64 // L - 1) // (64 // L)                      # every group has a window
        assert R * nh * L * L * 4 <= (8 << 20)

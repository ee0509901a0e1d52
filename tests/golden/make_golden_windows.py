"""Regenerate tests/golden/g15_windows.{npz,json}: the reference TULIP at three attention windows other than 16 tokens,
tiny widths (embed 48, patch_size (1, 4)), train mode with DropPath off:

    w4x8   window (4, 8) on an 8x512 image, 3 stages -- the last stage (2x32 tokens) takes the (1, 32) backup window;
    w2x16  window (2, 16) on 8x256, 2 stages;
    w8x8   window (8, 8) on 16x1024, 3 stages -- the last stage (4x64 tokens) takes the (1, 64) backup window.

Per config: loss, pixel loss, a fixed subsample of the prediction, the gradient norm of every parameter, and the
gradients of every stage's relative_position_bias_table, the qkv weight of the first encoder block, every QKV_ROW_STEP-th
row of the qkv weight of the last encoder block (the one that runs the backup window) and patch_embed.proj.weight.
Imports the reference exactly as make_golden.py does.  Data only:
nothing of the reference is stored but its outputs.

    python tests/golden/make_golden_windows.py
"""
import json
import os
import sys
from functools import partial

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import import_reference  # noqa: E402
from oracle import tulip_oracle as O  # noqa: E402

NAME = "g15_windows"
BATCH, SEED, NPRED = 2, 3, 4096
QKV_ROW_STEP = 6
CONFIGS = {
    "w4x8": dict(img_size=(8, 512), target_img_size=(32, 512), window_size=(4, 8), depths=(2, 2, 2), num_heads=(3, 6, 12)),
    "w2x16": dict(img_size=(8, 256), target_img_size=(32, 256), window_size=(2, 16), depths=(2, 2), num_heads=(3, 6)),
    "w8x8": dict(img_size=(16, 1024), target_img_size=(64, 1024), window_size=(8, 8), depths=(2, 2, 2), num_heads=(3, 6, 12)),
}


def config(name: str) -> O.TulipConfig:
    return O.tiny_config(drop_path_rate=0.0, **CONFIGS[name])


def grad_keys(cfg: O.TulipConfig):
    keys = ["patch_embed.proj.weight"]
    for s in range(cfg.num_layers):
        keys += [f"layers.{s}.blocks.{b}.attn.relative_position_bias_table" for b in range(cfg.depths[s])]
    for s in range(cfg.num_layers - 1):
        i = cfg.num_layers - s - 2
        keys += [f"layers_up.{i}.blocks.{b}.attn.relative_position_bias_table" for b in range(cfg.depths[s])]
    keys += ["layers.0.blocks.0.attn.qkv.weight"]
    return keys


def backup_qkv_key(cfg: O.TulipConfig) -> str:
    return f"layers.{cfg.num_layers - 1}.blocks.1.attn.qkv.weight"


def pred_index(n: int) -> np.ndarray:
    return np.random.default_rng(15).choice(n, size=min(NPRED, n), replace=False).astype(np.int64)


def main():
    T = import_reference()
    out, meta = {}, {"name": NAME, "batch": BATCH, "seed": SEED, "configs": {}}
    for name in CONFIGS:
        cfg = config(name)
        sd = O.key_seeded_state_dict(cfg, seed=SEED)
        lo, hi = O.synthetic_batch(cfg, BATCH, seed=1234 + SEED)
        ref = T.TULIP(img_size=cfg.img_size, target_img_size=cfg.target_img_size, patch_size=cfg.patch_size,
                      in_chans=cfg.in_chans, embed_dim=cfg.embed_dim, window_size=list(cfg.window_size),
                      depths=cfg.depths, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio, qkv_bias=True,
                      drop_path_rate=cfg.drop_path_rate, norm_layer=partial(nn.LayerNorm, eps=cfg.ln_eps),
                      pixel_shuffle=cfg.pixel_shuffle, circular_padding=cfg.circular_padding,
                      log_transform=cfg.log_transform, patch_unmerging=cfg.patch_unmerging)
        ref.load_state_dict(sd, strict=True)
        ref.train()
        ref.zero_grad()
        pred, loss, pix = ref(lo, hi)
        loss.backward()
        grads = {k: p.grad.detach().clone() for k, p in ref.named_parameters()}
        idx = pred_index(pred.numel())
        out[f"{name}::loss"] = np.float64(loss.item())
        out[f"{name}::pixel_loss"] = np.float64(pix.item())
        out[f"{name}::pred_index"] = idx
        out[f"{name}::pred"] = pred.detach().reshape(-1)[torch.from_numpy(idx)].numpy().copy()
        out[f"{name}::grad_keys"] = np.array(list(grads.keys()))
        out[f"{name}::grad_l2"] = np.array([grads[k].double().norm().item() for k in grads])
        keys = grad_keys(cfg)
        for k in keys:
            out[f"{name}::grad::{k}"] = grads[k].numpy().copy()
        kb = backup_qkv_key(cfg)
        out[f"{name}::grad_rows::{kb}"] = grads[kb][::QKV_ROW_STEP].numpy().copy()
        meta["configs"][name] = {"cfg": cfg.__dict__, "grad_keys": keys, "grad_rows": {kb: QKV_ROW_STEP}}
        print(f"{NAME}/{name}: loss {loss.item():.6f} pixel {pix.item():.6f}, {len(keys)} gradient tensors stored")
    np.savez_compressed(os.path.join(HERE, NAME + ".npz"), **out)
    with open(os.path.join(HERE, NAME + ".json"), "w") as f:
        json.dump(meta, f, indent=1, default=list)


if __name__ == "__main__":
    main()

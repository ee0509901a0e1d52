"""Regenerate tests/golden/g16_inchans.{npz,json}: the reference TULIP on multi-channel images (in_chans 2, 3, 4), tiny
widths (embed 48, patch_size (1, 4)), batch 2, train mode with DropPath off:

    c2  in_chans 2, pixel shuffle, circular padding, patch unmerging, log_transform;
    c3  in_chans 3, pixel_shuffle=False (FinalPatchExpanding), patch_unmerging=False, no circular padding;
    c4  in_chans 4, window (4, 8): the 32-token attention path and 32 patch-embedding taps.

Per config: loss, pixel loss, a fixed subsample of the prediction taken from every channel, and the gradients of
patch_embed.proj.weight, decoder_pred.weight, the head's expand bias and norm_up.weight, plus every EXPAND_ROW_STEP-th row
of the head's expand weight gradient (the whole tensor would take the fixture past its size budget).  Also the reference's
seeded initial patch_embed.proj.weight / decoder_pred.weight at in_chans 2 (torch.manual_seed(0), the c2 constructor).
Imports the reference exactly as make_golden.py does.  Data only: nothing of the reference is stored but its outputs.

    python tests/golden/make_golden_inchans.py
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

NAME = "g16_inchans"
BATCH, SEED, NPRED_PER_CHANNEL = 2, 5, 1024
EXPAND_ROW_STEP = 4
CONFIGS = {
    "c2": dict(in_chans=2, pixel_shuffle=True, circular_padding=True, patch_unmerging=True, log_transform=True),
    "c3": dict(in_chans=3, pixel_shuffle=False, circular_padding=False, patch_unmerging=False, log_transform=True),
    "c4": dict(in_chans=4, window_size=(4, 8)),
}


def config(name: str) -> O.TulipConfig:
    return O.tiny_config(drop_path_rate=0.0, **CONFIGS[name])


def grad_keys(cfg: O.TulipConfig):
    head = ["ps_head.conv_expand.0.bias"] if cfg.pixel_shuffle else []
    return ["patch_embed.proj.weight", "decoder_pred.weight"] + head + ["norm_up.weight"]


def expand_key(cfg: O.TulipConfig) -> str:
    return "ps_head.conv_expand.0.weight" if cfg.pixel_shuffle else "final_patch_expanding.expand.weight"


def pred_index(shape) -> np.ndarray:
    """flat indices into pred (B, C, H, W): NPRED_PER_CHANNEL fixed positions in every channel plane of every sample"""
    B, C, H, W = shape
    pos = np.random.default_rng(16).choice(H * W, size=min(NPRED_PER_CHANNEL, H * W), replace=False).astype(np.int64)
    return np.concatenate([(b * C + c) * H * W + pos for b in range(B) for c in range(C)])


def ref_model(T, cfg: O.TulipConfig):
    return T.TULIP(img_size=cfg.img_size, target_img_size=cfg.target_img_size, patch_size=cfg.patch_size,
                   in_chans=cfg.in_chans, embed_dim=cfg.embed_dim, window_size=list(cfg.window_size),
                   depths=cfg.depths, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio, qkv_bias=True,
                   drop_path_rate=cfg.drop_path_rate, norm_layer=partial(nn.LayerNorm, eps=cfg.ln_eps),
                   pixel_shuffle=cfg.pixel_shuffle, circular_padding=cfg.circular_padding,
                   log_transform=cfg.log_transform, patch_unmerging=cfg.patch_unmerging)


def main():
    T = import_reference()
    out, meta = {}, {"name": NAME, "batch": BATCH, "seed": SEED, "configs": {}}
    for name in CONFIGS:
        cfg = config(name)
        sd = O.key_seeded_state_dict(cfg, seed=SEED)
        lo, hi = O.synthetic_batch(cfg, BATCH, seed=1234 + SEED)
        ref = ref_model(T, cfg)
        ref.load_state_dict(sd, strict=True)
        ref.train()
        ref.zero_grad()
        pred, loss, pix = ref(lo, hi)
        loss.backward()
        grads = {k: p.grad.detach().clone() for k, p in ref.named_parameters()}
        idx = pred_index(tuple(pred.shape))
        out[f"{name}::loss"] = np.float64(loss.item())
        out[f"{name}::pixel_loss"] = np.float64(pix.item())
        out[f"{name}::pred_shape"] = np.array(pred.shape, dtype=np.int64)
        out[f"{name}::pred_index"] = idx
        out[f"{name}::pred"] = pred.detach().reshape(-1)[torch.from_numpy(idx)].numpy().copy()
        keys = grad_keys(cfg)
        for k in keys:
            out[f"{name}::grad::{k}"] = grads[k].numpy().copy()
        ke = expand_key(cfg)
        out[f"{name}::grad_rows::{ke}"] = grads[ke][::EXPAND_ROW_STEP].numpy().copy()
        meta["configs"][name] = {"cfg": cfg.__dict__, "grad_keys": keys, "grad_rows": {ke: EXPAND_ROW_STEP}}
        print(f"{NAME}/{name}: loss {loss.item():.6f} pixel {pix.item():.6f}, pred {tuple(pred.shape)}")
    # the seeded initialisation at in_chans 2 (same registration + init order => same weights)
    cfg = config("c2")
    torch.manual_seed(0)
    sd = ref_model(T, cfg).state_dict()
    for k in ("patch_embed.proj.weight", "decoder_pred.weight"):
        out[f"init_c2::{k}"] = sd[k].numpy().copy()
    np.savez_compressed(os.path.join(HERE, NAME + ".npz"), **out)
    with open(os.path.join(HERE, NAME + ".json"), "w") as f:
        json.dump(meta, f, indent=1, default=list)


if __name__ == "__main__":
    main()

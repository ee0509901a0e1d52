"""Regenerate tests/golden/g17_upscale.{npz,json}: the reference TULIP at upscale_factor 8, i.e. 16-pixel patches
((2, 8) and (4, 4)), tiny widths (embed 48, depths (2, 2)), batch 2, train mode with DropPath off.  The five
configurations and their batches are tests/upscale_cases.py:

    ps8_p2x8      (2, 8) patches, 16x512 -> 64x512, pixel shuffle, circular padding, patch unmerging, log transform;
    fe8_p2x8      the same image through FinalPatchExpanding / PatchExpanding;
    ps8_p4x4      (4, 4) patches, 16x256 -> 32x512, pixel shuffle, no circular padding;
    fe8_defaults  (4, 4) patches, 32x256 -> 64x512, the reference constructor's default flags (window 4, LayerNorm eps 1e-5);
    ps8_p2x8_c2   ps8_p2x8 with in_chans 2 (32 patch-embedding taps).

Per config: loss, pixel loss, a fixed subsample of the prediction, the gradient norm of every parameter, and the
gradients of patch_embed.proj.weight, decoder_pred.weight and every EXPAND_ROW_STEP-th row of the head's expand weight.
Also the reference's seeded initial patch_embed.proj.weight and ps_head.conv_expand.0.weight rows at patch_size (2, 8)
(torch.manual_seed(0), the ps8_p2x8 constructor).  Imports the reference exactly as make_golden.py does.  Data only:
nothing of the reference is stored but its outputs.

    python tests/golden/make_golden_upscale.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import import_reference  # noqa: E402
from oracle import tulip_oracle as O  # noqa: E402
from tests import upscale_cases as UC  # noqa: E402

NAME = "g17_upscale"
NPRED = 4096
EXPAND_ROW_STEP = 8
INIT_KEYS = ("patch_embed.proj.weight", "ps_head.conv_expand.0.weight")
INIT_ROW_STEP = 16


def pred_index(n: int) -> np.ndarray:
    return np.random.default_rng(17).choice(n, size=min(NPRED, n), replace=False).astype(np.int64)


def main():
    T = import_reference()
    out, meta = {}, {"name": NAME, "batch": UC.BATCH, "seed": UC.SEED, "configs": {}}
    for name in UC.NAMES:
        cfg = UC.config(name)
        UC.check_config(cfg)
        sd = O.key_seeded_state_dict(cfg, seed=UC.SEED)
        lo, hi = UC.batch(cfg, UC.BATCH, seed=1234 + UC.SEED)
        ref = T.TULIP(qkv_bias=True, **UC.model_kwargs(cfg))
        assert ref.upscale_factor == 8
        ref.load_state_dict(sd, strict=True)
        ref.train()
        ref.zero_grad()
        assert tuple(lo.shape) == (UC.BATCH, cfg.in_chans) + tuple(cfg.img_size)
        pred, loss, pix = ref(lo, hi)
        # forward_loss broadcasts silently: the target must have the prediction's shape
        assert tuple(pred.shape) == tuple(hi.shape) == (UC.BATCH, cfg.in_chans) + UC.output_size(cfg), (pred.shape, hi.shape)
        loss.backward()
        grads = {k: p.grad.detach().clone() for k, p in ref.named_parameters()}
        idx = pred_index(pred.numel())
        out[f"{name}::loss"] = np.float64(loss.item())
        out[f"{name}::pixel_loss"] = np.float64(pix.item())
        out[f"{name}::pred_shape"] = np.array(pred.shape, dtype=np.int64)
        out[f"{name}::pred_index"] = idx
        out[f"{name}::pred"] = pred.detach().reshape(-1)[torch.from_numpy(idx)].numpy().copy()
        out[f"{name}::grad_keys"] = np.array(list(grads.keys()))
        out[f"{name}::grad_l2"] = np.array([grads[k].double().norm().item() for k in grads])
        keys = ["patch_embed.proj.weight", "decoder_pred.weight"]
        for k in keys:
            out[f"{name}::grad::{k}"] = grads[k].numpy().copy()
        ke = UC.expand_key(cfg)
        out[f"{name}::grad_rows::{ke}"] = grads[ke][::EXPAND_ROW_STEP].numpy().copy()
        meta["configs"][name] = {"cfg": cfg.__dict__, "grad_keys": keys, "grad_rows": {ke: EXPAND_ROW_STEP}}
        print(f"{NAME}/{name}: loss {loss.item():.6f} pixel {pix.item():.6f}, pred {tuple(pred.shape)}")
    # the seeded initialisation at patch_size (2, 8) (same registration + init order => same weights)
    cfg = UC.config("ps8_p2x8")
    torch.manual_seed(0)
    sd = T.TULIP(qkv_bias=True, **UC.model_kwargs(cfg)).state_dict()
    for k in INIT_KEYS:
        out[f"init_ps8_p2x8::{k}"] = sd[k][::INIT_ROW_STEP if sd[k].shape[0] > 48 else 1].numpy().copy()
    meta["init_row_step"] = INIT_ROW_STEP
    np.savez_compressed(os.path.join(HERE, NAME + ".npz"), **out)
    with open(os.path.join(HERE, NAME + ".json"), "w") as f:
        json.dump(meta, f, indent=1, default=list)


if __name__ == "__main__":
    main()

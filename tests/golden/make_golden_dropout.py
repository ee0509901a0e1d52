"""Regenerate tests/golden/g14_tiny_dropout.{npz,json}: the reference TULIP (tiny config of g3_tiny_droppath) with element
dropout on (drop_rate = attn_drop_rate = 0.1) and DropPath on with injected draws, every nn.Dropout replaced by the
counter-based mask of tulip_amd/dropout.py at a fixed (seed, counter), each site with its index map (the roll and window
partition for proj_drop, the [B * nW, nh, N, N] flattening for attn_drop).  Imports the reference exactly as make_golden.py
does.  Data only: nothing of the reference is stored but its outputs.

    python tests/golden/make_golden_dropout.py
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
from tulip_amd import dropout as D  # noqa: E402

NAME = "g14_tiny_dropout"
SEED, COUNTER = 0x5EED_1234_ABCD, 7
P_DROP = 0.1
MASK_PS = (0.1, 0.5)


class _InjectedDropPath(nn.Module):
    """DropPath with given per-sample multipliers; called twice per block (attention branch, then MLP branch)."""

    def __init__(self, scales):           # [2][B]
        super().__init__()
        self.scales, self.calls = scales, 0

    def forward(self, x):
        s = self.scales[self.calls % 2]
        self.calls += 1
        return x * s.view(-1, *([1] * (x.dim() - 1)))


def _index_fn(kind, sp, B, C):
    if kind == D.ATTN:
        return lambda shape: D.attn_index(B, sp.H, sp.W, sp.nh, sp.win).reshape(shape)
    if kind == D.PROJ:          # [B nW, wh, ww, C] rolled + partitioned -> natural row * C + c
        rows = D.window_rows(B, sp.H, sp.W, sp.win, sp.sft).astype(np.uint64)
        return lambda shape: (rows[:, :, None] * np.uint64(C) + np.arange(C, dtype=np.uint64)).reshape(shape)
    return lambda shape: np.arange(int(np.prod(shape)), dtype=np.uint64).reshape(shape)     # natural [B, H, W, C]


def _patch_dropout(mod, site_id, index_fn):
    def forward(x):
        if not mod.training or mod.p == 0.0:
            return x
        m = D.multiplier(SEED, COUNTER, site_id, mod.p, index_fn(tuple(x.shape)))
        return x * torch.from_numpy(m)
    mod.forward = forward


def main():
    T = import_reference()
    cfg = O.tiny_config()
    batch, seed = 4, 1
    sd = O.key_seeded_state_dict(cfg, seed=seed)
    lo, hi = O.synthetic_batch(cfg, batch, seed=1234 + seed)
    ref = T.TULIP(img_size=cfg.img_size, target_img_size=cfg.target_img_size, patch_size=cfg.patch_size,
                  in_chans=cfg.in_chans, embed_dim=cfg.embed_dim, window_size=list(cfg.window_size),
                  depths=cfg.depths, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio, qkv_bias=True,
                  drop_rate=P_DROP, attn_drop_rate=P_DROP, drop_path_rate=cfg.drop_path_rate,
                  norm_layer=partial(nn.LayerNorm, eps=cfg.ln_eps), pixel_shuffle=cfg.pixel_shuffle,
                  circular_padding=cfg.circular_padding, log_transform=cfg.log_transform,
                  patch_unmerging=cfg.patch_unmerging)
    ref.load_state_dict(sd, strict=True)
    ref.train()

    # block geometry / order and DropPath slots from the engine's own block list (no GPU needed to build it)
    from tulip_amd.model import tulip as TA
    ours = TA.TULIP(img_size=cfg.img_size, target_img_size=cfg.target_img_size, patch_size=cfg.patch_size,
                    in_chans=cfg.in_chans, embed_dim=cfg.embed_dim, window_size=list(cfg.window_size), depths=cfg.depths,
                    num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio, drop_rate=P_DROP, attn_drop_rate=P_DROP,
                    drop_path_rate=cfg.drop_path_rate, norm_layer=partial(nn.LayerNorm, eps=cfg.ln_eps),
                    pixel_shuffle=cfg.pixel_shuffle, circular_padding=cfg.circular_padding,
                    log_transform=cfg.log_transform, patch_unmerging=cfg.patch_unmerging)
    from tulip_amd.engine import TulipEngine
    eng = TulipEngine(ours)
    g = torch.Generator().manual_seed(4321)
    drop_u = torch.rand(eng.n_drop_slots, batch, generator=g)
    B = batch
    _patch_dropout(ref.pos_drop, 0, lambda shape: np.arange(int(np.prod(shape)), dtype=np.uint64).reshape(shape))
    for sp in eng.blocks:
        blk = ref.get_submodule(sp.prefix)
        if sp.slot >= 0:
            keep = 1.0 - sp.rate
            u = drop_u[sp.slot:sp.slot + 2]
            blk.drop_path = _InjectedDropPath(torch.floor(keep + u) / keep)
        for kind, mod in ((D.ATTN, blk.attn.attn_drop), (D.PROJ, blk.attn.proj_drop), (D.DROP1, blk.mlp.drop1),
                          (D.DROP2, blk.mlp.drop2)):
            _patch_dropout(mod, D.site(sp.idx, kind), _index_fn(kind, sp, B, sp.C))

    ref.zero_grad()
    pred, loss, pix = ref(lo, hi)
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in ref.named_parameters()}
    out = {"drop_u": drop_u.numpy(), "loss": np.float64(loss.item()), "pixel_loss": np.float64(pix.item()),
           "pred": pred.detach().numpy().copy()}
    out["grad_keys"] = np.array(list(grads.keys()))
    out["grad_l2"] = np.array([grads[k].double().norm().item() for k in grads])
    keys = ["patch_embed.proj.weight", "patch_embed.norm.weight", "skip_connection_layers.0.weight", "norm_up.weight"]
    for sp in eng.blocks:      # every block: the small tensors of each kind; the weight matrices of the first and the last block
        keys += [sp.prefix + s for s in (".attn.qkv.bias", ".attn.proj.bias", ".mlp.fc1.bias", ".mlp.fc2.bias",
                                         ".norm1.weight", ".norm2.bias", ".attn.relative_position_bias_table")]
        if sp.idx in (0, len(eng.blocks) - 1):
            keys += [sp.prefix + s for s in (".attn.qkv.weight", ".attn.proj.weight", ".mlp.fc1.weight", ".mlp.fc2.weight")]
    for k in keys:
        out["grad::" + k] = grads[k].numpy().copy()
    # packed keep masks: pos_drop and the four kinds of block 0 at two probabilities, 8192 elements each
    n = 8192
    for p in MASK_PS:
        for site_id in (0, D.site(0, D.ATTN), D.site(0, D.PROJ), D.site(0, D.DROP1), D.site(0, D.DROP2)):
            out[f"mask::{site_id}::{p}"] = np.packbits(D.keep(SEED, COUNTER, site_id, p, np.arange(n)))
    print(f"{NAME}: loss {loss.item():.6f} pixel {pix.item():.6f}, {len(keys)} gradient tensors stored")
    np.savez_compressed(os.path.join(HERE, NAME + ".npz"), **out)
    meta = {"name": NAME, "batch": batch, "seed": seed, "cfg": cfg.__dict__, "drop_path": True, "drop_rate": P_DROP,
            "attn_drop_rate": P_DROP, "mask_seed": SEED, "mask_counter": COUNTER, "mask_n": n, "mask_ps": list(MASK_PS)}
    with open(os.path.join(HERE, NAME + ".json"), "w") as f:
        json.dump(meta, f, indent=1, default=list)


if __name__ == "__main__":
    main()

"""upscale_factor 8 (patch sizes (2, 8) and (4, 4)): the five tiny configurations of tests/golden/g17_upscale and their
batches, shared by tests/golden/make_golden_upscale.py, tests/test_upscale_cpu.py and tests/test_upscale_gpu.py.

The output image of TULIP is grid * upscale_factor (tulip.py:727-731), not target_img_size: the two differ for the
(4, 4)-patch models here, whose target is twice as wide as the input.  `batch` therefore draws the target at the output
size (the same generator sequence as oracle.tulip_oracle.synthetic_batch) and sub-samples rows AND columns for the input.
"""
from functools import partial

import torch
import torch.nn as nn

from oracle import tulip_oracle as O

BATCH, SEED = 2, 7
CONFIGS = {
    "ps8_p2x8": dict(patch_size=(2, 8), img_size=(16, 512), target_img_size=(64, 512)),
    "fe8_p2x8": dict(patch_size=(2, 8), img_size=(16, 512), target_img_size=(64, 512), pixel_shuffle=False,
                     patch_unmerging=False),
    "ps8_p4x4": dict(patch_size=(4, 4), img_size=(16, 256), target_img_size=(32, 512), circular_padding=False),
    # the reference constructor's default flags (tulip.py:531-535) on a small image
    "fe8_defaults": dict(patch_size=(4, 4), img_size=(32, 256), target_img_size=(64, 512), window_size=(4, 4), ln_eps=1e-5,
                         pixel_shuffle=False, circular_padding=False, log_transform=False, patch_unmerging=False),
    "ps8_p2x8_c2": dict(patch_size=(2, 8), img_size=(16, 512), target_img_size=(64, 512), in_chans=2),
}
NAMES = tuple(CONFIGS)


def config(name: str) -> O.TulipConfig:
    return O.tiny_config(drop_path_rate=0.0, **CONFIGS[name])


def output_size(cfg: O.TulipConfig):
    r = cfg.upscale_factor
    return cfg.grid[0] * r, cfg.grid[1] * r


def batch(cfg: O.TulipConfig, n: int, seed: int):
    """(lo, hi): hi (n, in_chans, grid * r) as synthetic_batch draws it, lo its row / column sub-sample at img_size"""
    Ho, Wo = output_size(cfg)
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(n, cfg.in_chans, Ho, Wo, generator=g)
    r[torch.rand(n, cfg.in_chans, Ho, Wo, generator=g) < 0.1] = 0
    hi = torch.log1p(r)
    assert Ho % cfg.img_size[0] == 0 and Wo % cfg.img_size[1] == 0
    lo = hi[:, :, 0::Ho // cfg.img_size[0], 0::Wo // cfg.img_size[1]].contiguous()
    return lo, hi


def check_config(cfg: O.TulipConfig):
    """upscale_factor 8, and every stage's token grid is tiled by its (effective) window"""
    assert cfg.upscale_factor == 8, cfg
    for s in range(cfg.num_layers):
        H, W = cfg.grid[0] >> s, cfg.grid[1] >> s
        assert (H << s, W << s) == tuple(cfg.grid)
        win, _ = O.effective_window(H, cfg.window_size, False)
        assert H % win[0] == 0 and W % win[1] == 0, (cfg, s)


def expand_key(cfg: O.TulipConfig) -> str:
    return "ps_head.conv_expand.0.weight" if cfg.pixel_shuffle else "final_patch_expanding.expand.weight"


def model_kwargs(cfg: O.TulipConfig) -> dict:
    """constructor arguments shared by the reference TULIP and tulip_amd's"""
    return dict(img_size=cfg.img_size, target_img_size=cfg.target_img_size, patch_size=cfg.patch_size,
                in_chans=cfg.in_chans, embed_dim=cfg.embed_dim, window_size=list(cfg.window_size), depths=cfg.depths,
                num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio, drop_path_rate=cfg.drop_path_rate,
                norm_layer=partial(nn.LayerNorm, eps=cfg.ln_eps), pixel_shuffle=cfg.pixel_shuffle,
                circular_padding=cfg.circular_padding, log_transform=cfg.log_transform,
                patch_unmerging=cfg.patch_unmerging)

"""The launch sequence of every Swin block route, as dry-run logs (tests/dry_run.py): a matrix of (model, batch size, engine knobs,
dropout state, form) scenarios, each one run_forward (+ run_backward) on a CPU-bound engine.  A change of the engine's host code
that is meant to leave every launch as it is shows that by equal logs before and after it:

    python tests/block_routes.py [scenario ...]     prints scenario, entry count and SHA-256 of each log (DRY_RUN_DUMP=dir: also
                                                    writes dir/<scenario>.log)

Forms: "train" = run_forward(with_loss=True, defer_loss_final=True) + run_backward, "train_ow" = the same with overwrite=True,
"infer" = run_forward(with_loss=False).  tests/test_block_routes_cpu.py reads the route rules off a part of the matrix.
"""
import functools
import os
import sys
from functools import partial

import torch
import torch.nn as nn

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dry_run import dry_run
from oracle import tulip_oracle as O
from tulip_amd.engine import TulipEngine
from tulip_amd.model import tulip as T

KW = dict(patch_size=(1, 4), in_chans=1, window_size=[2, 8], pixel_shuffle=True, circular_padding=True,
          log_transform=True, patch_unmerging=True)


def _base(**kw):
    """tulip_base (tulip.py:739-746) at the KITTI size; kw: its fixed arguments too (drop_rate)"""
    args = dict(KW, depths=(2, 2, 2, 2), embed_dim=96, num_heads=(3, 6, 12, 24), qkv_bias=True, mlp_ratio=4, drop_path_rate=0.1,
                drop_rate=0, attn_drop_rate=0, norm_layer=partial(nn.LayerNorm, eps=1e-6))
    args.update(kw)
    return T.TULIP(img_size=(16, 1024), target_img_size=(64, 1024), **args)


def _large(**kw):
    return T.tulip_large(img_size=(16, 2048), target_img_size=(64, 2048), **dict(KW, **kw))


def _tiny(img_size=None, **kw):
    """the oracle's tiny config (two stages, C = 48 / 96 with 3 / 6 heads: no fused block kernel covers it)"""
    cfg = O.tiny_config(**({} if img_size is None else dict(img_size=img_size, target_img_size=(4 * img_size[0], img_size[1]))))
    return T.TULIP(img_size=cfg.img_size, target_img_size=cfg.target_img_size, depths=cfg.depths, embed_dim=cfg.embed_dim,
                   num_heads=cfg.num_heads, norm_layer=partial(nn.LayerNorm, eps=1e-6), **dict(KW, **kw))


def _flip(knob):
    return {knob: not getattr(TulipEngine, knob)}


# the switches of the block routes, each flipped alone from its default on tulip_base at batch 8
KNOBS = ("fuse_block96", "fuse_block96_bwd", "fuse_wide", "fuse_wide_bwd", "fuse_deep", "fc1_grad96", "fc1_grad_wide",
         "recompute96", "split_wide", "split_wide_bwd", "pair96", "attn_fp8", "infer_no_save")
FORMS = ("train", "train_ow", "infer")

# name -> (model factory, batch, engine attributes, form, MC dropout: model.eval() with its nn.Dropout modules back in train())
SCENARIOS = {}


def _add(name, factory, B, attrs=None, forms=("train", "infer"), mc=False):
    for form in forms:
        SCENARIOS[f"{name}_{form}"] = (factory, B, dict(attrs or {}), form, mc)


_add("base8", _base, 8, forms=FORMS)
# batch 2: C = 384 below wide_min_windows, C = 768 below deep_min_windows; batch 64: the deep form above deep_max_windows
_add("base2", _base, 2, forms=FORMS)
_add("base64", _base, 64, forms=FORMS)
_add("large2", _large, 2, forms=FORMS)
_add("tiny2", _tiny, 2, forms=FORMS)
_add("tiny2_expanding", partial(_tiny, pixel_shuffle=False, patch_unmerging=False), 2, forms=FORMS)
# 32- and 64-token windows: every block runs the sequence (the second stage of the 8x8 model on its (1, 64) backup window)
_add("tiny2_win4x8", partial(_tiny, window_size=[4, 8]), 2)
_add("tiny2_win8x8", partial(_tiny, img_size=(8, 512), window_size=[8, 8]), 2)
for _k in KNOBS:
    _add(f"base8_{_k}", _base, 8, _flip(_k))
_add("base8_no96", _base, 8, dict(fuse_block96=False, fuse_block96_bwd=False))
_add("base8_nowide", _base, 8, dict(fuse_wide=False, fuse_wide_bwd=False))
_add("base2_wide_min32", _base, 2, dict(wide_min_windows=32))
_add("base64_deep_max256", _base, 64, dict(deep_max_windows=256))
# element dropout: a block with an active site runs the sequence both ways
_add("tiny2_dropout", partial(_tiny, drop_rate=0.1), 2, forms=("train_ow", "infer"))
_add("tiny2_attn_dropout", partial(_tiny, attn_drop_rate=0.1), 2, forms=("train_ow", "infer"))
_add("base8_dropout", partial(_base, drop_rate=0.1), 8, forms=("train_ow", "infer"))
_add("tiny2_mc_dropout", partial(_tiny, drop_rate=0.1), 2, forms=("infer",), mc=True)
_add("base8_mc_dropout", partial(_base, drop_rate=0.1), 8, forms=("infer",), mc=True)


class Run:
    """One scenario's log and what the rules need beside it."""


@functools.lru_cache(maxsize=None)
def scenario(name) -> Run:
    factory, B, attrs, form, mc = SCENARIOS[name]
    torch.manual_seed(0)
    model = factory()
    if mc:
        model.eval()
        for mod in model.modules():
            if isinstance(mod, nn.Dropout):
                mod.train()
    else:
        model.train(form != "infer")
    eng = TulipEngine(model)
    for k, v in attrs.items():
        assert hasattr(eng, k), k
        setattr(eng, k, v)
    eng.bind(torch.device("cpu"))
    r = Run()
    r.name, r.eng, r.B, r.form = name, eng, B, form
    g = torch.zeros(eng.params.total, dtype=torch.float32)
    with dry_run(eng, gflat=g) as dry:
        P = eng.plan(B)
        if form == "infer":
            eng.run_forward(P, with_loss=False)
            r.bwd0 = len(dry.log)
        else:
            eng.run_forward(P, with_loss=True, defer_loss_final=True)
            r.bwd0 = len(dry.log)            # index of the backward's first entry
            eng.run_backward(P, g, bucket_hook=lambda tag: dry.note("hook", tag), **(dict(overwrite=True) if form == "train_ow" else {}))
    r.dry, r.log, r.P = dry, dry.log, P
    return r


if __name__ == "__main__":
    import time
    for nm in sys.argv[1:] or SCENARIOS:
        t0 = time.time()
        run = scenario(nm)
        print(f"{nm:34s} {len(run.log):6d} {run.dry.sha256()}  ({time.time() - t0:.1f} s)", flush=True)
        if os.environ.get("DRY_RUN_DUMP"):
            with open(os.path.join(os.environ["DRY_RUN_DUMP"], nm + ".log"), "w") as f:
                f.write(run.dry.text())
        scenario.cache_clear()               # (a script run keeps no engine alive: the matrix holds tulip_large)

"""Cost of element dropout on the captured training step: tulip_base, KITTI 16x1024 -> 64x1024, batch 8 (bench.py's
workload) with drop_rate = attn_drop_rate = 0.1 against the same model at p = 0.  Every block with an active dropout site
runs the unfused launch sequence, so the difference is mostly the fused block kernels given up.

    python tools/bench_dropout.py [--steps 50] [--warmup 10] [--p 0.1]
"""
import argparse
import json
import os
import sys
from functools import partial

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def model(p):
    from tulip_amd.model import tulip as T
    torch.manual_seed(0)
    return T.TULIP(img_size=(16, 1024), target_img_size=(64, 1024), patch_size=(1, 4), in_chans=1, window_size=[2, 8],
                   depths=(2, 2, 2, 2), embed_dim=96, num_heads=(3, 6, 12, 24), qkv_bias=True, mlp_ratio=4,
                   drop_path_rate=0.1, drop_rate=p, attn_drop_rate=p, norm_layer=partial(nn.LayerNorm, eps=1e-6),
                   pixel_shuffle=True, circular_padding=True, log_transform=True, patch_unmerging=True).cuda().train()


def time_steps(p, steps, warmup, B=8):
    from tulip_amd.trainer import Trainer
    g = torch.Generator().manual_seed(1234)
    r = torch.rand(B, 1, 64, 1024, generator=g)
    r[torch.rand(B, 1, 64, 1024, generator=g) < 0.1] = 0
    hi = torch.log1p(r).cuda()
    lo = hi[:, :, 0::4, :].contiguous()
    tr = Trainer(model(p), B, use_graph=True)
    tr.load_batch(lo, hi)
    for _ in range(warmup):
        tr.step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        tr.step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, float(tr.P.losses[0].item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--p", type=float, default=0.1)
    a = ap.parse_args()
    res = {}
    for p in (0.0, a.p, 0.0, a.p):                  # interleaved: two runs each
        ms, loss = time_steps(p, a.steps, a.warmup)
        res.setdefault(str(p), []).append(round(ms, 4))
        print(f"p={p}: {ms:.4f} ms/step (loss {loss:.5f})", flush=True)
    print(json.dumps({"ms_per_step": res, "batch": 8, "steps": a.steps}))


if __name__ == "__main__":
    main()

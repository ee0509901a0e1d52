"""Cost of the attention window: (1) the window-attention kernels alone at equal token count for L = 16 / 32 / 64, and
(2) the captured training step of tulip_base, KITTI 16x1024 -> 64x1024, batch 8 (bench.py's workload), at window_size
(2, 8), (4, 8) and (2, 16).  The 32- and 64-token windows run the unfused launch sequence in every block (no fused block
kernel takes them), so (2) measures that together with the kernels of (1).

    python tools/bench_windows.py kernels [--iters 50]      # one launch set per iteration; run under
                                                            # rocprofv3 --kernel-trace --stats -- python ... for the
                                                            # per-kernel times (the event timings printed are per launch)
    python tools/bench_windows.py step [--steps 50] [--warmup 10]
"""
import argparse
import json
import os
import sys
from functools import partial

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# stage 0 of the bench workload: batch 8, 16x256 tokens, C = 96, 3 heads of 32 -- 32 768 tokens for every window
KERNEL_SHAPES = [((2, 8), (1, 4)), ((4, 8), (2, 4)), ((2, 16), (1, 8)), ((8, 8), (4, 4))]


def kernels(iters):
    from oracle import tulip_oracle as O
    from tulip_amd import ops
    B, H, W, C, nh = 8, 16, 256, 96, 3
    M = B * H * W
    g = torch.Generator().manual_seed(0)
    qkv = (torch.randn(M, 3 * C, generator=g) * 1.5).to(torch.bfloat16).cuda()
    dout = torch.randn(M, C, generator=g).to(torch.bfloat16).cuda()
    out = torch.empty(M, C, dtype=torch.bfloat16, device="cuda")
    dqkv = torch.empty_like(qkv)
    res = {}
    for win, sft in KERNEL_SHAPES:
        L = win[0] * win[1]
        table = torch.randn((2 * win[0] - 1) * (2 * win[1] - 1), nh, generator=g).cuda()
        rel32 = torch.from_numpy(O.relative_position_index(*win)).to(torch.int32).cuda()
        R = ops.window_attn_bwd_partial_rows(B, H, W, nh, win)
        part = torch.empty(R * nh, L * L, device="cuda")
        times = {}
        for name, fn in (("fwd", lambda: ops.window_attn_fwd(qkv, table, rel32, out, B, H, W, C, nh, win, sft, 1)),
                         ("bwd", lambda: ops.window_attn_bwd(qkv, dout, table, rel32, dqkv, part, B, H, W, C, nh, win, sft,
                                                             1))):
            for _ in range(5):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name] = round(e0.elapsed_time(e1) * 1000.0 / iters, 2)
        res[f"{win[0]}x{win[1]}"] = dict(L=L, partial_rows=R, **{k + "_us": v for k, v in times.items()})
        print(f"window {win}: L = {L}, fwd {times['fwd']:.2f} us, bwd {times['bwd']:.2f} us per launch", flush=True)
    print(json.dumps({"kernels": res, "tokens": M, "C": C, "heads": nh}))


def model(win):
    from tulip_amd.model import tulip as T
    torch.manual_seed(0)
    return T.TULIP(img_size=(16, 1024), target_img_size=(64, 1024), patch_size=(1, 4), in_chans=1, window_size=list(win),
                   depths=(2, 2, 2, 2), embed_dim=96, num_heads=(3, 6, 12, 24), qkv_bias=True, mlp_ratio=4,
                   drop_path_rate=0.1, norm_layer=partial(nn.LayerNorm, eps=1e-6), pixel_shuffle=True,
                   circular_padding=True, log_transform=True, patch_unmerging=True).cuda().train()


def time_steps(win, steps, warmup, B=8):
    from tulip_amd.trainer import Trainer
    g = torch.Generator().manual_seed(1234)
    r = torch.rand(B, 1, 64, 1024, generator=g)
    r[torch.rand(B, 1, 64, 1024, generator=g) < 0.1] = 0
    hi = torch.log1p(r).cuda()
    lo = hi[:, :, 0::4, :].contiguous()
    tr = Trainer(model(win), B, use_graph=True)
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


def step(steps, warmup):
    res = {}
    for win in ((2, 8), (4, 8), (2, 16), (2, 8), (4, 8), (2, 16)):      # interleaved: two runs each
        ms, loss = time_steps(win, steps, warmup)
        res.setdefault(f"{win[0]}x{win[1]}", []).append(round(ms, 4))
        print(f"window {win}: {ms:.4f} ms/step (loss {loss:.5f})", flush=True)
    print(json.dumps({"ms_per_step": res, "batch": 8, "steps": steps}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("kernels", "step"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if a.what == "kernels":
        kernels(a.iters)
    else:
        step(a.steps, a.warmup)


if __name__ == "__main__":
    main()

"""Cost of in_chans: (1) the launches that see the channel count alone -- the patch embedding forward / backward (partial
rows) and the fused head (norm_up + head + loss forward, the chain's data gradient, the side queue's weight gradient) --
at bench.py's shapes for in_chans 1, 2 and 4, and (2) the captured training step of tulip_base, KITTI 16x1024 -> 64x1024,
batch 8 (bench.py's workload), at in_chans 1, 2 and 4.

    python tools/bench_inchans.py kernels [--iters 50]      # one launch per iteration (event timings are per launch)
    python tools/bench_inchans.py step [--steps 50] [--warmup 10]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHANS = (1, 2, 4)


def _time(fn, iters):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1000.0 / iters, 2)


def kernels(iters):
    from tulip_amd import ops
    B, Hin, Win, E, kw = 8, 16, 1024, 96, 8
    H, W = Hin, Win // 4                             # head tokens: the embedding grid (16 x 256)
    M = B * H * W
    g = torch.Generator().manual_seed(0)
    dev = "cuda"
    res = {}
    for c in CHANS:
        T = c * kw
        img = torch.rand(B, c, Hin, Win, generator=g).to(dev)
        w = (torch.randn(E, c, 1, kw, generator=g) * 0.3).to(dev)
        b, gam, bet = torch.zeros(E, device=dev), torch.ones(E, device=dev), torch.zeros(E, device=dev)
        out = torch.empty(M, E, device=dev)
        dout = torch.randn(M, E, generator=g).to(dev)
        nb, stride = ops.patch_embed_bwd_blocks(M), E * T + 3 * E
        part = torch.empty(nb, stride, device=dev)
        p0 = part.data_ptr()
        x = torch.randn(M, E, generator=g).to(dev)
        xn = torch.empty(M, E, dtype=torch.bfloat16, device=dev)
        mean, rstd = torch.empty(M, device=dev), torch.empty(M, device=dev)
        We = (torch.randn(16 * E, E, generator=g) * 0.1).to(torch.bfloat16).to(dev)
        be = (torch.randn(16 * E, generator=g) * 0.1).to(dev)
        wd = (torch.randn(c, E, generator=g) * 0.2).to(dev)
        pred = torch.empty(B, c, 4 * H, 4 * W, device=dev)
        target = torch.rand(B, c, 4 * H, 4 * W, generator=g).to(dev)
        R = (M + 31) // 32
        lpart = torch.empty(2 * R, device=dev)
        dpart = torch.empty(R, 128 * c, device=dev)
        dx, lnp = torch.empty(M, E, device=dev), torch.empty(R, 2 * E, device=dev)
        sp = ops.tail_wgrad_splits(B, H, W, E)
        sw, sb = torch.empty(sp, 16 * E * E, device=dev), torch.empty(sp, 16 * E, device=dev)
        ops.tail_fwd_ln(x, gam, bet, 1e-6, xn, mean, rstd, We, be, wd, pred, B, H, W, E, target=target, loss_partials=lpart,
                        log_transform=True, in_chans=c)
        t = {
            "embed_fwd": _time(lambda: ops.patch_embed_fwd(img, w, b, gam, bet, out, B, c, Hin, Win, E, 1, 4, kw, True, 1e-6),
                               iters),
            "embed_bwd": _time(lambda: ops.patch_embed_bwd(img, w, b, gam, dout, p0, p0 + 4 * E * T, p0 + 4 * (E * T + E),
                                                           p0 + 4 * (E * T + 2 * E), B, c, Hin, Win, E, 1, 4, kw, True,
                                                           1e-6, partial_stride=stride), iters),
            "head_fwd_ln": _time(lambda: ops.tail_fwd_ln(x, gam, bet, 1e-6, xn, mean, rstd, We, be, wd, pred, B, H, W, E,
                                                         target=target, loss_partials=lpart, log_transform=True,
                                                         in_chans=c), iters),
            "head_bwd_dgrad_ln": _time(lambda: ops.tail_bwd_dgrad_ln(xn, We, be, wd, pred, dpart, B, H, W, E, x, mean, rstd,
                                                                     gam, dx, lnp, target=target, in_chans=c), iters),
            "head_wgrad": _time(lambda: ops.tail_wgrad(xn, We, be, wd, pred, sw, sb, B, H, W, E, target=target, in_chans=c),
                                iters),
        }
        res[str(c)] = {k + "_us": v for k, v in t.items()}
        print(f"in_chans {c}: " + ", ".join(f"{k} {v:.2f} us" for k, v in t.items()), flush=True)
    print(json.dumps({"kernels": res, "tokens": M, "E": E}))


def model(c):
    from tulip_amd.model.tulip import tulip_base
    torch.manual_seed(0)
    return tulip_base(img_size=(16, 1024), target_img_size=(64, 1024), patch_size=(1, 4), window_size=(2, 8),
                      pixel_shuffle=True, circular_padding=True, log_transform=True, patch_unmerging=True,
                      in_chans=c).cuda().train()


def time_steps(c, steps, warmup, B=8):
    from tulip_amd.trainer import Trainer
    g = torch.Generator().manual_seed(1234)
    r = torch.rand(B, c, 64, 1024, generator=g)
    r[torch.rand(B, c, 64, 1024, generator=g) < 0.1] = 0
    hi = torch.log1p(r).cuda()
    lo = hi[:, :, 0::4, :].contiguous()
    tr = Trainer(model(c), B, use_graph=True)
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
    for c in CHANS + CHANS:                                   # interleaved: two runs each
        ms, loss = time_steps(c, steps, warmup)
        res.setdefault(str(c), []).append(round(ms, 4))
        print(f"in_chans {c}: {ms:.4f} ms/step (loss {loss:.5f})", flush=True)
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

"""Cost of upscale_factor 8 (16-pixel patches) against upscale_factor 4 at the SAME output image:

(1) the head kernels -- norm_up + head + loss forward, the chain's data gradient with norm_up's backward, the side queue's
    weight gradient -- at r = 8 on B x 8 x 128 tokens against r = 4 on B x 16 x 256 tokens (B = 8, E = 96, a 64x1024 output
    either way: the same expand-GEMM FLOPs and pred bytes, a quarter of the xn rows), medians over --reps runs with the spread;
(2) the captured training step of tulip_base, KITTI 16x1024 -> 64x1024, batch 8, at patch_size (1, 4) (bench.py's workload),
    (2, 8) with the pixel-shuffle head and (2, 8) with FinalPatchExpanding, interleaved runs.

    python tools/bench_upscale.py kernels [--iters 50] [--reps 5]
    python tools/bench_upscale.py step [--steps 50] [--warmup 10]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
    return e0.elapsed_time(e1) * 1000.0 / iters


def kernels(iters, reps):
    from tulip_amd import ops
    B, E, c = 8, 96, 1
    g = torch.Generator().manual_seed(0)
    dev = "cuda"
    res = {}
    fns = {}
    for r, (H, W) in ((4, (16, 256)), (8, (8, 128))):
        M, NE = B * H * W, r * r * E
        x = torch.randn(M, E, generator=g).to(dev)
        gam, bet = torch.ones(E, device=dev), torch.zeros(E, device=dev)
        xn = torch.empty(M, E, dtype=torch.bfloat16, device=dev)
        mean, rstd = torch.empty(M, device=dev), torch.empty(M, device=dev)
        We = (torch.randn(NE, E, generator=g) * 0.1).to(torch.bfloat16).to(dev)
        be = (torch.randn(NE, generator=g) * 0.1).to(dev)
        wd = (torch.randn(c, E, generator=g) * 0.2).to(dev)
        pred = torch.empty(B, c, r * H, r * W, device=dev)
        target = torch.rand(B, c, r * H, r * W, generator=g).to(dev)
        R = (M + 31) // 32
        lpart, dpart = torch.empty(2 * R, device=dev), torch.empty(R, 128 * c, device=dev)
        dx, lnp = torch.empty(M, E, device=dev), torch.empty(R, 2 * E, device=dev)
        sp = ops.tail_wgrad_splits(B, H, W, E, c, r)
        sw, sb = torch.empty(sp, NE * E, device=dev), torch.empty(sp, NE, device=dev)
        fwd = lambda x=x, gam=gam, bet=bet, xn=xn, mean=mean, rstd=rstd, We=We, be=be, wd=wd, pred=pred, H=H, W=W, target=target, \
            lpart=lpart, r=r: ops.tail_fwd_ln(x, gam, bet, 1e-6, xn, mean, rstd, We, be, wd, pred, B, H, W, E, target=target,
                                              loss_partials=lpart, log_transform=True, in_chans=c, r=r)
        fwd()
        dgrad = lambda x=x, gam=gam, xn=xn, mean=mean, rstd=rstd, We=We, be=be, wd=wd, pred=pred, H=H, W=W, target=target, dpart=dpart, \
            dx=dx, lnp=lnp, r=r: ops.tail_bwd_dgrad_ln(xn, We, be, wd, pred, dpart, B, H, W, E, x, mean, rstd, gam, dx, lnp,
                                                       target=target, in_chans=c, r=r)
        wgrad = lambda xn=xn, We=We, be=be, wd=wd, pred=pred, sw=sw, sb=sb, H=H, W=W, target=target, r=r: \
            ops.tail_wgrad(xn, We, be, wd, pred, sw, sb, B, H, W, E, target=target, in_chans=c, r=r)
        # bytes a launch must move at least once (the roofline table's accounting): inputs read once + outputs written once
        px = pred.numel() * 4
        fns[r] = {"tail_fwd_ln": (fwd, M * E * 4 + NE * E * 2 + M * E * 2 + 2 * px),
                  "tail_bwd_dgrad_ln": (dgrad, M * E * 2 + NE * E * 2 + 2 * px + 2 * M * E * 4),
                  "tail_wgrad": (wgrad, M * E * 2 + NE * E * 2 + 2 * px + sp * (NE * E + NE) * 4)}
        res[str(r)] = {"tokens": M, "wgrad_splits": sp}
    for rep in range(reps):                                    # interleaved: r = 4, r = 8, r = 4, ...
        for r in (4, 8):
            for k, (fn, nbytes) in fns[r].items():
                res[str(r)].setdefault(k, {"us": [], "bytes": nbytes})["us"].append(round(_time(fn, iters), 2))
    for r in ("4", "8"):
        for k, v in res[r].items():
            if isinstance(v, dict):
                v["median_us"] = statistics.median(v["us"])
                v["spread_us"] = [min(v["us"]), max(v["us"])]
                v["gb_per_s"] = round(v["bytes"] / v["median_us"] / 1e3, 1)
                print(f"r {r} {k}: median {v['median_us']:.2f} us (min {min(v['us']):.2f}, max {max(v['us']):.2f}), "
                      f"{v['bytes'] / 1e6:.1f} MB, {v['gb_per_s']} GB/s", flush=True)
    print(json.dumps({"kernels": res, "B": B, "E": E}))


CONFIGS = {
    "p1x4_ps": dict(patch_size=(1, 4), pixel_shuffle=True, patch_unmerging=True),
    "p2x8_ps": dict(patch_size=(2, 8), pixel_shuffle=True, patch_unmerging=True),
    "p2x8_fe": dict(patch_size=(2, 8), pixel_shuffle=False, patch_unmerging=False),
}


def model(name):
    from tulip_amd.model.tulip import tulip_base
    torch.manual_seed(0)
    return tulip_base(img_size=(16, 1024), target_img_size=(64, 1024), window_size=(2, 8), circular_padding=True,
                      log_transform=True, **CONFIGS[name]).cuda().train()


def time_steps(name, steps, warmup, B=8):
    from tulip_amd.trainer import Trainer
    g = torch.Generator().manual_seed(1234)
    r = torch.rand(B, 1, 64, 1024, generator=g)
    r[torch.rand(B, 1, 64, 1024, generator=g) < 0.1] = 0
    hi = torch.log1p(r).cuda()
    lo = hi[:, :, 0::4, :].contiguous()
    tr = Trainer(model(name), B, use_graph=True)
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
    for name in tuple(CONFIGS) * 2:                            # interleaved: two runs each
        ms, loss = time_steps(name, steps, warmup)
        res.setdefault(name, []).append(round(ms, 4))
        print(f"{name}: {ms:.4f} ms/step (loss {loss:.5f})", flush=True)
    print(json.dumps({"ms_per_step": res, "batch": 8, "steps": steps}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("kernels", "step"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if a.what == "kernels":
        kernels(a.iters, a.reps)
    else:
        step(a.steps, a.warmup)


if __name__ == "__main__":
    main()

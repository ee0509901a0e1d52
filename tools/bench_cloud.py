#!/usr/bin/env python3
"""Dense clouds from the model, timed (run on the GPU box): KITTI tulip_base (16x1024 -> 64x1024), batch 8 and 64.
  upsampler   : CloudUpsampler.__call__ -- one HIP-graph replay: the eval forward + the three cloud launches for the whole batch
  composition : what produced the same clouds before CloudUpsampler existed: GraphedForward for the batch, then per image
                ops.eval_postprocess with a zero target, ops.range_to_xyz and the boolean-mask index pcd[img.reshape(-1) > 0]
                (one host synchronisation per image)
  forward     : GraphedForward alone, for the cloud stretch's share of the replay: (upsampler - forward) / upsampler
  from_pred   : the three cloud launches alone, outside a graph
Device events around blocks of calls that end in a synchronise; upsampler / composition and upsampler / forward alternate, 7 pairs,
median and [min, max].  Before timing, the two paths' clouds are compared bit for bit.  Writes the table to --out (default
profiles/cloud_bench.txt) and prints it."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_eval import paired, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_bench.txt"))
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_cloud.py measures on the GPU; no device found")
    from oracle import tulip_oracle as O
    from tulip_amd import evaluation as EV, ops
    from tulip_amd.cloud import CloudUpsampler
    from tulip_amd.infer import GraphedForward
    from tulip_amd.model.tulip import tulip_base
    dev = "cuda"
    cfg = O.tulip_base_config()
    H, W = cfg.target_img_size
    h, w = cfg.img_size
    torch.manual_seed(0)
    model = tulip_base(img_size=cfg.img_size, target_img_size=cfg.target_img_size, patch_size=cfg.patch_size, in_chans=1,
                       window_size=cfg.window_size, pixel_shuffle=True, circular_padding=True, log_transform=True,
                       patch_unmerging=True).to(dev).eval()
    med = lambda v: sorted(v)[len(v) // 2]
    lines = [f"dense clouds, KITTI tulip_base {h}x{w} -> {H}x{W}, log_transform, gate {EV.pred_gate('kitti', False)}; "
             f"ms per batch, median [min, max] of {args.reps} alternating blocks of {args.iters} calls",
             f"device: {torch.cuda.get_device_name(0)}"]
    for B in args.batches:
        lo, _ = O.synthetic_batch(cfg, B, seed=100 + B)
        lo = lo.to(dev)
        up = CloudUpsampler(model, "kitti", B, log_transform=True)
        gf = GraphedForward(model, B)
        ev = EV.RangeEvaluator("kitti", (h, w), (H, W), True, device=dev)
        zero = torch.zeros(H, W, device=dev)

        def composition():
            pred = gf(lo)
            out = []
            for b in range(B):
                ops.eval_postprocess(pred[b], zero, lo[b], ev.pred_img, ev.hi_img, ev.scratch, ev.mae, H, W, h, w, True,
                                     ev.gate[0], ev.gate[1], 0.0)
                ops.range_to_xyz(ev.pred_img, *ev.tables, EV.MAX_RANGE["kitti"], H, W, ev.pcd_pred)
                out.append(ev.pcd_pred[ev.pred_img.reshape(-1) > 0])
            return out

        new = lambda: up(lo)
        new()
        clouds = [c.clone() for c in up.clouds()]
        old = composition()
        same = all(a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(clouds, old))
        kept = sum(c.shape[0] for c in clouds)
        t_old, t_new = paired(composition, new, args.iters, args.reps)
        t_fwd, t_new2 = paired(lambda: gf(lo), new, args.iters, args.reps)
        pred = gf(lo).clone()
        t_cloud = [timed(lambda: up.from_pred(pred, lo), args.iters, warm=3) for _ in range(args.reps)]
        ratio = sorted(n / o for o, n in zip(t_old, t_new))
        share = sorted((n - f) / n for f, n in zip(t_fwd, t_new2))
        fmt = lambda v: f"{med(v):8.3f} [{min(v):.3f}, {max(v):.3f}]"
        lines += [f"B={B}: {kept} of {B * H * W} pixels kept; clouds of both paths bit-identical: {same}",
                  f"  composition (per batch)      {fmt(t_old)}   per image {med(t_old) / B:.4f}",
                  f"  upsampler   (per batch)      {fmt(t_new)}   per image {med(t_new) / B:.4f}",
                  f"  upsampler / composition      {med(ratio):8.3f} [{ratio[0]:.3f}, {ratio[-1]:.3f}]",
                  f"  forward alone (per batch)    {fmt(t_fwd)}   (upsampler beside it {fmt(t_new2)})",
                  f"  cloud stretch's share of the replay {med(share):.4f} [{share[0]:.4f}, {share[-1]:.4f}]",
                  f"  from_pred, three launches    {fmt(t_cloud)}"]
        if not same:
            lines.append("  MISMATCH between the two paths")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 0 if all("MISMATCH" not in l for l in lines) else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Launch times of the multi-channel evaluation kernels (run on the GPU box), each in alternation with the single-channel launch on
the channel-0 planes of the same inputs:
  post : tulip_eval_postprocess_c (one launch pair, C = 2, 3, 4) against tulip_eval_postprocess, one image, log_transform and every
         channel_log flag on, keep_close on; KITTI 64x1024 and DurLAR 128x2048
  mc   : tulip_mc_aggregate_c against tulip_mc_aggregate, 50 passes of one KITTI image
Device events around blocks of launches; 7 alternating pairs, median and [min, max].  Prints one JSON object."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_eval import paired  # noqa: E402


def record(workload, a, b, bytes_c):
    med = lambda v: sorted(v)[len(v) // 2]
    ratio = sorted(y / x for x, y in zip(a, b))
    return {"workload": workload, "single_channel_us": med(a) * 1e3, "single_channel_us_min_max": [min(a) * 1e3, max(a) * 1e3],
            "us": med(b) * 1e3, "us_min_max": [min(b) * 1e3, max(b) * 1e3], "ratio_over_single": med(ratio),
            "ratio_min_max": [ratio[0], ratio[-1]], "algorithmic_MB": bytes_c / 1e6, "algorithmic_GBps": bytes_c / med(b) / 1e6,
            "pairs": len(a)}


def main():
    from tulip_amd import ops
    dev, out = "cuda", {}
    g = torch.Generator().manual_seed(0)
    for ds, (H, W, h) in (("kitti", (64, 1024, 16)), ("durlar", (128, 2048, 32))):
        f = H // h
        for C in (2, 3, 4):
            hi = torch.log1p(torch.rand(C, H, W, generator=g))
            hi[:, torch.rand(H, W, generator=g) < 0.1] = 0
            pred = (hi + 0.01 * torch.randn(C, H, W, generator=g)).to(dev)
            hi = hi.to(dev)
            lo = hi[:, 0::f].contiguous()
            p_img, t_img = torch.empty(C, H, W, device=dev), torch.empty(C, H, W, device=dev)
            partials = torch.zeros((3 * C + 1) * 1024, dtype=torch.float64, device=dev)
            metrics = torch.zeros(3 * C + 1, device=dev)
            single = lambda: ops.eval_postprocess(pred, hi, lo, p_img, t_img, partials, metrics, H, W, h, W, True, 2 / 80, 1.0, 0.25)
            multi = lambda: ops.eval_postprocess_c(pred, hi, lo, p_img, t_img, partials, metrics, H, W, h, W, C, True,
                                                   [True] * (C - 1), 2 / 80, 1.0, 0.25)
            a, b = paired(single, multi, 200, 7)
            # per pixel and channel: pred and hi read, pred_img and hi_img written, lo read on every f-th row
            out[f"post_{ds}_C{C}"] = record(f"{ds} {H}x{W} one image, C={C} (single-channel launch: its channel-0 planes)", a, b,
                                            C * H * W * 4 * (4 + 1 / f))
    T, n = 50, 64 * 1024
    for C in (2, 3, 4):
        preds = torch.rand(T, C, n, generator=g).to(dev)
        first = preds[:, 0].contiguous()
        o1, oc = torch.empty(n, device=dev), torch.empty(C, n, device=dev)
        a, b = paired(lambda: ops.mc_aggregate(first, T, n, 0.03, o1), lambda: ops.mc_aggregate_c(preds, T, C, n, 0.03, oc), 200, 7)
        # channel 0 is read twice (mean, then deviations), the others once
        out[f"mc_kitti_C{C}"] = record(f"kitti 64x1024, {T} passes, C={C}", a, b, n * 4 * (T * (C + 1) + C))
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()

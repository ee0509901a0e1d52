#!/usr/bin/env python3
"""Measurements for the 8(f) rows around the hot path (run on the GPU box):
  prep     : tulip_range_prep, KITTI B=8 from the interleaved .npy payload -> GB/s against the HBM roofline
  prep_aug : tulip_range_prep_aug on the same two workloads (roll + flip + row phase, beam_drop 0.1, point_drop 0.05), timed in
             alternation with the plain launch: per-pair ratio and its spread over the repeats; `--only prep` runs just these
  prep_ch2 : RangePrep(in_chans=2) (tulip_range_prep_c, one launch) on the same two workloads from the interleaved payload, in
             alternation with the single-channel entry point once per channel plus the hole select in torch
  infer    : eval forward, tulip_base KITTI B=8, HIP-graph replay -> images/s (the MCdrop tile)
  evaluate : per-image post-processing + projection + voxel metrics + Chamfer -> ms/image, Chamfer pair rate
             against the fp32 vector-ALU rate, and the oracle (numpy/torch CPU) timed on the same image
Prints one JSON object."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def paired(fn_a, fn_b, iters, reps):
    """fn_a and fn_b timed in alternating blocks of `iters` calls, `reps` times: (ms_a, ms_b) lists, one pair per repeat"""
    a, b = [], []
    timed(fn_a, iters)
    timed(fn_b, iters)
    for _ in range(reps):
        a.append(timed(fn_a, iters, warm=1))
        b.append(timed(fn_b, iters, warm=1))
    return a, b


def pair_record(workload, a, b, algo_bytes):
    ratio = sorted(y / x for x, y in zip(a, b))
    med = lambda v: sorted(v)[len(v) // 2]
    return {"workload": workload, "plain_ms": med(a), "plain_ms_min_max": [min(a), max(a)], "ms": med(b),
            "ms_min_max": [min(b), max(b)], "algorithmic_GBps": algo_bytes / med(b) / 1e6,
            "plain_algorithmic_GBps": algo_bytes / med(a) / 1e6, "ratio_aug_over_plain": med(ratio),
            "ratio_min_max": [ratio[0], ratio[-1]], "pairs": len(a)}


def main():
    from tulip_amd import data as D, evaluation as EV
    from tulip_amd.infer import GraphedForward
    from tulip_amd.model.tulip import tulip_base
    from oracle import data_oracle as DO, eval_oracle as EO, tulip_oracle as O
    dev = "cuda"
    out = {}
    # ---- prep
    B, H, W = 8, 64, 1024
    raw = DO.synthetic_raw(B, H, W, seed=1)
    payload = torch.stack([raw, torch.rand_like(raw)], -1).contiguous().to(dev)
    prep = D.RangePrep("kitti", (16, 1024), (64, 1024), True)
    ms = timed(lambda: prep(payload), 200)
    algo = B * H * W * 4 * (1 + 1 + 0.25)            # channel-0 read + hi write + lo write
    touched = B * H * W * 4 * (2 + 1 + 0.25)         # the interleaved intensity shares the cache lines
    t0 = time.perf_counter()
    for _ in range(5):
        DO.range_prep(raw, DO.DATASETS["kitti"], (16, 1024), (64, 1024), True)
    cpu_ms = (time.perf_counter() - t0) / 5 * 1e3
    out["prep"] = {"workload": "kitti B=8 64x1024 from (H,W,2) payload", "ms": ms, "algorithmic_GBps": algo / ms / 1e6,
                   "touched_GBps": touched / ms / 1e6, "hbm_peak_GBps": 8000, "oracle_cpu_ms": cpu_ms,
                   "note": "2.6 MB per launch: launch-latency bound, not bandwidth bound"}
    big = torch.rand(64, 128, 2048, device=dev) * 100
    prep_big = D.RangePrep("durlar", (32, 2048), (128, 2048), True)
    ms = timed(lambda: prep_big(big), 50)
    out["prep_large"] = {"workload": "durlar B=64 128x2048", "ms": ms,
                         "algorithmic_GBps": 64 * 128 * 2048 * 4 * 2.25 / ms / 1e6}
    # ---- prep with the per-sample augmentation, in alternation with the plain launch of the same run
    from tulip_amd.augment import RangeAugment
    full = dict(beam_drop=0.1, point_drop=0.05)
    ids8 = torch.arange(1000, 1008, device=dev)
    prep_a = D.RangePrep("kitti", (16, 1024), (64, 1024), True, augment=RangeAugment(seed=0, **full))
    a, b = paired(lambda: prep(payload), lambda: prep_a(payload, sample_ids=ids8), 200, 7)
    out["prep_aug"] = pair_record("kitti B=8 64x1024 from (H,W,2) payload, roll+flip+row_phase, beam 0.1, point 0.05", a, b, algo)
    out["prep_aug"]["note"] = "launch-latency bound like prep: the ratio of prep_large_aug is the signal"
    ids64 = torch.arange(2000, 2064, device=dev)
    algo_big = 64 * 128 * 2048 * 4 * 2.25
    prep_big_a = D.RangePrep("durlar", (32, 2048), (128, 2048), True, augment=RangeAugment(seed=0, **full))
    a, b = paired(lambda: prep_big(big), lambda: prep_big_a(big, sample_ids=ids64), 50, 7)
    out["prep_large_aug"] = pair_record("durlar B=64 128x2048, roll+flip+row_phase, beam 0.1, point 0.05", a, b, algo_big)
    # which part costs what: one augmentation at a time against the same plain launch (the stores are the plain launch's aligned
    # ones for every draw; a shift with s % 4 != 0 reads two aligned source groups per four pixels, a mirror reads in descending order)
    for name, kw in (("none", dict(roll=False, flip=False, row_phase=False)), ("roll", dict(flip=False, row_phase=False)),
                     ("flip", dict(roll=False, row_phase=False)), ("row_phase", dict(roll=False, flip=False)),
                     ("drops", dict(roll=False, flip=False, row_phase=False, **full))):
        pk = D.RangePrep("durlar", (32, 2048), (128, 2048), True, augment=RangeAugment(seed=0, **kw))
        a, b = paired(lambda: prep_big(big), lambda: pk(big, sample_ids=ids64), 50, 5)
        out[f"prep_large_aug_{name}_only"] = pair_record(f"durlar B=64 128x2048, {kw}", a, b, algo_big)
    # ---- two-channel batches: one launch of RangePrep(in_chans=2) against what a caller had before it -- the single-channel entry
    # point once per channel (its own base offset and scale) and the hole select in torch -- in alternation
    from tulip_amd import ops

    def ch2_record(name, ds, lo_size, hi_size, pay, iters):
        Bc, Hc, Wc, f = pay.shape[0], hi_size[0], hi_size[1], hi_size[0] // lo_size[0]
        one = D.RangePrep(ds, lo_size, hi_size, True)
        two = D.RangePrep(ds, lo_size, hi_size, True, in_chans=2)

        def alternative():
            lo0, hi0 = one(pay)
            hi1 = torch.empty_like(hi0)
            lo1 = torch.empty_like(lo0)
            ops.range_prep(pay, 0, Hc * Wc * 2, Wc * 2, 2, 1, hi1, lo1, Bc, Hc, Wc, f, 1, 0, 0, 1.0, False, 0.0, 0.0, False, 0)
            hi1.masked_fill_(hi0 == 0, 0.0)
            lo1.masked_fill_(lo0 == 0, 0.0)
            return lo0, lo1, hi0, hi1
        lo, hi = two(pay)
        lo0, lo1, hi0, hi1 = alternative()
        assert torch.equal(hi[:, 0:1], hi0) and torch.equal(lo[:, 0:1], lo0) and torch.equal(hi[:, 1:2], hi1) and \
            torch.equal(lo[:, 1:2], lo1)
        a, b = paired(alternative, lambda: two(pay), iters, 7)
        ratio = sorted(y / x for x, y in zip(a, b))
        med = lambda v: sorted(v)[len(v) // 2]
        algo2 = Bc * Hc * Wc * (4 * 2 + 2 * (4 + 4 / f))            # 4*Cr bytes per pixel in, C*(4 + 4/f) out
        out[name] = {"workload": f"{ds} B={Bc} {Hc}x{Wc} from (H,W,2) payload, in_chans=2",
                     "alternative": "tulip_range_prep per channel (2 launches) + masked_fill_ per output (4 torch launches); "
                                    "its two channels stay separate (B,1,..) tensors: no concatenation is timed",
                     "alt_ms": med(a), "alt_ms_min_max": [min(a), max(a)], "ms": med(b), "ms_min_max": [min(b), max(b)],
                     "algorithmic_GBps": algo2 / med(b) / 1e6, "ratio_one_launch_over_alt": med(ratio),
                     "ratio_min_max": [ratio[0], ratio[-1]], "pairs": len(a)}
    ch2_record("prep_ch2", "kitti", (16, 1024), (64, 1024), payload, 200)
    big2 = torch.stack([big, torch.rand_like(big)], -1).contiguous()
    ch2_record("prep_large_ch2", "durlar", (32, 2048), (128, 2048), big2, 50)
    del big2
    if "--only" in sys.argv and sys.argv[sys.argv.index("--only") + 1] == "prep":
        print(json.dumps(out, indent=1))
        return
    # ---- inference
    m = tulip_base(img_size=(16, 1024), target_img_size=(64, 1024), patch_size=(1, 4), in_chans=1, window_size=(2, 8),
                   pixel_shuffle=True, circular_padding=True, log_transform=True, patch_unmerging=True).to(dev).eval()
    cfg = O.TulipConfig()
    for Bi in (8, 64):
        lo, hi = O.synthetic_batch(cfg, Bi, seed=2)
        gf = GraphedForward(m, Bi)
        gf(lo.to(dev))
        ms = timed(lambda: gf(), 50)
        out[f"infer_B{Bi}"] = {"workload": f"tulip_base KITTI 16x1024->64x1024 eval forward B={Bi}, graph replay",
                               "ms": ms, "images_per_s": Bi / ms * 1e3}
    # ---- evaluate
    for ds, HW, hw in (("kitti", (64, 1024), (16, 1024)), ("durlar", (128, 2048), (32, 2048))):
        pred, hi, lo = EO.synthetic_eval_case(ds, *HW, *hw, seed=3, log_transform=True)
        ev = EV.RangeEvaluator(ds, hw, HW, True, 0.1, False, False, dev)
        p, l, h_ = pred.to(dev), lo.to(dev), hi.to(dev)
        ms_all = timed(lambda: ev(p, l, h_), 10, warm=2)
        ms_pc = timed(lambda: ev.point_clouds(p, l, h_), 50)
        n = HW[0] * HW[1]
        from tulip_amd import ops
        ms_cd = timed(lambda: ops.chamfer_sq(ev.pcd_gt, n, ev.pcd_pred, n, ev.f64, ev.dist_a, ev.dist_b, ev.scratch,
                                             ev.cd), 10, warm=2)
        ms_vox = timed(lambda: ops.voxel_metrics(ev.pcd_pred, n, ev.pcd_gt, n, ev.f64, 0.1, ev.bm_pred, ev.bm_gt,
                                                 ev.bitmap_words, ev.scratch, ev.vox), 50)
        pairs = 2.0 * n * n
        rec = {"workload": f"{ds} {HW[0]}x{HW[1]} one image", "ms_total": ms_all, "ms_post_and_projection": ms_pc,
               "ms_voxel_metrics": ms_vox, "ms_chamfer": ms_cd, "chamfer_Gpairs_per_s": pairs / ms_cd / 1e6,
               # 8 flops per pair (3 sub, 3 mul/fma, 2 add folded into fma, 1 min counted as 1)
               "chamfer_valu_TFLOPs": pairs * 8 / ms_cd / 1e9, "valu_fp32_peak_TFLOPs": 157.3}
        if ds == "kitti":
            t0 = time.perf_counter()
            mae, mae_low, p_img, t_img = EO.postprocess(pred, hi, lo, ds, True)
            pp, pg = (EO.spherical_pcd(im, EO.kitti_tables(), 80) for im in (p_img, t_img))
            t1 = time.perf_counter()
            EO.voxel_metrics(pp, pg, 0.1)
            t2 = time.perf_counter()
            EO.chamfer_sq(pg, pp)
            t3 = time.perf_counter()
            rec["oracle_cpu_ms"] = {"post_and_projection": (t1 - t0) * 1e3, "voxel_metrics_sparse": (t2 - t1) * 1e3,
                                    "chamfer_bruteforce": (t3 - t2) * 1e3, "threads": torch.get_num_threads()}
        out[f"evaluate_{ds}"] = rec
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()

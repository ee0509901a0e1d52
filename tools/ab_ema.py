"""What the weight average costs (profiles/README.md, "Weight EMA"): bench.py's model and batch -- tulip_base KITTI 16x1024 ->
64x1024, batch 8, the captured step -- on `Trainer(ema_decay=0.999)` and on the Trainer without an average, both in this one
process, both warmed, then timed alternately in blocks of 50 steps between two device events; and the two streaming kernels
alone over the same W.total floats, tulip_ema_update (12 B per element: p read, shadow read and written) and tulip_adamw (30 B per
element as called here: p, g, m, v read, p, m, v and the bf16 shadow written), every launch between its own pair of events, the two
kernels alternating so that neither finds its buffers in the memory-side cache the other just swept.

    python tools/ab_ema.py [--blocks 6] [--block-steps 50] [--launches 200]        one JSON line per block, then a summary line
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6, help="timed blocks per arm (6 x 50 = 300 steps)")
    ap.add_argument("--block-steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--launches", type=int, default=200, help="isolated launches per kernel")
    a = ap.parse_args()
    import torch
    import bench
    from tulip_amd import ops
    from tulip_amd.trainer import Trainer
    if not torch.cuda.is_available():
        sys.exit("tools/ab_ema.py measures on the GPU: no device found")
    dev = torch.device("cuda", 0)
    args = argparse.Namespace(model="tulip_base", img=[16, 1024], target=[64, 1024], batch=8)
    arms = {}
    for name, kw in (("off", {}), ("on", dict(ema_decay=0.999))):
        torch.manual_seed(0)
        model = bench.make_model(args).to(dev).train()
        tr = Trainer(model, 8, lr=5e-4, betas=(0.9, 0.95), weight_decay=0.01, device=dev, **kw)
        tr.load_batch(*bench.synthetic(args, 0, dev))
        for _ in range(a.warmup):
            tr.step()
        arms[name] = tr
    torch.cuda.synchronize()
    assert arms["on"].step_form == arms["off"].step_form == "one_graph"
    ms = {"off": [], "on": []}
    for b in range(a.blocks):
        for name in (("off", "on") if b % 2 == 0 else ("on", "off")):
            tr = arms[name]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.block_steps):
                tr.step()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.block_steps)
            print(json.dumps({"block": b, "ema": name, "ms_per_step": round(ms[name][-1], 5)}), flush=True)
    W = arms["on"].eng.params
    n = W.total
    params = sum(W.numel.values())
    # the two kernels alone, on buffers of their own
    g = torch.Generator(device=dev).manual_seed(1)
    p = torch.randn(n, device=dev, generator=g) * 0.02
    grad = torch.randn(n, device=dev, generator=g) * 1e-3
    m, v, pb = torch.zeros_like(p), torch.zeros_like(p), torch.zeros(n, dtype=torch.bfloat16, device=dev)
    shadow = p.clone()
    counter, omd = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, device=dev)
    hyper = torch.tensor([5e-4, 0.9, 0.95, 1e-8, 0.01, 0.1, 0.05, 1.0], device=dev)
    launch = {"ema": lambda: ops.ema_update(p, shadow, n, 0.999, counter, omd),
              "adamw": lambda: ops.adamw(p, grad, m, v, pb, n, hyper, W.decay_mask)}
    for f in launch.values():
        f()
    torch.cuda.synchronize()
    us = {"ema": [], "adamw": []}
    pairs = []
    for _ in range(a.launches):
        for name, f in launch.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            pairs.append((name, e0, e1))
    torch.cuda.synchronize()
    for name, e0, e1 in pairs:
        us[name].append(e0.elapsed_time(e1) * 1e3)
    bytes_per = {"ema": 12, "adamw": 30}
    med = {k: statistics.median(x) for k, x in us.items()}
    rate = {k: bytes_per[k] * n / (med[k] * 1e-6) / 1e9 for k in us}
    out = {"steps_per_arm": a.blocks * a.block_steps,
           "ms_per_step_off": [round(x, 5) for x in ms["off"]], "ms_per_step_on": [round(x, 5) for x in ms["on"]],
           "mean_off_ms": round(statistics.mean(ms["off"]), 5), "mean_on_ms": round(statistics.mean(ms["on"]), 5),
           "ema_cost_us": round((statistics.mean(ms["on"]) - statistics.mean(ms["off"])) * 1e3, 2),
           "block_spread_off_us": round((max(ms["off"]) - min(ms["off"])) * 1e3, 2),
           "block_spread_on_us": round((max(ms["on"]) - min(ms["on"])) * 1e3, 2),
           "flat_elements": n, "parameters": params,
           "isolated_ema_update_us_median": round(med["ema"], 2), "isolated_adamw_us_median": round(med["adamw"], 2),
           "isolated_ema_update_us_min": round(min(us["ema"]), 2), "isolated_adamw_us_min": round(min(us["adamw"]), 2),
           "ema_update_GBps": round(rate["ema"], 1), "adamw_GBps": round(rate["adamw"], 1),
           "ema_over_adamw_rate": round(rate["ema"] / rate["adamw"], 3), "bytes_per_element": bytes_per,
           "loss_off": float(arms["off"].P.losses[0]), "loss_on": float(arms["on"].P.losses[0])}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

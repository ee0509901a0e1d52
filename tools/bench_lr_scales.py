"""Step time of the captured training step with per-parameter learning-rate scales (profiles/README.md, "Per-parameter
learning-rate scales"): bench.py's model, batch and timing loop -- tulip_base KITTI 16x1024 -> 64x1024, batch 8, 10 warm-up steps,
then 50 timed steps between two synchronisations, wall clock -- on `Trainer(lr_scales=layer_decay_scales(model))` and on the
Trainer without scales, interleaved, each run in a process of its own (bench.py has no switch for the scales).

    python tools/bench_lr_scales.py [--rounds 2]      one JSON line per run, then a summary line
    python tools/bench_lr_scales.py --one 0|1         a single run in this process (what the driver starts)
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one(scaled: bool, steps: int, warmup: int) -> dict:
    import torch
    import bench
    from tulip_amd.trainer import Trainer, layer_decay_scales
    args = argparse.Namespace(model="tulip_base", img=[16, 1024], target=[64, 1024], batch=8)
    dev = torch.device("cuda", 0)
    model = bench.make_model(args).to(dev).train()
    tr = Trainer(model, 8, lr=5e-4, betas=(0.9, 0.95), weight_decay=0.01, device=dev,
                 lr_scales=layer_decay_scales(model) if scaled else None)
    tr.load_batch(*bench.synthetic(args, 0, dev))
    for _ in range(warmup):
        tr.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    sites = list(tr.adamw_sites().values())
    return {"lr_scales": scaled, "groups": len(set(tr.lr_scales.values())), "ms_per_step": round(dt / steps * 1e3, 4),
            "tensors_per_site": {s: sites.count(s) for s in ("writeout", "fold", "blocks", "scan")},
            "loss": float(tr.P.losses[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", type=int, choices=[0, 1])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if a.one is not None:
        print(json.dumps(one(bool(a.one), a.steps, a.warmup)), flush=True)
        return
    res = {0: [], 1: []}
    for _ in range(a.rounds):
        for scaled in (0, 1):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(scaled), "--steps", str(a.steps),
                                "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit(f"run failed ({r.returncode}):\n{r.stdout[-1000:]}{r.stderr[-3000:]}")
            line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
            print(line, flush=True)
            res[scaled].append(json.loads(line)["ms_per_step"])
    print(json.dumps({"ms_per_step_without_scales": res[0], "ms_per_step_with_layer_decay_scales": res[1]}), flush=True)


if __name__ == "__main__":
    main()

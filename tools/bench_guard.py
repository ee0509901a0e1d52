"""Step time of the captured training step with the non-finite guard (profiles/README.md, "Non-finite guard"): bench.py's model,
batch and timing loop -- tulip_base KITTI 16x1024 -> 64x1024, batch 8, 10 warm-up steps, then 50 timed steps between two
synchronisations, wall clock -- on four Trainers, interleaved, each run in a process of its own (bench.py has no switch for
any of them; tools/bench_clip.py is the model):

    default      Trainer(...)                                                        the default plan: AdamW in the write-outs and fold launches
    grad_norm    Trainer(track_grad_norm=True)                                       the norm-first plan: the norm in front of one end-of-step AdamW
    guard        Trainer(skip_nonfinite=True)                                        the same plan + tulip_step_guard, gated AdamW
    guard_full   Trainer(skip_nonfinite=True, clip_grad=1.0, ema_decay=0.999)        ... with clipping and the gated weight average

`guard` launches one single-workgroup kernel more than `grad_norm`; the default plan launches none of this.

    python tools/bench_guard.py [--rounds 3]          one JSON line per run, then a summary line (per arm: the runs, min, max)
    python tools/bench_guard.py --one default|grad_norm|guard|guard_full      a single run in this process (what the driver starts)
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VARIANTS = {"default": {}, "grad_norm": dict(track_grad_norm=True), "guard": dict(skip_nonfinite=True),
            "guard_full": dict(skip_nonfinite=True, clip_grad=1.0, ema_decay=0.999)}


def one(variant: str, steps: int, warmup: int) -> dict:
    import torch
    import bench
    from tulip_amd.trainer import Trainer
    args = argparse.Namespace(model="tulip_base", img=[16, 1024], target=[64, 1024], batch=8)
    dev = torch.device("cuda", 0)
    model = bench.make_model(args).to(dev).train()
    kw = VARIANTS[variant]
    tr = Trainer(model, 8, lr=5e-4, betas=(0.9, 0.95), weight_decay=0.01, device=dev, **kw)
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
    guarded = bool(kw.get("skip_nonfinite"))
    return {"variant": variant, "ms_per_step": round(dt / steps * 1e3, 4), "fuse_adamw": bool(tr.fuse_adamw),
            "tensors_per_site": {s: sites.count(s) for s in ("writeout", "fold", "blocks", "scan")},
            "grad_norm": float(tr.grad_norm) if variant != "default" else None,
            "applied_steps": tr.applied_steps if guarded else tr.t, "skipped_steps": tr.skipped_steps if guarded else None,
            "loss": float(tr.P.losses[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", choices=list(VARIANTS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if a.one is not None:
        print(json.dumps(one(a.one, a.steps, a.warmup)), flush=True)
        return
    res = {v: [] for v in VARIANTS}
    for _ in range(a.rounds):
        for v in VARIANTS:
            r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--one", v, "--steps", str(a.steps),
                                "--warmup", str(a.warmup)], capture_output=True, text=True)
            if r.returncode != 0:
                sys.exit(f"run failed ({r.returncode}):\n{r.stdout[-1000:]}{r.stderr[-3000:]}")
            line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
            print(line, flush=True)
            res[v].append(json.loads(line)["ms_per_step"])
    print(json.dumps({"ms_per_step": res, "spread": {v: [min(x), max(x)] for v, x in res.items()}}), flush=True)


if __name__ == "__main__":
    main()

"""Step time of the captured training step per training loss (profiles/README.md, "Training loss"): bench.py's model, batch and
timing loop -- tulip_base KITTI 16x1024 -> 64x1024, batch 8, 10 warm-up steps, then 50 timed steps between two synchronisations,
wall clock -- on six Trainers, interleaved, each run in a process of its own (bench.py has no switch for the loss;
tools/bench_guard.py is the model):

    l1       TULIP(...)                  the default: the head kernels form sign(pred - target) / n themselves
    l2       TULIP(..., loss="l2")       + tulip_loss_bwd on the chain in front of the head's backward (the statistics pass beside it)
    berhu    TULIP(..., loss="berhu")    + tulip_loss_stats behind the head's forward and tulip_loss_bwd in front of its backward
    l1_m, l2_m, berhu_m                  the same losses over the valid pixels only, TULIP(..., loss_valid_min=0.0), on the seeded batch
                                         (10 % of its target pixels are 0): tulip_loss_stats_m behind the head's forward and
                                         tulip_loss_bwd_m in front of its backward, for every kind
    l1_e, l2_e, berhu_e                  the same losses with the edge term, TULIP(..., loss_edge_weight=0.5) (--edge-weight): tulip_loss_edge_stats
                                         and tulip_loss_edge_final behind the base loss's final launch, tulip_loss_edge_bwd in front of the
                                         head's backward; l1_e also gives up the in-head sign and pays the dpred launch l2 pays
    l1_c2                                the default loss on the two-channel model (in_chans=2: the seeded batch's range plus a seeded
                                         intensity channel in [0, 1]) -- what the three arms below stand beside
    l1_w, berhu_w                        in_chans=2 with TULIP(..., loss_channel_weights=(1.0, 0.25)) (--channel-weights): the _w launches
                                         in the places of the _m ones; l1_w gives up the in-head sign as l1_m does
    berhu_mew                            in_chans=2 with the mask, the edge term and the weights together

    python tools/bench_loss.py [--rounds 3]          one JSON line per run, then a summary line (per arm: the runs, min, max)
    python tools/bench_loss.py --parent DIR          ... with one more arm, "parent_l1": the `l1` run of the built checkout of another
                                                     commit at DIR (its own tools/bench_loss.py --one l1), in every round
    python tools/bench_loss.py --arms l1,l1_e,l2,berhu,berhu_e      ... these arms only
    python tools/bench_loss.py --one l1|l2|berhu|l1_m|...|berhu_e     a single run in this process (what the driver starts)
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KINDS = ("l1", "l2", "berhu")
VARIANTS = KINDS + tuple(k + "_m" for k in KINDS) + tuple(k + "_e" for k in KINDS) + ("l1_c2", "l1_w", "berhu_w", "berhu_mew")
TWO_CHANNEL = ("l1_c2", "l1_w", "berhu_w", "berhu_mew")


def one(variant: str, steps: int, warmup: int, edge_weight: float = 0.5, channel_weights=(1.0, 0.25)) -> dict:
    import torch
    from tulip_amd.model import tulip as T
    import bench
    from tulip_amd.trainer import Trainer
    args = argparse.Namespace(model="tulip_base", img=[16, 1024], target=[64, 1024], batch=8)
    dev = torch.device("cuda", 0)
    kind, masked, edge = variant.split("_")[0], variant.endswith("_m"), variant.endswith("_e")
    chans = 2 if variant in TWO_CHANNEL else 1
    weighted = variant in ("l1_w", "berhu_w", "berhu_mew")
    if variant == "berhu_mew":
        masked = edge = True
    torch.manual_seed(0)                     # bench.make_model's model, with the loss keywords
    model = T.tulip_base(img_size=tuple(args.img), target_img_size=tuple(args.target), patch_size=(1, 4), in_chans=chans,
                         window_size=[2, 8], swin_v2=False, pixel_shuffle=True, circular_padding=True, log_transform=True,
                         patch_unmerging=True, loss=kind, **(dict(loss_valid_min=0.0) if masked else {}),
                         **(dict(loss_edge_weight=edge_weight) if edge else {}),
                         **(dict(loss_channel_weights=tuple(channel_weights)) if weighted else {})).to(dev).train()
    tr = Trainer(model, 8, lr=5e-4, betas=(0.9, 0.95), weight_decay=0.01, device=dev)
    lo, hi = bench.synthetic(args, 0, dev)
    if chans == 2:                           # + an intensity channel in [0, 1], seeded; the low-resolution input is every fourth row
        it = torch.rand(hi.shape, generator=torch.Generator().manual_seed(4321)).to(dev)
        hi = torch.cat([hi, it], dim=1)
        lo = hi[:, :, 0::args.target[0] // args.img[0], :].contiguous()
    tr.load_batch(lo, hi)
    for _ in range(warmup):
        tr.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"variant": variant, "ms_per_step": round(dt / steps * 1e3, 4), "loss": float(tr.P.losses[0]),
            "pixel_loss": float(tr.P.losses[1]), "loss_c": float(tr.loss_c) if kind == "berhu" else None,
            "loss_valid": int(tr.loss_valid) if masked or weighted else None, "edge_loss": float(tr.edge_loss) if edge else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", choices=list(VARIANTS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--edge-weight", type=float, default=0.5, help="loss_edge_weight of the _e arms")
    ap.add_argument("--channel-weights", type=lambda t: tuple(float(x) for x in t.split(",")), default=(1.0, 0.25),
                    help="loss_channel_weights of the _w arms and berhu_mew (two floats, comma-separated)")
    ap.add_argument("--arms", help="comma-separated subset of the arms (default: all)")
    ap.add_argument("--parent", help="a built checkout of another commit: its l1 arm runs beside these")
    a = ap.parse_args()
    if a.one is not None:
        print(json.dumps(one(a.one, a.steps, a.warmup, a.edge_weight, a.channel_weights)), flush=True)
        return
    chosen = tuple(a.arms.split(",")) if a.arms else VARIANTS
    if set(chosen) - set(VARIANTS):
        sys.exit(f"unknown arms {sorted(set(chosen) - set(VARIANTS))}: choose from {VARIANTS}")
    arms = (("parent_l1",) if a.parent else ()) + chosen
    res = {v: [] for v in arms}
    for _ in range(a.rounds):
        for v in arms:
            script = os.path.join(os.path.abspath(a.parent), "tools", "bench_loss.py") if v == "parent_l1" else os.path.abspath(__file__)
            r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, script, "--one", "l1" if v == "parent_l1" else v,
                                "--steps", str(a.steps), "--warmup", str(a.warmup)] +
                               ([] if v == "parent_l1" else ["--edge-weight", str(a.edge_weight), "--channel-weights",
                                                             ",".join(map(str, a.channel_weights))]), capture_output=True, text=True)
            if r.returncode != 0:
                sys.exit(f"run failed ({r.returncode}):\n{r.stdout[-1000:]}{r.stderr[-3000:]}")
            line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            line["variant"] = v
            print(json.dumps(line), flush=True)
            res[v].append(line["ms_per_step"])
    print(json.dumps({"ms_per_step": res, "spread": {v: [min(x), max(x)] for v, x in res.items()}}), flush=True)


if __name__ == "__main__":
    main()

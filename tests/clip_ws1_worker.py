"""Worker of tests/test_clip_gpu.py::test_one_rank_rccl_plans: ONE rank on the `nccl` backend (= RCCL on ROCm) with the N > 1 step
structure forced on (tests/ema_ws1_worker.py is the model) and gradient clipping.  Per plan -- graph segments with the end-of-step
AdamW graph, the same with the bf16 gradient exchange, the one graph with captured collectives -- every optimizer step is checked
against the host definition (tests/clip_check.py: coefficient bit for bit, norm against float64, every update audited with the
clipped gradient scale), and the final master / moments are compared bit for bit with the one-GPU Trainer's under the same
clip_grad.  Tiny model, batch 4, small buckets (several all-reduces).  The results go to the file named on the command line."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    out_path, steps, clip = sys.argv[1], int(sys.argv[2]), float(sys.argv[3])
    from tests.clip_check import clipped_steps, differing, state_bits
    from tests.test_clip_gpu import tiny
    from tulip_amd.trainer import Trainer
    torch.cuda.set_device(0)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29559")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    res, final = {}, {}
    for name, kw, graph_collectives in [("one_gpu", dict(), "0"),
                                        ("segments", dict(force_segments=True, bucket_mb=0.25), "0"),
                                        ("bf16", dict(force_segments=True, bucket_mb=0.25, grad_dtype="bf16"), "0"),
                                        ("captured", dict(force_segments=True, bucket_mb=0.25), "1")]:
        os.environ["TULIP_GRAPH_COLLECTIVES"] = graph_collectives
        m, lo, hi = tiny()
        tr = Trainer(m, 4, clip_grad=clip, **kw)
        tr.load_batch(lo, hi)
        failures, seen = clipped_steps(tr, steps)
        torch.cuda.synchronize()
        final[name] = state_bits(tr)
        res[name] = {"failures": failures, "seen": seen, "t": tr.t, "form": tr.step_form, "segmented": tr.segmented,
                     "buckets": len(tr.bucketer.buckets), "bucket_adamw": tr.bucket_adamw, "fuse_adamw": tr.fuse_adamw,
                     "gb": tr.gb is not None, "differs_from_one_gpu": differing(final["one_gpu"], final[name])}
        del tr, m
        torch.cuda.synchronize()
    res["backend"] = dist.get_backend()
    torch.save(res, out_path)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

"""Worker of tests/test_guard_gpu.py::test_one_rank_rccl_plans: ONE rank on the `nccl` backend (= RCCL on ROCm) with the N > 1 step
structure forced on (tests/clip_ws1_worker.py is the model) and the non-finite guard.  Per plan -- graph segments with the
end-of-step AdamW graph, the same with the bf16 gradient exchange, the one graph with captured collectives -- the skip test (a batch
with a NaN sample: nothing of the training state changes, the counters move) and the recovery test (good, good, bad, good, good
against four good steps) of tests/guard_check.py.  Tiny model, batch 4, small buckets (several all-reduces).  The results go to
the file named on the command line."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    out_path = sys.argv[1]
    from tests.guard_check import recovery_failures, skipped_step_failures, tiny
    from tulip_amd.trainer import Trainer
    torch.cuda.set_device(0)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29561")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    res = {}
    for name, kw, graph_collectives in [("segments", dict(force_segments=True, bucket_mb=0.25), "0"),
                                        ("bf16", dict(force_segments=True, bucket_mb=0.25, grad_dtype="bf16"), "0"),
                                        ("captured", dict(force_segments=True, bucket_mb=0.25), "1")]:
        os.environ["TULIP_GRAPH_COLLECTIVES"] = graph_collectives
        m, lo, hi, bad_lo = tiny()
        tr = Trainer(m, 4, skip_nonfinite=True, ema_decay=0.5, **kw)
        skip = skipped_step_failures(tr, lo, hi, bad_lo=bad_lo)
        torch.cuda.synchronize()
        res[name] = {"skip": skip, "form": tr.step_form, "segmented": tr.segmented, "buckets": len(tr.bucketer.buckets),
                     "bucket_adamw": tr.bucket_adamw, "fuse_adamw": tr.fuse_adamw, "gb": tr.gb is not None}
        del tr, m

        def make():
            m, lo, hi, bad_lo = tiny(drop_path=0.0)
            return Trainer(m, 4, skip_nonfinite=True, ema_decay=0.9, **kw), lo, hi, bad_lo

        res[name]["recovery"] = recovery_failures(make, "batch")
        torch.cuda.synchronize()
    res["backend"] = dist.get_backend()
    torch.save(res, out_path)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

"""Worker of tests/test_ema_gpu.py::test_one_rank_rccl_plans: ONE rank on the `nccl` backend (= RCCL on ROCm) with the N > 1 step
structure forced on (tests/lr_scales_ws1_worker.py is the model) and a weight average kept by the Trainer.  Per plan -- graph
segments with the end-of-step AdamW graph, bucket_adamw, the one graph with captured collectives -- the average after every
optimizer step is compared bit for bit with the host definition applied to snapshots of the parameters (tests/ema_check.py).
The results go to the file named on the command line."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    out_path, steps = sys.argv[1], int(sys.argv[2])
    from tests.ema_check import tracked_steps
    from tests.test_adamw_audit_gpu import batch, make
    from tulip_amd.trainer import Trainer
    torch.cuda.set_device(0)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29557")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    res = {}
    for name, kw, graph_collectives in [("segments", dict(), "0"),
                                        ("bucket_adamw", dict(bucket_adamw=True), "0"),
                                        ("captured", dict(), "1")]:
        os.environ["TULIP_GRAPH_COLLECTIVES"] = graph_collectives
        m = make()
        tr = Trainer(m, 8, force_segments=True, ema_decay=0.999, **kw)
        tr.load_batch(*batch(m, 8))
        failures, updates, _ = tracked_steps(tr, steps)
        res[name] = {"failures": failures, "updates": updates, "num_updates": tr.ema.num_updates, "form": tr.step_form,
                     "segmented": tr.segmented, "buckets": len(tr.bucketer.buckets), "bucket_adamw": tr.bucket_adamw}
        del tr, m
        torch.cuda.synchronize()
    res["backend"] = dist.get_backend()
    torch.save(res, out_path)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

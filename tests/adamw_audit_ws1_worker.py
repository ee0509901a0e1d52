"""Worker of tests/test_adamw_audit_gpu.py::test_one_rank_rccl_plans: ONE rank on the `nccl` backend (= RCCL on ROCm) with the
N > 1 step structure forced on, every optimizer step of each plan audited (tests/adamw_audit.py) on the device.  The results
(violations, step form, bucket count) go to the file named on the command line."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    out_path, steps = sys.argv[1], int(sys.argv[2])
    from tests import adamw_audit as AA
    from tests.test_adamw_audit_gpu import audited_steps, batch, make
    from tulip_amd.trainer import Trainer
    torch.cuda.set_device(0)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29551")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    res = {}
    # (the gradient buffer is cleared, exchanged or reduce-scattered by these plans: gradient-unknown mode)
    for name, kw, graph_collectives in [("segments", dict(), "0"),
                                        ("captured", dict(), "1"),
                                        ("bucket_adamw", dict(bucket_adamw=True), "0"),
                                        ("bf16", dict(grad_dtype="bf16"), "0"),
                                        ("sharded", dict(exchange="sharded"), "0")]:
        os.environ["TULIP_GRAPH_COLLECTIVES"] = graph_collectives
        m = make()
        tr = Trainer(m, 8, force_segments=True, **kw)
        tr.load_batch(*batch(m, 8))
        v, _, _ = audited_steps(tr, steps, "unknown")
        res[name] = {"violations": v, "form": tr.step_form, "segmented": tr.segmented, "buckets": len(tr.bucketer.buckets),
                     "bucket_adamw": tr.bucket_adamw, "gb": tr.gb is not None}
        del tr, m
        torch.cuda.synchronize()
    res["backend"] = dist.get_backend()
    torch.save(res, out_path)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

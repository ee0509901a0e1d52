"""Worker of tests/test_lr_scales_gpu.py::test_one_rank_segmented_plans: ONE rank on the `nccl` backend (= RCCL on ROCm) with
the N > 1 step structure forced on (tests/adamw_audit_ws1_worker.py is the model), three learning-rate scales over the
tensors, every optimizer step of each plan audited group by group (tests/lr_scale_audit.py).  The results go to the file named
on the command line."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    out_path, steps = sys.argv[1], int(sys.argv[2])
    from tests.lr_scale_audit import audited_steps_scaled, sites_seen
    from tests.test_adamw_audit_gpu import batch, lr_at, make
    from tests.test_lr_scales_gpu import three_scales
    from tulip_amd.trainer import Trainer
    torch.cuda.set_device(0)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29553")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    res = {}
    # (the gradient buffer is cleared or exchanged by these plans: gradient-unknown mode)
    for name, kw in [("segments", dict()), ("bucket_adamw", dict(bucket_adamw=True)), ("bf16", dict(grad_dtype="bf16"))]:
        os.environ["TULIP_GRAPH_COLLECTIVES"] = "0"
        m = make()
        scales = three_scales(m)
        tr = Trainer(m, 8, force_segments=True, lr_scales=scales, **kw)
        tr.load_batch(*batch(m, 8))
        v, _, _ = audited_steps_scaled(tr, steps, "unknown", scales, lr_at)
        res[name] = {"violations": v, "form": tr.step_form, "segmented": tr.segmented, "buckets": len(tr.bucketer.buckets),
                     "bucket_adamw": tr.bucket_adamw, "gb": tr.gb is not None,
                     "sites": {k: sorted(s) for k, s in sites_seen(tr, scales).items()}}
        del tr, m
        torch.cuda.synchronize()
    m = make()
    try:
        Trainer(m, 8, force_segments=True, exchange="sharded", lr_scales=three_scales(m))
        res["sharded_raises"] = False
    except ValueError as e:
        res["sharded_raises"] = "sharded" in str(e)
    tr = Trainer(m, 8, force_segments=True, exchange="sharded", lr_scales={n: 1.0 for n in three_scales(m)})    # all ones: accepted
    res["sharded_ones_ok"] = tr.exchange == "sharded" and tr._lr_table is None
    res["backend"] = dist.get_backend()
    torch.save(res, out_path)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

"""GPU, round 3: the parity holes of VERDICT round 2 -- the bench's own configuration against the oracle, the reference's
unchanged calling convention on the drop-in module, `bench.py --gpus N` without a launcher, the GEMM panel touch
bit-compare, and stale fragment-major copies across plans (ADVICE)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import tulip_oracle as O
from tests.test_model_gpu import build, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kitti_b8_train_step_vs_oracle():
    """BASELINE.json configs[1] exactly as bench.py runs it: tulip_base, KITTI 16x1024 -> 64x1024, per-GPU batch 8, TRAIN
    mode (DropPath live, draws injected so the oracle sees the same ones), ONE graphed Trainer.step -- the only
    configuration where C = 384 runs fused with one window per workgroup, the stage groups are sized for 8 and the step is
    a captured HIP graph.  Loss, every parameter gradient and the post-AdamW parameters against the oracle's fp32 autograd
    + torch.optim.AdamW (main_lidar_upsampling.py:282-283 grouping)."""
    from tulip_amd.trainer import Trainer
    B = 8
    cfg = O.tulip_base_config()
    sd = O.key_seeded_state_dict(cfg, seed=31)
    lo, hi = O.synthetic_batch(cfg, B, seed=41)
    m = build(cfg, sd, train=True)
    lr, wd, betas = 5e-4, 0.01, (0.9, 0.95)
    tr = Trainer(m, B, lr=lr, betas=betas, weight_decay=wd)
    eng, W = tr.eng, tr.eng.params
    assert all(eng._fused_bwd(sp, B) for sp in eng.blocks if sp.C in (96, 192, 384))      # the bench's kernel mix ...
    assert all(eng._fusable_deep(sp, B) for sp in eng.blocks if sp.C == 768)               # ... round 5: the deep stage's sliced launches (32 windows)
    g = torch.Generator().manual_seed(7)
    table = torch.zeros(eng.n_drop_slots, B)
    du = {}
    for sp in eng.blocks:
        if sp.slot >= 0:
            u = torch.rand(2, B, generator=g)
            table[sp.slot:sp.slot + 2] = u
            du[sp.prefix] = u
    assert len(du) == 12                       # 14 blocks; rate 0 for encoder block 0 and its decoder twin (tulip.py:409-410,447)
    tr.inject_drop_u = table.to(DEV)
    tr.load_batch(lo.to(DEV), hi.to(DEV))
    p0 = W.flat.clone()
    # the gradients of the step, from an eager pass of the same launch sequence (deterministic reductions: same bits)
    tr._fwd_bwd(lambda tag: None)
    torch.cuda.synchronize()
    g_hip, loss_eager = tr.g.clone(), tr.P.losses.clone()
    tr.g.zero_()
    losses = tr.step().clone()                 # captures the HIP graph and replays it
    torch.cuda.synchronize()
    assert tr._segments is not None and len(tr._segments[True]) == 1
    assert torch.equal(losses, loss_eager)
    if tr.grad_overwrite:                      # the backward writes (does not add to) the buffer: it still holds the step's gradients,
        # bit for bit those of the eager pass -- except for the tensors whose optimizer step was taken in their weight-gradient
        # write-out (Trainer.fuse_adamw): their gradient is never stored (the buffer keeps the zeros put there above)
        stepped = torch.zeros(W.total, dtype=torch.bool, device=DEV)
        if tr._adam_mask is not None:
            stepped = ((tr._adam_mask & 2) != 0).repeat_interleave(64)[:W.total]
            assert tr.fused_adamw_params > 0.8 * sum(W.numel[n] for n in W.names)      # the deep stages: most of the model
        assert torch.equal(tr.g[~stepped], g_hip[~stepped]) and float(tr.g[stepped].abs().max() if stepped.any() else 0.0) == 0.0
    else:
        assert float(tr.g.abs().max()) == 0.0  # consumed and cleared by the fused AdamW
    p1 = W.flat.clone()
    dropped = sum(int((torch.floor(1 - sp.rate + du[sp.prefix]) == 0).sum()) for sp in eng.blocks if sp.slot >= 0)
    assert dropped > 0                         # the draw really drops some (sample, branch) pairs

    _, oloss, opix, og = O.tulip_loss_and_grads(sd, cfg, lo, hi, drop_u=du)
    assert abs(losses[0].item() - oloss.item()) <= 1e-3 * oloss.item(), (losses[0].item(), oloss.item())
    assert abs(losses[1].item() - opix.item()) <= 2e-3 * opix.item()
    worst, worst_t = 0.0, 0.0
    for n in W.names:
        gh = g_hip[W.offset[n]:W.offset[n] + W.numel[n]].view(W.shape[n])
        e = rel_l2(gh, og[n])
        table_ = n.endswith("relative_position_bias_table")
        assert e <= (1e-1 if table_ else 1.5e-2), (n, e)
        worst, worst_t = (worst, max(worst_t, e)) if table_ else (max(worst, e), worst_t)
    print(f"KITTI base B=8 train step: worst per-tensor rel L2 gradient error vs fp32 oracle {worst:.3e} (tables {worst_t:.3e})")

    # AdamW.  (i) exact arithmetic: torch.optim.AdamW fed with the HIP gradients must land on the fused kernel's
    # parameters (fp32, same formula); (ii) fed with the ORACLE's gradients: after one Adam step every element moves by
    # ~lr * sign(g), so elements whose gradient is smaller than the bf16 noise may differ by 2 lr -- bounded in bulk.
    for src in ("hip", "oracle"):
        ps = {n: p0[W.offset[n]:W.offset[n] + W.numel[n]].view(W.shape[n]).clone().requires_grad_(True) for n in W.names}
        opt = torch.optim.AdamW([{"params": [p for p in ps.values() if p.ndim <= 1], "weight_decay": 0.0},
                                 {"params": [p for p in ps.values() if p.ndim > 1], "weight_decay": wd}], lr=lr, betas=betas)
        for n, p in ps.items():
            p.grad = (g_hip[W.offset[n]:W.offset[n] + W.numel[n]].view(W.shape[n]).clone() if src == "hip"
                      else og[n].to(DEV))
        opt.step()
        big, tot, maxd = 0, 0, 0.0
        for n, p in ps.items():
            d = (p.detach() - p1[W.offset[n]:W.offset[n] + W.numel[n]].view(W.shape[n])).abs()
            maxd = max(maxd, d.max().item())
            big += int((d > 0.25 * lr).sum()); tot += d.numel()
        print(f"post-AdamW parameters vs torch.optim.AdamW on the {src} gradients: max |d| {maxd:.3e} ({maxd / lr:.3f} lr), "
              f"{big / tot:.4%} of elements off by more than lr/4")
        if src == "hip":
            assert maxd <= 2e-3 * lr, maxd
        else:
            assert maxd <= 2.05 * lr and big / tot <= 0.03, (maxd, big / tot)


def test_reference_loop_body_on_the_dropin(golden_dir, tmp_path):
    """The reference's calling convention, executed: autocast + GradScaler(65 536) + torch.optim.AdamW over timm groups +
    DistributedDataParallel over a one-rank nccl group (tests/refloop_worker.py restates engine_upsampling.py:69-100 and
    misc.py:292-305) against fixture g7 (the REFERENCE model under the same loop in fp32): losses within 2e-3, the scale
    never backs off (no inf-skips), gradient norms finite."""
    z = np.load(os.path.join(golden_dir, "g7_train_trajectory.npz"))
    out = tmp_path / "refloop.pt"
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29547")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "refloop_worker.py"), str(out), str(int(z["seed"])),
                        str(int(z["batch"])), str(int(z["data_seed"])), "4"], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = torch.load(out)
    assert got["backend"] == "nccl" and got["finite"]
    ref = z["loss"].tolist()
    print("reference-loop losses", [round(v, 6) for v in got["losses"]], "g7", [round(v, 6) for v in ref])
    for a, b in zip(got["losses"], ref):
        assert abs(a - b) <= 2e-3 * b, (got["losses"], ref)
    assert got["scales"] == [65536.0] * 4                     # GradScaler never found an inf/nan and never skipped a step
    assert all(np.isfinite(v) and v > 0 for v in got["norms"])


@pytest.mark.parametrize("exchange", ["allreduce", "sharded"])
def test_bench_self_spawns_its_ranks(exchange):
    """`python bench.py --gpus 2` with NO launcher in the environment (the driver's command line) must start its two ranks
    itself and print ONE JSON line from rank 0.  One GPU here, so the ranks share it over gloo (TULIP_BENCH_BACKEND);
    on a multi-GPU node the same entry point uses RCCL."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update(TULIP_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "2"]
                       + (["--exchange", "sharded"] if exchange == "sharded" else []),
                       env=env, capture_output=True, text=True, timeout=1200, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 16 and d["config"]["parallelism"] == "dp2"
    assert d["steps"] == 3 and d["warmup"] == 2 and d["value"] > 0
    ss = d["config"]["step_structure"]          # what the timed step was, without opening `comm`
    assert ss["form"] == "segments+detached_buckets" and ss["graph_segments"] >= 3 and ss["detached_bucket_graphs"] >= 3
    assert ss["ladder_rung"] == 0 and ss["after_failed"] == []
    assert ss["exchange"] == exchange        # (all-reduce plans: the chooser decides where the optimizer step goes)
    assert ss["optimizer"] in (("sharded_per_bucket",) if exchange == "sharded" else ("end_of_step", "per_bucket"))
    c = d["comm"]
    assert c["world_size_rccl"] == 2 and c["launcher"] == "bench.py spawn_ranks"
    assert c["collective_smoke"]["bucket"]["bytes"] == 66 << 20 and c["collective_smoke"]["bucket"]["busbw_GBps"] > 0
    assert len(c["buckets_MB"]) >= 3 and "NCCL_MIN_NCHANNELS" in c["env"]


def test_gemm_panel_touch_changes_no_bit():
    """The split first touch of the cold weight panel (csrc/gemm.hip, LDS-destination loads whose data is dropped) must not
    change a bit of any GEMM result: forward and data-gradient forms, split-K and fused-epilogue launches, on vs off."""
    from tulip_amd import ops
    from tulip_amd._lib import EPI_BF16, EPI_F32
    torch.manual_seed(3)
    outs = {}
    for on in (True, False):
        res = []
        for (M, N, K, bt) in [(512, 768, 768, False), (512, 768, 3072, False), (2048, 384, 1536, True), (32768, 96, 288, True),
                              (4096, 192, 192, False), (77, 96, 64, False)]:
            g = torch.Generator(device=DEV).manual_seed(M + N + K)
            A = torch.randn(M, K, device=DEV, generator=g).bfloat16()
            Wt = (torch.randn(K, N, device=DEV, generator=g) if bt else torch.randn(N, K, device=DEV, generator=g)).bfloat16()
            bias = torch.randn(N, device=DEV, generator=g)
            o16 = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
            o32 = torch.zeros(M, N, device=DEV)
            ws = torch.zeros(8 * M * N, device=DEV)
            ops.gemm(A, Wt, M, N, K, lda=K, ldb=N if bt else K, b_trans=bt, epi=EPI_BF16, bias=bias, out=o16, ldo=N, touch=on)
            ops.gemm(A, Wt, M, N, K, lda=K, ldb=N if bt else K, b_trans=bt, epi=EPI_F32, out=o32, ldo=N, splits=4,
                     workspace=ws.data_ptr(), workspace_bytes=ws.numel() * 4, touch=on)
            torch.cuda.synchronize()
            res += [o16.clone(), o32.clone()]
        outs[on] = res
    for a, b in zip(outs[True], outs[False]):
        assert torch.isfinite(a.float()).all() and a.float().abs().max() > 0
        assert torch.equal(a, b)


def test_graphed_forward_after_a_trainer_of_another_batch_size_sees_fresh_weights():
    """a Trainer captured at batch 4 (KITTI size: C = 384 runs unfused there) and, after it has stepped, a
    GraphedForward at batch 8 (C = 384 fused: streams the fragment-major weight copies).  The copies of EVERY fusable width
    are maintained by the captured AdamW from the start, so the batch-8 forward must see the updated weights."""
    from tulip_amd.infer import GraphedForward
    from tulip_amd.trainer import Trainer
    cfg = O.tulip_base_config()
    sd = O.key_seeded_state_dict(cfg, seed=5)
    m = build(cfg, sd, train=True)
    lo4, hi4 = O.synthetic_batch(cfg, 4, seed=9)
    tr = Trainer(m, 4, lr=5e-3, betas=(0.9, 0.95), weight_decay=0.01)      # large lr: stale weights would show
    tr.load_batch(lo4.to(DEV), hi4.to(DEV))
    tr.step()
    lo8, hi8 = O.synthetic_batch(cfg, 8, seed=10)
    gf = GraphedForward(m, 8)
    for _ in range(3):
        tr.step()
    torch.cuda.synchronize()
    m.eval()
    got = gf(lo8.to(DEV)).clone()
    with torch.no_grad():
        ref = m(lo8.to(DEV), hi8.to(DEV), mc_drop=True)       # autograd_forward refreshes every copy before it runs
    torch.cuda.synchronize()
    assert torch.equal(got, ref), (got - ref).abs().max().item()


def test_torch_adamw_state_round_trip_and_continuation():
    """a run of the reference's optimizer (torch.optim.AdamW over timm-style groups, main:282-283) continues
    with the fused step -- Trainer.import_torch_optimizer -- and back (export_torch_optimizer): two steps with torch.optim.AdamW
    through the module's own forward / backward, then one more step either way must land on the same parameters."""
    from tulip_amd.trainer import Trainer
    cfg = O.tiny_config(drop_path_rate=0.0)
    sd = O.key_seeded_state_dict(cfg, seed=3)
    lo, hi = O.synthetic_batch(cfg, 4, seed=77)
    lo, hi = lo.to(DEV), hi.to(DEV)

    def groups(m):
        return [{"params": [p for p in m.parameters() if p.ndim <= 1], "weight_decay": 0.0},
                {"params": [p for p in m.parameters() if p.ndim > 1], "weight_decay": 0.01}]

    def torch_step(m, opt):
        opt.zero_grad()
        _, loss, _ = m(lo, hi)
        loss.backward()
        opt.step()

    ma = build(cfg, sd, train=True)
    oa = torch.optim.AdamW(groups(ma), lr=5e-4, betas=(0.9, 0.95))
    for _ in range(2):
        torch_step(ma, oa)
    mb = build(cfg, {k: v.clone() for k, v in ma.state_dict().items()}, train=True)
    ob = torch.optim.AdamW(groups(mb), lr=5e-4, betas=(0.9, 0.95))
    ob.load_state_dict(oa.state_dict())              # what misc.load_model does with a reference checkpoint (misc.py:386-390)
    tr = Trainer(mb, 4, lr=1.0, betas=(0.5, 0.5), weight_decay=0.3)          # every hyper-parameter must come from the import
    tr.import_torch_optimizer(ob)
    assert tr.t == 2 and tr.lr == 5e-4 and tuple(tr.betas) == (0.9, 0.95) and tr.wd == 0.01
    tr.load_batch(lo, hi)
    tr.step()
    torch_step(ma, oa)                               # the uninterrupted reference-optimizer run
    torch.cuda.synchronize()
    pa, pb = dict(ma.named_parameters()), dict(mb.named_parameters())
    worst = max((pa[n] - pb[n]).abs().max().item() for n in pa)
    print(f"step 3 with the fused AdamW after import vs torch.optim.AdamW: max |d param| {worst:.3e} ({worst / 5e-4:.4f} lr)")
    assert worst <= 0.1 * 5e-4           # the two forwards / backwards are the same kernels: only the AdamW arithmetic differs
    # and back: the exported state is the imported one advanced by a step
    oc = torch.optim.AdamW(groups(mb), lr=1.0)
    tr.export_torch_optimizer(oc)
    sa, sc = oa.state_dict(), oc.state_dict()
    assert [g["params"] for g in sa["param_groups"]] == [g["params"] for g in sc["param_groups"]]
    assert sc["param_groups"][0]["lr"] == 5e-4 and tuple(sc["param_groups"][0]["betas"]) == (0.9, 0.95)
    for k in sa["state"]:
        assert float(sc["state"][k]["step"]) == float(sa["state"][k]["step"]) == 3.0
        for f in ("exp_avg", "exp_avg_sq"):
            a, c = sa["state"][k][f], sc["state"][k][f]
            assert (a - c).abs().max().item() <= 1e-5 * max(a.abs().max().item(), 1e-12) + 1e-12, (k, f)


def test_training_is_bit_reproducible_at_the_bench_configuration():
    """Two Trainers from the same seed, 60 graph-replayed steps of the bench's configuration each: parameters and every
    loss bit-identical.  (Round 3: the head's weight-gradient kernel returned a slightly different slab about once in 200
    launches inside the step -- an MFMA read a freshly packed bf16 operand too early, `mfma_operand_fence` in csrc/common.h;
    every reduction in the step is ordered, so any run-to-run difference is a bug of that kind.)"""
    import argparse
    import bench
    from tulip_amd.trainer import Trainer
    a = argparse.Namespace(model="tulip_base", img=[16, 1024], target=[64, 1024], batch=8)
    res = []
    for _ in range(2):
        m = bench.make_model(a).to(DEV).train()
        tr = Trainer(m, 8)
        lo, hi = bench.synthetic(a, 0, torch.device(DEV))
        tr.load_batch(lo, hi)
        ls = torch.stack([tr.step().clone() for _ in range(60)])
        torch.cuda.synchronize()
        res.append((tr.eng.params.flat.clone(), ls.cpu()))
        del tr, m
    assert torch.equal(res[0][1], res[1][1]), "losses differ between two identical runs"
    assert torch.equal(res[0][0], res[1][0]), "parameters differ between two identical runs"


@pytest.mark.parametrize("model,img,target,batch", [("tulip_base", (16, 1024), (64, 1024), 8), ("tulip_large", (16, 2048), (64, 2048), 2)])
def test_optimizer_step_in_the_weight_gradient_write_out_is_the_same_step(model, img, target, batch):
    """Trainer.fuse_adamw: tensors whose weight-gradient workgroups hold the complete gradient tile (no token split: ~90 % of
    tulip_base's parameters at the bench configuration) take their AdamW step in that kernel's write-out instead of in the
    launch at the end of the step.  Same operations (adamw_step4, csrc/common.h), so parameters, moments, the bf16 shadow
    and every loss must equal the run with gradients accumulated, cleared and stepped at the end (grad_overwrite and
    fuse_adamw off) bit for bit -- which also proves that no fused tensor is read by the backward after it has been stepped,
    and that every gradient element has exactly one producer.  tulip_large: the backup window, C = 1536 and the stand-alone
    LayerNorm parameter pass (C > 2048), whose two ranges the overwrite mode has to clear itself."""
    import argparse
    import bench
    from tests import adamw_audit as AA
    from tulip_amd.trainer import Trainer
    a = argparse.Namespace(model=model, img=list(img), target=list(target), batch=batch)
    res = []
    for fuse in (True, False):
        m = bench.make_model(a).to(DEV).train()
        tr = Trainer(m, batch)
        assert tr.fuse_adamw and tr.grad_overwrite
        tr.fuse_adamw = tr.grad_overwrite = fuse
        lo, hi = bench.synthetic(a, 0, torch.device(DEV))
        tr.load_batch(lo, hi)
        snaps, ls = [AA.snapshot(tr)], []
        for _ in range(8):
            ls.append(tr.step().clone())
            snaps.append(AA.snapshot(tr))
        ls = torch.stack(ls)
        torch.cuda.synchronize()
        # every step AdamW by its definition (an error both plans share passes the comparison below): with fuse the gradient of
        # what the end-of-step launch steps stays in g; without, the launch clears it
        bad = AA.audit_run(snaps, AA.layout_of(tr), [AA.Hyper(lr=5e-4, t=t) for t in range(1, 9)], "nonzero" if fuse else "unknown")
        assert bad == [], (fuse, "\n".join(bad[:40]))
        W = tr.eng.params
        assert (tr.fused_adamw_params > 0.8 * sum(W.numel[n] for n in W.names)) == fuse
        res.append((W.flat.clone(), W.shadow.clone(), tr.m.clone(), tr.v.clone(), ls.cpu()))
        del tr, m
    for x, y, what in zip(res[0], res[1], ("parameters", "bf16 shadow", "exp_avg", "exp_avg_sq", "losses")):
        assert torch.equal(x, y), what

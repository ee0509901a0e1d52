"""Every AdamW update of real training steps audited against its definition (tests/adamw_audit.py): after each Trainer.step()
a snapshot with no host sync in between, the learning rate changed at every step (a hyper block that reaches the wrong step
shows), the hyperparameters, step index and decay group from the test's own bookkeeping.  The default plan steps most
tensors beside the backward (the weight-gradient write-outs, the fold launches on the side queue) and the rest at the end;
the other plans step at the end, per bucket on the optimizer stream or in the sharded exchange."""
import os
import subprocess
import sys
from functools import partial

import pytest
import torch
import torch.nn as nn

from tests import adamw_audit as AA
from tulip_amd.trainer import Trainer, cosine_lr

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lr_at(t):
    """the learning rate of optimizer step t: warm-up then cosine, a different value at every step."""
    return cosine_lr(t / 4.0, 5e-4, 1e-5, 1.0, 3.0) + 1e-6 * t


def make(model="tulip_base", img=(16, 1024), target=(64, 1024), in_chans=1, window=(2, 8), drop=0.0):
    """bench.py's KITTI model (reference init under seed 0) with the features that change the launch sequence."""
    from tulip_amd.model import tulip as T
    torch.manual_seed(0)
    depths, heads = ((2, 2, 2, 2), (3, 6, 12, 24)) if model == "tulip_base" else ((2, 2, 2, 2, 2), (3, 6, 12, 24, 48))
    return T.TULIP(img_size=tuple(img), target_img_size=tuple(target), patch_size=(1, 4), in_chans=in_chans, embed_dim=96,
                   window_size=list(window), depths=depths, num_heads=heads, mlp_ratio=4, qkv_bias=True, drop_rate=drop,
                   attn_drop_rate=drop, drop_path_rate=0.1, norm_layer=partial(nn.LayerNorm, eps=1e-6), pixel_shuffle=True,
                   circular_padding=True, log_transform=True, patch_unmerging=True).to(DEV).train()


def batch(m, B, seed=1234):
    g = torch.Generator().manual_seed(seed)
    C, (Hh, Wh), (Hl, _) = m.in_chans, m.target_img_size, m.img_size
    r = torch.rand(B, C, Hh, Wh, generator=g)
    r[torch.rand(B, C, Hh, Wh, generator=g) < 0.1] = 0
    hi = torch.log1p(r)
    return hi[:, :, 0::Hh // Hl, :].contiguous().to(DEV), hi.to(DEV)


def audited_steps(tr, n, grad_mode, t0=0):
    """n micro-steps, a snapshot behind each (no sync), then every step audited.  Returns (violations, report, last snapshot)."""
    lay = AA.layout_of(tr)
    snaps, hypers, t = [AA.snapshot(tr)], [], t0
    for i in range(n):
        update = (tr.micro + 1) % tr.accum_iter == 0
        lr = lr_at(t + 1)
        tr.step(lr=lr)
        snaps.append(AA.snapshot(tr))
        if update:
            t += 1
        hypers.append(AA.Hyper(lr=lr, t=t) if update else None)
    rep = AA.Report(lay, snaps[0]["p"].device)
    v = AA.audit_run(snaps, lay, hypers, grad_mode, report=rep)
    assert torch.isfinite(tr.P.losses).all()
    return v, rep, snaps[-1]


@pytest.mark.parametrize("packed_gemm", [True, False])
def test_bench_configuration_every_update_is_adamw(packed_gemm):
    """KITTI tulip_base 16x1024 -> 64x1024, batch 8, the default Trainer (captured, fused AdamW in the write-outs and the fold
    launches, the rest at the end).  packed_gemm: gemm_stream_kernel in the backward chain beside the side queue's folds."""
    m = make()
    tr = Trainer(m, 8)
    tr.eng.packed_gemm = packed_gemm
    assert tr.fuse_adamw and tr.grad_overwrite
    tr.load_batch(*batch(m, 8))
    v, rep, _ = audited_steps(tr, 8, "nonzero")
    assert tr.fused_adamw_params > 0 and tr.step_form == "one_graph"
    st = rep.stats
    print(f"packed_gemm={packed_gemm}: worst p error {st.get('p_ulps', 0):.3g} ulp, worst v residual {st.get('v_frac', 0):.3g} "
          f"of its bound, rsqrtf(bc2) a neighbour of the rounded value at some step: {bool(st.get('rsqrt_ulp_off', 0))}")
    assert v == [], "\n".join(v[:40])


def test_unfused_plan_gradient_known_everywhere():
    """fuse_adamw off, grad_overwrite on: the end-of-step launch steps everything and the gradient stays in g -- the moments
    must be the float32 emulation bit for bit on every element."""
    m = make()
    tr = Trainer(m, 8)
    tr.fuse_adamw = False
    tr.load_batch(*batch(m, 8))
    v, rep, last = audited_steps(tr, 6, "known")
    assert tr.fused_adamw_params == 0 and bool((last["g"] != 0).any())
    assert v == [], "\n".join(v[:40])


def test_accumulation_with_the_gradient_norm():
    """accum_iter = 2, track_grad_norm: the non-update micro-steps leave everything bit-unchanged."""
    m = make()
    tr = Trainer(m, 8, accum_iter=2, track_grad_norm=True)
    assert not tr.fuse_adamw and not tr.grad_overwrite
    tr.load_batch(*batch(m, 8))
    v, _, _ = audited_steps(tr, 8, "unknown")
    assert tr.t == 4
    assert v == [], "\n".join(v[:40])


def test_eager_step():
    m = make()
    tr = Trainer(m, 8, use_graph=False)
    tr.load_batch(*batch(m, 8))
    v, _, _ = audited_steps(tr, 6, "known")
    assert v == [], "\n".join(v[:40])


def test_tulip_large():
    """16x2048, batch 2: the backup window, C = 1536 and the stand-alone LayerNorm parameter pass."""
    m = make("tulip_large", (16, 2048), (64, 2048))
    tr = Trainer(m, 2)
    tr.load_batch(*batch(m, 2))
    v, _, _ = audited_steps(tr, 6, "nonzero")
    assert tr.fused_adamw_params > 0
    assert v == [], "\n".join(v[:40])


def test_batch_64():
    """the deep stages as the GEMM sequence, other pack sets."""
    m = make()
    tr = Trainer(m, 64)
    tr.load_batch(*batch(m, 64))
    v, _, _ = audited_steps(tr, 6, "nonzero")
    assert v == [], "\n".join(v[:40])


@pytest.mark.parametrize("feature", ["fp8", "dropout", "window48", "inchans2"])
def test_features_that_change_the_launch_sequence(feature):
    kw = {"dropout": dict(drop=0.1), "window48": dict(window=(4, 8)), "inchans2": dict(in_chans=2)}.get(feature, {})
    m = make(**kw)
    tr = Trainer(m, 8, attn_fp8=True if feature == "fp8" else None)
    assert tr.eng.attn_fp8 == (feature == "fp8")
    tr.load_batch(*batch(m, 8))
    v, _, _ = audited_steps(tr, 6, "nonzero")
    assert v == [], "\n".join(v[:40])


def test_resume_continues_the_bias_corrections():
    """3 steps, state_dict() -> a new model and Trainer -> load_state_dict() -> 2 more steps audited at t = 4 and 5."""
    m = make()
    tr = Trainer(m, 8)
    lo, hi = batch(m, 8)
    tr.load_batch(lo, hi)
    v, _, last = audited_steps(tr, 3, "nonzero")
    assert v == [], "\n".join(v[:40])
    sd_model, sd_opt = {k: t.clone() for k, t in m.state_dict().items()}, tr.state_dict()
    del tr
    m2 = make()
    m2.load_state_dict(sd_model)
    tr2 = Trainer(m2, 8)
    tr2.load_state_dict(sd_opt)
    tr2.load_batch(lo, hi)
    s0 = AA.snapshot(tr2)
    lay = AA.layout_of(tr2)
    assert AA.audit_unchanged(last, s0, lay) == []          # the resumed state is the saved one, bit for bit
    v, _, _ = audited_steps(tr2, 2, "nonzero", t0=3)
    assert tr2.t == 5
    assert v == [], "\n".join(v[:40])


def test_one_rank_rccl_plans(tmp_path):
    """segmented all-reduce, the one-graph step with captured collectives, bucket_adamw, grad_dtype bf16, exchange sharded:
    one rank on RCCL in a child process (tests/adamw_audit_ws1_worker.py)."""
    out = tmp_path / "audit_ws1.pt"
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29551")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "adamw_audit_ws1_worker.py"), str(out), "4"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = torch.load(out)
    assert got["backend"] == "nccl"
    want_form = {"segments": "segments", "captured": "one_graph_captured_collectives", "bucket_adamw": "segments",
                 "bf16": "segments", "sharded": "segments"}
    for name, form in want_form.items():
        g = got[name]
        assert g["form"] == form and g["segmented"] and g["buckets"] >= 2, (name, g["form"], g["buckets"])
        assert g["violations"] == [], (name, "\n".join(g["violations"][:40]))
    assert got["bucket_adamw"]["bucket_adamw"] and got["sharded"]["bucket_adamw"] and got["bf16"]["gb"]

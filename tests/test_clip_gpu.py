"""Gradient clipping by global norm on the GPU: tulip_grad_clip against the host definition bit for bit (tulip_amd/clip.py), its
refusals, an inactive clip against the unclipped step, an active clip in every step form against the definition (tests/clip_check.py),
and Trainer(clip_grad=...) against the reference model's loop with torch.nn.utils.clip_grad_norm_ (tests/golden/g18_clip.npz).
Everything on the tiny model (8x256 -> 32x256, depths (2, 2), embed_dim 48) at batch 4."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import tulip_oracle as O
from tests.clip_check import clipped_steps, differing, f32_bits, lr_at, state_bits
from tests.ema_check import tracked_steps
from tests.test_model_gpu import build
from tulip_amd import _lib, ops
from tulip_amd.clip import clip_coef_host, clipped_grad_scale_host
from tulip_amd.trainer import Trainer, layer_decay_scales

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP = 0.05           # the tiny model's gradient norms are 0.4 - 3: coef < 0.15 at every step


def tiny(seed=0, drop=None):
    """the tiny model (DropPath 0.1; drop: element dropout at that rate too) and one batch of 4; the engine's DropPath seed is the
    torch seed in force when the model is bound"""
    torch.manual_seed(seed)
    cfg = O.tiny_config()
    sd = O.key_seeded_state_dict(cfg, seed=3)
    if drop is None:
        m = build(cfg, sd, train=True)
    else:
        from tests.test_dropout_gpu import _tiny_model
        m = _tiny_model(cfg, sd, drop)
    lo, hi = (t.to(DEV) for t in O.synthetic_batch(cfg, 4, seed=77))
    return m, lo, hi


# ---------------------------------------------------------------------------------------------------- G1. the kernel
def gradient(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * 0.01).to(DEV)


def run_clip(g, n, base, max_norm):
    part = torch.zeros(1024, dtype=torch.float64, device=DEV)
    gs = torch.full((1,), base, dtype=torch.float32, device=DEV)
    out = torch.full((2,), -7.0, dtype=torch.float32, device=DEV)
    ops.grad_clip(g, n, part, gs, torch.full((1,), max_norm, dtype=torch.float32, device=DEV), out)
    ref = torch.zeros(1, device=DEV)
    ops.grad_norm(g, n, torch.zeros(1024, dtype=torch.float64, device=DEV), ref,
                  scale_dev=torch.full((1,), base, dtype=torch.float32, device=DEV))
    torch.cuda.synchronize()
    return np.float32(out[0].item()), np.float32(out[1].item()), np.float32(gs.item()), np.float32(ref.item())


# n = 4: one float4; 1028: one workgroup + one lane; 1 048 580 = 1024 * 256 * 4 + 4: one float4 past the partial kernel's cap of
# 1024 workgroups (the grid-stride loop's second trip); 1003: n % 4 != 0, the scalar tail
@pytest.mark.parametrize("n", [4, 1028, 1024 * 256 * 4 + 4, 1003])
@pytest.mark.parametrize("base", [1.0, 0.25])
def test_kernel_is_the_host_definition_bit_for_bit(n, base):
    g = gradient(n)
    keep = g.clone()
    total = float(g.double().norm().item()) * base
    for max_norm in (total * 4.0, total / 1.5, total / 1000.0):               # above, below and far below the norm
        norm, coef, gs, norm_ref = run_clip(g, n, base, max_norm)
        assert f32_bits(norm) == f32_bits(norm_ref) and abs(float(norm) - total) <= 1e-6 * total
        want, _ = clip_coef_host(norm, max_norm)
        assert f32_bits(coef) == f32_bits(want), (n, base, max_norm, float(coef), float(want))
        assert f32_bits(gs) == f32_bits(clipped_grad_scale_host(base, want))
        assert (coef == np.float32(1.0)) == (max_norm > total) and (coef < 1.0 or f32_bits(gs) == f32_bits(base))
        assert torch.equal(g, keep)                                           # g is only read
    # a NaN gradient: NaN norm, NaN coefficient, NaN scale; an infinite one: coefficient 0
    g2 = g.clone()
    g2[n // 2] = float("nan")
    norm, coef, gs, _ = run_clip(g2, n, base, 1.0)
    assert np.isnan(norm) and np.isnan(coef) and np.isnan(gs)
    g2[n // 2] = float("inf")
    norm, coef, gs, _ = run_clip(g2, n, base, 1.0)
    assert np.isinf(norm) and coef == np.float32(0.0) and gs == np.float32(0.0)
    # all zeros: coefficient 1, the scale keeps its bits
    norm, coef, gs, _ = run_clip(torch.zeros(n, device=DEV), n, base, 1.0)
    assert norm == np.float32(0.0) and f32_bits(coef) == f32_bits(1.0) and f32_bits(gs) == f32_bits(base)


# ---------------------------------------------------------------------------------------------------- G2. bad arguments
def test_kernel_refuses_bad_arguments_before_any_launch():
    n = 1028
    g = gradient(n)
    part = torch.full((1024,), -3.0, dtype=torch.float64, device=DEV)
    gs = torch.full((1,), 0.5, dtype=torch.float32, device=DEV)
    mx = torch.full((1,), 0.001, dtype=torch.float32, device=DEV)
    out = torch.full((2,), -7.0, dtype=torch.float32, device=DEV)
    fn, st = _lib.load().tulip_grad_clip, torch.cuda.current_stream().cuda_stream
    G, Pp, S, M, Oo = g.data_ptr(), part.data_ptr(), gs.data_ptr(), mx.data_ptr(), out.data_ptr()
    cases = {"n == 0": (G, 0, Pp, S, M, Oo), "n < 0": (G, -4, Pp, S, M, Oo), "partials NULL": (G, n, None, S, M, Oo),
             "grad_scale NULL": (G, n, Pp, None, M, Oo), "max_norm NULL": (G, n, Pp, S, None, Oo), "out NULL": (G, n, Pp, S, M, None),
             "g NULL": (None, n, Pp, S, M, Oo), "g misaligned": (G + 4, n - 4, Pp, S, M, Oo)}
    for name, a in cases.items():
        assert fn(*a, st) == -1, name                                         # TULIP_ERR_ARG
    torch.cuda.synchronize()
    assert gs.item() == 0.5 and out.tolist() == [-7.0, -7.0] and bool((part == -3.0).all())          # nothing was written
    with pytest.raises(_lib.TulipHipError):
        ops.grad_clip(g, 0, part, gs, mx, out)
    with pytest.raises(_lib.TulipHipError):
        ops.grad_clip(g.data_ptr() + 4, n - 4, part, gs, mx, out)


# ---------------------------------------------------------------------------------------------------- G3. inactive = unclipped
@pytest.mark.parametrize("form", ["captured", "eager", "accum2"])
def test_inactive_clip_is_the_unclipped_step(form):
    """clip_grad = 1e9 never clips: coef == 1.0f, hyper[7] keeps its bits, and master, shadow and both moments are those of the
    Trainer without clipping, bit for bit -- although that one steps most tensors beside the backward (a tensor gets the same
    bits whichever AdamW site steps it)."""
    kw = {"captured": {}, "eager": dict(use_graph=False), "accum2": dict(accum_iter=2)}[form]
    runs = {}
    for clip in (None, 1e9):
        m, lo, hi = tiny()
        tr = Trainer(m, 4, clip_grad=clip, **kw)
        assert (tr.clip_coef is None) == (clip is None) and tr.clip_grad == clip
        if clip is not None:
            assert not tr.fuse_adamw and not tr.bucket_adamw
        tr.load_batch(lo, hi)
        losses = [tr.step(lr=lr_at(i // tr.accum_iter + 1)).clone() for i in range(3 * tr.accum_iter)]
        torch.cuda.synchronize()
        assert tr.t == 3
        if clip is not None:
            assert f32_bits(tr.clip_coef.item()) == f32_bits(1.0) and tr.grad_norm.item() > 0.0
        runs[clip] = (state_bits(tr), torch.stack(losses))
    assert differing(runs[None][0], runs[1e9][0]) == []
    assert torch.equal(runs[None][1], runs[1e9][1])


def test_default_trainer_is_unchanged():
    """clip_grad=None: no buffer, no key, the fused plan as before."""
    m, lo, hi = tiny()
    tr = Trainer(m, 4)
    assert tr.clip_grad is None and tr.clip_coef is None and not hasattr(tr, "_clip_max") and tr.fuse_adamw
    tr.step(lo, hi)
    assert "clip_grad" not in tr.state_dict() and tr.fused_adamw_params > 0
    with pytest.raises(ValueError):
        tr.clip_grad = 1.0                       # the plan differs: another Trainer


# ---------------------------------------------------------------------------------------------------- G4. active = the definition
@pytest.mark.parametrize("form", ["captured", "eager", "accum2", "lr_scales", "dropout"])
def test_active_clip_is_the_host_definition(form):
    m, lo, hi = tiny(drop=0.1 if form == "dropout" else None)
    scales = layer_decay_scales(m, layers_per_group=8) if form == "lr_scales" else None
    kw = {"eager": dict(use_graph=False), "accum2": dict(accum_iter=2), "lr_scales": dict(lr_scales=scales)}.get(form, {})
    tr = Trainer(m, 4, clip_grad=CLIP, **kw)
    assert not tr.fuse_adamw and tr.grad_overwrite == (form != "accum2")
    tr.load_batch(lo, hi)
    bad, seen = clipped_steps(tr, 3 * tr.accum_iter, scales=scales)
    assert tr.t == 3 == len(seen) and all(c < 0.8 for _, c in seen), seen
    assert bad == [], "\n".join(bad[:40])
    if form == "lr_scales":
        assert tr._lr_table is not None and len(set(tr.lr_scales.values())) >= 3
    if form == "captured":
        # a new max_norm is one uploaded float: the captured graphs stay, the next step clips to it
        segs = tr._segments
        tr.clip_grad = 2 * CLIP
        bad, seen2 = clipped_steps(tr, 1, t0=3)
        assert bad == [] and tr._segments is segs, "\n".join(bad[:40])
        want, _ = clip_coef_host(np.float32(seen2[0][0]), 2 * CLIP)
        assert f32_bits(seen2[0][1]) == f32_bits(want)
        with pytest.raises(ValueError):
            tr.clip_grad = -1.0
        with pytest.raises(ValueError):
            tr.clip_grad = None


def test_average_follows_the_clipped_weights():
    """ema_decay with clip_grad: the average is the host definition applied to the stepped (clipped) weights after every step."""
    m, lo, hi = tiny()
    tr = Trainer(m, 4, clip_grad=CLIP, ema_decay=0.5)
    tr.load_batch(lo, hi)
    coefs = []
    step = lambda: (tr.step(), coefs.append(tr.clip_coef.clone()))[0]
    bad, updates, _ = tracked_steps(tr, 3, step=step)
    assert bad == [] and updates == 3 == tr.ema.num_updates, "\n".join(bad)
    assert all(c.item() < 0.8 for c in coefs), coefs


def test_resume_carries_clip_grad():
    m, lo, hi = tiny()
    tr = Trainer(m, 4, clip_grad=CLIP)
    tr.step(lo, hi)
    sd = tr.state_dict()
    assert sd["clip_grad"] == CLIP
    m2, _, _ = tiny()
    tr2 = Trainer(m2, 4, clip_grad=1.0)
    tr2.load_state_dict({k: v for k, v in sd.items() if k != "clip_grad"})        # an older dictionary: the constructor's value
    assert tr2.clip_grad == 1.0
    tr2.load_state_dict(sd)
    torch.cuda.synchronize()
    assert tr2.clip_grad == CLIP and tr2._clip_max.item() == np.float32(CLIP)


def test_one_rank_rccl_plans(tmp_path):
    """force_segments (graph segments + the "adamw" graph), the same with the bf16 exchange, and the one graph with captured
    collectives: one rank on RCCL in a fresh child process (tests/clip_ws1_worker.py), ended by `timeout` if it stalls."""
    out = tmp_path / "clip_ws1.pt"
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29559")
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tests", "clip_ws1_worker.py"), str(out), "3",
                        str(CLIP)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = torch.load(out)
    assert got["backend"] == "nccl"
    want_form = {"one_gpu": "one_graph", "segments": "segments", "bf16": "segments", "captured": "one_graph_captured_collectives"}
    for name, form in want_form.items():
        g = got[name]
        assert g["form"] == form and g["segmented"] == (name != "one_gpu"), (name, g["form"])
        assert name == "one_gpu" or g["buckets"] >= 2, (name, g["buckets"])
        assert not g["bucket_adamw"] and not g["fuse_adamw"], name
        assert g["failures"] == [], (name, "\n".join(g["failures"][:40]))
        assert g["t"] == 3 == len(g["seen"]) and all(c < 0.8 for _, c in g["seen"]), (name, g["seen"])
    assert got["bf16"]["gb"]
    # fp32 exchange on one rank: the same gradients, the same norm, the same step as on one GPU
    for name in ("segments", "captured"):
        assert got[name]["differs_from_one_gpu"] == [], (name, got[name]["differs_from_one_gpu"])
        assert got[name]["seen"] == got["one_gpu"]["seen"], name


# ---------------------------------------------------------------------------------------------------- G5. the reference's loop
@pytest.mark.parametrize("use_graph", [True, False])
def test_clipped_training_matches_the_reference_loop(golden_dir, use_graph):
    """Reference model + torch.optim.AdamW + clip_grad_norm_ between backward() and step() (misc.py:299-300), 4 steps, fp32 on the
    CPU (tests/golden/make_golden_clip.py) against Trainer(clip_grad=...): bf16 GEMMs vs fp32, so losses to 3e-3 and pre-clip norms
    to 2e-2 (test_train_one_epoch_matches_reference_loop's tolerances), ||exp_avg|| to 2e-2 (linear in the gradients) and
    ||exp_avg_sq|| to 4e-2 (quadratic).  The unclipped run's moment norms lie far outside: clipping silently off cannot pass."""
    z = np.load(os.path.join(golden_dir, "g18_clip.npz"))
    clip, steps, B = float(z["clip_grad"]), int(z["steps"]), int(z["batch"])
    for key, rtol in (("m_norm", 2e-2), ("v_norm", 4e-2)):
        assert np.all(np.abs(z[key + "_unclipped"] - z[key]) > 5.0 * rtol * np.abs(z[key])), key
    cfg = O.tiny_config(drop_path_rate=0.0)
    m = build(cfg, O.key_seeded_state_dict(cfg, seed=int(z["seed"])), train=True)
    tr = Trainer(m, B, lr=float(z["lr"]), betas=tuple(z["betas"].tolist()), weight_decay=float(z["weight_decay"]),
                 use_graph=use_graph, clip_grad=clip)
    losses, norms, coefs, mn, vn = [], [], [], [], []
    for i in range(steps):
        lo, hi = O.synthetic_batch(cfg, B, seed=int(z["data_seed0"]) + i)
        losses.append(tr.step(lo.to(DEV), hi.to(DEV))[0].item())
        norms.append(tr.grad_norm.item())
        coefs.append(tr.clip_coef.item())
        mn.append(tr.m.double().norm().item())
        vn.append(tr.v.double().norm().item())
    print(f"use_graph={use_graph}: loss {losses} vs {z['loss'].tolist()}\n  norm {norms} vs {z['grad_norm'].tolist()}\n"
          f"  ||m|| {mn} vs {z['m_norm'].tolist()}\n  ||v|| {vn} vs {z['v_norm'].tolist()}\n  coef {coefs}")
    assert all(c < 0.8 for c in coefs), coefs
    np.testing.assert_allclose(losses, z["loss"], rtol=3e-3)
    np.testing.assert_allclose(norms, z["grad_norm"], rtol=2e-2)
    np.testing.assert_allclose(mn, z["m_norm"], rtol=2e-2)
    np.testing.assert_allclose(vn, z["v_norm"], rtol=4e-2)
    for got, key, rtol in ((mn, "m_norm", 2e-2), (vn, "v_norm", 4e-2)):
        assert np.all(np.abs(np.array(got) - z[key + "_unclipped"]) > rtol * np.abs(z[key + "_unclipped"])), key

"""Weight EMA on the GPU: tulip_ema_update against the host definition bit for bit (tulip_amd/ema.py), a captured
ParamEMA.update() replayed, the Trainer's average in every step form against snapshots of the parameters, evaluation with
the averaged weights, resume, and the average switched off."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import tulip_oracle as O
from tests.ema_check import bits, describe, to_np, tracked_steps
from tests.test_adamw_audit_gpu import batch, make
from tests.test_ema_cpu import value_set
from tests.test_model_gpu import build
from tulip_amd import _lib, ops
from tulip_amd.ema import ParamEMA, ema_update_host
from tulip_amd.trainer import Trainer

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tiled(n):
    s, p = value_set()
    reps = -(-n // s.size)
    return np.tile(s, reps)[:n].copy(), np.tile(p, reps)[:n].copy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def tiny(seed=0):
    """the tiny model (8x256 -> 32x256, depths (2, 2), embed_dim 48; DropPath 0.1), batch 4; the engine's DropPath seed is the
    torch seed in force when the model is bound"""
    torch.manual_seed(seed)
    cfg = O.tiny_config()
    m = build(cfg, O.key_seeded_state_dict(cfg, seed=3), train=True)
    lo, hi = (t.to(DEV) for t in O.synthetic_batch(cfg, 4, seed=77))
    return cfg, m, lo, hi


# ---------------------------------------------------------------------------------------------------- 1. the kernel
# n = 4: one float4; 1028: one full workgroup + one lane; 2 097 156 = 2048 * 256 * 4 + 4: one float4 past grid_for's cap of 2048
# workgroups, the grid-stride loop's second trip
@pytest.mark.parametrize("n", [4, 1028, 2048 * 256 * 4 + 4])
@pytest.mark.parametrize("warmup", [True, False])
def test_kernel_is_the_host_definition_bit_for_bit(n, warmup):
    s0, p0 = tiled(n)
    decay = 0.5 if warmup else 0.999           # (1 + k) / (10 + k) crosses 0.5 at update 8 of the 12
    ps = [dev(p0), dev(np.roll(p0, 1) * np.float32(1.5))]        # the parameters move between updates
    s = dev(s0)
    counter = torch.zeros(1, dtype=torch.int64, device=DEV) if warmup else None
    omd = torch.zeros(1, dtype=torch.float32, device=DEV)
    for k in range(12):
        ops.ema_update(ps[k % 2], s, n, decay, counter, omd)
    torch.cuda.synchronize()
    host, cnt = s0, (0 if warmup else None)
    for k in range(12):
        host, cnt = ema_update_host(host, to_np(ps[k % 2]), decay, cnt)
    got = to_np(s)
    diff = np.flatnonzero(bits(got) != bits(host))
    assert diff.size == 0, (diff.size, int(diff[0]), got[diff[0]], host[diff[0]])
    if warmup:
        assert int(counter.item()) == 12 == cnt
        assert omd.item() == np.float32(0.5)
    else:
        assert omd.item() == np.float32(1.0 - 0.999)
    assert np.array_equal(to_np(ps[0]), p0)                      # the parameters are only read


def test_kernel_refuses_bad_arguments_before_any_launch():
    n = 1028
    s0, p0 = tiled(n)
    s, p = dev(s0), dev(p0)
    counter = torch.full((1,), 3, dtype=torch.int64, device=DEV)
    omd = torch.full((1,), -7.0, dtype=torch.float32, device=DEV)
    fn, st = _lib.load().tulip_ema_update, torch.cuda.current_stream().cuda_stream
    P, S, C, M = p.data_ptr(), s.data_ptr(), counter.data_ptr(), omd.data_ptr()
    cases = {"n % 4": (P, S, 1026, 0.5, C, M), "p NULL": (None, S, n, 0.5, C, M), "shadow NULL": (P, None, n, 0.5, C, M),
             "omd NULL": (P, S, n, 0.5, C, None), "decay < 0": (P, S, n, -1e-9, C, M), "decay > 1": (P, S, n, 1.0000001, C, M),
             "decay NaN": (P, S, n, float("nan"), C, M), "misaligned": (P + 4, S, n - 4, 0.5, C, M)}
    for name, a in cases.items():
        assert fn(*a, st) == -1, name                                  # TULIP_ERR_ARG
    assert fn(P, S, 0, 0.5, C, M, st) == 0 and fn(P, S, -4, 0.5, C, M, st) == 0        # n <= 0: TULIP_OK, nothing to do
    torch.cuda.synchronize()
    assert np.array_equal(bits(to_np(s)), bits(s0)) and int(counter.item()) == 3 and omd.item() == -7.0
    with pytest.raises(_lib.TulipHipError):
        ops.ema_update(p, s, 1026, 0.5, counter, omd)


# ---------------------------------------------------------------------------------------------------- 2. graph replay
def test_captured_update_replays_with_the_counter_on_the_device():
    _, m, _, _ = tiny()
    ema = ParamEMA(m, 0.5)
    W = m.engine().params
    assert ema.shadow.numel() == W.total and ema.num_updates == 0
    host, cnt = to_np(ema.shadow), 0
    assert np.array_equal(bits(host), bits(to_np(W.flat)))             # starts as a copy of the parameters
    pad = np.ones(W.total, dtype=bool)
    for n in W.names:
        pad[W.offset[n]:W.offset[n] + W.numel[n]] = False
    scratch_s, scratch_p = torch.zeros(64, device=DEV), torch.ones(64, device=DEV)
    ops.ema_update(scratch_p, scratch_s, 64, 0.5, None, torch.zeros(1, device=DEV))      # load the kernels outside capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        g.capture_begin(capture_error_mode="thread_local")
        ema.update()
        g.capture_end()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert ema.num_updates == 0                                        # capturing launches nothing
    gen = torch.Generator().manual_seed(5)
    keep = (~torch.from_numpy(pad)).to(DEV)
    for k in range(5):
        fresh = (torch.randn(W.total, generator=gen) * 10.0 ** float(k - 3)).to(DEV)
        W.flat.copy_(torch.where(keep, fresh, torch.zeros_like(fresh)))            # fresh values, the padding stays 0
        g.replay()
        torch.cuda.synchronize()
        host, cnt = ema_update_host(host, to_np(W.flat), 0.5, cnt)
    got = to_np(ema.shadow)
    assert np.array_equal(bits(got), bits(host)), describe(W, got, host)
    assert ema.num_updates == 5 == cnt
    assert np.all(bits(got[pad]) == 0)                                 # padding exactly +0.0


# ---------------------------------------------------------------------------------------------------- 3. the Trainer, tiny model
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("accum_iter,calls", [(1, 4), (2, 6)])
def test_trainer_average_follows_every_optimizer_step(use_graph, accum_iter, calls):
    _, m, lo, hi = tiny()
    tr = Trainer(m, 4, use_graph=use_graph, accum_iter=accum_iter, ema_decay=0.9)
    assert isinstance(tr.ema, ParamEMA) and tr.ema.num_updates == 0
    tr.load_batch(lo, hi)
    bad, updates, _ = tracked_steps(tr, calls)
    assert bad == [], "\n".join(bad)
    assert updates == calls // accum_iter == tr.t == tr.ema.num_updates
    # a re-capture neither resets nor double-applies an update
    if use_graph:
        tr._segments = None
        bad, more, _ = tracked_steps(tr, accum_iter)
        assert bad == [] and more == 1 and tr.ema.num_updates == updates + 1, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------- 4. behind the fused sites
def test_average_is_taken_behind_the_fused_optimizer_sites():
    """tulip_base 16x1024 -> 64x1024, batch 8, captured: the write-out and fold AdamW sites on the side queue, pack_at_end and the
    end-of-step launch over the left-over blocks all run; an average taken before a late optimizer write is a mismatch."""
    m = make()
    tr = Trainer(m, 8, ema_decay=0.999)
    tr.load_batch(*batch(m, 8))
    bad, updates, _ = tracked_steps(tr, 4)
    assert tr.fused_adamw_params > 0 and tr.step_form == "one_graph" and tr._pack_at_end
    assert bad == [], "\n".join(bad)
    assert updates == 4 == tr.ema.num_updates
    sites = set(tr.adamw_sites().values())
    assert {"writeout", "fold"} <= sites and sites & {"blocks", "scan"}, sites


# ---------------------------------------------------------------------------------------------------- 5. evaluation, continuation
def test_evaluating_with_the_average_and_going_on_training():
    cfg, m, lo, hi = tiny()
    tr = Trainer(m, 4, ema_decay=0.9)
    _, m_twin, _, _ = tiny()
    twin = Trainer(m_twin, 4, ema_decay=0.9)
    for t in (tr, twin):
        for _ in range(3):
            t.step(lo, hi)
    ema, W = tr.ema, tr.eng.params

    def predict(model):
        model.eval()
        with torch.no_grad():
            out = model(lo, hi)[0].clone()
        model.train(True)
        return out

    before = predict(m)
    own = {k: v.clone() for k, v in m.state_dict().items()}
    shadow = ema.state_dict()["shadow_params"]
    assert set(shadow) == set(W.names) and any(not torch.equal(shadow[n], own[n]) for n in W.names)
    with ema.average_parameters():
        inside = predict(m)
        held = {k: v.clone() for k, v in m.state_dict().items()}
        with pytest.raises(RuntimeError):
            with ema.average_parameters():
                pass
        again = predict(m)                                   # the refused entry changed nothing
    after = predict(m)
    fresh = build(cfg, O.key_seeded_state_dict(cfg, seed=3))
    res = fresh.load_state_dict(shadow, strict=False)
    assert not res.unexpected_keys and not any(k in shadow for k in res.missing_keys)      # (buffers only)
    want = predict(fresh)
    assert torch.equal(inside, want) and torch.equal(again, want)
    assert not torch.equal(inside, before)
    for n in W.names:
        assert torch.equal(held[n], shadow[n]), n
        assert torch.equal(m.state_dict()[n], own[n]), n
    assert torch.equal(after, before)
    l4, l4_twin = tr.step(lo, hi).clone(), twin.step(lo, hi).clone()
    torch.cuda.synchronize()
    assert torch.equal(l4, l4_twin), (l4.tolist(), l4_twin.tolist())
    assert torch.equal(W.flat, twin.eng.params.flat) and torch.equal(ema.shadow, twin.ema.shadow)
    assert ema.num_updates == 4 == twin.ema.num_updates
    # the halves by their torch_ema names
    with pytest.raises(RuntimeError):
        ema.restore()
    ema.store(); ema.copy_to()
    assert torch.equal(W.flat, ema.shadow) and W.shadow_dirty
    ema.restore()
    assert torch.equal(W.flat, twin.eng.params.flat)


def test_average_refuses_a_reflattened_model():
    _, m, _, _ = tiny()
    ema = ParamEMA(m, 0.9)
    m.to(DEV)                       # TULIP._apply invalidates the engine
    m.engine().bind(torch.device("cuda", torch.cuda.current_device()))
    with pytest.raises(RuntimeError, match="new ParamEMA"):
        ema.update()
    W = ParamEMA(m, 0.9)._W
    W.master_partial = True
    try:
        with pytest.raises(RuntimeError, match="partial"):
            ParamEMA(m, 0.9)
    finally:
        W.master_partial = False
    with pytest.raises(ValueError):
        ParamEMA(m, 1.5)


# ---------------------------------------------------------------------------------------------------- 6. resume
def test_resume_continues_the_average():
    cfg, m, lo, hi = tiny()
    whole = Trainer(m, 4, ema_decay=0.9)
    for _ in range(4):
        whole.step(lo, hi)
    _, m1, _, _ = tiny()
    first = Trainer(m1, 4, ema_decay=0.9)
    for _ in range(2):
        first.step(lo, hi)
    torch.cuda.synchronize()
    sd_model, sd_opt = {k: v.clone() for k, v in m1.state_dict().items()}, first.state_dict()
    assert sd_opt["ema"]["num_updates"] == 2 and sd_opt["ema"]["decay"] == 0.9
    assert set(sd_opt["ema"]["shadow_params"]) == set(first.eng.params.names)
    del first
    _, m2, _, _ = tiny()
    m2.load_state_dict(sd_model)
    second = Trainer(m2, 4, ema_decay=0.9)
    second.load_state_dict(sd_opt)
    assert second.ema.num_updates == 2
    for _ in range(2):
        second.step(lo, hi)
    torch.cuda.synchronize()
    assert torch.equal(second.eng.params.flat, whole.eng.params.flat)
    got, want = to_np(second.ema.shadow), to_np(whole.ema.shadow)
    assert np.array_equal(bits(got), bits(want)), describe(second.eng.params, got, want)
    assert second.ema.num_updates == 4 == whole.ema.num_updates
    # a dictionary without the entry, EMA on: KeyError; a few names missing: KeyError with the count and the first three
    bare = {k: v for k, v in sd_opt.items() if k != "ema"}
    with pytest.raises(KeyError, match="ema"):
        second.load_state_dict(bare)
    names = second.eng.params.names
    cut = dict(sd_opt["ema"], shadow_params={n: t for n, t in sd_opt["ema"]["shadow_params"].items() if n not in names[:5]})
    with pytest.raises(KeyError, match="lacks 5 parameters") as e:
        second.ema.load_state_dict(cut)
    assert all(n in str(e.value) for n in names[:3]) and names[3] not in str(e.value)
    # EMA off: no key, and a dictionary that has one is read with one line on stderr
    _, m3, _, _ = tiny()
    off = Trainer(m3, 4)
    assert off.ema is None and "ema" not in off.state_dict()


def test_entry_without_an_average_is_ignored_with_one_line(capsys):
    _, m, lo, hi = tiny()
    on = Trainer(m, 4, ema_decay=0.9)
    on.step(lo, hi)
    sd = on.state_dict()
    _, m2, _, _ = tiny()
    off = Trainer(m2, 4)
    capsys.readouterr()
    off.load_state_dict(sd)
    err = capsys.readouterr().err
    assert len([l for l in err.splitlines() if "'ema'" in l]) == 1 and off.ema is None


# ---------------------------------------------------------------------------------------------------- 7. off is off
def test_the_average_observes_and_never_perturbs():
    runs = {}
    for name, kw in (("off", {}), ("on", dict(ema_decay=0.9))):
        _, m, lo, hi = tiny()
        tr = Trainer(m, 4, **kw)
        assert (tr.ema is None) == (name == "off")
        losses = [tr.step(lo, hi).clone() for _ in range(3)]
        torch.cuda.synchronize()
        runs[name] = (torch.stack(losses), tr.eng.params.flat.clone(), tr.m.clone(), tr.v.clone())
        if name == "on":
            assert tr.ema.num_updates == 3
    for a, b in zip(runs["off"], runs["on"]):
        assert torch.equal(a, b)
    _, m, _, _ = tiny()
    with pytest.raises(ValueError, match="sharded"):
        Trainer(m, 4, exchange="sharded", ema_decay=0.9)
    with pytest.raises(ValueError):
        Trainer(m, 4, ema_decay=-0.1)


def test_train_one_epoch_calls_a_foreign_average_after_every_step():
    """the reference's placement for an object the caller owns: update() behind every trainer.step() call, micro-steps included"""
    from types import SimpleNamespace
    from tulip_amd.trainer import train_one_epoch
    _, m, lo, hi = tiny()
    tr = Trainer(m, 4, accum_iter=2)
    ema = ParamEMA(m, 0.9)
    calls = []
    update = ema.update
    ema.update = lambda: (calls.append(tr.micro), update())[1]
    args = SimpleNamespace(lr=5e-4, min_lr=1e-5, warmup_epochs=1.0, epochs=3.0)
    train_one_epoch(tr, [(lo.cpu(), hi.cpu())] * 4, 1, args, ema=ema)
    assert calls == [1, 2, 3, 4] and ema.num_updates == 4 and tr.t == 2


# ---------------------------------------------------------------------------------------------------- 8. one-rank RCCL forms
def test_one_rank_rccl_plans(tmp_path):
    """segments, bucket_adamw and the one graph with captured collectives: one rank on RCCL in a fresh child process
    (tests/ema_ws1_worker.py), ended by `timeout` if it stalls."""
    out = tmp_path / "ema_ws1.pt"
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29557")
    r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.join(ROOT, "tests", "ema_ws1_worker.py"), str(out), "3"],
                       env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = torch.load(out)
    assert got["backend"] == "nccl"
    want_form = {"segments": "segments", "bucket_adamw": "segments", "captured": "one_graph_captured_collectives"}
    for name, form in want_form.items():
        g = got[name]
        assert g["form"] == form and g["segmented"] and g["buckets"] >= 2, (name, g["form"], g["buckets"])
        assert g["bucket_adamw"] == (name == "bucket_adamw"), name
        assert g["failures"] == [], (name, "\n".join(g["failures"]))
        assert g["updates"] == 3 == g["num_updates"], name

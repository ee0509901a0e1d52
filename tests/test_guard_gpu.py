"""The non-finite step guard on the GPU: tulip_step_guard against the host definition (tulip_amd/guard.py), the gated AdamW and EMA
entry points against the ungated ones, and Trainer(skip_nonfinite=True) in every step form (tests/guard_check.py) -- a guarded run
without a bad step is the unguarded run, a skipped step changes nothing, a run that skipped steps ends where the run without them
ends, checkpoints carry the applied count, and train_one_epoch goes on past a skipped step.  Every comparison is bit for bit.
Everything on the tiny model (8x256 -> 32x256, depths (2, 2), embed_dim 48) at batch 4."""
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import adamw_audit as AA
from tests.clip_check import differing, f32_bits, lr_at, state_bits
from tests.guard_check import (DEV, INF, NAN, guard_bits, optimizer_step, recovery_failures, skipped_step_failures, tiny)
from tulip_amd import _lib, ops
from tulip_amd.guard import guard_step_host
from tulip_amd.trainer import Trainer, layer_decay_scales, train_one_epoch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# one float4 per lane of one wave; several workgroups with a ragged last one; one 64-float block past the grid-stride cap of the
# scan (256 * 8 workgroups of 256 float4 lanes): the loop's second trip
SIZES = [64, 64 * 17, 2048 * 256 * 4 + 64]
CLIP = 0.05


def flag_of(value):
    return torch.full((1,), int(value), dtype=torch.int32, device=DEV).view(torch.uint32)


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(AA._bits(a), AA._bits(b))


# ---------------------------------------------------------------------------------------------------- K1. the decision kernel
@pytest.mark.parametrize("start", [(0, 0, 0), (41, 5, 3), (15000, (1 << 40) + 1, 0)])
def test_step_guard_is_the_host_definition_bit_for_bit(start):
    betas = (0.9, 0.95)
    norms = [1.5, NAN, INF, 0.0, 3.0e38, -INF, 2.0, 1e-45, np.uint32(0xFFC00001).view(np.float32), 7.0]
    state = torch.tensor(start, dtype=torch.int64, device=DEV)
    flag = flag_of(7)
    hyper = torch.tensor([5e-4, 0.9, 0.95, 1e-8, 0.01, -5.0, -6.0, 0.25], dtype=torch.float32, device=DEV)
    norm = torch.zeros(1, dtype=torch.float32, device=DEV)
    want, skips = tuple(start), 0
    for x in norms:
        norm.fill_(float(x))
        h0 = hyper.clone()
        ops.step_guard(norm, state, flag, hyper, *betas)
        torch.cuda.synchronize()
        want, skip, bc1, bc2 = guard_step_host(want, np.float32(x), betas)
        assert tuple(state.tolist()) == want and int(flag.item()) == int(skip), (float(x), state.tolist(), want)
        if skip:
            skips += 1
            assert same_bits(hyper, h0), (float(x), hyper.tolist())                      # all of hyper is untouched
        else:
            got = hyper.tolist()
            assert f32_bits(got[5]) == f32_bits(bc1) and f32_bits(got[6]) == f32_bits(bc2), (float(x), got[5:7], bc1, bc2)
            keep = [0, 1, 2, 3, 4, 7]
            assert same_bits(hyper[keep], h0[keep])
            if want[0] < 15000:                                                       # ... and the host's own upload, where it is not yet 1.0f
                assert f32_bits(got[5]) == f32_bits(np.float32(1.0 - betas[0] ** want[0]))
    assert skips == 4 and want[0] == start[0] + 6


def test_step_guard_refuses_bad_arguments_before_any_launch():
    state = torch.tensor([3, 2, 1], dtype=torch.int64, device=DEV)
    flag = flag_of(7)
    hyper = torch.full((8,), -2.0, dtype=torch.float32, device=DEV)
    norm = torch.full((1,), NAN, dtype=torch.float32, device=DEV)
    fn, st = _lib.load().tulip_step_guard, torch.cuda.current_stream().cuda_stream
    N, S, F, H = norm.data_ptr(), state.data_ptr(), flag.data_ptr(), hyper.data_ptr()
    cases = {"norm NULL": (None, S, F, H), "state NULL": (N, None, F, H), "flag NULL": (N, S, None, H), "hyper NULL": (N, S, F, None),
             "state misaligned": (N, S + 4, F, H)}
    for name, a in cases.items():
        assert fn(*a, 0.9, 0.95, st) == -1, name                                      # TULIP_ERR_ARG
    torch.cuda.synchronize()
    assert state.tolist() == [3, 2, 1] and int(flag.item()) == 7 and bool((hyper == -2.0).all())      # nothing was written
    with pytest.raises(_lib.TulipHipError):
        ops.step_guard(norm, None, flag, hyper, 0.9, 0.95)


# ---------------------------------------------------------------------------------------------------- K2. the gated AdamW
def adamw_inputs(n, seed=0):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    p = torch.randn(n, generator=gen, device=DEV)
    g = torch.randn(n, generator=gen, device=DEV) * 0.01
    m = torch.randn(n, generator=gen, device=DEV) * 0.01
    v = torch.rand(n, generator=gen, device=DEV) * 1e-4
    pb = p.to(torch.bfloat16)
    nb = n // 64
    # bit 0: decay on every other block; bits 2-7: three learning-rate groups; every fifth block stepped elsewhere (bit 1)
    idx = torch.arange(nb)
    mask = ((idx % 2) | ((idx % 3) << 2) | ((idx % 5 == 4).to(torch.int64) << 1)).to(torch.uint8).to(DEV)
    table = torch.ones(64, dtype=torch.float32)
    table[1], table[2] = 0.5, 0.31
    hyper = torch.tensor([5e-4, 0.9, 0.95, 1e-8, 0.01, 1.0 - 0.9 ** 3, 1.0 - 0.95 ** 3, 0.25], dtype=torch.float32, device=DEV)
    return dict(p=p, g=g, m=m, v=v, pb=pb), mask, table.to(DEV), hyper


def run_adamw(buf, n, hyper, mask, table, zero_grad, skip, blocks=None):
    b = {k: t.clone() for k, t in buf.items()}
    if blocks is None:
        ops.adamw(b["p"], b["g"], b["m"], b["v"], b["pb"], n, hyper, mask, zero_grad=zero_grad, lr_scale64=table, skip=skip)
    else:
        ops.adamw_blocks(b["p"], b["g"], b["m"], b["v"], b["pb"], blocks, blocks.numel(), hyper, mask, zero_grad=zero_grad,
                         lr_scale64=table, skip=skip)
    torch.cuda.synchronize()
    return b


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("scaled", [False, True])
def test_gated_adamw(n, scaled):
    """flag 0 and skip = NULL: the bits of the _s entry.  flag 1: p, m, v and the bf16 copy unchanged also where g holds NaN; g all
    zero where a taken step clears it (zero_grad; not in the blocks whose step is taken elsewhere), unchanged without."""
    for form in ("scan", "blocks"):
        buf, mask, table, hyper = adamw_inputs(n)
        mask_arg, table_arg = (mask, table) if scaled else (None, None)
        blocks = None
        if form == "blocks":                       # an explicit list: every third block, in descending order
            blocks = torch.arange(n // 64 - 1, -1, -3, dtype=torch.int32).to(DEV).contiguous()
        touched = torch.zeros(n, dtype=torch.bool, device=DEV)
        if blocks is None:
            touched[:] = True
            if scaled:
                touched = ((mask & 2) == 0).repeat_interleave(64)
        else:
            touched.view(-1, 64)[blocks.long()] = True
        for zero_grad in (False, True):
            want = run_adamw(buf, n, hyper, mask_arg, table_arg, zero_grad, None, blocks)
            assert not same_bits(want["p"], buf["p"]) and not same_bits(want["pb"], buf["pb"])
            got = run_adamw(buf, n, hyper, mask_arg, table_arg, zero_grad, flag_of(0), blocks)
            for k in buf:
                assert same_bits(got[k], want[k]), (form, zero_grad, k)
            # skip = NULL through the _g symbol itself
            b = {k: t.clone() for k, t in buf.items()}
            lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
            ptr = lambda t: None if t is None else t.data_ptr()
            if blocks is None:
                rc = lib.tulip_adamw_g(ptr(b["p"]), ptr(b["g"]), ptr(b["m"]), ptr(b["v"]), ptr(b["pb"]), n, ptr(hyper), ptr(mask_arg),
                                       ptr(table_arg), int(zero_grad), None, st)
            else:
                rc = lib.tulip_adamw_blocks_g(ptr(b["p"]), ptr(b["g"]), ptr(b["m"]), ptr(b["v"]), ptr(b["pb"]), ptr(blocks),
                                              blocks.numel(), ptr(hyper), ptr(mask_arg), ptr(table_arg), int(zero_grad), None, st)
            torch.cuda.synchronize()
            assert rc == 0
            for k in buf:
                assert same_bits(b[k], want[k]), (form, zero_grad, k, "skip NULL")
            for bad_g in (None, NAN, INF):
                bufx = dict(buf, g=buf["g"].clone())
                if bad_g is not None:              # in the first and in the last block (the scan and either list reach one of them)
                    bufx["g"][1] = bufx["g"][n - 2] = bad_g
                got = run_adamw(bufx, n, hyper, mask_arg, table_arg, zero_grad, flag_of(1), blocks)
                for k in ("p", "m", "v", "pb"):
                    assert same_bits(got[k], bufx[k]), (form, zero_grad, bad_g, k)
                if zero_grad:
                    assert not bool(AA._bits(got["g"])[touched].any()), (form, bad_g)
                    assert same_bits(got["g"][~touched], bufx["g"][~touched]), (form, bad_g)
                else:
                    assert same_bits(got["g"], bufx["g"]), (form, bad_g)


# ---------------------------------------------------------------------------------------------------- K3. the gated EMA update
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("warmup", [True, False])
def test_gated_ema_update(n, warmup):
    gen = torch.Generator(device=DEV).manual_seed(1)
    p = torch.randn(n, generator=gen, device=DEV)
    s = torch.randn(n, generator=gen, device=DEV)
    p[3], s[3] = 0.0, -0.0                          # omd = 0 would make this +0: the skipped launch must not touch it
    p[n - 1], s[n - 1] = 0.0, -0.0
    counter = lambda: torch.full((1,), 4, dtype=torch.int64, device=DEV) if warmup else None

    def run(skip):
        sh, c, omd = s.clone(), counter(), torch.full((1,), -3.0, dtype=torch.float32, device=DEV)
        ops.ema_update(p, sh, n, 0.9, c, omd, skip=skip)
        torch.cuda.synchronize()
        return sh, (None if c is None else int(c.item())), omd.item()

    want = run(None)
    assert not same_bits(want[0], s) and want[1] == (5 if warmup else None)
    got = run(flag_of(0))
    assert same_bits(got[0], want[0]) and got[1:] == want[1:]
    got = run(flag_of(1))
    assert same_bits(got[0], s) and got[1] == (4 if warmup else None) and got[2] == -3.0
    assert AA._bits(got[0])[3].item() == -2 ** 31 and AA._bits(got[0])[n - 1].item() == -2 ** 31


# ---------------------------------------------------------------------------------------------------- T1. no skip = no change
@pytest.mark.parametrize("form", ["captured", "eager", "accum2"])
@pytest.mark.parametrize("clip", [None, CLIP])
def test_no_skip_means_no_change(form, clip):
    """Six optimizer steps: the guarded Trainer's master, bf16 copy, moments and average are those of the norm-first Trainer without
    the guard -- the device's bias corrections are the host's uploads, the gated launches the ungated ones."""
    kw = {"captured": {}, "eager": dict(use_graph=False), "accum2": dict(accum_iter=2)}[form]
    runs = {}
    for guard in (False, True):
        m, lo, hi, _ = tiny()
        tr = Trainer(m, 4, track_grad_norm=True, clip_grad=clip, ema_decay=0.9, skip_nonfinite=guard, **kw)
        assert tr.skip_nonfinite is guard and not tr.fuse_adamw and not tr.bucket_adamw
        tr.load_batch(lo, hi)
        losses, norms = [], []
        for t in range(6):
            optimizer_step(tr, lr_at(t + 1))
            losses.append(tr.P.losses.clone())
            norms.append(tr.grad_norm.clone())
        torch.cuda.synchronize()
        if guard:
            assert (tr.skipped_steps, tr.applied_steps, tr.consecutive_skips, int(tr.last_step_skipped.item())) == (0, 6, 0, 0)
            assert set(tr.adamw_sites().values()) == {"scan"}
        else:
            with pytest.raises(AttributeError):
                tr.skipped_steps
        runs[guard] = (guard_bits(tr), torch.stack(losses), torch.stack(norms))
    assert differing(runs[False][0], runs[True][0]) == []
    assert torch.equal(runs[False][1], runs[True][1]) and torch.equal(runs[False][2], runs[True][2])


def test_guard_alone_computes_the_norm_and_default_is_unchanged():
    m, lo, hi, _ = tiny()
    tr = Trainer(m, 4, skip_nonfinite=True)
    assert not tr.track_grad_norm and tr.clip_grad is None and not tr.fuse_adamw
    tr.step(lo, hi)
    assert tr.grad_norm.item() > 0.0 and tr.applied_steps == 1 and set(tr.adamw_sites().values()) == {"scan"}
    m, lo, hi, _ = tiny()
    off = Trainer(m, 4)
    assert off.skip_nonfinite is False and off._guard_state is None and off._skip_flag is None and off.fuse_adamw
    off.step(lo, hi)
    assert "guard" not in off.state_dict() and off.fused_adamw_params > 0 and off.state_dict()["step"] == 1


# ---------------------------------------------------------------------------------------------------- T2. a skipped step
@pytest.mark.parametrize("form", ["accum2", "accum2_eager", "no_overwrite", "no_overwrite_eager", "no_overwrite_lr_scales_clip"])
@pytest.mark.parametrize("value", [NAN, INF])
def test_skipped_step_leaves_the_state_alone_poisoned_gradient(form, value, monkeypatch):
    """route (a): the backward accumulates; NaN / +Inf written into one element of the flat gradient before the last micro-step"""
    kw = dict(ema_decay=0.5)
    if form.startswith("accum2"):
        kw["accum_iter"] = 2
    else:
        monkeypatch.setenv("TULIP_GRAD_OVERWRITE", "0")
    if form.endswith("eager"):
        kw["use_graph"] = False
    m, lo, hi, _ = tiny()
    if form.endswith("lr_scales_clip"):
        kw.update(lr_scales=layer_decay_scales(m, layers_per_group=8), clip_grad=CLIP)
    tr = Trainer(m, 4, skip_nonfinite=True, **kw)
    assert not tr.grad_overwrite
    bad = skipped_step_failures(tr, lo, hi, poison=value)
    assert bad == [], "\n".join(bad)


@pytest.mark.parametrize("form", ["captured", "eager", "dropout"])
def test_skipped_step_leaves_the_state_alone_nan_batch(form):
    """route (b): the overwriting backward; a batch whose low-resolution input has one whole sample set to NaN"""
    kw = {"eager": dict(use_graph=False)}.get(form, {})
    m, lo, hi, bad_lo = tiny(drop=0.1 if form == "dropout" else None)
    tr = Trainer(m, 4, skip_nonfinite=True, ema_decay=0.5, **kw)
    assert tr.grad_overwrite
    bad = skipped_step_failures(tr, lo, hi, bad_lo=bad_lo)
    assert bad == [], "\n".join(bad)


# ---------------------------------------------------------------------------------------------------- T3. recovery
@pytest.mark.parametrize("case", ["one_bad", "two_bad", "clip_inf"])
def test_recovery(case, monkeypatch):
    """DropPath 0, captured, resident batch: good, good, bad [, bad], good, good ends bit for bit where four good steps at the
    same learning rates end.  clip_inf: +Inf in the gradient under clip_grad -- skipped, not stepped with coefficient 0."""
    if case == "clip_inf":
        monkeypatch.setenv("TULIP_GRAD_OVERWRITE", "0")

    def make():
        m, lo, hi, bad_lo = tiny(drop_path=0.0)
        tr = Trainer(m, 4, skip_nonfinite=True, ema_decay=0.9, clip_grad=CLIP if case == "clip_inf" else None)
        return tr, lo, hi, bad_lo

    bad = recovery_failures(make, INF if case == "clip_inf" else "batch", n_bad=2 if case == "two_bad" else 1)
    assert bad == [], "\n".join(bad)


# ---------------------------------------------------------------------------------------------------- T4. checkpoints
def test_checkpoint_carries_the_applied_count():
    m, lo, hi, bad_lo = tiny(drop_path=0.0)
    tr = Trainer(m, 4, skip_nonfinite=True, ema_decay=0.9)
    tr.step(lo, hi, lr=lr_at(1))
    tr.step(bad_lo, hi, lr=lr_at(2))
    tr.step(bad_lo, hi, lr=lr_at(3))
    tr.step(lo, hi, lr=lr_at(4))
    tr.step(bad_lo, hi, lr=lr_at(5))
    torch.cuda.synchronize()
    sd_model, sd = {k: v.clone() for k, v in m.state_dict().items()}, tr.state_dict()
    assert sd["step"] == tr.applied_steps == 2 and sd["guard"] == {"applied": 2, "skipped": 3, "consecutive": 1}
    assert sd["ema"]["num_updates"] == 2
    m2, _, _, _ = tiny(drop_path=0.0)
    m2.load_state_dict(sd_model)
    tr2 = Trainer(m2, 4, skip_nonfinite=True, ema_decay=0.9)
    tr2.load_state_dict(sd)
    assert (tr2.applied_steps, tr2.skipped_steps, tr2.consecutive_skips, tr2.t) == (2, 3, 1, 2)
    for t in (tr, tr2):
        t.step(lo, hi, lr=lr_at(6))
    torch.cuda.synchronize()
    assert differing(guard_bits(tr), guard_bits(tr2)) == []
    assert tr2.applied_steps == 3 == tr.applied_steps and tr2.consecutive_skips == 0
    # the torch optimizer's step count is the applied count, both ways
    ps = list(m2.parameters())                    # (the fused AdamW decays ndim > 1 parameters only: timm's two groups)
    opt = torch.optim.AdamW([{"params": [q for q in ps if q.ndim > 1], "weight_decay": 0.01},
                             {"params": [q for q in ps if q.ndim <= 1], "weight_decay": 0.0}], lr=1e-3)
    tr2.export_torch_optimizer(opt)
    assert {int(s["step"].item()) for s in opt.state.values()} == {3}
    tr2.import_torch_optimizer(opt)
    assert (tr2.applied_steps, tr2.skipped_steps, tr2.t) == (3, 3, 3)
    # a dictionary from an unguarded Trainer: every step was applied
    m3, _, _, _ = tiny(drop_path=0.0)
    plain = Trainer(m3, 4)
    for t in range(3):
        plain.step(lo, hi, lr=lr_at(t + 1))
    torch.cuda.synchronize()
    sd3 = plain.state_dict()
    assert "guard" not in sd3 and sd3["step"] == 3
    m4, _, _, _ = tiny(drop_path=0.0)
    m4.load_state_dict({k: v.clone() for k, v in m3.state_dict().items()})
    guarded = Trainer(m4, 4, skip_nonfinite=True)
    guarded.load_state_dict(sd3)
    assert (guarded.applied_steps, guarded.skipped_steps, guarded.consecutive_skips, guarded.t) == (3, 0, 0, 3)
    for t in (plain, guarded):
        t.step(lo, hi, lr=lr_at(4))
    torch.cuda.synchronize()
    assert differing(state_bits(plain), state_bits(guarded)) == [] and guarded.applied_steps == 4


# ---------------------------------------------------------------------------------------------------- T5. one-rank RCCL forms
def test_one_rank_rccl_plans(tmp_path):
    """graph segments with the end-of-step "adamw" graph, the same with the bf16 exchange, and the one graph with captured
    collectives: one rank on RCCL in a fresh child process (tests/guard_ws1_worker.py), ended by `timeout` if it stalls."""
    out = tmp_path / "guard_ws1.pt"
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29561")
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tests", "guard_ws1_worker.py"), str(out)],
                       env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = torch.load(out)
    assert got["backend"] == "nccl"
    want_form = {"segments": "segments", "bf16": "segments", "captured": "one_graph_captured_collectives"}
    for name, form in want_form.items():
        g = got[name]
        assert g["form"] == form and g["segmented"] and g["buckets"] >= 2, (name, g["form"], g["buckets"])
        assert not g["bucket_adamw"] and not g["fuse_adamw"], name
        assert g["skip"] == [], (name, "\n".join(g["skip"]))
        assert g["recovery"] == [], (name, "\n".join(g["recovery"]))
    assert got["bf16"]["gb"]


# ---------------------------------------------------------------------------------------------------- T6. refusals
def test_refusals():
    m, _, _, _ = tiny()
    with pytest.raises(ValueError, match="sharded"):
        Trainer(m, 4, exchange="sharded", skip_nonfinite=True)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="skip_nonfinite"):
            Trainer(m, 4, skip_nonfinite=bad)


# ---------------------------------------------------------------------------------------------------- T7. the epoch loop
ARGS = dict(lr=5e-4, min_lr=0.0, warmup_epochs=0, epochs=2)


class RecordingLoader(list):
    """a list of batches that records the trainer's loss after every step (a module-level class and no saved exception info: no
    reference cycle keeps a Trainer and its captured graphs alive beyond its test)"""
    def __init__(self, batches, trainer):
        super().__init__(batches)
        self.trainer, self.seen = trainer, []

    def __iter__(self):
        for b in list.__iter__(self):
            yield b
            self.seen.append(self.trainer.P.losses[0].item())


def exit_code(fn):
    """the status fn() exits with (None: it returned); the exception and its traceback are dropped here"""
    try:
        fn()
    except SystemExit as e:
        return e.code
    return None


def test_train_one_epoch_goes_on_past_a_skipped_step(capsys):
    m, lo, hi, bad_lo = tiny(drop_path=0.0)
    tr = Trainer(m, 4, skip_nonfinite=True)
    batches = [(lo, hi), (lo, hi), (bad_lo, hi), (lo, hi), (lo, hi)]
    loader = RecordingLoader(batches, tr)
    stats = train_one_epoch(tr, loader, 0, SimpleNamespace(**ARGS))
    seen = loader.seen
    assert len(seen) == 5 and not math.isfinite(seen[2]) and all(math.isfinite(seen[i]) for i in (0, 1, 3, 4)), seen
    finite = [seen[i] for i in (0, 1, 3, 4)]
    assert stats["loss"] == sum(finite) / 4
    assert (tr.skipped_steps, tr.applied_steps, tr.consecutive_skips) == (1, 4, 0)
    assert len([l for l in capsys.readouterr().out.splitlines() if "skipped" in l]) == 1


def test_train_one_epoch_stops_after_max_skipped_steps():
    m, lo, hi, bad_lo = tiny(drop_path=0.0)
    tr = Trainer(m, 4, skip_nonfinite=True)
    batches = [(lo, hi), (bad_lo, hi), (bad_lo, hi), (lo, hi)]
    assert exit_code(lambda: train_one_epoch(tr, batches, 0, SimpleNamespace(max_skipped_steps=2, **ARGS))) == 1
    assert (tr.skipped_steps, tr.applied_steps, tr.consecutive_skips) == (2, 1, 2)
    # a NaN target pixel: NaN loss, zero gradient there -- the step is taken, and the loss still stops the loop
    m, lo, hi, _ = tiny(drop_path=0.0)
    tr = Trainer(m, 4, skip_nonfinite=True)
    hi_nan = hi.clone()
    hi_nan[0, 0, 0, 0] = NAN
    assert exit_code(lambda: train_one_epoch(tr, [(lo, hi_nan)], 0, SimpleNamespace(**ARGS))) == 1
    assert (tr.skipped_steps, tr.applied_steps) == (0, 1) and math.isfinite(tr.grad_norm.item())


def test_train_one_epoch_unguarded_exits_as_before():
    m, lo, hi, bad_lo = tiny(drop_path=0.0)
    tr = Trainer(m, 4)
    assert exit_code(lambda: train_one_epoch(tr, [(lo, hi), (bad_lo, hi), (lo, hi)], 0, SimpleNamespace(**ARGS))) == 1
    assert tr.t == 2

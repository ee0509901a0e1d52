"""Shared by tests/test_guard_gpu.py and tests/guard_ws1_worker.py: Trainer(skip_nonfinite=True) steps -- a step whose gradient norm
is not finite leaves the whole training state bit-unchanged, and a run that skipped steps ends where the run that never saw them
ends.  Every comparison is bit for bit.  Tiny model (8x256 -> 32x256, depths (2, 2), embed_dim 48), batch 4."""
import math

import torch

from oracle import tulip_oracle as O
from tests import adamw_audit as AA
from tests.clip_check import differing, lr_at, state_bits

DEV = "cuda"
NAN, INF = float("nan"), float("inf")


def tiny(seed=0, drop_path=0.1, drop=None):
    """the tiny model (drop_path: DropPath rate; drop: element dropout at that rate too), one good batch of 4 and the same batch with
    one whole low-resolution sample set to NaN"""
    from tests.test_model_gpu import build
    torch.manual_seed(seed)
    cfg = O.tiny_config(drop_path_rate=drop_path)
    sd = O.key_seeded_state_dict(cfg, seed=3)
    if drop is None:
        m = build(cfg, sd, train=True)
    else:
        from tests.test_dropout_gpu import _tiny_model
        m = _tiny_model(cfg, sd, drop)
    lo, hi = (t.to(DEV) for t in O.synthetic_batch(cfg, 4, seed=77))
    bad = lo.clone()
    bad[1] = NAN
    return m, lo, hi, bad


def guard_bits(tr):
    """everything a skipped step must leave alone: master, bf16 copy, both moments, and the average's shadow and counter"""
    s = state_bits(tr)
    if tr.ema is not None:
        s["ema"] = tr.ema.shadow.clone()
        if tr.ema.counter is not None:
            s["ema_counter"] = tr.ema.counter.clone().view(torch.int32)
    return s


def poison_index(tr) -> int:
    """an element in the middle of the largest parameter tensor"""
    W = tr.eng.params
    n = max(W.names, key=lambda k: W.numel[k])
    return W.offset[n] + W.numel[n] // 2


def optimizer_step(tr, lr, poison=None):
    """accum_iter Trainer.step() calls on the resident batch = one optimizer step; poison: written into one element of the flat
    gradient before the last micro-step (the accumulating backward adds to it: no NaN passes through a forward kernel)"""
    for i in range(tr.accum_iter):
        if poison is not None and i == tr.accum_iter - 1:
            assert not tr.grad_overwrite, "poisoning g needs the accumulating backward"
            tr.g[poison_index(tr)] = poison
        tr.step(lr=lr)


def skipped_step_failures(tr, lo, hi, bad_lo=None, poison=None, warm=2):
    """`warm` good optimizer steps (moments, average and counter away from their initial values), then ONE bad one -- the batch with
    a NaN sample (bad_lo) or a poisoned gradient element -- and the list of everything that is not as the guard promises."""
    assert (bad_lo is None) != (poison is None)
    out = []
    tr.load_batch(lo, hi)
    for t in range(warm):
        optimizer_step(tr, lr_at(t + 1))
    torch.cuda.synchronize()
    if tr.applied_steps != warm or tr.skipped_steps != 0 or int(tr.last_step_skipped.item()) != 0:
        out.append(f"after {warm} good steps: applied {tr.applied_steps}, skipped {tr.skipped_steps}")
    before = guard_bits(tr)
    segs = tr._segments
    if bad_lo is not None:
        tr.load_batch(bad_lo, hi)
    optimizer_step(tr, lr_at(warm + 1), poison=poison)
    torch.cuda.synchronize()
    norm = tr.grad_norm.item()
    print(f"skipped step: grad_norm {norm!r}, form {tr.step_form}, overwrite {tr.grad_overwrite}")
    assert not math.isfinite(norm), f"the bad step's gradient norm read back finite ({norm!r}): the test would pass for the wrong reason"
    out += [f"changed by the skipped step: {k}" for k in differing(before, guard_bits(tr))]
    if (tr.applied_steps, tr.skipped_steps, tr.consecutive_skips, int(tr.last_step_skipped.item())) != (warm, 1, 1, 1):
        out.append(f"counters after the skipped step: applied {tr.applied_steps}, skipped {tr.skipped_steps}, "
                   f"consecutive {tr.consecutive_skips}, flag {int(tr.last_step_skipped.item())}")
    if tr.use_graph and tr._segments is not segs:
        out.append("the step was captured again")
    if not tr.grad_overwrite and bool((AA._bits(tr.g) != 0).any()):
        out.append(f"g is not all zero after the skipped step ({int((AA._bits(tr.g) != 0).sum())} elements)")
    # ... and the next good step is taken
    tr.load_batch(lo, hi)
    optimizer_step(tr, lr_at(warm + 2))
    torch.cuda.synchronize()
    if (tr.applied_steps, tr.skipped_steps, tr.consecutive_skips, int(tr.last_step_skipped.item())) != (warm + 1, 1, 0, 0):
        out.append(f"counters after the next good step: applied {tr.applied_steps}, skipped {tr.skipped_steps}, "
                   f"consecutive {tr.consecutive_skips}, flag {int(tr.last_step_skipped.item())}")
    after = guard_bits(tr)
    if not math.isfinite(tr.grad_norm.item()) or not all(bool(torch.isfinite(after[k].float()).all()) for k in ("p", "m", "v")):
        out.append("the step after the skipped one is not finite")
    if not {"p", "shadow", "m", "v"} <= set(differing(before, after)):
        out.append(f"the step after the skipped one changed only {differing(before, after)}")
    return out


def run_sequence(tr, lo, hi, plan, bad_lo=None):
    """plan: one entry per optimizer step -- (lr, None) good, (lr, "batch") the NaN batch, (lr, value) a poisoned gradient element.
    The batch is loaded at every step (resident buffers; a captured step is replayed, never captured again).  Returns the final bits."""
    segs = None
    for lr, what in plan:
        tr.load_batch(bad_lo if what == "batch" else lo, hi)
        optimizer_step(tr, lr, poison=None if what in (None, "batch") else what)
        if tr.use_graph:
            assert segs is None or tr._segments is segs, "the step was captured again between batches"
            segs = tr._segments
    torch.cuda.synchronize()
    return guard_bits(tr)


def recovery_failures(make, bad, n_bad=1):
    """Run A: good, good, n_bad x bad, good, good; run B: good x 4 at A's learning rates of the taken steps; `make()` -> (guarded
    Trainer, lo, hi, bad_lo).  `bad`: "batch" or the value poisoned into the gradient."""
    lrs = [lr_at(t + 1) for t in range(4 + n_bad)]
    plan_a = [(lrs[0], None), (lrs[1], None)] + [(lrs[2 + i], bad) for i in range(n_bad)] + [(lrs[2 + n_bad], None), (lrs[3 + n_bad], None)]
    plan_b = [(lr, what) for lr, what in plan_a if what is None]
    out = []
    tr, lo, hi, bad_lo = make()
    a = run_sequence(tr, lo, hi, plan_a, bad_lo)
    if (tr.applied_steps, tr.skipped_steps, tr.consecutive_skips) != (4, n_bad, 0):
        out.append(f"run A: applied {tr.applied_steps}, skipped {tr.skipped_steps}, consecutive {tr.consecutive_skips}")
    if tr.state_dict()["step"] != 4:
        out.append(f"run A: state_dict()['step'] = {tr.state_dict()['step']}")
    form = tr.step_form
    del tr
    tr, lo, hi, bad_lo = make()
    b = run_sequence(tr, lo, hi, plan_b, bad_lo)
    if (tr.applied_steps, tr.skipped_steps) != (4, 0):
        out.append(f"run B: applied {tr.applied_steps}, skipped {tr.skipped_steps}")
    out += [f"run A ({form}) differs from the run without the bad batch in {k}" for k in differing(a, b)]
    if not all(bool(torch.isfinite(a[k].float()).all()) for k in a if k != "ema_counter"):
        out.append("run A's final state is not finite")
    return out

"""Shared by tests/test_ema_gpu.py and tests/ema_ws1_worker.py: Trainer steps with the weight average checked, bit for bit,
against the host definition (tulip_amd.ema.ema_update_host) applied to snapshots of the flat parameter buffer."""
import numpy as np
import torch

from tulip_amd.ema import ema_update_host


def to_np(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy().copy()


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def where_of(W, idx: int) -> str:
    for n in W.names:
        if W.offset[n] <= idx < W.offset[n] + W.numel[n]:
            return f"{n}[{idx - W.offset[n]}]"
    return f"padding[{idx}]"


def describe(W, got: np.ndarray, want: np.ndarray) -> str:
    diff = np.flatnonzero(bits(got) != bits(want))
    names = sorted({where_of(W, int(i)).split("[")[0] for i in diff[:: max(1, diff.size // 64)]})
    i = int(diff[0])
    return (f"{diff.size} of {got.size} elements differ, first {where_of(W, i)}: {got[i]!r} != {want[i]!r}; "
            f"in {names[:6]}{' ...' if len(names) > 6 else ''}")


def tracked_steps(tr, calls: int, step=None):
    """`calls` Trainer.step() calls (micro-steps), a device synchronisation and a snapshot of W.flat behind each.  The host
    definition is applied to the snapshot after every call that was an optimizer step; the Trainer's shadow and counter must
    equal it after EVERY call (a micro-step that is no optimizer step leaves them as they were).
    Returns (list of failures, empty when every comparison held; number of optimizer steps; the losses of every call)."""
    W, ema = tr.eng.params, tr.ema
    torch.cuda.synchronize()
    host, n = to_np(ema.shadow), ema.num_updates
    bad, updates, losses = [], 0, []
    for i in range(calls):
        update = (tr.micro + 1) % tr.accum_iter == 0
        out = (step or tr.step)()
        torch.cuda.synchronize()
        losses.append(to_np(out))
        if update:
            host, n = ema_update_host(host, to_np(W.flat), ema.decay, n)
            updates += 1
        got = to_np(ema.shadow)
        if not np.array_equal(bits(got), bits(host)):
            bad.append(f"call {i + 1} ({'optimizer step' if update else 'micro-step'}): {describe(W, got, host)}")
        if ema.num_updates != n:
            bad.append(f"call {i + 1}: counter {ema.num_updates}, expected {n}")
    return bad, updates, losses

"""Shared by tests/test_clip_gpu.py and tests/clip_ws1_worker.py: Trainer steps with gradient clipping checked against the host
definition (tulip_amd/clip.py) -- the coefficient on the device bit for bit from the norm on the device, the norm against float64,
and every AdamW update audited (tests/adamw_audit.py) with the gradient scale fl32(base * coef) in place of 1/world."""
from dataclasses import dataclass

import numpy as np
import torch

from tests import adamw_audit as AA
from tests import lr_scale_audit as LS
from tulip_amd.clip import clip_coef_host, clipped_grad_scale_host

U = 2.0 ** -24


def f32_bits(x) -> int:
    return int(np.float32(x).view(np.uint32))


@dataclass
class ClipHyper(AA.Hyper):
    """adamw_audit.Hyper of a clipped step: the gradient scale the device reads is fl32(1/world * coef)."""
    coef: float = 1.0

    def f32(self):
        c = super().f32()
        c["gs"] = float(clipped_grad_scale_host(np.float32(c["gs"]), np.float32(self.coef)))
        return c


def lr_at(t):
    from tulip_amd.trainer import cosine_lr
    return cosine_lr(t / 4.0, 5e-4, 1e-5, 1.0, 3.0) + 1e-6 * t


def clipped_steps(tr, calls, scales=None, coef_below=0.8, step=None, t0=0):
    """`calls` Trainer.step() calls on the resident batch (micro-steps), a new learning rate at every optimizer step, snapshots
    around each.  At every optimizer step:
      * Trainer.clip_coef has the bits of clip_coef_host(Trainer.grad_norm, Trainer.clip_grad) and is below `coef_below`;
      * where the step keeps its gradient (the overwriting backward: accum_iter == 1) Trainer.grad_norm is the float64 norm of the
        snapshot's g to 1e-6 relative (tests/test_ops_gpu.py::test_grad_norm's tolerance), the moments are adamw_audit.emulate with
        ClipHyper (gs = fl32(base * coef)) bit for bit, and the audit runs gradient-known on fl32(g * gs);
      * elsewhere (AdamW clears the accumulated gradient) the audit runs gradient-unknown and the norm is checked against the
        gradient the moments imply, g^ = (m1 - b1 m0) / ((1 - b1) coef): each m1 carries at most 2u (|b1 m0| + |(1 - b1) g|) of
        rounding (adamw_audit's bound Em), so ||g^|| is within 2u (b1 ||m0|| + (1 - b1) ||g coef||) / ((1 - b1) coef) of the
        norm, plus the read-out's own 1e-6.
    A call that is no optimizer step leaves parameters, moments and shadow bit-unchanged.
    t0: the optimizer steps the Trainer has taken before (the test's own count).
    Returns (failures, [(norm, coef)] of the optimizer steps)."""
    lay = AA.layout_of(tr)
    groups = LS.groups_of(lay, scales or {})
    bad, seen, t = [], [], t0
    for i in range(calls):
        update = (tr.micro + 1) % tr.accum_iter == 0
        lr = lr_at(t + 1)
        before = AA.snapshot(tr)
        (step or tr.step)(lr=lr)
        after = AA.snapshot(tr)
        if not update:
            bad += [f"call {i + 1}: {s}" for s in AA.audit_unchanged(before, after, lay)]
            continue
        t += 1
        norm, coef_dev = np.float32(tr.grad_norm.item()), np.float32(tr.clip_coef.item())
        coef, _ = clip_coef_host(norm, tr.clip_grad)
        seen.append((float(norm), float(coef_dev)))
        if f32_bits(coef) != f32_bits(coef_dev):
            bad.append(f"call {i + 1}: clip_coef {coef_dev!r} on the device, {coef!r} from the host definition (norm {norm!r})")
        if not coef_dev < coef_below:
            bad.append(f"call {i + 1}: coef {coef_dev!r} is not below {coef_below} (norm {norm!r}, clip_grad {tr.clip_grad})")
        known = bool(tr.grad_overwrite)
        g = after["g"] if known else None
        b1 = float(np.float32(tr.betas[0]))
        if known:
            ref = float(g.double().norm().item()) / tr.world
            tol = 1e-6 * ref
        else:
            gh = (after["m"].double() - b1 * before["m"].double()) / (1.0 - b1)            # = g * fl32(base * coef)
            ref = float(gh.norm().item()) / float(coef)
            tol = 1e-6 * ref + 2 * U * (b1 * float(before["m"].double().norm().item()) + (1.0 - b1) * float(gh.norm().item())) \
                / ((1.0 - b1) * float(coef))
        if not abs(float(norm) - ref) <= tol:
            bad.append(f"call {i + 1}: grad_norm {float(norm)!r}, float64 {'of g' if known else 'from the moments'} {ref!r} (tolerance {tol:.3g})")
        h = ClipHyper(lr=lr, t=t, betas=tuple(tr.betas), eps=tr.eps, wd=tr.wd, world=tr.world, coef=float(coef))
        gc = None
        if known:
            # the moments are adamw_step4 on (g, gs = fl32(base * coef)) bit for bit: adamw_audit.emulate with the clipped Hyper
            decay, inside, _, _, _ = lay.tensors(g.device)
            _, me, ve = AA.emulate(before["p"], g, before["m"], before["v"], decay, h)
            for key, want in (("m", me), ("v", ve)):
                n_off = int((inside & (AA._bits(after[key]) != AA._bits(want))).sum())
                if n_off:
                    bad.append(f"call {i + 1} (t={t}): {key} differs from the emulation with gs = fl32(base * coef) in {n_off} elements")
            # ... and the audit on the gradient the step consumed, gr = fl32(g * gs) -- the one rounding the definition adds to an
            # unclipped step, where gs = 1/world is a power of two and g * gs is exact; the auditor's float64 bounds count the
            # roundings behind gr, so it is handed gr itself with a scale of 1
            gc = g * torch.tensor(h.f32()["gs"], dtype=torch.float32, device=g.device)
        for s, gl in sorted(groups.items()):
            hs = AA.Hyper(lr=LS.scaled_lr(lr, s), t=t, betas=tuple(tr.betas), eps=tr.eps, wd=tr.wd, world=1)
            idx = gl.index.to(after["p"].device)
            v = AA.audit(gl.cut(before), gl.cut(after), gl, hs, grad=None if gc is None else gc[idx])
            bad += [f"call {i + 1} (t={t}, scale {s:g}): {x}" for x in v]
    return bad, seen


def state_bits(tr):
    W = tr.eng.params
    return {"p": W.flat.clone(), "shadow": W.shadow.clone(), "m": tr.m.clone(), "v": tr.v.clone()}


def differing(a, b):
    return [k for k in a if not torch.equal(AA._bits(a[k]), AA._bits(b[k]))]

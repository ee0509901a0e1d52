"""tests/adamw_audit.py group by group: with per-parameter learning-rate scales every tensor is AdamW at its OWN rate,
lr_g = fl32(fl32(lr) * fl32(scale)) -- the product the kernels form (adamw_coef, csrc/common.h).  The auditor checks one
Hyper per call over a whole Layout, so the snapshots are cut into one compact set per distinct scale (every tensor with the
64-float padding behind it, re-addressed by a Layout of its own) and each set is audited, unchanged auditor, with that scale's
Hyper.  The scales come from the test's bookkeeping, never from the Trainer."""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from tests import adamw_audit as AA

ALIGN = 64


def scaled_lr(lr: float, scale: float) -> float:
    return float(np.float32(np.float32(lr) * np.float32(scale)))


class GroupLayout(AA.Layout):
    """The tensors `names` of a full Layout, packed one behind the other (each with its padding up to the 64-float boundary)."""

    def __init__(self, full: AA.Layout, names: List[str]):
        self.names = sorted(names, key=lambda n: full.offset[n])
        self.offset, self.numel, self.decays, self._dev = {}, {}, {}, {}
        off, pieces = 0, []
        for n in self.names:
            lo, hi = full.offset[n], (full.offset[n] + full.numel[n] + ALIGN - 1) // ALIGN * ALIGN
            self.offset[n], self.numel[n], self.decays[n] = off, full.numel[n], full.decays[n]
            pieces.append(torch.arange(lo, hi, dtype=torch.int64))
            off += hi - lo
        self.total = off
        self.index = torch.cat(pieces)

    def cut(self, snap: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        idx = self.index.to(snap["p"].device)
        return {k: t[idx] for k, t in snap.items()}


def groups_of(full: AA.Layout, scales: Dict[str, float]) -> Dict[float, GroupLayout]:
    """{float32 scale: GroupLayout}; names missing from `scales` are at 1.0.  Covers every tensor and every padding element."""
    by = {}
    for n in full.names:
        by.setdefault(float(np.float32(scales.get(n, 1.0))), []).append(n)
    out = {s: GroupLayout(full, names) for s, names in by.items()}
    assert sum(g.total for g in out.values()) == full.total
    return out


def audit_scaled(before, after, groups: Dict[float, GroupLayout], h: AA.Hyper, grad: Optional[torch.Tensor] = None,
                 known: Optional[torch.Tensor] = None, stats: Optional[dict] = None, **kw) -> List[str]:
    out = []
    for s, lay in sorted(groups.items()):
        hs = AA.Hyper(lr=scaled_lr(h.lr, s), t=h.t, betas=h.betas, eps=h.eps, wd=h.wd, world=h.world)
        idx = lay.index.to(after["p"].device)
        rep = AA.Report(lay, after["p"].device)
        v = AA.audit(lay.cut(before), lay.cut(after), lay, hs, grad=None if grad is None else grad[idx],
                     known=None if known is None else known[idx], report=rep, **kw)
        out.extend(f"scale {s:g} (lr {hs.lr:.6g}): {x}" for x in v)
        if stats is not None:
            for k, val in rep.stats.items():
                stats[k] = max(stats.get(k, 0.0), val)
    return out


def audit_run_scaled(snaps, full: AA.Layout, scales: Dict[str, float], hypers, grad_mode: str = "unknown", stats=None, **kw):
    """audit_run of tests/adamw_audit.py with every tensor at its own rate (hypers[i].lr is the UNSCALED rate of step i)."""
    groups = groups_of(full, scales)
    out = []
    for i, h in enumerate(hypers):
        a, b = snaps[i], snaps[i + 1]
        if h is None:
            v = AA.audit_unchanged(a, b, full)
        elif grad_mode == "unknown":
            v = audit_scaled(a, b, groups, h, stats=stats, **kw)
        else:
            g = b["g"]
            v = audit_scaled(a, b, groups, h, grad=g, known=(g != 0) if grad_mode == "nonzero" else None, stats=stats, **kw)
        out.extend(f"step {i + 1} (t={h.t if h else '-'}): {s}" for s in v)
    return out


def audited_steps_scaled(tr, n, grad_mode, scales, lr_at, t0=0):
    """n micro-steps of `tr`, a snapshot behind each (no sync), the learning rate changed at every step; every optimizer step
    audited group by group.  Returns (violations, stats, snapshots)."""
    lay = AA.layout_of(tr)
    snaps, hypers, t = [AA.snapshot(tr)], [], t0
    for _ in range(n):
        update = (tr.micro + 1) % tr.accum_iter == 0
        lr = lr_at(t + 1)
        tr.step(lr=lr)
        snaps.append(AA.snapshot(tr))
        if update:
            t += 1
        hypers.append(AA.Hyper(lr=lr, t=t) if update else None)
    stats = {}
    v = audit_run_scaled(snaps, lay, scales, hypers, grad_mode, stats=stats)
    assert torch.isfinite(tr.P.losses).all()
    return v, stats, snaps


def sites_seen(tr, scales: Dict[str, float]) -> Dict[str, set]:
    """{site: the distinct scales of the tensors it stepped} from the Trainer's plan, cross-checked against the plan's mask: a
    tensor is stepped beside the backward ("writeout" / "fold") exactly where bit 1 of its mask bytes is set."""
    W, sites = tr.eng.params, tr.adamw_sites()
    mask = tr._adam_mask.cpu() if tr._adam_mask is not None else None
    seen = {}
    for n in W.names:
        beside = bool((mask[W.offset[n] // ALIGN:(W.offset[n] + W.numel[n] + ALIGN - 1) // ALIGN] & 2).all()) if mask is not None else False
        assert beside == (sites[n] in ("writeout", "fold")), (n, sites[n], beside)
        seen.setdefault(sites[n], set()).add(float(np.float32(scales.get(n, 1.0))))
    return seen

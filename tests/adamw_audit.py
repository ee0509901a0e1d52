"""AdamW auditor: is every element that a training step wrote AdamW applied to a gradient, with that step's hyperparameters?

Works on snapshots (`snapshot(trainer)` before and after a step) and checks each element in float64 on the device the tensors
live on.  It trusts nothing of the code under test for what it expects:
  * hyperparameters come from the caller's own bookkeeping (`Hyper`: lr, betas, eps, weight decay, step index t, 1/world),
    rounded to float32 the way the device reads the 8-float hyper block (`float32(0.9)`, `float32(1 - 0.9**t)`, ...);
  * the decay group is the reference's rule (main_lidar_upsampling.py:282, timm's grouping): ndim > 1 decays, taken from
    `model.named_parameters()` -- never from FlatParams.decay_mask;  the FlatParams offsets give the layout only.

The expected step is torch.optim.AdamW:  p1 = p0 (1 - lr wd) - lr/bc1 * m1 / (sqrt(v1)/sqrt(bc2) + eps),
m1 = b1 m0 + (1 - b1) g,  v1 = b2 v0 + (1 - b2) g^2,  bc_i = 1 - b_i^t.  The device computes it in float32 in the order of
`adamw_step4` (csrc/common.h, contraction off):
    gr = g gs;  m = b1 m + (1 - b1) gr;  v = b2 v + ((1 - b2) gr) gr;  D = sqrtf(v) rsqrtf(bc2) + eps;
    p = p (1 - lr wd) - (lr / bc1) (m / D)                              (1 - lr wd -> 1 for the no-decay group)

Modes (per element):
  gradient known (`grad` given, element in `known`): m1 and v1 must equal a float32 emulation of adamw_step4 bit for bit
    (`exact=True`; one rounding per operation, so torch's float32 ops in the kernel's order are the emulation).
  gradient unknown (elsewhere): g^ = (m1 - b1 m0) / (1 - b1) is derived from the moments and v1 is checked against
    b2 v0 + (1 - b2) g^2 within the bound derived below.
  In both modes p1 must be within `ulps` float32 ulps of the emulation's last two lines evaluated on (p0, m1, v1) -- the ulp is
  the one of the largest of p1 and the two operands of the final subtraction, |p0 (1 - lr wd)| and |lr/bc1 * m1/D|: when the
  two nearly cancel, an ulp of the (tiny) result says nothing about the arithmetic.  rsqrtf (v_rsq_f32, <= 1 ulp) is the one
  operation of the formula that is not correctly rounded on gfx950 (sqrtf and the division are, without fast-math): the
  emulation takes rsqrt(bc2) as the correctly rounded value or one of its two float32 neighbours, one choice per step (all
  kernels read the same hyper block), whichever fits.  Evidence (MI355X, every plan of tests/test_adamw_audit_gpu.py): with
  the correctly rounded value alone, step t = 3 (bc2 = 0.142625) put some 0.02 % of the elements up to 4 ulps of the larger
  operand (2 of p1) off and every other step matched bit for bit -- one value of rsqrtf off by one ulp.  With the neighbour
  chosen, 2 ulps is a margin, not a need.  And p1 must be within the float64 bound `Ep` of torch.optim.AdamW's value (below).
  Always: the bf16 shadow is p1 rounded to bf16 (RNE) bit for bit, and the padding between parameters is bit-unchanged in p, m,
  v and the shadow.  `audit_unchanged` checks a micro-step that does not update (accum_iter > 1): everything bit-unchanged.

Bounds (u = 2^-24, unit roundoff of float32; every operation of the device is fl(x) = x (1 + d), |d| <= u; plus an absolute
floor of 16 * 2^-149 per bound against subnormal results).  Write A = |b1 m0|, B = |(1 - b1) g|.
  m:  m1 = (b1 m0 (1+d1) + (1 - b1) g (1+d2)) (1+d3)  =>  |m1 - (b1 m0 + (1 - b1) g)| <= 2u (A + B) (1 + 2u).  (1 - b1 and
      1 - b2 are exact in float32: Sterbenz.)  The products b1 m0 of two floats are exact in float64, so the float64 residual
      m1 - b1 m0 adds only a 2^-53 relative error:  |g^ - g| <= Eg = km u (A + |(1 - b1) g^|) / (1 - b1) (1 + 8u),  km = 2.
  v:  v1 = (b2 v0 (1+d4) + (1 - b2) g^2 (1+d5)(1+d6)) (1+d7)  =>  |v1 - (b2 v0 + (1 - b2) g^2)| <= kv u (b2 v0 + (1 - b2) g^2),
      kv = 3;  replacing g by g^:  (1 - b2) |g^2 - g^^2| <= (1 - b2) Eg (2 |g^| + Eg).
      Ev = kv u (b2 v0 + (1 - b2) (|g^| + Eg)^2) + (1 - b2) Eg (2 |g^| + Eg).
      The observed corruption m1 = b1 m0 + g gives g^ = g / (1 - b1) = 10 g: v misses its prediction by 99 (1 - b2) g^2, far
      outside Ev unless |g| is below ~4u A or ~2e-4 sqrt(v0) -- where the error does not matter for p either.
  p:  (float64 reference from the exact moments in gradient-known mode, from (m1, v1) otherwise; dm, dv: their bounds)
      D = sqrt(v)/sqrt(bc2) + eps,  q = m / D,  U = lr/bc1 q.  |q' - q| <= (dm + |q| dD) / (D - dD) with
      dD = min(sqrt(dv), dv / sqrt(v)) / sqrt(bc2) (|sqrt a - sqrt b| is below both).  The float32 evaluation adds: D relative
      4u (sqrtf, rsqrtf <= 2u, product, + eps), the quotient u, lr/bc1 u, the product u -> kU = 8 on |U|; 1 - lr wd and its
      product 2u -> kp = 3 on |p0 (1 - lr wd)|; the subtraction u |p1|.
      Ep = kp u |p0 (1 - lr wd)| + kU u |U| + lr/bc1 |q' - q| + u |p1|.
`exact=False` accepts any float32 evaluation of AdamW, torch.optim.AdamW's (lerp, addcmul, hyperparameters rounded from
Python doubles) included: the moments are then checked against their bounds instead of bit for bit (km = kv = 8: torch's lerp
weight float32(0.1) is 0.37u away from 1 - float32(0.9), times |g - m0| <= 10 B + 1.1 A, plus three roundings), kU = 16,
kp = 4, and no ulp check.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

U = 2.0 ** -24
FLOOR = 16 * 2.0 ** -149
_f32 = lambda x: float(np.float32(x))


@dataclass
class Hyper:
    """One optimizer step's hyperparameters as the test's own bookkeeping knows them (never read back from the Trainer)."""
    lr: float
    t: int
    betas: Tuple[float, float] = (0.9, 0.95)
    eps: float = 1e-8
    wd: float = 0.01
    world: int = 1

    def f32(self) -> Dict[str, float]:
        """The float32 values the device reads: the host computes the bias corrections in double and stores float32."""
        b1, b2 = self.betas
        return {"lr": _f32(self.lr), "b1": _f32(b1), "b2": _f32(b2), "eps": _f32(self.eps), "wd": _f32(self.wd),
                "bc1": _f32(1.0 - b1 ** self.t), "bc2": _f32(1.0 - b2 ** self.t), "gs": _f32(1.0 / self.world)}


class Layout:
    """Where each parameter lives in the flat buffers (FlatParams offsets) and whether it decays (the reference's rule)."""

    def __init__(self, model, params):
        ndim = {n: p.ndim for n, p in model.named_parameters()}
        self.names: List[str] = list(params.names)
        assert sorted(self.names) == sorted(ndim), "FlatParams and the module disagree on the parameter set"
        self.offset = {n: int(params.offset[n]) for n in self.names}
        self.numel = {n: int(params.numel[n]) for n in self.names}
        self.total = int(params.total)
        self.decays = {n: ndim[n] > 1 for n in self.names}
        self._dev = {}

    def tensors(self, device):
        """(per-element decay flag, per-element 'inside a parameter' flag, sorted starts, ends, names) on `device`."""
        key = str(device)
        if key not in self._dev:
            decay = torch.zeros(self.total, dtype=torch.bool)
            inside = torch.zeros(self.total, dtype=torch.bool)
            order = sorted(self.names, key=lambda n: self.offset[n])
            for n in order:
                lo, hi = self.offset[n], self.offset[n] + self.numel[n]
                inside[lo:hi] = True
                decay[lo:hi] = self.decays[n]
            starts = torch.tensor([self.offset[n] for n in order], dtype=torch.int64)
            ends = torch.tensor([self.offset[n] + self.numel[n] for n in order], dtype=torch.int64)
            self._dev[key] = (decay.to(device), inside.to(device), starts.to(device), ends.to(device), order)
        return self._dev[key]


def layout_of(trainer) -> Layout:
    return Layout(trainer.model, trainer.eng.params)


def snapshot(trainer, grad: bool = True) -> Dict[str, torch.Tensor]:
    """Clones of the fp32 master, the bf16 shadow, both moments (and the flat gradient) on the current stream, with no host
    sync: Trainer.step() orders all of its optimizer work before the caller's stream.  exchange="sharded": gather_state()
    first (master and moments whole again)."""
    if getattr(trainer, "exchange", "allreduce") == "sharded":
        trainer.gather_state()
    W = trainer.eng.params
    s = {"p": W.flat.clone(), "shadow": W.shadow.clone(), "m": trainer.m.clone(), "v": trainer.v.clone()}
    if grad:
        s["g"] = trainer.g.clone()
    return s


# ---------------------------------------------------------------------------------------------------------------- emulation
def emulate(p, g, m, v, decay, h: Hyper):
    """float32 adamw_step4 (csrc/common.h): one rounding per operation in the kernel's order; torch's float32 elementwise ops
    round once each and do not contract.  `decay`: bool per element.  Returns (p1, m1, v1)."""
    c = h.f32()
    f = lambda x: torch.tensor(x, dtype=torch.float32, device=p.device)
    b1, b2, eps, gs = f(c["b1"]), f(c["b2"]), f(c["eps"]), f(c["gs"])
    gr = g * gs
    m1 = b1 * m + (f(1.0) - b1) * gr
    v1 = b2 * v + ((f(1.0) - b2) * gr) * gr
    return _emulate_p(p, m1, v1, decay, c), m1, v1


def _coef(c, device, rsq_ulp=0):
    f = lambda x: torch.tensor(x, dtype=torch.float32, device=device)
    lr = f(c["lr"])
    dec = f(1.0) - lr * f(c["wd"])
    step = lr / f(c["bc1"])
    rbc2 = f(1.0 / math.sqrt(c["bc2"]))            # rsqrtf(bc2) correctly rounded; rsq_ulp: the float32 neighbour
    if rsq_ulp:
        rbc2 = torch.nextafter(rbc2, f(math.inf if rsq_ulp > 0 else 0.0))
    return dec, step, rbc2, f(c["eps"])


def _emulate_p(p, m1, v1, decay, c, parts=False, rsq_ulp=0):
    dec, step, rbc2, eps = _coef(c, p.device, rsq_ulp)
    pd = torch.where(decay, p * dec, p)
    upd = step * (m1 / (torch.sqrt(v1) * rbc2 + eps))
    p1 = pd - upd
    return (p1, pd, upd) if parts else p1


def _ulp(x):
    """float32 ulp of |x| (as float64), normal range and subnormals."""
    a = x.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- audit
class Report:
    def __init__(self, layout: Layout, device):
        self.layout, self.device = layout, device
        self.violations: List[str] = []
        self.stats: Dict[str, float] = {}

    def stat(self, key, value):
        self.stats[key] = max(self.stats.get(key, 0.0), float(value))

    def check(self, what: str, bad: torch.Tensor, excess: torch.Tensor, values: Dict[str, torch.Tensor], limit: int = 6):
        """Record violations of check `what` (`bad`: bool per element, `excess`: how far out, to pick the worst) -- one entry
        per parameter tensor (or 'padding'): count, worst element and its values."""
        if not bool(bad.any()):
            return
        _, _, starts, ends, order = self.layout.tensors(self.device)
        idx = torch.nonzero(bad).flatten()
        own = torch.searchsorted(starts, idx, right=True) - 1
        pad = (own < 0) | (idx >= ends[own.clamp_min(0)])
        own = torch.where(pad, torch.full_like(own, len(order)), own)
        counts = torch.bincount(own, minlength=len(order) + 1).cpu()
        ex = excess[idx].double()
        ex = torch.where(torch.isnan(ex), torch.full_like(ex, float("inf")), ex)
        out = []
        for k in torch.nonzero(counts).flatten().tolist():
            sel = own == k
            j = idx[sel][int(torch.argmax(ex[sel]))]
            name = "padding" if k == len(order) else order[k]
            n_all = (self.layout.total - sum(self.layout.numel.values())) if k == len(order) else self.layout.numel[name]
            vals = ", ".join(f"{key}={float(t[j]):.9g}" for key, t in values.items())
            off = int(j) - (0 if k == len(order) else self.layout.offset[name])
            out.append(f"{what}: {name}: {int(counts[k])}/{n_all} violate, worst [{off}] {vals}")
        self.violations.extend(out[:limit])
        if len(out) > limit:
            self.violations.append(f"{what}: ... (+{len(out) - limit} more tensors)")


def audit(before: Dict[str, torch.Tensor], after: Dict[str, torch.Tensor], layout: Layout, h: Hyper,
          grad: Optional[torch.Tensor] = None, known: Optional[torch.Tensor] = None, exact: bool = True, ulps: float = 2.0,
          report: Optional[Report] = None) -> List[str]:
    """Violations of one optimizer step from `before` to `after` (see the module docstring).  `grad`: the gradient the step
    consumed (None: gradient-unknown mode everywhere); `known`: bool per element, where `grad` is that gradient (default: all).
    `report`: collects the worst p error in ulps ('p_ulps') and the worst v residual as a fraction of its bound ('v_frac')."""
    dev = after["p"].device
    rep = report if report is not None else Report(layout, dev)
    rep.violations = []
    decay, inside, _, _, _ = layout.tensors(dev)
    c = h.f32()
    b1, b2 = c["b1"], c["b2"]
    c1, c2 = 1.0 - b1, 1.0 - b2
    km, kv, kU, kp = (2.0, 3.0, 8.0, 3.0) if exact else (8.0, 8.0, 16.0, 4.0)
    p0, m0, v0 = before["p"], before["m"], before["v"]
    p1, m1, v1 = after["p"], after["m"], after["v"]
    P0, M0, V0, P1, M1, V1 = (t.double() for t in (p0, m0, v0, p1, m1, v1))

    # ---- padding: bit-unchanged everywhere
    pad = ~inside
    for key in ("p", "m", "v", "shadow"):
        bad = pad & (_bits(before[key]) != _bits(after[key]))
        rep.check(f"padding written ({key})", bad, bad.double(), {"before": before[key], "after": after[key]})

    # ---- the moments
    if grad is not None:
        kn = inside if known is None else (known & inside)
        G = grad.double() * c["gs"]
        A, B = (b1 * M0).abs(), (c1 * G).abs()
        if exact:
            _, me, ve = emulate(p0, grad, m0, v0, decay, h)
            for key, got, want in (("m", m1, me), ("v", v1, ve)):
                bad = kn & (_bits(got) != _bits(want))
                rep.check(f"{key} != float32 adamw_step4 emulation", bad, (got.double() - want.double()).abs(),
                          {f"{key}0": before[key], f"{key}1": got, "expected": want, "g": grad})
        Em = km * U * (A + B) * (1 + 2 * U) + FLOOR
        em = (M1 - (b1 * M0 + c1 * G)).abs()
        bad = kn & ~(em <= Em)
        rep.check("m != b1 m0 + (1-b1) g", bad, em / Em, {"m0": m0, "m1": m1, "g": grad})
        Evk = kv * U * (b2 * V0 + c2 * G * G) + FLOOR
        evk = (V1 - (b2 * V0 + c2 * G * G)).abs()
        bad = kn & ~(evk <= Evk)
        rep.check("v != b2 v0 + (1-b2) g^2", bad, evk / Evk, {"v0": v0, "v1": v1, "g": grad})
        unk = inside & ~kn
    else:
        kn, unk = torch.zeros_like(inside), inside
    # gradient unknown: g^ from the moments, v1 against its prediction
    gh = (M1 - b1 * M0) / c1
    Eg = km * U * ((b1 * M0).abs() + (c1 * gh).abs()) / c1 * (1 + 8 * U) + FLOOR
    Ev = kv * U * (b2 * V0 + c2 * (gh.abs() + Eg) ** 2) + c2 * Eg * (2 * gh.abs() + Eg) + FLOOR
    ev = (V1 - (b2 * V0 + c2 * gh * gh)).abs()
    frac = ev / Ev
    bad = unk & ~(ev <= Ev)
    rep.check("v != b2 v0 + (1-b2) g^2 with g^ = (m1 - b1 m0)/(1-b1)", bad, frac,
              {"m0": m0, "m1": m1, "v0": v0, "v1": v1, "g^": gh})
    if bool(unk.any()):
        rep.stat("v_frac", frac[unk].max())

    # ---- the parameters: float32 emulation on (p0, m1, v1), in ulps; rsqrtf(bc2) is the correctly rounded value or one of its
    # two float32 neighbours -- one value for the whole step (every kernel reads the same hyper block): the one that reproduces
    # the most elements bit for bit (a faulty tensor must not pick it)
    if exact:
        best = None
        for r in (0, -1, 1):
            pe, pd, upd = _emulate_p(p0, m1, v1, decay, c, parts=True, rsq_ulp=r)
            scale = _ulp(torch.maximum(torch.maximum(pd.double().abs(), upd.double().abs()), pe.double().abs()))
            du = (P1 - pe.double()).abs() / scale
            du = torch.where(torch.isnan(du), torch.full_like(du, float("inf")), du)
            off = int((inside & (du > 0)).sum())
            if best is None or off < best[0]:
                best = (off, r, pe, du)
            if off == 0:
                break
        _, r, pe, du = best
        rep.stat("rsqrt_ulp_off", abs(r))
        bad = inside & ~(du <= ulps)
        rep.check(f"p more than {ulps:g} ulps from the float32 emulation", bad, du,
                  {"p0": p0, "p1": p1, "expected": pe, "m1": m1, "v1": v1})
        if bool(inside.any()):
            rep.stat("p_ulps", du[inside].max())
    # ---- ... and against torch.optim.AdamW in float64
    lr, wd, eps, bc1, bc2 = c["lr"], c["wd"], c["eps"], c["bc1"], c["bc2"]
    S, r2 = lr / bc1, 1.0 / math.sqrt(bc2)
    if grad is not None:
        G = grad.double() * c["gs"]
        Mr = torch.where(kn, b1 * M0 + c1 * G, M1)
        Vr = torch.where(kn, b2 * V0 + c2 * G * G, V1)
        dm = torch.where(kn, Em, torch.zeros_like(Em))
        dv = torch.where(kn, Evk, torch.zeros_like(Evk))
    else:
        Mr, Vr, dm, dv = M1, V1, torch.zeros_like(M1), torch.zeros_like(V1)
    D = Vr.sqrt() * r2 + eps
    q = Mr / D
    dD = torch.minimum(dv.sqrt(), dv / Vr.sqrt().clamp_min(1e-300)) * r2
    dq = torch.where(D > dD, (dm + q.abs() * dD) / (D - dD).clamp_min(1e-300), torch.full_like(D, float("inf")))
    dec = torch.where(decay, torch.full_like(P0, 1.0 - lr * wd), torch.ones_like(P0))
    pr = P0 * dec - S * q
    Ep = kp * U * (P0 * dec).abs() + kU * U * (S * q).abs() + S * dq + U * P1.abs() + FLOOR
    ep = (P1 - pr).abs()
    bad = inside & ~(ep <= Ep)
    rep.check("p outside the float64 bound of torch.optim.AdamW", bad, ep / Ep,
              {"p0": p0, "p1": p1, "expected": pr, "bound": Ep})

    # ---- the bf16 shadow: p1 rounded to bf16, exactly
    sb = p1.to(torch.bfloat16)
    bad = inside & (_bits(after["shadow"]) != _bits(sb))
    rep.check("shadow != bf16(p1)", bad, bad.double(), {"p1": p1, "shadow": after["shadow"], "expected": sb})
    return list(rep.violations)


def audit_unchanged(before: Dict[str, torch.Tensor], after: Dict[str, torch.Tensor], layout: Layout,
                    keys: Sequence[str] = ("p", "m", "v", "shadow")) -> List[str]:
    """A micro-step that does not update (accum_iter > 1): parameters, moments and the shadow bit-unchanged."""
    rep = Report(layout, after["p"].device)
    for key in keys:
        bad = _bits(before[key]) != _bits(after[key])
        rep.check(f"changed in a non-update micro-step ({key})", bad, bad.double(),
                  {"before": before[key], "after": after[key]})
    return list(rep.violations)


def audit_run(snaps: Sequence[Dict[str, torch.Tensor]], layout: Layout, hypers: Sequence[Optional[Hyper]],
              grad_mode: str = "unknown", report: Optional[Report] = None, **kw) -> List[str]:
    """Audit consecutive snapshots: hypers[i] is the step from snaps[i] to snaps[i+1] (None: a non-update micro-step).
    grad_mode: "unknown" (moments only), "known" (snaps[i+1]["g"] everywhere), "nonzero" (snaps[i+1]["g"] where it is not zero --
    the default plan: the elements stepped at the end keep their gradient, the ranges stepped beside the backward never store
    one)."""
    out = []
    rep = report if report is not None else Report(layout, snaps[0]["p"].device)
    for i, h in enumerate(hypers):
        a, b = snaps[i], snaps[i + 1]
        if h is None:
            v = audit_unchanged(a, b, layout)
        elif grad_mode == "unknown":
            v = audit(a, b, layout, h, report=rep, **kw)
        else:
            g = b["g"]
            known = (g != 0) if grad_mode == "nonzero" else None
            v = audit(a, b, layout, h, grad=g, known=known, report=rep, **kw)
        out.extend(f"step {i + 1} (t={h.t if h else '-'}): {s}" for s in v)
    return out

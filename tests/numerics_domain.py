"""Input builders, float64 references and acceptance predicates for the full-domain / out-of-scale numerics tests
(test_numerics_domain_cpu.py proves the predicates sharp on the CPU, test_numerics_domain_gpu.py applies them to the
kernels).  Everything here is plain torch / numpy on the CPU: no oracle module, no kernel code.

Every predicate returns a `Report`: the violations it found (an empty list = accepted), the worst error as a multiple of its
budget and where it occurred -- the tests assert on the first and print the second."""
import math
from dataclasses import dataclass, field

import numpy as np
import torch

F64 = torch.float64
SQRT1_2 = 0.70710678118654752440
INV_SQRT_2PI = 0.39894228040143267794


@dataclass
class Report:
    what: str
    violations: list = field(default_factory=list)
    worst: float = 0.0            # max over elements of |error| / budget
    where: str = ""

    @property
    def ok(self):
        return not self.violations

    def line(self):
        return f"{self.what}: worst error {self.worst:.3f} x budget at {self.where}"

    def __str__(self):
        return self.line() + ("" if self.ok else "; " + "; ".join(self.violations[:6]))


def _add(rep, cond_bad, msg, x=None):
    n = int(cond_bad.sum())
    if n:
        first = "" if x is None else f" (first at {x[cond_bad].reshape(-1)[0].item()!r})"
        rep.violations.append(f"{msg}: {n} elements{first}")


def _ratio(rep, err, budget, x):
    r = torch.where(budget > 0, err / budget.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    r = torch.nan_to_num(r, nan=math.inf)
    if r.numel():
        i = int(r.reshape(-1).argmax())
        if float(r.reshape(-1)[i]) >= rep.worst:
            rep.worst = float(r.reshape(-1)[i])
            rep.where = repr(x.reshape(-1)[i].item()) if torch.is_tensor(x) else str(x)
    return r


# ------------------------------------------------------------------ number formats
def bf16_from_bits(bits) -> torch.Tensor:
    """uint16 patterns (numpy / list / tensor of ints) -> bfloat16 tensor with exactly those bits"""
    a = np.asarray(bits, dtype=np.int64).astype(np.uint16).view(np.int16)
    return torch.from_numpy(a.copy()).view(torch.bfloat16)


def bits16(t) -> torch.Tensor:
    """bfloat16 / float16 tensor -> its bit patterns as int32 in [0, 65536)"""
    return t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def bits32(t) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def _floor_log2(r64):
    _, e = torch.frexp(r64.abs())                 # |r| = m 2^e, m in [0.5, 1); e = 0 for r = 0
    return e.to(torch.int64) - 1


def _pow2(k):
    """2^k as float64 for an int64 tensor k in the normal range, assembled from its bits: exact on every device (torch.ldexp is
    x * pow(2, k), and a device's float64 pow is not exact at every k -- a spacing one part in 2^53 off moves a tie)"""
    assert bool(((k > -1023) & (k < 1024)).all())
    return ((k.to(torch.int64) + 1023) << 52).view(torch.float64)


def _ulp_exp(r64, mant_bits, emin=-126):
    e = torch.where(r64 == 0, torch.full_like(_floor_log2(r64), emin), _floor_log2(r64)).clamp(min=emin)
    return e - mant_bits


def ulp(r64, mant_bits, emin=-126):
    """spacing of a binary format with `mant_bits` stored mantissa bits (bf16: 7, fp32: 23) at |r|, subnormal range included"""
    return _pow2(_ulp_exp(r64, mant_bits, emin))


def ulp_bf16(r64):
    return ulp(r64, 7)


def ulp_f32(r64):
    return ulp(r64, 23)


def round_bf16(r64, truncate=False) -> torch.Tensor:
    """float64 -> the bf16 value (returned as bfloat16) nearest to it, ties to even, computed exactly in float64 (a cast through
    float32 would round twice); overflow to inf; truncate=True chops instead (the wrong conversion of the CPU tests)."""
    k = _ulp_exp(torch.where(torch.isfinite(r64), r64, torch.zeros_like(r64)), 7)
    q = r64 * _pow2(-k)                           # exact: a power-of-two scaling, |q| < 2^9
    q = torch.trunc(q) if truncate else torch.round(q)     # torch.round: half to even
    out = q * _pow2(k)
    out = torch.where(out.abs() >= 2.0 ** 128, torch.copysign(torch.full_like(out, math.inf), r64), out)
    out = torch.where(torch.isfinite(r64), out, r64)
    return out.to(torch.float32).to(torch.bfloat16)        # exact: `out` is a bf16 value


# ------------------------------------------------------------------ 1. / 2. GELU and GELU'
GELU_E = 1e-6     # bound on the kernel's erf error: 1.5e-7 (Abramowitz-Stegun 7.1.26) + 6 roundings of terms <= 1.5 + 1 ulp of rcp
# Relative error of a probability p = __expf(s - lse), lse = mx + __logf(sum), of the attention backward (tests/attn_exact.py),
# per query row: lse is HELD in fp32, so it is off by up to ulp_f32(|lse|) (its own rounding, and the rounding of __logf(sum)
# scaled down to it), and exp turns an absolute error of its argument into a relative one of p -- at |lse| ~ 256 that term is
# 2^-15 and dominates; s - lse is exact or one rounding of a small number; the arguments that matter are -log n, small, where
# __expf (v_exp_f32 of x log2 e) and __logf are good to a few ulp: 8 x 2^-24 for the two of them and the roundings between.
# The same eps bounds the relative error of the row term delta = sum_key p dP against sum_key p |dP|: the common error of the p
# goes through linearly, and the fp32 sum over L <= 64 keys adds L 2^-24 < 2^-18, which fits under the half of ulp_f32(lse) that
# a round-to-nearest lse leaves unused.  (That holds for a delta summed over the keys; dO . O cancels across channels.)
# A derivation from the number formats, never fitted to a kernel.
ATTN_EXP_E = 8 * 2.0 ** -24


def attn_p_eps(lse64):
    return ulp_f32(lse64.abs()) + ATTN_EXP_E


def all_finite_bf16() -> torch.Tensor:
    """the 65 280 finite bf16 values, in pattern order"""
    p = np.arange(65536, dtype=np.int64)
    return bf16_from_bits(p[(p & 0x7F80) != 0x7F80])


def gelu_domain_matrix() -> torch.Tensor:
    """[512][128] bf16: every finite bf16 value once, zero padded"""
    v = torch.zeros(512 * 128, dtype=torch.bfloat16)
    f = all_finite_bf16()
    v[: f.numel()] = f
    return v.reshape(512, 128)


def gelu_ref(x64):
    return 0.5 * x64 * torch.special.erfc(-x64 * SQRT1_2)


def gelu_grad_ref(x64):
    return 0.5 * torch.special.erfc(-x64 * SQRT1_2) + x64 * torch.exp(-0.5 * x64 * x64) * INV_SQRT_2PI


def check_gelu(x, got, grad=False, what=None) -> Report:
    """x, got: bf16 tensors (input and the kernel's result).  |got - ref| <= 1/2 ulp_bf16(ref) (1 + 2^-6) + 1/2 |x| E for GELU,
    ... + 1/2 E + |x| phi(x) 2^-22 for GELU'; finite; sign of GELU = sign of x; GELU(x) == x bitwise where float64 says so."""
    rep = Report(what or ("gelu'" if grad else "gelu"))
    x64, g64 = x.to(F64).reshape(-1), got.to(F64).reshape(-1)
    xb, gb = x.reshape(-1), got.reshape(-1)
    ref = gelu_grad_ref(x64) if grad else gelu_ref(x64)
    half = 0.5 * ulp_bf16(ref) * (1 + 2.0 ** -6)
    if grad:
        budget = half + 0.5 * GELU_E + x64.abs() * torch.exp(-0.5 * x64 * x64) * INV_SQRT_2PI * 2.0 ** -22
    else:
        budget = half + 0.5 * x64.abs() * GELU_E
    fin = torch.isfinite(g64)
    _add(rep, ~fin, "non-finite result", x64)
    err = torch.where(fin, (g64 - ref).abs(), torch.full_like(ref, math.inf))
    r = _ratio(rep, err, budget, x64)
    _add(rep, r > 1, "error above budget", x64)
    if not grad:
        _add(rep, (x64 < 0) & (g64 > 0), "gelu(x) > 0 for x < 0", x64)
        _add(rep, (x64 > 0) & (g64 < 0), "gelu(x) < 0 for x > 0", x64)
        same = bits16(round_bf16(ref)) == bits16(xb)
        _add(rep, same & (bits16(gb) != bits16(xb)), "gelu(x) != x bitwise where float64 gelu(x) rounds to x", x64)
    return rep


def gelu_as7126_f32(x_f32: np.ndarray, grad=False) -> np.ndarray:
    """GELU / GELU' in float32 arithmetic with erf from Abramowitz & Stegun 7.1.26 as published:
    erf(z) = 1 - (a1 t + a2 t^2 + a3 t^3 + a4 t^4 + a5 t^5) exp(-z^2), t = 1 / (1 + p z), z >= 0; erf(-z) = -erf(z)."""
    f = np.float32
    p, a1, a2, a3, a4, a5 = f(0.3275911), f(0.254829592), f(-0.284496736), f(1.421413741), f(-1.453152027), f(1.061405429)
    x = x_f32.astype(np.float32)
    with np.errstate(over="ignore", under="ignore"):
        z = np.abs(x) * f(SQRT1_2)
        t = f(1) / (f(1) + p * z)
        gauss = np.exp(-(z * z)).astype(np.float32)
        erf = f(1) - ((((a5 * t + a4) * t + a3) * t + a2) * t + a1) * t * gauss
        erf = np.copysign(erf, x).astype(np.float32)
        if grad:
            return (f(0.5) * (f(1) + erf) + x * f(INV_SQRT_2PI) * gauss).astype(np.float32)
        return (f(0.5) * x * (f(1) + erf)).astype(np.float32)


def gelu_tanh_f64(x64):
    return 0.5 * x64 * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x64 + 0.044715 * x64 ** 3)))


def fused_block_fc1_bias() -> torch.Tensor:
    """the 384 fc1 pre-activations of item 2 (float32, every one a bf16 value): 0, +-2^-126, +-{2^-20 ... 100} with both bf16
    neighbours, and a uniform fill of [-6, 6]"""
    mags = bf16_from_bits(bits16(torch.tensor([2.0 ** -20, 1e-3, 0.25, 0.5, 1, 1.5, 2, 3, 4, 5, 5.5, 6, 8, 16, 100],
                                              dtype=torch.float32).to(torch.bfloat16)).numpy())
    b = bits16(mags)
    pos = torch.cat([b - 1, b, b + 1])
    pats = torch.cat([torch.tensor([0x0000, 0x0080, 0x8080]), pos, pos | 0x8000])
    vals = bf16_from_bits(pats.numpy()).float()
    fill = torch.linspace(-6, 6, 384 - vals.numel()).to(torch.bfloat16).float()
    out = torch.cat([vals, fill])
    assert out.numel() == 384 and torch.isfinite(out).all()
    return out


# ------------------------------------------------------------------ 3. fp32 <-> bf16 conversions
CAST_TAILS = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)


def cast_words() -> torch.Tensor:
    """float32 [393 216]: (p << 16) | t for every bf16 pattern p and the six low halves t -- ties both ways, carries into the
    exponent, overflow to inf, subnormals, +-0, +-inf, NaN payloads"""
    p = np.arange(65536, dtype=np.uint32)[:, None] << np.uint32(16)
    w = (p | np.asarray(CAST_TAILS, dtype=np.uint32)[None, :]).reshape(-1)
    return torch.from_numpy(w.view(np.float32).copy())


def check_cast(x32, got_bf16, what="fp32 -> bf16") -> Report:
    """bit-identical to torch's CPU conversion wherever x is not NaN (subnormals not flushed); NaN -> NaN (never inf)"""
    rep = Report(what)
    x32, got = x32.reshape(-1), got_bf16.reshape(-1)
    want = x32.to(torch.bfloat16)
    nan = torch.isnan(x32)
    _add(rep, ~nan & (bits16(got) != bits16(want)), "bits differ from round-to-nearest-even", x32)
    _add(rep, nan & ~torch.isnan(got.float()), "NaN did not stay NaN", bits32(x32))
    rep.worst = float(bool(rep.violations))
    return rep


def check_cast_up(pat_bf16, got32, what="bf16 -> fp32") -> Report:
    rep = Report(what)
    _add(rep, bits32(got32.reshape(-1)) != (bits16(pat_bf16.reshape(-1)) << 16), "bits differ", bits16(pat_bf16.reshape(-1)))
    rep.worst = float(bool(rep.violations))
    return rep


def cast_truncating(x32):
    return bf16_from_bits(((bits32(x32).to(torch.int64) >> 16) & 0xFFFF).numpy())


def cast_flushing(x32):
    sub = (x32.abs() < 2.0 ** -126) & (x32 != 0)
    return torch.where(sub, torch.copysign(torch.zeros_like(x32), x32), x32).to(torch.bfloat16)


def cast_nan_to_inf(x32):
    return torch.where(torch.isnan(x32), torch.copysign(torch.full_like(x32, math.inf), x32), x32).to(torch.bfloat16)


# ------------------------------------------------------------------ 4. log1p / expm1
PREP_GATE = (0.0, 120.0)
POST_GATE = (0.5, 100.0)


def all_fp16_image() -> torch.Tensor:
    """[1][256][256] float16 holding every fp16 pattern"""
    return torch.from_numpy(np.arange(65536, dtype=np.uint16).view(np.float16).copy()).reshape(1, 256, 256)


def check_log1p(raw16, got32, gate) -> Report:
    """range_prep with scale 1, log_transform 1: gate = (min, max) or None"""
    rep = Report("log1p, gate " + ("on" if gate else "off"))
    x = raw16.to(F64).reshape(-1)
    got = got32.to(F64).reshape(-1)
    if gate:
        keep = (x >= gate[0]) & (x <= gate[1])                      # NaN compares false: non-finite and out-of-range -> 0
        _add(rep, ~keep & (got != 0), "gated-out value did not produce 0", x)
        x = torch.where(keep, x, torch.zeros_like(x))
    ref = torch.log1p(x)
    _add(rep, torch.isnan(ref) != torch.isnan(got), "NaN positions differ", x)
    inf = torch.isinf(ref)
    _add(rep, inf & (got != ref), "infinite result differs", x)
    fin = torch.isfinite(ref)
    err = torch.where(fin, (got - ref).abs(), torch.zeros_like(ref))
    err = torch.where(fin & ~torch.isfinite(got), torch.full_like(err, math.inf), err)
    r = _ratio(rep, err, 2 * ulp_f32(ref), x)
    _add(rep, fin & (r > 1), "more than 2 fp32 ulp from float64 log1p", x)
    return rep


def check_expm1(pred32, got_pred_img, got_hi_img, gate, h_rows) -> Report:
    """eval_postprocess with log_transform 1, pred == hi == `pred32` [H][W], lo == pred32[::H/h]: hi_img = expm1(hi);
    pred_img = gated expm1(pred), rows 0::H/h restored from lo (so: ungated expm1)"""
    rep = Report("expm1")
    H = pred32.shape[0]
    f = H // h_rows
    x = pred32.to(F64)
    ref = torch.expm1(x)
    tol = 2 * ulp_f32(ref)
    e_hi = (got_hi_img.to(F64) - ref).abs()
    r = _ratio(rep, e_hi.reshape(-1), tol.reshape(-1), x.reshape(-1))
    _add(rep, r > 1, "hi_img more than 2 fp32 ulp from float64 expm1", x.reshape(-1))
    got = got_pred_img.to(F64)
    restored = torch.zeros_like(x, dtype=torch.bool)
    restored[::f] = True
    inside = (ref >= gate[0]) & (ref <= gate[1])
    near = ((ref - gate[0]).abs() <= tol) | ((ref - gate[1]).abs() <= tol)
    val_ok = (got - ref).abs() <= tol
    _add(rep, restored & ~val_ok, "restored row is not expm1(lo)", x)
    _add(rep, ~restored & ~near & inside & ~val_ok, "gated-in value more than 2 fp32 ulp off", x)
    _add(rep, ~restored & ~near & ~inside & (got != 0), "gated-out value did not produce 0", x)
    _add(rep, ~restored & near & ~(val_ok | (got == 0)), "value at a gate edge is neither expm1 nor 0", x)
    _ratio(rep, torch.where(restored | inside, (got - ref).abs(), torch.zeros_like(ref)).reshape(-1)[~near.reshape(-1)],
           tol.reshape(-1)[~near.reshape(-1)], x.reshape(-1)[~near.reshape(-1)])
    return rep


# ------------------------------------------------------------------ 5. LayerNorm
LN_FAMILIES = ("a", "b", "c", "d", "e", "f")
LN_WIDTHS = (48, 96, 384, 1536, 6144)


def ln_family_rows(fam, n, C, gen) -> torch.Tensor:
    r = torch.randn(n, C, generator=gen)
    if fam == "a":
        return r + 1000.0                                        # large common offset
    if fam == "b":
        return torch.full((n, C), 3.0)                           # zero variance
    if fam == "c":
        r[torch.arange(n), torch.randint(0, C, (n,), generator=gen)] = 1e4     # one outlier
        return r
    if fam == "d":
        return r * 1e-12                                         # eps dominates
    if fam == "e":
        return torch.where(torch.arange(C) % 2 == 0, 1e3, -1e3).expand(n, C).clone()
    return r                                                     # control


def ln_inputs(C, per_family=16, seed=0, families=LN_FAMILIES):
    """x [len(families) * per_family][C], gamma, beta (fp32), dy (bf16), and {family: row slice}"""
    gen = torch.Generator().manual_seed(1000 * seed + C)
    x = torch.cat([ln_family_rows(f, per_family, C, gen) for f in families])
    gamma = 1 + 0.1 * torch.randn(C, generator=gen)
    beta = 0.1 * torch.randn(C, generator=gen)
    dy = torch.randn(x.shape[0], C, generator=gen).to(torch.bfloat16)
    rows = {f: slice(i * per_family, (i + 1) * per_family) for i, f in enumerate(families)}
    return x, gamma, beta, dy, rows


def ln_torch(x, gamma, beta, dy, eps, dtype):
    """(y, mean, rstd, dx, dgamma, dbeta) of torch's LayerNorm in `dtype`, as float64 tensors"""
    xr = x.detach().to(dtype).clone().requires_grad_(True)
    g, b = gamma.detach().to(dtype).clone().requires_grad_(True), beta.detach().to(dtype).clone().requires_grad_(True)
    y, mean, rstd = torch.native_layer_norm(xr, (x.shape[-1],), g, b, eps)
    y.backward(dy.to(dtype))
    return {"y": y.detach().to(F64), "mean": mean.detach().reshape(-1).to(F64), "rstd": rstd.detach().reshape(-1).to(F64),
            "dx": xr.grad.to(F64), "dgamma": g.grad.to(F64), "dbeta": b.grad.to(F64)}


LN_OUTPUTS = ("y", "mean", "rstd", "dx", "dgamma", "dbeta")


def ln_baseline(x, gamma, beta, dy, eps):
    """float64 reference and the max |error| of torch float32 against it, per output"""
    ref = ln_torch(x, gamma, beta, dy, eps, F64)
    f32 = ln_torch(x, gamma, beta, dy, eps, torch.float32)
    err = {k: float((f32[k] - ref[k]).abs().max()) for k in LN_OUTPUTS}
    return ref, err


def check_ln(got: dict, ref: dict, err32: dict, what, factor=4.0) -> Report:
    """every output in `got` within factor x (torch float32's error) of float64; + 1/2 bf16 ulp of the reference for y"""
    rep = Report(what)
    rep.ratios = {}
    for k, g in got.items():
        g64, r64 = g.to(F64).reshape(-1), ref[k].reshape(-1)
        budget = torch.full_like(r64, factor * err32[k])
        if k == "y":
            budget = budget + 0.5 * ulp_bf16(r64)
        err = (g64 - r64).abs()
        err = torch.where(torch.isfinite(g64), err, torch.full_like(err, math.inf))
        sub = Report(k)
        r = _ratio(sub, err, budget, r64)
        # the kernel's own float32-side error (beyond the bf16 rounding of y) as a multiple of torch float32's
        excess = float((err - (budget - factor * err32[k])).clamp(min=0).max())
        rep.ratios[k] = excess / err32[k] if err32[k] > 0 else (0.0 if excess == 0 else math.inf)
        if sub.worst >= rep.worst:
            rep.worst, rep.where = sub.worst, f"{k} (ref {sub.where})"
        _add(rep, r > 1, f"{k}: above {factor} x torch-float32 error {err32[k]:.3e} (max err {float(err.max()):.3e})")
    return rep


def ln_onepass_f32(x, gamma, beta, eps):
    """the wrong LayerNorm of the CPU test: var = E[x^2] - E[x]^2 in float32"""
    x = x.float()
    m = x.mean(-1, keepdim=True)
    var = ((x * x).mean(-1, keepdim=True) - m * m).clamp(min=0)
    rstd = 1 / torch.sqrt(var + eps)
    return {"y": ((x - m) * rstd * gamma + beta).to(torch.bfloat16), "mean": m.reshape(-1), "rstd": rstd.reshape(-1)}


def ln_merge_scatter(rows, B, H, W, Cq):
    """merged rows [B H/2 W/2][4 Cq] -> the (B, H, W, Cq) tensor whose 2x2 patch merge (order (0,0), (1,0), (0,1), (1,1))
    gives those rows"""
    x = torch.empty(B, H, W, Cq, dtype=rows.dtype)
    r = rows.reshape(B, H // 2, W // 2, 4, Cq)
    for k, (dh, dw) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        x[:, dh::2, dw::2] = r[:, :, :, k]
    return x


def split3_exact(x):
    """three float32 slabs whose sum, in any order, is exactly x"""
    s0 = x.to(torch.bfloat16).float()
    r = x - s0
    s1 = r.to(torch.bfloat16).float()
    s2 = r - s1
    assert torch.equal((s0 + s1) + s2, x) and torch.equal(s0 + (s1 + s2), x)
    return torch.stack([s0, s1, s2])


# ------------------------------------------------------------------ 6. window attention
def rel_position_index(wh, ww) -> torch.Tensor:
    """[L][L] index into the ((2wh-1)(2ww-1), nh) bias table: (dh + wh-1)(2ww-1) + (dw + ww-1), d = query - key"""
    h, w = torch.meshgrid(torch.arange(wh), torch.arange(ww), indexing="ij")
    h, w = h.reshape(-1), w.reshape(-1)
    return (h[:, None] - h[None, :] + wh - 1) * (2 * ww - 1) + (w[:, None] - w[None, :] + ww - 1)


def region_labels(H, W, win, sft) -> torch.Tensor:
    """(H, W) labels of the shifted image: 3 x 3 bands [0, -w), [-w, -s), [-s, end) per axis, numbered in raster order"""
    lab = torch.zeros(H, W, dtype=torch.int64)
    cnt = 0
    for hs in (slice(0, -win[0]), slice(-win[0], -sft[0]), slice(-sft[0], None)):
        for ws in (slice(0, -win[1]), slice(-win[1], -sft[1]), slice(-sft[1], None)):
            lab[hs, ws] = cnt
            cnt += 1
    return lab


def to_windows(t, B, H, W, win, sft):
    """[B H W][ch] natural-order rows -> [B nW][L][ch]: cyclic shift by -sft, then window partition"""
    ch = t.shape[-1]
    x = torch.roll(t.reshape(B, H, W, ch), (-sft[0], -sft[1]), (1, 2))
    x = x.reshape(B, H // win[0], win[0], W // win[1], win[1], ch).permute(0, 1, 3, 2, 4, 5)
    return x.reshape(-1, win[0] * win[1], ch)


def from_windows(t, B, H, W, win, sft):
    ch = t.shape[-1]
    x = t.reshape(B, H // win[0], W // win[1], win[0], win[1], ch).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, ch)
    return torch.roll(x, (sft[0], sft[1]), (1, 2)).reshape(B * H * W, ch)


def attn_reference(qkv, table, B, H, W, C, nh, win, sft, masked, *, dtype=F64, softmax="exact", use_mask=True,
                   shift_error=(0, 0), round_p=False, p_mult=None, qk_cast=None):
    """The function documented above tulip_window_attn_fwd, in `dtype`: shift, partition, q * scale, + bias through the
    relative-position index, + 0 / -100 region mask, softmax, P.V, window reverse, reverse shift.  Returns (out [M][C],
    scores [B nW][nh][L][L]).  The keyword switches build the deliberately wrong variants of the CPU tests; p_mult
    ([B nW][nh][L][L], the attn_drop multiplier on the probabilities, ahead of their rounding) and qk_cast (a dtype q and k are
    rounded through: the fp8 scores) are the two documented options of the function."""
    L, P = win[0] * win[1], C // nh
    s_in = (sft[0] + shift_error[0], sft[1] + shift_error[1])
    t = to_windows(qkv.to(dtype), B, H, W, win, s_in).reshape(-1, L, 3, nh, P).permute(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]
    if qk_cast is not None:
        q, k = q.to(qk_cast).to(dtype), k.to(qk_cast).to(dtype)
    q = q * P ** -0.5
    s = q @ k.transpose(-2, -1)
    s = s + table.to(dtype)[rel_position_index(*win).reshape(-1)].reshape(L, L, nh).permute(2, 0, 1)[None]
    if masked and use_mask:
        lab = to_windows(region_labels(H, W, win, sft).reshape(H * W, 1), 1, H, W, win, (0, 0)).reshape(-1, L)
        mask = torch.where(lab[:, None, :] != lab[:, :, None], -100.0, 0.0).to(dtype)      # [nW][L][L]
        s = (s.reshape(B, -1, nh, L, L) + mask[None, :, None]).reshape(-1, nh, L, L)
    if softmax == "exact":
        p = torch.softmax(s, -1)
    else:                                           # no max subtraction
        e = torch.exp(s)
        p = e / e.sum(-1, keepdim=True)
    if p_mult is not None:
        p = p * p_mult.to(dtype)
    if round_p:
        p = p.to(torch.bfloat16).to(dtype)
    o = (p @ v).permute(0, 2, 1, 3).reshape(-1, L, C)
    return from_windows(o, B, H, W, win, s_in), s


def attn_inputs(family, B, H, W, C, nh, win, seed):
    """(qkv bf16 [M][3C], bias table fp32 [(2wh-1)(2ww-1)][nh], dout bf16 [M][C])"""
    gen = torch.Generator().manual_seed(seed)
    M, ntab = B * H * W, (2 * win[0] - 1) * (2 * win[1] - 1)
    qkv = torch.randn(M, 3, C, generator=gen)
    if family == "large":                           # (i): scores reach +-60
        qkv[:, :2] *= 4.0
        table = (torch.rand(ntab, nh, generator=gen) * 2 - 1) * 20.0
    elif family == "uniform":                       # (ii): exactly uniform softmax, v on small integers
        qkv[:, 0] = 0.0
        qkv[:, 2] = torch.randint(-3, 4, (M, C), generator=gen).float()
        table = torch.zeros(ntab, nh)
    else:                                           # (iii): the control
        qkv *= 1.5
        table = 0.5 * torch.randn(ntab, nh, generator=gen)
    dout = torch.randn(M, C, generator=gen).to(torch.bfloat16)
    return qkv.reshape(M, 3 * C).to(torch.bfloat16), table, dout


def _per_window_head(t, B, H, W, nh, win, sft):
    """[M][nh P] -> [B nW][nh][L P]"""
    L = win[0] * win[1]
    w = to_windows(t.to(F64), B, H, W, win, sft)
    return w.reshape(w.shape[0], L, nh, -1).permute(0, 2, 1, 3).reshape(w.shape[0], nh, -1)


def check_attn_fwd(got, ref, qkv, B, H, W, C, nh, win, sft, what) -> Report:
    """per window and head: |err| <= 2^-7 max|v| (P rows sum to 1; bf16 rounding of P and of the output: 2^-8 max|v|; x 2)"""
    rep = Report(what)
    v = _per_window_head(qkv.reshape(-1, 3, C)[:, 2], B, H, W, nh, win, sft).abs().amax(-1)
    g = _per_window_head(got, B, H, W, nh, win, sft)
    err = (g - _per_window_head(ref, B, H, W, nh, win, sft)).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, math.inf)).amax(-1)
    idx = torch.arange(err.numel()).reshape(err.shape)
    r = _ratio(rep, err.reshape(-1), (2.0 ** -7 * v).reshape(-1), idx.reshape(-1))
    rep.where = f"window-head #{rep.where}"
    _add(rep, r > 1, "window-heads above 2^-7 max|v|")
    return rep


def check_attn_dqkv(got, ref, B, H, W, C, nh, win, sft, what) -> Report:
    """per window and head, over that window-head's (q | k | v) slice of dqkv: |err| <= 2^-6 max|ref|"""
    rep = Report(what)

    def wh(t):        # [M][3 C] -> [B nW][nh][3 L P]
        parts = [_per_window_head(t.reshape(-1, 3, C)[:, i], B, H, W, nh, win, sft) for i in range(3)]
        return torch.cat(parts, -1)

    g, r64 = wh(got), wh(ref)
    err = torch.where(torch.isfinite(g), (g - r64).abs(), torch.full_like(g, math.inf)).amax(-1)
    idx = torch.arange(err.numel())
    r = _ratio(rep, err.reshape(-1), (2.0 ** -6 * r64.abs().amax(-1)).reshape(-1), idx)
    rep.where = f"window-head #{rep.where}"
    _add(rep, r > 1, "window-heads above 2^-6 max|ref|")
    return rep


ATTN_GRIDS = {(2, 8): (4, 16), (4, 8): (8, 16), (8, 8): (16, 16)}     # two windows each way
# seeds of family (i), one per (window, shifted): the first ones whose float64 scores (mask included) go above 92 and below -60 -- past
# 88.73 = log(FLT_MAX), where a float32 softmax without max subtraction overflows (the CPU test asserts both)
ATTN_LARGE_SEEDS = {((2, 8), False): 29, ((2, 8), True): 180, ((4, 8), False): 16, ((4, 8), True): 16, ((8, 8), False): 2,
                    ((8, 8), True): 2}


def attn_cases():
    """(family, C, nh, win, shifted) of item 6"""
    out = []
    for win in ATTN_GRIDS:
        for shifted in (False, True):
            for fam in ("large", "uniform", "control"):
                out.append((fam, 48, 3, win, shifted))
    out.append(("control", 96, 3, (2, 8), True))
    return out


def attn_seed(family, C, win, shifted):
    if family == "large":
        return ATTN_LARGE_SEEDS[(win, shifted)]
    return 100 + 10 * win[0] + int(shifted) + C


def attn_shift(win, shifted):
    return (win[0] // 2, win[1] // 2) if shifted else (0, 0)


# ------------------------------------------------------------------ 7. MC-dropout aggregate
def mc_cases():
    """(name, preds float32 [T][n], threshold)"""
    g = torch.Generator().manual_seed(7)
    out = []
    for n in (1, 257):
        base = torch.randn(n, generator=g) * 3            # both signs
        out.append((f"T=2 identical passes, n={n}", torch.stack([base, base]), 0.03))
        a, b = torch.rand(n, generator=g) + 0.5, torch.rand(n, generator=g) + 0.5
        out.append((f"mean exactly 0, n={n}", torch.stack([a, -a, b, -b]), 0.03))
        c = torch.rand(n, generator=g) * 50 + 1
        out.append((f"one outlier pass, n={n}", torch.stack([c, c, c, c + 40 * torch.rand(n, generator=g), c]), 0.5))
        d = torch.rand(6, n, generator=g) * 0.2 + torch.rand(n, generator=g) * 80
        out.append((f"generic, n={n}", d, 0.0005))
    return out


def check_mc(preds, thr, got, what) -> Report:
    """float64 statement of: mean over the passes, zeroed where the unbiased std exceeds threshold * mean.  Decisions are
    compared only where |sd - thr mean| > 1e-6 sd; kept means within one fp32 ulp of the float64 mean."""
    rep = Report(what)
    p = preds.to(F64)
    mean, sd = p.mean(0), p.std(0, unbiased=True)
    zero = sd > thr * mean
    safe = (sd - thr * mean).abs() > 1e-6 * sd
    g = got.to(F64).reshape(-1)
    _add(rep, safe & zero & (g != 0), "noisy pixel not zeroed", mean)
    kept_bad = (g - mean).abs() > ulp_f32(mean)
    _add(rep, safe & ~zero & kept_bad, "kept mean differs from float64", mean)
    _add(rep, ~safe & kept_bad & (g != 0), "pixel at the margin is neither the mean nor 0", mean)
    _ratio(rep, torch.where(safe & ~zero, (g - mean).abs(), torch.zeros_like(g)), ulp_f32(mean), mean)
    rep.n_compared = int(safe.sum())
    return rep

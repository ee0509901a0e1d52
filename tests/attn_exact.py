"""Exact tests of tulip_window_attn_fwd / _bwd and their _drop forms: case list, launch-rule functions, operand builders, float64
reference, checkers and a torch emulation with switchable defects (test_attn_exact_cpu.py proves the checkers sharp and the case
list complete, test_attn_exact_gpu.py applies them to the kernels).  Plain torch, on whichever device the caller names; no kernel
code.  39 GPU cases (gpu_cases()): per kernel instantiation (L, P, plain | drop | fp8) one small one-sweep case and one case of
>= 3 sweeps with a short last one per direction, and three single-row / single-column window grids.

The device of it all: SELECTOR operands.  Per (window, head, slot) q = A e_cq and k = A e_ck are one-hot over the head's channels
(the class ids come from a 4-subset of the P channels drawn per (window, head)), A a bf16 integer with T = A^2 scale >= 200, the
bias table holds only {0, -1000} and the shift mask adds the kernel's own 0 / -100: every logit is a T - 100 m - 1000 b with
a, m, b in {0, 1}.  All top-level logits of a row are bitwise equal in a kernel (the same operations on the same numbers), all
others are >= 100 below: the softmax is 1/n on the n top keys and < e^-100 elsewhere, bf16(p) is one fixed number whatever
few-ulp error the device's exp and rcp have, and with v on integers in [-4, 4], dout on integers in [-2, 2] and attn_drop at
p = 0.5 (multiplier exactly 0 or 2)

    out = bf16(sum_k bf16(p mult) v)        dV = bf16(sum_q bf16(p mult) dO)

are exactly known numbers (8-bit significands times small integers: the fp32 sum is exact in any order) and must match bit for
bit over the whole allocation, guard words included (-0 == +0).  dq, dk and d(bias) go through the unrounded p = exp(s - lse) and
are not exact: the reference carries, in float64, each value r and an error bound u propagated from a relative error
eps_i = numerics_domain.attn_p_eps(lse_i) on every p of query row i and on delta_i = sum p dP; a bf16 word must lie in
[bf16(r - u), bf16(r + u)] (one value -- "determined" -- wherever no tie lies inside), d(bias) within u + R ulp_f32.  The builder
asserts, from the reference alone, the gap, the rounding margin of 1/n, the stray mass, the coverage of n and the shares that keep
the intervals from hiding a failure (MIN_DETERMINED, MIN_NONZERO, DBIAS_U)."""
import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np
import torch

from tests import gemm_exact as GX
from tests import numerics_domain as ND
from tests.gemm_exact import Buf, Out, check_out
from tests.numerics_domain import Report
from tulip_amd import dropout as D

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
GAP = 100.0                    # (i): every other level of a row is at least this far below its top level
GAP_SLACK = 1e-9               # float64 rounding of (T - 100) against T where T = A^2 / sqrt(32) is irrational
TIE_MARGIN = Fraction(1, 4096)  # (ii): 1/n farther than 2^-12 relative from every tie between two bf16 neighbours
BIAS_LOW = -1000.0
T_RANGE = (200.0, 300.0)       # keeps ulp_f32(lse) at 2^-15
MIN_DETERMINED = 0.95
MIN_NONZERO = 0.25
DBIAS_U = 2.0 ** -10
DROP_P = 0.5
DROP_SEED, DROP_COUNTER, DROP_SITE = 0xA77E17, 5, D.site(3, D.ATTN)
REL_GUARD = 0x3FFFFFFF         # around rel_index: an index that lands nowhere near the table
CHUNK = 1 << 22                # score elements per chunk of windows
# class frequencies of the queries and of the keys: the keys use two of the four channels, so a query of the other two classes has no
# key of its class and its top level spans both key channels (dq then has more than one non-zero channel per row)
Q_WEIGHTS, K_WEIGHTS = (1.0, 1.0, 2.0, 2.0), (1.0, 1.0, 0.0, 0.0)
UNBIASED_KEYS = 5.0            # expected number of table entries at 0 among the L keys of a row


def _tie_distance(n):
    """relative distance of 1/n from the nearest tie between two bf16 neighbours, exactly"""
    x = Fraction(1, n)
    e = 0
    while Fraction(2) ** e > x:
        e -= 1
    ulp = Fraction(2) ** (e - 7)
    q = x / ulp
    frac = q - (q.numerator // q.denominator)
    return abs(frac - Fraction(1, 2)) * ulp / x


BAD_N = frozenset(n for n in range(1, 65) if _tie_distance(n) <= TIE_MARGIN)      # 9, 13, 15, 18, 26, 30, 36, 43, 52, 60


# ------------------------------------------------------------------ the launchers' rules (csrc/attention.hip), restated
def _route(groups, units, invalid=False):
    """(groups, sweeps, idle groups, short last sweep, invalid item in the last trip) of `units` work items dealt to `groups`"""
    sweeps = -(-units // groups)
    return (groups, sweeps, max(0, groups - units), sweeps > 1 and units % groups != 0, invalid)


def fwd16_route(total, L, nh):
    """pick_groups: one wave per group, ceil(4096 / nh) groups at most"""
    assert L == 16
    return _route(max(1, min(-(-4096 // nh), total)), total)


def bwd16_route(total, L, nh):
    """bwd_blocks_per_head: ceil(2048 / nh) groups at most, rounded up to the 4 waves of a workgroup"""
    assert L == 16
    return _route(4 * ((max(1, min(-(-2048 // nh), total)) + 3) // 4), total)


def _wide_route(total, L, nh, cap):
    assert L in (32, 64)
    it = 64 // L
    need = -(-total // it)
    return _route(max(1, min(cap // nh, need)), need, it == 2 and total % 2 == 1)


def wide_fwd_route(total, L, nh):
    """wide_groups: 2048 / nh one-wave workgroups per head at most, 64 / L windows per trip"""
    return _wide_route(total, L, nh, 2048)


def wide_bwd_route(total, L, nh):
    return _wide_route(total, L, nh, 512)


def fwd_route(total, L, nh):
    return fwd16_route(total, L, nh) if L == 16 else wide_fwd_route(total, L, nh)


def bwd_route(total, L, nh):
    return bwd16_route(total, L, nh) if L == 16 else wide_bwd_route(total, L, nh)


def partial_rows(total, L, nh):
    """tulip_window_attn_bwd_partial_rows: one row per workgroup of a head"""
    g = bwd_route(total, L, nh)[0]
    return g // 4 if L == 16 else g


def window_group(total, L, nh, fwd=False):
    """(partial row / group, sweep) of every window of the launch, as int64 [total]"""
    win = torch.arange(total)
    g = (fwd_route if fwd else bwd_route)(total, L, nh)[0]
    unit = win // (64 // L) if L != 16 else win
    grp, sweep = unit % g, unit // g
    return (grp // 4 if (L == 16 and not fwd) else grp), sweep


# ------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    name: str
    B: int
    nWy: int
    nWx: int
    win: tuple
    nh: int
    P: int
    shifted: bool
    variant: str                  # "plain" | "drop" | "fp8"
    fwd: tuple                    # the route the forward launch must take, written next to the shape
    bwd: tuple = None             # ... the backward launch; None: the case runs the forward only
    seed: int = 0

    @property
    def L(self):
        return self.win[0] * self.win[1]

    @property
    def H(self):
        return self.nWy * self.win[0]

    @property
    def W(self):
        return self.nWx * self.win[1]

    @property
    def C(self):
        return self.nh * self.P

    @property
    def total(self):
        return self.B * self.nWy * self.nWx

    @property
    def M(self):
        return self.total * self.L

    @property
    def sft(self):
        return (self.win[0] // 2, self.win[1] // 2) if self.shifted else (0, 0)

    @property
    def masked(self):
        """the `masked` argument of the launch"""
        return int(self.shifted) | (2 if self.variant == "fp8" else 0)

    @property
    def A(self):
        """q and k are A times a unit vector; the fp8 cases take an A that e4m3 changes (34 -> 32 and 38 -> 40, both ties)"""
        return {(16, False): 32.0, (16, True): 34.0, (32, False): 40.0, (32, True): 38.0}[(self.P, self.variant == "fp8")]

    @property
    def inst(self):
        return (self.L, self.P, self.variant)


def _c(name, B, grid, win, nh, P, shifted, variant, fwd, bwd=None, seed=0):
    return Case(name, B, grid[0], grid[1], win, nh, P, shifted, variant, fwd, bwd, seed)


N, Y = False, True
G33 = (3, 3)


def gpu_cases():
    """B x 3 x 3 windows with odd B: the total is odd and all nine mask labels occur in both axes.  Routes as
    (groups, sweeps, idle groups, short last sweep, invalid item in the last trip)."""
    out = [
        # ---- 16 tokens, one sweep; the backward deals 9 / 27 windows to 12 / 28 waves: idle groups
        _c("w2x8-p16-nh3", 1, G33, (2, 8), 3, 16, N, "plain", (9, 1, 0, N, N), (12, 1, 3, N, N)),
        _c("w2x8-p32-nh6-s", 3, G33, (2, 8), 6, 32, Y, "plain", (27, 1, 0, N, N), (28, 1, 1, N, N)),
        _c("w1x16-p16-nh12-s-drop", 1, G33, (1, 16), 12, 16, Y, "drop", (9, 1, 0, N, N), (12, 1, 3, N, N)),
        _c("w1x16-p32-nh3-drop", 1, G33, (1, 16), 3, 32, N, "drop", (9, 1, 0, N, N), (12, 1, 3, N, N)),
        _c("w2x8-p16-nh6-s-fp8", 1, G33, (2, 8), 6, 16, Y, "fp8", (9, 1, 0, N, N), (12, 1, 3, N, N)),
        _c("w2x8-p32-nh3-fp8", 3, G33, (2, 8), 3, 32, N, "fp8", (27, 1, 0, N, N), (28, 1, 1, N, N)),
        # ---- 16 tokens, 351 windows at 24 heads: 171 forward groups (171 + 171 + 9), 88 backward waves (3 x 88 + 87)
        _c("w2x8-p16-nh24-s-sweeps", 39, G33, (2, 8), 24, 16, Y, "plain", (171, 3, 0, Y, N), (88, 4, 0, Y, N)),
        _c("w1x16-p32-nh24-sweeps", 39, G33, (1, 16), 24, 32, N, "plain", (171, 3, 0, Y, N), (88, 4, 0, Y, N)),
        _c("w2x8-p16-nh24-drop-sweeps", 39, G33, (2, 8), 24, 16, N, "drop", (171, 3, 0, Y, N), (88, 4, 0, Y, N)),
        _c("w2x8-p32-nh24-s-drop-sweeps", 39, G33, (2, 8), 24, 32, Y, "drop", (171, 3, 0, Y, N), (88, 4, 0, Y, N)),
        _c("w1x16-p16-nh24-s-fp8-sweeps", 39, G33, (1, 16), 24, 16, Y, "fp8", (171, 3, 0, Y, N), (88, 4, 0, Y, N)),
        _c("w2x8-p32-nh24-s-fp8-sweeps", 39, G33, (2, 8), 24, 32, Y, "fp8", (171, 3, 0, Y, N), (88, 4, 0, Y, N)),
        # ---- 32 tokens, one sweep, an odd total: the second item of the last lane pair is invalid
        _c("w4x8-p16-nh3-s", 1, G33, (4, 8), 3, 16, Y, "plain", (5, 1, 0, N, Y), (5, 1, 0, N, Y)),
        _c("w2x16-p32-nh6", 1, G33, (2, 16), 6, 32, N, "plain", (5, 1, 0, N, Y), (5, 1, 0, N, Y)),
        _c("w1x32-p16-nh12-s-drop", 1, G33, (1, 32), 12, 16, Y, "drop", (5, 1, 0, N, Y), (5, 1, 0, N, Y)),
        _c("w4x8-p32-nh3-drop", 3, G33, (4, 8), 3, 32, N, "drop", (14, 1, 0, N, Y), (14, 1, 0, N, Y)),
        # ---- 32 tokens, forward sweeps: 135 windows = 68 pairs at 64 heads, 32 groups (32 + 32 + 4)
        _c("w4x8-p16-nh64-s-fsweeps", 15, G33, (4, 8), 64, 16, Y, "plain", (32, 3, 0, Y, Y)),
        _c("w2x16-p32-nh64-fsweeps", 15, G33, (2, 16), 64, 32, N, "plain", (32, 3, 0, Y, Y)),
        _c("w1x32-p16-nh64-drop-fsweeps", 15, G33, (1, 32), 64, 16, N, "drop", (32, 3, 0, Y, Y)),
        _c("w4x8-p32-nh64-s-drop-fsweeps", 15, G33, (4, 8), 64, 32, Y, "drop", (32, 3, 0, Y, Y)),
        # ---- 32 tokens, backward sweeps: 99 windows = 50 pairs at 24 heads, 21 groups (21 + 21 + 8)
        _c("w2x16-p16-nh24-s-bsweeps", 11, G33, (2, 16), 24, 16, Y, "plain", (50, 1, 0, N, Y), (21, 3, 0, Y, Y)),
        _c("w4x8-p32-nh24-bsweeps", 11, G33, (4, 8), 24, 32, N, "plain", (50, 1, 0, N, Y), (21, 3, 0, Y, Y)),
        _c("w4x8-p16-nh24-s-drop-bsweeps", 11, G33, (4, 8), 24, 16, Y, "drop", (50, 1, 0, N, Y), (21, 3, 0, Y, Y)),
        _c("w1x32-p32-nh24-s-drop-bsweeps", 11, G33, (1, 32), 24, 32, Y, "drop", (50, 1, 0, N, Y), (21, 3, 0, Y, Y)),
        # ---- 64 tokens, one sweep
        _c("w8x8-p16-nh3-s", 1, G33, (8, 8), 3, 16, Y, "plain", (9, 1, 0, N, N), (9, 1, 0, N, N)),
        _c("w4x16-p32-nh6", 1, G33, (4, 16), 6, 32, N, "plain", (9, 1, 0, N, N), (9, 1, 0, N, N)),
        _c("w2x32-p16-nh12-s-drop", 1, G33, (2, 32), 12, 16, Y, "drop", (9, 1, 0, N, N), (9, 1, 0, N, N)),
        _c("w1x64-p32-nh3-s-drop", 1, G33, (1, 64), 3, 32, Y, "drop", (9, 1, 0, N, N), (9, 1, 0, N, N)),
        # ---- 64 tokens, forward sweeps: 81 windows at 64 heads, 32 groups (32 + 32 + 17)
        _c("w8x8-p16-nh64-fsweeps", 9, G33, (8, 8), 64, 16, N, "plain", (32, 3, 0, Y, N)),
        _c("w4x16-p32-nh64-s-fsweeps", 9, G33, (4, 16), 64, 32, Y, "plain", (32, 3, 0, Y, N)),
        _c("w2x32-p16-nh64-s-drop-fsweeps", 9, G33, (2, 32), 64, 16, Y, "drop", (32, 3, 0, Y, N)),
        _c("w8x8-p32-nh64-drop-fsweeps", 9, G33, (8, 8), 64, 32, N, "drop", (32, 3, 0, Y, N)),
        # ---- 64 tokens, backward sweeps: 45 windows at 24 heads, 21 groups (21 + 21 + 3)
        _c("w8x8-p16-nh24-s-bsweeps", 5, G33, (8, 8), 24, 16, Y, "plain", (45, 1, 0, N, N), (21, 3, 0, Y, N)),
        _c("w1x64-p32-nh24-bsweeps", 5, G33, (1, 64), 24, 32, N, "plain", (45, 1, 0, N, N), (21, 3, 0, Y, N)),
        _c("w4x16-p16-nh24-drop-bsweeps", 5, G33, (4, 16), 24, 16, N, "drop", (45, 1, 0, N, N), (21, 3, 0, Y, N)),
        _c("w8x8-p32-nh24-s-drop-bsweeps", 5, G33, (8, 8), 24, 32, Y, "drop", (45, 1, 0, N, N), (21, 3, 0, Y, N)),
        # ---- one row of windows (H == wh), unshifted and shifted, and one column (W == ww)
        _c("w2x8-row-p16-nh3", 1, (1, 3), (2, 8), 3, 16, N, "plain", (3, 1, 0, N, N), (4, 1, 1, N, N)),
        _c("w4x8-row-p32-nh3-s", 3, (1, 3), (4, 8), 3, 32, Y, "plain", (5, 1, 0, N, Y), (5, 1, 0, N, Y)),
        _c("w8x8-col-p16-nh6-s", 1, (3, 1), (8, 8), 6, 16, Y, "plain", (3, 1, 0, N, N), (3, 1, 0, N, N)),
    ]
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def instantiations():
    """every kernel instantiation behind the four entry points: (L, P, variant)"""
    out = [(L, P, v) for L in (16, 32, 64) for P in (16, 32) for v in ("plain", "drop")]
    return out + [(16, P, "fp8") for P in (16, 32)]


def coverage_gaps(cases):
    """what section 4 of the case list's contract is missing, as strings (empty: complete)"""
    gaps = []
    for inst in instantiations():
        for direction in ("fwd", "bwd"):
            routes = [getattr(c, direction) for c in cases if c.inst == inst and getattr(c, direction) is not None]
            need = {"one sweep": any(r[1] == 1 for r in routes), ">= 3 sweeps, short last": any(r[1] >= 3 and r[3] for r in routes)}
            if inst[0] == 16 and direction == "bwd":
                need["idle groups"] = any(r[2] > 0 for r in routes)
            if inst[0] == 32:
                need["odd total"] = any(r[4] for r in routes)
            gaps += [f"{inst} {direction}: {k}" for k, ok in need.items() if not ok]
    shapes = {c.win for c in cases}
    for w in ((2, 8), (1, 16), (4, 8), (2, 16), (1, 32), (8, 8), (4, 16), (2, 32), (1, 64)):
        if w not in shapes:
            gaps.append(f"window {w}")
    for nh in (3, 6, 12, 24):
        if nh not in {c.nh for c in cases}:
            gaps.append(f"nh {nh}")
    if not any(c.nWy == 1 and not c.shifted for c in cases) or not any(c.nWy == 1 and c.shifted for c in cases):
        gaps.append("a single row of windows, unshifted and shifted")
    if not any(c.nWx == 1 for c in cases):
        gaps.append("a single column of windows")
    return gaps


# ------------------------------------------------------------------ geometry
def window_rows(c: Case, sft, device):
    """[total][L] natural token row of every window slot: rolled[hs] = x[(hs + sh) mod H]"""
    wh, ww = c.win
    b, wy, wx, i, j = torch.meshgrid(torch.arange(c.B), torch.arange(c.nWy), torch.arange(c.nWx), torch.arange(wh),
                                     torch.arange(ww), indexing="ij")
    h = (wy * wh + i + sft[0]) % c.H
    w = (wx * ww + j + sft[1]) % c.W
    return ((b * c.H + h) * c.W + w).reshape(c.total, c.L).to(device)


def window_labels(c: Case, sft, device, unrolled=False):
    """[nW][L] region label of every slot of a sample's windows (labels live on the ROLLED image; unrolled=True is the defect
    that takes them at the natural position)"""
    lab = ND.region_labels(c.H, c.W, c.win, sft).reshape(c.H * c.W, 1)
    if unrolled:
        lab = ND.to_windows(lab, 1, c.H, c.W, c.win, sft)
    else:
        lab = ND.to_windows(lab, 1, c.H, c.W, c.win, (0, 0))
    return lab.reshape(-1, c.L).to(device)


def mask_of(lab):
    """[nW][L][L]: 1 where query and key carry different labels"""
    return (lab[:, :, None] != lab[:, None, :]).to(F64)


def _fp8(t):
    return t.to(torch.float8_e4m3fn).to(t.dtype)


# ------------------------------------------------------------------ a problem
@dataclass
class Problem:
    case: Case
    qkv: Buf
    dout: Buf
    table: Buf
    rel: Buf
    mult: torch.Tensor            # [total][nh][L][L] float64 attn_drop multiplier, or None
    outs: dict                    # "out", and with a backward "dqkv", "part", "dtab": Out
    ref: dict
    stats: dict
    R: int = 0


def _windows_of(pb_or_flat, buf, rows, nh, P, parts):
    """[total][L] rows of a [M][parts nh P] buffer -> [parts][total][nh][L][P], fetched by address"""
    flat = pb_or_flat
    pos = buf.off + rows.reshape(-1)[:, None] * buf.pitch + torch.arange(parts * nh * P, device=flat.device)[None, :]
    t = flat[pos].reshape(rows.shape[0], rows.shape[1], parts, nh, P)
    return t.permute(2, 0, 3, 1, 4)


def _to_rows(t_w, rows, M):
    """[total][nh][L][P] -> [M][nh P] natural-order rows"""
    total, nh, L, P = t_w.shape
    out = torch.zeros(M, nh * P, dtype=t_w.dtype, device=t_w.device)
    out[rows.reshape(-1)] = t_w.permute(0, 2, 1, 3).reshape(total * L, nh * P)
    return out


def _chunks(c: Case):
    step = max(1, CHUNK // (c.nh * c.L * c.L))
    return [slice(a, min(c.total, a + step)) for a in range(0, c.total, step)]


def _levels(q, k, bias, mask, scale):
    """scores [t][nh][L][L] and, per row, the top level, the number of keys on it and the gap to the second level"""
    s = (q @ k.transpose(-1, -2)) * scale + bias[None]
    if mask is not None:
        s = s + mask[:, None] * -100.0
    top = s.amax(-1, keepdim=True)
    on_top = s >= top - GAP / 2
    n = on_top.sum(-1)
    second = torch.where(on_top, torch.full_like(s, -math.inf), s).amax(-1)
    return s, top.squeeze(-1), n, top.squeeze(-1) - second, on_top


def _draw_classes(gen, shape, weights):
    w = torch.tensor(weights, dtype=F64)
    return torch.multinomial(w, int(np.prod(shape)), replacement=True, generator=gen).reshape(shape)


def _onehot(cls, sub, A, P):
    """class ids [t][nh][L], channel subsets [t][nh][4] -> [t][nh][L][P] with A at the class's channel"""
    ch = torch.gather(sub, 2, cls)
    return torch.zeros(*cls.shape, P, dtype=F64).scatter_(3, ch[..., None], A)


def build(case: Case, device="cpu") -> Problem:
    c = case
    gen = torch.Generator().manual_seed(5000 + 17 * c.seed + 131 * c.L + 7 * c.nh + 3 * c.P + c.total + 977 * int(c.shifted)
                                        + 31 * len(c.variant))
    L, P, nh, total, M, C = c.L, c.P, c.nh, c.total, c.M, c.C
    nW = c.nWy * c.nWx
    scale = P ** -0.5
    fp8 = c.variant == "fp8"
    A_eff = float(_fp8(torch.tensor([c.A], dtype=F32))) if fp8 else c.A
    assert c.A == float(torch.tensor(c.A).to(BF16)) and c.A == int(c.A)
    assert (A_eff != c.A) == fp8, "the fp8 cases take an A that e4m3 changes"
    T = A_eff * A_eff * scale
    assert T_RANGE[0] <= T <= T_RANGE[1], T
    ntab = (2 * c.win[0] - 1) * (2 * c.win[1] - 1)
    rel = ND.rel_position_index(*c.win)
    lab = window_labels(c, c.sft, "cpu")
    mask = mask_of(lab) if c.shifted else None                                              # [nW][L][L]
    wloc = torch.arange(total) % nW
    bad_n = torch.tensor(sorted(BAD_N))
    # table: {0, -1000} per (entry, head), about UNBIASED_KEYS of the L keys of a row unbiased.  A query without a key of its class
    # has ALL its unbiased keys of one label on top, whatever the classes: a head's column is drawn until none of these counts
    # sits near a tie
    same = (1 - mask) if mask is not None else torch.ones(1, L, L, dtype=F64)
    table = torch.empty(ntab, nh, dtype=F64)
    for h in range(nh):
        for _ in range(100):
            cand = torch.rand(32, ntab, generator=gen) < min(0.5, UNBIASED_KEYS / L)
            unb = cand[:, rel.reshape(-1)].reshape(32, L, L).to(F64)
            counts = torch.stack([torch.einsum("cij,wij->cwi", unb, same), torch.einsum("cij,wij->cwi", unb, 1 - same)])
            ok = ~torch.isin(counts.to(torch.int64), bad_n).reshape(2, 32, -1).any(-1).any(0)
            if bool(ok.any()):
                table[:, h] = torch.where(cand[int(ok.nonzero()[0])], 0.0, BIAS_LOW)
                break
        else:
            raise AssertionError(f"{c.name}: no bias column for head {h}")
    bias = table[rel.reshape(-1)].reshape(L, L, nh).permute(2, 0, 1).contiguous()          # [nh][L][L]
    # classes: a 4-subset of the channels per (window, head); pairs with a row whose n sits too near a bf16 tie are drawn again
    sub = torch.rand(total, nh, P, generator=gen).argsort(-1)[..., :4]
    cq, ck = _draw_classes(gen, (total, nh, L), Q_WEIGHTS), _draw_classes(gen, (total, nh, L), K_WEIGHTS)
    todo = torch.arange(total * nh)
    for _ in range(200):
        if not todo.numel():
            break
        again = []
        step = max(1, CHUNK // (L * L))
        for a in range(0, todo.numel(), step):
            pr = todo[a:a + step]
            w, h = pr // nh, pr % nh
            q1 = torch.nn.functional.one_hot(cq[w, h], 4).to(F64) * A_eff
            k1 = torch.nn.functional.one_hot(ck[w, h], 4).to(F64) * A_eff
            s = (q1 @ k1.transpose(-1, -2)) * scale + bias[h]
            if mask is not None:
                s = s + mask[wloc[w]] * -100.0
            n = (s >= s.amax(-1, keepdim=True) - GAP / 2).sum(-1)
            again.append(pr[torch.isin(n, bad_n).any(-1)])
        todo = torch.cat(again)
        if not todo.numel():
            break
        w, h = todo // nh, todo % nh
        cq[w, h] = _draw_classes(gen, (todo.numel(), L), Q_WEIGHTS)
        ck[w, h] = _draw_classes(gen, (todo.numel(), L), K_WEIGHTS)
    assert not todo.numel(), f"{c.name}: {todo.numel()} (window, head) pairs keep a row with n in {sorted(BAD_N)}"
    q_w, k_w = _onehot(cq, sub, c.A, P), _onehot(ck, sub, c.A, P)
    v_w = torch.randint(-4, 5, (total, nh, L, P), generator=gen).to(F64)
    do_w = torch.randint(-2, 3, (total, nh, L, P), generator=gen).to(F64)
    # the channels in which a gradient can be non-zero at all: dq = dS.K lives in the channels of the pair's keys, dk in its queries'
    used = {"dq": (k_w != 0).any(2), "dk": (q_w != 0).any(2)}
    mult = None
    if c.variant == "drop":
        mult = torch.from_numpy(D.multiplier(DROP_SEED, DROP_COUNTER, DROP_SITE, DROP_P, D.attn_index(c.B, c.H, c.W, nh, c.win))
                                .astype(np.float64))
        assert set(mult.unique().tolist()) == {0.0, 2.0}
    rows = window_rows(c, c.sft, "cpu")
    qkv_nat = torch.cat([_to_rows(t, rows, M) for t in (q_w, k_w, v_w)], 1)
    dev = device
    qkv = Buf(M, 3 * C, 3 * C, BF16, "nan", dev).set(qkv_nat.to(dev))
    dout = Buf(M, C, C, BF16, "nan", dev).set(_to_rows(do_w, rows, M).to(dev))
    tab = Buf(ntab, nh, nh, F32, "nan", dev).set(table.to(dev))
    relb = Buf(L, L, L, torch.int32, REL_GUARD, dev).set(rel.to(dev))
    if fp8:                      # the reference takes q and k as the scores see them, in the products with dS too
        q_w, k_w = _fp8(q_w.to(F32)).to(F64), _fp8(k_w.to(F32)).to(F64)
    mv = lambda t: None if t is None else t.to(dev)
    q_w, k_w, v_w, do_w, bias, mask, mult, rows = (mv(t) for t in (q_w, k_w, v_w, do_w, bias, mask, mult, rows))
    used = {k: t.to(dev) for k, t in used.items()}
    wloc = wloc.to(dev)
    # ---- the float64 reference, in chunks of windows
    has_bwd = c.bwd is not None
    R = partial_rows(total, L, nh) if has_bwd else 0
    out_w = torch.empty(total, nh, L, P, dtype=F64, device=dev)
    n_seen, min_gap, masked_top, vmax = set(), math.inf, False, float(v_w.abs().max())
    if has_bwd:
        iv = {k: torch.empty(total, nh, L, P, dtype=F64, device=dev) for k in ("dv", "dq_lo", "dq_hi", "dq_r", "dq_u", "dk_lo", "dk_hi",
                                                                              "dk_r", "dk_u")}
        dense = torch.zeros(nh, L, L, dtype=F64, device=dev)
        dense_u, dense_abs = torch.zeros_like(dense), torch.zeros_like(dense)
    for sl in _chunks(c):
        q, k, v, do = q_w[sl], k_w[sl], v_w[sl], do_w[sl]
        m = mask[wloc[sl]] if mask is not None else None
        s, top, n, gap, on_top = _levels(q, k, bias, m, scale)
        n_seen |= set(n.unique().tolist())
        min_gap = min(min_gap, float(gap.min()))
        if m is not None:
            masked_top = masked_top or bool((on_top & (m[:, None] > 0)).any())
        p = torch.softmax(s, -1)
        assert bool(((p - 1.0 / n[..., None].to(F64)).abs()[on_top] < 1e-12).all()) and float(torch.where(on_top, torch.zeros_like(p), p).max()) < 1e-43
        pm = p if mult is None else p * mult[sl]
        pb = ND.round_bf16(pm).to(F64)
        assert bool((pb[~on_top] == 0).all())                                   # (iii) the stray mass rounds away
        out_w[sl] = pb @ v
        if not has_bwd:
            continue
        iv["dv"][sl] = pb.transpose(-1, -2) @ do
        eps = ND.attn_p_eps(torch.logsumexp(s, -1))[..., None]
        dP = do @ v.transpose(-1, -2)
        if mult is not None:
            dP = dP * mult[sl]
        Dsum = (p * dP.abs()).sum(-1, keepdim=True)
        dS = p * (dP - (p * dP).sum(-1, keepdim=True))
        # a p below the fp32 normal range may reach the kernel's arithmetic as 0, or as a subnormal, on whose grid of 2^-149 the
        # errors are absolute, not relative: two steps for p (the relative error of exp is far below a step at e^-100, what is left
        # is a rounding to the grid that need not be the nearest) and one for the rounding of the product.  Its share of delta is
        # uncertain in the same way, for every key of the row.
        stray = p < 2.0 ** -126
        grid = 2 * 2.0 ** -149 * dP.abs()
        d_stray = (torch.where(stray, p * dP.abs() + grid, torch.zeros_like(p))).sum(-1, keepdim=True)
        u = eps * p * (dP.abs() + Dsum) + p * d_stray
        us = u + grid + Dsum * 2 * 2.0 ** -149 + 2.0 ** -149
        lo = torch.where(stray, torch.minimum(dS - us, torch.zeros_like(dS)), dS - u)
        hi = torch.where(stray, torch.maximum(dS + us, torch.zeros_like(dS)), dS + u)
        dense += ((lo + hi) / 2).sum(0)                                         # (the centre of a stray's hull of 0 and the value)
        dense_u += ((hi - lo) / 2).sum(0)
        dense_abs += torch.maximum(lo.abs(), hi.abs()).sum(0)
        if L == 16:                                                             # the dS operand of the MFMA is bf16
            lo, hi = ND.round_bf16(lo).to(F64), ND.round_bf16(hi).to(F64)
        amax = torch.maximum(lo.abs(), hi.abs())
        for name, a_lo, a_hi, a_abs, opnd in (("dq", lo, hi, amax, k), ("dk", lo.transpose(-1, -2), hi.transpose(-1, -2),
                                                                        amax.transpose(-1, -2), q)):
            # opnd >= 0: the bounds go through the product as they are; + the fp32 roundings of L additions, of `scale` (1 / sqrt(32)
            # is not an fp32 number) and of the product with it
            slack = (L + 2) * 2.0 ** -24 * (a_abs @ opnd) * scale
            r_lo, r_hi = (a_lo @ opnd) * scale - slack, (a_hi @ opnd) * scale + slack
            iv[name + "_lo"][sl], iv[name + "_hi"][sl] = ND.round_bf16(r_lo).to(F64), ND.round_bf16(r_hi).to(F64)
            iv[name + "_r"][sl], iv[name + "_u"][sl] = (r_lo + r_hi) / 2, (r_hi - r_lo) / 2
    # ---- conditions on the data, from the reference alone
    assert min_gap >= GAP - GAP_SLACK, (c.name, min_gap)                                    # (i)
    assert not (n_seen & BAD_N), (c.name, sorted(n_seen & BAD_N))                            # (ii)
    assert L * math.exp(-GAP) * vmax * (2 if mult is not None else 1) < 2.0 ** -134, c.name                                   # (iii)
    pow2 = {x for x in n_seen if x > 1 and x & (x - 1) == 0}
    assert 1 in n_seen and pow2 and (n_seen - pow2 - {1}), (c.name, sorted(n_seen))          # (iv)
    assert masked_top or not c.shifted, f"{c.name}: no row has its top level on masked keys"
    stats = {"n": sorted(n_seen), "T": T, "gap": min_gap, "out_nonzero": float((ND.round_bf16(out_w) != 0).to(F64).mean())}
    # ---- outputs inside guard words, and their expected images
    o = Buf(M, C, C, BF16, "guard", dev)
    outs = {"out": Out(o, _canon(GX._image(o, o.index(), _to_rows(out_w, rows, M))), o.index())}
    ref = {"rows": rows, "used": used}
    if has_bwd:
        g = Buf(M, 3 * C, 3 * C, BF16, "guard", dev)
        nat = {k: _to_rows(t, rows, M) for k, t in iv.items()}
        exact = torch.cat([torch.zeros(M, 2 * C, dtype=F64, device=dev), nat["dv"]], 1)
        loose = torch.zeros(M, 3 * C, dtype=torch.bool, device=dev)
        loose[:, :2 * C] = True
        outs["dqkv"] = Out(g, _canon(GX._image(g, g.index(), exact, loose)), g.index(), loose)
        for name in ("dq", "dk"):
            used_nat = _to_rows(used[name][:, :, None, :].expand(total, nh, L, P).to(F64), rows, M) > 0
            lo_, hi_ = nat[name + "_lo"], nat[name + "_hi"]
            det = lo_ == hi_
            share = float(det.to(F64).mean())
            nz = float((lo_[det & used_nat] != 0).to(F64).mean())
            stats[name + "_determined"], stats[name + "_nonzero"] = share, nz
            assert share >= MIN_DETERMINED, f"{c.name}: only {share:.4f} of the {name} words are determined"
            assert nz >= MIN_NONZERO, f"{c.name}: only {nz:.4f} of the determined {name} words in the used channels are non-zero"
            ref[name] = (lo_, hi_, nat[name + "_r"], nat[name + "_u"])
        big = float(dense.abs().max())
        stats["dbias_u"] = float(dense_u.max()) / big
        assert stats["dbias_u"] < DBIAS_U, f"{c.name}: a d(bias) entry has u = {stats['dbias_u']:.3e} of the largest entry"
        budget = dense_u + R * ND.ulp_f32(dense_abs)
        part = Buf(R, nh * L * L, nh * L * L, F32, "guard", dev)
        every = torch.ones(R, nh * L * L, dtype=torch.bool, device=dev)
        outs["part"] = Out(part, GX._image(part, part.index(), torch.zeros(R, nh * L * L, dtype=F64, device=dev), every), part.index(), every)
        # the production fold: dense sums ADDED into table[rel[i][j]][h]
        dt = Buf(ntab, nh, nh, F32, "guard", dev).set(torch.zeros(ntab, nh, dtype=F64, device=dev))
        every_t = torch.ones(ntab, nh, dtype=torch.bool, device=dev)
        outs["dtab"] = Out(dt, GX._image(dt, dt.index(), torch.zeros(ntab, nh, dtype=F64, device=dev), every_t), dt.index(), every_t)
        relf = rel.reshape(-1).to(dev)
        fold = lambda x: torch.zeros(ntab, nh, dtype=F64, device=dev).index_add_(0, relf, x.reshape(nh, L * L).t().contiguous())
        npairs = torch.zeros(ntab, dtype=F64, device=dev).index_add_(0, relf, torch.ones(L * L, dtype=F64, device=dev))
        ref.update(dense=dense, dense_budget=budget, dtab=fold(dense),
                   dtab_budget=fold(budget) + npairs[:, None] * ND.ulp_f32(fold(dense_abs)))
    return Problem(c, qkv, dout, tab, relb, mult, outs, ref, stats, R)


# ------------------------------------------------------------------ checkers
def _canon(bits):
    """bit image with -0 mapped to +0 (the two count as equal)"""
    zero = 0x7FFF if bits.dtype == torch.int16 else 0x7FFFFFFF
    return torch.where((bits & zero) == 0, torch.zeros_like(bits), bits)


def _checked(name, out: Out, got_flat) -> Report:
    """check_out on the whole allocation: exact words bit for bit (-0 == +0), guard words included"""
    return check_out(name, out, _canon(GX._ibits(got_flat.contiguous())))


def check_interval(name, out: Out, got_flat, col0, ref) -> Report:
    """dq / dk: every word inside [bf16(r - u), bf16(r + u)]; worst = |got - r| / (u + 1/2 ulp_bf16(r))"""
    lo, hi, r, u = ref
    rep = Report(name)
    M, C = lo.shape
    g = got_flat[out.idx[:, col0:col0 + C].reshape(-1)].to(F64).reshape(M, C)
    fin = torch.isfinite(g)
    err = torch.where(fin, (g - r).abs(), torch.full_like(r, math.inf))
    elem = torch.arange(M * C, device=g.device).reshape(M, C)
    ND._ratio(rep, err.reshape(-1), (u + 0.5 * ND.ulp_bf16(r)).reshape(-1), elem.reshape(-1))
    if rep.where:
        e = int(rep.where)
        rep.where = f"row {e // C}, column {e % C}"
    bad = ~fin | (g < lo) | (g > hi)
    if bool(bad.any()):
        e = int(bad.reshape(-1).nonzero()[0])
        rep.violations.append(f"{int(bad.sum())} words outside their interval; first: row {e // C}, column {e % C} holds "
                              f"{float(g.reshape(-1)[e])!r}, interval [{float(lo.reshape(-1)[e])!r}, {float(hi.reshape(-1)[e])!r}]")
    return rep


def check_budget(name, got64, ref64, budget) -> Report:
    rep = Report(name)
    err = torch.where(torch.isfinite(got64), (got64 - ref64).abs(), torch.full_like(ref64, math.inf))
    elem = torch.arange(ref64.numel(), device=ref64.device)
    r = ND._ratio(rep, err.reshape(-1), budget.reshape(-1), elem)
    ND._add(rep, r > 1, "entries above their budget", elem)
    return rep


def check_fwd(pb: Problem, got: dict) -> list:
    return [_checked(f"{pb.case.name}.out", pb.outs["out"], got["out"])]


def check_bwd(pb: Problem, got: dict) -> list:
    c, name = pb.case, pb.case.name
    reps = [_checked(f"{name}.dqkv (dV and guard words)", pb.outs["dqkv"], got["dqkv"]),
            check_interval(f"{name}.dq", pb.outs["dqkv"], got["dqkv"], 0, pb.ref["dq"]),
            check_interval(f"{name}.dk", pb.outs["dqkv"], got["dqkv"], c.C, pb.ref["dk"]),
            _checked(f"{name}.partial rows (guard words)", pb.outs["part"], got["part"]),
            _checked(f"{name}.table gradient (guard words)", pb.outs["dtab"], got["dtab"])]
    part = pb.outs["part"]
    rows = got["part"][part.idx.reshape(-1)]
    rep = Report(f"{name}.partial rows written")
    left = GX._ibits(rows.contiguous()) == GX.GUARD32
    if bool(left.any()):
        e = int(left.nonzero()[0])
        per = c.nh * c.L * c.L
        rep.violations.append(f"{int(left.sum())} words of the {pb.R} partial rows still hold the fill pattern; first: row {e // per}, "
                              f"head {e % per // (c.L * c.L)}, entry {e % (c.L * c.L)}")
    reps.append(rep)
    dense = rows.to(F64).reshape(pb.R, c.nh, c.L, c.L).sum(0)
    reps.append(check_budget(f"{name}.d(bias), partial rows folded in float64", dense, pb.ref["dense"], pb.ref["dense_budget"]))
    dt = pb.outs["dtab"]
    reps.append(check_budget(f"{name}.d(bias table), the production fold", got["dtab"][dt.idx.reshape(-1)].to(F64).reshape(dt.idx.shape),
                             pb.ref["dtab"], pb.ref["dtab_budget"]))
    return reps


def check(pb: Problem, got: dict) -> list:
    return check_fwd(pb, got) + (check_bwd(pb, got) if pb.case.bwd is not None else [])


def failures(reps):
    return [str(r) for r in reps if not r.ok]


def fresh(pb: Problem) -> dict:
    """fresh copies of the output allocations of a launch"""
    return {k: o.buf.flat.clone() for k, o in pb.outs.items()}


# ------------------------------------------------------------------ a torch emulation of the launches, with switchable defects
DEFECTS = ("shift_plus", "no_reverse_shift", "labels_unrolled", "mask_unshifted", "rel_transposed", "table_head_stride1",
           "head_slice_off", "p_unrounded", "dv_undropped", "dp_unmasked", "delta_omitted", "dk_unscaled", "fp8_q_only",
           "dbias_last_sweep_missing", "idle_rows_unwritten", "odd_item_on_window0", "row_past_end")


def emulate(pb: Problem, defect=None) -> dict:
    """What correct kernels leave in the output allocations: the documented function in float32 with the kernels' rounding points
    (p to bf16 ahead of P.V and of dV, dS to bf16 ahead of the 16-token MFMAs, one rounding of every stored word), operands fetched
    and results stored by ADDRESS, the partial rows dealt as the launchers deal them -- so `defect` can name a wrong address as well
    as wrong arithmetic."""
    c = pb.case
    assert defect is None or defect in DEFECTS
    dev = pb.qkv.flat.device
    L, P, nh, total, M, C = c.L, c.P, c.nh, c.total, c.M, c.C
    nW = c.nWy * c.nWx
    scale = torch.tensor(P ** -0.5, dtype=F32)
    sft_in = (-c.sft[0], -c.sft[1]) if defect == "shift_plus" else c.sft
    rows_in = window_rows(c, sft_in, dev)
    rows_out = window_rows(c, (0, 0), dev) if defect == "no_reverse_shift" else rows_in
    q, k, v = (t.to(F32) for t in _windows_of(pb.qkv.flat, pb.qkv, rows_in, nh, P, 3))
    do = _windows_of(pb.dout.flat, pb.dout, rows_in, nh, P, 1)[0].to(F32)
    if c.variant == "fp8":
        q = _fp8(q)
        k = k if defect == "fp8_q_only" else _fp8(k)
    if defect == "head_slice_off":
        k = k.roll(-1, 1)
    rel = pb.rel.view.long()
    if defect == "rel_transposed":
        rel = rel.t()
    ntab = pb.table.rows
    hh = torch.arange(nh, device=dev)[:, None, None]
    pos = hh * ntab + rel[None] if defect == "table_head_stride1" else rel[None] * nh + hh
    bias = pb.table.flat[pb.table.off + pos]                                    # [nh][L][L]
    mask = None
    if c.shifted or defect == "mask_unshifted":
        msft = c.sft if c.shifted else (c.win[0] // 2, c.win[1] // 2)
        mask = mask_of(window_labels(c, msft, dev, unrolled=defect == "labels_unrolled")).to(F32)
    wloc = torch.arange(total, device=dev) % nW
    got = fresh(pb)
    has_bwd = c.bwd is not None
    out_w = torch.empty(total, nh, L, P, dtype=BF16, device=dev)
    if has_bwd:
        dq_w, dk_w, dv_w = (torch.empty(total, nh, L, P, dtype=BF16, device=dev) for _ in range(3))
        grp, sweep = (t.to(dev) for t in window_group(total, L, nh))
        last = c.bwd[1] - 1
        part = torch.zeros(pb.R, nh, L, L, dtype=F32, device=dev)
    for sl in _chunks(c):
        s = (q[sl] @ k[sl].transpose(-1, -2)) * scale + bias[None]
        if mask is not None:
            s = s + mask[wloc[sl]][:, None] * -100.0
        mx = s.amax(-1, keepdim=True)
        e = torch.exp(s - mx)
        ssum = e.sum(-1, keepdim=True)
        mu = pb.mult[sl].to(F32) if pb.mult is not None else None
        pf = (e if mu is None else e * mu) * (1.0 / ssum)
        pf = pf if defect == "p_unrounded" else pf.to(BF16).to(F32)
        out_w[sl] = (pf @ v[sl]).to(BF16)
        if not has_bwd:
            continue
        p = torch.exp(s - (mx + torch.log(ssum)))
        dP = do[sl] @ v[sl].transpose(-1, -2)
        if mu is not None and defect != "dp_unmasked":
            dP = dP * mu
        delta = torch.zeros_like(mx) if defect == "delta_omitted" else (p * dP).sum(-1, keepdim=True)
        dS = p * (dP - delta)
        pm = p if (mu is None or defect == "dv_undropped") else p * mu
        dv_w[sl] = (pm.to(BF16).to(F32).transpose(-1, -2) @ do[sl]).to(BF16)
        dsr = dS.to(BF16).to(F32) if L == 16 else dS
        dq_w[sl] = ((dsr @ k[sl]) * scale).to(BF16)
        dk = dsr.transpose(-1, -2) @ q[sl]
        dk_w[sl] = (dk if defect == "dk_unscaled" else dk * scale).to(BF16)
        keep = torch.ones(dS.shape[0], dtype=torch.bool, device=dev)
        if defect == "dbias_last_sweep_missing":
            keep = sweep[sl] != last
        part.index_add_(0, grp[sl][keep], dS[keep])

    def store(name, t_w, col0, width):
        o = pb.outs[name].buf
        idx = o.off + rows_out.reshape(-1)[:, None] * o.pitch + col0 + torch.arange(C, device=dev)[None, :]
        got[name][idx.reshape(-1)] = t_w.permute(0, 2, 1, 3).reshape(-1)

    targets = [("out", out_w, 0)] + ([("dqkv", dq_w, 0), ("dqkv", dk_w, C), ("dqkv", dv_w, 2 * C)] if has_bwd else [])
    for name, t_w, col0 in targets:
        if defect == "odd_item_on_window0" and L == 32 and total % 2 == 1:
            t_w = t_w.clone()
            t_w[0] = 0          # the invalid second item of the last trip (zero registers) lands on window 0
        store(name, t_w, col0, C)
    if defect == "row_past_end":
        for name in {t[0] for t in targets}:
            o = pb.outs[name].buf
            got[name][o.off + M * o.pitch: o.off + M * o.pitch + o.cols] = 0
    if has_bwd:
        flat = part.reshape(pb.R, -1)
        if defect == "idle_rows_unwritten" and L == 16:
            # a wave without a window returns before the workgroup's store: its 64 threads leave their 64 words of the row
            ngrp = c.bwd[0]
            guard = GX.filled(1, F32, "guard", dev)
            for wave in range(total, ngrp):
                flat.reshape(pb.R, nh, L * L)[wave // 4, :, 64 * (wave % 4):64 * (wave % 4) + 64] = guard
        pt = pb.outs["part"].buf
        got["part"][pt.off:pt.off + flat.numel()] = flat.reshape(-1)
        dt = pb.outs["dtab"].buf
        dense = got["part"][pt.off:pt.off + flat.numel()].reshape(pb.R, nh, L * L).sum(0)
        tab = torch.zeros(ntab, nh, dtype=F32, device=dev).index_add_(0, pb.rel.view.long().reshape(-1), dense.t().contiguous())
        got["dtab"][dt.off:dt.off + ntab * nh] = (got["dtab"][dt.off:dt.off + ntab * nh].reshape(ntab, nh) + tab).reshape(-1)
    return got

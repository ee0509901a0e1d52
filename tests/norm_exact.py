"""Exact tests of csrc/norm.hip (tulip_patch_embed_fwd / _bwd, tulip_layernorm_fwd / _bwd / _bwd_splitk / _bwd_params,
tulip_splitk_resid_ln): case lists with the launcher route each case must reach, integer operand builders, float64 references,
checkers and a torch emulation with switchable defects (test_norm_exact_cpu.py proves the checkers sharp and the lists
route-complete, test_norm_exact_gpu.py applies them to the kernels).  Plain torch on whichever device the caller names; no kernel
code.  Allocation kit: tests/gemm_exact.py; number formats and the torch-float32 baseline: tests/numerics_domain.py; the exact
LayerNorm rows: tests/glue_exact.py's construction.

Everything in front of the LayerNorm statistics is exact: images, conv weights, biases, slabs, residuals and incoming gradients are
small integers (sum |w x| + |b| < 2^20, asserted), so a conv accumulator, a slab fold and a residual sum are exactly known in any
order.  LayerNorm rows hold C/4 each of +1, -1, +m, -m (m in {1, 5, 11}, eps = 3: rstd 1/2, 1/4, 1/8) plus, on odd rows, a non-zero
integer offset; gamma is odd, beta an integer, so y is a non-zero multiple of 1/8 that bf16 holds exactly and 16 fp32 ulp of its
terms (plus the error of a mean that is an integer times a rounded 1/C) stay below half a bf16 ulp: bf16(y) cannot move.  In the
backward mean and rstd are operands, so xhat is exact and d(gamma), d(beta) and every partial row are exact sums.

Bit for bit: every guard word, padding column and row behind an output, out_bf16 / dx_bf16 (the one rounding of the fp32 value the
kernel itself stored, times its scale), y, mean of the offset-free rows, d(beta), and on the LayerNorm family d(gamma) and the
partial rows.  Within a budget from the reference alone: out, rstd, dx, the patch embedding's d(w), d(b), d(gamma) -- FACTOR x the
largest error torch float32 has on the same operands against float64, at least one fp32 ulp of the output's largest magnitude,
plus for sums over tokens the any-order summation bound (n - 1) 2^-24 sum |term| over the at most 64 tokens of non-zero dout (plus, in the atomic form,
the initial gradient as one more term)."""
import itertools
import math
from dataclasses import dataclass

import torch
import torch.nn.functional as Fn

from tests import gemm_exact as GX
from tests import glue_exact as GL
from tests import numerics_domain as ND
from tests.numerics_domain import Report

F64, F32, BF16 = GX.F64, GX.F32, GX.BF16
Buf, Out = GX.Buf, GX.Out
LN_EPS = GL.LN_EPS
FACTOR = 4.0
# output -> a factor of its own (DESIGN.md names the reason and the measured ratio for each).  "fold_vs_atomic" multiplies the whole
# per-output budget of the one comparison of two kernel results with each other: each lies within 1 x its budget of the same
# reference, in a summation order of its own, and the atomic form's add onto the non-zero initial gradient rounds at the magnitude
# of initial + gradient, which the partial form's budget does not hold.  Measured on the MI355X: 1.199 x at most (d(b), one token)
FACTORS = {"fold_vs_atomic": 2.0}
U32 = 2.0 ** -24
SCALES = (0.0, 0.25, 0.5, 1.0, 2.0)
NSLABS = (1, 3, 4, 5, 9)
MAX_NZ = 64
failures = GX.failures


# ------------------------------------------------------------------ routes: the launchers' documented rules
def embed_fwd_route(Cin, p0, kw, taps):
    if 1 <= Cin <= 4 and p0 == 1 and kw in (4, 8):
        return ("row", kw, Cin)
    return ("generic", taps <= 16)


def embed_bwd_route(E, taps, partial):
    lane = taps <= 32 and E in (48, 96)
    if partial and taps > 16 and not lane:
        return "refused"
    if partial and lane:
        return ("lane16", E // 16, 8 if taps <= 8 else 16 if taps <= 16 else 24 if taps <= 24 else 32)
    return ("generic", taps <= 16, "partial" if partial else "atomic")


def embed_bwd_blocks(ntok):
    return max(1, min((ntok + 3) // 4, 512))


def ln_route(C):
    nch = C // 4
    for n in (3, 6, 12):
        if nch == 64 * n:
            return (64, n, True)
    for lpr, n in ((16, 2), (16, 4), (64, 2), (64, 4), (64, 8), (64, 24)):
        if nch <= lpr * n:
            return (lpr, n, nch == lpr * n)
    return None


def ln_rpb(C):
    return 256 // ln_route(C)[0]


def ln_partial_rows(rows, C):
    nch = C // 4
    if rows <= 0 or nch > 512:
        return 0
    rpb = 16 if nch <= 64 else 4
    return max(1, min((rows + rpb - 1) // rpb, 512))


def ln_params_grid(rows, C):
    nch = C // 4
    tpr = 4
    while (1 << tpr) < nch and tpr < 6:
        tpr += 1
    gx = (nch + (1 << tpr) - 1) >> tpr
    rl = 256 >> tpr
    gy = 1 if rows <= 2048 else max(1, min((rows + rl * 4 - 1) // (rl * 4), 2048 // gx))
    rpb = (rows + gy - 1) // gy
    return tpr, gx, (rows + rpb - 1) // rpb, rpb


def splitk_ln_nch(N):
    return N // 256 if N > 0 and N % 256 == 0 and N // 256 in (1, 2, 3, 4, 6, 8) else None


# ------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Embed:
    B: int
    Cin: int
    Hin: int
    Win: int
    E: int
    p0: int
    p1: int
    kw: int
    circ: int
    route: object                 # what the launch must reach: embed_fwd_route's / embed_bwd_route's answer
    form: str = ""                # backward: "partial" | "atomic"
    what: str = ""
    bias0: int = 0                # added to every conv bias: a mean far above the spread (a one-pass variance cancels)

    def __post_init__(self):
        if not self.form and self.route[0] == "generic" and len(self.route) == 3:
            object.__setattr__(self, "form", self.route[2])

    Ho = property(lambda s: s.Hin // s.p0)
    Wo = property(lambda s: s.Win // s.p1)
    ntok = property(lambda s: s.B * s.Ho * s.Wo)
    taps = property(lambda s: s.Cin * s.p0 * s.kw)

    @property
    def name(self):
        return (f"e{self.E}-{self.B}x{self.Cin}x{self.Hin}x{self.Win}-p{self.p0}x{self.p1}k{self.kw}{'c' if self.circ else ''}"
                + (f"-b{self.bias0}" if self.bias0 else "") + (f"-{self.form}" if self.form else ""))


EMBED_FWD = [
    # the eight row instantiations: B = 2, Hin = 3, E = 96
    Embed(2, 1, 3, 20, 96, 1, 4, 4, 0, ("row", 4, 1)), Embed(2, 2, 3, 20, 96, 1, 4, 4, 0, ("row", 4, 2)),
    Embed(2, 3, 3, 20, 96, 1, 4, 4, 0, ("row", 4, 3)), Embed(2, 4, 3, 20, 96, 1, 4, 4, 0, ("row", 4, 4)),
    Embed(2, 1, 3, 20, 96, 1, 4, 8, 1, ("row", 8, 1)), Embed(2, 2, 3, 20, 96, 1, 4, 8, 1, ("row", 8, 2)),
    Embed(2, 3, 3, 20, 96, 1, 4, 8, 1, ("row", 8, 3)), Embed(2, 4, 3, 20, 96, 1, 4, 8, 1, ("row", 8, 4)),
    Embed(2, 1, 3, 24, 96, 1, 8, 8, 0, ("row", 8, 1), what="p1 = 8"), Embed(2, 2, 3, 24, 96, 1, 8, 8, 1, ("row", 8, 2), what="p1 = 8, circular"),
    # widths: one channel, the lower half only, the upper half all / all but one masked, both halves full
    Embed(2, 1, 3, 20, 1, 1, 4, 8, 1, ("row", 8, 1)), Embed(2, 1, 3, 20, 48, 1, 4, 8, 1, ("row", 8, 1)),
    Embed(2, 1, 3, 20, 64, 1, 4, 8, 1, ("row", 8, 1)), Embed(2, 1, 3, 20, 65, 1, 4, 8, 1, ("row", 8, 1)),
    Embed(2, 1, 3, 20, 128, 1, 4, 8, 1, ("row", 8, 1)),
    Embed(2, 1, 3, 20, 96, 1, 4, 8, 1, ("row", 8, 1), bias0=1024), Embed(2, 1, 4, 20, 96, 2, 4, 4, 0, ("generic", True), bias0=1024),
    # one-token-wide grids (every tap wraps), Hin = 1, token counts around the 4-token group
    Embed(2, 1, 3, 4, 96, 1, 4, 8, 1, ("row", 8, 1), what="Wo = 1"), Embed(2, 1, 3, 8, 96, 1, 8, 8, 1, ("row", 8, 1), what="Wo = 1, p1 = 8"),
    Embed(2, 1, 1, 20, 96, 1, 4, 8, 1, ("row", 8, 1), what="Hin = 1"),
    Embed(1, 1, 1, 4, 96, 1, 4, 4, 0, ("row", 4, 1), what="1 token"), Embed(1, 1, 3, 4, 96, 1, 4, 4, 0, ("row", 4, 1), what="3 tokens"),
    Embed(1, 1, 1, 20, 96, 1, 4, 8, 1, ("row", 8, 1), what="5 tokens"), Embed(2, 1, 2, 16, 96, 1, 4, 4, 0, ("row", 4, 1), what="16 tokens"),
    Embed(1, 1, 1, 68, 96, 1, 4, 8, 1, ("row", 8, 1), what="17 tokens"),
    # the second grid pass: 8193 tokens
    Embed(3, 1, 1, 10924, 96, 1, 4, 8, 1, ("row", 8, 1), what="8193 tokens"),
    Embed(3, 1, 2, 10924, 96, 2, 4, 4, 0, ("generic", True), what="8193 tokens"),
    # generic, taps in registers
    Embed(2, 1, 4, 24, 96, 2, 8, 8, 0, ("generic", True)), Embed(2, 1, 8, 20, 96, 4, 4, 4, 0, ("generic", True)),
    Embed(2, 1, 4, 20, 96, 2, 4, 8, 1, ("generic", True)), Embed(2, 1, 6, 20, 96, 3, 4, 4, 0, ("generic", True)),
    Embed(2, 3, 4, 10, 96, 2, 2, 2, 0, ("generic", True)), Embed(2, 1, 3, 48, 96, 1, 16, 16, 0, ("generic", True)),
    Embed(2, 1, 4, 20, 65, 2, 4, 4, 0, ("generic", True), what="E = 65"), Embed(1, 1, 2, 4, 128, 2, 4, 4, 0, ("generic", True), what="1 token"),
    # generic, tap loop
    Embed(2, 1, 8, 20, 96, 4, 4, 8, 1, ("generic", False)), Embed(2, 2, 4, 24, 96, 2, 8, 8, 0, ("generic", False)),
    Embed(2, 5, 3, 20, 96, 1, 4, 4, 0, ("generic", False)), Embed(2, 3, 4, 24, 96, 2, 8, 8, 1, ("generic", False)),
    Embed(2, 5, 3, 20, 128, 1, 4, 4, 0, ("generic", False), what="E = 128"),
]
BF16_VARIANTS = ("absent", "ld_e", "ld_2e")              # out_bf16: not given / its own [ntok][E] / the second half of a [ntok][2E] concat row

# taps -> (Cin, kw, circular) at p0 = 1, p1 = 4: every TAPS class of the 16-lane backward with taps == TAPS and taps < TAPS
_LANE_TAPS = {4: (1, 4, 0), 8: (1, 8, 1), 12: (3, 4, 0), 16: (2, 8, 1), 20: (5, 4, 0), 24: (3, 8, 1), 28: (7, 4, 0), 32: (4, 8, 1)}
EMBED_BWD = [Embed(2, ci, 3, 20, E, 1, 4, kw, circ, ("lane16", E // 16, (t + 7) // 8 * 8), "partial")
             for E in (48, 96) for t, (ci, kw, circ) in _LANE_TAPS.items()] + [
    Embed(2, 1, 3, 4, 96, 1, 4, 8, 1, ("lane16", 6, 8), "partial", "Wo = 1"), Embed(2, 1, 3, 20, 96, 1, 4, 8, 1, ("lane16", 6, 8), "partial", bias0=1024),
    Embed(2, 1, 3, 20, 65, 1, 4, 8, 1, ("generic", True, "atomic"), bias0=1024),
    Embed(1, 1, 1, 4, 48, 1, 4, 4, 0, ("lane16", 3, 8), "partial", "1 token"),
    Embed(2, 1, 3, 20, 64, 1, 4, 8, 1, ("generic", True, "partial")), Embed(2, 1, 3, 20, 65, 1, 4, 8, 1, ("generic", True, "partial")),
    Embed(2, 1, 3, 20, 128, 1, 4, 8, 1, ("generic", True, "partial")), Embed(2, 1, 4, 20, 64, 2, 4, 8, 1, ("generic", True, "partial")),
    Embed(1, 1, 1, 12, 1, 1, 4, 4, 0, ("generic", True, "partial"), what="E = 1, 3 tokens"),
    Embed(2, 1, 3, 20, 96, 1, 4, 8, 1, ("generic", True, "atomic")), Embed(2, 3, 4, 10, 65, 2, 2, 2, 0, ("generic", True, "atomic")),
    Embed(2, 1, 3, 20, 128, 1, 4, 4, 0, ("generic", True, "atomic")),
    Embed(2, 3, 4, 24, 96, 2, 8, 8, 1, ("generic", False, "atomic"), what="48 taps"), Embed(2, 1, 8, 20, 64, 4, 4, 8, 1, ("generic", False, "atomic"), what="32 taps"),
    # grid passes: 512 blocks of 4 tokens (generic) / of 16 tokens (16-lane form)
    Embed(3, 1, 1, 2732, 64, 1, 4, 8, 1, ("generic", True, "partial"), what="2049 tokens"),
    Embed(3, 1, 1, 2732, 96, 1, 4, 4, 0, ("generic", True, "atomic"), what="2049 tokens"),
    Embed(3, 1, 1, 10924, 96, 1, 4, 8, 1, ("lane16", 6, 8), "partial", "8193 tokens"),
]


@dataclass(frozen=True)
class Ln:
    C: int
    rows: int
    route: tuple                  # ln_route(C), written next to the width
    merge: tuple = None           # (B, H, W) of the un-merged tensor
    opts: str = "cover"           # backward option set: "full" | "cover" | "noparts" | "parts"
    what: str = ""

    @property
    def name(self):
        return f"c{self.C}-m{'x'.join(map(str, self.merge))}" if self.merge else f"c{self.C}-r{self.rows}"

    @property
    def crps(self):               # cast_rows_per_sample, counted in tokens of the dx tensor
        return 4 if self.C in (96, 384) else 3

    @property
    def nslab(self):
        return NSLABS[(self.C // 4 + self.rows) % len(NSLABS)]


_LN_ROUTES = {4: (16, 2, False), 48: (16, 2, False), 96: (16, 2, False), 128: (16, 2, True), 132: (16, 4, False), 192: (16, 4, False),
              256: (16, 4, True), 260: (64, 2, False), 384: (64, 2, False), 512: (64, 2, True), 516: (64, 4, False), 768: (64, 3, True),
              1024: (64, 4, True), 1028: (64, 8, False), 1536: (64, 6, True), 2048: (64, 8, True), 2052: (64, 24, False),
              3072: (64, 12, True), 6144: (64, 24, True)}
LN_CASES = [Ln(C, 256 // r[0] + 1, r, opts="full" if C in (96, 384) else "cover") for C, r in _LN_ROUTES.items()] + [
    Ln(C, n, r) for C, r in _LN_ROUTES.items() for n in (1, 256 // r[0] - 1)] + [
    Ln(192, 3, (16, 4, False), merge=(3, 2, 2), what="H/2 = W/2 = 1"), Ln(256, 9, (16, 4, True), merge=(3, 2, 6), what="H/2 = 1"),
    Ln(192, 9, (16, 4, False), merge=(3, 6, 2), what="W/2 = 1"),
    Ln(8, 4096 * 16 + 1, (16, 2, False), opts="noparts", what="grid cap, 16 lanes per row"),
    Ln(260, 4096 * 4 + 1, (64, 2, False), opts="noparts", what="grid cap, 64 lanes per row"),
    Ln(48, 512 * 16 + 1, (16, 2, False), opts="parts", what="partial-row cap"), Ln(384, 512 * 4 + 1, (64, 2, False), opts="parts", what="partial-row cap"),
]
BWD_LEVELS = {"src": ("dy", "slabs"), "dres": ("none", "separate", "inplace"), "parts": (False, True), "cast": ("none", "unscaled", "scaled")}


def pairwise_cover(levels):
    """a small list of option dicts in which every value of every option meets every value of every other option (greedy)"""
    keys = list(levels)
    allc = [dict(zip(keys, v)) for v in itertools.product(*levels.values())]
    pairs = lambda o: {(a, o[a], b, o[b]) for i, a in enumerate(keys) for b in keys[i + 1:]}
    need, out = set().union(*(pairs(o) for o in allc)), []
    while need:
        best = max(allc, key=lambda o: len(pairs(o) & need))
        out.append(best)
        need -= pairs(best)
    return out


def bwd_options(c: Ln):
    lv = dict(BWD_LEVELS)
    can = ln_partial_rows(c.rows, c.C) > 0
    if c.opts == "noparts" or not can:
        lv["parts"] = (False,)
    if c.opts == "parts":
        lv["parts"] = (True,)
    if c.opts == "full":
        return [dict(zip(lv, v)) for v in itertools.product(*lv.values())]
    if c.opts in ("noparts", "parts"):
        return [dict(src="dy", dres="none", parts=lv["parts"][0], cast="scaled"), dict(src="slabs", dres="inplace", parts=lv["parts"][0], cast="none")]
    return pairwise_cover(lv)


@dataclass(frozen=True)
class Params:
    C: int
    rows: int
    grid: tuple                   # ln_params_grid(rows, C) = (tpr_log2, gx, gy, rows per block)
    merge: tuple = None

    @property
    def name(self):
        return f"c{self.C}-m{'x'.join(map(str, self.merge))}" if self.merge else f"c{self.C}-r{self.rows}"


PARAMS = [Params(4, 1, (4, 1, 1, 1)), Params(4, 2048, (4, 1, 1, 2048)), Params(4, 2049, (4, 1, 33, 63)), Params(4, 4100, (4, 1, 65, 64)),
          Params(48, 1, (4, 1, 1, 1)), Params(48, 2048, (4, 1, 1, 2048)), Params(48, 2049, (4, 1, 33, 63)), Params(48, 4100, (4, 1, 65, 64)),
          Params(96, 1, (5, 1, 1, 1)), Params(96, 2048, (5, 1, 1, 2048)), Params(96, 2049, (5, 1, 65, 32)), Params(96, 4100, (5, 1, 129, 32)),
          Params(192, 1, (6, 1, 1, 1)), Params(192, 2048, (6, 1, 1, 2048)), Params(192, 2049, (6, 1, 129, 16)), Params(192, 4100, (6, 1, 257, 16)),
          Params(384, 1, (6, 2, 1, 1)), Params(384, 2048, (6, 2, 1, 2048)), Params(384, 2049, (6, 2, 129, 16)), Params(384, 4100, (6, 2, 257, 16)),
          Params(1536, 1, (6, 6, 1, 1)), Params(1536, 2048, (6, 6, 1, 2048)), Params(1536, 2049, (6, 6, 129, 16)), Params(1536, 4100, (6, 6, 257, 16)),
          Params(192, 9, (6, 1, 1, 9), merge=(3, 2, 6))]


@dataclass(frozen=True)
class SplitK:
    N: int
    M: int
    nslab: int
    bias: bool
    aux: bool
    rowscale: bool
    out16: bool
    rps: int = 3
    nch: int = 0                  # splitk_ln_nch(N)

    @property
    def name(self):
        f = "".join(ch for ch, on in zip("bars", (self.bias, self.aux, self.rowscale, self.out16)) if on) or "plain"
        return f"n{self.N}-m{self.M}-s{self.nslab}-{f}"


SPLITK = [SplitK(256, 1, 1, False, False, False, False, nch=1), SplitK(256, 5, 3, True, True, True, True, nch=1),
          SplitK(512, 8, 4, True, True, False, True, nch=2), SplitK(512, 5, 9, False, True, True, False, rps=2, nch=2),
          SplitK(768, 5, 5, True, False, False, True, nch=3), SplitK(768, 8, 3, False, True, True, True, nch=3),
          SplitK(1024, 1, 9, True, True, True, False, nch=4), SplitK(1024, 8, 4, False, False, False, True, nch=4),
          SplitK(1536, 5, 4, True, True, True, True, nch=6), SplitK(1536, 1, 5, False, True, False, False, nch=6),
          SplitK(2048, 8, 9, True, True, True, True, nch=8), SplitK(2048, 5, 1, True, False, False, False, nch=8),
          SplitK(256, 8, 5, True, False, True, True, nch=1)]      # a rowscale without aux: the launcher ignores it


# ------------------------------------------------------------------ pieces
@dataclass
class Prob:
    op: str
    case: object
    ins: dict                     # name -> Buf inside NaN
    outs: dict                    # name -> Buf, guard-filled (or holding the initial gradients)
    ref: dict                     # float64 references, budgets, index maps


def _seed(*v):
    s = 91
    for x in v:
        s = (s * 1000003 + int(x)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


_mat, _vec, odd_ints = GL._mat, GL._vec, GL.odd_ints


def _ovec(n, device, init=None):
    b = Buf(1, n, n + 8, F32, "guard", device)
    return b.set(init.reshape(1, n)) if init is not None else b


def _finite_err(g64, want):
    return torch.where(torch.isfinite(g64), (g64 - want).abs(), torch.full_like(want, math.inf))


def exact_rows(rows, K, gen):
    """glue_exact's rows: K/4 each of +1, -1, +m, -m in a seeded order; sum 0, variance + LN_EPS a power of 4; and the exact rstd"""
    kind = torch.randint(0, 3, (rows,), generator=gen)
    m = torch.tensor(GL.ROW_MAGS, dtype=F64)[kind][:, None]
    one = torch.ones(rows, K // 4, dtype=F64)
    v = torch.cat([one, -one, m * one, -m * one], 1).gather(1, torch.rand(rows, K, generator=gen).argsort(1))
    rstd = torch.tensor(GL.ROW_RSTD, dtype=F64)[kind]
    assert bool((v.sum(1) == 0).all()) and torch.equal(1 / torch.sqrt((v * v).mean(1) + LN_EPS), rstd)
    return v, rstd


def row_offsets(rows, gen):
    """0 on even rows, a non-zero integer on odd rows"""
    o = torch.randint(1, 7, (rows,), generator=gen).to(F64) * (2 * torch.randint(0, 2, (rows,), generator=gen).to(F64) - 1)
    o[0::2] = 0
    return o


def assert_half_ulp_margin(v, rstd, off, gamma, beta):
    """y = v rstd gamma + beta is a bf16 value, never 0, and the fp32 error of its terms cannot move its rounding"""
    term = v * rstd[:, None] * gamma
    y = term + beta
    assert torch.equal(GL.rounded(y), y) and bool((y != 0).all())
    slack = 16 * ND.ulp_f32(term.abs() + beta.abs()) + 2 * (ND.ulp_f32(off) * (off != 0) * rstd)[:, None] * gamma.abs()
    assert bool((slack < 0.5 * ND.ulp_bf16(y)).all())
    return y


def sample_scales(n, gen):
    start = int(torch.randint(1, len(SCALES), (1,), generator=gen))
    return torch.tensor(SCALES, dtype=F64)[(torch.arange(n) + start) % len(SCALES)]


def fold32(slabs64, order=None):
    """float32 left-to-right fold of [nslab][...] (the order fold_slabs4 promises), as float64"""
    s = slabs64.to(F32)
    acc = torch.zeros_like(s[0])
    for k in (order if order is not None else range(s.shape[0])):
        acc = acc + s[k]
    return acc.to(F64)


def make_slabs(shape, nslab, gen, mag):
    """integer slabs [nslab][*shape]; every fifth column order-sensitive where nslab >= 3: 2^24, 1, ..., 1, -2^24 folds to 0 left to
    right and to nslab - 2 right to left"""
    s = GX.ints(gen, (nslab,) + tuple(shape), -mag, mag, "cpu")
    if nslab >= 3:
        s[0, ..., 0::5], s[1:-1, ..., 0::5], s[-1, ..., 0::5] = 2.0 ** 24, 1.0, -2.0 ** 24
        assert not torch.equal(fold32(s), fold32(s, range(nslab - 1, -1, -1)))
    return s


def budget_of(want, err32, extra=None, half_bf16=False, factor=FACTOR):
    b = torch.full_like(want, max(factor * err32, float(ND.ulp_f32(want.abs().max().reshape(1))) if want.numel() else 0.0))
    if extra is not None:
        b = b + extra
    return b + 0.5 * ND.ulp_bf16(want) if half_bf16 else b


def check_budget(name, g64, want, budget, msg) -> Report:
    rep = Report(name)
    r = ND._ratio(rep, _finite_err(g64, want), budget, want)
    ND._add(rep, r > 1, msg, want)
    return rep


def check_image(name, buf, got_flat, idx=None, v64=None) -> Report:
    """the whole allocation as integers: untouched (idx None), or the logical elements at `idx` holding the rounding of v64"""
    idx = buf.index() if idx is None else idx
    want = GX._ibits(buf.flat).clone() if v64 is None else GX._image(buf, idx, v64)
    return GX.check_out(name, Out(buf, want, idx), got_flat)


def check_guards(name, buf, got_flat, idx) -> Report:
    """every word outside `idx` unchanged, every word inside written (no guard pattern left) and not NaN"""
    every = torch.ones(idx.shape, dtype=torch.bool, device=idx.device)
    rep = GX.check_out(name, Out(buf, GX._ibits(buf.flat).clone(), idx, every), got_flat)
    g = got_flat[idx.reshape(-1)]
    guard = GX.GUARD16 if g.dtype == BF16 else GX.GUARD32
    ND._add(rep, GX._ibits(g.contiguous()) == guard, "words never written")
    ND._add(rep, torch.isnan(g), "NaN stored")
    if rep.violations:
        rep.worst = math.inf
    return rep


def fresh(pb: Prob) -> dict:
    return {k: b.flat.clone() for k, b in pb.outs.items()}


# ------------------------------------------------------------------ patch embedding
def embed_index(c: Embed, defect=None):
    """[ntok][taps] positions of every tap of every token in the (B, Cin, Hin, Win) image; tap t = (ic p0 + i) kw + k"""
    tok = torch.arange(c.ntok)[:, None]
    w, t2 = tok % c.Wo, tok // c.Wo
    h, b = t2 % c.Ho, t2 // c.Ho
    t = torch.arange(c.taps)[None, :]
    k, tt = t % c.kw, t // c.kw
    i, ic = tt % c.p0, tt // c.p0
    if defect == "tap_order_channel_minor":
        ic, i = tt % c.Cin, tt // c.Cin
    col = c.p1 * w + k
    if c.circ:
        col = col - (1 if defect == "pad_is_1" else 2)
        col = torch.where(col < 0, torch.zeros_like(col) if defect == "wrap_left_clamped" else col + c.Win, col)
        col = torch.where(col >= c.Win, torch.full_like(col, c.Win - 1) if defect == "wrap_right_clamped" else col - c.Win, col)
    row = c.p0 * h + (0 if defect == "patch_row_ignored" else i)
    return ((b * (1 if defect == "batch_stride_ignores_cin" else c.Cin) + ic) * c.Hin + row) * c.Win + col


def embed_math(x, w, b, ga, be, dy, eps, dtype):
    """conv + LayerNorm forward and backward of [ntok][taps] patches in `dtype`, per token (no sum over tokens)"""
    x, w, b, ga, be = (t.to(dtype) for t in (x, w, b, ga, be))
    a = x @ w.t() + b
    mu = a.mean(1, keepdim=True)
    d = a - mu
    rs = 1 / torch.sqrt((d * d).mean(1, keepdim=True) + eps)
    xh = d * rs
    r = {"out": xh * ga + be}
    if dy is not None:
        dy = dy.to(dtype)
        gy = dy * ga
        r["dc"] = rs * (gy - gy.mean(1, keepdim=True) - xh * (gy * xh).mean(1, keepdim=True))
        r["xh"] = xh
    return r


def embed_nz_tokens(c: Embed, gen):
    """the tokens whose dout is not zero: all where there are at most MAX_NZ, else the first, the last, both sides of every grid
    pass boundary of either form and a seeded rest"""
    if c.ntok <= MAX_NZ:
        return torch.arange(c.ntok)
    per_pass = 512 * 4                                                 # the generic forms' pass; the 16-lane form's 8192 is a multiple
    must = {0, c.ntok - 1} | {p for q in range(per_pass, c.ntok, per_pass) for p in (q - 1, q)}
    rest = [int(t) for t in torch.randperm(c.ntok, generator=gen) if int(t) not in must][:MAX_NZ - len(must)]
    return torch.tensor(sorted(must | set(rest)))


def build_embed(c: Embed, device="cpu") -> Prob:
    bwd = bool(c.form)
    gen = _seed(5, c.B, c.Cin, c.Hin, c.Win, c.E, c.p0, c.p1, c.kw, c.circ)
    E, T, ntok = c.E, c.taps, c.ntok
    img = GX.ints(gen, (c.B * c.Cin * c.Hin, c.Win), -7, 7, "cpu")
    w, b = GX.ints(gen, (E, T), -3, 3, "cpu"), GX.ints(gen, (E,), -8, 8, "cpu") + c.bias0
    gamma, beta = odd_ints(gen, E), GX.ints(gen, (E,), -4, 4, "cpu")
    x = img.reshape(-1)[embed_index(c)]
    assert float((x.abs() @ w.abs().t() + b.abs()).max()) < GX.EXACT_LIMIT
    # the tap index against torch's own convolution (circular: two columns of wrap-around padding each side)
    im4 = img.reshape(c.B, c.Cin, c.Hin, c.Win)
    conv = Fn.conv2d(Fn.pad(im4, (2, 2, 0, 0), mode="circular") if c.circ else im4, w.reshape(E, c.Cin, c.p0, c.kw), b, stride=(c.p0, c.p1))
    assert torch.equal(conv.permute(0, 2, 3, 1).reshape(ntok, E), x @ w.t() + b)
    ins = {"img": _mat(c.B * c.Cin * c.Hin, c.Win, F32, "nan", device, img), "w": _vec(E * T, "nan", device, w.reshape(-1)),
           "b": _vec(E, "nan", device, b), "gamma": _vec(E, "nan", device, gamma), "beta": _vec(E, "nan", device, beta)}
    dy = None
    if bwd:
        nz = embed_nz_tokens(c, gen)
        assert nz.numel() <= MAX_NZ
        dy = torch.zeros(ntok, E, dtype=F64)
        dy[nz] = GX.ints(gen, (nz.numel(), E), -4, 4, "cpu")
        dy[nz, 0] = 1 + dy[nz, 0].abs()                                # no listed token's row is all zero
        ins["dout"] = _mat(ntok, E, F32, "nan", device, dy)
    r64, r32 = embed_math(x, w, b, gamma, beta, dy, LN_EPS, F64), embed_math(x, w, b, gamma, beta, dy, LN_EPS, F32)
    ref = {"out": r64["out"].to(device), "err_out": float((r32["out"].to(F64) - r64["out"]).abs().max())}
    if not bwd:
        o16c = Buf(ntok, 2 * E, 2 * E, BF16, "guard", device)
        outs = {"out": _mat(ntok, E, F32, "guard", device), "ld_e": _mat(ntok, E, BF16, "guard", device), "ld_2e": o16c}
        ref["idx16"] = {"ld_e": outs["ld_e"].index(), "ld_2e": o16c.index()[:, E:]}
        return Prob("embed_fwd", c, ins, outs, ref)
    n = int(nz.numel())
    sums = lambda f: {"dw": f["dc"].t() @ x.to(f["dc"].dtype), "db": f["dc"].sum(0), "dgamma": (dy.to(f["dc"].dtype) * f["xh"]).sum(0)}
    s64, s32 = sums(r64), sums(r32)
    absum = {"dw": r64["dc"].abs().t() @ x.abs(), "db": r64["dc"].abs().sum(0), "dgamma": (dy * r64["xh"]).abs().sum(0)}
    init = {k: GX.ints(gen, s, -5, 5, "cpu") for k, s in (("dw", (E, T)), ("db", (E,)), ("dgamma", (E,)), ("dbeta", (E,)))}
    if c.form == "partial":
        init = {k: torch.zeros_like(v) for k, v in init.items()}
    ref["dbeta"], ref["init"], ref["n_nz"] = (dy.sum(0) + init["dbeta"]).to(device), {k: v.to(device) for k, v in init.items()}, n
    terms = n + (c.form == "atomic")                                   # the initial gradient is one more term of the atomic sum
    for k in ("dw", "db", "dgamma"):
        ref[k] = (s64[k] + init[k]).to(device)
        err32 = float((s32[k].to(F64) - s64[k]).abs().max())
        ref["err_" + k] = err32
        ref["bud_" + k] = budget_of(ref[k], err32, ((terms - 1) * U32 * (absum[k] + init[k].abs())).to(device), factor=FACTORS.get(k, FACTOR))
    if c.form == "atomic":
        outs = {k: _ovec(v.numel(), device, v.reshape(-1)) for k, v in init.items()}
    else:
        cols = E * T + 3 * E
        outs = {"part": Buf(embed_bwd_blocks(ntok), cols, cols + 13, F32, "guard", device)}
    return Prob("embed_bwd", c, ins, outs, ref)


def embed_token_block(c: Embed):
    """partial row (block) of every token, and the rows whose block holds no token"""
    nb = embed_bwd_blocks(c.ntok)
    per = 16 if c.route[0] == "lane16" else 4
    blk = (torch.arange(c.ntok) % (nb * per)) // per
    return blk, nb


def check_embed_fwd(pb: Prob, got: dict, variant="ld_2e") -> list:
    c, reps = pb.case, []
    o = pb.outs["out"]
    reps.append(check_guards(f"{c.name}.out guards", o, got["out"], o.index()))
    g = got["out"][o.index()].to(F64)
    reps.append(check_budget(f"{c.name}.out", g, pb.ref["out"], budget_of(pb.ref["out"], pb.ref["err_out"], factor=FACTORS.get("out", FACTOR)),
                             f"out above its budget (torch-float32 error {pb.ref['err_out']:.3e})"))
    for v in ("ld_e", "ld_2e"):
        if v == variant:      # the one rounding of the fp32 value the launch itself stored
            reps.append(check_image(f"{c.name}.out_bf16 {v}", pb.outs[v], got[v], pb.ref["idx16"][v], g))
        else:
            reps.append(check_image(f"{c.name}.out_bf16 {v} (not given)", pb.outs[v], got[v]))
    return reps


def check_embed_bwd(pb: Prob, got: dict) -> list:
    c, reps, E, T = pb.case, [], pb.case.E, pb.case.taps
    if c.form == "atomic":
        vals = {}
        for k in ("dw", "db", "dgamma", "dbeta"):
            b = pb.outs[k]
            reps.append(check_guards(f"{c.name}.{k} guards", b, got[k], b.index()))
            vals[k] = got[k][b.index().reshape(-1)].to(F64)
    else:
        b = pb.outs["part"]
        reps.append(check_guards(f"{c.name}.partial rows guards", b, got["part"], b.index()))
        p = got["part"][b.index()].to(F64)
        blk, nb = embed_token_block(c)
        empty = torch.ones(nb, dtype=torch.bool)
        empty[blk] = False
        rep = Report(f"{c.name}.rows of blocks without tokens")
        ND._add(rep, (p[empty.to(p.device)] != 0).any(1), "rows not exactly zero")
        rep.worst = math.inf if rep.violations else 0.0
        reps.append(rep)
        tot = torch.nan_to_num(p, nan=math.inf).sum(0)
        vals = {"dw": tot[:E * T], "db": tot[E * T:E * T + E], "dgamma": tot[E * T + E:E * T + 2 * E], "dbeta": tot[E * T + 2 * E:]}
    rep = Report(f"{c.name}.dbeta")
    ND._add(rep, vals["dbeta"] != pb.ref["dbeta"], "d(beta) is not the exact sum", pb.ref["dbeta"])
    rep.worst = math.inf if rep.violations else 0.0
    reps.append(rep)
    for k in ("dw", "db", "dgamma"):
        reps.append(check_budget(f"{c.name}.{k}", vals[k], pb.ref[k].reshape(-1), pb.ref["bud_" + k].reshape(-1),
                                 f"{k} above its budget (torch-float32 error {pb.ref['err_' + k]:.3e}, {pb.ref['n_nz']} non-zero tokens)"))
    return reps


def embed_fold(pb: Prob, got: dict):
    """(dw, db, dgamma, dbeta) as float64 vectors minus the initial gradients: what either form accumulated"""
    if pb.case.form == "atomic":
        return torch.cat([got[k][pb.outs[k].index().reshape(-1)].to(F64) - pb.ref["init"][k].reshape(-1) for k in ("dw", "db", "dgamma", "dbeta")])
    return got["part"][pb.outs["part"].index()].to(F64).sum(0)


def check_fold_vs_atomic(pb: Prob, fold, atomic) -> list:
    """the float64 fold of the partial rows against what the atomic form added, per output; the ratios are against 1 x the budget
    of the output, the verdict against FACTORS["fold_vs_atomic"] x that budget (d(beta): equal)"""
    E, T, reps, at = pb.case.E, pb.case.taps, [], 0
    for k, n in (("dw", E * T), ("db", E), ("dgamma", E), ("dbeta", E)):
        bud = pb.ref["bud_" + k].reshape(-1) if k != "dbeta" else torch.zeros(E, dtype=F64, device=fold.device)
        rep = Report(f"{pb.case.name}.fold vs atomic {k}")
        r = ND._ratio(rep, _finite_err(fold[at:at + n], atomic[at:at + n]), bud, atomic[at:at + n])
        ND._add(rep, r > FACTORS["fold_vs_atomic"], f"partial-row fold and atomic {k} further apart than {FACTORS['fold_vs_atomic']} x the budget")
        reps.append(rep)
        at += n
    return reps


EMBED_DEFECTS = ("wrap_left_clamped", "wrap_right_clamped", "pad_is_1", "tap_order_channel_minor", "batch_stride_ignores_cin",
                 "patch_row_ignored", "tail_group_dropped", "clamped_token_stored", "second_pass_dropped", "upper_half_dropped",
                 "bf16_truncated", "ld16_is_E", "onepass_variance", "eps_dropped", "partial_padding_written",
                 "empty_block_row_unwritten", "atomic_form_overwrites", "dgamma_dbeta_swapped", "db_is_dbeta", "taps_mask_missing")


def _rnd(x32, defect):
    if defect == "bf16_truncated":
        return ND.cast_truncating(x32.contiguous().cpu()).to(x32.device).reshape(x32.shape)
    return x32.to(BF16)


def _ln32(a, C, eps, defect=None, divide=False):
    """float32 LayerNorm statistics the way the kernels form them: two passes, sums times a rounded 1/C (tulip_splitk_resid_ln:
    divided by C), and a reciprocal square root rounded once"""
    inv = torch.tensor(1.0 / C, dtype=F32, device=a.device)
    scale = (lambda s: (s.to(F64) / C).to(F32)) if divide else (lambda s: s * inv)
    mu = scale(a.sum(1, keepdim=True))
    d = a - mu
    var = (scale((a * a).sum(1, keepdim=True)) - mu * mu) if defect == "onepass_variance" else scale((d * d).sum(1, keepdim=True))
    return mu, d, (1 / torch.sqrt((var + (0.0 if defect == "eps_dropped" else eps)).to(F64))).to(F32)


def emulate_embed(pb: Prob, defect=None, variant="ld_2e") -> dict:
    c, got, i = pb.case, fresh(pb), pb.ins
    dev = i["img"].flat.device
    E, T, ntok = c.E, c.taps, c.ntok
    f = lambda n: i[n].view.to(F32).reshape(-1)
    x = i["img"].flat[i["img"].off + embed_index(c, defect).to(dev)].to(F32)
    w = f("w").reshape(E, T)
    a = x @ w.t() + f("b")
    # taps_mask_missing stands for the `t < g.taps` mask on the WEIGHT loads of patch_embed_bwd16_kernel only: the weights past taps
    # meet a zero tap, so it shows where the last channels' reads run into the NaN behind w.  The `v < g.taps` mask on the d(w)
    # store is a different fault that no defect models (d(w) of the next channel would be overwritten: the d(w) budget sees it).
    if defect == "taps_mask_missing" and c.form and c.route[0] == "lane16" and T < c.route[2]:
        wf = i["w"].flat                                              # weights t in [taps, TAPS) of channel ch: w[ch taps + t], times a zero tap
        past = wf[(i["w"].off + torch.arange(E, device=dev)[:, None] * T + torch.arange(T, c.route[2], device=dev)[None, :])]
        a = a + (past.to(F32) * 0).sum(1)
    mu, d, rs = _ln32(a, E, LN_EPS, defect)
    xh = d * rs
    keep = torch.ones(ntok, dtype=torch.bool, device=dev)
    if defect == "second_pass_dropped":
        keep[(512 * (4 if c.form and c.route[0] != "lane16" else 16)):] = False
    if not c.form:
        y = xh * f("gamma") + f("beta")
        if defect == "tail_group_dropped":
            keep[ntok - ntok % 4:] = False
        ch = torch.ones(E, dtype=torch.bool, device=dev)
        if defect == "upper_half_dropped":
            ch[64:] = False
        o = pb.outs["out"]
        sel = keep[:, None] & ch[None, :]
        got["out"][o.index()[sel]] = y[sel]
        if defect == "clamped_token_stored" and ntok % 4:
            got["out"][o.off + ntok * o.pitch + torch.arange(E, device=dev)] = y[-1]
        if variant != "absent":
            idx = pb.ref["idx16"][variant]
            if defect == "ld16_is_E" and variant == "ld_2e":
                idx = idx[0:1, :] + torch.arange(ntok, device=dev)[:, None] * E
            got[variant][idx[sel]] = _rnd(y, defect)[sel]
        return got
    dy = i["dout"].view.to(F32)
    gy = dy * f("gamma")
    inv = torch.tensor(1.0 / E, dtype=F32, device=dev)
    dc = rs * (gy - gy.sum(1, keepdim=True) * inv - xh * ((gy * xh).sum(1, keepdim=True) * inv))
    per = torch.cat([(dc[:, :, None] * x[:, None, :]).reshape(ntok, E * T), dc, dy * xh, dy], 1) * keep[:, None]   # [ntok][dw | db | dgamma | dbeta]
    seg = {"dw": slice(0, E * T), "db": slice(E * T, E * T + E), "dgamma": slice(E * T + E, E * T + 2 * E), "dbeta": slice(E * T + 2 * E, E * T + 3 * E)}
    if defect == "dgamma_dbeta_swapped":
        seg["dgamma"], seg["dbeta"] = seg["dbeta"], seg["dgamma"]
    if defect == "db_is_dbeta":
        seg["db"] = seg["dbeta"]
    order = torch.cat([torch.arange(per.shape[1], device=dev)[seg[k]] for k in ("dw", "db", "dgamma", "dbeta")])
    per = per[:, order]
    if c.form == "atomic":
        tot = per.sum(0)
        for k, s in (("dw", slice(0, E * T)), ("db", slice(E * T, E * T + E)), ("dgamma", slice(E * T + E, E * T + 2 * E)), ("dbeta", slice(E * T + 2 * E, None))):
            b = pb.outs[k]
            ix = b.index().reshape(-1)
            got[k][ix] = tot[s] + (0 if defect == "atomic_form_overwrites" else got[k][ix])
        return got
    blk, nb = embed_token_block(c)
    rows = torch.zeros(nb, per.shape[1], dtype=F32, device=dev).index_add_(0, blk.to(dev), per)
    b = pb.outs["part"]
    wr = torch.ones(nb, dtype=torch.bool, device=dev)
    if defect == "empty_block_row_unwritten":
        wr[:] = False
        wr[blk.to(dev)] = True
    got["part"][b.index()[wr]] = rows[wr]
    if defect == "partial_padding_written":
        got["part"][b.off + b.cols:b.off + b.pitch] = 0
    return got


# ------------------------------------------------------------------ LayerNorm family
def _rows_to_layout(v, c, device):
    """[rows][C] -> the tensor the launch reads: itself, or the (B, H, W, C/4) tensor whose 2x2 merge gives those rows"""
    if c.merge is None:
        return _mat(v.shape[0], c.C, F32, "nan", device, v)
    B, H, W = c.merge
    return _mat(B * H * W, c.C // 4, F32, "nan", device, ND.ln_merge_scatter(v, B, H, W, c.C // 4).reshape(-1, c.C // 4))


def _layout_index(buf, c, order=(0, 1, 2, 3)):
    """[rows][C] flat positions in `buf` (laid out as _rows_to_layout's tensor) of the merged rows' elements"""
    if c.merge is None:
        return buf.index()
    B, H, W = c.merge
    return GL.merge_gather(buf.index().reshape(B, H, W, c.C // 4), order)


def _ln_operands(c, gen):
    v, rstd = exact_rows(c.rows, c.C, gen)
    off = row_offsets(c.rows, gen)
    gamma, beta = odd_ints(gen, c.C), GX.ints(gen, (c.C,), -4, 4, "cpu")
    y = assert_half_ulp_margin(v, rstd, off, gamma, beta)
    return v, rstd, off, gamma, beta, y


def build_ln_fwd(c: Ln, device="cpu") -> Prob:
    if c.merge:
        assert c.rows == c.merge[0] * (c.merge[1] // 2) * (c.merge[2] // 2)
    gen = _seed(6, c.C, c.rows, *(c.merge or ()))
    v, rstd, off, gamma, beta, y = _ln_operands(c, gen)
    x = v + off[:, None]
    _, err = ND.ln_baseline(x, gamma, beta, torch.zeros(c.rows, c.C, dtype=F64), LN_EPS)
    ins = {"x": _rows_to_layout(x, c, device), "gamma": _vec(c.C, "nan", device, gamma), "beta": _vec(c.C, "nan", device, beta)}
    outs = {"y": _mat(c.rows, c.C, BF16, "guard", device), "mean": _ovec(c.rows, device), "rstd": _ovec(c.rows, device)}
    return Prob("ln_fwd", c, ins, outs, {"y": y.to(device), "mean": off.to(device), "rstd": rstd.to(device), "err": err})


def _check_stats(name, pb, got, reps, exact_mean_rows):
    for k in ("mean", "rstd"):
        b = pb.outs[k]
        reps.append(check_guards(f"{name}.{k} guards", b, got[k], b.index()))
        g, want = got[k][b.index().reshape(-1)].to(F64), pb.ref[k]
        reps.append(check_budget(f"{name}.{k}", g, want, budget_of(want, pb.ref["err"][k], factor=FACTORS.get(k, FACTOR)),
                                 f"{k} above its budget (torch-float32 error {pb.ref['err'][k]:.3e})"))
        if k == "mean":
            rep = Report(f"{name}.mean of offset-free rows")
            ND._add(rep, GX._ibits(got[k][b.index().reshape(-1)].contiguous())[exact_mean_rows] != 0, "mean of a row that sums to 0 is not +0")
            rep.worst = math.inf if rep.violations else 0.0
            reps.append(rep)


def check_ln_fwd(pb: Prob, got: dict) -> list:
    c, reps = pb.case, []
    reps.append(check_image(f"{c.name}.y", pb.outs["y"], got["y"], pb.outs["y"].index(), pb.ref["y"]))
    _check_stats(c.name, pb, got, reps, torch.arange(0, c.rows, 2, device=got["mean"].device))
    return reps


def build_ln_bwd(c: Ln, device="cpu") -> Prob:
    gen = _seed(7, c.C, c.rows, *(c.merge or ()))
    C, rows, ns = c.C, c.rows, c.nslab
    v, rstd, off, gamma, _, _ = _ln_operands(c, gen)
    x = v + off[:, None]
    xh = v * rstd[:, None]                                             # exact in the kernel too: mean and rstd are operands
    slabs = make_slabs((rows, C), ns, gen, 200)
    dys = {"dy": GX.ints(gen, (rows, C), -4, 4, "cpu"), "slabs": GL.rounded(fold32(slabs))}
    tokens, cdx = (rows, C) if c.merge is None else (c.merge[0] * c.merge[1] * c.merge[2], C // 4)
    nsamp = -(-tokens // c.crps)
    scale = sample_scales(nsamp, gen)
    dres = GX.ints(gen, (rows, C), -8, 8, "cpu")
    R = ln_partial_rows(rows, C)
    rpb = ln_rpb(C)
    ins = {"x": _rows_to_layout(x, c, device), "mean": _vec(rows, "nan", device, off), "rstd": _vec(rows, "nan", device, rstd),
           "gamma": _vec(C, "nan", device, gamma), "dy": _mat(rows, C, BF16, "nan", device, dys["dy"]),
           "slabs": _mat(ns * rows, C, F32, "nan", device, slabs.reshape(ns * rows, C)), "dres": _rows_to_layout(dres, c, device),
           "scale": _vec(nsamp, "nan", device, scale)}
    outs = {"dx": _mat(tokens, cdx, F32, "guard", device), "dx16": _mat(tokens, cdx, BF16, "guard", device)}
    if R:
        outs["part"] = _mat(R, 2 * C, F32, "guard", device)
    ref = {"scale": scale.to(device), "idx": _layout_index(outs["dx"], c), "idx16": _layout_index(outs["dx16"], c), "dres": dres.to(device)}
    blk = (torch.arange(rows) // rpb) % max(R, 1)
    for src, dy in dys.items():
        if R:                                                          # every partial row is an exact fp32 sum: below 2^24 eighths
            assert float(torch.zeros(R, 2 * C, dtype=F64).index_add_(0, blk, torch.cat([dy * xh, dy], 1).abs()).max()) * 8 < 2.0 ** 24
        gy = dy * gamma
        dx = rstd[:, None] * (gy - gy.mean(1, keepdim=True) - xh * (gy * xh).mean(1, keepdim=True))
        f32 = ND.ln_torch(x, gamma, torch.zeros(C, dtype=F64), dy, LN_EPS, F32)["dx"]
        ref[src] = {"dx": dx.to(device), "err": float((f32 - dx).abs().max()),
                    "err_res": float(((f32.to(F32) + dres.to(F32)).to(F64) - (dx + dres)).abs().max())}
        if R:
            ref[src]["part"] = (torch.zeros(R, 2 * C, dtype=F64).index_add_(0, blk, torch.cat([dy * xh, dy], 1)) + 0.0).to(device)
    return Prob("ln_bwd", c, ins, outs, ref)


def fresh_ln_bwd(pb: Prob, dres="none") -> dict:
    got = fresh(pb)
    if dres == "inplace":                                              # dx holds the residual gradient the launch adds to
        got["dx"][pb.ref["idx"].reshape(-1)] = pb.ref["dres"].reshape(-1).to(F32)
    return got


def cast_scales(pb: Prob, cast, idx16, per_row=False, not_quartered=False):
    """DropPath scale of every [rows][C] element of dx_bf16: scale[token of the dx tensor / crps]"""
    c, b = pb.case, pb.outs["dx16"]
    tok = (idx16 - b.off) // (c.C if not_quartered else b.cols)
    if per_row:
        tok = torch.arange(idx16.shape[0], device=idx16.device)[:, None].expand_as(idx16)
    sc = pb.ins["scale"]
    s = sc.flat[sc.off + (tok // c.crps).clamp(max=sc.cols - 1)].to(F64)
    return s if cast == "scaled" else torch.ones_like(s)


def check_ln_bwd(pb: Prob, got: dict, src="dy", dres="none", parts=False, cast="none") -> list:
    c, reps, r = pb.case, [], pb.ref[src]
    idx = pb.ref["idx"]
    reps.append(check_guards(f"{c.name}.dx guards", pb.outs["dx"], got["dx"], idx))
    want = r["dx"] + (pb.ref["dres"] if dres != "none" else 0)
    err = r["err_res"] if dres != "none" else r["err"]
    g = got["dx"][idx].to(F64)
    reps.append(check_budget(f"{c.name}.dx", g, want, budget_of(want, err, factor=FACTORS.get("dx", FACTOR)), f"dx above its budget (torch-float32 error {err:.3e})"))
    if cast == "none":
        reps.append(check_image(f"{c.name}.dx_bf16 (not given)", pb.outs["dx16"], got["dx16"]))
    else:
        reps.append(check_image(f"{c.name}.dx_bf16 {cast}", pb.outs["dx16"], got["dx16"], pb.ref["idx16"], g * cast_scales(pb, cast, pb.ref["idx16"])))
    if "part" in pb.outs:
        p = pb.outs["part"]
        reps.append(check_image(f"{c.name}.partial rows", p, got["part"], p.index(), r["part"]) if parts else
                    check_image(f"{c.name}.partial rows (not given)", p, got["part"]))
    return reps


LN_DEFECTS = ("rows_tail_dropped", "second_pass_dropped", "last_chunk_dropped", "merge_quadrants_swapped", "cast_scale_per_row",
              "cast_channels_not_quartered", "slab_order_reversed", "slab_fold_not_rounded", "dres_ignored", "params_overwrite",
              "params_row_block_tail_dropped", "partial_rows_past_count_written", "resid_scale_per_row", "resid_bias_after_scale")


def _ln_keep(c, defect, parts=False):
    """[rows] rows a launch stores, [C] channels it stores"""
    rpb = ln_rpb(c.C)
    rows_k, ch = torch.ones(c.rows, dtype=torch.bool), torch.ones(c.C, dtype=torch.bool)
    if defect == "rows_tail_dropped" and c.rows % rpb:
        rows_k[c.rows - c.rows % rpb:] = False
    if defect == "second_pass_dropped":
        rows_k[(512 if parts else 4096) * rpb:] = False
    if defect == "last_chunk_dropped" and not c.route[2]:
        ch[c.C - 4:] = False
    return rows_k, ch


def emulate_ln_fwd(pb: Prob, defect=None) -> dict:
    c, got, i = pb.case, fresh(pb), pb.ins
    dev = i["x"].flat.device
    order = (0, 2, 1, 3) if defect == "merge_quadrants_swapped" else (0, 1, 2, 3)
    a = i["x"].flat[_layout_index(i["x"], c, order)]
    mu, d, rs = _ln32(a, c.C, LN_EPS)
    y = (d * rs * i["gamma"].view.to(F32) + i["beta"].view.to(F32)).to(BF16)
    rk, ch = (t.to(dev) for t in _ln_keep(c, defect))
    sel = rk[:, None] & ch[None, :]
    got["y"][pb.outs["y"].index()[sel]] = y[sel]
    for k, val in (("mean", mu), ("rstd", rs)):
        got[k][pb.outs[k].index().reshape(-1)[rk]] = val.reshape(-1)[rk]
    return got


def emulate_ln_bwd(pb: Prob, defect=None, src="dy", dres="none", parts=False, cast="none") -> dict:
    c, got, i = pb.case, fresh_ln_bwd(pb, dres), pb.ins
    dev = i["x"].flat.device
    order = (0, 2, 1, 3) if defect == "merge_quadrants_swapped" else (0, 1, 2, 3)
    C, rows, ns = c.C, c.rows, c.nslab
    a = i["x"].flat[_layout_index(i["x"], c, order)]
    if src == "slabs":
        s = i["slabs"].view.reshape(ns, rows, C).to(F64)
        acc = fold32(s, range(ns - 1, -1, -1) if defect == "slab_order_reversed" else None).to(F32)
        dy = acc if defect == "slab_fold_not_rounded" else acc.to(BF16).to(F32)
    else:
        dy = i["dy"].view.to(F32)
    mu, rs = i["mean"].view.to(F32).reshape(-1, 1), i["rstd"].view.to(F32).reshape(-1, 1)
    xh = (a - mu) * rs
    gy = dy * i["gamma"].view.to(F32)
    inv = torch.tensor(1.0 / C, dtype=F32, device=dev)
    dx = rs * (gy - gy.sum(1, keepdim=True) * inv - xh * ((gy * xh).sum(1, keepdim=True) * inv))
    idx, idx16 = _layout_index(pb.outs["dx"], c, order), _layout_index(pb.outs["dx16"], c, order)
    if dres != "none" and defect != "dres_ignored":
        src_flat = got["dx"] if dres == "inplace" else i["dres"].flat
        dx = dx + src_flat[idx if dres == "inplace" else _layout_index(i["dres"], c, order)]
    rk, ch = (t.to(dev) for t in _ln_keep(c, defect, parts))
    sel = rk[:, None] & ch[None, :]
    got["dx"][idx[sel]] = dx[sel]
    if cast != "none":
        s = cast_scales(pb, cast, idx16, defect == "cast_scale_per_row", defect == "cast_channels_not_quartered" and c.merge is not None)
        got["dx16"][idx16[sel]] = (dx * s.to(F32)).to(BF16)[sel]
    if parts:
        R, p = ln_partial_rows(rows, C), pb.outs["part"]
        blk = ((torch.arange(rows) // ln_rpb(C)) % R).to(dev)
        per = torch.cat([dy * xh, dy], 1) * sel.to(F32).repeat(1, 2)
        got["part"][p.index().reshape(-1)] = torch.zeros(R, 2 * C, dtype=F32, device=dev).index_add_(0, blk, per).reshape(-1)
        if defect == "partial_rows_past_count_written":
            got["part"][p.off + R * p.pitch:p.off + (R + 1) * p.pitch] = 0
    return got


# ---- tulip_layernorm_bwd_params
def build_params(c: Params, device="cpu") -> Prob:
    gen = _seed(8, c.C, c.rows, *(c.merge or ()))
    v, rstd = exact_rows(c.rows, c.C, gen)
    off = row_offsets(c.rows, gen)
    dy = GX.ints(gen, (c.rows, c.C), -4, 4, "cpu")
    init = {"dgamma": GX.ints(gen, (c.C,), -5, 5, "cpu"), "dbeta": GX.ints(gen, (c.C,), -5, 5, "cpu")}
    xh = v * rstd[:, None]
    assert float((dy * xh).abs().sum(0).max()) * 8 + 40 < 2.0 ** 24
    ins = {"x": _rows_to_layout(v + off[:, None], c, device), "mean": _vec(c.rows, "nan", device, off), "rstd": _vec(c.rows, "nan", device, rstd),
           "dy": _mat(c.rows, c.C, BF16, "nan", device, dy)}
    outs = {k: _ovec(c.C, device, t) for k, t in init.items()}
    ref = {"dgamma": (init["dgamma"] + (dy * xh).sum(0)).to(device), "dbeta": (init["dbeta"] + dy.sum(0)).to(device)}
    return Prob("params", c, ins, outs, ref)


def check_params(pb: Prob, got: dict) -> list:
    return [check_image(f"{pb.case.name}.{k}", pb.outs[k], got[k], pb.outs[k].index(), pb.ref[k].reshape(1, -1)) for k in ("dgamma", "dbeta")]


def emulate_params(pb: Prob, defect=None) -> dict:
    c, got, i = pb.case, fresh(pb), pb.ins
    order = (0, 2, 1, 3) if defect == "merge_quadrants_swapped" else (0, 1, 2, 3)
    a = i["x"].flat[_layout_index(i["x"], c, order)]
    xh = (a - i["mean"].view.to(F32).reshape(-1, 1)) * i["rstd"].view.to(F32).reshape(-1, 1)
    dy = i["dy"].view.to(F32)
    _, _, gy, rpb = ln_params_grid(c.rows, c.C)
    keep = torch.ones(c.rows, 1, dtype=F32, device=a.device)
    if defect == "params_row_block_tail_dropped" and gy > 1:
        keep[(gy - 1) * rpb:] = 0
    for k, t in (("dgamma", dy * xh), ("dbeta", dy)):
        ix = pb.outs[k].index().reshape(-1)
        got[k][ix] = (t * keep).sum(0) + (0 if defect == "params_overwrite" and gy == 1 else got[k][ix])
    return got


# ---- tulip_splitk_resid_ln
def build_splitk(c: SplitK, device="cpu") -> Prob:
    gen = _seed(9, c.N, c.M, c.nslab, c.bias, c.aux, c.rowscale, c.out16)
    M, N = c.M, c.N
    slabs = make_slabs((M, N), c.nslab, gen, 40)
    bias = GX.ints(gen, (N,), -9, 9, "cpu")
    nsamp = -(-M // c.rps)
    scale = sample_scales(nsamp, gen)
    sc = scale[torch.arange(M) // c.rps][:, None] if c.rowscale else torch.ones(M, 1, dtype=F64)
    acc = fold32(slabs) + (bias if c.bias else 0)
    gamma, beta = odd_ints(gen, N), GX.ints(gen, (N,), -4, 4, "cpu")
    if c.aux:                                                          # the residual makes every row an exact LayerNorm row
        v, rstd = exact_rows(M, N, gen)
        off = row_offsets(M, gen)
        out = v + off[:, None]
        aux = out - sc * acc
        y = assert_half_ulp_margin(v, rstd, off, gamma, beta)
        assert float((aux.abs() + (sc * acc).abs()).max()) * 4 < GX.EXACT_LIMIT
    else:
        out, aux = acc, torch.zeros(M, N, dtype=F64)
    base, err = ND.ln_baseline(out, gamma, beta, torch.zeros(M, N, dtype=F64), LN_EPS)
    ins = {"slabs": _mat(c.nslab * M, N, F32, "nan", device, slabs.reshape(-1, N)), "bias": _vec(N, "nan", device, bias),
           "aux": Buf(M, N, N + 8, F32, "nan", device).set(aux), "scale": _vec(nsamp, "nan", device, scale),
           "gamma": _vec(N, "nan", device, gamma), "beta": _vec(N, "nan", device, beta)}
    outs = {"out": Buf(M, N, N + 12, F32, "guard", device), "out16": Buf(M, N, N + 20, BF16, "guard", device),
            "y": _mat(M, N, BF16, "guard", device), "mean": _ovec(M, device), "rstd": _ovec(M, device)}
    ref = {"out": out.to(device), "err": err, "exact": c.aux, "y": (y if c.aux else base["y"]).to(device),
           "mean": (off if c.aux else base["mean"]).to(device), "rstd": (rstd if c.aux else base["rstd"]).to(device)}
    return Prob("splitk", c, ins, outs, ref)


def check_splitk(pb: Prob, got: dict) -> list:
    c, reps, o = pb.case, [], pb.outs
    reps.append(check_image(f"{c.name}.out", o["out"], got["out"], o["out"].index(), pb.ref["out"]))
    reps.append(check_image(f"{c.name}.out_bf16", o["out16"], got["out16"], o["out16"].index(), pb.ref["out"]) if c.out16 else
                check_image(f"{c.name}.out_bf16 (not given)", o["out16"], got["out16"]))
    if pb.ref["exact"]:
        reps.append(check_image(f"{c.name}.ln_out", o["y"], got["y"], o["y"].index(), pb.ref["y"]))
    else:
        reps.append(check_guards(f"{c.name}.ln_out guards", o["y"], got["y"], o["y"].index()))
        reps.append(check_budget(f"{c.name}.ln_out", got["y"][o["y"].index()].to(F64), pb.ref["y"],
                                 budget_of(pb.ref["y"], pb.ref["err"]["y"], half_bf16=True, factor=FACTORS.get("y", FACTOR)), "ln_out above its budget"))
    dev = got["mean"].device
    _check_stats(c.name, pb, got, reps, torch.arange(0, c.M if pb.ref["exact"] else 0, 2, device=dev))
    return reps


def emulate_splitk(pb: Prob, defect=None) -> dict:
    c, got, i = pb.case, fresh(pb), pb.ins
    M, N = c.M, c.N
    dev = i["slabs"].flat.device
    s = i["slabs"].view.reshape(c.nslab, M, N).to(F64)
    a = fold32(s, range(c.nslab - 1, -1, -1) if defect == "slab_order_reversed" else None).to(F32)
    bias = i["bias"].view.to(F32) if c.bias else 0
    if defect != "resid_bias_after_scale":
        a = a + bias
    if c.aux:
        r = torch.arange(M, device=dev)
        sc = i["scale"].flat[i["scale"].off + ((r if defect == "resid_scale_per_row" else r // c.rps)).clamp(max=i["scale"].cols - 1)][:, None] if c.rowscale else 1.0
        a = i["aux"].view + sc * a
    if defect == "resid_bias_after_scale":
        a = a + bias
    rk = torch.ones(M, dtype=torch.bool, device=dev)
    if defect == "rows_tail_dropped" and M % 4:
        rk[M - M % 4:] = False
    got["out"][pb.outs["out"].index()[rk]] = a[rk]
    if c.out16:
        got["out16"][pb.outs["out16"].index()[rk]] = a.to(BF16)[rk]
    mu, d, rs = _ln32(a, N, LN_EPS, divide=True)
    got["y"][pb.outs["y"].index()[rk]] = (d * rs * i["gamma"].view.to(F32) + i["beta"].view.to(F32)).to(BF16)[rk]
    for k, val in (("mean", mu), ("rstd", rs)):
        got[k][pb.outs[k].index().reshape(-1)[rk]] = val.reshape(-1)[rk]
    return got


# ------------------------------------------------------------------ one table over the seven entry points
OPS = {"embed_fwd": (EMBED_FWD, build_embed, emulate_embed, check_embed_fwd), "embed_bwd": (EMBED_BWD, build_embed, emulate_embed, check_embed_bwd),
       "ln_fwd": (LN_CASES, build_ln_fwd, emulate_ln_fwd, check_ln_fwd), "ln_bwd": (LN_CASES, build_ln_bwd, emulate_ln_bwd, check_ln_bwd),
       "params": (PARAMS, build_params, emulate_params, check_params), "splitk": (SPLITK, build_splitk, emulate_splitk, check_splitk)}
APPLIES = {"embed_fwd": ("wrap_left_clamped", "wrap_right_clamped", "pad_is_1", "tap_order_channel_minor", "batch_stride_ignores_cin",
                         "patch_row_ignored", "tail_group_dropped", "clamped_token_stored", "second_pass_dropped", "upper_half_dropped",
                         "bf16_truncated", "ld16_is_E", "onepass_variance", "eps_dropped"),
           "embed_bwd": ("wrap_left_clamped", "wrap_right_clamped", "pad_is_1", "tap_order_channel_minor", "batch_stride_ignores_cin",
                         "patch_row_ignored", "second_pass_dropped", "onepass_variance", "eps_dropped", "partial_padding_written",
                         "empty_block_row_unwritten", "atomic_form_overwrites", "dgamma_dbeta_swapped", "db_is_dbeta", "taps_mask_missing"),
           "ln_fwd": ("rows_tail_dropped", "second_pass_dropped", "last_chunk_dropped", "merge_quadrants_swapped"),
           "ln_bwd": ("rows_tail_dropped", "second_pass_dropped", "last_chunk_dropped", "merge_quadrants_swapped", "cast_scale_per_row",
                      "cast_channels_not_quartered", "slab_order_reversed", "slab_fold_not_rounded", "dres_ignored",
                      "partial_rows_past_count_written"),
           "params": ("merge_quadrants_swapped", "params_overwrite", "params_row_block_tail_dropped"),
           "splitk": ("rows_tail_dropped", "slab_order_reversed", "resid_scale_per_row", "resid_bias_after_scale")}


def case_of(op, name):
    (c,) = [c for c in OPS[op][0] if c.name == name]
    return c


def ratios(reps):
    """'output ratio' of every budgeted report, for the measured-ratio line the GPU tests print"""
    return " ".join(f"{r.what.rsplit('.', 1)[-1]}={r.worst:.3f}" for r in reps if 0 < r.worst < math.inf)


def emulate(pb: Prob, defect=None, **opt) -> dict:
    """what a launch of pb's entry point leaves in fresh output allocations, in float32 with the kernels' rounding points and write
    sets; `defect` breaks one thing (APPLIES names the defects of each entry point)"""
    assert defect is None or defect in APPLIES[pb.op], (pb.op, defect)
    return OPS[pb.op][2](pb, defect, **opt)


def check(pb: Prob, got: dict, **opt) -> list:
    return OPS[pb.op][3](pb, got, **opt)

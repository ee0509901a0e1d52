"""Exact tests of the one-launch stage boundaries (csrc/glue.hip: tulip_merge_fwd, tulip_merge_bwd, tulip_unmerge_skip_fwd,
tulip_skip_unmerge_bwd): case lists, operand builders, float64 references, checkers and a torch emulation with switchable defects
(test_glue_exact_cpu.py proves the checkers sharp and the case list complete, test_glue_exact_gpu.py applies them to the kernels).
Plain torch on whichever device the caller names; no kernel code.  The allocation kit (Buf, Out, guard patterns, check_out) is
tests/gemm_exact.py's.

The kernels are chains of bf16 GEMMs with stated rounding points, so INTEGER operands make them exact: every GEMM of a chain has
sum_k |a_k b_k| (+ |bias|) below 2^20 quanta (asserted in float64 by the builder), so its fp32 accumulation is exact in any order
and every bf16 tensor between two GEMMs is the one round-to-nearest-even of an exactly known number.

The LayerNorm of the PatchMerging pair is made exact by its rows: a merged row holds K/4 each of +1, -1, +m, -m with m in
{1, 5, 11} varying by row (a seeded permutation, different in the four 2x2 sub-pixels), so its sum is 0 and its variance 1, 13 or
61; with eps = 3 the variance + eps is 4, 16 or 64 and rstd 1/2, 1/4 or 1/8 -- one eps per launch and still three rstd values.
gamma is odd and beta an integer, so (x - mean) rstd gamma is an odd multiple of 1/2, 1/4 or 1/8 and never cancels beta: every xm
value is a non-zero multiple of 1/8 that bf16 holds exactly.  The kernel's rstd may be a few fp32 ulp off (a rounded 1/K, an
approximate rsqrt); the builder asserts that 16 fp32 ulp of the terms stay below half a bf16 ulp of the result, so bf16(xm) cannot
move.  In the backward mean and rstd are operands (0 and the exact power of two), so xhat is exact too.

What cannot be exact: rstd itself (within 2 fp32 ulp), and dx_prev of merge_bwd, which carries two divisions by 4 Cp -- compared per
element with the float64 LayerNorm backward of the exact bf16 d(norm out), budget 4 x the largest error torch's float32 layer_norm
autograd has on the same rows against float64 (numerics_domain.check_ln's rule), at least one fp32 ulp of the row's largest |dx|."""
import math
from dataclasses import dataclass

import torch

from tests import gemm_exact as GX
from tests import numerics_domain as ND
from tests.numerics_domain import Report

F64, F32, BF16 = GX.F64, GX.F32, GX.BF16
Buf, Out = GX.Buf, GX.Out
EXACT_LIMIT, MIN_TIES = GX.EXACT_LIMIT, GX.MIN_TIES
SCALES = (0.0, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0)          # DropPath scales of the cast outputs: x * scale is exact in fp32
LN_EPS = 3.0
ROW_MAGS = (1.0, 5.0, 11.0)                              # variance (1 + m^2) / 2 = 1, 13, 61; + eps = 4, 16, 64
ROW_RSTD = (0.5, 0.25, 0.125)
XM_QUANTUM = 0.125
GATHER = ((0, 0), (1, 0), (0, 1), (1, 1))                # PatchMerging's 2x2 order (dh, dw) of the four channel groups
LN_FACTOR = 4.0


# ------------------------------------------------------------------ cases
def merge_fwd_route(Cin, rows):
    """(row block, KSPLIT, column slices, workgroup order) of tulip_merge_fwd -- the launcher's documented rule: Cin = 96 32-row
    blocks, one slice; 192: 32 rows x 2 slices from 8192 rows, else 16 rows x 4 slices with K split in two; 384: 16 rows x 4
    slices from 4096 rows, else 16 rows x 16 slices with K split in four.  With more than one slice the workgroups are XCD-affine
    where the row-block count is a multiple of 8 and slice-minor otherwise."""
    if Cin == 96:
        bm, ks = 32, 1
    elif Cin == 192:
        bm, ks = (32, 1) if rows >= 8192 else (16, 2)
    else:
        bm, ks = (16, 1) if rows >= 4096 else (16, 4)
    nsl = (2 * Cin) // ((4 // ks) * 3 * 16)
    order = "single" if nsl == 1 else "xcd" if (rows // bm) % 8 == 0 else "slice-minor"
    return bm, ks, nsl, order


@dataclass(frozen=True)
class MergeFwd:
    Cin: int
    B: int
    H: int
    W: int
    route: tuple                  # what the grid must reach: merge_fwd_route's answer, written next to the shape
    what: str = ""

    @property
    def rows(self):
        return self.B * (self.H // 2) * (self.W // 2)

    @property
    def name(self):
        return f"c{self.Cin}-{self.B}x{self.H}x{self.W}"


MERGE_FWD = [
    MergeFwd(96, 1, 2, 64, (32, 1, 1, "single"), "one workgroup"),
    MergeFwd(96, 32, 2, 2, (32, 1, 1, "single"), "every merged row its own sample"),
    MergeFwd(96, 8, 8, 2, (32, 1, 1, "single"), "W/2 = 1"),
    MergeFwd(96, 3, 2, 64, (32, 1, 1, "single"), "three row blocks"),
    MergeFwd(192, 1, 2, 64, (16, 2, 4, "slice-minor"), "2 row blocks"),
    MergeFwd(192, 3, 2, 64, (16, 2, 4, "slice-minor"), "6 row blocks"),
    MergeFwd(192, 1, 8, 64, (16, 2, 4, "xcd"), "8 row blocks"),
    MergeFwd(192, 2, 64, 128, (16, 2, 4, "xcd"), "4096 rows: the last 16-row launch below the 32-row form, 256 row blocks"),
    MergeFwd(192, 2, 128, 128, (32, 1, 2, "xcd"), "8192 rows: 32-row form"),
    MergeFwd(192, 257, 2, 64, (32, 1, 2, "slice-minor"), "32-row form, 257 row blocks"),
    MergeFwd(384, 1, 2, 64, (16, 4, 16, "slice-minor"), "2 row blocks"),
    MergeFwd(384, 1, 4, 64, (16, 4, 16, "slice-minor"), "KITTI deepest level, batch 1"),
    MergeFwd(384, 3, 4, 64, (16, 4, 16, "slice-minor"), "KITTI deepest level, batch 3"),
    MergeFwd(384, 1, 8, 64, (16, 4, 16, "xcd"), "8 row blocks"),
    MergeFwd(384, 8, 8, 256, (16, 1, 4, "xcd"), "KSPLIT 1"),
    MergeFwd(384, 129, 2, 64, (16, 1, 4, "slice-minor"), "KSPLIT 1, 258 row blocks"),
]


@dataclass(frozen=True)
class MergeBwd:
    Cp: int
    B: int
    H: int
    W: int
    crps: int                     # cast_rows_per_sample (fine tokens)

    @property
    def rows(self):
        return self.B * (self.H // 2) * (self.W // 2)

    @property
    def bm(self):
        return 32 if self.Cp == 96 else 16

    @property
    def name(self):
        return f"c{self.Cp}-{self.B}x{self.H}x{self.W}"


MERGE_BWD = [MergeBwd(96, 1, 2, 64, 128), MergeBwd(96, 3, 2, 64, 128), MergeBwd(96, 32, 2, 2, 4),
             MergeBwd(192, 1, 2, 64, 128), MergeBwd(192, 3, 2, 64, 128)]
CAST_VARIANTS = ("none", "scaled", "unscaled")           # dx_bf16 absent / with cast_rowscale / without


@dataclass(frozen=True)
class Unmerge:
    C: int
    B: int
    H: int
    W: int                        # the COARSE grid

    @property
    def M(self):
        return self.B * self.H * self.W

    @property
    def crps(self):
        return self.H * self.W

    @property
    def name(self):
        return f"c{self.C}-{self.B}x{self.H}x{self.W}"


UNMERGE = [Unmerge(C, *g) for C in (192, 384) for g in ((1, 1, 16), (1, 2, 8), (16, 1, 1), (4, 2, 2), (3, 4, 4))]


# ------------------------------------------------------------------ pieces
@dataclass
class Prob:
    op: str
    case: object
    ins: dict                     # name -> Buf inside NaN (operands), or a plain contiguous bf16 matrix (weights: packed by the caller)
    outs: dict                    # name -> Out
    ref: dict                     # float64 references and budgets
    ties: dict                    # bf16 tensor -> share of exact ties among its values


def _seed(*v):
    s = 77
    for x in v:
        s = (s * 1000003 + int(x)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _mat(rows, cols, dtype, fill, device, values=None, back=3):
    b = Buf(rows, cols, cols, dtype, fill, device, back=back)      # contiguous: the launches take no pitch for it
    return b.set(values) if values is not None else b


def _vec(n, fill, device, values=None):
    b = Buf(1, n, n + 8, F32, fill, device)
    return b.set(values.reshape(1, n)) if values is not None else b


def gemm64(A, Bt, add=None, quantum=1.0):
    """A [M][K] . Bt [N][K]^T (+ add) in float64, after asserting -- on |A| |Bt|^T + |add|, which bounds every partial sum in every
    order -- that the accumulation stays below 2^20 quanta; A holds multiples of `quantum`, Bt and add integers (times it)."""
    assert torch.equal(torch.round(A / quantum) * quantum, A) and torch.equal(torch.round(Bt), Bt)
    bound = float(A.abs().sum(1).max()) * float(Bt.abs().max())       # cheap; the matrix of bounds only where this is not enough
    if add is not None:
        bound += float(add.abs().max())
    if bound / quantum >= EXACT_LIMIT:
        b = A.abs() @ Bt.abs().t()
        bound = float((b + add.abs() if add is not None else b).max())
    assert bound / quantum < EXACT_LIMIT, bound / quantum
    out = A @ Bt.t()
    return (out + add if add is not None else out) + 0.0


def rounded(v64):
    return ND.round_bf16(v64).to(F64)


def merge_scatter(rows_t, B, H, W, C):
    """merged rows [B H/2 W/2][4C] -> the (B, H, W, C) tensor whose 2x2 patch merge gives those rows"""
    x = torch.empty(B, H, W, C, dtype=rows_t.dtype, device=rows_t.device)
    r = rows_t.reshape(B, H // 2, W // 2, 4, C)
    for k, (dh, dw) in enumerate(GATHER):
        x[:, dh::2, dw::2] = r[:, :, :, k]
    return x


def merge_gather(x, order=(0, 1, 2, 3)):
    """(B, H, W, C) -> merged rows [B H/2 W/2][4C], channel groups in PatchMerging's order (or a wrong one)"""
    parts = [x[:, dh::2, dw::2] for dh, dw in GATHER]
    return torch.cat([parts[o] for o in order], -1).reshape(-1, 4 * x.shape[-1])


def ln_rows(rows, K, gen):
    """merged rows [rows][K] (float64 integers) with sum 0 and variance + LN_EPS a power of 4, and their exact rstd"""
    kind = torch.randint(0, 3, (rows,), generator=gen)
    m = torch.tensor(ROW_MAGS, dtype=F64)[kind][:, None]
    one = torch.ones(rows, K // 4, dtype=F64)
    base = torch.cat([one, -one, m * one, -m * one], 1)
    v = base.gather(1, torch.rand(rows, K, generator=gen).argsort(1))
    rstd = torch.tensor(ROW_RSTD, dtype=F64)[kind]
    assert bool((v.sum(1) == 0).all()) and torch.equal(1 / torch.sqrt((v * v).mean(1) + LN_EPS), rstd)
    q = v.reshape(rows, 4, K // 4)
    for a in range(4):
        for b in range(a + 1, 4):
            assert bool((q[:, a] != q[:, b]).any(1).all()), "two sub-pixels of a row carry the same pattern"
    return v, rstd


def unshuf_tokens(M, N, psH, psW, device):
    """gemm_exact's inverse PixelShuffle map, both index tensors [M][N]"""
    tok, col = GX.unshuf_tokens(M, N, psH, psW, device)
    return tok.expand(M, N), col.expand(M, N)


def odd_ints(gen, n):
    return (2 * torch.randint(-2, 2, (n,), generator=gen) + 1).to(F64)           # {-3, -1, 1, 3}


def sample_scales(nsamp, gen):
    """one scale per sample, cyclic through SCALES from a seeded start: adjacent samples always differ; the first sample's is
    not 0 (a launch of one sample still shows its values)"""
    start = int(torch.randint(1, len(SCALES), (1,), generator=gen))
    return torch.tensor(SCALES, dtype=F64)[(torch.arange(nsamp) + start) % len(SCALES)]


# ------------------------------------------------------------------ builders
def build_merge_fwd(c: MergeFwd, device="cpu") -> Prob:
    gen = _seed(1, c.Cin, c.B, c.H, c.W)
    rows, K, N = c.rows, 4 * c.Cin, 2 * c.Cin
    v, rstd = ln_rows(rows, K, gen)
    gamma, beta = odd_ints(gen, K), GX.ints(gen, (K,), -4, 4, "cpu")
    w = GX.ints(gen, (N, K), -8, 8, "cpu")
    v, rstd, gamma, beta, w = (t.to(device) for t in (v, rstd, gamma, beta, w))
    term = v * rstd[:, None] * gamma
    xm = term + beta
    # exactly a bf16 value, and 16 fp32 ulp of the terms below half a bf16 ulp of it (in particular never 0)
    assert torch.equal(rounded(xm), xm) and torch.equal(torch.round(xm / XM_QUANTUM) * XM_QUANTUM, xm)
    assert bool((16 * ND.ulp_f32(term.abs() + beta.abs()) < 0.5 * ND.ulp_bf16(xm)).all())
    y = gemm64(xm, w, quantum=XM_QUANTUM)
    ins = {"x": _mat(c.B * c.H * c.W, c.Cin, F32, "nan", device, merge_scatter(v, c.B, c.H, c.W, c.Cin).reshape(-1, c.Cin)),
           "gamma": _vec(K, "nan", device, gamma), "beta": _vec(K, "nan", device, beta), "w": w.to(BF16).contiguous()}
    o_xm, o_y = _mat(rows, K, BF16, "guard", device), _mat(rows, N, F32, "guard", device)
    o_mean, o_rstd = _vec(rows, "guard", device), _vec(rows, "guard", device)
    o_y16 = Buf(rows, N, GX._pitch(N), BF16, "guard", device)                      # a pitch that is neither N nor 2N
    every = torch.ones(1, rows, dtype=torch.bool, device=device)
    outs = {"xm": Out(o_xm, GX._image(o_xm, o_xm.index(), xm), o_xm.index()),
            "mean": Out(o_mean, GX._image(o_mean, o_mean.index(), torch.zeros(1, rows, dtype=F64, device=device)), o_mean.index()),
            "rstd": Out(o_rstd, GX._image(o_rstd, o_rstd.index(), rstd[None, :], every), o_rstd.index(), every, "rstd", rstd[None, :]),
            "y": Out(o_y, GX._image(o_y, o_y.index(), y), o_y.index()),
            "y16": Out(o_y16, GX._image(o_y16, o_y16.index(), y), o_y16.index())}
    return Prob("merge_fwd", c, ins, outs, {"xm": xm, "y": y, "rstd": rstd}, {"y16": GX.tie_fraction(y)})


def build_merge_bwd(c: MergeBwd, device="cpu") -> Prob:
    gen = _seed(2, c.Cp, c.B, c.H, c.W)
    Cp, Cs, K4, rows, bm = c.Cp, 2 * c.Cp, 4 * c.Cp, c.rows, c.bm
    tokens = c.B * c.H * c.W
    v, rstd = ln_rows(rows, K4, gen)
    gamma = odd_ints(gen, K4)
    dx_in = GX.ints(gen, (rows, Cs), -512, 512, "cpu")
    dys, wskip = GX.ints(gen, (rows, Cs), -4, 4, "cpu"), GX.ints(gen, (Cs, 2 * Cs), -4, 4, "cpu")
    wred = GX.ints(gen, (Cs, K4), -2, 2, "cpu")
    nsamp = -(-tokens // c.crps)
    scale = sample_scales(nsamp, gen)
    dyb = rounded(gemm64(dys, wskip[:, Cs:].t().contiguous(), add=dx_in))          # dx_in + dy_skip . W_skip[:, Cs:]
    ties = {"dyb": GX.tie_fraction(gemm64(dys, wskip[:, Cs:].t().contiguous(), add=dx_in))}
    assert ties["dyb"] >= MIN_TIES, ties
    dn_exact = gemm64(dyb, wred.t().contiguous())                                   # dyb . W_red  [rows][4 Cp]
    ties["dnorm"] = GX.tie_fraction(dn_exact)
    dn = rounded(dn_exact)
    xh = v * rstd[:, None]                                                          # exact in the kernel too: mean 0, rstd 2^-k
    # every partial row is an fp32 sum over one row block: exact while sum |dn xhat| stays below 2^24 eighths
    assert float((dn * xh).abs().reshape(rows // bm, bm, K4).sum(1).max()) / XM_QUANTUM < 2.0 ** 24
    assert float(dn.abs().reshape(rows // bm, bm, K4).sum(1).max()) < 2.0 ** 24
    dgamma, dbeta = (dn * xh).sum(0), dn.sum(0)
    gy = dn * gamma
    dx = rstd[:, None] * (gy - gy.mean(1, keepdim=True) - xh * (gy * xh).mean(1, keepdim=True))
    f64, f32 = (ND.ln_torch(v, gamma, torch.zeros(K4, dtype=F64), dn, LN_EPS, t) for t in (F64, F32))
    assert float((f64["dx"] - dx).abs().max()) <= 1e-9 * float(dx.abs().max())    # the formula is torch's float64 autograd
    err32 = float((f32["dx"] - f64["dx"]).abs().max())
    budget = torch.maximum(torch.full((rows, 1), LN_FACTOR * err32, dtype=F64), ND.ulp_f32(dx.abs().amax(1, keepdim=True))).expand(rows, K4)
    to = lambda t: t.to(device)
    r_part = rows // bm
    ins = {"dx_in": _mat(rows, Cs, F32, "nan", device, dx_in), "dys": _mat(rows, Cs, BF16, "nan", device, dys),
           "wskip": wskip.to(BF16).contiguous().to(device), "wred": wred.to(BF16).contiguous().to(device),
           "x_prev": _mat(tokens, Cp, F32, "nan", device, merge_scatter(v, c.B, c.H, c.W, Cp).reshape(-1, Cp)),
           "mean": _vec(rows, "nan", device, torch.zeros(rows, dtype=F64)), "rstd": _vec(rows, "nan", device, rstd),
           "gamma": _vec(K4, "nan", device, gamma), "scale": _vec(nsamp, "nan", device, scale)}
    o_dyb, o_dx, o_c = _mat(rows, Cs, BF16, "guard", device), _mat(tokens, Cp, F32, "guard", device), _mat(tokens, Cp, BF16, "guard", device)
    o_part = _mat(r_part, 2 * K4, F32, "guard", device)
    # dx_prev / dx_bf16 in MERGED-row order: position [r][q Cp + ci] of the (B, H, W, Cp) tensor
    idx_m = merge_gather(o_dx.index().reshape(c.B, c.H, c.W, Cp))
    every = torch.ones(rows, K4, dtype=torch.bool, device=device)
    outs = {"dyb": Out(o_dyb, GX._image(o_dyb, o_dyb.index(), to(dyb)), o_dyb.index()),
            "dx": Out(o_dx, GX._ibits(o_dx.flat).clone(), idx_m, every, "ln_dx", to(dx)),
            "dx16": Out(o_c, None, merge_gather(o_c.index().reshape(c.B, c.H, c.W, Cp))),
            "part": Out(o_part, GX._ibits(o_part.flat).clone(), o_part.index(), torch.ones(r_part, 2 * K4, dtype=torch.bool, device=device), "partials")}
    ref = {"dyb": to(dyb), "dn": to(dn), "dx": to(dx), "budget": to(budget), "err32": err32, "dgamma": to(dgamma), "dbeta": to(dbeta),
           "scale": to(scale)}
    return Prob("merge_bwd", c, ins, outs, ref, ties)


def build_unmerge_fwd(c: Unmerge, device="cpu") -> Prob:
    gen = _seed(3, c.C, c.B, c.H, c.W)
    C, Cf, M = c.C, c.C // 2, c.M
    x, wexp, bexp = GX.ints(gen, (M, C), -8, 8, device), GX.ints(gen, (2 * C, C), -8, 8, device), GX.ints(gen, (1, 2 * C), -64, 64, device)
    xsave = GX.ints(gen, (4 * M, Cf), -8, 8, device)
    wskip, bskip = GX.ints(gen, (Cf, C), -4, 4, device), GX.ints(gen, (1, Cf), -64, 64, device)
    z = gemm64(x, wexp, add=bexp.expand(M, 2 * C))
    ties = {"cat": GX.tie_fraction(z)}
    assert ties["cat"] >= MIN_TIES, ties
    tok, ch = GX.pixshuf_tokens(M, 2 * C, c.H, c.W, device)
    first = torch.zeros(4 * M, Cf, dtype=F64, device=device)
    first[tok.reshape(-1), ch.reshape(-1)] = rounded(z).reshape(-1)
    out = gemm64(torch.cat([first, xsave], 1), wskip, add=bskip.expand(4 * M, Cf))
    ins = {"x": _mat(M, C, BF16, "nan", device, x), "wexp": wexp.to(BF16).contiguous(), "bexp": _vec(2 * C, "nan", device, bexp),
           "wskip": wskip.to(BF16).contiguous(), "bskip": _vec(Cf, "nan", device, bskip)}
    o_cat, o_out = _mat(4 * M, C, BF16, "guard", device), _mat(4 * M, Cf, F32, "guard", device)
    o_cat.view[:, Cf:] = xsave.to(BF16)                                            # read by the launch, and must survive it
    idx = o_cat.off + tok * o_cat.pitch + ch
    outs = {"cat": Out(o_cat, GX._image(o_cat, idx, z), idx), "out": Out(o_out, GX._image(o_out, o_out.index(), out), o_out.index())}
    return Prob("unmerge_fwd", c, ins, outs, {"z": z, "out": out}, ties)


def build_unmerge_bwd(c: Unmerge, device="cpu") -> Prob:
    gen = _seed(4, c.C, c.B, c.H, c.W)
    C, Cf, M = c.C, c.C // 2, c.M
    dys, wskip = GX.ints(gen, (4 * M, Cf), -8, 8, device), GX.ints(gen, (Cf, C), -8, 8, device)
    wexp = GX.ints(gen, (2 * C, C), -2, 2, device)
    nsamp = -(-M // c.crps)
    scale = sample_scales(nsamp, gen).to(device)
    dzf = gemm64(dys, wskip[:, :Cf].t().contiguous())                               # dy_skip . W_skip[:, :C/2]  [4M][C/2]
    ties = {"dz": GX.tie_fraction(dzf)}
    assert ties["dz"] >= MIN_TIES, ties
    tok, col = unshuf_tokens(4 * M, Cf, c.H, c.W, device)
    dz = torch.zeros(M, 2 * C, dtype=F64, device=device)
    dz[tok.reshape(-1), col.reshape(-1)] = rounded(dzf).reshape(-1)
    dx = gemm64(dz, wexp.t().contiguous())                                          # dz . We  [M][C]
    ins = {"dys": _mat(4 * M, Cf, BF16, "nan", device, dys), "wskip": wskip.to(BF16).contiguous(), "wexp": wexp.to(BF16).contiguous(),
           "scale": _vec(nsamp, "nan", device, scale)}
    o_dz, o_dx, o_c = _mat(M, 2 * C, BF16, "guard", device), _mat(M, C, F32, "guard", device), _mat(M, C, BF16, "guard", device)
    idz = o_dz.off + tok * o_dz.pitch + col
    outs = {"dz": Out(o_dz, GX._image(o_dz, idz, dzf), idz), "dx": Out(o_dx, GX._image(o_dx, o_dx.index(), dx), o_dx.index()),
            "dx16": Out(o_c, None, o_c.index())}
    s_row = scale[torch.arange(M, device=device) // c.crps][:, None]
    ties["dx16"] = GX.tie_fraction(dx * s_row)
    return Prob("unmerge_bwd", c, ins, outs, {"dzf": dzf, "dx": dx, "scale": scale}, ties)


BUILDERS = {"merge_fwd": build_merge_fwd, "merge_bwd": build_merge_bwd, "unmerge_fwd": build_unmerge_fwd, "unmerge_bwd": build_unmerge_bwd}


def fresh(pb: Prob, skip=True) -> dict:
    """the output allocations a launch (or the emulation) writes into: guard-filled copies; merge_bwd without the skip operand
    READS dyb, which then holds its values (and must still hold them afterwards)"""
    got = {k: o.buf.flat.clone() for k, o in pb.outs.items()}
    if pb.op == "merge_bwd" and not skip:
        got["dyb"] = pb.outs["dyb"].want.clone().view(BF16)
    return got


def cast_scale(pb: Prob, cast, pos, width):
    """the DropPath scale of the cast output at flat positions `pos` of a [tokens][width] allocation: scale[token / crps]"""
    b = pb.outs["dx16"].buf
    tokn = (pos - b.off) // width
    s = pb.ref["scale"][tokn // pb.case.crps]
    return s if cast == "scaled" else torch.ones_like(s)


# ------------------------------------------------------------------ checkers
def _finite_err(g64, want):
    return torch.where(torch.isfinite(g64), (g64 - want).abs(), torch.full_like(want, math.inf))


def check(pb: Prob, got: dict, y16=True, cast="scaled") -> list:
    """Reports of every output allocation of the launch: whole images as integers, the loose outputs by their predicates.
    y16 / cast name the options the launch ran with: an option not given leaves its allocation untouched."""
    reps = []
    dev = next(iter(got.values())).device
    for name, out in pb.outs.items():
        if name == "y16" and not y16 or name == "dx16" and cast == "none":
            untouched = Out(out.buf, GX._ibits(out.buf.flat).clone(), out.idx)
            reps.append(GX.check_out(f"{pb.case.name}.{name} (not given)", untouched, got[name]))
            continue
        if name == "dx16":
            # bf16(dx * scale) of the dx the launch itself stored (merge_bwd: dx_prev is not exact) / of the reference
            src = got["dx"][pb.outs["dx"].idx].to(F64) if pb.op == "merge_bwd" else pb.ref["dx"]
            s = cast_scale(pb, cast, out.idx, out.buf.cols)
            out = Out(out.buf, GX._image(out.buf, out.idx, src * s), out.idx)
        reps.append(GX.check_out(f"{pb.case.name}.{name}", out, got[name]))
        if out.kind == "rstd":
            rep = Report(f"{pb.case.name}.rstd")
            g, want = got[name][out.idx.reshape(-1)].to(F64), out.ref64.reshape(-1)
            r = ND._ratio(rep, _finite_err(g, want), 2 * ND.ulp_f32(want), want)
            ND._add(rep, r > 1, "rstd more than 2 fp32 ulp from the power of two", want)
            reps.append(rep)
        elif out.kind == "ln_dx":
            rep = Report(f"{pb.case.name}.dx_prev")
            g, want = got[name][out.idx].to(F64), out.ref64
            r = ND._ratio(rep, _finite_err(g, want), pb.ref["budget"], want)
            ND._add(rep, r > 1, f"dx_prev above max({LN_FACTOR} x torch-float32 error {pb.ref['err32']:.3e}, 1 fp32 ulp of the row's largest)", want)
            reps.append(rep)
        elif out.kind == "partials":
            rep = Report(f"{pb.case.name}.partials")
            p = got[name][out.idx]                                                  # [R][2 K4]
            K4 = p.shape[1] // 2
            stale = GX._ibits(p.contiguous()) == GX.GUARD32
            ND._add(rep, stale.any(1), "partial rows with words never written")
            ND._add(rep, ~torch.isfinite(p).all(1), "partial rows not finite")
            tot = torch.nan_to_num(p.to(F64), nan=math.inf).sum(0)
            ND._add(rep, tot[:K4] != pb.ref["dgamma"], "dgamma: the float64 sum of the partial rows is not the exact sum", pb.ref["dgamma"])
            ND._add(rep, tot[K4:] != pb.ref["dbeta"], "dbeta: the float64 sum of the partial rows is not the exact sum", pb.ref["dbeta"])
            rep.worst = math.inf if rep.violations else 0.0
            reps.append(rep)
    return reps


failures = GX.failures


# ------------------------------------------------------------------ a torch emulation of the four launches, with switchable defects
DEFECTS = ("gather_perm", "pixshuf_swapped", "unshuf_wrong_half", "bias_dropped", "no_mid_rounding", "truncate", "scale_off_by_one",
           "block_unwritten", "xsave_overwritten", "dgamma_dbeta_swapped", "stale_partial", "row_past_end")
APPLIES = {"merge_fwd": ("gather_perm", "truncate", "block_unwritten", "row_past_end"),
           "merge_bwd": ("gather_perm", "no_mid_rounding", "truncate", "scale_off_by_one", "block_unwritten", "dgamma_dbeta_swapped",
                         "stale_partial", "row_past_end"),
           "unmerge_fwd": ("pixshuf_swapped", "bias_dropped", "no_mid_rounding", "truncate", "block_unwritten", "xsave_overwritten",
                           "row_past_end"),
           "unmerge_bwd": ("unshuf_wrong_half", "no_mid_rounding", "truncate", "scale_off_by_one", "block_unwritten", "row_past_end")}
PERMUTED = (0, 2, 1, 3)


def _rnd(x32, defect):
    if defect == "truncate":
        return ND.cast_truncating(x32.contiguous().cpu()).to(x32.device).reshape(x32.shape)
    return x32.to(BF16)


def _store(got, out: Out, name, vals, idx, keep=None):
    """vals -> the allocation by address; keep: the source rows that are stored"""
    v = vals if vals.dtype == out.buf.flat.dtype else vals.to(out.buf.flat.dtype)
    if keep is not None:
        v, idx = v[keep], idx[keep]
    got[name][idx.reshape(-1)] = v.reshape(-1)


def _past_end(got, out: Out, name):
    b = out.buf
    p = b.off + b.rows * b.pitch
    got[name][p:p + b.cols] = 0


def _keep(rows, bm, defect):
    """source rows stored: all, or all but the last row block (block_unwritten)"""
    keep = torch.ones(rows, dtype=torch.bool)
    if defect == "block_unwritten":
        keep[rows - bm:] = False
    return keep


def _cast_index(pb, cast, pos, width, defect):
    """scale of each stored word of the cast output; scale_off_by_one: the NEXT token's sample (wrong on a sample's last token)"""
    b = pb.outs["dx16"].buf
    tokn = (pos - b.off) // width
    if defect == "scale_off_by_one":
        tokn = tokn + 1
    sc = pb.ins["scale"]
    s = sc.flat[sc.off + (tokn // pb.case.crps).clamp(max=sc.cols - 1)]
    return s if cast == "scaled" else torch.ones_like(s)


def emulate(pb: Prob, defect=None, y16=True, cast="scaled", skip=True) -> dict:
    """What a correct launch leaves in the output allocations, computed in fp32 from the operand allocations (every GEMM operand
    bf16, fp32 accumulation, LayerNorm with a rounded 1/K and torch's rsqrt), stored by address; `defect` breaks one thing."""
    assert defect is None or defect in APPLIES[pb.op], (pb.op, defect)
    c, got = pb.case, fresh(pb, skip)
    dev = pb.outs[next(iter(pb.outs))].buf.flat.device
    f = lambda name: pb.ins[name].view.to(F32)
    if pb.op == "merge_fwd":
        bm = merge_fwd_route(c.Cin, c.rows)[0]
        K = 4 * c.Cin
        rows_ = merge_gather(f("x").reshape(c.B, c.H, c.W, c.Cin), PERMUTED if defect == "gather_perm" else (0, 1, 2, 3))
        inv_k = torch.tensor(1.0 / K, dtype=F32, device=dev)
        mu = rows_.sum(1) * inv_k
        d = rows_ - mu[:, None]
        rs = torch.rsqrt((d * d).sum(1) * inv_k + torch.tensor(LN_EPS, dtype=F32, device=dev))
        xm = _rnd(d * rs[:, None] * f("gamma") + f("beta"), defect)
        y = xm.to(F32) @ pb.ins["w"].to(F32).t()
        keep = _keep(c.rows, bm, defect).to(dev)
        o = pb.outs
        _store(got, o["xm"], "xm", xm, o["xm"].idx, keep)
        _store(got, o["mean"], "mean", mu[None, :], o["mean"].idx, None)
        _store(got, o["rstd"], "rstd", rs[None, :], o["rstd"].idx, None)
        _store(got, o["y"], "y", y, o["y"].idx, keep)
        if y16:
            _store(got, o["y16"], "y16", _rnd(y, defect), o["y16"].idx, keep)
        if defect == "row_past_end":
            _past_end(got, o["y16"] if y16 else o["y"], "y16" if y16 else "y")
    elif pb.op == "merge_bwd":
        Cp, Cs, K4, rows, bm = c.Cp, 2 * c.Cp, 4 * c.Cp, c.rows, c.bm
        order = PERMUTED if defect == "gather_perm" else (0, 1, 2, 3)
        o = pb.outs
        if skip:
            dyb = _rnd(f("dx_in") + f("dys") @ pb.ins["wskip"].to(F32)[:, Cs:], defect)
            _store(got, o["dyb"], "dyb", dyb, o["dyb"].idx)
        else:
            dyb = got["dyb"][o["dyb"].idx]
        dn = dyb.to(F32) @ pb.ins["wred"].to(F32)
        dn = dn if defect == "no_mid_rounding" else _rnd(dn, defect).to(F32)
        xg = merge_gather(f("x_prev").reshape(c.B, c.H, c.W, Cp), order)
        xh = (xg - f("mean").reshape(-1, 1)) * f("rstd").reshape(-1, 1)
        gy = dn * f("gamma")
        inv_k = torch.tensor(1.0 / K4, dtype=F32, device=dev)
        m1, m2 = gy.sum(1, keepdim=True) * inv_k, (gy * xh).sum(1, keepdim=True) * inv_k
        dx = f("rstd").reshape(-1, 1) * (gy - m1 - xh * m2)
        keep = _keep(rows, bm, defect).to(dev)
        idx = merge_gather(o["dx"].buf.index().reshape(c.B, c.H, c.W, Cp), order)
        _store(got, o["dx"], "dx", dx, idx, keep)
        if cast != "none":
            idc = merge_gather(o["dx16"].buf.index().reshape(c.B, c.H, c.W, Cp), order)
            _store(got, o["dx16"], "dx16", _rnd(dx * _cast_index(pb, cast, idc, Cp, defect), defect), idc, keep)
        pg = (dn * xh).reshape(rows // bm, bm, K4).sum(1)
        pbeta = dn.reshape(rows // bm, bm, K4).sum(1)
        part = torch.cat([pbeta, pg] if defect == "dgamma_dbeta_swapped" else [pg, pbeta], 1)
        pk = torch.ones(rows // bm, dtype=torch.bool, device=dev)
        if defect in ("stale_partial", "block_unwritten"):
            pk[-1] = False
        _store(got, o["part"], "part", part, o["part"].idx, pk)
        if defect == "row_past_end":
            _past_end(got, o["part"], "part")
    elif pb.op == "unmerge_fwd":
        C, Cf, M = c.C, c.C // 2, c.M
        o = pb.outs
        z = f("x") @ pb.ins["wexp"].to(F32).t()
        if defect != "bias_dropped":
            z = z + f("bexp")
        tok, ch = GX.pixshuf_tokens(M, 2 * C, c.H, c.W, dev, swap=defect == "pixshuf_swapped")
        cat = o["cat"].buf
        keep = _keep(M, 16, defect).to(dev)
        zb = _rnd(z, defect)
        _store(got, o["cat"], "cat", zb, cat.off + tok * cat.pitch + ch, keep)
        if defect == "xsave_overwritten":
            got["cat"][(cat.off + tok * cat.pitch + Cf + ch).reshape(-1)] = zb.reshape(-1)
        first = torch.zeros(4 * M, Cf, dtype=F32, device=dev)
        first[tok.reshape(-1), ch.reshape(-1)] = (z if defect == "no_mid_rounding" else zb.to(F32)).reshape(-1)
        full = torch.cat([first, cat.view[:, Cf:].to(F32)], 1)
        out = full @ pb.ins["wskip"].to(F32).t() + f("bskip")
        fine_keep = torch.zeros(4 * M, dtype=torch.bool, device=dev)
        fine_keep[tok[keep].reshape(-1)] = True
        _store(got, o["out"], "out", out, o["out"].idx, fine_keep)
        if defect == "row_past_end":
            _past_end(got, o["out"], "out")
    else:
        C, Cf, M = c.C, c.C // 2, c.M
        o = pb.outs
        ws = pb.ins["wskip"].to(F32)
        dzf = f("dys") @ (ws[:, Cf:] if defect == "unshuf_wrong_half" else ws[:, :Cf])
        tok, col = unshuf_tokens(4 * M, Cf, c.H, c.W, dev)
        keep = _keep(M, 16, defect).to(dev)
        fine_keep = keep[tok[:, 0]]
        zb = _rnd(dzf, defect)
        b = o["dz"].buf
        _store(got, o["dz"], "dz", zb, b.off + tok * b.pitch + col, fine_keep)
        dz = torch.zeros(M, 2 * C, dtype=F32, device=dev)
        dz[tok.reshape(-1), col.reshape(-1)] = (dzf if defect == "no_mid_rounding" else zb.to(F32)).reshape(-1)
        dx = dz @ pb.ins["wexp"].to(F32)
        _store(got, o["dx"], "dx", dx, o["dx"].idx, keep)
        if cast != "none":
            idc = o["dx16"].idx
            _store(got, o["dx16"], "dx16", _rnd(dx * _cast_index(pb, cast, idc, C, defect), defect), idc, keep)
        if defect == "row_past_end":
            _past_end(got, o["dx"], "dx")
    return got


def cases_of(op):
    return {"merge_fwd": MERGE_FWD, "merge_bwd": MERGE_BWD, "unmerge_fwd": UNMERGE, "unmerge_bwd": UNMERGE}[op]

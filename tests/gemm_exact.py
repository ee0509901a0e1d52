"""Exact tests of tulip_gemm_bf16, tulip_wgrad_group and tulip_reduce_rows_multi: operand builders, float64 references, checkers
and a torch emulation with switchable defects (test_gemm_exact_cpu.py proves the checkers sharp and the case list complete,
test_gemm_exact_gpu.py applies them to the kernels).  Plain torch, on whichever device the caller names; no kernel code.

The device of it all: INTEGER operands.  A and B hold integers in [-8, 8], the bias integers in [-64, 64], residual and
accumulate-into values integers, row scales come from {0, 0.5, 1, 1.25, 2}; every partial and final value stays below 2^20, so
fp32 accumulation is exact in ANY order (1.25 costs two fractional bits: 22 <= 24).  Every fp32 output must then equal the float64
result bit for bit, every bf16 output its single round-to-nearest-even -- whatever the tile, the stage depth, the split count or the
kernel.  The builders assert (from the reference alone) the magnitude bound and that at least 1 % of the bf16 outputs of a case are
exact ties between two bf16 neighbours: the rounding mode is really exercised.

Beside the tensors: every logical tensor sits inside a larger allocation (rows in front and behind, a pitch larger than the row).
Around OPERANDS the allocation is NaN -- a kernel that reads outside its operand poisons its result.  Around OUTPUTS (and in the
outputs themselves unless the case accumulates, and in the workspace past the required bytes) it holds a fixed non-canonical NaN
pattern; the expected image of the WHOLE allocation is built from the reference and compared as integers, so a wrong value, a store
into a pitch gap, a row past the last row and a write past the workspace are all the same finding: a word that differs."""
import math
from dataclasses import dataclass, field, replace

import torch

from tests import numerics_domain as ND
from tests.numerics_domain import Report
from tulip_amd._lib import (EPI_BF16, EPI_F32, EPI_GELU_BWD, EPI_GELU_DUAL, EPI_PIXSHUF2_F32, EPI_RESID_F32, EPI_SPLIT_F32,
                            EPI_UNSHUF2_BF16, ROUTE_A_TRANS, ROUTE_B_TRANS, ROUTE_DEEP, ROUTE_FOLD, ROUTE_FULL, ROUTE_MID,
                            ROUTE_SPLITS_SHIFT, ROUTE_STREAM, ROUTE_TILE)

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
GUARD32 = 0x7FC5A5A5          # a quiet NaN whose payload no arithmetic produces
GUARD16 = 0x7FA5
BN = 96                       # column tile of the tile families
EXACT_LIMIT = 2.0 ** 20
MIN_TIES = 0.01
ROWSCALES = (0.0, 0.5, 1.0, 1.25, 2.0)
EPI_NAMES = {EPI_BF16: "bf16", EPI_GELU_DUAL: "gelu_dual", EPI_GELU_BWD: "gelu_bwd", EPI_F32: "f32", EPI_RESID_F32: "resid",
             EPI_PIXSHUF2_F32: "pixshuf", EPI_SPLIT_F32: "split", EPI_UNSHUF2_BF16: "unshuf"}
EPIS = tuple(EPI_NAMES)


# ------------------------------------------------------------------ routes (the bit field of tulip_gemm_route, tulip_hip.h)
STREAM_DEPTHS = (96, 384, 768, 1536)
TILE_ROWS = (64, 128, 256)


def route_key(r):
    """bit field -> (family, variant, deep, a_trans, b_trans): what names a kernel instantiation"""
    return (r & 3, (r >> 2) & 3, bool(r & ROUTE_DEEP), bool(r & ROUTE_A_TRANS), bool(r & ROUTE_B_TRANS))


def route_name(r):
    fam, var, deep, at, bt = route_key(r)
    lay = ("t" if at else "n") + ("t" if bt else "n")
    if fam == ROUTE_MID:
        s = "mid"
    elif fam == ROUTE_STREAM:
        s = f"stream{STREAM_DEPTHS[var]}"
    else:
        s = ("full" if fam == ROUTE_FULL else "tile") + str(TILE_ROWS[var]) + ("-deep" if deep else "")
    return f"{s}/{lay}"


def route_splits(r):
    return r >> ROUTE_SPLITS_SHIFT


def route_folds(r):
    return bool(r & ROUTE_FOLD)


def reachable_routes():
    """every kernel instantiation behind tulip_gemm_bf16, as route names -- enumerated from the header's encoding: the tile family
    at 64 / 128 rows in four layouts and at 256 rows without a transposed A, 128-deep stages at 64 rows only; the unchecked twins without a transposed A; the mid
    kernel in both B layouts; the stream kernel at four depths"""
    out = set()
    for at in (False, True):
        for bt in (False, True):
            lay = ("t" if at else "n") + ("t" if bt else "n")
            for rows in TILE_ROWS:
                if rows == 256 and at:
                    continue                     # (a k-slow LDS tile holds 128 rows: no 256-row tile with a transposed A)
                out.add(f"tile{rows}/{lay}")
                if not at:
                    out.add(f"full{rows}/{lay}")
            out.add(f"tile64-deep/{lay}")
            if not at:
                out.add(f"full64-deep/{lay}")
    out |= {"mid/nn", "mid/nt"} | {f"stream{d}/nn" for d in STREAM_DEPTHS}
    return out


def route_accepts(route, epi):
    """the launcher runs this epilogue on this route (the mid kernel has no PixelShuffle write-outs)"""
    return not (route.startswith("mid") and epi in (EPI_PIXSHUF2_F32, EPI_UNSHUF2_BF16))


def tile_rows_of(route):
    s = route.split("/")[0]
    return 192 if s == "mid" else 32 if s.startswith("stream") else int("".join(c for c in s.split("-")[0] if c.isdigit()))


def tile_cols_of(route):
    return 192 if route.startswith("mid") else BN


def plan_splits(K, splits):
    """(K range per split, splits launched): K is cut in multiples of 32 (tulip_gemm_effective_splits)"""
    splits = max(1, splits)
    kchunk = (-(-K // splits) + 31) // 32 * 32
    return kchunk, -(-K // kchunk)


# ------------------------------------------------------------------ allocations
def _ibits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def filled(n, dtype, fill, device):
    """n elements of `dtype`: 'nan', 'guard' (the non-canonical NaN pattern) or a number"""
    if fill == "guard":
        if dtype == BF16:
            return torch.full((n,), GUARD16, dtype=torch.int16, device=device).view(BF16)
        return torch.full((n,), GUARD32, dtype=torch.int32, device=device).view(dtype)
    return torch.full((n,), float("nan") if fill == "nan" else fill, dtype=dtype, device=device)


class Buf:
    """a logical [rows][cols] tensor inside a flat allocation of (front + rows + back) rows of `pitch` elements"""

    def __init__(self, rows, cols, pitch, dtype, fill, device, front=2, back=3):
        assert pitch >= cols
        self.rows, self.cols, self.pitch, self.off = rows, cols, pitch, front * pitch
        self.flat = filled((front + rows + back) * pitch, dtype, fill, device)

    @property
    def view(self):
        return self.flat.as_strided((self.rows, self.cols), (self.pitch, 1), self.off)

    def set(self, values):
        self.view.copy_(values.to(self.flat.dtype))
        return self

    def index(self):
        """flat positions of the logical elements, [rows][cols]"""
        d = self.flat.device
        return self.off + torch.arange(self.rows, device=d)[:, None] * self.pitch + torch.arange(self.cols, device=d)[None, :]

    def addr(self, flat=None):
        f = self.flat if flat is None else flat
        return f.data_ptr() + self.off * f.element_size()


def ints(gen, shape, lo, hi, device):
    return torch.randint(lo, hi + 1, shape, generator=gen).to(F64).to(device)


# ------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    name: str
    M: int
    N: int
    K: int
    route: str = ""               # the kernel this shape must reach (route_name), written next to the shape
    a_trans: bool = False
    b_trans: bool = False
    epi: int = EPI_BF16
    splits: int = 1
    accumulate: bool = False
    bias: bool = True
    out2: bool = False            # F32 / RESID / PIXSHUF: the bf16 second output; a_trans with F32 / SPLIT: the row sums
    rowscale: bool = False
    rps: int = 1
    ps: tuple = (0, 0)            # psH, psW (the coarse grid of both shuffles)
    out1: bool = True             # PIXSHUF: the fp32 output is given
    odd_pitch: bool = False       # the scattered (unaligned) write-out of the shuffles: ldo2 % 8 != 0 / ldo odd
    checked: bool = False
    mid: bool = False
    packed: bool = False
    tight_out: bool = False       # ldo == N (SPLIT slabs that tulip_reduce_splits folds)
    seed: int = 0

    @property
    def id(self):
        return self.name

    def flags(self):
        return dict(checked=self.checked, mid=True if self.mid else None, b_packed=self.packed)

    def route_args(self):
        return dict(a_trans=self.a_trans, b_trans=self.b_trans, epi=self.epi, accumulate=self.accumulate, splits=self.splits,
                    **self.flags())


def rowsum_form(c: Case) -> bool:
    """out2 receives the row sums of opA (fp32, ldo2 = 0) instead of a bf16 copy: the weight-gradient form, a_trans with
    TULIP_EPI_F32 or TULIP_EPI_SPLIT_F32"""
    return c.out2 and c.a_trans and c.epi in (EPI_F32, EPI_SPLIT_F32)


def addressed(c: Case) -> dict:
    """what the launch addresses, from the header: name -> (dtype, rows, columns) of `out`, `out2` and `aux`.  The GPU test
    asserts every allocation against it before the call: a builder mistake must not become a store out of bounds."""
    M, N = c.M, c.N
    eff = plan_splits(c.K, c.splits)[1]
    d = {}
    if c.epi in (EPI_BF16, EPI_GELU_DUAL, EPI_GELU_BWD):
        d["out"] = (BF16, M, N)
        if c.epi == EPI_GELU_DUAL:
            d["out2"] = (BF16, M, N)
        if c.epi == EPI_GELU_BWD:
            d["aux"] = (BF16, M, N)
    elif c.epi in (EPI_F32, EPI_RESID_F32):
        d["out"] = (F32, M, N)
        if c.out2:
            d["out2"] = (F32, 1, M) if rowsum_form(c) else (BF16, M, N)
        if c.epi == EPI_RESID_F32:
            d["aux"] = (F32, M, N)
    elif c.epi == EPI_SPLIT_F32:
        d["out"] = (F32, eff * M, N)
        if c.out2:
            assert rowsum_form(c)
            d["out2"] = (F32, eff, M)
    elif c.epi == EPI_PIXSHUF2_F32:
        if c.out1:
            d["out"] = (F32, 4 * M, N // 4)
        if c.out2:
            d["out2"] = (BF16, 4 * M, N // 4)
    elif c.epi == EPI_UNSHUF2_BF16:
        d["out"] = (BF16, M // 4, 4 * N)
    return d


def shuffle_grid(M, fine):
    """(B, psH, psW) with B psH psW == M (PixelShuffle: rows are coarse tokens) or 4 B psH psW == M (its inverse: fine tokens)"""
    n = M // 4 if fine else M
    assert not fine or M % 4 == 0
    for B in (2, 3, 1):
        if n % B == 0:
            q = n // B
            h = int(math.isqrt(q))
            while q % h:
                h -= 1
            if h > 1 or q < 4:
                return B, h, q // h
    raise AssertionError(f"no grid for {M}")


def with_epilogue(base: Case, epi, variant=0) -> Case:
    """`base` (shape, layout, flags, route) with epilogue `epi` fully specified.  variant 1 switches the options that have two
    forms: accumulate, the unaligned scatter pitch, the PixelShuffle without its fp32 output."""
    kw = dict(epi=epi, name=f"{base.name}-{EPI_NAMES[epi]}" + ("-v1" if variant else ""), bias=True)
    M = base.M
    if epi == EPI_GELU_BWD:
        kw.update(bias=False)
    elif epi == EPI_F32:
        # the weight-gradient form (a_trans) spends out2 on the row sums; elsewhere it is the bf16 copy at a pitch of its own
        # (the row sums exist unsplit or as TULIP_EPI_SPLIT_F32 slabs: a folded launch refuses them)
        folds = plan_splits(base.K, base.splits)[1] > 1
        kw.update(out2=not (base.a_trans and folds), rowscale=not base.a_trans, rps=24, accumulate=bool(variant),
                  bias=not base.a_trans)
    elif epi == EPI_RESID_F32:
        kw.update(out2=not variant, rowscale=True, rps=40)
    elif epi == EPI_PIXSHUF2_F32:
        B, h, w = shuffle_grid(M, fine=False)
        kw.update(ps=(h, w), out2=True, out1=not variant, odd_pitch=bool(variant))
    elif epi == EPI_UNSHUF2_BF16:
        B, h, w = shuffle_grid(M, fine=True)
        kw.update(ps=(h, w), odd_pitch=bool(variant), bias=bool(variant))
    elif epi == EPI_SPLIT_F32:
        kw.update(bias=False, out2=base.a_trans)
    return replace(base, **kw)


# ------------------------------------------------------------------ a problem: operands, outputs, expected images
@dataclass
class Out:
    buf: Buf
    want: torch.Tensor                 # expected bit image of buf.flat (int16 / int32)
    idx: torch.Tensor                  # flat positions of the logical elements, shaped like the logical result
    loose: torch.Tensor = None         # bool, shaped like idx: elements checked by a predicate of their own, not bit for bit
    kind: str = "exact"                # "exact" | "gelu_bwd" | "gelu_dual"
    ref64: torch.Tensor = None         # loose elements: the float64 value


@dataclass
class Problem:
    case: Case
    A: Buf
    B: Buf
    bias: Buf
    aux: Buf
    rowscale: Buf
    outs: dict
    ws: torch.Tensor                   # workspace: exactly the required floats, then guard words (None: no fold)
    ws_need: int
    acc: torch.Tensor                  # the exact [M][N] product, float64
    ties: float
    lda: int = 0
    ldb: int = 0


def tie_fraction(v64):
    q = v64.abs() / ND.ulp_bf16(v64)
    return float(((q - torch.floor(q)) == 0.5).to(F64).mean()) if v64.numel() else 0.0


def _pitch(cols, mult=8, extra=2):
    """a pitch larger than the row by at least 8 elements, a multiple of `mult`"""
    return (cols + 8 + extra * mult + mult - 1) // mult * mult


def pixshuf_tokens(M, N, psH, psW, device, swap=False):
    """[M][N] -> (fine token, channel) of the PixelShuffle(2) scatter: m = (b, h, w), n = 4c + 2i + j -> (b, 2h + i, 2w + j), c"""
    m = torch.arange(M, device=device)[:, None]
    n = torch.arange(N, device=device)[None, :]
    w, t = m % psW, m // psW
    h, b = t % psH, t // psH
    c, i, j = n // 4, (n // 2) % 2, n % 2
    if swap:
        i, j = j, i
    return (b * 2 * psH + 2 * h + i) * (2 * psW) + 2 * w + j, c.expand(M, N)


def unshuf_tokens(M, N, psH, psW, device):
    """[M][N] -> (coarse token, column): m = (b, 2h + i, 2w + j), n = c -> (b, h, w), 4c + 2i + j"""
    m = torch.arange(M, device=device)[:, None]
    n = torch.arange(N, device=device)[None, :]
    wf, t = m % (2 * psW), m // (2 * psW)
    hf, b = t % (2 * psH), t // (2 * psH)
    return (b * psH + hf // 2) * psW + wf // 2, 4 * n + 2 * (hf % 2) + (wf % 2)


def _bits_of(v64, dtype):
    """float64 exact values -> the bit image of their one rounding to `dtype`"""
    if dtype == BF16:
        return _ibits(ND.round_bf16(v64).contiguous())
    f = v64.to(F32)
    assert torch.equal(f.to(F64), v64), "an fp32 output of these tests is exactly representable"
    return _ibits(f.contiguous())


def _image(buf, idx, v64, loose=None):
    """expected image of the allocation: what it holds now, with the logical elements replaced by the rounding of v64"""
    want = _ibits(buf.flat).clone()
    bits = _bits_of(v64, buf.flat.dtype)          # (signed zeros as float64 arithmetic leaves them: -3 * 0.0 is -0.0 in fp32 too)
    if loose is None:
        want[idx.reshape(-1)] = bits.reshape(-1)
    else:
        keep = ~loose.reshape(-1)
        want[idx.reshape(-1)[keep]] = bits.reshape(-1)[keep]
    return want


def build(case: Case, device="cpu") -> Problem:
    c = case
    gen = torch.Generator().manual_seed(1000 + c.seed + 7 * c.M + 13 * c.N + 31 * c.K + 101 * c.epi + c.splits)
    M, N, K = c.M, c.N, c.K
    kchunk, eff = plan_splits(K, c.splits)
    # operands inside NaN
    ar, ac = (K, M) if c.a_trans else (M, K)
    br, bc = (K, N) if c.b_trans else (N, K)
    A = Buf(ar, ac, _pitch(ac), BF16, "nan", device).set(ints(gen, (ar, ac), -8, 8, device))
    B = Buf(br, bc, _pitch(bc), BF16, "nan", device).set(ints(gen, (br, bc), -8, 8, device))
    A64 = A.view.to(F64).t() if c.a_trans else A.view.to(F64)
    B64 = B.view.to(F64).t() if c.b_trans else B.view.to(F64)
    acc = A64 @ B64.t() + 0.0
    bias = Buf(1, N, N + 8, F32, "nan", device).set(ints(gen, (1, N), -64, 64, device)) if c.bias else None
    v = acc + bias.view.to(F64) if c.bias else acc
    nsamp = -(-M // max(1, c.rps))
    rowscale = None
    s_row = torch.ones(M, 1, dtype=F64, device=device)
    if c.rowscale:
        # (cyclic from a random start: a case of few samples still sees several scales, 0 among them only once in five)
        pick = ((torch.arange(nsamp) + 1 + int(torch.randint(0, 4, (1,), generator=gen))) % len(ROWSCALES))[None, :]
        rowscale = Buf(1, nsamp, nsamp + 4, F32, "nan", device).set(torch.tensor(ROWSCALES, dtype=F64)[pick].to(device))
        s_row = rowscale.view.to(F64).reshape(-1)[torch.arange(M, device=device) // c.rps][:, None]
    aux, outs, rounded = None, {}, []

    def plain(dtype, cols=N, rows=M, mult=8, tight=False):
        return Buf(rows, cols, cols if tight else _pitch(cols, mult), dtype, "guard", device)

    if c.epi == EPI_BF16:
        o = plain(BF16)
        outs["out"] = Out(o, _image(o, o.index(), v), o.index())
        rounded.append(v)
    elif c.epi == EPI_GELU_DUAL:
        o, o2 = plain(BF16), plain(BF16)
        outs["out"] = Out(o, _image(o, o.index(), v), o.index())
        every = torch.ones(M, N, dtype=torch.bool, device=device)
        outs["out2"] = Out(o2, _image(o2, o2.index(), v, every), o2.index(), every, "gelu_dual")
        rounded.append(v)
    elif c.epi == EPI_GELU_BWD:
        pick = torch.randint(0, 3, (M, N), generator=gen).to(device)
        a64 = torch.tensor([0.0, 16.0, -16.0], dtype=F64, device=device)[pick]
        aux = Buf(M, N, _pitch(N), BF16, "nan", device).set(a64)
        o = plain(BF16)
        loose = a64 != 0
        ref = torch.where(loose, v * ND.gelu_grad_ref(a64), v / 2)
        outs["out"] = Out(o, _image(o, o.index(), ref, loose), o.index(), loose, "gelu_bwd", ref)
        rounded.append((v / 2)[~loose])
    elif c.epi in (EPI_F32, EPI_RESID_F32):
        o = plain(F32, mult=4)
        if c.epi == EPI_RESID_F32:
            aux = Buf(M, N, _pitch(N, 4), F32, "nan", device).set(ints(gen, (M, N), -1000, 1000, device))
            res = aux.view.to(F64) + s_row * v
            copy = res                               # the bf16 copy of the stored stream (the scale is inside the result)
        else:
            res = v
            if c.accumulate:
                o.set(ints(gen, (M, N), -1000, 1000, device))
                res = o.view.to(F64) + v
            copy = res * s_row
        outs["out"] = Out(o, _image(o, o.index(), res), o.index())
        if c.out2 and not rowsum_form(c):
            o2 = plain(BF16)
            outs["out2"] = Out(o2, _image(o2, o2.index(), copy), o2.index())
            rounded.append(copy)
        elif c.out2:                                  # weight-gradient form: row sums of opA = sum over k, as fp32 [M]
            rs = Buf(1, M, M + 8, F32, "guard", device)
            sums = A64.sum(1)[None, :]
            if c.accumulate:
                rs.set(ints(gen, (1, M), -1000, 1000, device))
                sums = rs.view.to(F64) + sums
            outs["out2"] = Out(rs, _image(rs, rs.index(), sums), rs.index())
    elif c.epi == EPI_SPLIT_F32:
        o = Buf(eff * M, N, N if c.tight_out else _pitch(N, 4), F32, "guard", device)
        slabs = torch.stack([A64[:, z * kchunk:min(K, (z + 1) * kchunk)] @ B64[:, z * kchunk:min(K, (z + 1) * kchunk)].t()
                             for z in range(eff)]) + 0.0
        outs["out"] = Out(o, _image(o, o.index(), slabs.reshape(eff * M, N)), o.index())
        if c.out2:                                    # row sums per split, [splits][M]
            rs = Buf(eff, M, M, F32, "guard", device)
            sums = torch.stack([A64[:, z * kchunk:min(K, (z + 1) * kchunk)].sum(1) for z in range(eff)])
            outs["out2"] = Out(rs, _image(rs, rs.index(), sums), rs.index())
    elif c.epi == EPI_PIXSHUF2_F32:
        psH, psW = c.ps
        assert M % (psH * psW) == 0 and N % 4 == 0
        tok, ch = pixshuf_tokens(M, N, psH, psW, device)
        if c.out1:
            o = Buf(4 * M, N // 4, N // 4, F32, "guard", device)          # (B, 2H, 2W, C_out), contiguous by definition
            idx = o.off + tok * o.pitch + ch
            outs["out"] = Out(o, _image(o, idx, v), idx)
        if c.out2:
            p2 = _pitch(N // 4) + (4 if c.odd_pitch else 0)
            o2 = Buf(4 * M, N // 4, p2, BF16, "guard", device)
            idx2 = o2.off + tok * o2.pitch + ch
            outs["out2"] = Out(o2, _image(o2, idx2, v), idx2)
            rounded.append(v)
    elif c.epi == EPI_UNSHUF2_BF16:
        psH, psW = c.ps
        assert M % (4 * psH * psW) == 0
        tok, col = unshuf_tokens(M, N, psH, psW, device)
        o = Buf(M // 4, 4 * N, _pitch(4 * N) + (1 if c.odd_pitch else 0), BF16, "guard", device,
                front=3 if c.odd_pitch else 2)
        idx = o.off + tok * o.pitch + col
        outs["out"] = Out(o, _image(o, idx, v), idx)
        rounded.append(v)
    else:
        raise AssertionError(c.epi)
    # conditions on the data, from the reference alone
    big = max([float(acc.abs().max())] + [float(x.abs().max()) for x in rounded if x.numel()])
    for out in outs.values():
        if out.buf.flat.dtype == F32:
            big = max(big, float(out.want.view(F32)[out.idx.reshape(-1)].abs().max()))
    assert big < EXACT_LIMIT, (c.name, big)
    ties = tie_fraction(torch.cat([x.reshape(-1) for x in rounded])) if rounded else 1.0
    assert ties >= MIN_TIES, f"{c.name}: only {ties:.4f} of the bf16 outputs are exact ties"
    fold = eff > 1 and c.epi != EPI_SPLIT_F32
    need = eff * M * N if fold else 0
    ws = filled(need + 64, F32, "guard", device) if fold else None
    return Problem(c, A, B, bias, aux, rowscale, outs, ws, need, acc, ties, A.pitch, B.pitch)


# ------------------------------------------------------------------ checkers
def _locate(out: Out, pos, case_route):
    """a flat position of an output allocation in words: logical element + tile coordinates, or the guard word it is"""
    hit = (out.idx.reshape(-1) == pos).nonzero()
    if hit.numel():
        e = int(hit[0])
        ncol = out.idx.shape[-1]
        m, n = e // ncol, e % ncol
        tr, tc = tile_rows_of(case_route) if case_route else 64, tile_cols_of(case_route) if case_route else BN
        return f"element [{m}][{n}] (tile ({m // tr}, {n // tc}), row {m % tr}, column {n % tc} of it)"
    b = out.buf
    return f"guard word {pos} (allocation row {pos // b.pitch - b.off // b.pitch}, column {pos % b.pitch}; logical {b.rows} x {b.cols})"


def check_out(name, out: Out, got_flat, route="") -> Report:
    """the whole allocation after the launch against its expected image, as integers; loose elements by their own predicate"""
    rep = Report(name)
    got = _ibits(got_flat.contiguous())
    want = out.want
    exact = torch.ones_like(want, dtype=torch.bool)
    if out.loose is not None:
        exact[out.idx.reshape(-1)[out.loose.reshape(-1)]] = False
    bad = exact & (got != want)
    nbad = int(bad.sum())
    if nbad:
        pos = int(bad.nonzero()[0])
        logical = torch.zeros_like(bad)
        logical[out.idx.reshape(-1)] = True
        nguard = int((bad & ~logical).sum())
        rep.violations.append(f"{nbad} words differ ({nguard} of them guard words); first: {_locate(out, pos, route)} holds "
                              f"{int(got[pos]) & 0xFFFFFFFF:#x}, expected {int(want[pos]) & 0xFFFFFFFF:#x}")
        rep.worst, rep.where = math.inf, _locate(out, pos, route)
    if out.kind == "gelu_bwd" and bool(out.loose.any()):
        # one bf16 ulp: one fp32 ulp of error in the factor (far below half a bf16 ulp of the product), then one rounding
        sel = out.loose.reshape(-1)
        g = got_flat[out.idx.reshape(-1)[sel]].to(F64)
        w = ND.round_bf16(out.ref64.reshape(-1)[sel]).to(F64)
        err = torch.where(torch.isfinite(g), (g - w).abs(), torch.full_like(w, math.inf))
        r = ND._ratio(rep, err, ND.ulp_bf16(w), w)
        ND._add(rep, r > 1, "GELU_BWD more than one bf16 ulp from bf16(acc * gelu'(aux))", w)
    return rep


def check_gelu_dual(out: Out, got_out_flat, stored: Out, got2_flat) -> Report:
    """out2 = bf16(gelu(out)) on the STORED out (numerics_domain.check_gelu)"""
    x = got_out_flat[stored.idx.reshape(-1)]
    y = got2_flat[out.idx.reshape(-1)]
    return ND.check_gelu(x, y, what="GELU_DUAL out2")


def check_ws(pb: Problem, got_ws) -> Report:
    rep = Report("workspace")
    if pb.ws is None:
        return rep
    tail = _ibits(got_ws.contiguous())[pb.ws_need:]
    bad = tail != _ibits(pb.ws)[pb.ws_need:]
    if bool(bad.any()):
        pos = int(bad.nonzero()[0])
        rep.violations.append(f"{int(bad.sum())} guard words past the required {pb.ws_need * 4} workspace bytes changed; first: word "
                              f"{pb.ws_need + pos}")
        rep.worst, rep.where = math.inf, f"workspace word {pb.ws_need + pos}"
    return rep


def check_all(pb: Problem, got: dict, route="") -> list:
    """got: name -> the allocation after the launch ('out', 'out2', 'ws').  Reports of every output of the case."""
    reps = []
    for name, out in pb.outs.items():
        reps.append(check_out(f"{pb.case.name}.{name}", out, got[name], route or pb.case.route))
        if out.kind == "gelu_dual":
            reps.append(check_gelu_dual(out, got["out"], pb.outs["out"], got[name]))
    if pb.ws is not None:
        reps.append(check_ws(pb, got["ws"]))
    return reps


def failures(reps):
    return [str(r) for r in reps if not r.ok]


# ------------------------------------------------------------------ a torch emulation of the launch, with switchable defects
DEFECTS = ("truncate", "half_away", "drop_k_tail", "overread_last_split", "row_past_m", "pitch_spill", "ldb_is_k",
           "bias_per_split", "fold_skips_slab0", "accumulate_ignored", "pixshuf_swapped")


def _round_f32_bf16(x32, defect):
    if defect == "truncate":
        return ND.cast_truncating(x32.cpu()).to(x32.device).reshape(x32.shape)
    if defect == "half_away":
        b = (_ibits(x32.contiguous()).to(torch.int64) & 0xFFFFFFFF) + 0x8000
        return ND.bf16_from_bits(((b >> 16) & 0xFFFF).cpu().numpy()).to(x32.device).reshape(x32.shape)
    return x32.to(BF16)


def _gelu32(x32):
    return 0.5 * x32 * (1 + torch.erf(x32 * ND.SQRT1_2))


def _gelu_grad32(x32):
    return 0.5 * (1 + torch.erf(x32 * ND.SQRT1_2)) + x32 * torch.exp(-0.5 * x32 * x32) * ND.INV_SQRT_2PI


def emulate(pb: Problem, defect=None) -> dict:
    """What a correct kernel leaves in the output allocations: fp32 accumulation over 32-deep k chunks, the K range cut as the
    launcher cuts it, slabs folded in order, the epilogue in fp32.  Operands are fetched by ADDRESS (base + row * pitch + column)
    from the padded allocations, results stored by address -- so `defect` can name a wrong address as well as wrong arithmetic."""
    c = pb.case
    assert defect is None or defect in DEFECTS
    dev = pb.A.flat.device
    M, N, K = c.M, c.N, c.K
    kchunk, eff = plan_splits(K, c.splits)
    rows = M + (1 if defect == "row_past_m" else 0)
    cols = N + (8 if defect == "pitch_spill" else 0)
    mi, ni = torch.arange(rows, device=dev), torch.arange(cols, device=dev)
    ldb = K if (defect == "ldb_is_k" and c.b_trans) else pb.B.pitch

    def fetch(buf, trans, ri, ki, pitch, limit):
        # rows at or past `limit` are the zero fill of a bounds-checked load (the defects that store too much compute on them)
        pos = buf.off + (ki[None, :] * pitch + ri[:, None] if trans else ri[:, None] * pitch + ki[None, :])
        v = buf.flat[pos.clamp(max=buf.flat.numel() - 1)].to(F32)
        return torch.where((ri < limit)[:, None], v, torch.zeros_like(v))

    slabs = []
    for z in range(eff):
        k0, k1 = z * kchunk, min(K, (z + 1) * kchunk)
        if z == eff - 1:
            if defect == "overread_last_split":
                k1 = k0 + max(kchunk, 32) if k1 % 32 == 0 else (k1 + 31) // 32 * 32 + 32
            if defect == "drop_k_tail":
                k1 = k1 // 32 * 32
        slab = torch.zeros(rows, cols, dtype=F32, device=dev)
        for kc in range(k0, k1, 32):
            ki = torch.arange(kc, min(kc + 32, k1), device=dev)
            slab = slab + fetch(pb.A, c.a_trans, mi, ki, pb.A.pitch, M) @ fetch(pb.B, c.b_trans, ni, ki, ldb, N).t()
        slabs.append(slab)
    got = {k: o.buf.flat.clone() for k, o in pb.outs.items()}
    if pb.ws is not None:
        got["ws"] = pb.ws.clone()
        got["ws"][:pb.ws_need] = torch.stack([s[:M, :N] for s in slabs]).reshape(-1)

    def store(name, v, idx_fn=None):
        """rows x cols values -> the allocation, by address"""
        o = pb.outs[name].buf
        idx = (o.off + mi[:, None] * o.pitch + ni[None, :]) if idx_fn is None else idx_fn(o)
        got[name][idx.reshape(-1)] = v.to(o.flat.dtype).reshape(-1) if v.dtype != BF16 else v.reshape(-1)

    if c.epi == EPI_SPLIT_F32:
        o = pb.outs["out"].buf
        for z, s in enumerate(slabs):
            idx = o.off + (z * M + mi[:, None]) * o.pitch + ni[None, :]
            got["out"][idx.reshape(-1)] = s.reshape(-1)
        if c.out2:
            for z in range(eff):
                k0, k1 = z * kchunk, min(K, (z + 1) * kchunk)
                a = fetch(pb.A, c.a_trans, mi[:M], torch.arange(k0, k1, device=dev), pb.A.pitch, M)
                r = pb.outs["out2"].buf
                got["out2"][r.off + z * r.pitch: r.off + z * r.pitch + M] = a.sum(1)
        return got
    total = torch.zeros_like(slabs[0]) if defect == "fold_skips_slab0" and eff > 1 else slabs[0]
    for s in slabs[1:]:
        total = total + s
    v = total
    if c.bias:
        b = pb.bias.flat[pb.bias.off + ni.clamp(max=N - 1)]
        v = v + (b * eff if defect == "bias_per_split" else b)
    srow = torch.ones(rows, 1, dtype=F32, device=dev)
    if c.rowscale:
        srow = pb.rowscale.flat[pb.rowscale.off + mi.clamp(max=M - 1) // c.rps][:, None]
    rnd = lambda x: _round_f32_bf16(x.contiguous(), defect)
    if c.epi == EPI_BF16:
        store("out", rnd(v))
    elif c.epi == EPI_GELU_DUAL:
        h = rnd(v)
        store("out", h)
        store("out2", rnd(_gelu32(h.to(F32))))
    elif c.epi == EPI_GELU_BWD:
        a = pb.aux.flat[pb.aux.off + mi.clamp(max=M - 1)[:, None] * pb.aux.pitch + ni.clamp(max=N - 1)[None, :]].to(F32)
        store("out", rnd(v * _gelu_grad32(a)))
    elif c.epi in (EPI_F32, EPI_RESID_F32):
        o = pb.outs["out"].buf
        oidx = o.off + mi[:, None] * o.pitch + ni[None, :]
        if c.epi == EPI_RESID_F32:
            a = pb.aux.flat[pb.aux.off + mi.clamp(max=M - 1)[:, None] * pb.aux.pitch + ni.clamp(max=N - 1)[None, :]]
            res = a + srow * v
            copy = res
        else:
            res = v
            if c.accumulate and defect != "accumulate_ignored":
                res = o.flat[oidx] + v
            copy = res * srow
        store("out", res)
        if c.out2 and not rowsum_form(c):
            store("out2", rnd(copy))
        elif c.out2:
            a = fetch(pb.A, c.a_trans, mi[:M], torch.arange(K, device=dev), pb.A.pitch, M).sum(1)
            r = pb.outs["out2"].buf
            if c.accumulate and defect != "accumulate_ignored":
                a = a + r.flat[r.off:r.off + M]
            got["out2"][r.off:r.off + M] = a
    elif c.epi == EPI_PIXSHUF2_F32:
        tok, ch = pixshuf_tokens(M, N, c.ps[0], c.ps[1], dev, swap=defect == "pixshuf_swapped")
        if c.out1:
            store("out", v[:M, :N], lambda o: o.off + tok * o.pitch + ch)
        if c.out2:
            store("out2", rnd(v[:M, :N]), lambda o: o.off + tok * o.pitch + ch)
    elif c.epi == EPI_UNSHUF2_BF16:
        tok, col = unshuf_tokens(M, N, c.ps[0], c.ps[1], dev)
        store("out", rnd(v[:M, :N]), lambda o: o.off + tok * o.pitch + col)
    return got


# ------------------------------------------------------------------ the case list of the GPU test (and of the coverage assertion)
def _b(name, M, N, K, route, **kw):
    return Case(name, M, N, K, route, **kw)


LAYOUTS = {"nn": (False, False), "nt": (False, True), "tn": (True, False), "tt": (True, True)}


def base_shapes():
    """One base case per kernel instantiation: the smallest shape that reaches it, with the route it must reach.  Where a route
    has a whole and a ragged form both are listed."""
    out = []
    for lay, (at, bt) in LAYOUTS.items():
        kw = dict(a_trans=at, b_trans=bt)
        # 64-row tiles, 32-deep: ragged M, ragged N, a k tail (K = 200: six whole chunks and one of 8)
        out.append(_b(f"t64-{lay}-ragged", 200, 104, 200, f"tile64/{lay}", **kw))
        out.append(_b(f"t64-{lay}-k48", 64, 96, 48, f"tile64/{lay}", **kw))
        # 128-deep stages: kchunk >= 256 on a small grid; K = 264 puts a k tail inside a deep stage
        out.append(_b(f"t64d-{lay}-k264", 72, 104, 264, f"tile64-deep/{lay}", **kw))
        # 128- and 256-row tiles need >= 512 of them (and >= 32 column tiles for 256 rows); a_trans: M = Nw
        out.append(_b(f"t128-{lay}", 3000 if not at else 2048, 3072, 32, f"tile128/{lay}", **kw))
        if not at:
            out.append(_b(f"t256-{lay}", 4096, 3064, 32, f"tile256/{lay}", **kw))
        else:
            # regression: the launcher sent this weight-gradient shape to 256-row tiles, which the k-slow LDS layout of a
            # transposed A (128 rows per k) cannot hold -- every output was wrong; it now stays on 128 rows
            out.append(_b(f"t128-{lay}-m4096", 4096, 3072, 32, f"tile128/{lay}", **kw))
        if not at:
            out.append(_b(f"f64-{lay}", 128, 192, 32, f"full64/{lay}", **kw))
            out.append(_b(f"f64-{lay}-checked", 128, 192, 32, f"tile64/{lay}", checked=True, **kw))
            out.append(_b(f"f64d-{lay}", 64, 96, 256, f"full64-deep/{lay}", **kw))
            out.append(_b(f"f128-{lay}", 2048, 3072, 32, f"full128/{lay}", **kw))
            out.append(_b(f"f256-{lay}", 4096, 3072, 64, f"full256/{lay}", **kw))
            out.append(_b(f"mid-{lay}-ragged", 200, 200, 64, f"mid/{lay}", mid=True, **kw))
            out.append(_b(f"mid-{lay}", 192, 384, 128, f"mid/{lay}", mid=True, **kw))
    for d in STREAM_DEPTHS:
        out.append(_b(f"stream{d}", 64, 96, d, f"stream{d}/nn", packed=True))
    return out


def _extras():
    """beyond (route, epilogue): whole 64-row shapes, K = 32, split-K forms, the fused fold with every epilogue"""
    out = []
    for lay, (at, bt) in LAYOUTS.items():
        kw = dict(a_trans=at, b_trans=bt)
        whole = f"full64/{lay}" if not at else f"tile64/{lay}"
        out.append(with_epilogue(_b(f"x64-{lay}-whole-k32", 64, 96, 32, whole, **kw), EPI_BF16))
        out.append(with_epilogue(_b(f"x64-{lay}-m200-n96", 200, 96, 48, f"tile64/{lay}", **kw), EPI_BF16))
        out.append(with_epilogue(_b(f"x64-{lay}-m64-n104", 64, 104, 200, f"tile64/{lay}", **kw), EPI_F32))
        # the K = 256 whole deep stage of the transposed-A form
        if at:
            out.append(with_epilogue(_b(f"x64d-{lay}-k256", 64, 96, 256, f"tile64-deep/{lay}", **kw), EPI_F32))
    # split-K: a ragged last chunk (K = 200 in three: 96 + 96 + 8), raw slabs and the fused fold with every epilogue it takes
    for epi in EPIS:
        for lay in ("nn", "tt"):
            at, bt = LAYOUTS[lay]
            b = _b(f"split3-{lay}", 200, 104, 200, f"tile64/{lay}", a_trans=at, b_trans=bt, splits=3)
            out.append(with_epilogue(b, epi))
    out.append(with_epilogue(_b("split7-nt", 72, 104, 264, "tile64/nt", b_trans=True, splits=7), EPI_RESID_F32))
    out.append(with_epilogue(_b("split2-deep", 64, 96, 520, "tile64-deep/nn", splits=2), EPI_BF16))
    out.append(with_epilogue(_b("mid-split2", 192, 200, 256, "mid/nn", mid=True, splits=2), EPI_F32))
    out.append(with_epilogue(_b("mid-split2-nt", 200, 192, 128, "mid/nt", mid=True, b_trans=True, splits=2), EPI_SPLIT_F32))
    for d in STREAM_DEPTHS:
        out.append(with_epilogue(_b(f"stream{d}-split2", 96, 192, 2 * d, f"stream{d}/nn", packed=True, splits=2), EPI_F32, 1))
    out.append(with_epilogue(_b("stream96-split3-raw", 32, 96, 288, "stream96/nn", packed=True, splits=3), EPI_SPLIT_F32))
    return out


def gpu_cases():
    """every base shape with every epilogue its route accepts (both variants on the small shapes), and the extras"""
    out = []
    for b in base_shapes():
        small = b.M * b.N <= 1 << 16
        for epi in EPIS:
            if not route_accepts(b.route, epi):
                continue
            if epi in (EPI_PIXSHUF2_F32,) and b.N % 4:
                continue
            if epi == EPI_UNSHUF2_BF16 and b.M % 4:
                continue
            out.append(with_epilogue(b, epi))
            if small and epi in (EPI_F32, EPI_RESID_F32, EPI_PIXSHUF2_F32, EPI_UNSHUF2_BF16):
                out.append(with_epilogue(b, epi, 1))
    out += _extras()
    names = [c.name for c in out]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return out


# ------------------------------------------------------------------ grouped weight gradient and the row fold
def wgrad_kernel(items, small_tiles=False):
    """The documented rule, stated once: large tiles (192 x 192 where both dimensions are multiples of 192, 384 x 96 for Kw == 96
    and Nw % 96 == 0, 96 x 384 for Nw == 96 and Kw % 96 == 0) only if EVERY item of the group has a large-tile shape and a token
    count that is a multiple of 32; else the 64 x 96 tile for all.  items: (Mtok, Nw, Kw, ...).  Returns 'large' / 'small' and the
    tiles per token split of each item as tulip_wgrad_tiles must report them."""
    def shape(Nw, Kw):
        if small_tiles:
            return None
        if Nw % 192 == 0 and Kw % 192 == 0:
            return (192, 192)
        if Kw == 96 and Nw % 96 == 0:
            return (384, 96)
        if Nw == 96 and Kw % 96 == 0:
            return (96, 384)
        return None
    large = all(shape(it[1], it[2]) is not None and it[0] % 32 == 0 for it in items)
    tiles = []
    for it in items:
        tm, tn = (shape(it[1], it[2]) if large else None) or (64, 96)
        tiles.append(-(-it[1] // tm) * -(-it[2] // tn))
    return ("large" if large else "small"), tiles


@dataclass
class WgradItem:
    Mtok: int
    Nw: int
    Kw: int
    splits: int = 1
    db: bool = True
    overwrite: bool = False
    wide: bool = True              # ldy > Nw and ldx > Kw


@dataclass
class WgradProblem:
    items: list
    dY: list
    X: list
    dW: list                       # Out
    db: list                       # Out or None
    ws: torch.Tensor
    ws_need: int


def build_wgrad(items, device="cpu", seed=0) -> WgradProblem:
    gen = torch.Generator().manual_seed(4242 + seed)
    dYs, Xs, dWs, dbs, need = [], [], [], [], 0
    for it in items:
        dY = Buf(it.Mtok, it.Nw, _pitch(it.Nw) if it.wide else it.Nw, BF16, "nan", device).set(ints(gen, (it.Mtok, it.Nw), -8, 8, device))
        X = Buf(it.Mtok, it.Kw, _pitch(it.Kw) if it.wide else it.Kw, BF16, "nan", device).set(ints(gen, (it.Mtok, it.Kw), -8, 8, device))
        g = dY.view.to(F64).t() @ X.view.to(F64) + 0.0
        s = dY.view.to(F64).sum(0)[None, :] + 0.0
        w = Buf(it.Nw, it.Kw, it.Kw, F32, "guard", device)                 # (the gradient is contiguous: ldo = Kw)
        b = Buf(1, it.Nw, it.Nw + 8, F32, "guard", device) if it.db else None
        if not it.overwrite:
            w.set(ints(gen, (it.Nw, it.Kw), -1000, 1000, device))
            g = w.view.to(F64) + g
            if b is not None:
                b.set(ints(gen, (1, it.Nw), -1000, 1000, device))
                s = b.view.to(F64) + s
        assert float(g.abs().max()) < EXACT_LIMIT and float(s.abs().max()) < EXACT_LIMIT
        dYs.append(dY), Xs.append(X)
        dWs.append(Out(w, _image(w, w.index(), g), w.index()))
        dbs.append(Out(b, _image(b, b.index(), s), b.index()) if b is not None else None)
        eff = plan_splits(it.Mtok, it.splits)[1]
        if eff > 1:
            need += (it.Nw * it.Kw + (it.Nw if it.db else 0)) * eff
    return WgradProblem(items, dYs, Xs, dWs, dbs, filled(need + 64, F32, "guard", device), need)


def check_wgrad(pb: WgradProblem, got_dW, got_db, got_ws, what="") -> list:
    reps = []
    for i, it in enumerate(pb.items):
        reps.append(check_out(f"{what}item{i}.dW", pb.dW[i], got_dW[i], "tile64/tt"))
        if pb.db[i] is not None:
            reps.append(check_out(f"{what}item{i}.db", pb.db[i], got_db[i], "tile64/tt"))
    rep = Report(what + "workspace")
    bad = _ibits(got_ws.contiguous())[pb.ws_need:] != _ibits(pb.ws)[pb.ws_need:]
    if bool(bad.any()):
        rep.violations.append(f"{int(bad.sum())} guard words past the required {pb.ws_need * 4} bytes changed")
    return reps + [rep]


@dataclass
class Region:
    part: Buf                      # [rows][n] at pitch stride, inside NaN
    out: Out
    rows: int
    n: int
    overwrite: bool
    index: torch.Tensor = None     # int32 [scatter_len]
    nh: int = 0
    length: int = 0


def build_region(rows, n, stride, overwrite, device="cpu", seed=0, scatter=None) -> Region:
    """scatter = (nh, length, table entries): the dense [nh][length] sums are ADDED to out[index[ij] * nh + h]"""
    gen = torch.Generator().manual_seed(977 + seed + rows + 3 * n)
    part = Buf(rows, n, stride, F32, "nan", device).set(ints(gen, (rows, n), -64, 64, device))
    tot = part.view.to(F64).sum(0)
    if scatter is None:
        o = Buf(1, n, n + 8, F32, "guard", device)
        if not overwrite:
            o.set(ints(gen, (1, n), -1000, 1000, device))
            tot = o.view.to(F64).reshape(-1) + tot
        return Region(part, Out(o, _image(o, o.index(), tot[None, :]), o.index()), rows, n, overwrite)
    nh, length, ntab = scatter
    assert n == nh * length and not overwrite
    index = torch.randint(0, ntab, (length,), generator=gen).to(torch.int32).to(device)
    index[:ntab] = torch.arange(ntab, dtype=torch.int32, device=device)        # every entry has pairs
    o = Buf(ntab, nh, nh, F32, "guard", device)
    o.set(ints(gen, (ntab, nh), -1000, 1000, device))
    ref = o.view.to(F64).clone()                                                 # [ntab][nh]
    ref.index_add_(0, index.long(), tot.reshape(nh, length).t().contiguous())
    assert float(ref.abs().max()) < EXACT_LIMIT
    return Region(part, Out(o, _image(o, o.index(), ref), o.index()), rows, n, overwrite, index, nh, length)


def wgrad_groups():
    """name -> (items, the kernel the group must get): one group per tile shape, the mixed group whose one ragged item sends
    every item to the small tiles, token counts ragged to 8 (small tiles) and to 32 (large), splits 1 and > 1, with and without
    db, overwrite 0 and 1 -- all at ldy > Nw, ldx > Kw except where an item says otherwise"""
    W = WgradItem
    return {
        "192x192": ([W(64, 192, 192), W(128, 384, 192, splits=2, db=False, overwrite=True)], "large"),
        "384x96": ([W(64, 384, 96, overwrite=True), W(96, 288, 96, splits=3)], "large"),
        "96x384": ([W(64, 96, 384, db=False), W(160, 96, 288, splits=2, overwrite=True)], "large"),
        "64x96": ([W(72, 136, 200), W(200, 64, 104, splits=3, overwrite=True), W(64, 96, 96, db=False, wide=False)], "small"),
        # 128-deep stages of the 64 x 96 group kernel: every item's token range per split >= 256; 264 leaves a tail inside a stage
        "64x96-deep": ([W(264, 136, 104), W(520, 64, 96, splits=2, overwrite=True)], "small"),
        "mixed": ([W(64, 192, 192), W(64, 384, 96, splits=2), W(64, 104, 96, overwrite=True)], "small"),
        "mtok-ragged-8": ([W(72, 192, 192), W(136, 96, 384, splits=2, overwrite=True)], "small"),
        "mtok-ragged-32": ([W(96, 192, 192, overwrite=True), W(160, 288, 96, splits=2), W(32, 96, 96, db=False)], "large"),
    }


def region_cases():
    """(name, rows, n, stride, overwrite, scatter): n % 4 == 0 with stride > n, one row and many rows, both overwrite forms, the
    deterministic scatter lengths 256 / 1024 / 4096 and the atomic form (64)"""
    return [("one-row", 1, 104, 112, False, None), ("one-row-set", 1, 8, 12, True, None),
            ("many-rows", 37, 200, 208, False, None), ("many-rows-set", 150, 4100, 4104, True, None),
            ("scatter256", 9, 3 * 256, 3 * 256 + 4, False, (3, 256, 45)), ("scatter1024", 5, 2 * 1024, 2 * 1024 + 8, False, (2, 1024, 105)),
            ("scatter4096", 3, 2 * 4096, 2 * 4096 + 4, False, (2, 4096, 225)), ("scatter64-atomic", 7, 3 * 64, 3 * 64 + 4, False, (3, 64, 21))]

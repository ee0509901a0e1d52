"""csrc/norm.hip on integer operands (tests/norm_exact.py), through tulip_amd.ops: tulip_patch_embed_fwd / _bwd, tulip_layernorm_fwd /
_bwd / _bwd_splitk / _bwd_params and tulip_splitk_resid_ln, one case per launcher route and per edge of the accepted domain.  Bit
for bit: every guard word around and between the output rows (the padding columns of the partial rows, the rows behind the last
partial row, the other half of the concat row beside out_bf16), out_bf16 / dx_bf16 as the one rounding of the fp32 value the launch
itself stored (times its DropPath scale), d(beta), and on exact LayerNorm rows y, mean == 0, d(gamma) and the partial rows; no NaN
leaking in from the padding around the operands; a second partial launch identical to the first.  Within a budget taken from the
reference alone: out, rstd, dx, d(w), d(b), d(gamma).  No fraction of elements is allowed to differ anywhere.  Route table, run
time and the measured budget ratios: DESIGN.md, "Exact LayerNorm and patch-embedding tests"."""
from dataclasses import replace

import pytest
import torch

from tests import gemm_exact as GX
from tests import norm_exact as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = GX.F32, GX.BF16


@pytest.fixture(scope="module")
def ops():
    from tulip_amd import ops as o
    return o


def holds(b, rows, cols, dtype):
    """the allocation really holds the [rows][cols] tensor the header says the launch addresses"""
    assert (b.rows, b.cols, b.flat.dtype) == (rows, cols, dtype), (b.rows, b.cols, b.flat.dtype, rows, cols, dtype)
    assert b.pitch >= b.cols and b.off + (b.rows - 1) * b.pitch + b.cols <= b.flat.numel()


def verdict(name, reps, opt=""):
    line = X.ratios(reps)
    if line:
        print(f"{name} {opt}: measured / budget {line}")
    return X.failures(reps)


def embed_args(c):
    return dict(B=c.B, Cin=c.Cin, Hin=c.Hin, Win=c.Win, E=c.E, p0=c.p0, p1=c.p1, kw=c.kw, circular=c.circ, eps=X.LN_EPS)


def holds_embed(pb):
    c, i = pb.case, pb.ins
    holds(i["img"], c.B * c.Cin * c.Hin, c.Win, F32), holds(i["w"], 1, c.E * c.taps, F32)
    for k in ("b", "gamma", "beta"):
        holds(i[k], 1, c.E, F32)
    assert c.taps == c.Cin * c.p0 * c.kw and c.ntok == c.B * (c.Hin // c.p0) * (c.Win // c.p1)


@pytest.mark.parametrize("case", X.EMBED_FWD, ids=lambda c: c.name)
def test_patch_embed_fwd(ops, case):
    c = case
    assert X.embed_fwd_route(c.Cin, c.p0, c.kw, c.taps) == c.route
    pb = X.build_embed(c, DEV)
    i, o = pb.ins, pb.outs
    holds_embed(pb)
    holds(o["out"], c.ntok, c.E, F32), holds(o["ld_e"], c.ntok, c.E, BF16), holds(o["ld_2e"], c.ntok, 2 * c.E, BF16)
    for variant in X.BF16_VARIANTS:
        got = X.fresh(pb)
        o16, ld = None, 0
        if variant == "ld_e":
            o16, ld = o["ld_e"].addr(got["ld_e"]), c.E
        elif variant == "ld_2e":                                       # the second half of the concat row
            o16, ld = o["ld_2e"].addr(got["ld_2e"]) + 2 * c.E, 2 * c.E
        ops.patch_embed_fwd(i["img"].addr(), i["w"].addr(), i["b"].addr(), i["gamma"].addr(), i["beta"].addr(), o["out"].addr(got["out"]),
                            out_bf16=o16, ld_bf16=ld, **embed_args(c))
        torch.cuda.synchronize()
        bad = verdict(c.name, X.check_embed_fwd(pb, got, variant), variant)
        assert not bad, (c.name, c.route, variant, bad)


def launch_embed_bwd(ops, pb):
    c, i, o = pb.case, pb.ins, pb.outs
    got = X.fresh(pb)
    E, T = c.E, c.taps
    if c.form == "partial":
        p = o["part"]
        holds(p, ops.patch_embed_bwd_blocks(c.ntok), E * T + 3 * E, F32)
        base = p.addr(got["part"])
        ptrs, stride = [base, base + 4 * E * T, base + 4 * (E * T + E), base + 4 * (E * T + 2 * E)], p.pitch
    else:
        holds(o["dw"], 1, E * T, F32)
        for k in ("db", "dgamma", "dbeta"):
            holds(o[k], 1, E, F32)
        ptrs, stride = [o[k].addr(got[k]) for k in ("dw", "db", "dgamma", "dbeta")], 0
    ops.patch_embed_bwd(i["img"].addr(), i["w"].addr(), i["b"].addr(), i["gamma"].addr(), i["dout"].addr(), *ptrs,
                        partial_stride=stride, **embed_args(c))
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("case", X.EMBED_BWD, ids=lambda c: c.name)
def test_patch_embed_bwd(ops, case):
    c = case
    assert X.embed_bwd_route(c.E, c.taps, c.form == "partial") == c.route
    pb = X.build_embed(c, DEV)
    holds_embed(pb)
    holds(pb.ins["dout"], c.ntok, c.E, F32)
    assert pb.ref["n_nz"] <= X.MAX_NZ
    got = launch_embed_bwd(ops, pb)
    bad = verdict(c.name, X.check_embed_bwd(pb, got), c.form)
    assert not bad, (c.name, c.route, c.form, bad)
    if c.form == "partial":
        again = launch_embed_bwd(ops, pb)                              # the partial forms are deterministic
        assert torch.equal(GX._ibits(again["part"]), GX._ibits(got["part"])), (c.name, c.route, "second launch differs")
        at = replace(c, form="atomic", route=X.embed_bwd_route(c.E, c.taps, False))
        pa = X.build_embed(at, DEV)                                    # the same operands (the seed does not hold the form)
        assert torch.equal(pa.ins["dout"].flat.nan_to_num(), pb.ins["dout"].flat.nan_to_num())
        ga = launch_embed_bwd(ops, pa)
        bad = verdict(c.name, X.check_fold_vs_atomic(pb, X.embed_fold(pb, got), X.embed_fold(pa, ga)), "fold vs atomic")
        assert not bad, (c.name, c.route, "fold vs atomic", bad)


def ln_geom(c):
    m = c.merge
    return dict(merge=bool(m), B=m[0] if m else 0, H=m[1] if m else 0, W=m[2] if m else 0)


def holds_x(pb):
    c = pb.case
    if c.merge:
        holds(pb.ins["x"], c.merge[0] * c.merge[1] * c.merge[2], c.C // 4, F32)
    else:
        holds(pb.ins["x"], c.rows, c.C, F32)


@pytest.mark.parametrize("case", X.LN_CASES, ids=lambda c: c.name)
def test_layernorm_fwd(ops, case):
    c = case
    assert X.ln_route(c.C) == c.route
    pb = X.build_ln_fwd(c, DEV)
    i, o = pb.ins, pb.outs
    holds_x(pb)
    holds(i["gamma"], 1, c.C, F32), holds(i["beta"], 1, c.C, F32)
    holds(o["y"], c.rows, c.C, BF16), holds(o["mean"], 1, c.rows, F32), holds(o["rstd"], 1, c.rows, F32)
    got = X.fresh(pb)
    ops.layernorm_fwd(i["x"].addr(), i["gamma"].addr(), i["beta"].addr(), o["y"].addr(got["y"]), o["mean"].addr(got["mean"]),
                      o["rstd"].addr(got["rstd"]), c.rows, c.C, X.LN_EPS, **ln_geom(c))
    torch.cuda.synchronize()
    bad = verdict(c.name, X.check_ln_fwd(pb, got))
    assert not bad, (c.name, c.route, bad)


def run_ln_bwd(ops, case, sources):
    c = case
    assert X.ln_route(c.C) == c.route
    R = ops.layernorm_bwd_partial_rows(c.rows, c.C)
    assert R == X.ln_partial_rows(c.rows, c.C)
    pb = X.build_ln_bwd(c, DEV)
    i, o = pb.ins, pb.outs
    tokens, cdx = (c.rows, c.C) if not c.merge else (c.merge[0] * c.merge[1] * c.merge[2], c.C // 4)
    holds_x(pb)
    holds(i["mean"], 1, c.rows, F32), holds(i["rstd"], 1, c.rows, F32), holds(i["gamma"], 1, c.C, F32)
    holds(i["dy"], c.rows, c.C, BF16), holds(i["slabs"], c.nslab * c.rows, c.C, F32), holds(i["dres"], tokens, cdx, F32)
    holds(o["dx"], tokens, cdx, F32), holds(o["dx16"], tokens, cdx, BF16)
    assert i["scale"].cols * c.crps >= tokens
    if R:
        holds(o["part"], R, 2 * c.C, F32)
    for opt in X.bwd_options(c):
        if opt["src"] not in sources:
            continue
        got = X.fresh_ln_bwd(pb, opt["dres"])
        dx = o["dx"].addr(got["dx"])
        kw = dict(dres={"none": None, "separate": i["dres"].addr(), "inplace": dx}[opt["dres"]], dx=dx, rows=c.rows, C=c.C,
                  param_partials=o["part"].addr(got["part"]) if opt["parts"] else None,
                  dx_bf16=o["dx16"].addr(got["dx16"]) if opt["cast"] != "none" else None,
                  cast_rowscale=i["scale"].addr() if opt["cast"] == "scaled" else None,
                  cast_rows_per_sample=c.crps if opt["cast"] == "scaled" else 1, **ln_geom(c))
        common = dict(x=i["x"].addr(), mean=i["mean"].addr(), rstd=i["rstd"].addr(), gamma=i["gamma"].addr())
        if opt["src"] == "dy":
            ops.layernorm_bwd(dy=i["dy"].addr(), **common, **kw)
        else:
            ops.layernorm_bwd_splitk(slabs=i["slabs"].addr(), nslab=c.nslab, **common, **kw)
        torch.cuda.synchronize()
        bad = verdict(c.name, X.check_ln_bwd(pb, got, **opt), opt)
        assert not bad, (c.name, c.route, opt, bad)


@pytest.mark.parametrize("case", X.LN_CASES, ids=lambda c: c.name)
def test_layernorm_bwd(ops, case):
    run_ln_bwd(ops, case, ("dy",))


@pytest.mark.parametrize("case", X.LN_CASES, ids=lambda c: c.name)
def test_layernorm_bwd_splitk(ops, case):
    run_ln_bwd(ops, case, ("slabs",))


@pytest.mark.parametrize("case", X.PARAMS, ids=lambda c: c.name)
def test_layernorm_bwd_params(ops, case):
    c = case
    assert X.ln_params_grid(c.rows, c.C) == c.grid
    pb = X.build_params(c, DEV)
    i, o = pb.ins, pb.outs
    holds_x(pb)
    holds(i["mean"], 1, c.rows, F32), holds(i["rstd"], 1, c.rows, F32), holds(i["dy"], c.rows, c.C, BF16)
    holds(o["dgamma"], 1, c.C, F32), holds(o["dbeta"], 1, c.C, F32)
    got = X.fresh(pb)
    ops.layernorm_bwd_params(i["dy"].addr(), i["x"].addr(), i["mean"].addr(), i["rstd"].addr(), o["dgamma"].addr(got["dgamma"]),
                             o["dbeta"].addr(got["dbeta"]), c.rows, c.C, **ln_geom(c))
    torch.cuda.synchronize()
    bad = verdict(c.name, X.check_params(pb, got))
    assert not bad, (c.name, c.grid, bad)


@pytest.mark.parametrize("case", X.SPLITK, ids=lambda c: c.name)
def test_splitk_resid_ln(ops, case):
    c = case
    assert X.splitk_ln_nch(c.N) == c.nch and ops.splitk_resid_ln_supported(c.N)
    pb = X.build_splitk(c, DEV)
    i, o = pb.ins, pb.outs
    holds(i["slabs"], c.nslab * c.M, c.N, F32), holds(i["bias"], 1, c.N, F32), holds(i["aux"], c.M, c.N, F32)
    holds(i["gamma"], 1, c.N, F32), holds(i["beta"], 1, c.N, F32)
    holds(o["out"], c.M, c.N, F32), holds(o["out16"], c.M, c.N, BF16), holds(o["y"], c.M, c.N, BF16)
    holds(o["mean"], 1, c.M, F32), holds(o["rstd"], 1, c.M, F32)
    assert i["scale"].cols * c.rps >= c.M and all(b.pitch % 4 == 0 and b.pitch > c.N for b in (o["out"], o["out16"], i["aux"]))
    got = X.fresh(pb)
    ops.splitk_resid_ln(i["slabs"].addr(), c.nslab, c.M, c.N, i["bias"].addr() if c.bias else None, i["aux"].addr() if c.aux else None,
                        i["aux"].pitch if c.aux else 0, i["scale"].addr() if c.rowscale else None, c.rps,
                        o["out"].addr(got["out"]), o["out"].pitch, o["out16"].addr(got["out16"]) if c.out16 else None,
                        o["out16"].pitch if c.out16 else 0, i["gamma"].addr(), i["beta"].addr(), o["y"].addr(got["y"]),
                        o["mean"].addr(got["mean"]), o["rstd"].addr(got["rstd"]), X.LN_EPS)
    torch.cuda.synchronize()
    bad = verdict(c.name, X.check_splitk(pb, got))
    assert not bad, (c.name, c.nch, bad)

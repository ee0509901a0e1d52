"""tulip_merge_fwd, tulip_merge_bwd, tulip_unmerge_skip_fwd and tulip_skip_unmerge_bwd on integer operands (tests/glue_exact.py),
through tulip_amd.ops: every fp32 output of a GEMM equal to the float64 result bit for bit, every bf16 tensor its one
round-to-nearest-even, mean exactly 0, rstd within 2 fp32 ulp, dx_prev per element within its budget, the partial rows written,
finite and summing to the exact d(gamma) / d(beta), dx_bf16 the exact rounding of the stored dx times its DropPath scale, every
guard word around the outputs (the pitch gap of y_bf16, the x_save half of the concat rows, the rows behind the partial rows)
unchanged, no NaN leaking in from the padding around the operands, and no allocation touched whose option is not given -- on the
smallest grids at which each route of the launchers and each edge of their accepted domain exists.  No fraction of elements is
allowed to differ anywhere.  Grid / route table, run time and the measured dx_prev error: DESIGN.md, "Exact stage-boundary tests"."""
import pytest
import torch

from tests import gemm_exact as GX
from tests import glue_exact as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 1024                        # bytes in front of a packed weight copy


@pytest.fixture(scope="module")
def ops():
    from tulip_amd import ops as o
    return o


def packed(ops, w, transpose=False):
    """address of the fragment-major copy of the bf16 matrix w (or of its transpose), inside NaN; and the allocation that holds it"""
    w = w.to(DEV).contiguous()
    flat = GX.filled(w.numel() + 1024, GX.BF16, "nan", DEV)
    it, n = ops.pack_items([(w, flat.data_ptr() + PAD, w.shape[0], w.shape[1], int(transpose))])
    ops.pack_bf16_multi(it, n)
    torch.cuda.synchronize()
    return flat.data_ptr() + PAD, flat


def holds(b, rows, cols, dtype):
    """the allocation really holds the [rows][cols] tensor the header says the launch addresses"""
    assert (b.rows, b.cols, b.flat.dtype) == (rows, cols, dtype), (b.rows, b.cols, b.flat.dtype, rows, cols, dtype)
    assert b.pitch >= b.cols and b.off + (b.rows - 1) * b.pitch + b.cols <= b.flat.numel()


def launch(ops, pb, y16=True, cast="scaled", skip=True):
    """one call on fresh copies of the case's output allocations; every allocation is first held against the header's shapes"""
    c, i, o = pb.case, pb.ins, pb.outs
    got = X.fresh(pb, skip)
    at = lambda name: o[name].buf.addr(got[name])
    keep = []
    if pb.op == "merge_fwd":
        rows, K, N = c.rows, 4 * c.Cin, 2 * c.Cin
        holds(i["x"], c.B * c.H * c.W, c.Cin, GX.F32), holds(i["gamma"], 1, K, GX.F32), holds(i["beta"], 1, K, GX.F32)
        holds(o["xm"].buf, rows, K, GX.BF16), holds(o["mean"].buf, 1, rows, GX.F32), holds(o["rstd"].buf, 1, rows, GX.F32)
        holds(o["y"].buf, rows, N, GX.F32), holds(o["y16"].buf, rows, N, GX.BF16)
        assert tuple(i["w"].shape) == (N, K) and o["y16"].buf.pitch % 4 == 0
        wp, k = packed(ops, i["w"])
        keep.append(k)
        ops.merge_fwd(x=i["x"].addr(), gamma=i["gamma"].addr(), beta=i["beta"].addr(), w_packed=wp, xm=at("xm"), mean=at("mean"),
                      rstd=at("rstd"), y=at("y"), y_bf16=at("y16") if y16 else None, ld_bf16=o["y16"].buf.pitch if y16 else 0,
                      B=c.B, H=c.H, W=c.W, Cin=c.Cin, eps=X.LN_EPS)
    elif pb.op == "merge_bwd":
        Cp, Cs, K4, rows, tokens = c.Cp, 2 * c.Cp, 4 * c.Cp, c.rows, c.B * c.H * c.W
        R = ops.merge_bwd_partial_rows(Cp, c.B, c.H, c.W)
        holds(i["dx_in"], rows, Cs, GX.F32), holds(i["dys"], rows, Cs, GX.BF16), holds(i["x_prev"], tokens, Cp, GX.F32)
        holds(i["mean"], 1, rows, GX.F32), holds(i["rstd"], 1, rows, GX.F32), holds(i["gamma"], 1, K4, GX.F32)
        holds(o["dyb"].buf, rows, Cs, GX.BF16), holds(o["dx"].buf, tokens, Cp, GX.F32), holds(o["dx16"].buf, tokens, Cp, GX.BF16)
        holds(o["part"].buf, R, 2 * K4, GX.F32)
        assert tuple(i["wskip"].shape) == (Cs, 2 * Cs) and tuple(i["wred"].shape) == (Cs, K4) and i["scale"].cols * c.crps >= tokens
        wr, k = packed(ops, i["wred"], True)
        keep.append(k)
        ws = None
        if skip:
            ws, k = packed(ops, i["wskip"], True)
            keep.append(k)
        ops.merge_bwd(dx_in=i["dx_in"].addr() if skip else None, dy_skip=i["dys"].addr() if skip else None, w_skip_t_packed=ws,
                      dyb=at("dyb"), w_red_t_packed=wr, x_prev=i["x_prev"].addr(), mean=i["mean"].addr(), rstd=i["rstd"].addr(),
                      gamma=i["gamma"].addr(), dx_prev=at("dx"), param_partials=at("part"),
                      dx_bf16=at("dx16") if cast != "none" else None, cast_rowscale=i["scale"].addr() if cast == "scaled" else None,
                      cast_rows_per_sample=c.crps if cast == "scaled" else 0, B=c.B, H=c.H, W=c.W, Cp=Cp)
    elif pb.op == "unmerge_fwd":
        C, Cf, M = c.C, c.C // 2, c.M
        holds(i["x"], M, C, GX.BF16), holds(i["bexp"], 1, 2 * C, GX.F32), holds(i["bskip"], 1, Cf, GX.F32)
        holds(o["cat"].buf, 4 * M, C, GX.BF16), holds(o["out"].buf, 4 * M, Cf, GX.F32)
        assert tuple(i["wexp"].shape) == (2 * C, C) and tuple(i["wskip"].shape) == (Cf, C)
        we, k1 = packed(ops, i["wexp"])
        ws, k2 = packed(ops, i["wskip"])
        keep += [k1, k2]
        ops.unmerge_skip_fwd(x_bf16=i["x"].addr(), w_expand_packed=we, b_expand=i["bexp"].addr(), cat=at("cat"), w_skip_packed=ws,
                             b_skip=i["bskip"].addr(), out=at("out"), B=c.B, H=c.H, W=c.W, C=C)
    else:
        C, Cf, M = c.C, c.C // 2, c.M
        holds(i["dys"], 4 * M, Cf, GX.BF16), holds(o["dz"].buf, M, 2 * C, GX.BF16), holds(o["dx"].buf, M, C, GX.F32)
        holds(o["dx16"].buf, M, C, GX.BF16)
        assert tuple(i["wexp"].shape) == (2 * C, C) and tuple(i["wskip"].shape) == (Cf, C) and i["scale"].cols * c.crps >= M
        ws, k1 = packed(ops, i["wskip"], True)
        we, k2 = packed(ops, i["wexp"], True)
        keep += [k1, k2]
        ops.skip_unmerge_bwd(dy_skip=i["dys"].addr(), w_skip_t_packed=ws, dz=at("dz"), w_expand_t_packed=we, dx=at("dx"),
                             dx_bf16=at("dx16") if cast != "none" else None, cast_rowscale=i["scale"].addr() if cast == "scaled" else None,
                             cast_rows_per_sample=c.crps if cast == "scaled" else 0, B=c.B, H=c.H, W=c.W, C=C)
    torch.cuda.synchronize()
    return got


def verdict(pb, got, **opt):
    reps = X.check(pb, got, **opt)
    for r in reps:
        if "dx_prev" in r.what:
            print(f"{r.line()} {opt}")
    return X.failures(reps)


@pytest.mark.parametrize("case", X.MERGE_FWD, ids=lambda c: c.name)
def test_merge_fwd_is_exact(ops, case):
    assert ops.merge_fwd_supported(case.Cin, case.B, case.H, case.W)
    assert X.merge_fwd_route(case.Cin, case.rows) == case.route
    pb = X.build_merge_fwd(case, DEV)
    print(f"{case.name}: route {case.route}, ties of y_bf16 {pb.ties['y16']:.3f}")
    for y16 in (True, False):
        bad = verdict(pb, launch(ops, pb, y16=y16), y16=y16)
        assert not bad, (case.name, case.route, f"y_bf16 {'given' if y16 else 'absent'}", bad)


@pytest.mark.parametrize("case", X.MERGE_BWD, ids=lambda c: c.name)
def test_merge_bwd_is_exact(ops, case):
    assert ops.merge_bwd_supported(case.Cp, case.B, case.H, case.W)
    assert ops.merge_bwd_partial_rows(case.Cp, case.B, case.H, case.W) == case.rows // case.bm
    pb = X.build_merge_bwd(case, DEV)
    print(f"{case.name}: ties dyb {pb.ties['dyb']:.3f}, d(norm out) {pb.ties['dnorm']:.3f}; torch-float32 dx error {pb.ref['err32']:.3e}")
    for skip in (True, False):
        for cast in X.CAST_VARIANTS:
            bad = verdict(pb, launch(ops, pb, cast=cast, skip=skip), cast=cast)
            assert not bad, (case.name, f"skip operand {'given' if skip else 'absent'}", f"dx_bf16 {cast}", bad)


@pytest.mark.parametrize("case", X.UNMERGE, ids=lambda c: c.name)
def test_unmerge_skip_fwd_is_exact(ops, case):
    assert ops.unmerge_skip_supported(case.C, case.B, case.H, case.W)
    pb = X.build_unmerge_fwd(case, DEV)
    print(f"{case.name}: ties of z {pb.ties['cat']:.3f}")
    bad = verdict(pb, launch(ops, pb))
    assert not bad, (case.name, bad)


@pytest.mark.parametrize("case", X.UNMERGE, ids=lambda c: c.name)
def test_skip_unmerge_bwd_is_exact(ops, case):
    assert ops.unmerge_skip_supported(case.C, case.B, case.H, case.W)
    pb = X.build_unmerge_bwd(case, DEV)
    print(f"{case.name}: ties dz {pb.ties['dz']:.3f}, dx_bf16 {pb.ties['dx16']:.3f}")
    for cast in X.CAST_VARIANTS:
        bad = verdict(pb, launch(ops, pb, cast=cast), cast=cast)
        assert not bad, (case.name, f"dx_bf16 {cast}", bad)

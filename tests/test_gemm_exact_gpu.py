"""tulip_gemm_bf16, tulip_wgrad_group and tulip_reduce_rows_multi on integer operands (tests/gemm_exact.py): every fp32 output
equal to the float64 result bit for bit, every bf16 output its one round-to-nearest-even (GELU_BWD: exact where aux is 0, within one
bf16 ulp elsewhere; GELU_DUAL's out2: numerics_domain.check_gelu on the stored out), every guard word around the outputs and
behind the workspace unchanged, no NaN leaking in from the padding around the operands -- on every kernel instantiation behind
the launcher (each case first asserts, through tulip_gemm_route, that it reaches the kernel written next to its shape) with every
epilogue it takes, and identical bits across `splits`, TULIP_GEMM_CHECKED, TULIP_GEMM_MID, packed or plain B, small or large
weight-gradient tiles, fused or separate fold.  Route table and run time: DESIGN.md, "Exact GEMM tests"."""
import pytest
import torch

from tests import gemm_exact as GX

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = GX.gpu_cases()
BY_NAME = {c.name: c for c in CASES}


@pytest.fixture(scope="module")
def ops():
    from tulip_amd import ops as o
    return o


def packed_b(ops, pb):
    """fragment-major copy of the [N][K] matrix, inside NaN (1 KiB on either side)"""
    src = pb.B.view.contiguous()
    flat = GX.filled(src.numel() + 1024, GX.BF16, "nan", DEV)
    it, n = ops.pack_items([(src, flat.data_ptr() + 1024, src.shape[0], src.shape[1], 0)])
    ops.pack_bf16_multi(it, n)
    torch.cuda.synchronize()
    return flat


def launch(ops, pb, **override):
    """one tulip_gemm_bf16 call on fresh copies of the case's output allocations; override: splits / checked / mid / packed.
    The workspace is exactly effective_splits * M * N * 4 bytes, followed by guard words."""
    c = pb.case
    splits = override.get("splits", c.splits)
    is_packed = override.get("packed", c.packed)
    got = {k: o.buf.flat.clone() for k, o in pb.outs.items()}
    eff = GX.plan_splits(c.K, splits)[1]
    need = eff * c.M * c.N if eff > 1 and c.epi != GX.EPI_SPLIT_F32 else 0
    ws = GX.filled(need + 64, GX.F32, "guard", DEV)
    keep = [packed_b(ops, pb)] if is_packed else []
    o, o2 = pb.outs.get("out"), pb.outs.get("out2")
    rowsum = GX.rowsum_form(c)
    # every allocation against what the header says the launch addresses, before anything runs
    want = GX.addressed(c if splits == c.splits else GX.replace(c, splits=splits))
    have = {**{k: v.buf for k, v in pb.outs.items()}, **({"aux": pb.aux} if pb.aux is not None else {})}
    assert set(want) == set(have), (sorted(want), sorted(have))
    for k, (dtype, rows, cols) in want.items():
        b = have[k]
        assert (b.flat.dtype, b.rows, b.cols) == (dtype, rows, cols), (k, b.flat.dtype, b.rows, b.cols, dtype, rows, cols)
        assert b.off + (b.rows - 1) * b.pitch + b.cols <= b.flat.numel() and b.pitch >= b.cols
    assert (pb.A.rows, pb.A.cols) == ((c.K, c.M) if c.a_trans else (c.M, c.K))
    assert (pb.B.rows, pb.B.cols) == ((c.K, c.N) if c.b_trans else (c.N, c.K))
    assert pb.bias is None or pb.bias.cols == c.N
    assert pb.rowscale is None or pb.rowscale.cols * c.rps >= c.M
    assert c.epi not in (GX.EPI_PIXSHUF2_F32,) or c.M % (c.ps[0] * c.ps[1]) == 0
    assert c.epi not in (GX.EPI_UNSHUF2_BF16,) or c.M % (4 * c.ps[0] * c.ps[1]) == 0
    ops.gemm(pb.A.addr(), keep[0].data_ptr() + 1024 if is_packed else pb.B.addr(), c.M, c.N, c.K, lda=pb.A.pitch,
             ldb=c.K if is_packed else pb.B.pitch, a_trans=c.a_trans, b_trans=c.b_trans, epi=c.epi,
             bias=pb.bias.addr() if pb.bias is not None else None,
             out=o.buf.addr(got["out"]) if o is not None else None, ldo=o.buf.pitch if o is not None else c.N,
             out2=o2.buf.addr(got["out2"]) if o2 is not None else None, ldo2=0 if (o2 is None or rowsum) else o2.buf.pitch,
             aux=pb.aux.addr() if pb.aux is not None else None, ldaux=pb.aux.pitch if pb.aux is not None else 0,
             rowscale=pb.rowscale.addr() if pb.rowscale is not None else None, rows_per_sample=c.rps,
             accumulate=c.accumulate, psH=c.ps[0], psW=c.ps[1], splits=splits, workspace=ws if need else None,
             workspace_bytes=need * 4, checked=override.get("checked", c.checked),
             mid=True if override.get("mid", c.mid) else None, b_packed=is_packed)
    torch.cuda.synchronize()
    got["ws"] = ws
    return got, need


def verify(pb, got, need, route):
    bad = GX.failures(GX.check_all(pb, got, route))
    tail = got["ws"].view(torch.int32)[need:]
    if not bool((tail == GX.GUARD32).all()):
        bad.append(f"{int((tail != GX.GUARD32).sum())} guard words behind the {need * 4} workspace bytes changed")
    return bad


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_gemm_is_exact(ops, case):
    r = GX.route_name(ops.gemm_route(case.M, case.N, case.K, **case.route_args()))
    assert r == case.route, f"{case.M} x {case.N} x {case.K} no longer reaches {case.route}: the launcher sends it to {r}"
    pb = GX.build(case, DEV)
    got, need = launch(ops, pb)
    bad = verify(pb, got, need, r)
    assert not bad, bad


def same_bits(a, b):
    return [k for k in a if k != "ws" and not torch.equal(a[k].view(torch.int16), b[k].view(torch.int16))]


@pytest.mark.parametrize("name", ["t64-nn-ragged-bf16", "t64-tt-ragged-resid", "t64-nn-ragged-f32-v1", "t64-nt-ragged-resid", "t64d-nn-k264-gelu_dual",
                                  "t64d-tn-k264-gelu_bwd", "t64-tn-ragged-unshuf", "t64-nt-ragged-pixshuf", "mid-nn-f32",
                                  "stream1536-bf16"])
def test_result_does_not_depend_on_splits(ops, name):
    """splits in {1, 2, 3, 7}: the same bits -- each launch also checked against the reference and its own workspace guard"""
    case = BY_NAME[name]
    pb = GX.build(case, DEV)
    first = None
    for splits in (1, 2, 3, 7):
        if case.packed and not ops.gemm_packed_supported(case.M, case.N, case.K, splits):
            continue
        r = GX.route_name(ops.gemm_route(case.M, case.N, case.K, **{**case.route_args(), "splits": splits}))
        got, need = launch(ops, pb, splits=splits)
        assert need == (GX.plan_splits(case.K, splits)[1] * case.M * case.N if GX.plan_splits(case.K, splits)[1] > 1 else 0)
        bad = verify(pb, got, need, r)
        assert not bad, (splits, r, bad)
        first = first or got
        assert not same_bits(first, got), (splits, same_bits(first, got))


@pytest.mark.parametrize("name,override,other", [
    ("f64-nn-bf16", dict(checked=True), "tile64/nn"), ("f64-nt-resid", dict(checked=True), "tile64/nt"),
    ("f64d-nn-f32-v1", dict(checked=True), "tile64-deep/nn"), ("f64d-nt-gelu_dual", dict(checked=True), "tile64-deep/nt"),
    ("f128-nn-bf16", dict(checked=True), "tile128/nn"), ("f256-nt-f32", dict(checked=True), "tile256/nt"),
    ("mid-nn-bf16", dict(mid=False), "full64/nn"), ("mid-nt-ragged-resid", dict(mid=False), "tile64/nt"),
    ("mid-split2-f32", dict(mid=False), "tile64/nn"),
    ("stream96-bf16", dict(packed=False), "full64/nn"), ("stream384-resid", dict(packed=False), "full64-deep/nn"),
    ("stream768-f32", dict(packed=False), "full64-deep/nn"), ("stream1536-pixshuf", dict(packed=False), "full64-deep/nn"),
    ("stream384-split2-f32-v1", dict(packed=False), "tile64-deep/nn")])
def test_twin_kernels_give_identical_bits(ops, name, override, other):
    """TULIP_GEMM_CHECKED against the unchecked kernel, the mid kernel against the tile kernels, packed against plain B"""
    case = BY_NAME[name]
    args = {**case.route_args(), **{"b_packed" if k == "packed" else k: (v if k != "mid" else None) for k, v in override.items()}}
    assert GX.route_name(ops.gemm_route(case.M, case.N, case.K, **args)) == other
    pb = GX.build(case, DEV)
    a, need_a = launch(ops, pb)
    b, need_b = launch(ops, pb, **override)
    assert not verify(pb, a, need_a, case.route) and not verify(pb, b, need_b, other)
    assert not same_bits(a, b), same_bits(a, b)


def test_folded_weight_gradient_form_refuses_row_sums(ops):
    """regression: a_trans, TULIP_EPI_F32, out2 = row sums and splits > 1 used to run and never write out2; the launcher now refuses
    before any launch (the sums exist unsplit or as TULIP_EPI_SPLIT_F32 slabs), and nothing is touched"""
    from tulip_amd import _lib
    case = GX.replace(BY_NAME["t64-tt-ragged-f32-v1"], name="rowsum-fold", splits=1)
    pb = GX.build(case, DEV)
    with pytest.raises(_lib.TulipHipError):
        launch(ops, pb, splits=3)
    got, need = launch(ops, pb)
    assert not verify(pb, got, need, case.route)


def test_split_slabs_folded_by_reduce_splits(ops):
    """TULIP_EPI_SPLIT_F32 slabs [splits][M][N] (ldo = N), folded into an accumulating output by tulip_reduce_splits"""
    case = GX.with_epilogue(GX.Case("slabs", 200, 104, 200, "tile64/nt", b_trans=True, splits=3, tight_out=True), GX.EPI_SPLIT_F32)
    pb = GX.build(case, DEV)
    got, need = launch(ops, pb)
    assert not verify(pb, got, need, case.route)
    gen = torch.Generator().manual_seed(5)
    o = GX.Buf(1, case.M * case.N, case.M * case.N + 8, GX.F32, "guard", DEV).set(GX.ints(gen, (1, case.M * case.N), -1000, 1000, DEV))
    want = GX.Out(o, GX._image(o, o.index(), o.view.to(GX.F64) + pb.acc.reshape(1, -1)), o.index())
    res = o.flat.clone()
    ops.reduce_splits(pb.outs["out"].buf.addr(got["out"]), o.addr(res), case.M * case.N, 3)
    torch.cuda.synchronize()
    rep = GX.check_out("reduce_splits", want, res)
    assert rep.ok, str(rep)


# ------------------------------------------------------------------ grouped weight gradient
def run_wgrad(ops, pb, fold=True, small_tiles=False, extra=(), separate_fold=False):
    dW = [o.buf.flat.clone() for o in pb.dW]
    db = [None if o is None else o.buf.flat.clone() for o in pb.db]
    ws = pb.ws.clone()
    items = [ops.wgrad_item(pb.dY[i].addr(), pb.dY[i].pitch, pb.X[i].addr(), pb.X[i].pitch, it.Nw, it.Kw, it.Mtok,
                            pb.dW[i].buf.addr(dW[i]), None if db[i] is None else pb.db[i].buf.addr(db[i]), it.splits, it.overwrite)
             for i, it in enumerate(pb.items)]
    ops.wgrad_group(items, list(extra), ws, pb.ws_need * 4, fold=fold and not separate_fold, small_tiles=small_tiles)
    if separate_fold:
        ops.reduce_rows_multi(ops.wgrad_group_regions(items, ws) + list(extra))
    torch.cuda.synchronize()
    return dW, db, ws


def region_of(ops, r, out_flat):
    return ops.reduce_region(r.part.addr(), r.part.pitch, r.out.buf.addr(out_flat), r.n, r.rows, overwrite=r.overwrite,
                             scatter_index=r.index, scatter_nh=r.nh, scatter_len=r.length)


@pytest.mark.parametrize("name", list(GX.wgrad_groups()))
def test_wgrad_group_is_exact(ops, name):
    items, want = GX.wgrad_groups()[name]
    kind, tiles = GX.wgrad_kernel([(i.Mtok, i.Nw, i.Kw) for i in items])
    assert kind == want and all(ops.wgrad_tiles(i.Nw, i.Kw, small_tiles=(kind == "small")) == t for i, t in zip(items, tiles))
    pb = GX.build_wgrad(items, DEV)
    # extra regions ride along in the fold launch: a plain one and a scattered one
    extras = [GX.build_region(37, 200, 208, False, DEV, seed=1), GX.build_region(9, 3 * 256, 3 * 256 + 4, False, DEV, seed=2, scatter=(3, 256, 45))]
    ex_out = [r.out.buf.flat.clone() for r in extras]
    dW, db, ws = run_wgrad(ops, pb, extra=[region_of(ops, r, f) for r, f in zip(extras, ex_out)])
    bad = GX.failures(GX.check_wgrad(pb, dW, db, ws, what=f"{name}."))
    bad += GX.failures([GX.check_out(f"extra{i}", r.out, f) for i, (r, f) in enumerate(zip(extras, ex_out))])
    assert not bad, bad
    # TULIP_WGRAD_SMALL_TILES, and fold = 0 followed by tulip_wgrad_group_regions + tulip_reduce_rows_multi: the same bits
    for kw in (dict(small_tiles=True), dict(separate_fold=True), dict(small_tiles=True, separate_fold=True)):
        dW2, db2, ws2 = run_wgrad(ops, pb, **kw)
        bad = GX.failures(GX.check_wgrad(pb, dW2, db2, ws2, what=f"{name}{sorted(kw)}."))
        assert not bad, bad
        for a, b in zip(dW + [d for d in db if d is not None], dW2 + [d for d in db2 if d is not None]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, kw)


def test_wgrad_group_without_fold_leaves_the_slabs(ops):
    """fold = 0: un-split items are complete, split items untouched (their slabs wait in the workspace), guard words intact"""
    items, _ = GX.wgrad_groups()["192x192"]
    pb = GX.build_wgrad(items, DEV)
    dW, db, ws = run_wgrad(ops, pb, fold=False)
    assert GX.check_out("unsplit", pb.dW[0], dW[0]).ok and GX.check_out("unsplit.db", pb.db[0], db[0]).ok
    assert torch.equal(dW[1].view(torch.int32), pb.dW[1].buf.flat.view(torch.int32))
    assert bool((ws.view(torch.int32)[pb.ws_need:] == GX.GUARD32).all())
    slabs = ws[:pb.ws_need].reshape(2, 384 * 192).to(GX.F64).sum(0).reshape(384, 192)
    assert torch.equal(slabs, pb.dY[1].view.to(GX.F64).t() @ pb.X[1].view.to(GX.F64))


# ------------------------------------------------------------------ the row fold alone
@pytest.mark.parametrize("name,rows,n,stride,overwrite,scatter", GX.region_cases(), ids=[r[0] for r in GX.region_cases()])
def test_reduce_rows_multi_is_exact(ops, name, rows, n, stride, overwrite, scatter):
    r = GX.build_region(rows, n, stride, overwrite, DEV, scatter=scatter)
    out = r.out.buf.flat.clone()
    ops.reduce_rows_multi([region_of(ops, r, out)])
    torch.cuda.synchronize()
    rep = GX.check_out(name, r.out, out)
    assert rep.ok, str(rep)


def test_reduce_rows_multi_48_regions(ops):
    from tulip_amd import _lib
    regs = [GX.build_region(1 + 5 * (k % 7), 8 + 4 * k, 8 + 4 * k + 4 * (k % 3 + 1), bool(k % 2), DEV, seed=k)
            for k in range(_lib.REDUCE_REGIONS_MAX - 2)]
    regs += [GX.build_region(9, 3 * 256, 3 * 256 + 4, False, DEV, seed=90, scatter=(3, 256, 45)),
             GX.build_region(3, 2 * 1024, 2 * 1024 + 8, False, DEV, seed=91, scatter=(2, 1024, 105))]
    assert len(regs) == 48
    outs = [r.out.buf.flat.clone() for r in regs]
    ops.reduce_rows_multi([region_of(ops, r, f) for r, f in zip(regs, outs)])
    torch.cuda.synchronize()
    bad = GX.failures([GX.check_out(f"region{k}", r.out, f) for k, (r, f) in enumerate(zip(regs, outs))])
    assert not bad, bad

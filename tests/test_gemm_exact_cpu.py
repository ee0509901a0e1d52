"""CPU: the exact-GEMM test kit (tests/gemm_exact.py) is sharp and its case list complete.

1. A torch emulation of the launch (fp32 accumulation over 32-deep k chunks, the K range cut as the launcher cuts it, slabs folded
   in order, results stored by address) passes every checker, and each of eleven plausible kernel defects is rejected by at least
   one of them.
2. Route coverage through tulip_gemm_route (host code: no GPU): every case of test_gemm_exact_gpu.py reaches the kernel written
   next to its shape, together the cases reach every kernel instantiation behind tulip_gemm_bf16 -- enumerated here from the
   header's encoding -- and every (kernel, epilogue) pair the launcher accepts.  A dispatch change that adds, removes or moves a
   route fails here until the case list follows."""
import pytest
import torch

from tests import gemm_exact as GX
from tulip_amd import _lib, ops

CASES = GX.gpu_cases()
SMALL = [c for c in CASES if c.M * c.N <= 1 << 15 and c.K <= 300]


def test_float64_reference_is_the_integer_product():
    """the float64 matmul of the references against an int64 matmul, once, at the largest depth the cases use"""
    g = torch.Generator().manual_seed(1)
    K = max(c.K for c in CASES)
    a, b = torch.randint(-8, 9, (200, K), generator=g), torch.randint(-8, 9, (104, K), generator=g)
    assert torch.equal((a.to(GX.F64) @ b.to(GX.F64).t()).to(torch.int64), a @ b.t())
    assert K * 64 + 64 < GX.EXACT_LIMIT


@pytest.mark.parametrize("epi", GX.EPIS, ids=lambda e: GX.EPI_NAMES[e])
def test_emulation_passes_every_checker(epi):
    cases = [c for c in SMALL if c.epi == epi]
    assert len(cases) >= 8
    for c in cases:
        pb = GX.build(c)
        assert pb.ties >= GX.MIN_TIES or not any(o.buf.flat.dtype == GX.BF16 for o in pb.outs.values())
        bad = GX.failures(GX.check_all(pb, GX.emulate(pb)))
        assert not bad, (c.name, bad)


# defect -> the cases it is tried on (a defect only shows where the launch has the feature it breaks)
DEFECT_CASES = {
    "truncate": ["t64-nn-ragged-bf16", "t64-tt-ragged-unshuf", "split3-nn-f32"],
    "half_away": ["t64-nn-ragged-bf16", "t64-nt-ragged-pixshuf", "f64-nn-gelu_dual"],
    "drop_k_tail": ["t64-nn-ragged-bf16", "t64d-tt-k264-f32", "split3-nn-split"],
    "overread_last_split": ["t64-nn-ragged-f32", "split3-tt-bf16", "t64-tn-k48-resid"],
    "row_past_m": ["t64-nn-ragged-bf16", "f64-nt-f32", "split3-nn-split"],
    "pitch_spill": ["t64-nn-ragged-resid", "f64-nn-bf16", "t64-tt-ragged-gelu_bwd"],
    "ldb_is_k": ["t64-nt-ragged-bf16", "t64-tt-k48-f32"],
    "bias_per_split": ["split3-nn-bf16", "split3-tt-resid", "split7-nt-resid"],
    "fold_skips_slab0": ["split3-nn-gelu_bwd", "split3-tt-f32", "split2-deep-bf16"],
    "accumulate_ignored": ["t64-nn-ragged-f32-v1", "t64-tt-ragged-f32-v1"],
    "pixshuf_swapped": ["t64-nn-ragged-pixshuf", "t64-tn-k48-pixshuf-v1"],
}


def test_the_defect_list_is_the_emulators():
    assert set(DEFECT_CASES) == set(GX.DEFECTS)


@pytest.mark.parametrize("defect", GX.DEFECTS)
def test_each_defect_is_rejected(defect):
    by_name = {c.name: c for c in CASES}
    for name in DEFECT_CASES[defect]:
        pb = GX.build(by_name[name])
        assert not GX.failures(GX.check_all(pb, GX.emulate(pb))), name
        bad = GX.failures(GX.check_all(pb, GX.emulate(pb, defect)))
        assert bad, f"{defect} passes every checker on {name}"
        if defect in ("row_past_m", "pitch_spill"):
            assert "guard word" in " ".join(bad), bad          # named as what it is: a word beside the tensor


def test_reports_name_element_tile_and_guard_word():
    c = next(c for c in CASES if c.name == "t64-nn-ragged-bf16")
    pb = GX.build(c)
    got = GX.emulate(pb)
    o = pb.outs["out"].buf
    got["out"][o.off + 130 * o.pitch + 100] = 1.0
    (rep,) = [r for r in GX.check_all(pb, got) if not r.ok]
    assert "element [130][100] (tile (2, 1), row 2, column 4 of it)" in str(rep)
    got = GX.emulate(pb)
    got["out"][o.off + 3 * o.pitch + c.N] = 1.0                # the first word of row 3's pitch gap
    (rep,) = [r for r in GX.check_all(pb, got) if not r.ok]
    assert f"guard word {o.off + 3 * o.pitch + c.N} (allocation row 3, column {c.N}" in str(rep)
    # workspace: one word past the required bytes
    c = next(c for c in CASES if c.name == "split3-nn-bf16")
    pb = GX.build(c)
    assert pb.ws_need == 3 * c.M * c.N and pb.ws.numel() > pb.ws_need
    got = GX.emulate(pb)
    got["ws"][pb.ws_need] = 0.0
    assert any("workspace" in f for f in GX.failures(GX.check_all(pb, got)))


def test_a_nan_that_leaks_in_from_padding_is_seen():
    """every operand is surrounded by NaN: an address one row or one column off poisons whole output rows"""
    c = next(c for c in CASES if c.name == "t64-nn-ragged-f32")
    pb = GX.build(c)
    assert torch.isnan(pb.A.flat.float()).sum() == pb.A.flat.numel() - c.M * c.K
    assert torch.isnan(pb.B.flat.float()).sum() == pb.B.flat.numel() - c.N * c.K
    pb.A.off += 8                                              # the operand pointer eight elements late
    assert GX.failures(GX.check_all(pb, GX.emulate(pb)))


# ------------------------------------------------------------------ route coverage (tulip_gemm_route: host code only)
def _route(c):
    return ops.gemm_route(c.M, c.N, c.K, **c.route_args())


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_reaches_the_route_written_next_to_its_shape(case):
    r = _route(case)
    assert GX.route_name(r) == case.route, (f"{case.M} x {case.N} x {case.K} (splits {case.splits}) no longer reaches {case.route}: "
                                            f"the launcher sends it to {GX.route_name(r)}")
    kchunk, eff = GX.plan_splits(case.K, case.splits)
    assert GX.route_splits(r) == eff == ops.gemm_effective_splits(case.K, case.splits)
    assert GX.route_folds(r) == (eff > 1 and case.epi != GX.EPI_SPLIT_F32)


def test_the_cases_reach_every_route_and_every_epilogue_on_it():
    reach = GX.reachable_routes()
    assert len(reach) == 28
    seen = {(GX.route_name(_route(c)), c.epi) for c in CASES}
    got = {r for r, _ in seen}
    assert got - reach == set(), f"routes the header's encoding does not list: {sorted(got - reach)}"
    assert reach - got == set(), f"kernels no case reaches: {sorted(reach - got)}"
    missing = [(r, GX.EPI_NAMES[e]) for r in sorted(reach) for e in GX.EPIS if GX.route_accepts(r, e) and (r, e) not in seen]
    assert not missing, missing
    # the fold kernel behind every family, and every epilogue it takes
    folded = {(GX.route_name(r)[:3], c.epi) for c in CASES for r in [_route(c)] if GX.route_folds(r)}
    assert {e for _, e in folded} == set(GX.EPIS) - {GX.EPI_SPLIT_F32}
    assert {f for f, _ in folded} >= {"til", "mid", "str"}


def test_a_sweep_of_the_launcher_finds_no_route_outside_the_list():
    """shapes across both tile-count thresholds, every layout and flag: whatever tulip_gemm_route answers is one of the twenty-eight"""
    reach, seen = GX.reachable_routes(), set()
    for M in (8, 64, 72, 128, 200, 2048, 3000, 4096, 8192):
        for N in (8, 96, 104, 192, 3064, 3072):
            for K in (32, 48, 96, 256, 264, 384, 768, 1536, 3072):
                for at in (False, True):
                    for bt in (False, True):
                        for flags in ({}, {"checked": True}, {"mid": True}, {"b_packed": True}):
                            for splits in (1, 2, 5):
                                if flags.get("b_packed") and (at or bt or not ops.gemm_packed_supported(M, N, K, splits)):
                                    continue
                                seen.add(GX.route_name(ops.gemm_route(M, N, K, a_trans=at, b_trans=bt, splits=splits, **flags)))
    assert seen <= reach, sorted(seen - reach)
    assert seen == reach, sorted(reach - seen)


def test_route_refuses_what_the_launcher_refuses():
    lib = _lib.load()
    E = -1
    assert lib.tulip_gemm_route(64, 96, 36, 0, 0, 0, 0, 1) == E            # K % 8
    assert lib.tulip_gemm_route(64, 100, 32, 0, 0, 0, 0, 1) == E           # N % 8
    assert lib.tulip_gemm_route(60, 96, 32, 1, 0, 0, 0, 1) == E            # M % 8 with a transposed A
    assert lib.tulip_gemm_route(60, 96, 32, 0, 0, 0, 0, 1) >= 0
    assert lib.tulip_gemm_route(0, 96, 32, 0, 0, 0, 0, 1) == E             # empty: nothing is launched
    assert lib.tulip_gemm_route(64, 96, 256, 0, 0, 0, _lib.GEMM_B_PACKED, 1) == E
    assert lib.tulip_gemm_route(64, 96, 96, 0, 1, 0, _lib.GEMM_B_PACKED, 1) == E
    with pytest.raises(_lib.TulipHipError):
        ops.gemm_route(64, 96, 36)
    # the mid kernel only where it fits: else the tile kernels, silently (the flag is a wish)
    assert GX.route_name(ops.gemm_route(200, 200, 96, mid=True)) == "tile64/nn"
    assert GX.route_name(ops.gemm_route(200, 200, 128, mid=True, epi=GX.EPI_PIXSHUF2_F32)) == "tile64/nn"
    assert GX.route_name(ops.gemm_route(200, 200, 128, mid=True, a_trans=True)) == "tile64/tn"


# ------------------------------------------------------------------ grouped weight gradient, row fold
@pytest.mark.parametrize("name", list(GX.wgrad_groups()))
def test_wgrad_group_expectation_through_wgrad_tiles(name):
    """the rule of gemm_exact.wgrad_kernel against tulip_wgrad_tiles: per item the tiles of the kernel the group gets"""
    items, want = GX.wgrad_groups()[name]
    kind, tiles = GX.wgrad_kernel([(i.Mtok, i.Nw, i.Kw) for i in items])
    assert kind == want
    small = [-(-i.Nw // 64) * -(-i.Kw // 96) for i in items]
    for it, s in zip(items, small):
        assert ops.wgrad_tiles(it.Nw, it.Kw, small_tiles=True) == s
    if want == "large":
        # every item has a large-tile shape (tulip_wgrad_tiles reports fewer, larger tiles) and whole 32-token steps
        for it, t, s in zip(items, tiles, small):
            assert ops.wgrad_tiles(it.Nw, it.Kw) == t < s and it.Mtok % 32 == 0, (name, it)
    else:
        # one item without a large-tile shape (tulip_wgrad_tiles reports the 64 x 96 count) or with a ragged token count
        assert tiles == small
        assert any(ops.wgrad_tiles(it.Nw, it.Kw) == s or it.Mtok % 32 for it, s in zip(items, small)), name


def test_wgrad_and_region_builders_and_checkers():
    items, _ = GX.wgrad_groups()["64x96"]
    pb = GX.build_wgrad(items)
    assert pb.ws_need == (64 * 104 + 64) * 3 and pb.ws.numel() == pb.ws_need + 64
    want_w = [o.want.view(GX.F32) for o in pb.dW]
    want_b = [None if o is None else o.want.view(GX.F32) for o in pb.db]
    assert not GX.failures(GX.check_wgrad(pb, want_w, want_b, pb.ws))
    # accumulate ignored on item 0 / a store past the gradient's last row on item 1
    wrong = [w.clone() for w in want_w]
    o = pb.dW[0].buf
    wrong[0][o.off:o.off + o.rows * o.pitch] -= o.view.reshape(-1)
    assert GX.failures(GX.check_wgrad(pb, wrong, want_b, pb.ws))
    wrong = [w.clone() for w in want_w]
    o = pb.dW[1].buf
    wrong[1][o.off + o.rows * o.pitch] = 0.0
    assert any("guard" in f for f in GX.failures(GX.check_wgrad(pb, wrong, want_b, pb.ws)))
    for name, rows, n, stride, ov, sc in GX.region_cases():
        r = GX.build_region(rows, n, stride, ov, scatter=sc)
        good = r.out.want.view(GX.F32)
        assert GX.check_out(name, r.out, good).ok
        bad = good.clone()
        bad[r.out.idx.reshape(-1)[-1]] += 1.0
        assert not GX.check_out(name, r.out, bad).ok

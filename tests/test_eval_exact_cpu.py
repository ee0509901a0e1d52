"""CPU: the evaluation-kernel test kit (tests/eval_exact.py) is sharp and its case lists complete.

1. Every builder holds its conditions (asserted inside the builders), the planted Chamfer reference agrees with float64 brute force on
   512 sampled rows each way, the numpy emulation of every launch passes every checker on every case, and each listed defect, switched
   on alone, is rejected by at least one case.
2. The Chamfer cases reach the routes written next to them -- computed from launch_nn's documented rule -- and together every route class.
3. Refusals: the launchers check their arguments before any launch, so they are called here with dummy pointers."""
import functools

import numpy as np
import pytest
import torch

from tests import eval_exact as X
from tests import numerics_domain as ND
from tulip_amd import _lib


@functools.lru_cache(maxsize=None)
def chamfer_problem(name):
    (c,) = [c for c in X.chamfer_cases() if c.name == name]
    return X.build_chamfer(c)


@functools.lru_cache(maxsize=None)
def voxel_list():
    return X.voxel_problems()


@functools.lru_cache(maxsize=None)
def voxel_problems():
    return {p.name: p for p in voxel_list()}


@functools.lru_cache(maxsize=None)
def post_problem(name):
    (c,) = [c for c in X.post_cases() if c.name == name]
    return X.build_post(c)


def chamfer_verdict(pb, defect=None, bufs=None):
    bufs = X.emulate_chamfer(pb, bufs or X.alloc_chamfer(pb), defect)
    return X.failures([X.check_chamfer(pb, bufs)])


def voxel_verdict(pb, defect=None, scratch=None):
    bufs = X.emulate_voxel(pb, X.alloc_voxel(pb, scratch=scratch), defect)
    return X.failures([X.check_voxel(pb, bufs)]), bufs


def post_verdict(pb, keep, defect=None):
    bufs = X.emulate_post(pb, X.alloc_post(pb), keep, defect)
    return X.failures([X.check_post(pb, bufs, keep)]), bufs


# ------------------------------------------------------------------ case lists and routes
def test_case_lists():
    for names in ([c.name for c in X.chamfer_cases()], [c.name for c in X.post_cases()], [p.name for p in voxel_list()]):
        assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    assert X.largest_buffer_bytes() <= X.MAX_BUFFER_BYTES
    for p in voxel_problems().values():
        assert max(p.pred.nbytes, p.gt.nbytes, p.words * 4) <= X.MAX_BUFFER_BYTES
    sizes = {(c.na, c.nb) for c in X.chamfer_cases()}
    assert {(1, 1), (1, 1024), (1, 1025), (255, 1023), (1024, 2048), (1025, 3073), (40960, 54273), (262444, 1), (1, 262444)} <= sizes
    small = [c for c in X.chamfer_cases() if c.kind != "planted"]
    assert {c.f64 for c in small} == {False, True} and len([c for c in small if c.f64]) == len(small) // 2
    assert {(c.H, c.h, c.W) for c in X.post_cases()} >= {(4, 1, 3), (4, 4, 5), (6, 2, 255), (8, 2, 257), (132, 33, 2048)}
    assert any(c.w and c.w != c.W for c in X.post_cases()) and sum(c.logt for c in X.post_cases()) == 1
    # the second trip of every capped grid-stride loop: 1024 blocks x 256 (4096 x 256 for mc_aggregate)
    assert 132 * 2048 > 262144 and 130 * 2048 > 262144 and 128 * 2056 > 262144 and X.MC_N > 1048576


def test_chamfer_cases_reach_the_routes_written_next_to_them():
    traits = set()
    for c in X.chamfer_cases():
        assert X.nn_route(c.na, c.nb) == c.route_ab and X.nn_route(c.nb, c.na) == c.route_ba, (c.name, X.nn_route(c.na, c.nb), X.nn_route(c.nb, c.na))
        traits |= X.route_traits(c.na, c.nb) | X.route_traits(c.nb, c.na)
        if X.reduction_blocks(c.na, c.nb) > X.RB:
            traits.add("reduction-stride")
    assert traits >= {"partial-tile", "full-tile", "one-point-last-slice", "two-tiles-ragged", "two-tiles-full", "many-query-blocks",
                      "reduction-stride"}, traits
    by = {c.name: c for c in X.chamfer_cases()}
    p = by["planted-40960x54273"]
    assert p.route_ab == (40, 27, 2, 1025) and p.route_ba == (54, 20, 2, 2048)          # the last slice's second tile holds one point
    assert by["stride-262444x1-f32"].route_ab[0] == 257 and X.reduction_blocks(262444, 1) == 1026
    assert by["stride-1x262444-f32"].route_ab == (1, 257, 1, 300)


# ------------------------------------------------------------------ Chamfer
@pytest.mark.parametrize("case", X.chamfer_cases(), ids=lambda c: c.name)
def test_chamfer_emulation_passes(case):
    pb = chamfer_problem(case.name)
    assert pb.a.dtype == (np.float64 if case.f64 else np.float32)
    bufs = X.emulate_chamfer(pb, X.alloc_chamfer(pb))
    rep = X.check_chamfer(pb, bufs)
    print(rep.line())
    assert rep.ok, str(rep)                                           # (unfused fp32 arithmetic: up to 0.71 of the budget)
    untouched = X.check_chamfer(pb, X.alloc_chamfer(pb))              # NaN prefill: nothing written is every element wrong
    assert not untouched.ok


def test_planted_reference_against_sampled_brute_force():
    pb = chamfer_problem("planted-40960x54273")
    rng = np.random.default_rng(0)
    a64, b64 = pb.a32.astype(np.float64), pb.b32.astype(np.float64)
    for q, t, ref in ((a64, b64, pb.dist_a), (b64, a64, pb.dist_b)):
        rows = rng.choice(q.shape[0], 512, replace=False)
        bf = X.brute_nn(q[rows], t, chunk=64)
        assert np.abs(bf - ref[rows]).max() <= 1e-12 * ref[rows].max()
    # adversarial placement: the only partner of a query sits at index 0, on both sides of every tile and slice edge and at the end
    qs, ts = X.planted_specials(pb.case.na, pb.case.nb)
    assert {0, 1023, 1024, 2047, 2048, 53247, 53248, pb.case.nb - 1} <= set(ts) and {0, 255, 257, 1023, 1025, pb.case.na - 1} <= set(qs)
    count = np.bincount(pb.cand_b, minlength=pb.case.na)
    for j in ts:
        assert count[pb.cand_b[j]] == 1
    assert bool((count[qs] == 1).all()) and int(count.max()) > 1
    # a dropped partner shows as at least (0.51 s)^2 where |delta|^2 < (0.49 s)^2 is expected
    assert pb.dist_a.max() < (0.49 * X.SPACING) ** 2 < (0.51 * X.SPACING) ** 2


CHAMFER_DEFECT_CASES = {
    "drop_last_target": ["1x1025-f32", "255x1023-f32", "planted-40960x54273"],
    "pad_origin": ["planted-40960x54273", "ring-300x700-f32", "ring-300x700-f64"],
    "skip_tile2": ["planted-40960x54273"],
    "queries_256": ["1025x3073-f32", "1024x2048-f64"],
    "swap_dist": ["255x1023-f32", "1x1025-f64"],
    "swap_inv": ["255x1023-f32", "1x1025-f32"],
    "gemm_form": ["far-700x1100-f32", "far-700x1100-f64"],
    "f64_as_f32": ["255x1023-f64", "1x1-f64"],
}


def test_the_defect_lists_are_the_emulators():
    assert set(CHAMFER_DEFECT_CASES) | {"stale_min"} == set(X.CHAMFER_DEFECTS)
    assert set(VOXEL_DEFECT_CASES) == set(X.VOXEL_DEFECTS) and set(POST_DEFECT_CASES) == set(X.POST_DEFECTS)
    assert set(XYZ_DEFECT_CASES) == set(X.XYZ_DEFECTS)


@pytest.mark.parametrize("defect", sorted(CHAMFER_DEFECT_CASES))
def test_each_chamfer_defect_is_rejected(defect):
    for name in CHAMFER_DEFECT_CASES[defect]:
        pb = chamfer_problem(name)
        bad = chamfer_verdict(pb, defect)
        assert bad, f"{defect} passes on {name}"


def test_minima_that_are_not_reset_are_seen():
    first, second = X.stale_pair()
    bufs = X.emulate_chamfer(first, X.alloc_chamfer(first))
    assert X.check_chamfer(first, bufs).ok
    bufs["a"], bufs["b"] = X.alloc_chamfer(second)["a"], X.alloc_chamfer(second)["b"]
    assert not chamfer_verdict(second, None, bufs)
    bufs = X.emulate_chamfer(first, X.alloc_chamfer(first))
    bufs["a"], bufs["b"] = X.alloc_chamfer(second)["a"], X.alloc_chamfer(second)["b"]
    assert chamfer_verdict(second, "stale_min", bufs)
    # on NaN-prefilled buffers the same defect is invisible: the sequence is needed
    assert not chamfer_verdict(second, "stale_min")


def test_a_written_guard_word_is_seen():
    pb = chamfer_problem("255x1023-f32")
    bufs = X.emulate_chamfer(pb, X.alloc_chamfer(pb))
    bufs["dist_a"].flat[X.NG + pb.case.na] = 1.0
    assert "guard" in " ".join(X.failures([X.check_chamfer(pb, bufs)]))
    p = voxel_problems()["capacity-4x4x8-4words-f32"]
    bufs = X.emulate_voxel(p, X.alloc_voxel(p))
    bufs["bm_gt"].flat[X.NG + p.words] = 0                            # a word beyond bitmap_words
    assert "guard" in " ".join(X.failures([X.check_voxel(p, bufs)]))


# ------------------------------------------------------------------ voxel metrics
def test_voxel_emulation_passes_every_case():
    kept = {}
    for name, pb in voxel_problems().items():
        bad, bufs = voxel_verdict(pb, scratch=kept[pb.after]["scratch"] if pb.after else None)
        assert not bad, (name, bad)
        kept[name] = bufs
        untouched = X.alloc_voxel(pb)
        assert not X.check_voxel(pb, untouched).ok
    for tn in ("f32", "f64"):
        assert voxel_problems()[f"capacity-4x5x7-5words-{tn}"].after and voxel_problems()[f"capacity-4x4x8-after-refusal-{tn}"].after


def test_face_lattices_sit_on_faces():
    """the share of lattice points that another division moves to another voxel: the cases are where the rounding decides"""
    for name, pb in voxel_problems().items():
        if not name.startswith("faces") or not name.endswith("f32"):
            continue
        both = np.vstack((pb.pred, pb.gt))
        mn, g = both.min(0), np.float32(X.GRID)
        right = ((both - mn) / g).astype(int)
        low = (np.nextafter((both - mn) / g, np.float32(-1))).astype(int)
        wide = ((both.astype(np.float64) - mn) / 0.1).astype(int)
        axis = int(name.split("axis")[1][0])
        moved_low = float((right != low)[:, axis].mean())
        moved_wide = float((right != wide)[:, axis].mean())
        print(f"{name}: a quotient 1 ulp low moves {moved_low:.3f}, float64 arithmetic {moved_wide:.3f}")
        assert moved_low > 0.5 and moved_wide > 0.1, (name, moved_low, moved_wide)


VOXEL_DEFECT_CASES = {
    "mul_inv_grid": ["faces-min-79.3-axis0-f32", "faces-min-79.3-axis2-f32", "faces-min-12.625-axis1-f64"],
    "f64_on_f32": ["faces-min0.0-axis1-f32", "faces-min-79.3-axis2-f32"],
    "f32_on_f64": ["faces-min0.0-axis0-f64", "faces-min-12.625-axis1-f64"],
    "minmax_one_cloud": ["minimum-from-gt-f32", "minimum-from-gt-f64"],
    "count_duplicates": ["duplicates-f32"],
    "dims_no_plus1": ["axis-maximum-f32", "all-identical-f64"],
    "round_not_trunc": ["unequal-3000-700-f32"],
    "capacity_ge": ["capacity-4x4x8-4words-f32", "capacity-4x4x8-4words-f64"],
    "dirty_bitmap": ["one-point-same-voxel-f32", "stride-262444x5-f64"],
    "swap_pr": ["unequal-3000-700-f64", "pred-inside-gt-f32"],
}


@pytest.mark.parametrize("defect", sorted(VOXEL_DEFECT_CASES))
def test_each_voxel_defect_is_rejected(defect):
    for name in VOXEL_DEFECT_CASES[defect]:
        pb = voxel_problems()[name]
        bad, _ = voxel_verdict(pb, defect)
        assert bad, f"{defect} passes on {name}"


def test_multiplying_by_the_reciprocal_shows_only_off_zero():
    """at min = 0 (and at -12.625, which float32 subtracts exactly) a float32 multiply by 1/grid moves no lattice point: -79.3 is
    what rejects it in float32"""
    for axis in range(3):
        bad, _ = voxel_verdict(voxel_problems()[f"faces-min0.0-axis{axis}-f32"], "mul_inv_grid")
        assert not bad


# ------------------------------------------------------------------ post-processing
@pytest.mark.parametrize("case", X.post_cases(), ids=lambda c: c.name)
def test_post_emulation_passes(case):
    pb = post_problem(case.name)
    mae = {}
    for keep in (0.0, X.KEEP):
        bad, bufs = post_verdict(pb, keep)
        assert not bad, (case.name, keep, bad)
        mae[keep] = bufs["mae"].arr().copy()
        assert not X.check_post(pb, X.alloc_post(pb), keep).ok
    assert np.array_equal(mae[0.0], mae[X.KEEP])                      # keep_close acts after both MAE
    r0, r1 = X.post_ref(pb, 0.0), X.post_ref(pb, X.KEEP)
    assert r0["mae"] == r1["mae"] and r0["mae_low"] == r1["mae_low"]
    if case.lw != case.W:
        assert r0["mae_low"] == 0 and not r0["restored"].any()
    if case.logt:
        return
    # the probes say what the issue says of them
    P, f = pb.probes, case.H // case.h
    at = lambda img, name: img[P[name]]
    restored = lambda name: bool(r0["restored"][P[name]])
    assert r0["kept"][P["gate_min_kept"]] and r0["kept"][P["gate_max_kept"]]
    assert not r0["kept"][P["below_gate_min"]] and not r0["kept"][P["above_gate_max"]] and not r0["kept"][P["negative"]]
    for name in ("below_gate_min", "above_gate_max", "negative"):
        assert r0["p_mae"][P[name]] == 0
    assert at(r1["hi_img"], "above_keep_pred") == X.KEEP and at(r1["hi_img"], "keep_edge_pred") == 0 and at(r0["hi_img"], "keep_edge_pred") > X.KEEP
    if not restored("keep_edge_pred"):
        assert at(r1["pred_img"], "keep_edge_pred") == X.KEEP and at(r1["pred_img"], "above_keep_pred") == 0
    if case.lw == case.W:
        n = "gated_out_restored_lo_below_gate"
        assert restored(n) and at(r0["p_mae"], n) == 0 and at(r0["pred_img"], n) == X.Q < pb.gate[0]
        assert at(r1["pred_img"], "lo_keep_edge") == X.KEEP and at(r1["pred_img"], "lo_above_keep") == 0 < at(r0["pred_img"], "lo_above_keep")
        if "lo_above_gate" in P:
            assert at(r0["pred_img"], "lo_above_gate") == 1.5 > pb.gate[1] and at(r1["pred_img"], "lo_above_gate") == 0
        else:
            assert case.h * case.W == 3


POST_DEFECT_CASES = {
    "mae_after_restore": [("4x1x3", 0.0), ("8x2x257-log", 0.0)],
    "gate_exclusive": [("4x1x3", 0.0), ("8x2x256-w128-nothing-restored", X.KEEP)],
    "restored_gated": [("4x1x3", 0.0), ("4x4x5-every-row-restored", X.KEEP), ("8x2x257-log", 0.0)],
    "keep_before_mae": [("4x1x3", X.KEEP), ("132x33x2048-stride", X.KEEP)],
    "lo_row_mod": [("6x2x255", 0.0), ("8x2x257", X.KEEP)],
    "low_div_hw": [("4x1x3", 0.0), ("8x4x64-power-of-two-divisors", 0.0)],
    "restore_when_w_differs": [("8x2x256-w128-nothing-restored", 0.0)],
}


@pytest.mark.parametrize("defect", sorted(POST_DEFECT_CASES))
def test_each_post_defect_is_rejected(defect):
    for name, keep in POST_DEFECT_CASES[defect]:
        pb = post_problem(name)
        bad, _ = post_verdict(pb, keep, defect)
        assert bad, f"{defect} passes on {name} keep_close {keep}"


# ------------------------------------------------------------------ projections and the MC aggregate
def test_projection_emulation_passes():
    for H, W in X.XYZ_SHAPES:
        pb = X.build_xyz(H, W)
        assert X.check_xyz(pb, X.emulate_xyz(pb, X.alloc_xyz(pb))).ok
        assert not X.check_xyz(pb, X.alloc_xyz(pb)).ok
    for H, W in X.DURLAR_SHAPES:
        pb = X.build_durlar(H, W)
        assert X.check_xyz(pb, X.emulate_xyz(pb, X.alloc_xyz(pb))).ok
        assert not X.check_xyz(pb, X.alloc_xyz(pb)).ok
    assert int(X.build_durlar(4, 48).tables[2][0]) == 48               # the row offset equals W


XYZ_DEFECT_CASES = {"product_order": [("xyz", 7, 257), ("xyz", 3, 5)], "fma": [("durlar", 4, 48)], "offset_sign": [("durlar", 4, 48), ("durlar", 5, 64)],
                    "t_in_f64": [("durlar", 4, 48)]}


@pytest.mark.parametrize("defect", sorted(XYZ_DEFECT_CASES))
def test_each_projection_defect_is_rejected(defect):
    for kind, H, W in XYZ_DEFECT_CASES[defect]:
        pb = X.build_durlar(H, W) if kind == "durlar" else X.build_xyz(H, W)
        assert not X.check_xyz(pb, X.emulate_xyz(pb, X.alloc_xyz(pb), defect)).ok, (defect, kind, H, W)


def test_mc_stride_case_and_an_unwritten_tail():
    preds, thr = X.mc_stride_case()
    assert tuple(preds.shape) == (2, 1048576 + 257)
    p = preds.double()
    mean, sd = p.mean(0), p.std(0, unbiased=True)
    got = torch.where(sd > thr * mean, torch.zeros_like(mean), mean).float()
    rep = ND.check_mc(preds, thr, got, "mc stride")
    assert rep.ok and 0.1 < float((got == 0).float().mean()) < 0.9    # both decisions occur
    # check_mc compares with `>`: a NaN left from the prefill passes it, so the GPU test also asserts that every element is finite
    got[1048576:] = float("nan")
    assert not bool(torch.isfinite(got).all())


# ------------------------------------------------------------------ refusals: before any launch, so with dummy pointers
FAKE, E = 4096, -1


def test_refused_arguments():
    lib = _lib.load()
    ch = lambda na=5, nb=7, f64=0: lib.tulip_chamfer_sq(FAKE, na, FAKE, nb, f64, FAKE, FAKE, FAKE, FAKE, None)
    assert ch(na=0) == E and ch(nb=0) == E and ch(na=-3) == E and ch(na=0, f64=1) == E
    vx = lambda n_p=5, n_g=7, grid=0.1, words=4: lib.tulip_voxel_metrics(FAKE, n_p, FAKE, n_g, 0, grid, FAKE, FAKE, words, FAKE, FAKE, None)
    assert vx(grid=0.0) == E and vx(grid=-0.1) == E and vx(grid=float("nan")) == E and vx(n_p=0) == E and vx(n_g=0) == E and vx(words=0) == E
    po = lambda H=8, W=16, h=2, w=16: lib.tulip_eval_postprocess(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, H, W, h, w, 0, 0.0, 1.0, 0.0, None)
    assert po(H=9) == E and po(h=3) == E and po(h=0) == E and po(H=0) == E and po(W=0) == E
    mc = lambda passes=2, n=16: lib.tulip_mc_aggregate(FAKE, passes, n, 0.03, FAKE, None)
    assert mc(passes=1) == E and mc(passes=0) == E and mc(n=0) == E
    assert lib.tulip_range_to_xyz(FAKE, FAKE, FAKE, FAKE, FAKE, 80.0, 0, 4, FAKE, None) == E
    assert lib.tulip_range_to_xyz_durlar(FAKE, FAKE, FAKE, FAKE, 120.0, 0.0, 0.0, 4, 0, FAKE, None) == E

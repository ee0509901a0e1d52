"""The evaluation kernels of csrc/evalpost.hip on adversarial small clouds and images (tests/eval_exact.py), through tulip_amd.ops:
every Chamfer dist element within 6 x 2^-24 of the float64 nearest-neighbour distance of the float32 coordinates (no element
excluded; an exact 0 exactly 0), out[0] against its own dist arrays and the reference; voxel metrics `==` the dense-grid restatement
of the reference on face lattices, degenerate clouds and the capacity boundary, bitmaps and counters handed back clean; the
post-processed images bit for bit and both MAE within one fp32 ulp on pixels that make every difference exact; both projections bit
for bit; the second trip of every capped grid-stride loop.  Every output sits between guard words that must survive, prefilled with
NaN.  Case / route table, the derivation of the Chamfer budget and the measured ratios: DESIGN.md, "Exact evaluation-kernel tests"."""
import numpy as np
import pytest
import torch

from tests import eval_exact as X
from tests import numerics_domain as ND

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from tulip_amd import ops as o
    return o


def holds(buf, n, dtype):
    """the allocation really holds what the header says the launch addresses"""
    assert buf.n >= n and buf.dtype == dtype and buf.flat.numel() == buf.n + 2 * X.NG, (buf.n, n, buf.dtype, dtype)


def run_chamfer(ops, pb, bufs=None):
    c = pb.case
    bufs = bufs or X.alloc_chamfer(pb, DEV)
    t = X.F64 if c.f64 else X.F32
    holds(bufs["a"], 3 * c.na, t), holds(bufs["b"], 3 * c.nb, t), holds(bufs["dist_a"], c.na, X.F32), holds(bufs["dist_b"], c.nb, X.F32)
    holds(bufs["scratch"], 2 * min(X.RB, X.reduction_blocks(c.na, c.nb)), X.F64), holds(bufs["out"], 1, X.F64)
    ops.chamfer_sq(bufs["a"].body, c.na, bufs["b"].body, c.nb, c.f64, bufs["dist_a"].body, bufs["dist_b"].body, bufs["scratch"].body,
                   bufs["out"].body)
    torch.cuda.synchronize()
    return bufs


@pytest.mark.parametrize("case", X.chamfer_cases(), ids=lambda c: c.name)
def test_chamfer_every_element(ops, case):
    assert X.nn_route(case.na, case.nb) == case.route_ab and X.nn_route(case.nb, case.na) == case.route_ba
    pb = X.build_chamfer(case)
    rep = X.check_chamfer(pb, run_chamfer(ops, pb))
    print(f"{rep.line()}; routes {case.route_ab} / {case.route_ba}")
    assert rep.ok, str(rep)


def test_chamfer_second_call_does_not_see_the_first(ops):
    first, second = X.stale_pair()
    bufs = run_chamfer(ops, first)
    rep = X.check_chamfer(first, bufs)
    assert rep.ok, str(rep)
    fresh = X.alloc_chamfer(second, DEV)
    bufs["a"], bufs["b"] = fresh["a"], fresh["b"]                     # the same dist, scratch and out buffers
    rep = X.check_chamfer(second, run_chamfer(ops, second, bufs))
    print(rep.line())
    assert rep.ok, str(rep)


def run_voxel(ops, pb, scratch=None):
    bufs = X.alloc_voxel(pb, DEV, scratch)
    t = X.F64 if pb.pred.dtype == np.float64 else X.F32
    n_p, n_g = pb.pred.shape[0], pb.gt.shape[0]
    holds(bufs["pred"], 3 * n_p, t), holds(bufs["gt"], 3 * n_g, t), holds(bufs["bm_pred"], pb.words, torch.int32)
    holds(bufs["bm_gt"], pb.words, torch.int32), holds(bufs["scratch"], X.COUNTERS_AT + 4, X.F64), holds(bufs["out"], 8, X.F64)
    ops.voxel_metrics(bufs["pred"].body, n_p, bufs["gt"].body, n_g, t == X.F64, X.GRID, bufs["bm_pred"].body, bufs["bm_gt"].body, pb.words,
                      bufs["scratch"].body, bufs["out"].body)
    torch.cuda.synchronize()
    return bufs


def test_voxel_metrics_are_the_references(ops):
    kept, bad = {}, []
    for pb in X.voxel_problems():
        bufs = run_voxel(ops, pb, kept[pb.after]["scratch"] if pb.after else None)
        kept = {pb.name: bufs}
        rep = X.check_voxel(pb, bufs)
        if not rep.ok:
            bad.append(str(rep))
    assert not bad, bad


def run_post(ops, pb, keep):
    c = pb.case
    bufs = X.alloc_post(pb, DEV)
    n = c.H * c.W
    holds(bufs["pred"], n, X.F32), holds(bufs["hi"], n, X.F32), holds(bufs["lo"], c.h * c.lw, X.F32), holds(bufs["pred_img"], n, X.F32)
    holds(bufs["hi_img"], n, X.F32), holds(bufs["partials"], 2 * min(X.RB, -(-n // 256)), X.F64), holds(bufs["mae"], 2, X.F32)
    ops.eval_postprocess(bufs["pred"].body, bufs["hi"].body, bufs["lo"].body, bufs["pred_img"].body, bufs["hi_img"].body,
                         bufs["partials"].body, bufs["mae"].body, c.H, c.W, c.h, c.lw, int(c.logt), pb.gate[0], pb.gate[1], keep)
    torch.cuda.synchronize()
    return bufs


@pytest.mark.parametrize("case", X.post_cases(), ids=lambda c: c.name)
def test_postprocess_order_of_operations(ops, case):
    pb = X.build_post(case)
    mae = {}
    for keep in (0.0, X.KEEP):
        bufs = run_post(ops, pb, keep)
        rep = X.check_post(pb, bufs, keep)
        print(rep.line())
        assert rep.ok, str(rep)
        mae[keep] = bufs["mae"].arr().copy()
    assert np.array_equal(mae[0.0], mae[X.KEEP])                      # keep_close changes neither MAE
    if case.lw != case.W:
        assert mae[0.0][1] == 0


def test_range_to_xyz_bit_exact(ops):
    for H, W in X.XYZ_SHAPES:
        pb = X.build_xyz(H, W)
        b = X.alloc_xyz(pb, DEV)
        holds(b["img"], H * W, X.F32), holds(b["xyz"], 3 * H * W, X.F32), holds(b["sin_h"], W, X.F32), holds(b["cos_h"], W, X.F32)
        holds(b["sin_v"], H, X.F32), holds(b["cos_v"], H, X.F32)
        ops.range_to_xyz(b["img"].body, b["sin_h"].body, b["cos_h"].body, b["sin_v"].body, b["cos_v"].body, pb.max_range, H, W, b["xyz"].body)
        torch.cuda.synchronize()
        rep = X.check_xyz(pb, b)
        assert rep.ok, str(rep)


def test_range_to_xyz_durlar_bit_exact_and_a_permutation(ops):
    from tulip_amd import evaluation as EV
    for H, W in X.DURLAR_SHAPES:
        pb = X.build_durlar(H, W)
        b = X.alloc_xyz(pb, DEV)
        holds(b["img"], H * W, X.F32), holds(b["xyz"], 3 * H * W, X.F64), holds(b["colt"], 4 * W, X.F64), holds(b["rowt"], 2 * H, X.F64)
        holds(b["row_offset"], H, torch.int32)
        assert 0 <= int(pb.tables[2].min()) and int(pb.tables[2].max()) <= W          # (u + W - offset) % W stays inside the row
        ops.range_to_xyz_durlar(b["img"].body, b["colt"].body, b["rowt"].body, b["row_offset"].body, pb.max_range, EV.DURLAR_ORIGIN_OFFSET,
                                EV.DURLAR_Z_OFFSET, H, W, b["xyz"].body)
        torch.cuda.synchronize()
        rep = X.check_xyz(pb, b)                                      # no NaN left of the prefill: every destination written
        assert rep.ok, str(rep)


def test_mc_aggregate_second_trip_of_the_stride_loop(ops):
    preds, thr = X.mc_stride_case()
    out = X.Guarded(X.MC_N, X.F32, DEV)
    ops.mc_aggregate(preds.to(DEV), X.MC_T, X.MC_N, thr, out.body)
    torch.cuda.synchronize()
    got = out.body.cpu()
    assert bool(torch.isfinite(got).all()) and out.guard_violation("out") is None
    rep = ND.check_mc(preds, thr, got, "mc_aggregate, n = 1048576 + 257")
    print(rep.line())
    assert rep.ok, str(rep)

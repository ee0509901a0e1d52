"""CPU: the exact stage-boundary test kit (tests/glue_exact.py) is sharp and its case list complete.

1. Every builder holds its bounds on every case (magnitudes, tie shares, exact LayerNorm rows: asserted inside the builders), a
   torch emulation of the four launches passes every checker on every case and option, and each of twelve plausible kernel
   defects is rejected on every operation it can occur in.
2. Every grid of the lists is accepted by its *_supported query; the tulip_merge_fwd grids reach the (row block, KSPLIT, slices,
   workgroup order) written next to them -- computed from the launcher's documented rule -- and together reach both workgroup
   orders of every instantiation with more than one column slice.
3. Refusals: the launchers check their arguments before any launch, so they are called here with dummy pointers."""
import ctypes
import functools

import pytest
import torch

from tests import gemm_exact as GX
from tests import glue_exact as X
from tulip_amd import _lib, ops

OPS = ("merge_fwd", "merge_bwd", "unmerge_fwd", "unmerge_bwd")


@functools.lru_cache(maxsize=None)
def problem(op, name):
    (c,) = [c for c in X.cases_of(op) if c.name == name]
    return X.BUILDERS[op](c)


def options(op):
    if op == "merge_fwd":
        return [dict(y16=True), dict(y16=False)]
    if op == "merge_bwd":
        return [dict(cast=v, skip=s) for v in X.CAST_VARIANTS for s in (True, False)]
    if op == "unmerge_bwd":
        return [dict(cast=v) for v in X.CAST_VARIANTS]
    return [{}]


def verdict(pb, got, **opt):
    opt.pop("skip", None)
    return X.failures(X.check(pb, got, **opt))


def test_case_lists():
    for op in OPS:
        names = [c.name for c in X.cases_of(op)]
        assert len(set(names)) == len(names)
    assert len(X.MERGE_FWD) == 16 and len(X.MERGE_BWD) == 5 and len(X.UNMERGE) == 10
    assert max(c.B * c.H * c.W * c.Cin * 4 for c in X.MERGE_FWD) <= 26 << 20         # the largest tensor of any case: 25 MiB


@pytest.mark.parametrize("op", OPS)
def test_builders_hold_their_bounds_and_the_emulation_passes(op):
    for c in X.cases_of(op):
        pb = problem(op, c.name)                                   # (magnitude bounds and exact-row conditions: inside the builder)
        for k in ("cat", "dz", "dyb"):
            assert pb.ties.get(k, 1.0) >= X.MIN_TIES, (c.name, pb.ties)
        for out in pb.outs.values():                               # every output sits inside guard words, in front and behind
            b = out.buf
            assert b.off >= b.pitch and b.off + b.rows * b.pitch + b.pitch <= b.flat.numel()
        for opt in options(op):
            bad = verdict(pb, X.emulate(pb, **opt), **opt)
            assert not bad, (c.name, opt, bad)


def test_merge_rows_are_exact_by_construction():
    pb = problem("merge_fwd", "c96-3x2x64")
    rstd = pb.ref["rstd"]
    assert set(rstd.tolist()) == {0.5, 0.25, 0.125}                # three rstd values under ONE eps
    xm = pb.ref["xm"]
    assert bool((xm != 0).all()) and torch.equal(X.rounded(xm), xm)
    # the fp32 emulation (rounded 1/K, torch's rsqrt) is not exact in rstd and still stores the exact xm
    got = X.emulate(pb)
    o = pb.outs["rstd"]
    g = got["rstd"][o.idx.reshape(-1)].to(X.F64)
    assert bool(((g - rstd).abs() <= 2 * X.ND.ulp_f32(rstd)).all())
    # an untouched output is a failure of every word of it
    assert len(verdict(pb, X.fresh(pb))) >= 5


# defect -> (operation, case, options) it is tried on: everywhere it can occur
DEFECT_CASES = {
    "gather_perm": [("merge_fwd", "c96-1x2x64", {}), ("merge_fwd", "c384-1x4x64", dict(y16=False)), ("merge_bwd", "c96-3x2x64", {}),
                    ("merge_bwd", "c192-1x2x64", dict(cast="none", skip=False))],
    "pixshuf_swapped": [("unmerge_fwd", "c192-1x2x8", {}), ("unmerge_fwd", "c384-3x4x4", {})],
    "unshuf_wrong_half": [("unmerge_bwd", "c192-1x1x16", {}), ("unmerge_bwd", "c384-4x2x2", dict(cast="none"))],
    "bias_dropped": [("unmerge_fwd", "c192-16x1x1", {}), ("unmerge_fwd", "c384-1x1x16", {})],
    "no_mid_rounding": [("merge_bwd", "c96-1x2x64", {}), ("unmerge_fwd", "c192-4x2x2", {}), ("unmerge_bwd", "c384-1x2x8", {})],
    "truncate": [("merge_fwd", "c192-1x2x64", {}), ("merge_bwd", "c192-3x2x64", {}), ("unmerge_fwd", "c384-16x1x1", {}),
                 ("unmerge_bwd", "c192-3x4x4", {})],
    "scale_off_by_one": [("merge_bwd", "c96-32x2x2", {}), ("merge_bwd", "c192-3x2x64", dict(skip=False)),
                         ("unmerge_bwd", "c192-16x1x1", {}), ("unmerge_bwd", "c384-3x4x4", {})],
    "block_unwritten": [("merge_fwd", "c96-3x2x64", {}), ("merge_fwd", "c384-3x4x64", dict(y16=False)), ("merge_bwd", "c96-3x2x64", {}),
                        ("unmerge_fwd", "c192-3x4x4", {}), ("unmerge_bwd", "c384-4x2x2", {})],
    "xsave_overwritten": [("unmerge_fwd", "c192-1x1x16", {}), ("unmerge_fwd", "c384-4x2x2", {})],
    "dgamma_dbeta_swapped": [("merge_bwd", "c96-1x2x64", {}), ("merge_bwd", "c192-3x2x64", dict(cast="none", skip=False))],
    "stale_partial": [("merge_bwd", "c96-3x2x64", {}), ("merge_bwd", "c192-1x2x64", {})],
    "row_past_end": [("merge_fwd", "c96-32x2x2", {}), ("merge_fwd", "c192-1x8x64", dict(y16=False)), ("merge_bwd", "c96-1x2x64", {}),
                     ("unmerge_fwd", "c192-1x2x8", {}), ("unmerge_bwd", "c384-16x1x1", {})],
}


def test_the_defect_list_is_the_emulators():
    assert set(DEFECT_CASES) == set(X.DEFECTS) and len(X.DEFECTS) == 12
    tried = {(op, d) for d, lst in DEFECT_CASES.items() for op, _, _ in lst}
    assert tried == {(op, d) for op, ds in X.APPLIES.items() for d in ds}


@pytest.mark.parametrize("defect", X.DEFECTS)
def test_each_defect_is_rejected(defect):
    for op, name, opt in DEFECT_CASES[defect]:
        pb = problem(op, name)
        assert not verdict(pb, X.emulate(pb, **opt), **opt), (op, name)
        bad = verdict(pb, X.emulate(pb, defect, **opt), **opt)
        assert bad, f"{defect} passes every checker on {op} {name} {opt}"
        if defect == "row_past_end":
            assert "guard word" in " ".join(bad), bad                # named as what it is: a word behind the tensor


def test_the_scale_defect_shows_only_where_a_block_spans_samples():
    """with one sample per launch an off-by-one scale index reads the same scale: the case list needs its many-sample grids"""
    pb = problem("merge_bwd", "c96-1x2x64")
    assert pb.ins["scale"].cols == 1
    assert not verdict(pb, X.emulate(pb, "scale_off_by_one"))
    pb = problem("merge_bwd", "c96-32x2x2")
    assert pb.ins["scale"].cols == 32 and pb.case.crps == 4
    s = pb.ref["scale"]
    assert bool((s[1:] != s[:-1]).all())
    assert verdict(pb, X.emulate(pb, "scale_off_by_one"))
    assert verdict(pb, X.emulate(pb, "scale_off_by_one", cast="scaled", skip=False), cast="scaled")
    # without a scale the index is never used
    assert not verdict(pb, X.emulate(pb, "scale_off_by_one", cast="unscaled"), cast="unscaled")


def test_a_nan_that_leaks_in_from_padding_is_seen():
    for op, name, operand in (("merge_fwd", "c96-1x2x64", "x"), ("merge_bwd", "c96-1x2x64", "dys"), ("unmerge_fwd", "c192-1x1x16", "x"),
                              ("unmerge_bwd", "c192-1x1x16", "dys")):
        pb = problem(op, name)
        b = pb.ins[operand]
        assert torch.isnan(b.flat.float()).sum() == b.flat.numel() - b.rows * b.cols
        b.off += 8                                                  # the operand pointer eight elements late
        try:
            assert verdict(pb, X.emulate(pb)), (op, operand)
        finally:
            b.off -= 8


def test_a_written_guard_column_and_a_touched_option_are_seen():
    pb = problem("merge_fwd", "c192-1x2x64")
    o = pb.outs["y16"].buf
    assert o.pitch > o.cols and o.pitch != 2 * o.cols and o.pitch % 4 == 0
    got = X.emulate(pb)
    got["y16"][o.off + 5 * o.pitch + o.cols] = 1.0                  # the first guard column of row 5
    assert "guard word" in " ".join(verdict(pb, got))
    got = X.emulate(pb, y16=True)                                   # y_bf16 written although the launch was told it is absent
    assert verdict(pb, got, y16=False)
    pb = problem("unmerge_bwd", "c192-4x2x2")
    assert verdict(pb, X.emulate(pb, cast="scaled"), cast="none") and verdict(pb, X.emulate(pb, cast="unscaled"), cast="scaled")


# ------------------------------------------------------------------ accepted grids and routes (host code only)
def test_every_grid_is_supported_and_partial_rows():
    lib = _lib.load()
    for c in X.MERGE_FWD:
        assert lib.tulip_merge_fwd_supported(c.Cin, c.B, c.H, c.W) == 1, c
        assert c.rows % 32 == 0
    for c in X.MERGE_BWD:
        assert lib.tulip_merge_bwd_supported(c.Cp, c.B, c.H, c.W) == 1, c
        assert lib.tulip_merge_bwd_partial_rows(c.Cp, c.B, c.H, c.W) == c.rows // (32 if c.Cp == 96 else 16) == c.rows // c.bm
    for c in X.MERGE_FWD:                                           # the same grids one level up, where Cp exists
        if c.Cin in (96, 192):
            assert lib.tulip_merge_bwd_partial_rows(c.Cin, c.B, c.H, c.W) == c.rows // (32 if c.Cin == 96 else 16)
    for c in X.UNMERGE:
        assert lib.tulip_unmerge_skip_supported(c.C, c.B, c.H, c.W) == 1 and c.M % 16 == 0, c
    assert {(c.B, c.H, c.W) for c in X.UNMERGE} == {(1, 1, 16), (1, 2, 8), (16, 1, 1), (4, 2, 2), (3, 4, 4)}
    assert {(c.rows, c.crps) for c in X.MERGE_BWD if c.Cp == 96} == {(32, 128), (96, 128), (32, 4)}
    assert {c.rows for c in X.MERGE_BWD if c.Cp == 192} == {32, 96}


def test_merge_fwd_grids_reach_the_routes_written_next_to_them():
    for c in X.MERGE_FWD:
        assert X.merge_fwd_route(c.Cin, c.rows) == c.route, (c.name, X.merge_fwd_route(c.Cin, c.rows))
    # the rule's thresholds, and the row-block counts the issue names
    by = {c.name: c for c in X.MERGE_FWD}
    assert by["c192-2x64x128"].rows == 4096 and by["c192-2x128x128"].rows == 8192 and by["c192-257x2x64"].rows == 8224
    assert by["c384-8x8x256"].rows == 4096 and by["c384-129x2x64"].rows == 4128
    assert by["c384-1x4x64"].rows // 16 == 4 and by["c384-3x4x64"].rows // 16 == 12         # KITTI deepest level, batch 1 / 3
    blocks = lambda c: c.rows // c.route[0]
    assert blocks(by["c192-257x2x64"]) == 257 and blocks(by["c384-129x2x64"]) == 258 and blocks(by["c96-1x2x64"]) == 1
    # both workgroup orders of every instantiation with more than one column slice
    inst = {}
    for c in X.MERGE_FWD:
        bm, ks, nsl, order = c.route
        inst.setdefault((c.Cin, bm, ks, nsl), set()).add(order)
    assert set(inst) == {(96, 32, 1, 1), (192, 32, 1, 2), (192, 16, 2, 4), (384, 16, 1, 4), (384, 16, 4, 16)}
    for key, orders in inst.items():
        assert orders == ({"single"} if key[3] == 1 else {"xcd", "slice-minor"}), (key, orders)


# ------------------------------------------------------------------ refusals: before any launch, so with dummy pointers
FAKE = 4096
E = -1


def _desc(cls, ints, **kw):
    d = cls()
    for name, _t in cls._fields_:
        setattr(d, name, kw[name] if name in kw else (0 if name in ints else FAKE))
    return d


def merge_fwd_rc(**kw):
    base = dict(ld_bf16=192, B=1, H=2, W=64, Cin=96, eps=3.0)
    d = _desc(_lib.MergeFwdDesc, ("ld_bf16", "B", "H", "W", "Cin", "eps"), **{**base, **kw})
    return _lib.load().tulip_merge_fwd(ctypes.byref(d), None)


def merge_bwd_rc(**kw):
    base = dict(cast_rows_per_sample=128, B=1, H=2, W=64, Cp=96)
    d = _desc(_lib.MergeBwdDesc, ("cast_rows_per_sample", "B", "H", "W", "Cp"), **{**base, **kw})
    return _lib.load().tulip_merge_bwd(ctypes.byref(d), None)


def unmerge_rc(**kw):
    d = _desc(_lib.UnmergeSkipDesc, ("B", "H", "W", "C"), **{**dict(B=1, H=1, W=16, C=192), **kw})
    return _lib.load().tulip_unmerge_skip_fwd(ctypes.byref(d), None)


def unmerge_bwd_rc(**kw):
    base = dict(cast_rows_per_sample=16, B=1, H=1, W=16, C=192)
    d = _desc(_lib.SkipUnmergeBwdDesc, ("cast_rows_per_sample", "B", "H", "W", "C"), **{**base, **kw})
    return _lib.load().tulip_skip_unmerge_bwd(ctypes.byref(d), None)


def test_refused_grids_and_widths():
    lib = _lib.load()
    fwd, bwd, un = lib.tulip_merge_fwd_supported, lib.tulip_merge_bwd_supported, lib.tulip_unmerge_skip_supported
    assert fwd(96, 1, 2, 64) == 1 and bwd(96, 1, 2, 64) == 1 and un(192, 1, 1, 16) == 1
    for q, rc, cin in ((fwd, merge_fwd_rc, "Cin"), (bwd, merge_bwd_rc, "Cp")):
        # odd H, odd W (with an even row count that would pass), rows % 32, B = 0, negative sizes
        for B, H, W in ((1, 3, 64), (2, 2, 63), (32, 3, 4), (32, 4, 3), (1, 2, 32), (1, 2, 96), (3, 2, 32), (0, 2, 64), (-1, 2, 64), (1, 0, 64)):
            assert q(96, B, H, W) == 0, (B, H, W)
            assert rc(B=B, H=H, W=W) == E, (B, H, W)
            assert lib.tulip_merge_bwd_partial_rows(96, B, H, W) == 0
        for width in ((48, 768, 0, 100) if cin == "Cin" else (384, 48, 0, 100)):
            assert q(width, 1, 2, 64) == 0 and rc(**{cin: width}) == E, width
    assert lib.tulip_merge_bwd_partial_rows(384, 1, 2, 64) == 0
    for B, H, W in ((1, 1, 8), (1, 3, 5), (3, 1, 8), (0, 1, 16), (1, 0, 16), (1, 16, 0), (-16, 1, 1)):      # M % 16, empty
        assert un(192, B, H, W) == 0 and unmerge_rc(B=B, H=H, W=W) == E and unmerge_bwd_rc(B=B, H=H, W=W) == E, (B, H, W)
    for C in (96, 768, 0, 200):
        assert un(C, 1, 1, 16) == 0 and unmerge_rc(C=C) == E and unmerge_bwd_rc(C=C) == E, C
    for f in (lib.tulip_merge_fwd, lib.tulip_merge_bwd, lib.tulip_unmerge_skip_fwd, lib.tulip_skip_unmerge_bwd):
        assert f(None, None) == E


def test_refused_pointers_and_options():
    for name in ("x", "gamma", "beta", "w_packed", "xm", "mean", "rstd", "y"):
        assert merge_fwd_rc(**{name: None}) == E, name
    for ld in (190, 191, 193, 2):
        assert merge_fwd_rc(ld_bf16=ld) == E, ld
    for name in ("dyb", "w_red_t_packed", "x_prev", "mean", "rstd", "gamma", "dx_prev", "param_partials"):
        assert merge_bwd_rc(**{name: None}) == E, name
    assert merge_bwd_rc(dx_in=None) == E and merge_bwd_rc(w_skip_t_packed=None) == E         # dy_skip without its companions
    for crps in (0, -4):
        assert merge_bwd_rc(cast_rows_per_sample=crps) == E and unmerge_bwd_rc(cast_rows_per_sample=crps) == E
    for name in ("x_bf16", "w_expand_packed", "b_expand", "cat", "w_skip_packed", "b_skip", "out"):
        assert unmerge_rc(**{name: None}) == E, name
    for name in ("dy_skip", "w_skip_t_packed", "dz", "w_expand_t_packed", "dx"):
        assert unmerge_bwd_rc(**{name: None}) == E, name

"""CPU: the exact LayerNorm / patch-embedding test kit (tests/norm_exact.py) is sharp and its case lists route-complete.

1. Every builder holds its bounds on every case of the GPU lists (the 2^20 exactness bound, at most 64 non-zero dout tokens, the
   half-ulp margin of the exact rows, an order-sensitive slab family: asserted inside the builders), and a float32 torch emulation
   of the seven entry points passes every checker on every case and option.
2. Each of the emulation's defects is rejected by the cases named next to it.
3. The route functions agree with the literals written next to the cases and with the library's host-side answers, and the lists
   reach every route: a literal here, so dropping a case family fails.
4. Refusals: the launchers check their arguments before any launch, so they are called here with dummy pointers."""
import functools

import pytest
import torch

from tests import norm_exact as X
from tulip_amd import _lib


@functools.lru_cache(maxsize=None)
def problem(op, name):
    return X.OPS[op][1](X.case_of(op, name))


def options(op, c):
    if op == "embed_fwd":
        return [dict(variant=v) for v in X.BF16_VARIANTS]
    if op == "ln_bwd":
        return X.bwd_options(c)
    return [{}]


def verdict(op, pb, defect, opt):
    assert pb.op == op
    return X.failures(X.check(pb, X.emulate(pb, defect, **opt), **opt))


def test_case_lists():
    for op, (cases, *_) in X.OPS.items():
        names = [c.name for c in cases]
        assert len(set(names)) == len(names), op
    for c in X.EMBED_FWD:
        assert X.embed_fwd_route(c.Cin, c.p0, c.kw, c.taps) == c.route and not c.form, c.name
    for c in X.EMBED_BWD:
        assert X.embed_bwd_route(c.E, c.taps, c.form == "partial") == c.route and c.form in ("partial", "atomic"), c.name
    for c in X.LN_CASES:
        assert X.ln_route(c.C) == c.route, c.name
        if c.merge:
            assert c.rows == c.merge[0] * (c.merge[1] // 2) * (c.merge[2] // 2) and c.crps & (c.crps - 1)
    for c in X.PARAMS:
        assert X.ln_params_grid(c.rows, c.C) == c.grid, (c.name, X.ln_params_grid(c.rows, c.C))
    for c in X.SPLITK:
        assert X.splitk_ln_nch(c.N) == c.nch, c.name
    # both branches of fast_div for every divisor: power-of-two and other token-grid widths, heights, merged widths, heights
    pow2 = lambda v: v & (v - 1) == 0
    for vals in ([c.Wo for c in X.EMBED_FWD], [c.Ho for c in X.EMBED_FWD], [c.Wo for c in X.EMBED_BWD], [c.Ho for c in X.EMBED_BWD],
                 [c.merge[2] // 2 for c in X.LN_CASES if c.merge], [c.merge[1] // 2 for c in X.LN_CASES if c.merge],
                 [c.C // 4 for c in X.LN_CASES if c.merge], [c.crps for c in X.LN_CASES], [c.rps for c in X.SPLITK]):
        assert {pow2(v) for v in vals} == {True, False}, vals
    assert max(c.B * c.Cin * c.Hin * c.Win * 4 for c in X.EMBED_FWD + X.EMBED_BWD) <= 264 << 10      # the largest image: 256 KiB


def test_the_lists_reach_every_route():
    row = {("row", kw, cin) for kw in (4, 8) for cin in (1, 2, 3, 4)}
    assert {c.route for c in X.EMBED_FWD} == row | {("generic", True), ("generic", False)}
    lane = {("lane16", cpl, t) for cpl in (3, 6) for t in (8, 16, 24, 32)}
    assert {c.route for c in X.EMBED_BWD} == lane | {("generic", True, "partial"), ("generic", True, "atomic"), ("generic", False, "atomic")}
    # every TAPS class of the 16-lane form with taps == TAPS and with taps < TAPS, at both widths
    assert {(c.route[1], c.route[2], c.taps == c.route[2]) for c in X.EMBED_BWD if c.route[0] == "lane16"} == \
        {(cpl, t, full) for cpl in (3, 6) for t in (8, 16, 24, 32) for full in (True, False)}
    # dispatch_ln: the three special widths, then six (LPR, NCH) steps, each with and without a ragged last chunk
    assert {c.route for c in X.LN_CASES} == {(64, 3, True), (64, 6, True), (64, 12, True)} | {
        (lpr, n, e) for lpr, n in ((16, 2), (16, 4), (64, 2), (64, 4), (64, 8), (64, 24)) for e in (True, False)}
    assert {X.ln_partial_rows(c.rows, c.C) > 0 for c in X.LN_CASES} == {True, False}
    assert {c.nch for c in X.SPLITK} == {1, 2, 3, 4, 6, 8} and {c.nslab for c in X.SPLITK} == set(X.NSLABS)
    assert {c.nslab for c in X.LN_CASES} == set(X.NSLABS)
    assert {(c.grid[0], c.grid[2] > 1) for c in X.PARAMS} == {(t, g) for t in (4, 5, 6) for g in (True, False)}
    assert {c.grid[1] > 1 for c in X.PARAMS} == {True, False}
    assert any(c.rows % c.grid[3] for c in X.PARAMS if c.grid[2] > 1)                                 # a ragged last row block
    for flag in ("bias", "aux", "rowscale", "out16"):
        assert {getattr(c, flag) for c in X.SPLITK} == {True, False}


def test_backward_options_cover_every_pair():
    full = [c for c in X.LN_CASES if c.opts == "full"]
    assert {c.route[0] for c in full} == {16, 64} and all(len(X.bwd_options(c)) == 36 for c in full)
    keys = list(X.BWD_LEVELS)
    for c in X.LN_CASES:
        if c.opts != "cover":
            continue
        opts = X.bwd_options(c)
        lv = dict(X.BWD_LEVELS, parts=(False, True) if X.ln_partial_rows(c.rows, c.C) else (False,))
        for i, a in enumerate(keys):
            for b in keys[i + 1:]:
                assert {(o[a], o[b]) for o in opts} == {(u, v) for u in lv[a] for v in lv[b]}, (c.name, a, b)
        assert len(opts) <= 12


@pytest.mark.parametrize("op", list(X.OPS))
def test_builders_hold_their_bounds_and_the_emulation_passes(op):
    for c in X.OPS[op][0]:
        pb = problem(op, c.name)
        for b in pb.outs.values():                                      # every output sits inside guard words, in front and behind
            assert b.off >= b.pitch and b.off + b.rows * b.pitch + b.pitch <= b.flat.numel()
        if op == "embed_bwd":
            assert pb.ref["n_nz"] <= X.MAX_NZ
        for opt in options(op, c):
            bad = verdict(op, pb, None, opt)
            assert not bad, (c.name, opt, bad)


def test_budget_conditions_hold_for_the_reference_alone():
    gen = torch.Generator().manual_seed(3)
    for ns in (3, 4, 5, 9):                                             # left to right 0, right to left nslab - 2
        s = X.make_slabs((2, 10), ns, gen, 50)
        assert torch.equal(X.fold32(s)[:, 0::5], torch.zeros(2, 2, dtype=X.F64))
        assert torch.equal(X.fold32(s, range(ns - 1, -1, -1))[:, 0::5], torch.full((2, 2), ns - 2.0, dtype=X.F64))
    v, rstd = X.exact_rows(64, 96, gen)
    assert set(rstd.tolist()) == {0.5, 0.25, 0.125}
    off = X.row_offsets(64, gen)
    assert bool((off[0::2] == 0).all()) and bool((off[1::2] != 0).all())
    gamma, beta = X.odd_ints(gen, 96), torch.zeros(96, dtype=X.F64)
    X.assert_half_ulp_margin(v, rstd, off, gamma, beta)
    with pytest.raises(AssertionError):                                 # a gamma of 1/3: y is no bf16 value
        X.assert_half_ulp_margin(v, rstd, off, gamma / 3, beta)
    with pytest.raises(AssertionError):                                 # an offset of 2^20: the error of the mean reaches the rounding
        X.assert_half_ulp_margin(v, rstd, off * 2.0 ** 20, gamma, beta)
    # the token choice of the large backward cases: first, last, both sides of every pass boundary
    c = X.case_of("embed_bwd", "e96-3x1x1x10924-p1x4k8c-partial")
    nz = set(X.embed_nz_tokens(c, gen).tolist())
    assert len(nz) == X.MAX_NZ and {0, 2047, 2048, 8191, 8192} <= nz and c.ntok == 8193
    # an untouched output is a failure of every checker
    for op, name in (("embed_fwd", "e96-2x1x3x20-p1x4k8c"), ("ln_fwd", "c96-r17"), ("params", "c48-r1"), ("splitk", "n256-m5-s3-bars")):
        pb = problem(op, name)
        assert X.failures(X.OPS[op][3](pb, X.fresh(pb))), (op, name)


# defect -> (entry point, case) that must reject it; every entry point the defect can occur in is named
DEFECT_CASES = {
    "wrap_left_clamped": [("embed_fwd", "e96-2x1x3x20-p1x4k8c"), ("embed_fwd", "e96-2x1x3x4-p1x4k8c"), ("embed_bwd", "e48-2x1x3x20-p1x4k8c-partial"),
                          ("embed_bwd", "e96-2x1x3x20-p1x4k8c-atomic")],
    "wrap_right_clamped": [("embed_fwd", "e96-2x1x3x20-p1x4k8c"), ("embed_fwd", "e96-2x1x3x4-p1x4k8c"), ("embed_bwd", "e48-2x1x3x20-p1x4k8c-partial"),
                           ("embed_bwd", "e96-2x1x3x20-p1x4k8c-atomic")],
    "pad_is_1": [("embed_fwd", "e96-2x1x3x20-p1x4k8c"), ("embed_fwd", "e96-2x2x3x24-p1x8k8c"), ("embed_bwd", "e96-2x4x3x20-p1x4k8c-partial")],
    "tap_order_channel_minor": [("embed_fwd", "e96-2x3x4x10-p2x2k2"), ("embed_fwd", "e96-2x2x4x24-p2x8k8"), ("embed_bwd", "e65-2x3x4x10-p2x2k2-atomic"),
                                ("embed_bwd", "e96-2x3x4x24-p2x8k8c-atomic")],
    "batch_stride_ignores_cin": [("embed_fwd", "e96-2x2x3x20-p1x4k4"), ("embed_fwd", "e128-2x5x3x20-p1x4k4"), ("embed_bwd", "e48-2x3x3x20-p1x4k4-partial")],
    "patch_row_ignored": [("embed_fwd", "e96-2x1x8x20-p4x4k4"), ("embed_fwd", "e96-3x1x2x10924-p2x4k4"), ("embed_bwd", "e64-2x1x4x20-p2x4k8c-partial"),
                          ("embed_bwd", "e64-2x1x8x20-p4x4k8c-atomic")],
    "tail_group_dropped": [("embed_fwd", "e96-2x1x3x20-p1x4k4"), ("embed_fwd", "e96-1x1x1x4-p1x4k4"), ("embed_fwd", "e96-3x1x1x10924-p1x4k8c")],
    "clamped_token_stored": [("embed_fwd", "e96-1x1x3x4-p1x4k4"), ("embed_fwd", "e96-1x1x1x68-p1x4k8c")],
    "second_pass_dropped": [("embed_fwd", "e96-3x1x1x10924-p1x4k8c"), ("embed_fwd", "e96-3x1x2x10924-p2x4k4"), ("embed_bwd", "e64-3x1x1x2732-p1x4k8c-partial"),
                            ("embed_bwd", "e96-3x1x1x2732-p1x4k4-atomic"), ("embed_bwd", "e96-3x1x1x10924-p1x4k8c-partial"), ("ln_fwd", "c8-r65537"),
                            ("ln_fwd", "c260-r16385"), ("ln_bwd", "c8-r65537"), ("ln_bwd", "c260-r16385"), ("ln_bwd", "c48-r8193"), ("ln_bwd", "c384-r2049")],
    "upper_half_dropped": [("embed_fwd", "e65-2x1x3x20-p1x4k8c"), ("embed_fwd", "e128-2x1x3x20-p1x4k8c"), ("embed_fwd", "e96-2x1x4x24-p2x8k8")],
    "bf16_truncated": [("embed_fwd", "e96-2x1x3x20-p1x4k4"), ("embed_fwd", "e128-2x5x3x20-p1x4k4")],
    "ld16_is_E": [("embed_fwd", "e96-2x1x3x20-p1x4k4"), ("embed_fwd", "e65-2x1x4x20-p2x4k4")],
    "onepass_variance": [("embed_fwd", "e96-2x1x3x20-p1x4k8c-b1024"), ("embed_fwd", "e96-2x1x4x20-p2x4k4-b1024"),
                         ("embed_bwd", "e96-2x1x3x20-p1x4k8c-b1024-partial"), ("embed_bwd", "e65-2x1x3x20-p1x4k8c-b1024-atomic")],
    "eps_dropped": [("embed_fwd", "e1-2x1x3x20-p1x4k8c"), ("embed_fwd", "e96-2x1x3x20-p1x4k8c"), ("embed_bwd", "e48-2x1x3x20-p1x4k4-partial"),
                    ("embed_bwd", "e128-2x1x3x20-p1x4k4-atomic")],
    "partial_padding_written": [("embed_bwd", "e48-2x1x3x20-p1x4k4-partial"), ("embed_bwd", "e64-2x1x3x20-p1x4k8c-partial")],
    "empty_block_row_unwritten": [("embed_bwd", "e48-2x1x3x20-p1x4k4-partial"), ("embed_bwd", "e96-2x4x3x20-p1x4k8c-partial")],
    "atomic_form_overwrites": [("embed_bwd", "e96-2x1x3x20-p1x4k8c-atomic"), ("embed_bwd", "e96-2x3x4x24-p2x8k8c-atomic")],
    "dgamma_dbeta_swapped": [("embed_bwd", "e48-2x1x3x20-p1x4k4-partial"), ("embed_bwd", "e128-2x1x3x20-p1x4k4-atomic")],
    "db_is_dbeta": [("embed_bwd", "e64-2x1x3x20-p1x4k8c-partial"), ("embed_bwd", "e96-2x1x3x20-p1x4k8c-atomic")],
    "taps_mask_missing": [("embed_bwd", "e48-2x1x3x20-p1x4k4-partial"), ("embed_bwd", "e96-2x5x3x20-p1x4k4-partial"), ("embed_bwd", "e96-2x7x3x20-p1x4k4-partial")],
    "rows_tail_dropped": [("ln_fwd", "c96-r17"), ("ln_fwd", "c384-r5"), ("ln_fwd", "c4-r1"), ("ln_bwd", "c96-r17"), ("ln_bwd", "c768-r3"),
                          ("splitk", "n256-m5-s3-bars"), ("splitk", "n256-m1-s1-plain")],
    "last_chunk_dropped": [("ln_fwd", "c132-r17"), ("ln_fwd", "c2052-r5"), ("ln_bwd", "c260-r5"), ("ln_bwd", "c1028-r5")],
    "merge_quadrants_swapped": [("ln_fwd", "c192-m3x2x2"), ("ln_fwd", "c256-m3x2x6"), ("ln_fwd", "c192-m3x6x2"), ("ln_bwd", "c192-m3x2x2"),
                                ("ln_bwd", "c256-m3x2x6"), ("params", "c192-m3x2x6")],
    "cast_scale_per_row": [("ln_bwd", "c192-m3x2x2"), ("ln_bwd", "c256-m3x2x6")],
    "cast_channels_not_quartered": [("ln_bwd", "c192-m3x6x2"), ("ln_bwd", "c256-m3x2x6")],
    "slab_order_reversed": [("ln_bwd", "c128-r17"), ("ln_bwd", "c1024-r5"), ("splitk", "n256-m5-s3-bars"), ("splitk", "n2048-m8-s9-bars")],
    "slab_fold_not_rounded": [("ln_bwd", "c128-r17"), ("ln_bwd", "c1536-r5")],
    "dres_ignored": [("ln_bwd", "c96-r17"), ("ln_bwd", "c384-r5")],
    "params_overwrite": [("params", "c4-r1"), ("params", "c384-r2048")],
    "params_row_block_tail_dropped": [("params", "c4-r2049"), ("params", "c384-r4100")],
    "partial_rows_past_count_written": [("ln_bwd", "c96-r17"), ("ln_bwd", "c2048-r5")],
    "resid_scale_per_row": [("splitk", "n256-m5-s3-bars"), ("splitk", "n512-m5-s9-ar")],
    "resid_bias_after_scale": [("splitk", "n256-m5-s3-bars"), ("splitk", "n1024-m1-s9-bar")],
}


def test_the_defect_list_is_the_emulators():
    assert set(DEFECT_CASES) == set(X.EMBED_DEFECTS) | set(X.LN_DEFECTS)
    assert len(X.EMBED_DEFECTS) == 20 and len(X.LN_DEFECTS) == 14
    tried = {(op, d) for d, lst in DEFECT_CASES.items() for op, _ in lst}
    assert tried == {(op, d) for op, ds in X.APPLIES.items() for d in ds}


@pytest.mark.parametrize("defect", sorted(DEFECT_CASES))
def test_each_defect_is_rejected(defect):
    for op, name in DEFECT_CASES[defect]:
        pb = problem(op, name)
        caught = []
        for opt in options(op, pb.case):
            assert not verdict(op, pb, None, opt), (op, name, opt)
            if verdict(op, pb, defect, opt):
                caught.append(opt)
        assert caught, f"{defect} passes every checker on {op} {name}"


def test_stray_stores_are_named_as_guard_words():
    pb = problem("embed_fwd", "e96-1x1x3x4-p1x4k4")
    bad = verdict("embed_fwd", pb, "clamped_token_stored", dict(variant="absent"))
    assert "guard word" in " ".join(bad), bad
    pb = problem("embed_bwd", "e64-2x1x3x20-p1x4k8c-partial")
    bad = verdict("embed_bwd", pb, "partial_padding_written", {})
    assert "guard word" in " ".join(bad), bad


def test_route_functions_agree_with_the_library():
    lib = _lib.load()
    for C in list(range(0, 2600, 4)) + [3072, 6144]:
        for rows in (0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193, 100000):
            assert lib.tulip_layernorm_bwd_partial_rows(rows, C) == X.ln_partial_rows(rows, C), (rows, C)
    for ntok in list(range(0, 40)) + [2044, 2045, 2047, 2048, 2049, 2052, 2053, 8193, 1 << 20]:
        assert lib.tulip_patch_embed_bwd_blocks(ntok) == X.embed_bwd_blocks(ntok), ntok
    for N in list(range(-256, 2600, 64)) + [255, 257, 4096]:
        assert bool(lib.tulip_splitk_resid_ln_supported(N)) == (X.splitk_ln_nch(N) is not None), N
    assert X.ln_route(6148) is None and X.ln_route(6144) == (64, 24, True)


def test_refused_arguments_return_before_any_launch():
    lib = _lib.load()
    f = 4096                                                            # a dummy address: nothing may be launched
    pe_f = lambda B, Cin, Hin, Win, E, p0, p1, kw, circ: lib.tulip_patch_embed_fwd(f, f, f, f, f, f, B, Cin, Hin, Win, E, p0, p1, kw, circ, 3.0, None, 0, None)
    pe_b = lambda B, Cin, Hin, Win, E, p0, p1, kw, circ, ps: lib.tulip_patch_embed_bwd(f, f, f, f, f, f, f, f, f, B, Cin, Hin, Win, E, p0, p1, kw, circ, 3.0, ps, None)
    bad_geom = [(2, 1, 3, 20, 0, 1, 4, 8, 1), (2, 1, 3, 20, 129, 1, 4, 8, 1), (2, 1, 3, 20, 96, 2, 4, 8, 1), (2, 1, 4, 18, 96, 2, 4, 4, 0),
                (2, 1, 3, 20, 96, 1, 4, 4, 1), (2, 1, 3, 32, 96, 1, 16, 8, 1), (2, 1, 3, 20, 96, 1, 2, 8, 1), (2, 1, 3, 20, 96, 1, 4, 8, 0),
                (2, 1, 3, 24, 96, 1, 8, 4, 0)]
    for g in bad_geom:
        assert pe_f(*g) == -1 and pe_b(*g, 0) == -1 and pe_b(*g, 4096) == -1, g
    # the partial backward: more than 16 taps outside E = 48 / 96, or more than 32 taps
    for g in [(2, 1, 8, 20, 64, 4, 4, 8, 1), (2, 5, 3, 20, 128, 1, 4, 4, 0), (2, 3, 4, 24, 96, 2, 8, 8, 1), (2, 5, 3, 24, 48, 1, 8, 8, 1)]:
        assert pe_b(*g, 4096) == -1, g
        assert X.embed_bwd_route(g[4], g[1] * g[5] * g[7], True) == "refused"
    assert pe_f(0, 1, 3, 20, 96, 1, 4, 8, 1) == 0 and pe_b(0, 1, 3, 20, 96, 1, 4, 8, 1, 4096) == 0 and pe_b(0, 1, 3, 20, 96, 1, 4, 8, 1, 0) == 0

    ln_f = lambda rows, C, m=0, B=0, H=0, W=0: lib.tulip_layernorm_fwd(f, f, f, f, f, f, rows, C, 3.0, m, B, H, W, None)
    ln_b = lambda rows, C, m=0, B=0, H=0, W=0, part=None: lib.tulip_layernorm_bwd(f, f, f, f, f, None, f, rows, C, m, B, H, W, part, None, None, 1, None)
    ln_s = lambda ns, rows, C, m=0, B=0, H=0, W=0, part=None: lib.tulip_layernorm_bwd_splitk(f, ns, f, f, f, f, None, f, rows, C, m, B, H, W, part, None, None, 1, None)
    ln_p = lambda rows, C, m=0, B=0, H=0, W=0: lib.tulip_layernorm_bwd_params(f, f, f, f, f, f, rows, C, m, B, H, W, None)
    for a in [(5, 6), (5, 0), (5, 6148), (3, 192, 1, 3, 3, 2), (3, 192, 1, 3, 2, 3), (3, 200, 1, 3, 2, 2), (4, 192, 1, 3, 2, 2)]:
        assert ln_f(*a) == -1 and ln_b(*a) == -1 and ln_s(3, *a) == -1, a
        if a[1] != 6148:
            assert ln_p(*a) == -1, a
    assert ln_b(5, 2052, part=f) == -1 and ln_s(3, 5, 2052, part=f) == -1
    assert ln_s(0, 5, 96) == -1
    assert ln_f(0, 96) == 0 and ln_b(0, 96) == 0 and ln_s(3, 0, 96) == 0 and ln_p(0, 96) == 0

    sk = lambda M, N, ldo=None, ldaux=None, ldo2=None, aux=None, o2=None: lib.tulip_splitk_resid_ln(
        f, 3, M, N, None, aux, ldaux or N, None, 1, f, ldo or N, o2, ldo2 or N, f, f, f, f, f, 3.0, None)
    for N in (128, 1280, 1792, 0, 300):
        assert sk(5, N) == -1 and not lib.tulip_splitk_resid_ln_supported(N), N
    assert sk(5, 256, ldo=258) == -1 and sk(5, 256, ldaux=258, aux=f) == -1 and sk(5, 256, ldo2=258, o2=f) == -1
    assert lib.tulip_splitk_resid_ln(f, 0, 5, 256, None, None, 0, None, 1, f, 256, None, 0, f, f, f, f, f, 3.0, None) == -1
    assert sk(0, 256) == 0


def test_fold_against_atomic_is_checked_per_output():
    """both forms of the backward on the same operands: the emulations agree within the factor written in FACTORS, a partial form
    that drops its second pass does not, and d(beta) has no tolerance at all"""
    from dataclasses import replace
    assert X.FACTORS["fold_vs_atomic"] == 2.0
    for name in ("e64-3x1x1x2732-p1x4k8c-partial", "e48-1x1x1x4-p1x4k4-partial", "e96-2x1x3x20-p1x4k8c-partial"):
        pb = problem("embed_bwd", name)
        c = pb.case
        pa = X.build_embed(replace(c, form="atomic", route=X.embed_bwd_route(c.E, c.taps, False)))
        atomic = X.embed_fold(pa, X.emulate(pa))
        reps = X.check_fold_vs_atomic(pb, X.embed_fold(pb, X.emulate(pb)), atomic)
        assert [r.what.rsplit(" ", 1)[-1] for r in reps] == ["dw", "db", "dgamma", "dbeta"] and not X.failures(reps), (name, X.failures(reps))
        if c.ntok > 2048:
            assert X.failures(X.check_fold_vs_atomic(pb, X.embed_fold(pb, X.emulate(pb, "second_pass_dropped")), atomic)), name
        off = atomic.clone()
        off[-1] += 1
        assert X.failures(X.check_fold_vs_atomic(pb, off, atomic)[3:]), name

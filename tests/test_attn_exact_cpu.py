"""tests/attn_exact.py on the CPU: the case list covers every kernel instantiation's sweeps, the launch-rule functions give what the
cases write next to their shapes, the float64 reference agrees with numerics_domain.attn_reference, the clean torch emulation
passes every case, and every defect of the emulation fails the case named beside it -- the checkers the GPU test applies to the
kernels are sharp."""
import functools

import pytest
import torch

from tests import attn_exact as X
from tests import numerics_domain as ND

CASES = X.gpu_cases()
BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=4)
def problem(name):
    return X.build(BY_NAME[name], "cpu")


def test_case_list_is_complete():
    assert X.coverage_gaps(CASES) == []
    assert len(CASES) == 39                                   # the count the module docstring names
    assert max(c.M for c in CASES) < 6000
    for c in CASES:
        assert c.fwd == X.fwd_route(c.total, c.L, c.nh), c.name
        assert c.bwd is None or c.bwd == X.bwd_route(c.total, c.L, c.nh), c.name
        assert c.total % 2 == 1 and (c.variant != "fp8" or c.L == 16)
    # a case list without its short sweeps is found incomplete
    assert X.coverage_gaps([c for c in CASES if "sweeps" not in c.name])
    assert X.coverage_gaps([c for c in CASES if not (c.L == 16 and c.bwd and c.bwd[2])])
    assert X.coverage_gaps([c for c in CASES if c.nWx != 1])


def test_launch_rules_by_hand():
    """the rules read from csrc/attention.hip, at counts worked out by hand"""
    assert X.fwd16_route(256, 16, 3) == (256, 1, 0, False, False)            # ceil(4096 / 3) = 1366 groups at most
    assert X.fwd16_route(4096, 16, 3) == (1366, 3, 0, True, False)           # 1366 + 1366 + 1364
    assert X.bwd16_route(9, 16, 3) == (12, 1, 3, False, False)               # 9 waves rounded up to 3 workgroups
    assert X.bwd16_route(2048, 16, 3) == (684, 3, 0, True, False)            # ceil(2048 / 3) = 683 -> 171 workgroups
    assert X.wide_fwd_route(9, 32, 3) == (5, 1, 0, False, True)
    assert X.wide_fwd_route(16, 32, 3) == (8, 1, 0, False, False)
    assert X.wide_bwd_route(99, 32, 24) == (21, 3, 0, True, True)            # 50 pairs on 512 / 24 = 21 groups
    assert X.wide_bwd_route(45, 64, 24) == (21, 3, 0, True, False)
    assert X.wide_bwd_route(4, 64, 1024) == (1, 4, 0, False, False)          # 512 / nh == 0: one group
    assert X.partial_rows(351, 16, 24) == 22 and X.partial_rows(99, 32, 24) == 21
    grp, sweep = X.window_group(99, 32, 24)
    assert grp.tolist()[:4] == [0, 0, 1, 1] and sweep[41] == 0 and grp[42] == 0 and sweep[42] == 1 and sweep[98] == 2
    grp, sweep = X.window_group(351, 16, 24)
    assert grp[7] == 1 and grp[88] == 0 and sweep[88] == 1 and sweep[350] == 3


def test_rounding_margin_of_one_over_n():
    assert X.BAD_N == {9, 13, 15, 18, 26, 30, 36, 43, 52, 60}
    for n in range(1, 65):          # outside BAD_N a relative error of 2^-12 either way leaves bf16(1/n) where it is
        if n not in X.BAD_N:
            x = torch.tensor([1.0 / n], dtype=torch.float64)
            assert torch.equal(ND.round_bf16(x * (1 - 2.0 ** -12)), ND.round_bf16(x * (1 + 2.0 ** -12))), n
    assert float(torch.tensor([34.0, 38.0]).to(torch.float8_e4m3fn).float()[0]) == 32.0
    assert float(torch.tensor([34.0, 38.0]).to(torch.float8_e4m3fn).float()[1]) == 40.0


@pytest.mark.parametrize("name", ["w2x8-p32-nh6-s", "w1x16-p32-nh3-drop", "w2x8-p16-nh6-s-fp8", "w4x8-p16-nh3-s", "w1x64-p32-nh3-s-drop",
                                  "w4x8-row-p32-nh3-s", "w8x8-col-p16-nh6-s"])
def test_reference_is_the_documented_function(name):
    """the expected image of `out` is bf16 of numerics_domain.attn_reference (p rounded, attn_drop and fp8 by keyword)"""
    pb = problem(name)
    c = pb.case
    ref, _ = ND.attn_reference(pb.qkv.view, pb.table.view, c.B, c.H, c.W, c.C, c.nh, c.win, c.sft, c.shifted, round_p=True,
                               p_mult=pb.mult, qk_cast=torch.float8_e4m3fn if c.variant == "fp8" else None)
    o = pb.outs["out"]
    want = o.want[o.idx.reshape(-1)].reshape(c.M, c.C)
    assert torch.equal(X._canon(ND.bits16(ND.round_bf16(ref)).to(torch.int16)), want)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_clean_emulation_passes(case):
    pb = problem(case.name)
    s = pb.stats
    print(f"{case.name}: n {s['n']}, T {s['T']:.2f}, out non-zero {s['out_nonzero']:.3f}" + (
        f", determined dq {s['dq_determined']:.4f} dk {s['dk_determined']:.4f}, non-zero dq {s['dq_nonzero']:.3f} dk {s['dk_nonzero']:.3f}, "
        f"d(bias) u {s['dbias_u']:.2e}" if case.bwd else ""))
    reps = X.check(pb, X.emulate(pb))
    for r in reps:
        print(r.line())
    assert not X.failures(reps), X.failures(reps)


# defect -> the case that finds it, and the report that must fail
DEFECT_CASES = {
    "shift_plus": ("w2x8-p32-nh6-s", ".out"),
    "no_reverse_shift": ("w2x8-p32-nh6-s", ".out"),
    "labels_unrolled": ("w2x8-p32-nh6-s", ".out"),
    "mask_unshifted": ("w2x8-p16-nh3", ".out"),
    "rel_transposed": ("w2x8-p16-nh3", ".out"),
    "table_head_stride1": ("w2x8-p16-nh3", ".out"),
    "head_slice_off": ("w4x16-p32-nh6", ".out"),
    "p_unrounded": ("w8x8-p16-nh3-s", ".out"),
    "dv_undropped": ("w1x16-p32-nh3-drop", ".dqkv (dV"),
    "dp_unmasked": ("w1x32-p16-nh12-s-drop", ".dq"),
    "delta_omitted": ("w2x8-p16-nh3", ".dq"),
    "dk_unscaled": ("w2x16-p32-nh6", ".dk"),
    "fp8_q_only": ("w2x8-p16-nh6-s-fp8", ".dq"),
    "dbias_last_sweep_missing": ("w2x16-p16-nh24-s-bsweeps", ".d(bias), partial rows"),
    "idle_rows_unwritten": ("w2x8-p16-nh3", ".partial rows written"),
    "odd_item_on_window0": ("w4x8-p16-nh3-s", ".out"),
    "row_past_end": ("w2x8-p16-nh3", ".out"),
}


def test_every_defect_is_listed():
    assert set(DEFECT_CASES) == set(X.DEFECTS)


@pytest.mark.parametrize("defect", X.DEFECTS)
def test_defect_fails_its_case(defect):
    name, what = DEFECT_CASES[defect]
    pb = problem(name)
    reps = X.check(pb, X.emulate(pb, defect))
    bad = [r for r in reps if not r.ok]
    print(f"{defect} on {name}: " + "; ".join(str(r) for r in bad))
    assert any(r.what.startswith(name + what) for r in bad), (defect, name, [r.what for r in bad])


def test_d_bias_last_sweep_also_found_at_16_tokens():
    pb = problem("w2x8-p16-nh24-s-sweeps")
    bad = X.failures(X.check(pb, X.emulate(pb, "dbias_last_sweep_missing")))
    assert any("d(bias)" in b for b in bad), bad

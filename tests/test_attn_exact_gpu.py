"""tulip_window_attn_fwd / _bwd and their _drop forms on selector operands (tests/attn_exact.py), through tulip_amd.ops: `out` and dV
equal to the float64 result bit for bit over the whole allocation, dq and dk inside the interval their float64 value and its
propagated error bound round to, d(bias) within its budget through the float64 fold of the partial rows and through the production
fold into the table, every partial row written, every guard word around the three outputs unchanged and no NaN (or far index)
leaking in from the padding around the operands -- on the smallest grids at which each kernel instantiation takes one sweep,
three sweeps with a short last one, idle groups and an invalid second item."""
import pytest
import torch

from tests import attn_exact as X
from tests import gemm_exact as GX

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from tulip_amd import ops as o
    return o


def holds(b, rows, cols, dtype):
    """the allocation really holds the tight [rows][cols] tensor the launch addresses"""
    assert (b.rows, b.cols, b.pitch, b.flat.dtype) == (rows, cols, cols, dtype), (b.rows, b.cols, b.pitch, b.flat.dtype)
    assert b.off + rows * cols <= b.flat.numel()


def launch(ops, pb):
    """forward (and backward, and the production fold of the partial rows) on fresh copies of the case's output allocations"""
    c = pb.case
    L, LL, ntab = c.L, c.L * c.L, (2 * c.win[0] - 1) * (2 * c.win[1] - 1)
    got = X.fresh(pb)
    at = lambda name: pb.outs[name].buf.addr(got[name])
    holds(pb.qkv, c.M, 3 * c.C, GX.BF16), holds(pb.table, ntab, c.nh, GX.F32), holds(pb.rel, L, L, torch.int32)
    holds(pb.outs["out"].buf, c.M, c.C, GX.BF16)
    geom = (c.B, c.H, c.W, c.C, c.nh, c.win, c.sft, c.masked)
    drop = ()
    if c.variant == "drop":
        drop = (torch.tensor([X.DROP_COUNTER], dtype=torch.int64, device=DEV), X.DROP_SEED, X.DROP_SITE, X.DROP_P)
    fwd, bwd = (ops.window_attn_fwd_drop, ops.window_attn_bwd_drop) if drop else (ops.window_attn_fwd, ops.window_attn_bwd)
    fwd(pb.qkv.addr(), pb.table.addr(), pb.rel.addr(), at("out"), *geom, *drop)
    if c.bwd is not None:
        assert ops.window_attn_bwd_partial_rows(c.B, c.H, c.W, c.nh, c.win) == pb.R == X.partial_rows(c.total, L, c.nh)
        holds(pb.dout, c.M, c.C, GX.BF16), holds(pb.outs["dqkv"].buf, c.M, 3 * c.C, GX.BF16)
        holds(pb.outs["part"].buf, pb.R, c.nh * LL, GX.F32), holds(pb.outs["dtab"].buf, ntab, c.nh, GX.F32)
        bwd(pb.qkv.addr(), pb.dout.addr(), pb.table.addr(), pb.rel.addr(), at("dqkv"), at("part"), *geom, *drop)
        ops.reduce_rows_multi([ops.reduce_region(at("part"), c.nh * LL, at("dtab"), c.nh * LL, pb.R, scatter_index=pb.rel.addr(),
                                                 scatter_nh=c.nh, scatter_len=LL)])
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("case", X.gpu_cases(), ids=lambda c: c.name)
def test_window_attention_is_exact(ops, case):
    assert case.fwd == X.fwd_route(case.total, case.L, case.nh)
    assert case.bwd is None or case.bwd == X.bwd_route(case.total, case.L, case.nh)
    pb = X.build(case, DEV)
    s = pb.stats
    print(f"{case.name}: fwd route {case.fwd}, bwd route {case.bwd}, n {s['n']}, out non-zero {s['out_nonzero']:.3f}" + (
        f", determined dq {s['dq_determined']:.4f} dk {s['dk_determined']:.4f}, non-zero dq {s['dq_nonzero']:.3f} dk {s['dk_nonzero']:.3f}, "
        f"d(bias) u {s['dbias_u']:.2e} of the largest entry" if case.bwd else ""))
    reps = X.check(pb, launch(ops, pb))
    for r in reps:
        print(r.line())
    assert not X.failures(reps), (case.name, X.failures(reps))

"""The scalar math inside the kernels on its whole input domain, and the row / window kernels on inputs that are not N(0, 1):
every finite bf16 value through GELU and GELU', special values through the bf16 conversions, every fp16 value through
log1p / expm1, LayerNorm rows with offsets, zero variance and outliers, window attention with large, saturated and uniform
logits, the MC-dropout aggregate's edges.  Inputs, float64 references and predicates: tests/numerics_domain.py (proved sharp
on the CPU by test_numerics_domain_cpu.py).  Every test prints its worst error as a multiple of its budget."""
import math

import numpy as np
import pytest
import torch

from tests import numerics_domain as ND

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from tulip_amd import ops as _ops
    from tulip_amd import _lib
    _lib.load()
    return _ops


def accept(rep):
    print(rep.line())
    assert rep.ok, str(rep)


# ------------------------------------------------------------------ 1. GELU / GELU' in the GEMM epilogues
def test_gelu_epilogue_on_every_finite_bf16_value(ops):
    V = ND.gelu_domain_matrix()
    Vd = V.to(DEV)
    eye = torch.eye(128, dtype=BF16, device=DEV)
    h, g = torch.empty(512, 128, dtype=BF16, device=DEV), torch.empty(512, 128, dtype=BF16, device=DEV)
    ops.gemm(Vd, eye, 512, 128, 128, lda=128, ldb=128, epi=ops.EPI_GELU_DUAL, out=h, out2=g, ldo2=128)
    torch.cuda.synchronize()
    assert torch.equal(h.cpu().float(), V.float())            # one product by 1.0 plus zeros: exact (-0 == +0)
    accept(ND.check_gelu(h.cpu(), g.cpu()))                   # g = bf16(gelu(h)); h carries +0 where V has -0 (-0 + 0 = +0)


def test_gelu_grad_epilogue_on_every_finite_bf16_value(ops):
    V = ND.gelu_domain_matrix()
    A, Bm = torch.zeros(512, 8, dtype=BF16, device=DEV), torch.zeros(128, 8, dtype=BF16, device=DEV)
    A[:, 0] = 1.0
    Bm[:, 0] = 1.0                                             # acc = 1 exactly
    out = torch.empty(512, 128, dtype=BF16, device=DEV)
    ops.gemm(A, Bm, 512, 128, 8, lda=8, ldb=8, epi=ops.EPI_GELU_BWD, out=out, aux=V.to(DEV), ldaux=128)
    torch.cuda.synchronize()
    accept(ND.check_gelu(V, out.cpu(), grad=True))


# ------------------------------------------------------------------ 2. the packed twin inside the fused C = 96 block
def test_gelu_packed_twin_in_the_fused_block(ops):
    """gelu_exact2 / gelu_exact_and_grad2 (reached only from the fused blocks), through tulip_swin96_block_fwd with the shape
    and descriptor of test_swin96_fused_block_forward_matches_separate_kernels (unshifted, bf16 scores): fc1 weight 0 and fc1
    bias = 384 chosen values, so every token's pre-activation is the bias."""
    from tulip_amd.model.tulip import tulip_base
    torch.manual_seed(0)
    m = tulip_base(img_size=(16, 1024), target_img_size=(64, 1024), patch_size=(1, 4), in_chans=1, window_size=[2, 8],
                   pixel_shuffle=True, circular_padding=True, log_transform=True, patch_unmerging=True).to(DEV).train()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.ndim == 1 or "relative_position_bias_table" in n:
                p.add_(0.2 * torch.randn_like(p))
    eng = m.engine()
    eng.bind(torch.device(DEV, torch.cuda.current_device()))
    sp = eng.enc_blocks[0][0]
    assert not sp.shift and sp.C == 96
    p, W_ = sp.prefix, eng.params
    bias = ND.fused_block_fc1_bias()
    ow, ob = W_.offset[p + ".mlp.fc1.weight"], W_.offset[p + ".mlp.fc1.bias"]
    assert W_.numel[p + ".mlp.fc1.weight"] == 384 * 96 and W_.numel[p + ".mlp.fc1.bias"] == 384
    with torch.no_grad():
        W_.flat[ow:ow + 384 * 96].zero_()
        W_.flat[ob:ob + 384].copy_(bias.to(DEV))
    W_.refresh_shadow()
    P = eng.plan(2)
    M = 2 * sp.H * sp.W
    xin = P["enc0.in"]
    xin.copy_((torch.randn(M, 96, device=DEV) * 1.5 + 0.2).view_as(xin))
    du = torch.rand(eng.n_drop_slots, 2, device=DEV)
    du[:, 0] = 0.01
    eng.draw_drop_scales(P, True, du)
    names = ["xn1", "mean1", "rstd1", "qkv", "o", "x1", "xn2", "mean2", "rstd2", "h", "g"]
    want = bias.to(BF16)
    for fc1_grad in (False, True):
        buf = {k: torch.full_like(P[p + "." + k], float("nan") if P[p + "." + k].dtype == torch.float32 else 0) for k in names}
        buf["out"] = torch.full((M, 96), float("nan"), device=DEV)
        ops.swin96_block_fwd(
            x_in=xin, x1=buf["x1"], x_out=buf["out"], xn1=buf["xn1"], qkv=buf["qkv"], attn_out=buf["o"], xn2=buf["xn2"],
            fc1_pre=buf["h"], fc1_act=buf["g"], mean1=buf["mean1"], rstd1=buf["rstd1"], mean2=buf["mean2"],
            rstd2=buf["rstd2"], w_qkv=W_.p16(p + ".attn.qkv.weight"), w_proj=W_.p16(p + ".attn.proj.weight"),
            w_fc1=W_.p16(p + ".mlp.fc1.weight"), w_fc2=W_.p16(p + ".mlp.fc2.weight"), b_qkv=W_.p32(p + ".attn.qkv.bias"),
            b_proj=W_.p32(p + ".attn.proj.bias"), b_fc1=W_.p32(p + ".mlp.fc1.bias"), b_fc2=W_.p32(p + ".mlp.fc2.bias"),
            norm1_weight=W_.p32(p + ".norm1.weight"), norm1_bias=W_.p32(p + ".norm1.bias"),
            norm2_weight=W_.p32(p + ".norm2.weight"), norm2_bias=W_.p32(p + ".norm2.bias"),
            bias_table=W_.p32(p + ".attn.relative_position_bias_table"), rel_index=eng._rel32,
            drop_scale_attn=eng._ds(P, sp, 0), drop_scale_mlp=eng._ds(P, sp, 1), B=2, H=sp.H, W=sp.W,
            shift_h=sp.sft[0], shift_w=sp.sft[1], masked=int(sp.shift) | (4 if fc1_grad else 0), eps=eng.eps)
        torch.cuda.synchronize()
        hbuf, gbuf = buf["h"].reshape(M, 384), buf["g"].reshape(M, 384)
        for t in (hbuf, gbuf):                                  # every token computed the same thing
            assert torch.equal(t.view(torch.int16), t[:1].view(torch.int16).expand(M, 384))
        if fc1_grad:
            accept(ND.check_gelu(want, hbuf[0].cpu(), grad=True, what="fused block gelu' (packed)"))
        else:
            assert torch.equal(hbuf[0].cpu().float(), want.float())          # the saved pre-activation is the bias
        accept(ND.check_gelu(want, gbuf[0].cpu(), what="fused block gelu (packed)"))
        assert torch.isfinite(buf["out"]).all()


# ------------------------------------------------------------------ 3. conversions
def test_bf16_conversions_on_special_values(ops):
    x = ND.cast_words()
    xd = x.to(DEV)
    n = x.numel()
    y = torch.empty(n, dtype=BF16, device=DEV)
    ops.cast_flat(xd, y, n)
    accept(ND.check_cast(x, y.cpu(), "cast_flat"))
    rows, cols = 512, 768
    for rs in (None, torch.ones(rows, device=DEV)):
        y = torch.empty(rows, cols, dtype=BF16, device=DEV)
        ops.cast_f32_bf16(xd, y, rows, cols, rs, 1)
        accept(ND.check_cast(x, y.cpu(), "cast_f32_bf16" + (" with rowscale 1.0" if rs is not None else "")))
    pats = ND.bf16_from_bits(np.arange(65536))
    up = torch.empty(65536, device=DEV)
    ops.cast_bf16_f32(pats.to(DEV), up, 65536)
    accept(ND.check_cast_up(pats, up.cpu()))


# ------------------------------------------------------------------ 4. log1p / expm1
def test_log1p_expm1_on_every_fp16_value(ops):
    raw = ND.all_fp16_image()
    rawd = raw.to(DEV)
    res = {}
    for gate in (ND.PREP_GATE, None):
        hi = torch.full((1, 1, 256, 256), -7.0, device=DEV)
        ops.range_prep(rawd, 1, 65536, 256, 1, 0, hi, None, 1, 256, 256, 1, 1, 0, 0, 1.0, int(gate is not None),
                       *(gate or (0.0, 0.0)), 1, 0)
        torch.cuda.synchronize()
        accept(ND.check_log1p(raw, hi.cpu(), gate))
        res[gate] = hi
    pred = res[ND.PREP_GATE].reshape(256, 256)
    lo = pred[::4].contiguous()
    pred_img, hi_img = torch.full((256, 256), -7.0, device=DEV), torch.full((256, 256), -7.0, device=DEV)
    partials, mae = torch.zeros(2048, dtype=F64, device=DEV), torch.zeros(2, device=DEV)
    ops.eval_postprocess(pred, pred, lo, pred_img, hi_img, partials, mae, 256, 256, 64, 256, 1, *ND.POST_GATE, 0.0)
    torch.cuda.synchronize()
    accept(ND.check_expm1(pred.cpu(), pred_img.cpu(), hi_img.cpu(), ND.POST_GATE, 64))


# ------------------------------------------------------------------ 5. LayerNorm
def _eps32(eps):
    return float(np.float32(eps))           # the kernel's argument is a float: the references get the same number


def _check_constant_rows(got, beta, eps, what):
    """zero variance: mean exactly 3, rstd = 1/sqrt(eps) to 2 fp32 ulp, y = bf16(beta)"""
    assert torch.equal(got["mean"].cpu(), torch.full_like(got["mean"].cpu(), 3.0)), what
    want = torch.full_like(got["rstd"].cpu().to(F64), 1 / math.sqrt(_eps32(eps)))
    assert bool(((got["rstd"].cpu().to(F64) - want).abs() <= 2 * ND.ulp_f32(want)).all()), (what, got["rstd"][:2])
    assert torch.equal(got["y"].cpu().float(), beta.to(BF16).float().expand_as(got["y"])), what


def _ln_family_check(got, x, gamma, beta, dy, eps, fam, what, table):
    ref, err = ND.ln_baseline(x, gamma, beta, dy, _eps32(eps))
    got = {k: v.cpu() for k, v in got.items()}
    if fam == "b":
        _check_constant_rows(got, beta, eps, what)
        got = {k: v for k, v in got.items() if k not in ("y", "mean", "rstd")}
    rep = ND.check_ln(got, ref, err, what)
    table.append((what, {k: (err[k], rep.ratios[k]) for k in got}))
    return rep


def _print_ln_table(table):
    for what, d in table:
        print(what + ": " + ", ".join(f"{k} torch-f32 err {e:.2e} kernel x{r:.2f}" for k, (e, r) in d.items()))


@pytest.mark.parametrize("C,eps", [(48, 1e-5), (96, 1e-6), (384, 1e-5), (1536, 1e-5), (6144, 1e-5)])
def test_layernorm_on_rows_that_are_not_standard_normal(ops, C, eps):
    x, gamma, beta, dy, rows = ND.ln_inputs(C)
    xd, gd, bd, dyd = x.to(DEV), gamma.to(DEV), beta.to(DEV), dy.to(DEV)
    reps, table = [], []
    for fam, sl in rows.items():
        n = sl.stop - sl.start
        xs, dys = xd[sl], dyd[sl]
        y = torch.empty(n, C, dtype=BF16, device=DEV)
        mean, rstd = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
        ops.layernorm_fwd(xs, gd, bd, y, mean, rstd, n, C, eps)
        dx = torch.full((n, C), float("nan"), device=DEV)
        dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        R = ops.layernorm_bwd_partial_rows(n, C)
        if R > 0:
            part = torch.full((R, 2 * C), float("nan"), device=DEV)
            ops.layernorm_bwd(dys, xs, mean, rstd, gd, None, dx, n, C, param_partials=part)
            ops.reduce_rows2(part, 2 * C, dg, C, part[:, C:], 2 * C, db, C, R)
        else:                                                   # C > 2048: the stand-alone parameter-gradient kernel
            ops.layernorm_bwd(dys, xs, mean, rstd, gd, None, dx, n, C)
            ops.layernorm_bwd_params(dys, xs, mean, rstd, dg, db, n, C)
        torch.cuda.synchronize()
        got = {"y": y, "mean": mean, "rstd": rstd, "dx": dx, "dgamma": dg, "dbeta": db}
        reps.append(_ln_family_check(got, x[sl], gamma, beta, dy[sl], eps, fam, f"LayerNorm C={C} family ({fam})", table))
    _print_ln_table(table)
    for rep in reps:
        accept(rep)


def test_layernorm_patch_merge_on_rows_that_are_not_standard_normal(ops):
    B, H, W, Cq, eps = 1, 4, 8, 24, 1e-5
    C, fams = 4 * Cq, ("a", "b", "c", "d", "e", "f", "a", "c")
    gen = torch.Generator().manual_seed(5)
    rows = torch.cat([ND.ln_family_rows(f, 1, C, gen) for f in fams])
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=gen), 0.1 * torch.randn(C, generator=gen)
    dy = torch.randn(8, C, generator=gen).to(BF16)
    x4 = ND.ln_merge_scatter(rows, B, H, W, Cq).to(DEV)
    y = torch.empty(8, C, dtype=BF16, device=DEV)
    mean, rstd = torch.empty(8, device=DEV), torch.empty(8, device=DEV)
    ops.layernorm_fwd(x4, gamma.to(DEV), beta.to(DEV), y, mean, rstd, 8, C, eps, merge=True, B=B, H=H, W=W)
    dx4 = torch.full_like(x4, float("nan"))
    ops.layernorm_bwd(dy.to(DEV), x4, mean, rstd, gamma.to(DEV), None, dx4, 8, C, merge=True, B=B, H=H, W=W)
    torch.cuda.synchronize()
    dx = torch.cat([dx4[:, 0::2, 0::2], dx4[:, 1::2, 0::2], dx4[:, 0::2, 1::2], dx4[:, 1::2, 1::2]], -1).reshape(8, C)
    reps, table = [], []
    for fam in sorted(set(fams)):
        idx = [i for i, f in enumerate(fams) if f == fam]
        got = {"y": y[idx], "mean": mean[idx], "rstd": rstd[idx], "dx": dx[idx]}
        reps.append(_ln_family_check(got, rows[idx], gamma, beta, dy[idx], eps, fam, f"merge LayerNorm family ({fam})", table))
    _print_ln_table(table)
    for rep in reps:
        accept(rep)


def test_splitk_resid_layernorm_on_rows_that_are_not_standard_normal(ops):
    N, eps = 256, 1e-5
    x, gamma, beta, dy, rows = ND.ln_inputs(N)
    M = x.shape[0]
    slabs = ND.split3_exact(x).to(DEV)
    out, xn = torch.full((M, N), float("nan"), device=DEV), torch.empty(M, N, dtype=BF16, device=DEV)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    assert ops.splitk_resid_ln_supported(N)
    ops.splitk_resid_ln(slabs, 3, M, N, None, None, 0, None, 1, out, N, None, 0, gamma.to(DEV), beta.to(DEV), xn, mean, rstd, eps)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), x)                           # the three slabs sum to x exactly, in any order
    reps, table = [], []
    for fam, sl in rows.items():
        got = {"y": xn[sl], "mean": mean[sl], "rstd": rstd[sl]}
        reps.append(_ln_family_check(got, x[sl], gamma, beta, dy[sl], eps, fam, f"split-K fold + LayerNorm family ({fam})", table))
    _print_ln_table(table)
    for rep in reps:
        accept(rep)


# ------------------------------------------------------------------ 6. window attention
def _close(a, b, rtol, atol_scale, what):
    """test_ops_gpu.close: |a - b| <= rtol |b| + atol_scale max|b|"""
    a, b = a.to(F64).cpu(), b.to(F64).cpu()
    err, tol = (a - b).abs(), rtol * b.abs() + atol_scale * (b.abs().max().item() + 1e-30)
    r = (err / tol).max().item()
    print(f"{what}: worst error {r:.3f} x budget")
    assert not (err > tol).any(), f"{what}: {(err > tol).sum().item()}/{err.numel()} out of tolerance, max err {err.max().item():.3e}"


@pytest.mark.parametrize("fam,C,nh,win,shifted", ND.attn_cases())
def test_window_attention_large_saturated_and_uniform_logits(ops, fam, C, nh, win, shifted):
    H, W = ND.ATTN_GRIDS[win]
    B, sft, L = 1, ND.attn_shift(win, shifted), win[0] * win[1]
    M = B * H * W
    qkv, table, dout = ND.attn_inputs(fam, B, H, W, C, nh, win, ND.attn_seed(fam, C, win, shifted))
    qr, tr = qkv.to(F64).requires_grad_(True), table.to(F64).requires_grad_(True)
    ref, scores = ND.attn_reference(qr, tr, B, H, W, C, nh, win, sft, int(shifted))
    if fam == "large":
        assert float(scores.detach().abs().max()) > 40
    ref.backward(dout.to(F64))
    rel32 = ND.rel_position_index(*win).to(torch.int32).contiguous().to(DEV)
    qd, td = qkv.to(DEV), table.to(DEV)
    out = torch.full((M, C), float("nan"), dtype=BF16, device=DEV)
    ops.window_attn_fwd(qd, td, rel32, out, B, H, W, C, nh, win, sft, int(shifted))
    dqkv = torch.full((M, 3 * C), float("nan"), dtype=BF16, device=DEV)
    R = ops.window_attn_bwd_partial_rows(B, H, W, nh, win)
    part = torch.full((R * nh, L * L), float("nan"), device=DEV)
    ops.window_attn_bwd(qd, dout.to(DEV), td, rel32, dqkv, part, B, H, W, C, nh, win, sft, int(shifted))
    dtab = torch.zeros(table.shape[0], nh, device=DEV)
    ops.reduce_rows_multi([ops.reduce_region(part, nh * L * L, dtab, nh * L * L, R, scatter_index=rel32, scatter_nh=nh,
                                             scatter_len=L * L)])
    torch.cuda.synchronize()
    tag = f"{fam} {win[0]}x{win[1]}{' shifted' if shifted else ''} C={C}"
    accept(ND.check_attn_fwd(out.cpu(), ref.detach(), qkv, B, H, W, C, nh, win, sft, "attention fwd " + tag))
    if fam == "uniform":
        # exactly uniform softmax over the query's mask region (a power of two of keys; a masked key carries exp(-100) < 2^-144
        # of the sum): the bf16 rounding of the mean of v, exactly
        assert torch.equal(out.cpu().float(), ND.round_bf16(ref.detach()).float())
    accept(ND.check_attn_dqkv(dqkv.cpu(), qr.grad, B, H, W, C, nh, win, sft, "attention dqkv " + tag))
    assert torch.isfinite(part).all()
    _close(dtab, tr.grad, 2e-2, 5e-3, "attention dtable " + tag)


# ------------------------------------------------------------------ 7. MC-dropout aggregate
def test_mc_aggregate_edges(ops):
    for name, preds, thr in ND.mc_cases():
        T, n = preds.shape
        out = torch.full((n,), float("nan"), device=DEV)
        ops.mc_aggregate(preds.to(DEV).contiguous(), T, n, thr, out)
        torch.cuda.synchronize()
        accept(ND.check_mc(preds, thr, out.cpu(), "mc_aggregate " + name))

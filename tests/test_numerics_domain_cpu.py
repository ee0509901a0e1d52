"""The predicates of tests/numerics_domain.py are sharp: for each of them a correct implementation of the operation passes
and a plausible wrong one fails, on exactly the inputs the GPU tests (test_numerics_domain_gpu.py) feed the kernels -- and
those inputs leave no case vacuous."""
import math

import numpy as np
import pytest
import torch

from oracle import tulip_oracle as O
from tests import numerics_domain as ND

F64 = torch.float64


# ------------------------------------------------------------------ helpers of the helpers
def test_round_bf16_is_round_to_nearest_even_on_float64():
    x = ND.cast_words()
    x = x[torch.isfinite(x)]
    assert torch.equal(ND.bits16(ND.round_bf16(x.to(F64))), ND.bits16(x.to(torch.bfloat16)))
    # a float64 just above a bf16 tie that a cast through float32 would round down to the tie, then to even
    t = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=F64)
    assert float(ND.round_bf16(t)) == 1.0 + 2.0 ** -7 and float(t.float().to(torch.bfloat16)) == 1.0
    assert float(ND.ulp_bf16(torch.tensor([1.0], dtype=F64))) == 2.0 ** -7
    assert float(ND.ulp_bf16(torch.tensor([0.0], dtype=F64))) == 2.0 ** -133
    assert float(ND.ulp_f32(torch.tensor([3.0], dtype=F64))) == 2.0 ** -22


# ------------------------------------------------------------------ 1. GELU
def test_gelu_domain_is_every_finite_bf16_value():
    V = ND.gelu_domain_matrix()
    assert V.shape == (512, 128) and torch.isfinite(V.float()).all()
    assert len(set(ND.bits16(V).reshape(-1)[:65280].tolist())) == 65280
    b = ND.fused_block_fc1_bias()
    assert b.numel() == 384 and torch.equal(b, b.to(torch.bfloat16).float())
    for v in (0.0, 2.0 ** -126, -2.0 ** -126, 5.5, -100.0, 2.0 ** -20):
        assert (b == v).any(), v


@pytest.mark.parametrize("grad", [False, True])
def test_gelu_predicate_accepts_formula_7_1_26_in_float32(grad):
    x = ND.all_finite_bf16()
    got = torch.from_numpy(ND.gelu_as7126_f32(x.float().numpy(), grad)).to(torch.bfloat16)
    rep = ND.check_gelu(x, got, grad)
    print(rep)
    assert rep.ok, str(rep)
    assert 0 < rep.worst <= 1


@pytest.mark.parametrize("grad", [False, True])
def test_gelu_predicate_rejects_tanh_gelu_and_truncation(grad):
    x = ND.all_finite_bf16()
    x64 = x.to(F64)
    if grad:
        xr = x64.clone().requires_grad_(True)
        ND.gelu_tanh_f64(xr).sum().backward()
        tanh = torch.nan_to_num(xr.grad, nan=0.0)                # |x| > 1e100-ish never occurs in bf16; inf * 0 at the far ends
        tanh = torch.where(x64.abs() > 1e10, (x64 > 0).to(F64), tanh)
        exact = ND.gelu_grad_ref(x64)
    else:
        tanh = torch.where(x64.abs() > 1e10, x64.clamp(min=0), ND.gelu_tanh_f64(x64))
        exact = ND.gelu_ref(x64)
    rep = ND.check_gelu(x, ND.round_bf16(tanh), grad)
    assert not rep.ok and any("above budget" in v for v in rep.violations), str(rep)
    rep = ND.check_gelu(x, ND.round_bf16(exact, truncate=True), grad)
    assert not rep.ok and any("above budget" in v for v in rep.violations), str(rep)
    assert ND.check_gelu(x, ND.round_bf16(exact), grad).ok          # and the correctly rounded float64 result passes


def test_gelu_predicate_rejects_wrong_sign_and_broken_identity():
    x = ND.all_finite_bf16()
    good = ND.round_bf16(ND.gelu_ref(x.to(F64)))
    bad = good.clone()
    i = int((x.float() == -30.0).nonzero()[0])
    bad[i] = 1e-30                                                  # inside the absolute budget, wrong sign
    rep = ND.check_gelu(x, bad)
    assert any("> 0 for x < 0" in v for v in rep.violations), str(rep)
    bad = good.clone()
    j = int((x.float() == 16.0).nonzero()[0])
    bad[j] = ND.bf16_from_bits([int(ND.bits16(x[j:j + 1])) - 1])[0]  # one bf16 step: 2^-4 ... but the |x| E term is 8e-6
    rep = ND.check_gelu(x, bad)
    assert any("bitwise" in v for v in rep.violations), str(rep)


# ------------------------------------------------------------------ 3. conversions
def test_cast_predicate_accepts_torch_and_rejects_truncation_flush_and_nan_to_inf():
    x = ND.cast_words()
    assert x.numel() == 393216 == 512 * 768
    assert ND.check_cast(x, x.to(torch.bfloat16)).ok
    for wrong, msg in ((ND.cast_truncating, "bits differ"), (ND.cast_flushing, "bits differ"), (ND.cast_nan_to_inf, "NaN")):
        rep = ND.check_cast(x, wrong(x))
        assert not rep.ok and any(msg in v for v in rep.violations), (wrong.__name__, str(rep))
    # the inputs hold what they claim: ties both ways, a carry into the exponent, overflow to inf, subnormals, NaN payloads
    b = ND.bits32(x).to(torch.int64) & 0xFFFFFFFF
    for word in (0x3F808000, 0x3F818000, 0x3FFF8000, 0x7F7F8000, 0x00000001, 0x007F8000, 0x7F800001, 0xFFC0FFFF, 0x80000000):
        assert (b == word).any(), hex(word)
    assert ND.bits16(x.to(torch.bfloat16))[(b == 0x3F808000)].item() == 0x3F80          # tie -> even (down)
    assert ND.bits16(x.to(torch.bfloat16))[(b == 0x3F818000)].item() == 0x3F82          # tie -> even (up)
    assert ND.bits16(x.to(torch.bfloat16))[(b == 0x7F7F8000)].item() == 0x7F80          # overflow -> inf
    pats = ND.bf16_from_bits(np.arange(65536))
    assert ND.check_cast_up(pats, pats.float()).ok
    assert not ND.check_cast_up(pats, torch.nan_to_num(pats.float(), nan=0.0)).ok


# ------------------------------------------------------------------ 4. log1p / expm1
def test_log1p_expm1_predicates_accept_float32_libm_and_reject_the_naive_forms():
    raw = ND.all_fp16_image()
    x32 = raw.float()
    for gate in (ND.PREP_GATE, None):
        v = torch.where((x32 >= gate[0]) & (x32 <= gate[1]), x32, torch.zeros_like(x32)) if gate else x32
        rep = ND.check_log1p(raw, torch.log1p(v), gate)
        print(rep)
        assert rep.ok and 0 < rep.worst <= 1, str(rep)
        naive = torch.log(1.0 + v)
        rep = ND.check_log1p(raw, naive, gate)
        assert any("2 fp32 ulp" in s for s in rep.violations), str(rep)
    rep = ND.check_log1p(raw, torch.log1p(x32), ND.PREP_GATE)                       # a gate that is ignored
    assert any("did not produce 0" in s for s in rep.violations)
    pred = torch.log1p(torch.where((x32 >= 0) & (x32 <= 120), x32, torch.zeros_like(x32)))[0]
    assert float(pred.max()) > 4.7 and int((pred > 0).sum()) > 20000
    good = torch.expm1(pred)

    def post(f):
        img = f(pred)
        out = torch.where((img >= ND.POST_GATE[0]) & (img <= ND.POST_GATE[1]), img, torch.zeros_like(img))
        out[::4] = img[::4]
        return out, img

    rep = ND.check_expm1(pred, *post(torch.expm1), ND.POST_GATE, 64)
    print(rep)
    assert rep.ok and 0 < rep.worst <= 1, str(rep)
    rep = ND.check_expm1(pred, *post(lambda t: torch.exp(t) - 1.0), ND.POST_GATE, 64)
    assert any("hi_img" in s for s in rep.violations) and any("restored" in s for s in rep.violations), str(rep)
    rep = ND.check_expm1(pred, good, good, ND.POST_GATE, 64)                         # gate not applied
    assert any("gated-out" in s for s in rep.violations), str(rep)
    ref = torch.expm1(pred.to(F64))                                                  # both gate decisions occur
    assert ((ref > 100) & (ref <= 120)).any() and ((ref > 0) & (ref < 0.5)).any()


# ------------------------------------------------------------------ 5. LayerNorm
def _ln_parts(C, eps):
    x, gamma, beta, dy, rows = ND.ln_inputs(C)
    return x, gamma, beta, dy, rows


@pytest.mark.parametrize("C,eps", [(48, 1e-5), (96, 1e-6), (384, 1e-5), (1536, 1e-5), (6144, 1e-5)])
def test_layernorm_predicate_accepts_torch_float32_and_rejects_one_pass_variance_and_dropped_eps(C, eps):
    x, gamma, beta, dy, rows = _ln_parts(C, eps)
    for fam, sl in rows.items():
        ref, err = ND.ln_baseline(x[sl], gamma, beta, dy[sl], eps)
        f32 = ND.ln_torch(x[sl], gamma, beta, dy[sl], eps, torch.float32)
        f32["y"] = f32["y"].to(torch.bfloat16)
        rep = ND.check_ln(f32, ref, err, f"C={C} family {fam}")
        assert rep.ok, str(rep)
        # no family is vacuous: torch float32 has an error on every output -- except the constant rows, whose mean and
        # output are exact
        if fam == "b":
            assert err["y"] == 0 and err["mean"] == 0 and err["dx"] > 0, err
        else:
            assert err["y"] > 0 and err["dx"] > 0 and err["rstd"] > 0 and err["dgamma"] > 0, (fam, err)
        if fam == "a":
            rep = ND.check_ln(ND.ln_onepass_f32(x[sl], gamma, beta, eps), ref, err, "one-pass variance")
            assert any(v.startswith("rstd") for v in rep.violations) and any(v.startswith("y") for v in rep.violations), str(rep)
        if fam == "d":
            noeps = ND.ln_torch(x[sl], gamma, beta, dy[sl], 1e-30, torch.float32)
            noeps["y"] = noeps["y"].to(torch.bfloat16)
            rep = ND.check_ln({k: noeps[k] for k in ("y", "rstd", "dx")}, ref, err, "eps dropped")
            assert len(rep.violations) == 3, str(rep)
        if fam == "b":
            assert float(ref["mean"].min()) == float(ref["mean"].max()) == 3.0
            assert torch.allclose(ref["rstd"], torch.full_like(ref["rstd"], 1 / math.sqrt(eps)), rtol=1e-15)
            assert torch.equal(ref["y"], beta.to(F64).expand_as(ref["y"]))


def test_layernorm_merge_scatter_and_exact_slab_split():
    rows = torch.randn(8, 96)
    x = ND.ln_merge_scatter(rows, 1, 4, 8, 24)
    cat = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1).reshape(8, 96)
    assert torch.equal(cat, rows)
    x, *_ = ND.ln_inputs(256, per_family=16)
    s = ND.split3_exact(x)
    assert s.shape == (3, 96, 256) and bool((s[1] != 0).any()) and bool((s[2] != 0).any())


# ------------------------------------------------------------------ 6. window attention
def _oracle_attention(qkv, table, B, H, W, C, nh, win, sft, shifted):
    """tulip_oracle's index tables (window_token_index, relative_position_index, shift_attention_mask), float64, no rounding"""
    L, P = win[0] * win[1], C // nh
    idx = torch.from_numpy(O.window_token_index(H, W, win, sft))
    nW = idx.shape[0]
    t = qkv.to(F64).reshape(B, H * W, 3 * C)[:, idx.reshape(-1)].reshape(B * nW, L, 3, nh, P).permute(2, 0, 3, 1, 4)
    rel = torch.from_numpy(O.relative_position_index(*win))
    attn = (t[0] @ t[1].transpose(-2, -1)) * P ** -0.5 + table.to(F64)[rel.reshape(-1)].reshape(L, L, nh).permute(2, 0, 1)[None]
    if shifted:
        mask = torch.from_numpy(O.shift_attention_mask(H, W, win, sft)).to(F64)
        attn = (attn.reshape(B, nW, nh, L, L) + mask[None, :, None]).reshape(B * nW, nh, L, L)
    o = (torch.softmax(attn, -1) @ t[2]).permute(0, 2, 1, 3).reshape(B, nW * L, C)
    out = torch.zeros(B, H * W, C, dtype=F64)
    out[:, idx.reshape(-1)] = o
    return out.reshape(B * H * W, C)


@pytest.mark.parametrize("fam,C,nh,win,shifted", ND.attn_cases())
def test_attention_reference_and_predicates(fam, C, nh, win, shifted):
    H, W = ND.ATTN_GRIDS[win]
    B, sft = 1, ND.attn_shift(win, shifted)
    qkv, table, dout = ND.attn_inputs(fam, B, H, W, C, nh, win, ND.attn_seed(fam, C, win, shifted))
    args = (qkv, table, B, H, W, C, nh, win, sft, int(shifted))
    ref, s = ND.attn_reference(*args)
    assert torch.equal(ND.rel_position_index(*win), torch.from_numpy(O.relative_position_index(*win)))
    if fam == "control":                 # the restatement is the oracle's function
        assert (ref - _oracle_attention(qkv, table, B, H, W, C, nh, win, sft, shifted)).abs().max().item() <= 1e-12
    chk = lambda got, what: ND.check_attn_fwd(got, ref, qkv, B, H, W, C, nh, win, sft, what)
    # passes: the reference rounded through bf16 at P and at the output
    rounded = ND.attn_reference(*args, round_p=True)[0].to(torch.bfloat16)
    rep = chk(rounded, "bf16-rounded reference")
    assert rep.ok and 0 <= rep.worst <= 1, str(rep)
    if fam == "large":
        assert float(s.abs().max()) > 40 and float(s.max()) > 88.73 and float(s.min()) < -40
        nomax = ND.attn_reference(*args, dtype=torch.float32, softmax="nomax")[0]
        assert not chk(nomax, "float32 softmax without max subtraction").ok
        assert chk(ND.attn_reference(*args, dtype=torch.float32)[0], "float32 softmax").ok
    if fam == "uniform":
        p = torch.softmax(s, -1)
        n = (p > 1e-3).sum(-1)
        assert bool(((n & (n - 1)) == 0).all()) and float((p[p > 1e-3] * n[..., None].expand_as(p)[p > 1e-3] - 1).abs().max()) < 1e-40
        assert torch.equal(ND.round_bf16(ref).float(), rounded.float())
    if shifted:
        assert not chk(ND.attn_reference(*args, use_mask=False)[0], "mask omitted").ok
        assert not chk(ND.attn_reference(*args, shift_error=(0, 1))[0], "shift off by one token").ok
    # backward predicate: float64 autograd passes, a gradient with one window-head's dq zeroed fails
    qr, tr = qkv.to(F64).requires_grad_(True), table.to(F64).requires_grad_(True)
    ND.attn_reference(qr, tr, *args[2:])[0].backward(dout.to(F64))
    g = qr.grad.to(torch.bfloat16)
    rep = ND.check_attn_dqkv(g, qr.grad, B, H, W, C, nh, win, sft, "bf16-rounded autograd")
    assert rep.ok and rep.worst <= 2.0 ** -2, str(rep)
    bad = qr.grad.clone()
    bad[:, 2 * C:] = 0
    assert not ND.check_attn_dqkv(bad, qr.grad, B, H, W, C, nh, win, sft, "dv dropped").ok
    assert float(tr.grad.abs().max()) > 0


# ------------------------------------------------------------------ 7. MC-dropout aggregate
def test_mc_predicate():
    for name, preds, thr in ND.mc_cases():
        p = preds.to(F64)
        mean, sd = p.mean(0), p.std(0, unbiased=True)
        good = torch.where(sd > thr * mean, torch.zeros_like(mean), mean).float()
        rep = ND.check_mc(preds, thr, good, name)
        assert rep.ok and rep.n_compared > 0, str(rep)
        if "identical" in name:
            # sd = 0: positive means are kept; a negative mean has 0 > thr * mean and is zeroed, by the definition
            assert bool((sd == 0).all()) and torch.equal(good != 0, (mean > 0))
            if preds.shape[1] > 1:
                assert not ND.check_mc(preds, thr, mean.float(), name).ok             # "keep everything" is caught
        if "outlier" in name:
            assert not ND.check_mc(preds, thr, mean.float(), name).ok                 # never zeroing is caught
            if preds.shape[1] > 1:
                assert bool((good == 0).any()) and bool((good != 0).any())               # both decisions occur
        if "exactly 0" in name:
            assert bool((mean == 0).all()) and bool((good == 0).all())

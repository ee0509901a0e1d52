"""The AdamW auditor (tests/adamw_audit.py) has teeth: on a real FlatParams layout (the tiny model, padding between parameters)
and realistic optimizer state, it accepts the float32 emulation of adamw_step4 and torch.optim.AdamW, and rejects each fault
a step plan could make -- naming the tensor it was injected into."""
import re

import numpy as np
import pytest
import torch

from tests import adamw_audit as AA
from tests.test_host_logic import tiny
from tulip_amd.engine import FlatParams
from tulip_amd.trainer import cosine_lr

STEPS = 5


def _lr(t):
    """lr of optimizer step t: warm-up then cosine, so that neighbouring steps differ by a few per cent or more."""
    return cosine_lr(t - 1, 5e-4, 1e-5, 2, STEPS + 2) + 1e-5


@pytest.fixture(scope="module")
def run():
    torch.manual_seed(0)
    _, model = tiny()
    fp = FlatParams(model, torch.device("cpu"))
    lay = AA.Layout(model, fp)
    gen = torch.Generator().manual_seed(1)
    decay, inside, *_ = lay.tensors("cpu")
    # per-tensor gradient magnitude 1e-5 .. 1e-1, per-element log-normal spread, 1 % exact zeros, nothing in the padding
    scale = torch.zeros(lay.total, dtype=torch.float64)
    for n in lay.names:
        scale[lay.offset[n]:lay.offset[n] + lay.numel[n]] = 10.0 ** float(torch.empty(1).uniform_(-5, -1, generator=gen))
    grads = []
    for t in range(1, STEPS + 1):
        g = torch.randn(lay.total, generator=gen, dtype=torch.float64) * scale * torch.exp(
            torch.randn(lay.total, generator=gen, dtype=torch.float64))
        g[torch.rand(lay.total, generator=gen) < 0.01] = 0
        grads.append(torch.where(inside, g, torch.zeros_like(g)).float())
    hyp = [AA.Hyper(lr=_lr(t), t=t) for t in range(1, STEPS + 1)]
    # the float32 emulation
    p = fp.flat.clone()
    emu = [{"p": p, "m": torch.zeros_like(p), "v": torch.zeros_like(p), "shadow": p.to(torch.bfloat16)}]
    for g, h in zip(grads, hyp):
        s = emu[-1]
        p1, m1, v1 = AA.emulate(s["p"], g, s["m"], s["v"], decay, h)
        emu.append({"p": p1, "m": m1, "v": v1, "shadow": p1.to(torch.bfloat16), "g": g})
    # torch.optim.AdamW (foreach=False), timm's grouping, on per-tensor copies
    params = {n: torch.nn.Parameter(fp.flat[lay.offset[n]:lay.offset[n] + lay.numel[n]].clone()) for n in lay.names}
    opt = torch.optim.AdamW([{"params": [params[n] for n in lay.names if lay.decays[n]], "weight_decay": 0.01},
                             {"params": [params[n] for n in lay.names if not lay.decays[n]], "weight_decay": 0.0}],
                            lr=5e-4, betas=(0.9, 0.95), eps=1e-8, foreach=False)
    ref = [emu[0]]
    for g, h in zip(grads, hyp):
        for grp in opt.param_groups:
            grp["lr"] = h.lr
        for n in lay.names:
            params[n].grad = g[lay.offset[n]:lay.offset[n] + lay.numel[n]].clone()
        opt.step()
        s = {k: torch.zeros_like(fp.flat) for k in ("p", "m", "v")}
        s["p"].copy_(fp.flat)                         # (padding: the initial zeros)
        for n in lay.names:
            sl = slice(lay.offset[n], lay.offset[n] + lay.numel[n])
            s["p"][sl] = params[n].detach()
            s["m"][sl] = opt.state[params[n]]["exp_avg"]
            s["v"][sl] = opt.state[params[n]]["exp_avg_sq"]
        s["shadow"], s["g"] = s["p"].to(torch.bfloat16), g
        ref.append(s)
    return {"lay": lay, "emu": emu, "ref": ref, "grads": grads, "hyp": hyp, "decay": decay}


def _check(run, snaps, t, mode, exact=True):
    """audit of step t (1-based) in `mode`: 'known' or 'unknown'."""
    a, b = snaps[t - 1], snaps[t]
    return AA.audit(a, b, run["lay"], run["hyp"][t - 1], grad=b["g"] if mode == "known" else None, exact=exact)


@pytest.mark.parametrize("mode", ["known", "unknown"])
def test_the_emulation_is_accepted_at_every_step(run, mode):
    for t in range(1, STEPS + 1):
        assert _check(run, run["emu"], t, mode) == [], t


@pytest.mark.parametrize("mode", ["known", "unknown"])
def test_torch_adamw_is_accepted_at_every_step(run, mode):
    """torch.optim.AdamW's float32 evaluation (lerp, addcmul, hyperparameters from Python doubles) is not the kernel's bit
    pattern: accepted by the float64 bounds (exact=False), and its moments are indeed not bit-identical to the emulation."""
    for t in range(1, STEPS + 1):
        assert _check(run, run["ref"], t, mode, exact=False) == [], t
    assert not torch.equal(run["ref"][STEPS]["m"], run["emu"][STEPS]["m"])


def test_the_bounds_are_tight_enough_to_be_worth_having(run):
    """On correct steps the worst p error stays within the ulp budget and the worst v residual well inside its bound."""
    rep = AA.Report(run["lay"], "cpu")
    for t in range(1, STEPS + 1):
        AA.audit(run["emu"][t - 1], run["emu"][t], run["lay"], run["hyp"][t - 1], report=rep)
    assert rep.stats["p_ulps"] == 0.0            # the emulation against itself
    assert 0.0 < rep.stats["v_frac"] < 1.0


# ---------------------------------------------------------------------------------------------------------------- faults
T_FAULT = 3


def _names(run):
    lay = run["lay"]
    big = lambda n: lay.numel[n] >= 256
    dec = next(n for n in lay.names if lay.decays[n] and big(n) and n.endswith("qkv.weight"))
    nodec = max((n for n in lay.names if not lay.decays[n] and "norm" in n and n.endswith(".weight")), key=lambda n: lay.numel[n])
    return dec, nodec


def _elem(run, name, t=T_FAULT):
    """the element of `name` with the largest gradient (where a wrong moment matters)."""
    lay, g = run["lay"], run["grads"][t - 1]
    lo = lay.offset[name]
    gg = g[lo:lo + lay.numel[name]].abs()
    return lo + int(torch.argmax(gg))


def _after(run, t=T_FAULT):
    return {k: v.clone() for k, v in run["emu"][t].items()}


def _restep(run, out, sl, h, decay=None, g=None, twice=False, t=T_FAULT):
    """recompute `sl` of the step's result with other hyperparameters / decay / gradient."""
    a = run["emu"][t - 1]
    g = run["grads"][t - 1] if g is None else g
    dec = run["decay"] if decay is None else decay
    p1, m1, v1 = AA.emulate(a["p"][sl], g[sl], a["m"][sl], a["v"][sl], dec[sl], h)
    if twice:
        p1, m1, v1 = AA.emulate(p1, g[sl], m1, v1, dec[sl], h)
    out["p"][sl], out["m"][sl], out["v"][sl] = p1, m1, v1
    out["shadow"][sl] = p1.to(torch.bfloat16)
    return out


def _tensor_slice(run, name):
    lay = run["lay"]
    return slice(lay.offset[name], lay.offset[name] + lay.numel[name])


def _assert_rejected(run, after, name, modes=("known", "unknown"), t=T_FAULT):
    snaps = list(run["emu"])
    snaps[t] = after
    for mode in modes:
        v = _check(run, snaps, t, mode)
        assert v, (mode, "fault not detected")
        for line in v:
            assert f": {name}: " in line, (mode, line)


def _b1m_plus_g(run, after, idx, t=T_FAULT):
    """the observed corruption: exp_avg = b1 m + g (instead of b1 m + (1 - b1) g), the step taken with it."""
    a, g, h = run["emu"][t - 1], run["grads"][t - 1], run["hyp"][t - 1]
    b1 = torch.tensor(np.float32(h.betas[0]))
    after["m"][idx] = b1 * a["m"][idx] + g[idx]
    c = h.f32()
    after["p"][idx] = AA._emulate_p(a["p"][idx], after["m"][idx], after["v"][idx], run["decay"][idx], c)
    after["shadow"][idx] = after["p"][idx].to(torch.bfloat16)
    return after


def test_rejects_b1m_plus_g_on_one_element(run):
    for name in _names(run):
        j = _elem(run, name)
        _assert_rejected(run, _b1m_plus_g(run, _after(run), torch.tensor([j])), name)


def test_rejects_b1m_plus_g_on_the_observed_pattern(run):
    """one component of 16 consecutive float4s: every fourth element of 64."""
    name, _ = _names(run)
    lo = run["lay"].offset[name] + 128
    idx = lo + 1 + 4 * torch.arange(16)
    _assert_rejected(run, _b1m_plus_g(run, _after(run), idx), name)
    snaps = list(run["emu"])
    snaps[T_FAULT] = _b1m_plus_g(run, _after(run), idx)
    v = _check(run, snaps, T_FAULT, "unknown")
    n = max(int(re.search(r": (\d+)/", line).group(1)) for line in v)
    assert n >= 12, v                                   # (elements whose gradient is far below its moment can hide)


@pytest.mark.parametrize("dt", [-1, 1])
def test_rejects_the_lr_of_the_neighbouring_step(run, dt):
    name, _ = _names(run)
    h = run["hyp"][T_FAULT - 1]
    wrong = AA.Hyper(lr=_lr(T_FAULT + dt), t=h.t)
    assert abs(wrong.lr - h.lr) > 0.02 * h.lr
    _assert_rejected(run, _restep(run, _after(run), _tensor_slice(run, name), wrong), name)


@pytest.mark.parametrize("dt", [-1, 1])
def test_rejects_a_step_index_off_by_one(run, dt):
    for name in _names(run):
        h = run["hyp"][T_FAULT - 1]
        _assert_rejected(run, _restep(run, _after(run), _tensor_slice(run, name), AA.Hyper(lr=h.lr, t=h.t + dt)), name)


def test_rejects_decay_in_the_wrong_group(run):
    dec, nodec = _names(run)
    flip = ~run["decay"]
    for name in (dec, nodec):
        _assert_rejected(run, _restep(run, _after(run), _tensor_slice(run, name), run["hyp"][T_FAULT - 1], decay=flip), name)


def test_rejects_an_element_not_stepped(run):
    for name in _names(run):
        j = _elem(run, name)
        after = _after(run)
        for k in ("p", "m", "v", "shadow"):
            after[k][j] = run["emu"][T_FAULT - 1][k][j]
        _assert_rejected(run, after, name)


def test_rejects_an_element_stepped_twice(run):
    for name in _names(run):
        j = _elem(run, name)
        _assert_rejected(run, _restep(run, _after(run), slice(j, j + 1), run["hyp"][T_FAULT - 1], twice=True), name)


def test_rejects_p_from_the_old_moment(run):
    for name in _names(run):
        j = torch.tensor([_elem(run, name)])
        a, after = run["emu"][T_FAULT - 1], _after(run)
        c = run["hyp"][T_FAULT - 1].f32()
        after["p"][j] = AA._emulate_p(a["p"][j], a["m"][j], after["v"][j], run["decay"][j], c)
        after["shadow"][j] = after["p"][j].to(torch.bfloat16)
        _assert_rejected(run, after, name)


def test_rejects_a_shadow_one_bf16_ulp_off(run):
    for name in _names(run):
        j = _elem(run, name)
        after = _after(run)
        after["shadow"].view(torch.int16)[j] += 1
        _assert_rejected(run, after, name)


def test_rejects_padding_written(run):
    lay = run["lay"]
    _, inside, *_ = lay.tensors("cpu")
    j = int(torch.nonzero(~inside)[0])
    for k in ("p", "m", "v", "shadow"):
        after = _after(run)
        after[k][j] = 1e-3
        _assert_rejected(run, after, "padding")


def test_rejects_a_change_in_a_non_update_micro_step(run):
    name, nodec = _names(run)
    s = run["emu"][T_FAULT]
    assert AA.audit_unchanged(s, {k: v.clone() for k, v in s.items()}, run["lay"]) == []
    for k, nm in (("p", name), ("m", nodec), ("v", name), ("shadow", nodec)):
        after = {kk: v.clone() for kk, v in s.items()}
        j = _elem(run, nm)
        after[k].view(torch.int16 if k == "shadow" else torch.int32)[j] += 1
        v = AA.audit_unchanged(s, after, run["lay"])
        assert len(v) == 1 and f": {nm}: 1/" in v[0], v


def test_at_t1_the_unknown_mode_is_nearly_exact(run):
    """m0 = v0 = 0: g^ is (1 - b1) g / (1 - b1) up to one rounding, and a moment scaled by a few ulps is caught."""
    name, _ = _names(run)
    j = _elem(run, name, t=1)
    after = {k: v.clone() for k, v in run["emu"][1].items()}
    after["v"][j] = after["v"][j] * (1 + 8 * AA.U)
    v = AA.audit(run["emu"][0], after, run["lay"], run["hyp"][0])
    assert any(f": {name}: " in line for line in v), v


@pytest.mark.parametrize("r", [-1, 1])
def test_rsqrt_one_ulp_off_for_the_whole_step_is_accepted(run, r):
    """the device's rsqrtf(bc2) may be a float32 neighbour of the correctly rounded value: the same one for every element."""
    t = T_FAULT
    a, after = run["emu"][t - 1], _after(run)
    after["p"] = AA._emulate_p(a["p"], after["m"], after["v"], run["decay"], run["hyp"][t - 1].f32(), rsq_ulp=r)
    after["shadow"] = after["p"].to(torch.bfloat16)
    assert not torch.equal(after["p"], run["emu"][t]["p"])
    snaps = list(run["emu"])
    snaps[t] = after
    for mode in ("known", "unknown"):
        assert _check(run, snaps, t, mode) == [], mode

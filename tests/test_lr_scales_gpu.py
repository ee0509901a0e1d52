"""Per-parameter learning-rate scales (layer-wise lr decay) in the fused AdamW: every optimizer step of real training steps
audited against AdamW at each tensor's OWN rate fl32(lr * scale) (tests/adamw_audit.py, called group by group through
tests/lr_scale_audit.py), in every step structure; against torch.optim.AdamW over groups carrying lr * lr_scale; through the
torch.optim import / export and the Trainer's own checkpoint."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import tulip_oracle as O
from tests import adamw_audit as AA
from tests.lr_scale_audit import audited_steps_scaled, sites_seen
from tests.test_adamw_audit_gpu import batch, lr_at, make
from tests.test_model_gpu import build
from tulip_amd.trainer import Trainer

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = lambda x: float(np.float32(x))


def three_scales(model):
    """1.0 / 0.5 / 2^-7 round-robin over the tensors in registration order: neighbours in every launch differ."""
    return {n: (1.0, 0.5, 0.0078125)[i % 3] for i, (n, _) in enumerate(model.named_parameters())}


def layer_decay(model):
    from tulip_amd.trainer import layer_decay_scales
    return layer_decay_scales(model)


def check_sites(tr, scales, want):
    seen = sites_seen(tr, scales)
    assert set(seen) == set(want), (sorted(seen), want)
    for site, sc in seen.items():
        assert len(sc) >= 2, f"site {site} stepped tensors of one scale only: {sc}"
    return seen


@pytest.mark.parametrize("mode", ["captured", "eager", "accum2"])
def test_every_update_is_adamw_at_its_groups_rate(mode):
    """tulip_base KITTI batch 8 (the audit tests' model), three scales, three optimizer steps (t = 1, 2, 3), a new learning
    rate at each.  captured: the default plan -- weight-gradient write-outs, fold launches and the listed blocks at the end;
    eager and accum_iter = 2 (with the gradient-norm read-out): everything in the scanning launch.  Together the four AdamW
    sites; each must have stepped tensors of at least two scales.  Without the scales in the kernels every tensor of the 0.5
    and 2^-7 groups moves at the unscaled rate and fails the parameter checks."""
    m = make()
    scales = three_scales(m)
    kw = {"captured": {}, "eager": dict(use_graph=False), "accum2": dict(accum_iter=2, track_grad_norm=True)}[mode]
    tr = Trainer(m, 8, lr_scales=scales, **kw)
    tr.load_batch(*batch(m, 8))
    n, grad_mode = {"captured": (3, "nonzero"), "eager": (3, "known"), "accum2": (6, "unknown")}[mode]
    v, stats, _ = audited_steps_scaled(tr, n, grad_mode, scales, lr_at)
    assert tr.t == 3
    if mode == "captured":
        assert tr.fuse_adamw and tr.fused_adamw_params > 0 and tr.step_form == "one_graph"
        check_sites(tr, scales, {"writeout", "fold", "blocks" if tr._adam_blocks is not None else "scan"})
    else:
        assert tr.fused_adamw_params == 0
        check_sites(tr, scales, {"scan"})
    print(f"{mode}: worst p error {stats.get('p_ulps', 0):.3g} ulp, worst v residual {stats.get('v_frac', 0):.3g} of its bound")
    assert v == [], "\n".join(v[:40])


def test_one_rank_segmented_plans(tmp_path):
    """The N > 1 step structure on one rank over RCCL (tests/lr_scales_ws1_worker.py): graph segments with the end-of-step
    launch, bucket_adamw (tulip_adamw on each bucket's slice of the mask), bf16 gradient exchange; exchange='sharded' refuses
    scales other than 1.0."""
    out = tmp_path / "lr_scales_ws1.pt"
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29553")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lr_scales_ws1_worker.py"), str(out), "3"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = torch.load(out)
    assert got["backend"] == "nccl"
    for name in ("segments", "bucket_adamw", "bf16"):
        g = got[name]
        assert g["form"] == "segments" and g["segmented"] and g["buckets"] >= 2, (name, g["form"], g["buckets"])
        assert g["violations"] == [], (name, "\n".join(g["violations"][:40]))
        assert list(g["sites"]) == ["scan"] and len(g["sites"]["scan"]) == 3, g["sites"]
    assert got["bucket_adamw"]["bucket_adamw"] and got["bf16"]["gb"]
    assert got["sharded_raises"] is True and got["sharded_ones_ok"] is True


def _state(tr):
    W = tr.eng.params
    return {"p": W.flat.clone(), "m": tr.m.clone(), "v": tr.v.clone(), "shadow": W.shadow.clone()}


def _same_bits(a, b):
    return [k for k in a if not torch.equal(AA._bits(a[k]), AA._bits(b[k]))]


def test_all_ones_is_the_step_without_scales():
    """lr_scales=None against {every name: 1.0}: three captured steps, p / m / v / bf16 shadow bit-identical.  And with ONE
    tensor at 0.5 -- the table and the `_s` launches in use everywhere -- every other tensor (group 0, table entry 1.0f) is
    still bit-identical after the first step (later steps see the changed tensor through the forward)."""
    runs = {}
    for name in ("none", "ones", "one_half"):
        m = make()
        last = [n for n, _ in m.named_parameters()][-1]
        sc = {"none": None, "ones": {n: 1.0 for n, _ in m.named_parameters()}, "one_half": {last: 0.5}}[name]
        tr = Trainer(m, 8, lr_scales=sc)
        assert (tr._lr_table is not None) == (name == "one_half")
        tr.load_batch(*batch(m, 8))
        tr.step(lr=lr_at(1))
        first = _state(tr)
        if name != "one_half":
            tr.step(lr=lr_at(2)); tr.step(lr=lr_at(3))
        runs[name] = (first, _state(tr), tr.eng.params, last)
        del tr, m
    assert _same_bits(runs["none"][1], runs["ones"][1]) == []
    a, (b, _, W, last) = runs["none"][0], runs["one_half"]
    others = torch.ones(W.total, dtype=torch.bool, device=DEV)
    others[W.offset[last]:W.offset[last] + W.numel[last]] = False
    for k in a:
        assert torch.equal(AA._bits(a[k])[others], AA._bits(b[k])[others]), k
    assert not torch.equal(a["p"][~others], b["p"][~others])                                               # the scaled tensor moved differently
    assert torch.equal(a["m"][~others], b["m"][~others]) and torch.equal(a["v"][~others], b["v"][~others])  # same gradient, same moments


# ---------------------------------------------------------------------------------------------------------------- torch.optim.AdamW
LR, WD, BETAS = 5e-4, 0.01, (0.9, 0.95)


def torch_groups(model, scales, lr):
    """One group per (scale, decays): what timm's param_groups_layer_decay builds, after the schedule has set lr * lr_scale."""
    by = {}
    for n, p in model.named_parameters():
        by.setdefault((f32(scales[n]), p.ndim > 1), []).append(p)
    return [{"params": ps, "weight_decay": WD if dec else 0.0, "lr": lr * s, "lr_scale": s} for (s, dec), ps in by.items()]


def tiny():
    cfg = O.tiny_config(drop_path_rate=0.0)
    return cfg, O.key_seeded_state_dict(cfg, seed=3), tuple(t.to(DEV) for t in O.synthetic_batch(cfg, 4, seed=77))


def params_of(m):
    return {n: p.detach().clone() for n, p in m.named_parameters()}


def run_torch(cfg, sd, lo, hi, scales, steps):
    m = build(cfg, sd, train=True)
    opt = torch.optim.AdamW(torch_groups(m, scales, LR), lr=LR, betas=BETAS)
    out = [params_of(m)]
    for _ in range(steps):
        opt.zero_grad()
        _, loss, _ = m(lo, hi)
        loss.backward()
        opt.step()
        out.append(params_of(m))
    return out


def run_fused(cfg, sd, lo, hi, scales, steps, with_arg=True):
    m = build(cfg, sd, train=True)
    tr = Trainer(m, 4, lr=LR, betas=BETAS, weight_decay=WD, **(dict(lr_scales=scales) if with_arg else {}))
    tr.load_batch(lo, hi)
    out = [params_of(m)]
    for _ in range(steps):
        tr.step()
        out.append(params_of(m))
    return out


def worst_update_difference(a, b, k):
    """max over tensors of |(a_k - a_0) - (b_k - b_0)| / |b_k - b_0| (L2): the parameters' own size cancels out."""
    worst = 0.0
    for n in a[0]:
        da, db = (a[k][n] - a[0][n]).double(), (b[k][n] - b[0][n]).double()
        if float(db.norm()) == 0.0:
            assert float(da.norm()) == 0.0, n
            continue
        worst = max(worst, float((da - db).norm() / db.norm()))
    return worst


def test_three_steps_against_torch_adamw_on_the_module_path():
    """The tiny model of fixture g3 (no DropPath), batch 4, the same seeded weights and batch on both sides: three steps of the
    module behind autograd with torch.optim.AdamW over groups carrying lr * lr_scale, against three steps of
    Trainer(lr_scales=layer_decay_scales(model)).  Figure: the largest per-tensor relative L2 difference of the three-step
    UPDATE p3 - p0.  Its bound is twice the same figure with every scale at 1.0 -- a comparison that runs only code the parent
    commit has (the scaled rates change the size of the update, not the arithmetic); it is measured in this test, on the same
    device, before the scaled comparison.  Measured on an MI355X: all ones 3.05e-02, with the scales 1.63e-02 (after one
    step with the scales: 1.7e-05); worst |update ratio / scale - 1| after step 1: 9.7e-05.
    After step 1 m / sqrt(v) is the gradient's sign and both runs hold the same gradients bit for bit, so every tensor's update
    is its rate: |update with scales| / |update without| must be the tensor's scale within the same bound."""
    cfg, sd, (lo, hi) = tiny()
    m0 = build(cfg, sd, train=True)
    scales = layer_decay(m0)
    ones = {n: 1.0 for n in scales}
    assert len(set(scales.values())) >= 3
    base = worst_update_difference(run_fused(cfg, sd, lo, hi, ones, 3, with_arg=False), run_torch(cfg, sd, lo, hi, ones, 3), 3)
    fused, ref = run_fused(cfg, sd, lo, hi, scales, 3), run_torch(cfg, sd, lo, hi, scales, 3)
    got = worst_update_difference(fused, ref, 3)
    print(f"worst per-tensor relative update difference after 3 steps: all ones {base:.3e}, with layer-decay scales {got:.3e}; "
          f"after 1 step with scales {worst_update_difference(fused, ref, 1):.3e}")
    assert base > 0.0
    tol = 2.0 * base
    assert got <= tol, (got, tol)
    plain = run_fused(cfg, sd, lo, hi, ones, 1, with_arg=False)
    worst_ratio = 0.0
    for n, s in scales.items():
        du, d1 = float((fused[1][n] - fused[0][n]).double().norm()), float((plain[1][n] - plain[0][n]).double().norm())
        if d1 == 0.0:
            assert du == 0.0, n
            continue
        worst_ratio = max(worst_ratio, abs(du / d1 / f32(s) - 1.0))
    print(f"worst |update ratio / scale - 1| after step 1: {worst_ratio:.3e}")
    assert worst_ratio <= tol, (worst_ratio, tol)


def test_import_export_round_trip_and_checkpoint():
    """torch.optim.AdamW over layer_decay_scales groups, one torch step through the module, import_torch_optimizer, one fused step
    audited at t = 2 with every group at its own rate; export_torch_optimizer leaves lr * lr_scale in every group and refuses
    groups that mix scales; state_dict() -> a new Trainer -> load_state_dict() reproduces the next step bit for bit; a dictionary
    without the scales loads as all ones."""
    cfg, sd, (lo, hi) = tiny()
    ma = build(cfg, sd, train=True)
    scales = layer_decay(ma)
    oa = torch.optim.AdamW(torch_groups(ma, scales, LR), lr=LR, betas=BETAS)
    oa.zero_grad()
    ma(lo, hi)[1].backward()
    oa.step()
    tr = Trainer(ma, 4, lr=1.0, betas=(0.5, 0.5), weight_decay=0.3)        # every hyper-parameter must come from the import
    tr.import_torch_optimizer(oa)
    assert tr.t == 1 and tr.lr == LR and tuple(tr.betas) == BETAS and tr.wd == WD
    assert tr.lr_scales == {n: f32(s) for n, s in scales.items()} and tr._lr_table is not None
    tr.load_batch(lo, hi)
    v, _, _ = audited_steps_scaled(tr, 1, "nonzero", scales, lr_at, t0=1)
    assert tr.t == 2
    assert v == [], "\n".join(v[:40])
    # without lr_scale in the groups the scales come from the groups' own rates
    ob = torch.optim.AdamW([{k: g[k] for k in ("params", "weight_decay", "lr")} for g in torch_groups(ma, scales, LR)], lr=LR, betas=BETAS)
    tr.export_torch_optimizer(ob)
    for g in ob.param_groups:
        g.pop("lr_scale", None)
    probe = Trainer(ma, 4)
    probe.import_torch_optimizer(ob)
    assert probe.lr == tr.lr and probe.t == 2
    assert all(abs(probe.lr_scales[n] - tr.lr_scales[n]) <= 2.0 ** -22 * tr.lr_scales[n] for n in scales)
    del probe
    # export
    oc = torch.optim.AdamW(torch_groups(ma, scales, 1.0), lr=1.0)
    tr.export_torch_optimizer(oc)
    assert tr.lr == lr_at(2)
    for g in oc.param_groups:
        assert g["lr"] == tr.lr * g["lr_scale"] and tuple(g["betas"]) == BETAS
        assert all(float(oc.state[p]["step"]) == 2.0 for p in g["params"])
    assert sorted({g["lr_scale"] for g in oc.param_groups}) == sorted({f32(s) for s in scales.values()})
    two = torch.optim.AdamW([{"params": [p for p in ma.parameters() if p.ndim <= 1], "weight_decay": 0.0},
                             {"params": [p for p in ma.parameters() if p.ndim > 1], "weight_decay": WD}], lr=1.0)
    with pytest.raises(ValueError, match="mixes"):
        tr.export_torch_optimizer(two)
    # the Trainer's own checkpoint
    sd_model, sd_opt = {k: t.clone() for k, t in ma.state_dict().items()}, tr.state_dict()
    assert sd_opt["lr_scales"] == tr.lr_scales
    mb = build(cfg, sd_model, train=True)
    tb = Trainer(mb, 4)
    tb.load_state_dict(sd_opt)
    assert tb.lr_scales == tr.lr_scales and tb._lr_table is not None and tb.t == 2
    tb.load_batch(lo, hi)
    tr.step(lr=lr_at(3)); tb.step(lr=lr_at(3))
    assert _same_bits(_state(tr), _state(tb)) == []
    old = {k: v for k, v in sd_opt.items() if k != "lr_scales"}              # saved before the scales existed
    tb.load_state_dict(old)
    assert set(tb.lr_scales.values()) == {1.0} and tb._lr_table is None and tb._segments is None
    # the Trainer that has captured and stepped WITH the scales plans and captures again: a step without them (t = 3 again),
    # then with the scales set back (t = 4), each audited at the rates in force
    assert tb.t == 2
    v, _, _ = audited_steps_scaled(tb, 1, "nonzero", {}, lr_at, t0=2)
    assert tb.t == 3 and tb._segments is not None
    assert v == [], "\n".join(v[:40])
    tb.set_lr_scales(scales)
    assert tb._lr_table is not None and tb._segments is None
    v, _, _ = audited_steps_scaled(tb, 1, "nonzero", scales, lr_at, t0=3)
    assert tb.t == 4
    assert v == [], "\n".join(v[:40])
    with pytest.raises(KeyError):
        Trainer(mb, 4, lr_scales={"no.such.parameter": 0.5})
    with pytest.raises(ValueError, match="distinct learning-rate scales"):
        from tulip_amd.trainer import layer_decay_scales
        Trainer(mb, 4, lr_scales=layer_decay_scales(mb, 0.75, 1))


def test_bench_configuration_with_layer_decay_scales():
    """KITTI tulip_base, batch 8, layer_decay_scales(model) (18 groups, 0.75**17 .. 1.0), the default captured Trainer: one
    step, audited like test_bench_configuration_every_update_is_adamw (the gradient is known where it was stored)."""
    m = make()
    scales = layer_decay(m)
    assert len(set(scales.values())) == 18
    tr = Trainer(m, 8, lr_scales=scales)
    tr.load_batch(*batch(m, 8))
    v, stats, _ = audited_steps_scaled(tr, 1, "nonzero", scales, lr_at)
    assert tr.fuse_adamw and tr.fused_adamw_params > 0 and tr.step_form == "one_graph"
    seen = sites_seen(tr, scales)
    assert {"writeout", "fold"} <= set(seen) and all(len(s) >= 2 for s in seen.values()), seen
    print(f"worst p error {stats.get('p_ulps', 0):.3g} ulp, worst v residual {stats.get('v_frac', 0):.3g} of its bound")
    assert v == [], "\n".join(v[:40])

"""The selectable training loss on the GPU, TULIP(loss="l2" | "berhu"): the four kernels of csrc/loss.hip against the host definition
(tulip_amd/loss.py), their edge values, the model's loss and parameter gradients against the oracle's autograd of the same
definition, and the Trainer's step forms.  Everything on the tiny model (8x256 -> 32x256, depths (2, 2), embed_dim 48)."""
import math

import numpy as np
import pytest
import torch

from oracle import tulip_oracle as O
from tulip_amd import _lib, ops
from tulip_amd import loss as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN, INF = float("nan"), float("inf")
KINDS = ("l2", "berhu")
# one element; a tail without a float4 group; one short of / one past a workgroup's 256 lanes (a float4 group + scalar tail: 63 / 64
# groups + 3 / 1 tail elements); 257 workgroups' worth of float4 groups + a tail (more than one workgroup, a ragged last one)
SIZES = (1, 3, 255, 257, 1024 * 256 + 5)
PEAK = 12.0                     # |d| of the planted extreme element: above every |randn - randn| difference of these sizes


def bufs():
    z = lambda n: torch.zeros(n, dtype=torch.float32, device=DEV)
    return dict(stats=z(4 * _lib.LOSS_BLOCKS_MAX), vpart=z(_lib.LOSS_BLOCKS_MAX), c=z(1), losses=z(2))


def inputs(n, variant, seed=0):
    """seeded fp32 randn (pred, target) with the element of largest |d| planted first, last (the scalar tail when n % 4 != 0), or with
    a negative sign in the middle"""
    rng = np.random.default_rng(1000 * seed + n)
    pred, target = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    i = {"first": 0, "last": n - 1, "negative": n // 2}[variant]
    pred[i] = target[i] + np.float32(-PEAK if variant == "negative" else PEAK)
    d = pred - target
    assert int(np.argmax(np.abs(d))) == i and (d[i] < 0) == (variant == "negative")
    return pred, target


def run(kind, pred, target, log_transform=0, gscale_dev=None, gscale=1.0, b=None):
    """the step's launch order: stats -> bwd -> value (berhu) -> final; (dpred, losses, C) on the host"""
    b = b or bufs()
    n = pred.numel()
    dpred = torch.full_like(pred, 7.0)
    ops.loss_stats(pred, target, b["stats"], n, log_transform)
    ops.loss_bwd(kind, pred, target, b["stats"], gscale_dev, gscale, dpred, b["c"], n)
    if kind == "berhu":
        ops.loss_value(pred, target, b["stats"], b["vpart"], n)
    ops.loss_final(kind, b["stats"], b["vpart"], b["losses"], n, log_transform)
    torch.cuda.synchronize()
    return dpred.cpu().numpy(), b["losses"].cpu().numpy(), b["c"].cpu().numpy()[0]


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------- 1. kernels vs the definition
@pytest.mark.parametrize("variant", ["first", "last", "negative"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_kernels_match_the_host_definition(kind, n, variant):
    """dpred elementwise at rtol 1e-6 (at most six fp32 roundings: p - t, the constant 0.2f, 0.2f * max, d / C, g / n, the product
    ~ 3.6e-7), C exactly the float32 product, both losses at rtol 1e-5 (positive terms, short per-thread sums, the fold in double)."""
    p_h, t_h = inputs(n, variant)
    pred, target = torch.from_numpy(p_h).to(DEV), torch.from_numpy(t_h).to(DEV)
    dpred, losses, c = run(kind, pred, target)
    print(f"{kind} n={n} {variant}: losses {losses.tolist()} C {c!r}")
    np.testing.assert_allclose(dpred, L.loss_grad(kind, p_h, t_h), rtol=1e-6, atol=0)
    np.testing.assert_allclose(losses[0], L.loss_value(kind, p_h, t_h), rtol=1e-5, atol=0)
    np.testing.assert_allclose(losses[1], L.pixel_loss(p_h, t_h, False), rtol=1e-5, atol=0)
    if kind == "berhu":
        want_c = np.float32(0.2) * np.float32(np.max(np.abs(p_h - t_h)))
        assert bits(c) == bits(want_c) == bits(L.berhu_c32(p_h, t_h)), (c, want_c)
        assert c == np.float32(0.2) * np.float32(PEAK)
    # gscale from device memory and as an argument, 0.25 (a power of two: the same roundings, a quarter of the value)
    gdev = torch.full((1,), 0.25, dtype=torch.float32, device=DEV)
    for kw in (dict(gscale_dev=gdev, gscale=123.0), dict(gscale=0.25)):
        dq, lq, _ = run(kind, pred, target, **kw)
        np.testing.assert_allclose(dq, L.loss_grad(kind, p_h, t_h, gscale=0.25), rtol=1e-6, atol=0)
        assert np.array_equal(bits(dq), bits(np.float32(0.25) * dpred)) and np.array_equal(bits(lq), bits(losses))
    # log_transform changes losses[1] only
    dl, ll, cl = run(kind, pred, target, log_transform=1)
    assert np.array_equal(bits(dl), bits(dpred)) and bits(ll[0]) == bits(losses[0]) and bits(cl) == bits(c)
    np.testing.assert_allclose(ll[1], L.pixel_loss(p_h, t_h, True), rtol=1e-5, atol=0)
    assert n < 255 or ll[1] != losses[1]
    # the same bits run to run
    d2, l2, c2 = run(kind, pred, target)
    assert np.array_equal(bits(d2), bits(dpred)) and np.array_equal(bits(l2), bits(losses)) and bits(c2) == bits(c)


@pytest.mark.parametrize("kind", KINDS + ("l1",))
def test_unaligned_pointers_take_the_scalar_route(kind):
    """pred / target / dpred one float past a 16-byte boundary: no float4 access, the same results as the aligned call."""
    n = 257 + 1024
    p_h, t_h = inputs(n, "last", seed=3)
    pred, target = torch.from_numpy(p_h).to(DEV), torch.from_numpy(t_h).to(DEV)
    want_d, want_l, want_c = run(kind, pred, target, log_transform=1)
    np.testing.assert_allclose(want_d, L.loss_grad(kind, p_h, t_h), rtol=1e-6, atol=0)
    np.testing.assert_allclose(want_l[0], L.loss_value(kind, p_h, t_h), rtol=1e-5, atol=0)
    hold = [torch.zeros(n + 4, dtype=torch.float32, device=DEV) for _ in range(3)]
    po, to, do = (h[1:1 + n] for h in hold)
    assert po.data_ptr() % 16 == 4
    po.copy_(pred)
    to.copy_(target)
    b = bufs()
    ops.loss_stats(po, to, b["stats"], n, 1)
    ops.loss_bwd(kind, po, to, b["stats"], None, 1.0, do, b["c"], n)
    if kind == "berhu":
        ops.loss_value(po, to, b["stats"], b["vpart"], n)
    ops.loss_final(kind, b["stats"], b["vpart"], b["losses"], n, 1)
    torch.cuda.synchronize()
    assert np.array_equal(bits(do.cpu().numpy()), bits(want_d)) and bits(b["c"].cpu().numpy()[0]) == bits(want_c)
    got_l = b["losses"].cpu().numpy()                                                       # (another partition of the sums)
    np.testing.assert_allclose(got_l[0], L.loss_value(kind, p_h, t_h), rtol=1e-5, atol=0)
    np.testing.assert_allclose(got_l[1], L.pixel_loss(p_h, t_h, True), rtol=1e-5, atol=0)
    assert hold[2][0].item() == 0.0 and not hold[2][1 + n:].any().item()                    # nothing written outside dpred


# ---------------------------------------------------------------------------------------------------- 2. edge values
@pytest.mark.parametrize("kind", KINDS)
def test_edge_values(kind):
    n = 257
    p_h, t_h = inputs(n, "first", seed=5)
    pred = torch.from_numpy(p_h).to(DEV)
    # pred == target: zeros (berHu's C == 0, where the reference's formula is 0/0)
    dpred, losses, c = run(kind, pred, pred.clone())
    assert not dpred.any() and losses[0] == 0.0 and losses[1] == 0.0 and c == 0.0
    # one NaN in the last element (the scalar tail): a NaN loss, a NaN C, a NaN in that gradient element
    bad = torch.from_numpy(t_h).to(DEV)
    bad[-1] = NAN
    dpred, losses, c = run(kind, pred, bad)
    assert math.isnan(losses[0]) and math.isnan(dpred[-1])
    if kind == "berhu":
        assert math.isnan(c)
    else:
        assert np.isfinite(dpred[:-1]).all()
    # ... and in a float4 group of another wave: fmaxf would have dropped it on the way to C
    bad = torch.from_numpy(t_h).to(DEV)
    bad[130] = NAN
    dpred, losses, c = run(kind, pred, bad)
    assert math.isnan(losses[0]) and math.isnan(dpred[130]) and (kind != "berhu" or math.isnan(c))
    # one +Inf: a non-finite loss
    bad = torch.from_numpy(t_h).to(DEV)
    bad[7] = INF
    dpred, losses, c = run(kind, pred, bad)
    assert not math.isfinite(losses[0]) and not math.isfinite(dpred[7])


def test_bad_arguments_return_err_arg():
    lib = _lib.load()
    x = torch.zeros(4096, dtype=torch.float32, device=DEV)
    a = x.data_ptr()
    assert lib.tulip_loss_bwd(3, a, a, a, None, 1.0, a, a, 8, None) == -1 and lib.tulip_loss_final(-1, a, a, a, 8, 0, None) == -1
    assert lib.tulip_loss_stats(a, a, a, 0, 0, None) == -1 and lib.tulip_loss_value(a, a, a, a, -3, None) == -1
    assert lib.tulip_loss_stats(a, None, a, 8, 0, None) == -1 and lib.tulip_loss_bwd(_lib.LOSS_BERHU, a, a, None, None, 1.0, a, a, 8, None) == -1
    assert lib.tulip_loss_bwd(_lib.LOSS_L2, a, a, None, None, 1.0, None, None, 8, None) == -1
    with pytest.raises(_lib.TulipHipError, match="TULIP_ERR_ARG"):
        ops.loss_final("berhu", x, None, x, 8, 0)
    with pytest.raises(KeyError):
        ops.loss_bwd("huber", x, x, x, None, 1.0, x, x, 8)
    torch.cuda.synchronize()
    assert not x.any().item()


# ---------------------------------------------------------------------------------------------------- 3. model vs the oracle
MODEL_CASES = {
    # name: (config overrides, batch, weight seed, data seed)
    "pixel_shuffle": (dict(), 2, 11, 111),
    "final_expanding": (dict(pixel_shuffle=False), 3, 12, 112),
    "in_chans2": (dict(in_chans=2), 2, 13, 113),
}
_oracle_cache = {}


def oracle_grads(case, kind, lowp):
    """(loss, {name: grad}) of the oracle's forward with the loss of tulip_amd/loss.py written in torch, by autograd; computed once"""
    key = (case, kind, lowp)
    if key not in _oracle_cache:
        cfg, sd, lo, hi = model_case(case)
        leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
        full = dict(sd)
        full.update(leaves)
        pred = O.tulip_forward(full, cfg, lo, None, lowp=lowp)
        loss = L.torch_loss(kind, pred, hi)
        loss.backward()
        _oracle_cache[key] = (loss.item(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()},
                              L.pixel_loss(pred.detach().numpy(), hi.numpy(), cfg.log_transform))
    return _oracle_cache[key]


def model_case(case):
    kw, B, wseed, dseed = MODEL_CASES[case]
    cfg = O.tiny_config(drop_path_rate=0.0, **kw)
    return cfg, O.key_seeded_state_dict(cfg, seed=wseed), *O.synthetic_batch(cfg, B, seed=dseed)


def build(cfg, sd, loss, train=False):
    from functools import partial
    import torch.nn as nn
    from tulip_amd.model import tulip as T
    kw = {} if loss is None else dict(loss=loss)
    m = T.TULIP(img_size=cfg.img_size, target_img_size=cfg.target_img_size, patch_size=cfg.patch_size, in_chans=cfg.in_chans,
                embed_dim=cfg.embed_dim, window_size=list(cfg.window_size), depths=cfg.depths, num_heads=cfg.num_heads,
                mlp_ratio=cfg.mlp_ratio, drop_path_rate=cfg.drop_path_rate, norm_layer=partial(nn.LayerNorm, eps=cfg.ln_eps),
                pixel_shuffle=cfg.pixel_shuffle, circular_padding=cfg.circular_padding, log_transform=cfg.log_transform,
                patch_unmerging=cfg.patch_unmerging, **kw)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    m.train(train)
    return m


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def device_grads(case, kind):
    cfg, sd, lo, hi = model_case(case)
    m = build(cfg, sd, kind)
    pred, loss, pix = m(lo.to(DEV), hi.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    m.last_pred = pred.detach().cpu()
    return m, loss.item(), pix.item(), {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_model_loss_and_gradients_vs_oracle(case, kind):
    """model(lo, hi) and loss.backward() through the autograd bridge against the oracle's autograd of the same loss, at the
    tolerances tests/test_model_gpu.py::test_backup_window_gradients_vs_oracle uses for L1: loss 1e-3 relative, gradient rel_l2
    1.5e-2 against the fp32 oracle and 1e-2 against the low-precision one (bias tables 1e-1 and 5e-2)."""
    ol, og, opix = oracle_grads(case, kind, False)
    _, olp, _ = oracle_grads(case, kind, True)
    m, loss, pix, g = device_grads(case, kind)
    worst = max((rel_l2(g[n], og[n]), n) for n in g if not n.endswith("relative_position_bias_table"))
    worst_lp = max((rel_l2(g[n], olp[n]), n) for n in g if not n.endswith("relative_position_bias_table"))
    print(f"{case} {kind}: loss {loss!r} oracle {ol!r} (rel {abs(loss - ol) / ol:.2e}); pixel {pix!r} oracle {opix!r}; "
          f"worst rel_l2 vs fp32 {worst}, vs lowp {worst_lp}")
    assert abs(loss - ol) <= 1e-3 * ol
    assert abs(pix - opix) <= 1e-3 * opix                                   # pixel_loss keeps its meaning: the L1 metric
    for n in g:
        table = n.endswith("relative_position_bias_table")
        assert rel_l2(g[n], og[n]) <= (1e-1 if table else 1.5e-2), n
        assert rel_l2(g[n], olp[n]) <= (5e-2 if table else 1.0e-2), n
    if kind == "berhu":
        cfg, sd, lo, hi = model_case(case)               # C as the backward formed it from this forward's pred, on the device
        want_c = np.float32(0.2) * np.float32((m.last_pred - hi).abs().max().item())
        assert bits(m.engine().plan(lo.shape[0]).loss_c.cpu().numpy()[0]) == bits(want_c)


def test_berhu_gradient_is_not_the_l1_gradient():
    """The test must tell the losses apart: on this seed the oracle alone separates the berHu and the L1 gradient of
    decoder_pred.weight by more than 10 % rel_l2, and so does the device."""
    case = "pixel_shuffle"
    _, og_b, _ = oracle_grads(case, "berhu", False)
    _, og_1, _ = oracle_grads(case, "l1", False)
    assert rel_l2(og_b["decoder_pred.weight"], og_1["decoder_pred.weight"]) > 0.10
    _, _, _, gb = device_grads(case, "berhu")
    _, _, _, g1 = device_grads(case, "l1")
    _, _, _, g2 = device_grads(case, "l2")
    assert rel_l2(gb["decoder_pred.weight"], g1["decoder_pred.weight"]) > 0.10
    assert rel_l2(g2["decoder_pred.weight"], g1["decoder_pred.weight"]) > 0.10
    assert rel_l2(g1["decoder_pred.weight"], og_1["decoder_pred.weight"]) <= 1.5e-2


def test_no_grad_forward_returns_the_chosen_loss():
    """model(x, target) under no_grad (the evaluation call): the same loss values as the differentiable call, nothing else moves"""
    case, kind = "pixel_shuffle", "berhu"
    cfg, sd, lo, hi = model_case(case)
    m = build(cfg, sd, kind)
    with torch.no_grad():
        _, loss, pix = m(lo.to(DEV), hi.to(DEV))
    _, loss_g, pix_g, _ = device_grads(case, kind)
    assert bits(loss.item()) == bits(loss_g) and bits(pix.item()) == bits(pix_g)
    ol, _, _ = oracle_grads(case, kind, False)
    assert abs(loss.item() - ol) <= 1e-3 * ol


# ---------------------------------------------------------------------------------------------------- 4. Trainer
def trainer_run(loss, steps=3, batch=2, **kw):
    from tulip_amd.trainer import Trainer
    cfg = O.tiny_config(drop_path_rate=0.0)
    sd = O.key_seeded_state_dict(cfg, seed=3)
    m = build(cfg, sd, loss, train=True)
    tr = Trainer(m, batch, lr=5e-4, **kw)
    lo, hi = (t.to(DEV) for t in O.synthetic_batch(cfg, batch, seed=77))
    tr.load_batch(lo, hi)
    losses = [tr.step().clone() for _ in range(steps)]
    torch.cuda.synchronize()
    return tr, torch.stack(losses).cpu().numpy(), tr.eng.params.flat.clone().cpu().numpy(), (lo, hi)


def test_trainer_graph_and_eager_steps_are_bit_identical():
    """The project's standing rule for the two step forms, with loss="berhu": the same losses and the same parameters, bit for bit."""
    tr_g, lg, pg, _ = trainer_run("berhu", use_graph=True)
    tr_e, le, pe, _ = trainer_run("berhu", use_graph=False)
    print("berhu trainer losses", lg.tolist(), "C", tr_g.loss_c.item())
    assert np.isfinite(lg).all() and lg[-1, 0] < lg[0, 0]
    assert np.array_equal(bits(lg), bits(le)) and np.array_equal(bits(pg), bits(pe))
    assert bits(tr_g.loss_c.item()) == bits(tr_e.loss_c.item()) and tr_g.loss_c.item() > 0.0
    # ... and berHu is not L1 here either
    _, l1, p1, _ = trainer_run("l1", use_graph=True)
    assert not np.array_equal(bits(l1[:, 0]), bits(lg[:, 0])) and not np.array_equal(bits(p1), bits(pg))
    np.testing.assert_allclose(l1[0, 1], lg[0, 1], rtol=1e-5)                  # the first step's pixel_loss: the same L1 metric


def test_trainer_l2_and_accumulation_run():
    tr, l2, p2, _ = trainer_run("l2", use_graph=True)
    assert np.isfinite(l2).all() and l2[-1, 0] < l2[0, 0]
    with pytest.raises(AttributeError):
        tr.loss_c
    for kind in KINDS:
        for use_graph in (True, False):
            tr, la, pa, _ = trainer_run(kind, steps=4, accum_iter=2, use_graph=use_graph)
            assert np.isfinite(la).all() and np.isfinite(pa).all()
            # the resident batch twice per optimizer step: both micro-steps of the first window report the same loss
            assert bits(la[0, 0]) == bits(la[1, 0]) and la[2, 0] < la[0, 0]


@pytest.mark.parametrize("use_graph", [True, False])
def test_trainer_skips_a_nonfinite_target(use_graph):
    """skip_nonfinite with loss="berhu": one NaN in the target reaches C, every gradient and the norm; the step is skipped, the
    parameters stay, and the following clean step is applied."""
    tr, _, _, (lo, hi) = trainer_run("berhu", steps=2, use_graph=use_graph, skip_nonfinite=True)
    assert int(tr.last_step_skipped.item()) == 0 and tr.applied_steps == 2
    before = tr.eng.params.flat.clone()
    bad = hi.clone()
    bad[1, 0, 5, 9] = NAN
    losses = tr.step(lo, bad).clone()
    torch.cuda.synchronize()
    assert int(tr.last_step_skipped.item()) != 0 and tr.applied_steps == 2 and tr.skipped_steps == 1
    assert math.isnan(losses[0].item()) and math.isnan(tr.loss_c.item())
    assert torch.equal(tr.eng.params.flat.view(torch.int32), before.view(torch.int32))
    losses = tr.step(lo, hi).clone()
    torch.cuda.synchronize()
    assert int(tr.last_step_skipped.item()) == 0 and tr.applied_steps == 3 and math.isfinite(losses[0].item())
    assert not torch.equal(tr.eng.params.flat.view(torch.int32), before.view(torch.int32))
    assert torch.isfinite(tr.eng.params.flat).all().item()


def test_explicit_l1_is_the_default_constructor():
    _, la, pa, _ = trainer_run("l1", use_graph=True)
    _, lb, pb, _ = trainer_run(None, use_graph=True)
    assert np.array_equal(bits(la), bits(lb)) and np.array_equal(bits(pa), bits(pb))
    with pytest.raises(ValueError, match="sharded"):
        from tulip_amd.trainer import Trainer
        cfg = O.tiny_config(drop_path_rate=0.0)
        Trainer(build(cfg, O.key_seeded_state_dict(cfg, seed=3), "l2", train=True), 2, exchange="sharded")

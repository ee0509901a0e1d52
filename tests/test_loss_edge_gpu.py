"""The edge term of the training loss on the GPU, TULIP(loss_edge_weight=...): the tulip_loss_edge_* kernels of csrc/loss.hip against
the host definition (tulip_amd/loss.py) at the shapes where the halo logic can break, bit for bit where the arithmetic is fixed;
the masked forms on the hole patterns of tests/test_loss_mask_gpu.py; plane isolation; the model's loss and parameter gradients
against the oracle's autograd of the same definition; and the Trainer's step forms.  Everything on the tiny model (8x256 -> 32x256,
depths (2, 2), embed_dim 48).  Tolerances are those of tests/test_loss_gpu.py."""
import math

import numpy as np
import pytest
import torch

import test_loss_edge_cpu as C
import test_loss_gpu as G
import test_loss_mask_gpu as M
from oracle import tulip_oracle as O
from tulip_amd import _lib, ops
from tulip_amd import loss as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN, INF = float("nan"), float("inf")
KINDS = ("l1", "l2", "berhu")
VMIN = 0.0
WEIGHT = 0.5
bits = G.bits
# (B, C, H, W).  One pixel; one row; one column; the plane that is all border; adjacent planes and samples with W % 4 != 0; the
# 8 x 128 tile -1 / +1 each way (one tile with a ragged edge, four tiles of which three are slivers), two planes of the latter;
# more tiles (4 * 32 * 9 = 1152) than TULIP_LOSS_BLOCKS_MAX with ragged edges both ways: the stride loop, 1.1e6 elements
SHAPES = ((1, 1, 1, 1), (1, 1, 1, 5), (1, 1, 5, 1), (1, 1, 3, 3), (2, 3, 5, 7), (1, 1, 7, 127), (1, 1, 7, 129), (1, 1, 9, 127),
          (2, 1, 9, 129), (2, 2, 250, 1100))
MASK_SHAPES = ((2, 3, 5, 7), (1, 2, 9, 129), (1, 1, 7, 127))
ids = lambda s: "x".join(map(str, s))


def make(shape, what, seed=0):
    """(pred, target, base gradient) in float32: seeded randn, or -- "int" -- integer-valued with d = pred - target in [-3, 3]"""
    rng = np.random.default_rng(100 * seed + int(np.prod(shape)) + shape[-1])
    if what == "int":
        target = rng.integers(-2, 3, shape).astype(np.float32)
        pred = target + rng.integers(-3, 4, shape).astype(np.float32)
    else:
        pred, target = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    return pred, target, (rng.standard_normal(shape) / np.prod(shape)).astype(np.float32)


def run(p_h, t_h, base_h, weight=WEIGHT, gscale_dev=None, gscale=1.0, valid_min=None, base_loss=1.25, offset=0):
    """stats -> final -> bwd as the step issues them (masked: behind tulip_loss_stats_m, whose counts they read), from a base
    gradient already in dpred and a base loss already in losses[0].  offset: the three arrays start that many floats past a 16-byte
    boundary.  (dpred, edge_out, losses, partials) on the host; nothing is written around dpred."""
    B, C, H, W = p_h.shape
    n = p_h.size

    def put(a):
        hold = torch.zeros(n + 8, dtype=torch.float32, device=DEV)
        v = hold[offset:offset + n].view(p_h.shape)
        v.copy_(torch.from_numpy(a))
        assert v.data_ptr() % 16 == 4 * offset
        return hold, v
    (_, pred), (_, target), (dhold, dpred) = put(p_h), put(t_h), put(base_h)
    part = torch.full((_lib.LOSS_BLOCKS_MAX,), -3.0, dtype=torch.float32, device=DEV)
    edge = torch.full((1,), -3.0, dtype=torch.float32, device=DEV)
    losses = torch.tensor([base_loss, 3.0], dtype=torch.float32, device=DEV)
    kw = {}
    if valid_min is not None:
        counts = torch.full((_lib.LOSS_BLOCKS_MAX,), 12345, dtype=torch.int32, device=DEV)
        stats = torch.zeros(4 * _lib.LOSS_BLOCKS_MAX, dtype=torch.float32, device=DEV)
        ops.loss_stats_m(pred, target, stats, n, 0, C, H * W, valid_min, counts)
        kw = dict(mask=(C, valid_min), counts=counts)
    dims = (B * C, H, W)
    ops.loss_edge_stats(pred, target, part, *dims, **kw)
    ops.loss_edge_final(part, edge, losses, weight, *dims, **kw)
    ops.loss_edge_bwd(pred, target, gscale_dev, gscale, weight, dpred, *dims, **kw)
    torch.cuda.synchronize()
    assert not dhold[:offset].any().item() and not dhold[offset + n:].any().item()
    nb = ops.loss_edge_blocks(*dims)
    part = part.cpu().numpy()
    assert (part[nb:] == -3.0).all()
    return dpred.cpu().numpy(), edge.cpu().numpy()[0], losses.cpu().numpy(), part[:nb]


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------- 1. kernels vs the definition
@pytest.mark.parametrize("what", ["randn", "int"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_kernels_match_the_host_definition(shape, what):
    """dpred bit for bit (the float32 arithmetic is fixed: tulip_amd/loss.py, edge_grad32).  Integer input: every workgroup's sum is an
    integer below 2^24, so edge_out and losses[0] are edge_total32's bits; randn input: rtol 1e-5, the sums' tolerance of
    tests/test_loss_gpu.py (positive terms, short per-thread sums, the fold in double)."""
    p_h, t_h, base = make(shape, what)
    got = run(p_h, t_h, base)
    dpred, edge, losses, part = got
    print(f"{shape} {what}: edge {edge!r} losses {losses.tolist()} workgroups {part.size}")
    assert part.size == min(_lib.LOSS_BLOCKS_MAX, shape[0] * shape[1] * -(-shape[2] // 8) * -(-shape[3] // 128))
    assert np.array_equal(bits(dpred), bits(L.edge_grad32(p_h, t_h, base, WEIGHT)))
    if max(shape[2:]) > 1:
        assert not np.array_equal(bits(dpred), bits(base))                                        # the term does something
    want_e, want_t = L.edge_total32(p_h, t_h, np.float32(1.25), WEIGHT)
    if what == "int":
        assert part.max(initial=0.0) < 2 ** 24 and np.array_equal(part, np.round(part))
        assert bits(edge) == bits(want_e) and bits(losses[0]) == bits(want_t), (edge, want_e, losses[0], want_t)
    else:
        np.testing.assert_allclose(edge, L.edge_value(p_h, t_h), rtol=1e-5, atol=0)
        np.testing.assert_allclose(losses[0], 1.25 + WEIGHT * L.edge_value(p_h, t_h), rtol=1e-5, atol=0)
        assert bits(losses[0]) == bits(np.float32(1.25) + np.float32(WEIGHT) * edge)              # a multiply, then an add
    assert losses[1] == 3.0                                                                       # pixel_loss is not touched
    # gscale from device memory and as an argument: the same bits as the host's
    gdev = torch.full((1,), 0.3, dtype=torch.float32, device=DEV)
    a = run(p_h, t_h, base, gscale_dev=gdev, gscale=123.0)
    b = run(p_h, t_h, base, gscale=0.3)
    assert same(a, b) and np.array_equal(bits(a[0]), bits(L.edge_grad32(p_h, t_h, base, WEIGHT, 0.3)))
    assert same(a[1:], got[1:])                                                                   # gscale is the gradient's alone
    # one float past a 16-byte boundary, and a second run: the same bits
    assert same(run(p_h, t_h, base, offset=1), got) and same(run(p_h, t_h, base), got)
    # another weight, the value's base loss
    c = run(p_h, t_h, base, weight=2.0, base_loss=0.0)
    assert np.array_equal(bits(c[0]), bits(L.edge_grad32(p_h, t_h, base, 2.0))) and bits(c[1]) == bits(edge)
    assert bits(c[2][0]) == bits(np.float32(0.0) + np.float32(2.0) * edge)


def test_nonfinite_inputs():
    """A NaN response has sign 0 in k and makes the edge sum, and losses[0], NaN; elsewhere the gradient stays finite."""
    p_h, t_h, base = make((1, 2, 9, 129), "randn", seed=3)
    p_h[0, 1, 4, 64] = NAN
    dpred, edge, losses, _ = run(p_h, t_h, base)
    assert math.isnan(edge) and math.isnan(losses[0]) and losses[1] == 3.0
    assert np.isfinite(dpred).all() and np.array_equal(bits(dpred), bits(L.edge_grad32(p_h, t_h, base, WEIGHT)))
    p_h[0, 1, 4, 64] = INF
    dpred, edge, losses, _ = run(p_h, t_h, base)
    assert not math.isfinite(edge) and np.array_equal(bits(dpred), bits(L.edge_grad32(p_h, t_h, base, WEIGHT)))


def test_bad_arguments_return_err_arg():
    x = torch.zeros(4096, dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.TulipHipError, match="TULIP_ERR_ARG"):
        ops.loss_edge_stats(x, x, x, 0, 4, 4)
    with pytest.raises(_lib.TulipHipError, match="TULIP_ERR_ARG"):
        ops.loss_edge_bwd(x, x, None, 1.0, -0.5, x, 1, 4, 4)
    with pytest.raises(_lib.TulipHipError, match="TULIP_ERR_ARG"):
        ops.loss_edge_final(x, x, x, NAN, 1, 4, 4)
    with pytest.raises(_lib.TulipHipError, match="TULIP_ERR_ARG"):
        ops.loss_edge_bwd(x, x, None, 1.0, 0.5, x, 3, 4, 4, mask=(2, 0.0), counts=x)
    torch.cuda.synchronize()
    assert not x.any().item()


# ---------------------------------------------------------------------------------------------------- 2. the masked forms
def masked_inputs(shape, variant, seed=0):
    B, C, H, W = shape
    p, t = M.inputs((B, C, H * W), variant, seed)
    rng = np.random.default_rng(seed + 5)
    base = (rng.standard_normal(shape) / np.prod(shape)).astype(np.float32)
    return p.reshape(shape), t.reshape(shape), base


def check_masked(p_h, t_h, base, got):
    dpred, edge, losses, _ = got
    m = L.valid_mask(t_h, VMIN)
    assert np.array_equal(bits(dpred), bits(L.edge_grad32(p_h, t_h, base, WEIGHT, valid_min=VMIN)))
    assert not bits(dpred[~m]).any()                                                              # +0.0 at the invalid elements
    np.testing.assert_allclose(edge, L.edge_value(p_h, t_h, VMIN), rtol=1e-5, atol=0)
    assert bits(losses[0]) == bits(np.float32(1.25) + np.float32(WEIGHT) * edge) and losses[1] == 3.0
    return m


@pytest.mark.parametrize("variant", ["seeded", "all_valid", "none_valid", "last_only", "nonfinite_invalid"])
@pytest.mark.parametrize("shape", MASK_SHAPES, ids=ids)
def test_masked_kernels_match_the_host_definition(shape, variant):
    p_h, t_h, base = masked_inputs(shape, variant)
    got = run(p_h, t_h, base, valid_min=VMIN)
    m = check_masked(p_h, t_h, base, got)
    dpred, edge, losses, part = got
    print(f"{shape} {variant}: edge {edge!r} n_v {int(m.sum())} of {m.size}")
    assert same(run(p_h, t_h, base, valid_min=VMIN, offset=1), got) and same(run(p_h, t_h, base, valid_min=VMIN), got)
    gdev = torch.full((1,), 0.3, dtype=torch.float32, device=DEV)
    a = run(p_h, t_h, base, valid_min=VMIN, gscale_dev=gdev, gscale=9.0)
    assert same(a, run(p_h, t_h, base, valid_min=VMIN, gscale=0.3))
    assert np.array_equal(bits(a[0]), bits(L.edge_grad32(p_h, t_h, base, WEIGHT, 0.3, valid_min=VMIN)))
    if variant == "all_valid":
        assert m.all() and same(got, run(p_h, t_h, base))                                         # the unmasked launches' bits
    elif variant == "none_valid":
        assert not m.any() and not bits(dpred).any() and bits(edge) == 0 and not bits(part).any() and losses[0] == 1.25
    elif variant == "last_only":
        # one valid pixel among holes: its own d has the taps' weight 0 and every neighbour's d is 0 -- no response, k == 0, the base
        # gradient stays at the valid elements
        assert int(m.sum()) == shape[1] and bits(edge) == 0 and losses[0] == 1.25
        assert np.array_equal(bits(dpred[-1, :, -1, -1]), bits(base[-1, :, -1, -1] + np.float32(0.0))) and dpred[-1, :, -1, -1].all()
    elif variant == "nonfinite_invalid":
        # the same inputs with finite values at the invalid pixels: not one bit moves
        assert not np.isfinite(p_h).all() and np.isfinite(dpred).all() and math.isfinite(edge)
        p2, t2 = np.where(m, p_h, np.float32(0.5)), np.where(m, t_h, np.float32(-1.0))
        assert np.array_equal(L.valid_mask(t2, VMIN), m)
        assert same(run(p2, t2, base, valid_min=VMIN), got)
    else:
        assert 0 < int(m.sum()) < m.size


def test_a_hole_drops_exactly_the_responses_centred_on_it():
    """integer input, every pixel valid but one hole beside valid pixels (in_chans 2: both of its elements): the edge sum is exact --
    the sum over all responses of the field with d = 0 at the hole, minus the two centred on it, over n_v = n - 2."""
    shape = (1, 2, 9, 129)
    p_h, t_h, base = make(shape, "int", seed=7)
    t_h[:, 0] = np.abs(t_h[:, 0]) + 1.0
    p_h = t_h + np.random.default_rng(3).integers(-3, 4, shape).astype(np.float32)
    t_h[0, 0, 7, 127] = 0.0                                                                       # across the tile's corner
    p_h[0, :, 7, 127] = (NAN, 2.0)
    got = run(p_h, t_h, base, valid_min=VMIN)
    dpred, edge, losses, part = got
    m = L.valid_mask(t_h, VMIN)
    assert int(m.sum()) == m.size - 2
    d = np.where(m, p_h.astype(np.float64) - t_h, 0.0)
    e_h, e_v = L.edge_responses(d)
    s = np.abs(e_h) + np.abs(e_v)
    assert s[0, :, 7, 127].min() > 0                                                              # there is something to drop
    total = s.sum() - s[0, :, 7, 127].sum()
    assert float(part.astype(np.float64).sum()) == total
    assert bits(edge) == bits(np.float32(total * (1.0 / (m.size - 2)))) == bits(L.edge_total32(p_h, t_h, 1.25, WEIGHT, VMIN)[0])
    assert np.array_equal(bits(dpred), bits(L.edge_grad32(p_h, t_h, base, WEIGHT, valid_min=VMIN)))
    assert not bits(dpred[0, :, 7, 127]).any()


# ---------------------------------------------------------------------------------------------------- 3. plane isolation
@pytest.mark.parametrize("plane", [(0, 0), (0, 1), (1, 0)])
def test_an_impulse_at_a_planes_last_pixel_stays_in_its_plane(plane):
    """d = one 1 at the last pixel of plane (b, c), which lies next to the first pixel of the next plane (the next sample's for
    c = 1): its three neighbours in the plane respond (|e_h| + |e_v| = 2 each; the corner's own response is 0), nothing else does."""
    shape = (2, 2, 9, 129)
    b, c = plane
    t_h = np.zeros(shape, dtype=np.float32)
    p_h = t_h.copy()
    p_h[b, c, -1, -1] = 1.0
    base = make(shape, "randn", seed=9)[2]
    dpred, edge, losses, part = run(p_h, t_h, base)
    assert np.array_equal(bits(dpred), bits(L.edge_grad32(p_h, t_h, base, WEIGHT)))
    others = np.ones(shape, dtype=bool)
    others[b, c] = False
    assert np.array_equal(bits(dpred[others]), bits(base[others] + np.float32(0.0)))              # k == 0 in every other plane
    assert not np.array_equal(bits(dpred[b, c]), bits(base[b, c]))
    # one workgroup per tile here, four tiles per plane: the neighbours lie in the plane's other three tiles (the corner's own sees 0)
    first = 4 * (2 * b + c)
    assert part.size == 16 and part[first:first + 4].tolist() == [2.0, 2.0, 2.0, 0.0] and np.count_nonzero(part) == 3
    assert bits(edge) == bits(np.float32(6.0 * (1.0 / p_h.size)))


# ---------------------------------------------------------------------------------------------------- 4. model vs the oracle
_oracle_cache = {}


def case_data(case, masked):
    return M.masked_case(case) if masked else G.model_case(case)


def oracle_grads(case, kind, lowp, masked=False, weight=WEIGHT):
    """(loss, {name: grad}, pred) of the oracle's forward with torch_loss(..., edge_weight=) by autograd; computed once"""
    key = (case, kind, lowp, masked, weight)
    if key not in _oracle_cache:
        cfg, sd, lo, hi = case_data(case, masked)
        leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
        full = dict(sd)
        full.update(leaves)
        pred = O.tulip_forward(full, cfg, lo, None, lowp=lowp)
        loss = L.torch_loss(kind, pred, hi, valid_min=VMIN if masked else None, edge_weight=weight)
        loss.backward()
        _oracle_cache[key] = (loss.item(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()},
                              pred.detach())
    return _oracle_cache[key]


def device_grads(case, kind, masked=False, weight=WEIGHT):
    cfg, sd, lo, hi = case_data(case, masked)
    kw = dict(loss_valid_min=VMIN) if masked else {}
    if weight is not None:
        kw["loss_edge_weight"] = weight
    m = M.build(cfg, sd, kind, **kw)
    pred, loss, pix = m(lo.to(DEV), hi.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    P = m.engine().plan(lo.shape[0])
    return (P, pred.detach().cpu(), loss.item(), pix.item(), {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()})


# the oracle's own worst rel_l2 between its lowp=True and lowp=False gradients at weight 0.5, measured on the CPU and held to the
# oracle there (tests/test_loss_edge_cpu.py, test_the_recorded_low_precision_distance_is_the_oracles); see the docstring below
OWN_LOWP = C.OWN_LOWP
MODEL = [(case, kind, False) for case in G.MODEL_CASES for kind in KINDS] + [("in_chans2", "berhu", True)]


@pytest.mark.parametrize("case,kind,masked", MODEL, ids=lambda v: str(v))
def test_model_loss_and_gradients_vs_oracle(case, kind, masked):
    """model(lo, hi) and loss.backward() with loss_edge_weight=0.5 against the oracle's autograd of torch_loss(..., edge_weight=0.5),
    at the tolerances of tests/test_loss_gpu.py: loss 1e-3 relative, gradient rel_l2 1.5e-2 against the fp32 oracle and 1e-2
    against the low-precision one (bias tables 1e-1 and 5e-2).  The edge read-out is the host value for the device's own pred.

    The four in_chans2 cases miss the 1.5e-2 bound against the fp32 oracle while they keep the 1e-2 bound against the low-precision
    oracle (0.62e-2 to 0.72e-2): the term's gradient is a sign function of responses, and responses near zero flip under the bf16
    forward.  The oracle shows the same on the CPU without any device, in the worst rel_l2 between its own lowp=True and lowp=False
    gradients (bias tables aside), OWN_LOWP.  Measured, worst tensor of each case at weight 0.5:

        case                    device vs fp32 oracle    oracle lowp vs fp32 (OWN_LOWP)    the same at weight 0
        in_chans2 l1            1.78e-2                  1.65e-2                           1.05e-2
        in_chans2 l2            1.69e-2                  1.64e-2                           0.87e-2
        in_chans2 berhu         1.64e-2                  1.57e-2                           0.94e-2
        in_chans2 berhu masked  1.85e-2                  1.73e-2                           1.14e-2

    For these four the fp32 bound is twice the OWN_LOWP figure (the factor covers the device's rounding order on top of bf16
    operands); the six cases of the other two configurations meet 1.5e-2 and keep it.  tests/test_loss_edge_cpu.py holds the
    recorded figures to the oracle."""
    rel_l2 = G.rel_l2
    ol, og, _ = oracle_grads(case, kind, False, masked)
    _, olp, _ = oracle_grads(case, kind, True, masked)
    P, pred, loss, pix, g = device_grads(case, kind, masked)
    cfg, sd, lo, hi = case_data(case, masked)
    vm = VMIN if masked else None
    worst = max((rel_l2(g[n], og[n]), n) for n in g if not n.endswith("relative_position_bias_table"))
    worst_lp = max((rel_l2(g[n], olp[n]), n) for n in g if not n.endswith("relative_position_bias_table"))
    own = max((rel_l2(olp[n], og[n]), n) for n in g if not n.endswith("relative_position_bias_table"))
    print(f"{case} {kind} masked={masked}: loss {loss!r} oracle {ol!r} (rel {abs(loss - ol) / ol:.2e}); worst rel_l2 vs fp32 {worst}, "
          f"vs lowp {worst_lp}; the oracle's own lowp vs fp32 {own}")
    assert abs(loss - ol) <= 1e-3 * ol
    np.testing.assert_allclose(pix, L.pixel_loss(pred.numpy(), hi.numpy(), cfg.log_transform, valid_min=vm), rtol=1e-5)
    np.testing.assert_allclose(P.loss_edge.item(), L.edge_value(pred.numpy(), hi.numpy(), vm), rtol=1e-5)
    np.testing.assert_allclose(loss, L.loss_value(kind, pred.numpy(), hi.numpy(), vm) + WEIGHT * L.edge_value(pred.numpy(), hi.numpy(), vm),
                               rtol=2e-5)
    bound = 1.5e-2
    if (case, kind, masked) in OWN_LOWP:
        bound = 2 * OWN_LOWP[case, kind, masked]             # (from the recorded figure, not from `own` as measured in this run)
    for n in g:
        table = n.endswith("relative_position_bias_table")
        assert rel_l2(g[n], og[n]) <= (1e-1 if table else bound), n
        assert rel_l2(g[n], olp[n]) <= (5e-2 if table else 1.0e-2), n


def test_the_edge_term_changes_the_gradient():
    """weight 0.5 against weight 0: the oracle alone separates decoder_pred.weight's gradients by more than three times the
    tolerance applied above, and so does the device; a model built with weight 0.0 gives the gradient of one built without."""
    case = "pixel_shuffle"
    for kind in ("l1", "berhu"):
        _, og_e, _ = oracle_grads(case, kind, False)
        _, og_0, _ = oracle_grads(case, kind, False, weight=0.0)
        assert G.rel_l2(og_e["decoder_pred.weight"], og_0["decoder_pred.weight"]) > 3 * 1.5e-2
        _, _, le, _, ge = device_grads(case, kind)
        _, _, l0, _, g0 = device_grads(case, kind, weight=0.0)
        _, _, ln, _, gn = device_grads(case, kind, weight=None)
        assert G.rel_l2(ge["decoder_pred.weight"], g0["decoder_pred.weight"]) > 3 * 1.5e-2 and le > l0
        assert bits(l0) == bits(ln) and all(torch.equal(g0[n].view(torch.int32), gn[n].view(torch.int32)) for n in g0)


def test_no_grad_forward_returns_the_total():
    case, kind = "pixel_shuffle", "l1"
    cfg, sd, lo, hi = G.model_case(case)
    m = M.build(cfg, sd, kind, loss_edge_weight=WEIGHT)
    with torch.no_grad():
        _, loss, pix = m(lo.to(DEV), hi.to(DEV))
    _, _, loss_g, pix_g, _ = device_grads(case, kind)
    assert bits(loss.item()) == bits(loss_g) and bits(pix.item()) == bits(pix_g)
    ol, _, _ = oracle_grads(case, kind, False)
    assert abs(loss.item() - ol) <= 1e-3 * ol


# ---------------------------------------------------------------------------------------------------- 5. Trainer
def trainer_run(loss, steps=3, batch=2, model_kw={}, **kw):
    from tulip_amd.trainer import Trainer
    cfg = O.tiny_config(drop_path_rate=0.0)
    sd = O.key_seeded_state_dict(cfg, seed=3)
    m = M.build(cfg, sd, loss, train=True, **model_kw)
    tr = Trainer(m, batch, lr=5e-4, **kw)
    lo, hi = (t.to(DEV) for t in O.synthetic_batch(cfg, batch, seed=77))
    tr.load_batch(lo, hi)
    losses = [tr.step().clone() for _ in range(steps)]
    torch.cuda.synchronize()
    return tr, torch.stack(losses).cpu().numpy(), tr.eng.params.flat.clone().cpu().numpy(), (lo, hi)


@pytest.mark.parametrize("kind,masked", [("l1", False), ("berhu", True)])
def test_trainer_graph_and_eager_steps_are_bit_identical(kind, masked):
    mk = dict(loss_edge_weight=WEIGHT, **(dict(loss_valid_min=VMIN) if masked else {}))
    tr_g, lg, pg, (lo, hi) = trainer_run(kind, model_kw=mk, use_graph=True)
    tr_e, le, pe, _ = trainer_run(kind, model_kw=mk, use_graph=False)
    print(f"{kind} masked={masked} edge trainer losses", lg.tolist(), "edge", tr_g.edge_loss.item())
    assert np.isfinite(lg).all() and lg[-1, 0] < lg[0, 0]
    assert np.array_equal(bits(lg), bits(le)) and np.array_equal(bits(pg), bits(pe))
    assert bits(tr_g.edge_loss.item()) == bits(tr_e.edge_loss.item()) and tr_g.edge_loss.item() > 0.0
    # the read-out is the host value for the last forward's pred, and losses[0] the total
    vm = VMIN if masked else None
    pred, target = tr_g.P.pred.cpu().numpy(), hi.cpu().numpy()
    np.testing.assert_allclose(tr_g.edge_loss.item(), L.edge_value(pred, target, vm), rtol=1e-5)
    np.testing.assert_allclose(lg[-1, 0], L.loss_value(kind, pred, target, vm) + WEIGHT * L.edge_value(pred, target, vm), rtol=2e-5)
    assert tr_g.state_dict()["loss_edge_weight"] == WEIGHT
    # ... and the term is not nothing: another trajectory than without it
    _, l0, p0, _ = trainer_run(kind, model_kw={k: v for k, v in mk.items() if k != "loss_edge_weight"}, use_graph=True)
    assert not np.array_equal(bits(l0[:, 0]), bits(lg[:, 0])) and not np.array_equal(bits(p0), bits(pg))
    np.testing.assert_allclose(l0[0, 1], lg[0, 1], rtol=1e-5)                  # the first step's pixel_loss: the same L1 metric


def test_trainer_accumulation_runs():
    for use_graph in (True, False):
        tr, la, pa, _ = trainer_run("l1", steps=4, accum_iter=2, use_graph=use_graph, model_kw=dict(loss_edge_weight=WEIGHT))
        assert np.isfinite(la).all() and np.isfinite(pa).all()
        assert bits(la[0, 0]) == bits(la[1, 0]) and la[2, 0] < la[0, 0]


@pytest.mark.parametrize("kind", ["l1", "berhu"])
def test_weight_zero_is_the_step_without_the_argument(kind):
    tr_a, la, pa, _ = trainer_run(kind, model_kw=dict(loss_edge_weight=0.0), use_graph=True)
    tr_b, lb, pb, _ = trainer_run(kind, use_graph=True)
    assert np.array_equal(bits(la), bits(lb)) and np.array_equal(bits(pa), bits(pb))
    assert set(tr_a.P.bufs) == set(tr_b.P.bufs) and tr_a.state_dict()["loss_edge_weight"] == 0.0
    with pytest.raises(AttributeError):
        tr_a.edge_loss


@pytest.mark.parametrize("use_graph", [True, False])
def test_trainer_skips_a_nonfinite_target(use_graph):
    """skip_nonfinite with the edge term beside loss="l2": one NaN in the target (no mask: every pixel is valid) reaches the loss, the
    responses around it and the norm; the step is skipped, the parameters stay, and the following clean step is applied."""
    tr, _, _, (lo, hi) = trainer_run("l2", steps=2, use_graph=use_graph, skip_nonfinite=True, model_kw=dict(loss_edge_weight=WEIGHT))
    assert int(tr.last_step_skipped.item()) == 0 and tr.applied_steps == 2
    before = tr.eng.params.flat.clone()
    bad = hi.clone()
    bad[1, 0, 5, 9] = NAN
    losses = tr.step(lo, bad).clone()
    torch.cuda.synchronize()
    assert int(tr.last_step_skipped.item()) != 0 and tr.applied_steps == 2 and tr.skipped_steps == 1
    assert math.isnan(losses[0].item()) and math.isnan(tr.edge_loss.item())
    assert torch.equal(tr.eng.params.flat.view(torch.int32), before.view(torch.int32))
    losses = tr.step(lo, hi).clone()
    torch.cuda.synchronize()
    assert int(tr.last_step_skipped.item()) == 0 and tr.applied_steps == 3 and math.isfinite(losses[0].item())
    assert not torch.equal(tr.eng.params.flat.view(torch.int32), before.view(torch.int32))
    assert torch.isfinite(tr.eng.params.flat).all().item()

"""GPU: the multi-channel evaluation kernels (csrc/evalpost.hip: tulip_eval_postprocess_c, tulip_mc_aggregate_c) against their host
definition (tulip_amd/eval_channels.py), against the single-channel kernels on the channel-0 planes, and through ChannelEvaluator and
the loops evaluate_multichannel / MCdrop_multichannel.

Tolerances.  A plane that no expm1 produced is bit-identical to the host definition; n_valid is exact; a MAE column (the same float64
sum in another order, then one float32 rounding) agrees to 1e-6 relative, the tolerance of tests/test_eval_gpu.py.  A plane of a logged
channel agrees within 3e-7, that file's bound of the device's expm1f against the host's at values up to 1.05 (every channel value of
these cases is drawn in [0, 1]); its MAE columns are means of |p - t| with both operands within that bound, so they get 6e-7 absolute
on top.  Every decision is identical: the cases keep channel 0 at least 1e-6 away from 0, gmin, gmax and keep_close (asserted here for
every pixel, so no pixel is left out of a comparison)."""
import functools
import json
from functools import partial
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import eval_channels_cases as K
from tulip_amd import eval_channels as EC
from tulip_amd import evaluation as EV

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 12345.0
SHAPES = {"f4_restored": (8, 16, 2, 16), "widths_differ": (8, 16, 2, 8), "ragged": (6, 10, 3, 10)}
STRIDE = (260, 1024, 65, 1024)        # 1040 blocks' worth of pixels: the second trip of the loop capped at 1024 blocks
LOGS = {"plain": (False, None), "log0": (True, None), "logc": (False, 0), "log0_logc": (True, 0)}


@pytest.fixture(scope="module")
def ops():
    from tulip_amd import ops as _ops
    return _ops


def run_post(ops, pred, hi, lo, log_transform, logs, keep_close, single=False):
    """one launch pair on (C,H,W) host arrays -> (pred_img, hi_img, metrics) host arrays; every output buffer ends in a sentinel
    zone that must come back untouched.  single: tulip_eval_postprocess on the channel-0 planes."""
    C, H, W = pred.shape
    h, w = lo.shape[1:]
    if single:
        pred, hi, lo, C = pred[:1], hi[:1], lo[:1], 1
    S = 2 if single else 3 * C + 1
    n = C * H * W
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    p_img, t_img = (torch.full((n + 64,), SENTINEL, dtype=torch.float32, device=DEV) for _ in range(2))
    metrics = torch.full((S + 16,), SENTINEL, dtype=torch.float32, device=DEV)
    partials = torch.full((S * 1024 + 16,), SENTINEL, dtype=torch.float64, device=DEV)
    if single:
        ops.eval_postprocess(d(pred), d(hi), d(lo), p_img, t_img, partials, metrics, H, W, h, w, log_transform, *K.GATE, keep_close)
    else:
        ops.eval_postprocess_c(d(pred), d(hi), d(lo), p_img, t_img, partials, metrics, H, W, h, w, C, log_transform, logs, *K.GATE,
                               keep_close)
    torch.cuda.synchronize()
    for buf, used in ((p_img, n), (t_img, n), (metrics, S), (partials, S * 1024)):
        assert bool((buf[used:] == SENTINEL).all()), "a write past the end of an output buffer"
    return (p_img[:n].cpu().numpy().reshape(C, H, W), t_img[:n].cpu().numpy().reshape(C, H, W), metrics[:S].cpu().numpy(),
            p_img[:n].view(C, H, W), t_img[:n].view(C, H, W))


def check_post(ops, C, shape, log_transform, bit, keep, inject, seed):
    H, W, h, w = shape
    logs = [bit == k for k in range(C - 1)]
    kc = K.KEEP_CLOSE if keep else 0.0
    pred, hi, lo = K.post_case(C, H, W, h, w, log_transform, logs, seed=seed, inject=inject)
    assert K.margins_hold(pred, hi, lo, log_transform, K.KEEP_CLOSE) == 0          # the share of pixels left out is zero
    want = EC.eval_channels(pred, hi, lo, log_transform, logs, K.GATE, kc)
    p_img, t_img, m, _, _ = run_post(ops, pred, hi, lo, log_transform, logs, kc)
    logged = [bool(log_transform)] + logs
    tag = (C, shape, log_transform, bit, keep, inject)
    for c in range(C):
        assert K.planes_agree(p_img[c], want.pred_img[c], logged[c]), ("pred_img", c) + tag
        assert K.planes_agree(t_img[c], want.hi_img[c], logged[c]), ("hi_img", c) + tag
        extra = 6e-7 if logged[c] else 0.0
        assert K.close(m[c], want.mae[c], 1e-6, extra), ("mae", c, m[c], want.mae[c]) + tag
        assert K.close(m[C + c], want.mae_low[c], 1e-6, extra), ("mae_low", c, m[C + c], want.mae_low[c]) + tag
        assert K.close(m[2 * C + c], want.mae_valid[c], 1e-6, extra), ("mae_valid", c, m[2 * C + c], want.mae_valid[c]) + tag
        if w != W:
            assert m[C + c] == 0
    assert m[3 * C] == want.n_valid, tag
    # the hole rule on the device's own planes: +0.0 in every channel of a pixel that is a hole and whose row is not restored
    not_restored = np.ones((H, W), dtype=bool)
    if w == W:
        not_restored[0::H // h] = False
    for c in range(1, C):
        v = p_img[c][want.hole & not_restored]
        assert not v.any() and not np.signbit(v).any(), ("hole", c) + tag
    return want


@pytest.mark.parametrize("keep", [False, True], ids=["keep_off", "keep_on"])
@pytest.mark.parametrize("logs", sorted(LOGS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("C", [2, 3, 4])
def test_postprocess_c_vs_host_definition(ops, C, shape, logs, keep):
    log_transform, bit = LOGS[logs]
    for inject in (False, True):
        H, W, _, _ = SHAPES[shape]
        want = check_post(ops, C, SHAPES[shape], log_transform, bit, keep, inject, seed=H * W + C)
        if not inject:
            assert np.isfinite(want.mae).all() and 0 < want.n_valid < H * W and want.hole.any()


@pytest.mark.parametrize("keep", [False, True], ids=["keep_off", "keep_on"])
@pytest.mark.parametrize("logs", sorted(LOGS))
def test_postprocess_c_second_trip_of_the_stride_loop(ops, logs, keep):
    log_transform, bit = LOGS[logs]
    for inject in (False, True):
        want = check_post(ops, 2, STRIDE, log_transform, bit, keep, inject, seed=77)
        if not inject:
            assert np.isfinite(want.mae).all() and want.hole[256:].any() and want.valid[256:].any()     # rows of the second trip


@pytest.mark.parametrize("log_transform", [False, True], ids=["plain", "log"])
@pytest.mark.parametrize("shape", [SHAPES["f4_restored"], SHAPES["widths_differ"], SHAPES["ragged"], STRIDE], ids=str)
def test_channel_0_is_bit_identical_to_the_single_channel_kernel(ops, shape, log_transform):
    H, W, h, w = shape
    for C in ((2,) if shape == STRIDE else (2, 3, 4)):
        logs = [k == 0 for k in range(C - 1)]
        pred, hi, lo = K.post_case(C, H, W, h, w, log_transform, logs, seed=5 + C, inject=True)
        _, _, m, p_c, t_c = run_post(ops, pred, hi, lo, log_transform, logs, K.KEEP_CLOSE)
        _, _, m1, p_1, t_1 = run_post(ops, pred, hi, lo, log_transform, logs, K.KEEP_CLOSE, single=True)
        assert torch.equal(p_c[0].view(torch.int32), p_1[0].view(torch.int32))
        assert torch.equal(t_c[0].view(torch.int32), t_1[0].view(torch.int32))
        assert K.close(m[0], m1[0], 1e-6) and K.close(m[C], m1[1], 1e-6)
        pred, hi, lo = K.post_case(C, H, W, h, w, log_transform, logs, seed=5 + C, inject=False)      # finite MAE columns
        _, _, m, p_c, t_c = run_post(ops, pred, hi, lo, log_transform, logs, 0.0)
        _, _, m1, p_1, t_1 = run_post(ops, pred, hi, lo, log_transform, logs, 0.0, single=True)
        assert torch.equal(p_c[0], p_1[0]) and torch.equal(t_c[0], t_1[0])
        assert np.isfinite(m1).all() and K.close(m[0], m1[0], 1e-6) and K.close(m[C], m1[1], 1e-6)


# ------------------------------------------------------------------ MC aggregate
def check_mc(ops, T, C, n, seed):
    preds, thr = K.mc_case(T, C, n, seed)
    assert K.mc_margin(preds, thr) == 0                     # the share of pixels left out is zero
    want = EC.mc_aggregate_channels(preds, thr)
    d = torch.from_numpy(preds).to(DEV)
    out = torch.full((C * n + 64,), SENTINEL, dtype=torch.float32, device=DEV)
    ops.mc_aggregate_c(d, T, C, n, thr, out)
    single = torch.full((n,), SENTINEL, dtype=torch.float32, device=DEV)
    ops.mc_aggregate(d[:, 0].contiguous(), T, n, thr, single)
    torch.cuda.synchronize()
    assert bool((out[C * n:] == SENTINEL).all())
    got = out[:C * n].view(C, n)
    assert torch.equal(got[0], single)
    g = got.cpu().numpy()
    assert np.isfinite(g).all()
    drop = want[0] == 0
    assert 0.2 < drop.mean() < 0.5 and np.array_equal(g[0] == 0, drop)
    mean = (preds.astype(np.float64).sum(axis=0) / T).astype(np.float32)      # the float64 sum of these values is exact
    for c in range(C):
        assert not g[c][drop].any() and np.array_equal(g[c][~drop], mean[c][~drop]), c
    assert K.same_bits(g, want)


@pytest.mark.parametrize("C", [2, 3, 4])
@pytest.mark.parametrize("T", [2, 12])
def test_mc_aggregate_c(ops, T, C):
    check_mc(ops, T, C, 8 * 16, seed=100 * T + C)


def test_mc_aggregate_c_second_trip_of_the_stride_loop(ops):
    check_mc(ops, 2, 2, 4096 * 256 + 257, seed=9)


def test_mc_aggregate_channels_shape(ops):
    preds, thr = K.mc_case(3, 2, 8 * 16, seed=4)
    out = EV.mc_aggregate_channels(torch.from_numpy(preds).to(DEV).view(3, 2, 8, 16), thr)
    assert tuple(out.shape) == (1, 2, 8, 16)
    assert K.same_bits(out[0].cpu().numpy().reshape(2, -1), EC.mc_aggregate_channels(preds, thr))


# ------------------------------------------------------------------ ChannelEvaluator
@functools.lru_cache(maxsize=None)
def evaluator_case(ds, log_transform, seed=31):
    """(pred, lo, hi) device tensors (1,2,..) of a seeded two-channel image whose channel 0 keeps the margins of the dataset's gate and
    of keep_close (asserted for every pixel), so the host definition takes every decision as the device does, with the log too"""
    gate = EV.pred_gate(ds, False)
    P, T, L = K.post_case(2, 16, 64, 4, 64, log_transform, [log_transform], seed=seed, inject=False, gate=gate)
    assert K.margins_hold(P, T, L, log_transform, K.KEEP_CLOSE, gate) == 0
    return tuple(torch.from_numpy(a)[None].to(DEV) for a in (P, L, T))


@pytest.mark.parametrize("log_transform", [False, True], ids=["plain", "log"])
@pytest.mark.parametrize("ds", ["carla", "durlar"])
def test_channel_evaluator_vs_range_evaluator(ds, log_transform):
    pred, lo, hi = evaluator_case(ds, log_transform)
    logs = [log_transform]
    ev = EV.ChannelEvaluator(ds, (4, 64), (16, 64), log_transform, 2, logs, 0.1, True, False, DEV)
    ev1 = EV.RangeEvaluator(ds, (4, 64), (16, 64), log_transform, 0.1, True, False, DEV)
    for _ in range(2):                                  # the second call finds the scratch, counters and bitmaps of the first
        res = ev(pred, lo, hi)
        res1 = ev1(pred[:, :1].contiguous(), lo[:, :1].contiguous(), hi[:, :1].contiguous())
        assert res.dtype == torch.float64 and res.is_cuda and res.numel() == 8 + len(EV.channel_columns(2)) == len(ev.columns)
        assert torch.equal(res[:8], res1) and bool(torch.isfinite(res).all())
        assert not ev.bm_pred.any().item() and not ev.bm_gt.any().item()      # bitmaps handed back clean
    assert tuple(ev.pred_img.shape) == tuple(ev.hi_img.shape) == (2, 16, 64)
    assert torch.equal(ev.pred_img[0], ev1.pred_img) and torch.equal(ev.hi_img[0], ev1.hi_img)
    assert ev.pcd_pred.dtype == (torch.float64 if ds == "durlar" else torch.float32)
    assert torch.equal(ev.pcd_pred, ev1.pcd_pred) and torch.equal(ev.pcd_gt, ev1.pcd_gt)
    want = EC.eval_channels(pred[0].cpu().numpy(), hi[0].cpu().numpy(), lo[0].cpu().numpy(), log_transform, logs, ev.gate, ev.keep_close)
    r = dict(zip(ev.columns, res.cpu().numpy()))
    extra = 6e-7 if log_transform else 0.0
    assert r["n_valid"] == want.n_valid > 0 and r["status"] == 0
    for name, v in (("mae", want.mae[0]), ("mae_low_res", want.mae_low[0]), ("mae_valid", want.mae_valid[0]), ("mae_ch1", want.mae[1]),
                    ("mae_low_res_ch1", want.mae_low[1]), ("mae_valid_ch1", want.mae_valid[1])):
        assert K.close(r[name], v, 1e-6, extra), (name, r[name], v)


def test_channel_evaluator_refuses_a_single_channel_image():
    ev = EV.ChannelEvaluator("carla", (4, 64), (16, 64), False, 2, None, device=DEV)
    pred, lo, hi = evaluator_case("carla", False)
    with pytest.raises(ValueError):
        ev(pred[:, :1].contiguous(), lo[:, :1].contiguous(), hi[:, :1].contiguous())


# ------------------------------------------------------------------ loops
REF_KEYS = ["mae", "chamfer_dist", "iou", "precision", "recall", "f1"]


class _StandIn(torch.nn.Module):
    """hands out prepared predictions, one batch per call (the pattern of tests/test_eval_gpu.py)"""
    in_chans = 2

    def __init__(self, preds):
        super().__init__()
        self.preds, self.i = preds, 0

    def forward(self, lo, hi, eval=False, mc_drop=False):
        p = self.preds[self.i]
        self.i += 1
        return p.to(lo.device), None, None


def test_loop_files_equal_the_evaluator_called_directly(tmp_path):
    cases = [evaluator_case("carla", True, seed) for seed in (31, 32, 33)]
    loader = [({"sample": cases[0][1]}, {"sample": cases[0][2]}),
              ({"sample": torch.cat([cases[1][1], cases[2][1]])}, {"sample": torch.cat([cases[1][2], cases[2][2]])})]
    model = _StandIn([cases[0][0], torch.cat([cases[1][0], cases[2][0]])])
    args = SimpleNamespace(img_size_low_res=(4, 64), img_size_high_res=(16, 64), grid_size=0.1, log_transform=True,
                           dataset_select="carla", output_dir=str(tmp_path), channel_log=[True])
    scalars = {}
    avg = EV.evaluate_multichannel(loader, model, DEV, SimpleNamespace(add_scalar=lambda k, v, s: scalars.__setitem__(k, v)), args)
    res = json.load(open(tmp_path / "results.txt"))
    chan = json.load(open(tmp_path / "results_channels.txt"))
    assert list(res.keys()) == REF_KEYS and list(chan.keys()) == list(EV.channel_columns(2))
    assert avg["per_image"] == res and avg["per_image_channels"] == chan and not model.training
    ev = EV.ChannelEvaluator("carla", (4, 64), (16, 64), True, 2, [True], 0.1, False, False, DEV)
    rows = np.stack([ev(*c).cpu().numpy() for c in cases])
    for k, name in enumerate(ev.columns):
        col = res[name] if name in res else chan.get(name)
        if col is not None:
            assert col == rows[:, k].tolist(), name
    for name in EV.channel_columns(2):
        assert avg[name] == float(np.sum(chan[name]) / 3)
    assert avg["loss"] == float(rows[:, 0].sum() / 3) == scalars["Metrics/test_average_loss"]
    assert avg["mae_low_res"] == float(rows[:, 1].sum() / 3)


def _tiny2():
    from oracle import tulip_oracle as O
    from tulip_amd.model import tulip as T
    cfg = O.tiny_config(in_chans=2, drop_path_rate=0.0)
    m = T.TULIP(img_size=cfg.img_size, target_img_size=cfg.target_img_size, patch_size=cfg.patch_size, in_chans=cfg.in_chans,
                embed_dim=cfg.embed_dim, window_size=list(cfg.window_size), depths=cfg.depths, num_heads=cfg.num_heads,
                mlp_ratio=cfg.mlp_ratio, drop_path_rate=cfg.drop_path_rate, norm_layer=partial(nn.LayerNorm, eps=cfg.ln_eps),
                pixel_shuffle=cfg.pixel_shuffle, circular_padding=cfg.circular_padding, log_transform=cfg.log_transform,
                patch_unmerging=cfg.patch_unmerging)
    m.load_state_dict(O.key_seeded_state_dict(cfg, seed=0), strict=True)
    return m.to(DEV)


def test_loops_with_the_hip_model_and_range_prep(tmp_path):
    """the whole path: RangePrep(in_chans=2) batches -> TULIP(in_chans=2) forward -> device evaluation, one read-back at the end"""
    from tulip_amd.data import RangePrep
    prep = RangePrep("carla", (8, 256), (32, 256), log_transform=True, in_chans=2, channel_log=[True])
    g = torch.Generator().manual_seed(17)
    raw = torch.stack([torch.rand(2, 32, 256, generator=g) * 85.0, torch.rand(2, 32, 256, generator=g)], dim=-1)
    raw[..., 0][torch.rand(2, 32, 256, generator=g) < 0.1] = 0
    lo, hi = prep(raw.contiguous().to(DEV))
    assert tuple(lo.shape) == (2, 2, 8, 256) and tuple(hi.shape) == (2, 2, 32, 256)
    model = _tiny2()
    n_valid = []
    for name, loader in (("ones", [(lo[i:i + 1], hi[i:i + 1]) for i in range(2)]), ("pair", [(lo, hi)])):
        out = tmp_path / name
        args = SimpleNamespace(img_size_low_res=(8, 256), img_size_high_res=(32, 256), grid_size=0.1, log_transform=True,
                               dataset_select="carla", output_dir=str(out), keep_close_scan=False, channel_log=[True],
                               num_mcdropout_iterations=10, noise_threshold=0.03)
        avg = EV.evaluate_multichannel(loader, model, DEV, None, args)
        res = json.load(open(out / "results.txt"))
        chan = json.load(open(out / "results_channels.txt"))
        assert list(res.keys()) == REF_KEYS and list(chan.keys()) == list(EV.channel_columns(2))
        for d in (res, chan):
            assert all(len(v) == 2 and np.isfinite(v).all() for v in d.values()), d
        assert min(chan["n_valid"]) > 0 and avg["per_image"] == res and avg["per_image_channels"] == chan
        n_valid.append(chan["n_valid"])
    assert n_valid[0] == n_valid[1]                     # a property of the targets alone
    expect = (hi[:, 0] > 0).sum(dim=(1, 2)).tolist()
    assert n_valid[0] == [float(v) for v in expect]
    avg2 = EV.MCdrop_multichannel([(lo[i:i + 1], hi[i:i + 1]) for i in range(2)], model, DEV, None, args)
    res2 = json.load(open(out / "results_mcdrop.txt"))
    chan2 = json.load(open(out / "results_mcdrop_channels.txt"))
    assert list(res2.keys()) == REF_KEYS and res2["iou"] == [] and res2["f1"] == [] and len(res2["mae"]) == 2
    assert list(chan2.keys()) == list(EV.channel_columns(2)) and all(len(v) == 2 for v in chan2.values())
    assert np.isfinite(avg2["loss"]) and avg2["per_image"] == res2 and chan2["n_valid"] == n_valid[0]
    assert all(np.isfinite(v).all() for v in chan2.values())

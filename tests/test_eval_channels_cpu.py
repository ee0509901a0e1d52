"""CPU: the multi-channel evaluation (tulip_amd/eval_channels.py, ChannelEvaluator and the loops of tulip_amd/evaluation.py).

1. The host definition: channel 0 is the single-channel chain (oracle/eval_oracle.py, pinned to the reference by g10_eval.npz), the
   hole and valid rules, the valid-pixel metric, keep_close over all channels, no restore when the widths differ.
2. The MC aggregate's definition: channel 0 is the single-channel aggregate and decides the drop for every channel.  Against
   oracle.eval_oracle.mc_aggregate "equals" means the same drop mask and kept values within T * 2^-23: the oracle's mean is torch's
   float32 sum, the definition's (and the kernels') is the float64 mean rounded once, so bit equality with the oracle is not
   attainable; tests/test_eval_channels_gpu.py pins the definition's channel 0 bit for bit to tulip_mc_aggregate instead.
3. Refusals of the two C entry points (before any launch, so with dummy pointers) and of the Python surface (before any device use)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import eval_oracle as EO
from tests import eval_channels_cases as K
from tulip_amd import _lib
from tulip_amd import eval_channels as EC
from tulip_amd import evaluation as EV

F32 = np.float32
CARLA_GATE = EO.pred_gate("carla", False)


@pytest.mark.parametrize("ds,shape,log_transform,keep", [("carla", (16, 64, 4, 64), False, False), ("carla", (16, 64, 4, 32), False, False),
                                                         ("durlar", (16, 64, 4, 64), False, True), ("kitti", (64, 1024, 16, 1024), False, False),
                                                         ("carla", (16, 64, 4, 64), True, False), ("durlar", (16, 64, 4, 64), True, True)])
def test_channel_0_is_the_single_channel_chain(ds, shape, log_transform, keep):
    H, W, h, w = shape
    (pred, hi, lo), (P, T, L) = K.stack_case(ds, 3, H, W, h, w, 31, log_transform)
    mae, mae_low, p_img, t_img = EO.postprocess(pred, hi, lo, ds, log_transform, mc_drop=False, keep_close_scan=keep)
    r = EC.eval_channels(P, T, L, log_transform, [False, True], EO.pred_gate(ds, False), 0.25 if keep and ds == "durlar" else 0.0)
    if log_transform:       # numpy's float32 expm1 against torch's: the bound of tests/test_eval_gpu.py for two expm1 of values <= 1.05
        assert np.array_equal(r.pred_img[0] == 0, p_img == 0)
        assert np.abs(r.pred_img[0] - p_img).max() <= 3e-7 and np.abs(r.hi_img[0] - t_img).max() <= 3e-7
        assert K.close(r.mae[0], mae, 1e-6, 6e-7) and K.close(r.mae_low[0], mae_low, 1e-6, 6e-7)
    else:
        assert K.same_bits(r.pred_img[0], p_img) and K.same_bits(r.hi_img[0], t_img)
        assert K.close(r.mae[0], mae, 1e-6) and K.close(r.mae_low[0], mae_low, 1e-6)
    if w != W:
        assert mae_low == 0 and not r.mae_low.any()


def _small(C=3, H=4, W=6, h=2, fill=0.5):
    pred = np.full((C, H, W), fill, dtype=np.float32)
    hi = np.full((C, H, W), fill, dtype=np.float32)
    return pred, hi, np.ascontiguousarray(hi[:, 0::H // h])


def test_hole_rule_yields_positive_zero_in_every_other_channel():
    pred, hi, lo = _small()
    holes = {(1, 0): 0.0, (1, 1): 0.001, (1, 2): 7.0, (1, 3): np.nan, (1, 4): -0.3, (3, 5): -np.inf}    # row 1, 3: not restored
    for k, (px, v0) in enumerate(holes.items()):
        pred[0][px] = v0
        pred[1][px] = (np.nan, np.inf, -np.inf, -2.0, -0.0, np.nan)[k]
        pred[2][px] = (-1.0, np.nan, np.inf, -np.inf, np.nan, -0.0)[k]
    for logs in ([False, False], [True, False], [True, True]):
        r = EC.eval_channels(pred, hi, lo, False, logs, CARLA_GATE)
        for px in holes:
            assert r.hole[px]
            for c in range(3):
                v = r.pred_img[c][px]
                assert v == 0 and not np.signbit(v), (px, c, v)
        assert int(r.hole.sum()) == len(holes)
        assert np.isfinite(r.mae).all() and np.isfinite(r.mae_valid).all()
        # a hole costs the whole target value in every channel: |0 - 0.5| there, 0 elsewhere
        inv = np.expm1(F32(0.5))
        want = [F32(0.5), inv if logs[0] else F32(0.5), inv if logs[1] else F32(0.5)]
        for c in range(3):
            assert K.close(r.mae[c], len(holes) * float(want[c]) / 24, 1e-6)


def test_negative_zero_range_is_a_hole():
    pred, hi, lo = _small()
    pred[0][1, 2], pred[1][1, 2], pred[2][1, 2] = -0.0, 0.75, np.nan
    r = EC.eval_channels(pred, hi, lo, False, None, (0.0, 1.0))          # MCdrop's KITTI gate lets -0.0 through
    assert np.signbit(r.pred_img[0][1, 2]) and r.hole[1, 2] and int(r.hole.sum()) == 1
    assert r.pred_img[1][1, 2] == 0 and not np.signbit(r.pred_img[1][1, 2]) and not np.signbit(r.pred_img[2][1, 2])
    r = EC.eval_channels(pred, hi, lo, True, [True, False], CARLA_GATE)  # expm1(-0.0) = -0.0 fails a gate above 0
    assert r.hole[1, 2] and r.pred_img[0][1, 2] == 0 and not np.signbit(r.pred_img[0][1, 2]) and r.pred_img[1][1, 2] == 0


def test_nan_target_is_not_valid_and_the_valid_metric_skips_it():
    pred, hi, lo = _small()
    pred[:, 1, 1] = (0.6, 0.7, 0.9)
    hi[0][1, 3], hi[0][3, 0], hi[0][3, 1], hi[0][1, 5] = np.nan, 0.0, -0.0, -0.2
    hi[1][3, 0] = 0.0
    r = EC.eval_channels(pred, hi, lo, False, None, CARLA_GATE)
    assert not r.valid[1, 3] and not r.valid[3, 0] and not r.valid[3, 1] and not r.valid[1, 5] and r.n_valid == 24 - 4
    assert np.isnan(r.mae[0]) and np.isfinite(r.mae[1:]).all()               # the plain mean keeps the reference's NaN ...
    for c, d in enumerate((0.1, 0.2, 0.4)):                                  # ... the valid-pixel mean does not see it
        assert K.close(r.mae_valid[c], d / 20, 2e-6)
    assert K.close(r.mae[1], (0.2 + 0.5) / 24, 2e-6)                          # channel 1: + the zeroed target pixel (3, 0)


def test_no_valid_pixel_gives_zero():
    pred, hi, lo = _small()
    hi[0] = 0.0
    hi[0][0, 0] = np.nan
    r = EC.eval_channels(pred, hi, lo, False, None, CARLA_GATE)
    assert r.n_valid == 0 and r.mae_valid.dtype == np.float32 and not r.mae_valid.any() and not np.isnan(r.mae_valid).any()


def test_widths_differ_no_row_is_restored():
    pred, hi, _ = _small()
    pred[:, 0, :] = 0.25
    lo = np.ascontiguousarray(hi[:, 0::2, 0::2])
    r = EC.eval_channels(pred, hi, lo, False, None, CARLA_GATE)
    assert not r.mae_low.any() and K.same_bits(r.pred_img, pred)
    r = EC.eval_channels(pred, hi, np.ascontiguousarray(hi[:, 0::2]), False, None, CARLA_GATE)
    assert K.same_bits(r.pred_img, hi) and all(K.close(v, 0.25 / 2, 1e-6) for v in r.mae_low)     # row 0 of the two restored rows
    assert all(K.close(v, 0.25 * 6 / 24, 1e-6) for v in r.mae)                                   # taken before the restore


def test_keep_close_zeroes_all_channels_of_a_pixel_together():
    pred, hi, lo = _small(fill=0.2)
    pred[0][1, 1], hi[0][3, 3], hi[0][0, 2] = 0.3, 0.4, 0.9           # (0, 2): a restored row takes the far value from lo
    lo = np.ascontiguousarray(hi[:, 0::2])
    r = EC.eval_channels(pred, hi, lo, False, None, (0.3 / 120, 1.0), keep_close=0.25)
    for c in range(3):
        assert r.pred_img[c][1, 1] == 0 and r.pred_img[c][0, 2] == 0 and r.hi_img[c][3, 3] == 0 and r.hi_img[c][0, 2] == 0
        assert r.hi_img[c][1, 1] == F32(0.2) and r.pred_img[c][3, 3] == F32(0.2)
    assert int((r.pred_img == 0).sum()) == 6 and int((r.hi_img == 0).sum()) == 6
    assert not r.hole.any() and r.n_valid == 24                       # both classes are taken before keep_close
    off = EC.eval_channels(pred, hi, lo, False, None, (0.3 / 120, 1.0), keep_close=0.0)
    assert not (off.pred_img == 0).any() and np.array_equal(off.mae, r.mae) and np.array_equal(off.mae_valid, r.mae_valid)


@pytest.mark.parametrize("C", [2, 3, 4])
@pytest.mark.parametrize("log_transform,bit", [(False, None), (True, None), (False, 0), (True, 0)])
def test_seeded_cases_keep_their_margins(C, log_transform, bit):
    """the cases of the GPU test: every decision has its margin, both classes of pixel occur, the definition is finite without injections"""
    logs = [bit == k for k in range(C - 1)]
    for H, W, h, w in ((8, 16, 2, 16), (8, 16, 2, 8), (6, 10, 3, 10)):
        for inject in (False, True):
            pred, hi, lo = K.post_case(C, H, W, h, w, log_transform, logs, seed=H * W + C, inject=inject)
            assert K.margins_hold(pred, hi, lo, log_transform, K.KEEP_CLOSE) == 0
            r = EC.eval_channels(pred, hi, lo, log_transform, logs, K.GATE, K.KEEP_CLOSE)
            assert 0 < r.hole.sum() < H * W and 0 < r.n_valid < H * W
            if not inject:
                assert np.isfinite(r.mae).all() and np.isfinite(r.mae_low).all() and np.isfinite(r.mae_valid).all()
                assert (r.mae_low > 0).all() == (w == W)


# ------------------------------------------------------------------ MC aggregate
@pytest.mark.parametrize("T,C", [(2, 2), (12, 3), (5, 4)])
def test_mc_channel_0_is_the_single_channel_aggregate_and_a_drop_zeroes_all_channels(T, C):
    preds, thr = K.mc_case(T, C, 8 * 16, seed=T * 10 + C)
    assert K.mc_margin(preds, thr) == 0
    out = EC.mc_aggregate_channels(preds, thr)
    ref = EO.mc_aggregate(torch.from_numpy(np.ascontiguousarray(preds[:, 0])), thr)[0].numpy()
    drop = ref == 0
    assert 0.2 < drop.mean() < 0.5
    assert np.array_equal(out[0] == 0, drop) and np.abs(out[0] - ref).max() <= T * 2.0 ** -23    # torch's mean: T float32 additions of values < 2
    mean = (preds.astype(np.float64).sum(axis=0) / T).astype(np.float32)
    assert np.array_equal(out[0][~drop], mean[0][~drop])
    for c in range(1, C):
        assert not out[c][drop].any() and np.array_equal(out[c][~drop], mean[c][~drop]) and (out[c][~drop] > 0).all()


def test_mc_definition_refuses_one_pass():
    with pytest.raises(ValueError):
        EC.mc_aggregate_channels(np.zeros((1, 2, 8), dtype=np.float32), 0.03)


# ------------------------------------------------------------------ refusals: before any launch, so with dummy pointers
FAKE, E = 4096, -1


def test_refused_arguments_of_the_c_abi():
    lib = _lib.load()

    def po(H=8, W=16, h=2, w=16, C=2, bits=0, **null):
        ptr = [None if null.get(k) else FAKE for k in ("pred", "hi", "lo", "pred_img", "hi_img", "partials", "metrics")]
        return lib.tulip_eval_postprocess_c(*ptr, H, W, h, w, C, 0, bits, 0.0, 1.0, 0.0, None)
    for k in ("pred", "hi", "lo", "pred_img", "hi_img", "partials", "metrics"):
        assert po(**{k: True}) == E, k
    assert po(C=1) == E and po(C=5) == E and po(C=0) == E and po(C=-2) == E
    assert po(H=9) == E and po(h=3) == E and po(h=0) == E and po(H=0) == E and po(W=0) == E and po(w=0) == E and po(H=-8, h=-2) == E
    assert po(C=2, bits=2) == E and po(C=3, bits=4) == E and po(C=4, bits=8) == E      # a log flag of a channel that is not there

    def mc(passes=2, C=2, n=16, preds=FAKE, out=FAKE):
        return lib.tulip_mc_aggregate_c(preds, passes, C, n, 0.03, out, None)
    assert mc(passes=1) == E and mc(passes=0) == E and mc(n=0) == E and mc(n=-4) == E
    assert mc(C=1) == E and mc(C=5) == E and mc(C=0) == E and mc(preds=None) == E and mc(out=None) == E


def test_refused_arguments_of_the_python_surface():
    mk = lambda C, logs=None: EV.ChannelEvaluator("carla", (4, 64), (16, 64), False, C, logs, device="cpu")
    with pytest.raises(ValueError, match="RangeEvaluator"):
        mk(1)
    for bad in (0, 5, -1, 2.0, True, None, "2"):
        with pytest.raises(ValueError, match="in_chans"):
            mk(bad)
    for C, logs in ((2, [True, False]), (3, [True]), (2, []), (2, [1]), (2, ["yes"]), (2, True), (2, "T"), (3, [True, None])):
        with pytest.raises(ValueError, match="channel_log"):
            mk(C, logs)
    with pytest.raises(RuntimeError, match="GPU only"):           # valid arguments reach the device check, and only then
        mk(2, [True])
    assert EV.channel_columns(2) == ("mae_ch1", "mae_low_res_ch1", "mae_valid_ch1", "mae_valid", "n_valid")
    assert EV.channel_columns(3)[3:6] == ("mae_ch2", "mae_low_res_ch2", "mae_valid_ch2") and len(EV.channel_columns(4)) == 11
    args = SimpleNamespace(dataset_select="carla", img_size_low_res=(4, 64), img_size_high_res=(16, 64), log_transform=False,
                           grid_size=0.1, output_dir=None, num_mcdropout_iterations=10, noise_threshold=0.03)
    for loop in (EV.evaluate_multichannel, EV.MCdrop_multichannel):
        with pytest.raises(ValueError, match="evaluate"):
            loop([], SimpleNamespace(in_chans=1), "cpu", None, args)
        with pytest.raises(ValueError, match="in_chans"):
            loop([], SimpleNamespace(in_chans=5), "cpu", None, args)
        args.channel_log = [True, True]
        with pytest.raises(ValueError, match="channel_log"):
            loop([], SimpleNamespace(in_chans=2), "cpu", None, args)
        del args.channel_log
    with pytest.raises(ValueError):
        EV.mc_aggregate_channels(torch.zeros(2, 2, 4, 4), 0.03)   # a host tensor

"""Multi-channel input batches on the GPU: tulip_range_prep_c / tulip_range_prep_aug_c through RangePrep(in_chans=...).

Channel 0 of every output has the bits of RangePrep(in_chans=1) of the same library on the same payload (which
tests/test_data_gpu.py holds to the reference); channels without a log have the bits of the host definition
(tulip_amd/prep_channels.py: one float32 multiply and a select have one correct result); channels with a log have its zero pattern
and are within LOG_ATOL of it.  The augmented outputs are bit for bit `augment.apply` of the plain multi-channel output.  Payloads:
oracle.data_oracle.synthetic_raw for channel 0 (holes and gate-edge values), intensities with negatives, NaN and infinities inside
the holes and finite values elsewhere; every case asserts on the host that it holds holes, gate-rejected pixels and valid pixels."""
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import data_oracle as DO
from oracle import tulip_oracle as O
from tulip_amd import augment as A
from tulip_amd import data as D
from tulip_amd import ops
from tulip_amd import prep_channels as PC

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOG_ATOL = 2.4e-7          # tests/test_data_gpu.py: this kernel family's log1pf against the host's, arguments in [0, 1.6]
SCALES = (0.5, 2.0, 1 / 255)
BAD = np.array([-3.0, np.nan, np.inf, -np.inf, -0.0, 1e30, -1e-30, 7.5], dtype=np.float32)


def bits(a):
    if torch.is_tensor(a):
        a = a.cpu().numpy()
    assert a.dtype == np.float32
    return np.ascontiguousarray(a).view(np.uint32)


def make_payload(ds, B, H, W, Cr, seed):
    """(B,H,W,Cr) float32: synthetic_raw ranges; channel c >= 1 scaled by SCALES[c-1] lies in [0, 1.5] outside the holes and is one
    of BAD inside them"""
    r0 = DO.synthetic_raw(B, H, W, seed=seed).numpy()
    scale, gate = D.DATASET_PREP[ds]
    v0, hole = PC.holes(r0, scale, gate)
    assert hole.any() and (~hole).any() and (r0 == 0).any()
    if gate is not None:
        assert (hole & (r0 != 0)).any()                             # gate-rejected pixels, below the minimum or above the maximum
        assert (r0 * np.float32(scale) > 1).any() and ((r0 != 0) & (r0 * np.float32(scale) < np.float32(gate[0]))).any()
    g = np.random.default_rng(seed)
    chans = [r0]
    for c in range(1, Cr):
        x = (g.random((B, H, W), dtype=np.float32) * np.float32(1.5 / SCALES[c - 1])).astype(np.float32)
        x[hole] = BAD[(np.arange(int(hole.sum())) + c) % BAD.size]
        assert not np.isfinite(x[hole]).all() and (x[hole] < 0).any() and np.isfinite(x[~hole]).all()
        chans.append(x)
    return np.ascontiguousarray(np.stack(chans, -1))


def check_against_definition(got, want, logs):
    """channels 1.. of one output against the host definition"""
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    for c in range(1, got.shape[1]):
        if not logs[c - 1]:
            assert np.array_equal(bits(got[:, c]), bits(want[:, c])), f"channel {c}"
        else:
            assert np.isfinite(got[:, c]).all()
            assert np.array_equal(bits(got[:, c]) == 0, bits(want[:, c]) == 0), f"channel {c}: zero pattern"
            assert np.abs(got[:, c] - want[:, c]).max() <= LOG_ATOL, f"channel {c}"


def check_plain(ds, lo_size, hi_size, log_t, raw, C, logs, dev_raw=None, **kw):
    """one plain case: both outputs, then each output alone"""
    scales = SCALES[:C - 1]
    prep = D.RangePrep(ds, lo_size, hi_size, log_t, in_chans=C, channel_scale=scales, channel_log=logs, **kw)
    one = D.RangePrep(ds, lo_size, hi_size, log_t, **kw)
    dev_raw = torch.from_numpy(raw).to(DEV) if dev_raw is None else dev_raw
    lo, hi = prep(dev_raw)
    lo1, hi1 = one(dev_raw)
    B = raw.shape[0]
    assert tuple(lo.shape) == (B, C) + tuple(lo_size) and tuple(hi.shape) == (B, C) + tuple(hi_size)
    assert lo.is_contiguous() and hi.is_contiguous() and lo.dtype == hi.dtype == torch.float32
    assert np.array_equal(bits(lo[:, :1]), bits(lo1)) and np.array_equal(bits(hi[:, :1]), bits(hi1))
    scale, gate = D.DATASET_PREP[ds]
    wlo, whi = PC.prep_channels(raw, scale, gate, log_t, C, scales, logs, prep.f, prep.fw, kw.get("row_phase", 0),
                                kw.get("col_phase", 0), kw.get("roll_shift") or 0)
    check_against_definition(lo, wlo, logs)
    check_against_definition(hi, whi, logs)
    lo_only, none = prep(dev_raw, want_hi=False)
    assert none is None and np.array_equal(bits(lo_only), bits(lo))
    none, hi_only = prep(dev_raw, want_lo=False)
    assert none is None and np.array_equal(bits(hi_only), bits(hi))
    return lo, hi


# ---------------------------------------------------------------------------------------------------- 1. fast path, plain
@pytest.mark.parametrize("ds", ["kitti", "durlar", "carla"])
@pytest.mark.parametrize("log_t", [True, False])
def test_interleaved_pair_payload(ds, log_t):
    """(8,16) -> (2,16), Cr = C = 2, B = 4: the 16-byte kernel; roll_shift 0 and 4 keep its 16-byte stores, 5 does not"""
    raw = make_payload(ds, 4, 8, 16, 2, seed=31)
    for shift in (0, 4, 5):
        for logs in ((False,), (True,)):
            check_plain(ds, (2, 16), (8, 16), log_t, raw, 2, logs, roll_shift=shift)


@pytest.mark.parametrize("C", [2, 3, 4])
def test_interleaved_quad_payload(C):
    """Cr = 4 (one 16-byte load per pixel), C of its channels taken"""
    raw = make_payload("durlar", 4, 8, 16, 4, seed=32)
    for log_t, logs, shift in ((True, (True, False, True)[:C - 1], 0), (False, (False, True, False)[:C - 1], 5)):
        check_plain("durlar", (2, 16), (8, 16), log_t, raw, C, logs, roll_shift=shift)


def test_more_than_one_block_and_grid_stride():
    """(64,128) -> (16,128), B = 3: 2048 four-pixel groups per image, 8 workgroups per sample"""
    raw = make_payload("carla", 3, 64, 128, 2, seed=33)
    check_plain("carla", (16, 128), (64, 128), True, raw, 2, (True,), roll_shift=64)


# ---------------------------------------------------------------------------------------------------- 2. generic path, plain
def test_three_raw_channels():
    raw = make_payload("durlar", 4, 8, 16, 3, seed=34)
    for log_t, logs, shift in ((True, (False, True), 0), (False, (True, False), 5)):
        check_plain("durlar", (2, 16), (8, 16), log_t, raw, 3, logs, roll_shift=shift)
    check_plain("durlar", (2, 16), (8, 16), True, raw, 2, (True,))                  # Cr = 3, C = 2: the extra channel is ignored


def test_width_18_crosses_no_alignment():
    raw = make_payload("carla", 4, 8, 18, 2, seed=35)
    for shift in (0, 7):
        check_plain("carla", (2, 18), (8, 18), True, raw, 2, (True,), roll_shift=shift)


def test_tile_edges():
    """H = 40 > TI = 32 and W = 72 > TJ = 64 in the LDS-tile kernel (Cr = 3), W = 72 in the 16-byte kernel (Cr = 2)"""
    for Cr in (3, 2):
        raw = make_payload("durlar", 2, 40, 72, Cr, seed=36)
        check_plain("durlar", (10, 72), (40, 72), True, raw, Cr, (True, False)[:Cr - 1], roll_shift=9)


@pytest.mark.parametrize("col_phase", [0, 1])
def test_width_subsampling(col_phase):
    raw = make_payload("durlar", 4, 8, 16, 2, seed=37)
    for shift in (0, 3):
        check_plain("durlar", (2, 8), (8, 16), True, raw, 2, (True,), roll_shift=shift, col_phase=col_phase)
    raw = make_payload("durlar", 4, 8, 16, 3, seed=37)
    check_plain("durlar", (2, 8), (8, 16), False, raw, 3, (False, True), col_phase=col_phase)


def test_row_phase():
    for Cr in (2, 3):
        raw = make_payload("carla", 4, 8, 16, Cr, seed=38)
        check_plain("carla", (2, 16), (8, 16), True, raw, Cr, (True, False)[:Cr - 1], row_phase=1)
        check_plain("carla", (2, 16), (8, 16), False, raw, Cr, (False, False)[:Cr - 1], row_phase=3, roll_shift=2)


def test_misaligned_payload_view():
    """the same payload one element into its buffer: 4-byte aligned only, so the 16-byte loads are not taken"""
    raw = make_payload("durlar", 4, 8, 16, 2, seed=39)
    buf = torch.empty(raw.size + 1, dtype=torch.float32, device=DEV)
    view = buf[1:].view(raw.shape)
    view.copy_(torch.from_numpy(raw))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    lo, hi = check_plain("durlar", (2, 16), (8, 16), True, raw, 2, (True,), dev_raw=view)
    lo2, hi2 = D.RangePrep("durlar", (2, 16), (8, 16), True, in_chans=2, channel_scale=SCALES[:1], channel_log=(True,))(
        torch.from_numpy(raw).to(DEV))
    assert torch.equal(lo, lo2) and torch.equal(hi, hi2)                            # both kernel families: the same bits


def test_planar_source_through_the_entry_point():
    """channel stride H*W, pixel stride 1 (a (B,C,H,W) source): the LDS-tile kernel's addressing, against the interleaved call"""
    raw = make_payload("carla", 4, 8, 16, 3, seed=40)
    prep = D.RangePrep("carla", (2, 16), (8, 16), True, in_chans=3, channel_scale=SCALES[:2], channel_log=(False, True))
    lo, hi = prep(torch.from_numpy(raw).to(DEV))
    planar = torch.from_numpy(np.ascontiguousarray(np.moveaxis(raw, 3, 1))).to(DEV)
    hi2, lo2 = torch.full_like(hi, -1), torch.full_like(lo, -1)
    gmin, gmax = prep.gate
    ops.range_prep_c(planar, 0, 3 * 8 * 16, 16, 1, 0, hi2, lo2, 4, 8, 16, 4, 1, 0, 0, prep.scale, True, gmin, gmax, True, 0, 3,
                     8 * 16, prep.channel_scale, prep.channel_log)
    assert np.array_equal(bits(hi2), bits(hi)) and np.array_equal(bits(lo2), bits(lo))


# ---------------------------------------------------------------------------------------------------- 3. augmented
@pytest.mark.parametrize("Cr", [2, 3])
def test_augmented_is_a_gather_of_the_plain_output(Cr):
    """tests/test_augment_gpu.py's coverage recipe: B = 64, ids 0..63, seed 0, (8,16) -> (2,16), with beam and point drops;
    Cr = C = 2: the 16-byte kernel, Cr = C = 3: the LDS-tile kernel.  The log path is included: a gather moves bits."""
    ids = np.arange(64)
    par = A.params(0, ids, 16, 4)
    assert {(s % 4, fl) for s, fl, _ in par.tolist()} == {(r, fl) for r in range(4) for fl in (0, 1)}
    assert set(par[:, 0]) == set(range(16)) and set(par[:, 2]) == set(range(4))
    bm, pm = A.beam_mask(0, ids, 2, 0.25), A.point_mask(0, ids, 2, 16, 0.5)
    dropped = bm[:, :, None] | pm
    assert bm.any() and pm.any() and not dropped.all()
    raw = make_payload("durlar", 64, 8, 16, Cr, seed=41)
    dev_raw = torch.from_numpy(raw).to(DEV)
    aug = A.RangeAugment(seed=0, beam_drop=0.25, point_drop=0.5)
    kw = dict(in_chans=Cr, channel_scale=SCALES[:Cr - 1], channel_log=(True, False)[:Cr - 1])
    plain = D.RangePrep("durlar", (2, 16), (8, 16), True, **kw)
    prep = D.RangePrep("durlar", (2, 16), (8, 16), True, augment=aug, **kw)
    lo0, hi0 = plain(dev_raw)
    pout = torch.full((64, 4), -1, dtype=torch.int32, device=DEV)
    lo, hi = prep(dev_raw, sample_ids=torch.as_tensor(ids, dtype=torch.int64).to(DEV), params_out=pout)
    assert tuple(lo.shape) == (64, Cr, 2, 16) and tuple(hi.shape) == (64, Cr, 8, 16)
    assert np.array_equal(pout.cpu().numpy(), np.concatenate([par, np.zeros((64, 1), np.int64)], 1))
    wlo, whi = A.apply(hi0.cpu().numpy(), 0, ids, 4, beam_drop=0.25, point_drop=0.5)
    assert np.array_equal(bits(hi), bits(whi))
    assert np.array_equal(bits(lo), bits(wlo))
    assert not bits(lo)[np.broadcast_to(dropped[:, None], lo.shape)].any()          # a dropped pixel: +0.0 in every channel
    # the draws are those of in_chans=1 for the same ids, and channel 0 is its output
    one = D.RangePrep("durlar", (2, 16), (8, 16), True, augment=aug)
    pout1 = torch.full((64, 4), -1, dtype=torch.int32, device=DEV)
    lo1, hi1 = one(dev_raw, sample_ids=ids.tolist(), params_out=pout1)
    assert torch.equal(pout1, pout)
    assert np.array_equal(bits(lo[:, :1]), bits(lo1)) and np.array_equal(bits(hi[:, :1]), bits(hi1))
    # each output alone
    lo_only, none = prep(dev_raw, sample_ids=ids.tolist(), want_hi=False)
    assert none is None and np.array_equal(bits(lo_only), bits(lo))
    none, hi_only = prep(dev_raw, sample_ids=ids.tolist(), want_lo=False)
    assert none is None and np.array_equal(bits(hi_only), bits(hi))


def test_augmented_width_subsampling_and_quad_payload():
    """fw = 2 with a column phase (any shift is legal), on Cr = 4 / C = 3 in the 16-byte kernel and on W = 18 in the LDS-tile one"""
    ids = np.arange(64)
    aug = A.RangeAugment(seed=0, beam_drop=0.25, point_drop=0.5)
    for W, w, fw, cp, Cr, C in ((16, 8, 2, 1, 4, 3), (18, 18, 1, 0, 2, 2), (16, 16, 1, 0, 4, 4)):
        raw = make_payload("carla", 64, 8, W, Cr, seed=42)
        dev_raw = torch.from_numpy(raw).to(DEV)
        kw = dict(col_phase=cp, in_chans=C, channel_scale=SCALES[:C - 1], channel_log=(False, True, True)[:C - 1])
        lo0, hi0 = D.RangePrep("carla", (2, w), (8, W), True, **kw)(dev_raw)
        lo, hi = D.RangePrep("carla", (2, w), (8, W), True, augment=aug, **kw)(dev_raw, sample_ids=ids.tolist())
        wlo, whi = A.apply(hi0.cpu().numpy(), 0, ids, 4, fw, cp, beam_drop=0.25, point_drop=0.5)
        assert np.array_equal(bits(hi), bits(whi)) and np.array_equal(bits(lo), bits(wlo))


# ---------------------------------------------------------------------------------------------------- 4. loader
def test_loader_yields_multichannel_pairs(tmp_path):
    root = tmp_path / "train"
    root.mkdir()
    pay = make_payload("kitti", 5, 8, 16, 2, seed=43)
    for i in range(5):
        np.save(root / f"{i:06d}.npy", pay[i])
    (tmp_path / "carla").mkdir()
    (tmp_path / "carla" / "a.rimg").write_bytes(np.array([8, 16], dtype=np.uint).tobytes() + np.zeros(128, np.float16).tobytes())
    aug = A.RangeAugment(seed=3, beam_drop=0.25, point_drop=0.25)
    for augment in (None, aug):
        prep = D.RangePrep("kitti", (2, 16), (8, 16), True, in_chans=2, augment=augment)
        kw = {} if augment is None else dict(sample_ids=list(range(5)))
        wlo, whi = prep(torch.from_numpy(pay).to(DEV), **kw)                        # the direct call on the stacked payloads
        ld = D.DeviceRangeLoader(str(root), prep, 2, drop_last=False)
        seen = 0
        for lo, hi in ld:
            n = lo.shape[0]
            assert n == (2 if seen < 4 else 1) and tuple(lo.shape) == (n, 2, 2, 16) and tuple(hi.shape) == (n, 2, 8, 16)
            assert np.array_equal(bits(lo), bits(wlo[seen:seen + n])) and np.array_equal(bits(hi), bits(whi[seen:seen + n]))
            seen += n
        assert seen == 5
        with pytest.raises(ValueError, match="rimg"):
            next(iter(D.DeviceRangeLoader(str(tmp_path / "carla"), prep, 1)))
    scale, gate = D.DATASET_PREP["kitti"]
    dlo, dhi = PC.prep_channels(pay, scale, gate, True, 2, f=4)
    check_against_definition(D.RangePrep("kitti", (2, 16), (8, 16), True, in_chans=2)(torch.from_numpy(pay).to(DEV))[1], dhi, (False,))


# ---------------------------------------------------------------------------------------------------- 5. into the model
def test_batch_feeds_the_two_channel_model():
    """tests/test_inchans_gpu.py's smallest two-channel configuration (fixture g16_inchans, c2) without the log, with the masked
    loss: the batch of RangePrep(in_chans=2) goes straight through model(lo, hi) and one Trainer step, and both give the bits they
    give on the host-definition tensors uploaded by hand (no log anywhere: the inputs are bit-equal)."""
    from tulip_amd.model import tulip as T
    from tulip_amd.trainer import Trainer
    cfg = O.TulipConfig(img_size=(8, 256), target_img_size=(32, 256), patch_size=(1, 4), in_chans=2, embed_dim=48,
                        window_size=(2, 8), depths=(2, 2), num_heads=(3, 6), mlp_ratio=4.0, drop_path_rate=0.0, ln_eps=1e-6,
                        pixel_shuffle=True, circular_padding=True, log_transform=False, patch_unmerging=True)
    sd = O.key_seeded_state_dict(cfg, seed=5)

    def model():
        m = T.TULIP(img_size=cfg.img_size, target_img_size=cfg.target_img_size, patch_size=cfg.patch_size, in_chans=2,
                    embed_dim=cfg.embed_dim, window_size=list(cfg.window_size), depths=cfg.depths, num_heads=cfg.num_heads,
                    mlp_ratio=cfg.mlp_ratio, drop_path_rate=0.0, norm_layer=partial(nn.LayerNorm, eps=cfg.ln_eps),
                    pixel_shuffle=True, circular_padding=True, log_transform=False, patch_unmerging=True, loss_valid_min=0.0)
        m.load_state_dict(sd, strict=True)
        return m.to(DEV).train()
    raw = make_payload("kitti", 2, 32, 256, 2, seed=44)
    prep = D.RangePrep("kitti", (8, 256), (32, 256), False, in_chans=2, channel_scale=SCALES[:1])
    lo, hi = prep(torch.from_numpy(raw).to(DEV))
    scale, gate = D.DATASET_PREP["kitti"]
    wlo, whi = PC.prep_channels(raw, scale, gate, False, 2, SCALES[:1], f=4)
    assert np.array_equal(bits(lo), bits(wlo)) and np.array_equal(bits(hi), bits(whi))
    hlo, hhi = torch.from_numpy(wlo).to(DEV), torch.from_numpy(whi).to(DEV)
    ma, mb = model(), model()
    pa, la, xa = ma(lo, hi)
    pb, lb, xb = mb(hlo, hhi)
    assert tuple(pa.shape) == (2, 2, 32, 256)
    assert torch.isfinite(pa).all() and torch.isfinite(la).all() and torch.isfinite(xa).all()
    assert torch.equal(pa, pb) and torch.equal(la, lb) and torch.equal(xa, xb)
    ta, tb = Trainer(ma, 2, use_graph=False), Trainer(mb, 2, use_graph=False)
    sa = ta.step(lo, hi).clone()
    sb = tb.step(hlo, hhi).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(sa).all() and torch.equal(sa, sb)
    assert torch.equal(ta.eng.params.flat, tb.eng.params.flat)

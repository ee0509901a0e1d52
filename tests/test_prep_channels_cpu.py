"""CPU: multi-channel input batches, RangePrep(in_chans=...).  The host definition (tulip_amd/prep_channels.py) on a hand-made
image, every refusal of RangePrep with no device present, the C ABI of the two entry points (header, ctypes signature, both
library builds) and their TULIP_ERR_ARG answers, which come before any launch and therefore need no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tulip_amd import _lib
from tulip_amd import augment as A
from tulip_amd import data as D
from tulip_amd import prep_channels as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------- 1. the definition
def hand_made():
    """one 2x4 image, [range m, intensity, reflectivity]: holes (0.0 and -0.0) with every kind of bad intensity, a NaN range, a
    range below CARLA's 2 m gate, and ordinary pixels"""
    rng = np.array([[0.0, -0.0, NAN, 1.0], [40.0, 0.0, 80.0, 0.0]], dtype=np.float32)
    inten = np.array([[NAN, -3.0, 5.0, 7.0], [0.25, INF, -0.0, -INF]], dtype=np.float32)
    refl = np.array([[-1.0, 2.0, 3.0, 4.0], [8.0, NAN, 16.0, 32.0]], dtype=np.float32)
    return np.stack([rng, inten, refl], -1)[None]


def test_hole_zeroes_the_other_channels_with_positive_zero_bits():
    raw = hand_made()
    scale, gate = D.DATASET_PREP["kitti"]
    lo, hi = PC.prep_channels(raw, scale, gate, False, 3, [0.5, 2.0], [False, False])
    assert hi.shape == (1, 3, 2, 4) and hi.dtype == np.float32 and lo.shape == (1, 3, 2, 4)
    v0, hole = PC.holes(raw[..., 0], scale, gate)
    assert hole.tolist() == [[[True, True, False, False], [False, True, False, True]]]
    for c in (1, 2):
        assert not bits(hi[0, c])[hole[0]].any()                    # +0.0: all 32 bits clear, whatever the raw value was
    # outside the holes: one float32 multiply
    assert np.array_equal(bits(hi[0, 1])[~hole[0]], bits(raw[0, ..., 1] * np.float32(0.5))[~hole[0]])
    assert np.array_equal(bits(hi[0, 2])[~hole[0]], bits(raw[0, ..., 2] * np.float32(2.0))[~hole[0]])
    assert bits(hi[0, 1, 1, 2]) == 0x80000000                       # a -0.0 intensity outside a hole stays -0.0
    # channel 0 is the single-channel chain
    assert np.array_equal(bits(hi[0, 0]), bits(raw[0, ..., 0] * np.float32(scale)))


def test_nan_range_is_not_a_hole_and_negative_zero_is():
    raw = hand_made()
    scale, gate = D.DATASET_PREP["kitti"]
    v0, hole = PC.holes(raw[..., 0], scale, gate)
    assert np.isnan(v0[0, 0, 2]) and not hole[0, 0, 2]
    assert bits(v0[0, 0, 1]) == 0x80000000 and hole[0, 0, 1]
    _, hi = PC.prep_channels(raw, scale, gate, True, 2, [1.0], [True])
    assert np.isnan(hi[0, 0, 0, 2]) and hi[0, 1, 0, 2] == np.log1p(np.float32(5.0))
    assert bits(hi[0, 1, 0, 1]) == 0                                # log1p(+0.0) = +0.0
    # behind a gate a rejected range (here the NaN and the 1 m return) is zero, and therefore a hole
    scale, gate = D.DATASET_PREP["carla"]
    v0, hole = PC.holes(raw[..., 0], scale, gate)
    assert hole.tolist() == [[[True, True, True, True], [False, True, False, True]]]
    _, hi = PC.prep_channels(raw, scale, gate, True, 3, [1.0, 1.0], [True, False])
    assert not bits(hi[0, 1:])[:, hole[0]].any()


def test_geometry_and_augmentation_are_shared_by_the_channels():
    g = np.random.default_rng(0)
    raw = (g.random((3, 8, 16, 4), dtype=np.float32) * 100).astype(np.float32)
    raw[..., 0][g.random((3, 8, 16)) < 0.2] = 0
    scale, gate = D.DATASET_PREP["durlar"]
    lo, hi = PC.prep_channels(raw, scale, gate, True, 3, [0.01, 0.02], [True, False], f=4, fw=2, row_phase=1, col_phase=1,
                              roll_shift=5)
    lo0, hi0 = PC.prep_channels(raw, scale, gate, True, 3, [0.01, 0.02], [True, False])
    assert lo.shape == (3, 3, 2, 8)
    assert np.array_equal(bits(hi), bits(np.roll(hi0, 5, -1)))
    assert np.array_equal(bits(lo), bits(np.roll(hi0[:, :, 1::4, 1::2], 5, -1)))
    # the draws do not depend on C: applying the definition to all channels is applying it to each
    alo, ahi = A.apply(hi0, 0, [5, 6, 7], 4, beam_drop=0.3, point_drop=0.3)
    for c in range(3):
        clo, chi = A.apply(hi0[:, c:c + 1], 0, [5, 6, 7], 4, beam_drop=0.3, point_drop=0.3)
        assert np.array_equal(bits(alo[:, c:c + 1]), bits(clo)) and np.array_equal(bits(ahi[:, c:c + 1]), bits(chi))
    dropped = A.beam_mask(0, [5, 6, 7], 2, 0.3)[:, :, None] | A.point_mask(0, [5, 6, 7], 2, 16, 0.3)
    assert dropped.any() and not bits(alo)[np.broadcast_to(dropped[:, None], alo.shape)].any()
    with pytest.raises(ValueError):
        PC.prep_channels(raw[..., :2], scale, gate, True, 3)
    with pytest.raises(ValueError):
        PC.prep_channels(raw, scale, gate, True, 3, [1.0])


# ---------------------------------------------------------------------------------------------------- 2. refusals
def test_default_is_the_single_channel_object():
    p = D.RangePrep("kitti", (2, 16), (8, 16), True)
    assert p.in_chans == 1 and p.channel_scale == () and p.channel_log == ()
    p = D.RangePrep("kitti", (2, 16), (8, 16), True, in_chans=3)
    assert p.channel_scale == (1.0, 1.0) and p.channel_log == (False, False)
    p = D.RangePrep("kitti", (2, 16), (8, 16), True, in_chans=3, channel_scale=[1 / 255, 2], channel_log=(True, False))
    assert p.channel_scale == (1 / 255, 2.0) and p.channel_log == (True, False)


@pytest.mark.parametrize("kw", [dict(in_chans=0), dict(in_chans=5), dict(in_chans=True), dict(in_chans=2.0),
                                dict(in_chans=2, channel_scale=[True]), dict(in_chans=2, channel_scale=[NAN]),
                                dict(in_chans=2, channel_scale=[INF]), dict(in_chans=3, channel_scale=[1.0, -INF]),
                                dict(in_chans=2, channel_scale=["1"]), dict(in_chans=2, channel_scale=[1.0, 1.0]),
                                dict(in_chans=3, channel_scale=[1.0]), dict(in_chans=1, channel_scale=[1.0]),
                                dict(in_chans=2, channel_scale=[]), dict(in_chans=2, channel_log=[]),
                                dict(in_chans=2, channel_log=[True, False]), dict(in_chans=4, channel_log=[True]),
                                dict(in_chans=1, channel_log=[False]), dict(in_chans=2, channel_log=[1])])
def test_constructor_refuses(kw):
    with pytest.raises(ValueError):
        D.RangePrep("kitti", (2, 16), (8, 16), True, **kw)


def test_call_refuses_before_the_device_is_touched():
    """CPU tensors: a call that got as far as the device would raise RuntimeError (no CPU fallback), not ValueError"""
    p = D.RangePrep("kitti", (2, 16), (8, 16), True, in_chans=3)
    with pytest.raises(ValueError, match="in_chans=3"):
        p(torch.zeros(2, 8, 16))                                    # 3-D raw
    with pytest.raises(ValueError, match="in_chans=3"):
        p(torch.zeros(2, 8, 16, 2))                                 # Cr < C
    with pytest.raises(ValueError, match="rimg"):
        p.from_rimg(torch.zeros(2, 16, 8, dtype=torch.float16))
    with pytest.raises(ValueError, match="sample_ids"):             # the keywords of before keep their checks
        p(torch.zeros(2, 8, 16, 3), sample_ids=[1, 2])
    with pytest.raises(RuntimeError, match="GPU only"):
        p(torch.zeros(2, 8, 16, 4))                                 # extra raw channels are fine: this one reaches the device check
    # in_chans=1 takes what it took
    with pytest.raises(RuntimeError, match="GPU only"):
        D.RangePrep("kitti", (2, 16), (8, 16), True)(torch.zeros(2, 8, 16))


def test_loader_refuses_rimg_files(tmp_path):
    (tmp_path / "a.rimg").write_bytes(np.array([8, 16], dtype=np.uint).tobytes() + np.zeros(128, np.float16).tobytes())
    ld = D.DeviceRangeLoader(str(tmp_path), D.RangePrep("carla", (2, 16), (8, 16), True, in_chans=2), 1, device="cpu")
    with pytest.raises(ValueError, match="rimg"):
        next(iter(ld))


# ---------------------------------------------------------------------------------------------------- 3. the C ABI
def header_args():
    src = open(os.path.join(ROOT, "include", "tulip_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(tulip_range_prep\w*)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        out[m.group(1)] = [" ".join(a.split()) for a in m.group(2).split(",")]
    return out


TRAILING = ["int C", "int64_t chan_stride", "const float* chan_scale", "uint32_t chan_log"]
PAIRS = (("tulip_range_prep", "tulip_range_prep_c"), ("tulip_range_prep_aug", "tulip_range_prep_aug_c"))


def test_header_signature_and_argument_counts_agree():
    decl = header_args()
    for old, new in PAIRS:
        assert new in decl, f"{new} is not declared in tulip_hip.h"
        assert decl[new] == decl[old] + TRAILING                    # the leading arguments are the existing entry point's
        assert len(_lib.SIGNATURES[new]) == len(decl[new])
        assert _lib.SIGNATURES[new][:len(decl[old])] == _lib.SIGNATURES[old]
        assert _lib.SIGNATURES[new][len(decl[old]):] == [ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint32]
    hdr = open(os.path.join(ROOT, "include", "tulip_hip.h")).read()
    assert int(re.search(r"#define TULIP_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 6      # additive: no bump


def test_both_builds_export_both_symbols_at_abi_6():
    from tulip_amd.csrc.build import build
    build(force=False, verbose=False)
    lib = _lib.load()
    with _lib.dev_library() as dev:
        assert dev is not lib and dev.tulip_dev_variants() == 1 and lib.tulip_dev_variants() == 0
        for L in (lib, dev):
            assert L.tulip_abi_version() == 6
            for _, new in PAIRS:
                assert hasattr(L, new), new


def _plain_args(raw=4096, dtype=0, hi=8192, lo=12288, C=2, sc=1, scales=True, log=0, H=8, W=16, sj=2):
    s = (ctypes.c_float * 3)(1.0, 1.0, 1.0) if scales else None
    return [raw, dtype, H * W * sj, W * sj, sj, 0, hi, lo, 2, H, W, 4, 1, 0, 0, 0.0125, 0, 0.0, 0.0, 1, 0, None, C, sc, s, log]


def _aug_args(ids=16384, flags=7, **kw):
    a = _plain_args(**kw)
    return a[:20] + [ids, 0, flags, 0, 0, None] + a[21:]


@pytest.mark.parametrize("build_name", ["product", "dev"])
def test_argument_errors_come_before_any_launch(build_name):
    """every refused call returns TULIP_ERR_ARG (-1) on a machine with no GPU: nothing was launched, no pointer was followed (the
    device pointers here are made-up numbers)"""
    from tulip_amd.csrc.build import build
    build(force=False, verbose=False)
    bad = [dict(C=0), dict(C=-1), dict(C=5), dict(scales=False), dict(scales=False, C=4), dict(dtype=1), dict(dtype=2),
           dict(log=2), dict(C=3, log=4), dict(C=1, log=1),                     # flag bits of channels that are not there
           dict(raw=None), dict(hi=None, lo=None), dict(H=7), dict(W=0)]        # what tulip_range_prep refuses
    def run(lib):
        for kw in bad:
            assert lib.tulip_range_prep_c(*_plain_args(**kw)) == -1, kw
            assert lib.tulip_range_prep_aug_c(*_aug_args(**kw)) == -1, kw
        for kw in (dict(ids=None), dict(ids=16388), dict(flags=8)):             # what tulip_range_prep_aug refuses
            assert lib.tulip_range_prep_aug_c(*_aug_args(**kw)) == -1, kw
    if build_name == "dev":
        with _lib.dev_library() as dev:
            run(dev)
    else:
        run(_lib.load())

"""CPU: the dense-cloud definition (tulip_amd/cloud.py) against the reference-pinned oracle and its corner rules, the C ABI of
csrc/cloud.hip (symbols, signatures, refusals before any launch), CloudUpsampler's argument errors, and the self-check of the
cases tests/test_cloud_gpu.py runs."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import eval_oracle as EO
from tests import cloud_cases as CC
from tulip_amd import _lib
from tulip_amd import cloud as CL
from tulip_amd import evaluation as EV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ the definition against the oracle
SIZES = {"kitti": (64, 1024, 16, 1024), "carla": (32, 256, 8, 256), "durlar": (32, 256, 8, 256)}


@pytest.mark.parametrize("log_transform", [False, True])
@pytest.mark.parametrize("dataset", ["kitti", "carla", "durlar"])
def test_definition_is_the_oracles_cloud_without_the_no_return_rows(golden_dir, dataset, log_transform):
    H, W, h, w = SIZES[dataset]
    pred, hi, lo = EO.synthetic_eval_case(dataset, H, W, h, w, seed=77, log_transform=log_transform)
    _, _, p_img, _ = EO.postprocess(pred, hi, lo, dataset, log_transform)
    cloud, planes = CL.image_cloud(pred[0].numpy(), lo[0].numpy(), dataset, log_transform)
    assert cloud.dtype == np.float32 and cloud.shape[1] == 3
    if dataset == "durlar":
        lut = np.load(os.path.join(golden_dir, "g10_eval.npz"))["durlar_elevation_lut"]
        pcd = EO.durlar_pcd(p_img, lut[:H], 120)                             # float64, destination order
        dst = (np.arange(W)[None, :] + W - EO.DURLAR_OFFSET_LUT[:H][:, None]) % W
        img_dst = np.empty_like(p_img)
        np.put_along_axis(img_dst, dst, p_img, axis=1)
        want = pcd[img_dst.reshape(-1) > 0].astype(np.float32)              # rounded once
    else:
        tables = EO.kitti_tables() if dataset == "kitti" else EO.carla_tables(H, W)
        pcd = EO.spherical_pcd(p_img, tables, EO.MAX_RANGE[dataset])
        assert pcd.dtype == np.float32
        img_dst = p_img
        want = pcd[p_img.reshape(-1) > 0]
    assert np.array_equal(bits(planes[0]), bits(img_dst))
    assert 0.5 * H * W < want.shape[0] < H * W                               # the case has no-return pixels, and not only those
    assert cloud.shape == want.shape and np.array_equal(bits(cloud), bits(want))


def test_batch_is_the_concatenation_with_offsets():
    pred, hi, lo = EO.synthetic_eval_case("carla", 16, 64, 4, 64, seed=3, log_transform=False)
    p = np.stack([pred[0, 0].numpy(), np.zeros((16, 64), F32), pred[0, 0].numpy()[::-1].copy()])[:, None]
    l = np.stack([lo[0, 0].numpy(), np.zeros((4, 64), F32), lo[0, 0].numpy()])[:, None]
    points, offsets, planes = CL.batch_cloud(p, l, "carla")
    assert offsets.dtype == np.int64 and offsets.shape == (4,) and offsets[0] == 0
    assert offsets[1] == offsets[2] and offsets[3] == points.shape[0] > offsets[1] > 0          # the empty image in the middle
    for b in range(3):
        assert np.array_equal(bits(points[offsets[b]:offsets[b + 1]]), bits(CL.image_cloud(p[b], l[b], "carla")[0]))
    assert planes.shape == (3, 1, 16, 64)


# ------------------------------------------------------------------ corner rules, hand-made images
GATE = EV.pred_gate("carla", False)           # (0.025, 1.0)


def one_plane(values, H=4, W=8):
    img = np.full((H, W), F32(0.5))
    img.reshape(-1)[:len(values)] = np.asarray(values, dtype=F32)
    return img[None]


def test_specials_in_the_prediction():
    vals = [-0.0, np.nan, np.inf, -np.inf, 0.0, 0.3]
    pred = one_plane(vals)
    lo = np.zeros((1, 2, 4), F32)                                            # w != W: nothing is restored
    planes = CL.range_planes(pred, lo, False, None, GATE)
    flat = planes[0].reshape(-1)
    assert np.array_equal(bits(flat[:5]), bits(np.zeros(5, F32)))            # all become +0.0 (the gate's select), the -0.0 too
    cloud, pl = CL.image_cloud(pred, lo, "carla")
    assert cloud.shape[0] == 4 * 8 - 5 and np.isfinite(cloud).all()


def test_values_on_both_gate_bounds_are_kept():
    gmin, gmax = F32(GATE[0]), F32(GATE[1])
    vals = [gmin, np.nextafter(gmin, F32(0)), gmax, np.nextafter(gmax, F32(2))]
    planes = CL.range_planes(one_plane(vals), np.zeros((1, 2, 4), F32), False, None, GATE)
    assert np.array_equal(bits(planes[0].reshape(-1)[:4]), bits(np.array([gmin, 0, gmax, 0], F32)))


def test_restored_rows_are_not_gated():
    pred = one_plane([], H=4, W=8)
    lo = np.zeros((1, 2, 8), F32)
    lo[0, 0, :4] = [0.0, 1.5, -0.0, np.nan]                                  # KITTI's ungated input: 1.5 = 120 m
    lo[0, 1] = 0.01                                                          # under the gate, kept all the same
    cloud, planes = CL.image_cloud(pred, lo, "carla")
    assert np.array_equal(bits(planes[0, 0]), bits(lo[0, 0])) and np.array_equal(bits(planes[0, 2]), bits(lo[0, 1]))
    kept_row0 = planes[0, 0] > 0
    assert kept_row0.tolist() == [False, True, False, False] + [False] * 4
    assert cloud.shape[0] == 1 + 8 + 16                                      # 1.5; the 0.01 row; the two prediction rows
    tables = EO.carla_tables(4, 8)
    assert np.array_equal(bits(cloud[0]), bits(EO.spherical_pcd(planes[0], tables, 80)[1]))


def test_keep_close_zeroes_the_pixel_in_every_channel():
    pred = np.stack([one_plane([0.2, 0.3, 0.25])[0], np.full((4, 8), F32(7.0))])
    lo = np.zeros((2, 2, 4), F32)
    planes = CL.range_planes(pred, lo, False, (False,), GATE, keep_close=0.25)
    assert planes[0].reshape(-1)[:3].tolist() == [F32(0.2), 0.0, F32(0.25)]         # above it, not at it
    assert planes[1].reshape(-1)[:3].tolist() == [7.0, 0.0, 7.0] and not planes[:, 1:].any()      # 0.5 everywhere else
    assert CL.image_cloud(pred, lo, "carla", False, (False,), GATE, 0.25)[0].shape == (2, 4)


def test_no_restore_when_the_widths_differ():
    pred = one_plane([], H=4, W=8)
    lo = np.zeros((1, 2, 4), F32)
    assert CL.image_cloud(pred, lo, "carla")[0].shape[0] == 32
    assert CL.image_cloud(pred, np.zeros((1, 2, 8), F32), "carla")[0].shape[0] == 16


def test_a_hole_zeroes_the_attribute_channels_nan_included():
    rng0 = one_plane([0.3, 0.001, np.nan, 0.3])
    attr = one_plane([2.0, 3.0, np.nan, np.nan])
    pred = np.concatenate([rng0, attr, np.log1p(attr)])
    planes = CL.range_planes(pred, np.zeros((3, 2, 4), F32), False, (False, True), GATE)
    a1, a2 = planes[1].reshape(-1)[:4], planes[2].reshape(-1)[:4]
    assert np.array_equal(bits(a1[:3]), bits(np.array([2.0, 0.0, 0.0], F32))) and np.isnan(a1[3])   # outside a hole a NaN stays
    assert abs(a2[0] - 2.0) <= 2.0 ** -22 and np.array_equal(bits(a2[1:3]), bits(np.zeros(2, F32))) and np.isnan(a2[3])
    cloud = CL.project_planes(planes, "carla")
    assert cloud.shape == (30, 5) and np.array_equal(bits(cloud[0, 3:]), bits(np.array([a1[0], a2[0]])))
    assert np.isnan(cloud[1, 3])                                             # the kept pixel with the NaN attribute: row 1


def test_log_transform_inverts_both_inputs():
    pred = np.log1p(one_plane([0.3, 0.01], H=4, W=8))
    lo = np.log1p(np.full((1, 2, 8), F32(0.7)))
    planes = CL.range_planes(pred, lo, True, None, GATE)
    assert np.array_equal(bits(planes[0, 0]), bits(torch.expm1(torch.from_numpy(lo[0, 0])).numpy())) and abs(planes[0, 1, 0] - 0.5) <= 2.0 ** -23
    wide = CL.range_planes(pred, lo, True, None, GATE, wide=True)
    assert wide.dtype == np.float64 and np.abs(wide - planes).max() <= 2.0 ** -24


def test_definition_refuses_malformed_images():
    z = np.zeros((1, 4, 8), F32)
    for pred, lo in ((z.astype(np.float64), z), (z[0], z), (z, np.zeros((2, 2, 8), F32)), (z, np.zeros((1, 3, 8), F32)),
                     (np.zeros((5, 4, 8), F32), np.zeros((5, 2, 8), F32))):
        with pytest.raises(ValueError):
            CL.range_planes(pred, lo, False, None, GATE)
    with pytest.raises(ValueError):
        CL.range_planes(np.zeros((2, 4, 8), F32), np.zeros((2, 2, 8), F32), False, (True, False), GATE)


# ------------------------------------------------------------------ C ABI
NEW = ("tulip_cloud_tile", "tulip_cloud_spherical", "tulip_cloud_durlar")
FAKE, E = 4096, -1


def test_symbols_signatures_and_version():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tulip_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    assert lib.tulip_abi_version() == _lib.ABI_VERSION == 6 and re.search(r"#define\s+TULIP_ABI_VERSION\s+6\b", hdr)
    with _lib.dev_library() as dev:
        for name in NEW:
            assert hasattr(dev, name), name
        assert dev.tulip_cloud_tile() == lib.tulip_cloud_tile()
    for name in NEW:
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        args = m.group(1).strip()
        assert len(_lib.SIGNATURES[name]) == (0 if args in ("", "void") else args.count(",") + 1), name
    T = lib.tulip_cloud_tile()
    assert T > 0 and T % 256 == 0


def _sph(lib, B=2, C=2, H=8, W=16, h=2, w=16, bits_=0, **null):
    names = ("pred", "lo", "sin_h", "cos_h", "sin_v", "cos_v", "rng", "counts", "tile_offsets", "offsets", "points")
    p = {k: (None if null.get(k) else FAKE) for k in names}
    return lib.tulip_cloud_spherical(p["pred"], p["lo"], B, C, H, W, h, w, 0, bits_, 0.0, 1.0, 0.0, 80.0, p["sin_h"], p["cos_h"],
                                     p["sin_v"], p["cos_v"], p["rng"], p["counts"], p["tile_offsets"], p["offsets"], p["points"],
                                     None), names


def _dur(lib, B=2, C=2, H=8, W=16, h=2, w=16, bits_=0, **null):
    names = ("pred", "lo", "col_tables", "row_tables", "row_offset", "rng", "counts", "tile_offsets", "offsets", "points")
    p = {k: (None if null.get(k) else FAKE) for k in names}
    return lib.tulip_cloud_durlar(p["pred"], p["lo"], B, C, H, W, h, w, 0, bits_, 0.0, 1.0, 0.0, 120.0, p["col_tables"],
                                  p["row_tables"], p["row_offset"], 0.015806, 0.03618, p["rng"], p["counts"], p["tile_offsets"],
                                  p["offsets"], p["points"], None), names


@pytest.mark.parametrize("entry", [_sph, _dur])
def test_refused_arguments_return_before_any_launch(entry):
    """every call below carries a dummy pointer or a refused size: TULIP_ERR_ARG comes back without a launch (there is no GPU here)"""
    lib = _lib.load()
    _, names = entry(lib, B=0)
    for k in names:
        assert entry(lib, **{k: True})[0] == E, k
    call = lambda **kw: entry(lib, **kw)[0]
    assert call(C=0) == E and call(C=5) == E and call(C=-1) == E
    assert call(H=9) == E and call(h=3) == E                                  # H % h
    assert call(B=0) == E and call(B=-1) == E and call(H=0) == E and call(W=0) == E and call(h=0) == E and call(w=0) == E
    assert call(H=-8, h=-2) == E and call(W=-16) == E
    assert call(C=1, bits_=1) == E and call(C=2, bits_=2) == E and call(C=3, bits_=4) == E and call(C=4, bits_=8) == E


# ------------------------------------------------------------------ CloudUpsampler's argument errors (no GPU needed)
def _model(C=1, lo=(8, 256), hi=(32, 256)):
    return SimpleNamespace(in_chans=C, img_size=lo, target_img_size=hi)


def test_cloud_upsampler_argument_errors():
    mk = lambda model=None, ds="carla", B=2, **kw: CL.CloudUpsampler(model or _model(), ds, B, device="cpu", **kw)
    with pytest.raises(NotImplementedError, match="Cannot find the dataset"):
        mk(ds="nuscenes")
    with pytest.raises(ValueError, match="cannot reshape array"):             # the evaluator's KITTI size check
        mk(ds="kitti")
    with pytest.raises(IndexError, match="out of bounds"):                    # the evaluator's DurLAR row limit
        mk(_model(1, (64, 256), (256, 256)), ds="durlar")
    for bad in (0, -1, 2.0, True, None, "2"):
        with pytest.raises(ValueError, match="batch_size"):
            mk(B=bad)
    with pytest.raises(ValueError, match="channel_log"):
        mk(channel_log=[True])                                                # one channel has no flags
    for C, logs in ((2, [True, False]), (3, [True]), (2, [1]), (2, "T")):
        with pytest.raises(ValueError, match="channel_log"):
            mk(_model(C), channel_log=logs)
    with pytest.raises(ValueError, match="in_chans"):
        mk(_model(5))
    for bad in (-0.1, float("nan"), "0.25", None, True):
        with pytest.raises(ValueError, match="keep_close"):
            mk(keep_close=bad)
    for bad in (0.5, (0.0,), (0.0, 1.0, 2.0), "ab", (None, 1.0)):
        with pytest.raises(ValueError, match="gate"):
            mk(gate=bad)
    with pytest.raises(ValueError, match="multiple"):
        mk(_model(1, (8, 256), (30, 256)))
    with pytest.raises(RuntimeError, match="GPU only"):                       # valid arguments reach the device check, and only then
        mk(_model(2), channel_log=[True], keep_close=0.25, gate=(0.0, 1.0))


# ------------------------------------------------------------------ self-check of the GPU cases
def _T():
    return _lib.load().tulip_cloud_tile()


def test_gpu_cases_cover_what_they_claim():
    T = _T()
    cases = CC.kernel_cases(T)
    assert len({c.name for c in cases}) == len(cases)
    tiles = lambda c: -(-(c.H * c.W) // T)
    assert any(c.H * c.W < T for c in cases) and any(c.H * c.W == 2 * T for c in cases)
    part = [c for c in cases if c.H * c.W == T + 476]
    assert part and (T + 476) % 64 and {c.pattern for c in part if c.B == 3 and c.C == 1 and not c.log} >= set(CC.PATTERNS)
    assert any(c.B * tiles(c) > 256 and c.B == 5 and c.H * c.W == 64 * T for c in cases)
    assert {c.B for c in cases} >= {1, 3} and {c.C for c in cases} >= {1, 2, 4}
    assert any(c.w != c.W for c in cases) and any(c.keep_close > 0 for c in cases)
    dur = [c for c in cases if c.dataset == "durlar"]
    assert dur and all((c.H, c.W) == (8, 96) for c in dur)
    assert max(EV.DURLAR_PIXEL_OFFSET[:8]) > 0 and (CL.destination_columns("durlar", 8, 96)[0] != np.arange(96)).all()
    assert (CL.destination_columns("durlar", 8, 96)[0, :48] > 47).all()        # the rotation crosses the row end
    assert any(c.log and not any(c.channel_log) for c in cases) and any(c.log and any(c.channel_log) for c in cases)
    assert all(c.keep_close == 0 for c in cases if c.log)


@pytest.mark.parametrize("name", CC.case_names())
def test_gpu_case_inputs(name):
    """the 4-ulp gate margin of the log cases, and the patterns are what the host definition keeps"""
    T = _T()
    assert CC.case_names(T) == CC.case_names()
    for pattern in (None, "sparser"):
        pb = CC.problem(name, T, pattern)
        CC.assert_gate_margin(pb)
        CC.assert_planted(pb)
        c = pb.case
        assert pb.pred.shape == (c.B, c.C, c.H, c.W) and pb.lo.shape == (c.B, c.C, c.h, c.w)
        assert pb.counts.sum() == pb.offsets[-1] and pb.counts.shape == (c.B * -(-(c.H * c.W) // T),)
        if pattern is None:
            n = c.H * c.W
            want = {"all": c.B * n, "none": 0, "none_middle": (c.B - 1) * n, "alternating": c.B * ((n + 1) // 2),
                    "lane63": c.B * (n // 64), "tile_first": c.B * -(-n // T), "last_pixel": 1}.get(c.pattern)
            assert want is None or pb.offsets[-1] == want
            if c.pattern == "none_middle":
                assert pb.offsets[c.B // 2] == pb.offsets[c.B // 2 + 1]
            if c.pattern == "random":
                assert 0.4 * c.B * n < pb.offsets[-1] < 0.6 * c.B * n
        else:
            assert pb.offsets[-1] < CC.problem(name, T).offsets[-1] or CC.problem(name, T).offsets[-1] < 0.2 * c.B * c.H * c.W
        if not c.log and c.keep_close == 0 and pb.offsets[-1] >= 1000:         # exact hits on both (inclusive) gate bounds are kept
            kept = pb.planes[:, 0][pb.planes[:, 0] > 0]
            assert (kept == F32(c.gate[0])).any() and (kept == F32(c.gate[1])).any()

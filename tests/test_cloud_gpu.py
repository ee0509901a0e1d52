"""GPU: csrc/cloud.hip and CloudUpsampler against the host definition (tulip_amd/cloud.py) and the evaluator's own clouds.

Kernel level (tests/cloud_cases.py): synthetic (pred, lo) through ops.cloud_spherical / ops.cloud_durlar into NaN-prefilled,
guarded buffers; offsets, counts, the post-processed planes and every row are compared with the host definition bit for bit, the
rows at or beyond offsets[B] and the guard words must keep their pre-fill.  Planes stored as log1p: the planes within 2 fp32 ulp
of the chain with a float64 expm1 (the budget tests/eval_exact.py uses for this expm1f), the rows bit for bit the host projection
of the device's own planes.

Model level: CloudUpsampler's graph against RangeEvaluator / ChannelEvaluator fed with the module's forward, image by image."""
import numpy as np
import pytest
import torch

from oracle import tulip_oracle as O
from tests import cloud_cases as CC
from tulip_amd import cloud as CL
from tulip_amd import evaluation as EV
from tulip_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("name", CC.case_names())
def test_kernels_against_the_host_definition(name):
    T = ops.cloud_tile()
    assert T > 0 and T % 256 == 0 and CC.case_names(T) == CC.case_names()
    pb = CC.problem(name, T)
    bufs = CC.alloc_outputs(pb.case, T, DEV)
    CC.launch(pb, bufs, DEV)
    bad = CC.check(pb, bufs)
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", ["partial-B3-C1-all", "two_tiles-B3-C4-tile_first", "scan2-B5-C1-random", "durlar-B2-C1-random"])
def test_second_call_into_the_same_buffers(name):
    """a sparser pattern after a denser one: counts, offsets, planes and rows are the sparser pattern's; what lies beyond the
    first call's rows was never written"""
    T = ops.cloud_tile()
    first, second = CC.problem(name, T), CC.problem(name, T, "sparser")
    bufs = CC.alloc_outputs(first.case, T, DEV)
    CC.launch(first, bufs, DEV)
    assert not CC.check(first, bufs)
    CC.launch(second, bufs, DEV)
    bad = CC.check(second, bufs, untouched_from=int(max(first.offsets[-1], second.offsets[-1])))
    assert not bad, (name, bad)


# ------------------------------------------------------------------ model level
def build(cfg, seed):
    from functools import partial
    import torch.nn as nn
    from tulip_amd.model import tulip as T
    m = T.TULIP(img_size=cfg.img_size, target_img_size=cfg.target_img_size, patch_size=cfg.patch_size, in_chans=cfg.in_chans,
                embed_dim=cfg.embed_dim, window_size=list(cfg.window_size), depths=cfg.depths, num_heads=cfg.num_heads,
                mlp_ratio=cfg.mlp_ratio, drop_path_rate=cfg.drop_path_rate, norm_layer=partial(nn.LayerNorm, eps=cfg.ln_eps),
                pixel_shuffle=cfg.pixel_shuffle, circular_padding=cfg.circular_padding, log_transform=cfg.log_transform,
                patch_unmerging=cfg.patch_unmerging)
    m.load_state_dict(O.key_seeded_state_dict(cfg, seed=seed), strict=True)
    return m.to(DEV).eval()


MODELS = {
    "carla": (lambda: O.tiny_config(drop_path_rate=0.0), True),
    "durlar": (lambda: O.tiny_config(drop_path_rate=0.0), False),
    "kitti": (lambda: O.tulip_base_config(img_size=(16, 1024), target_img_size=(64, 1024), drop_path_rate=0.0), True),
}


def evaluator_cloud(ev, dataset, pred_b, lo_b):
    """the evaluator's pcd_pred rows at the pixels whose post-processed range is > 0, as float32 (DurLAR: rounded once, the mask
    taken to pcd row order)"""
    ev.point_clouds(pred_b, lo_b, torch.zeros_like(pred_b))
    img = ev.pred_img if ev.pred_img.dim() == 2 else ev.pred_img[0]
    if dataset == "durlar":
        mask = torch.from_numpy(CL.to_destination(img.cpu().numpy(), dataset)).reshape(-1) > 0
        return ev.pcd_pred.cpu()[mask].float(), mask
    mask = img.reshape(-1).cpu() > 0
    return ev.pcd_pred.cpu()[mask], mask


@pytest.mark.parametrize("dataset", ["carla", "durlar", "kitti"])
def test_upsampler_equals_the_evaluators_cloud(dataset):
    make, log_t = MODELS[dataset]
    cfg = make()
    m = build(cfg, seed=5)
    B = 2
    up = CL.CloudUpsampler(m, dataset, B, log_transform=log_t)
    ev = EV.RangeEvaluator(dataset, cfg.img_size, cfg.target_img_size, log_t, device=DEV)
    for seed in (11, 12):                                   # the second replay has another input
        lo, hi = O.synthetic_batch(cfg, B, seed=seed)
        lo, hi = lo.to(DEV), hi.to(DEV)
        if not log_t:
            lo = torch.expm1(lo)
        with torch.no_grad():
            pred = m(lo, hi, mc_drop=True).clone()
        points, offsets = up(lo)
        assert points.shape == (B * cfg.target_img_size[0] * cfg.target_img_size[1], 3) and offsets.shape == (B + 1,)
        assert points.dtype == torch.float32 and offsets.dtype == torch.int64 and points.is_cuda and offsets.is_cuda
        clouds = up.clouds()
        assert len(clouds) == B and int(offsets[0]) == 0
        for b in range(B):
            want, mask = evaluator_cloud(ev, dataset, pred[b:b + 1], lo[b:b + 1])
            got = clouds[b].cpu()
            assert int(mask.sum()) > cfg.img_size[0] * cfg.img_size[1] // 2            # the restored rows at least
            assert got.shape == want.shape, (dataset, seed, b, got.shape, want.shape)
            assert torch.equal(bits(got), bits(want)), (dataset, seed, b)
            plane = up.range_images[b, 0].cpu().numpy()
            assert np.array_equal(plane.view(np.uint32),
                                  CL.to_destination((ev.pred_img.cpu().numpy()), dataset).view(np.uint32))


def test_upsampler_attribute_column_is_the_channel_evaluators_plane():
    cfg = O.tiny_config(drop_path_rate=0.0, in_chans=2)
    m = build(cfg, seed=6)
    B, logs = 2, (True,)
    up = CL.CloudUpsampler(m, "carla", B, log_transform=True, channel_log=logs)
    ev = EV.ChannelEvaluator("carla", cfg.img_size, cfg.target_img_size, True, 2, logs, device=DEV)
    lo, hi = O.synthetic_batch(cfg, B, seed=21)
    lo, hi = lo.to(DEV), hi.to(DEV)
    with torch.no_grad():
        pred = m(lo, hi, mc_drop=True).clone()
    points, offsets = up(lo)
    assert points.shape[1] == 4
    clouds = up.clouds()
    for b in range(B):
        want_xyz, mask = evaluator_cloud(ev, "carla", pred[b:b + 1], lo[b:b + 1])
        want_attr = ev.pred_img[1].reshape(-1).cpu()[mask]
        got = clouds[b].cpu()
        assert got.shape == (int(mask.sum()), 4) and int(mask.sum()) > 0
        assert torch.equal(bits(got[:, :3]), bits(want_xyz)) and torch.equal(bits(got[:, 3]), bits(want_attr)), b


def test_from_pred_of_an_mc_aggregate():
    cfg = O.tiny_config(drop_path_rate=0.0)
    m = build(cfg, seed=7)
    up = CL.CloudUpsampler(m, "carla", 1, log_transform=False, keep_close=0.6)
    H, W = cfg.target_img_size
    g = torch.Generator().manual_seed(31)
    base = torch.rand(1, 1, H, W, generator=g)
    noise = 0.02 * torch.randn(10, 1, H, W, generator=g) * (torch.rand(1, 1, H, W, generator=g) < 0.4)
    preds = (base + noise).float().to(DEV)
    lo = torch.rand(1, 1, *cfg.img_size, generator=g).to(DEV)
    agg = EV.mc_aggregate(preds, 0.03)
    points, offsets = up.from_pred(agg, lo)
    want, want_off, planes = CL.batch_cloud(agg.cpu().numpy(), lo.cpu().numpy(), "carla", False, None, None, 0.6)
    off = offsets.cpu().numpy()
    assert np.array_equal(off, want_off) and 0 < off[1] < H * W
    assert (agg == 0).sum() > 0 and (planes[0, 0] == 0).sum() > int((agg == 0).sum().cpu())     # dropped, gated and keep_close pixels
    assert np.array_equal(up.clouds()[0].cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(up.range_images.cpu().numpy().view(np.uint32), planes.view(np.uint32))


def test_upsampler_refuses_wrong_batches():
    cfg = O.tiny_config(drop_path_rate=0.0)
    m = build(cfg, seed=7)
    up = CL.CloudUpsampler(m, "carla", 2)
    h, w = cfg.img_size
    for bad in (torch.zeros(2, 1, h, w), torch.zeros(1, 1, h, w, device=DEV), torch.zeros(2, 1, h, w, device=DEV).double(),
                torch.zeros(2, 2, h, w, device=DEV), np.zeros((2, 1, h, w), np.float32)):
        with pytest.raises(ValueError):
            up(bad)
    with pytest.raises(ValueError):
        up.from_pred(torch.zeros(2, 1, h, w, device=DEV), torch.zeros(2, 1, h, w, device=DEV))

"""CPU: upscale_factor 8 -- 16-pixel patches (2, 8) and (4, 4).

  1. the oracle reproduces the reference fixture g17_upscale (tests/golden/make_golden_upscale.py) for the five configs,
     within the bands of test_windows_cpu.test_oracle_matches_reference_fixture: the yardstick of the GPU tests is the reference;
  2. the drop-in TULIP has the reference's state_dict keys / order / shapes and seeded initialisation at these patch sizes;
  3. its engine builds without a GPU (the five configs, TULIP() with the constructor defaults, KITTI tulip_base and DurLAR
     tulip_large at (2, 8)); what is not built is refused when the engine is built, naming the limit;
  4. the library exports the head entry points with trailing (in_chans, r), and they refuse what is not built before any launch;
  5. a wrongly shaped target is a ValueError.
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import tulip_oracle as O
from tulip_amd import _lib

from tests import upscale_cases as UC

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
NAMES = UC.NAMES
NEW_SYMBOLS = ("tulip_tail_fwd_r", "tulip_tail_fwd_ln_r", "tulip_tail_bwd_r", "tulip_tail_bwd_dgrad_r", "tulip_tail_bwd_dgrad_ln_r",
               "tulip_tail_wgrad_r", "tulip_tail_wgrad_splits_r", "tulip_tail_fused_bwd_supported_r")


def fixture():
    z = np.load(os.path.join(GOLD, "g17_upscale.npz"), allow_pickle=False)
    with open(os.path.join(GOLD, "g17_upscale.json")) as f:
        return z, json.load(f)


def fixture_config(meta, name) -> O.TulipConfig:
    return O.TulipConfig(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in meta["configs"][name]["cfg"].items()})


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def make_model(cfg: O.TulipConfig, **kw):
    from tulip_amd.model import tulip as T
    return T.TULIP(**UC.model_kwargs(cfg), **kw)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_configs_are_what_the_cases_say(name):
    _, meta = fixture()
    cfg = fixture_config(meta, name)
    assert cfg == UC.config(name)
    UC.check_config(cfg)
    assert meta["batch"] == UC.BATCH and meta["seed"] == UC.SEED


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_reference_fixture(name):
    z, meta = fixture()
    cfg = fixture_config(meta, name)
    sd = O.key_seeded_state_dict(cfg, seed=meta["seed"])
    lo, hi = UC.batch(cfg, meta["batch"], seed=1234 + meta["seed"])
    pred, loss, pix, grads = O.tulip_loss_and_grads(sd, cfg, lo, hi)
    assert tuple(pred.shape) == tuple(z[f"{name}::pred_shape"].tolist()) == tuple(hi.shape)
    assert abs(loss.item() - float(z[f"{name}::loss"])) <= 1e-5 * float(z[f"{name}::loss"])
    assert abs(pix.item() - float(z[f"{name}::pixel_loss"])) <= 1e-5 * float(z[f"{name}::pixel_loss"])
    got = pred.reshape(-1)[torch.from_numpy(z[f"{name}::pred_index"])].numpy()
    assert np.abs(got - z[f"{name}::pred"]).max() <= 1e-5
    for k in meta["configs"][name]["grad_keys"]:
        assert rel_l2(grads[k], z[f"{name}::grad::{k}"]) <= 1e-4, k
    for k, step in meta["configs"][name]["grad_rows"].items():
        assert rel_l2(grads[k][::step], z[f"{name}::grad_rows::{k}"]) <= 1e-4, k
    for k, l2 in zip(z[f"{name}::grad_keys"].tolist(), z[f"{name}::grad_l2"]):
        assert abs(grads[k].double().norm().item() - l2) <= 1e-4 * l2 + 1e-12, k


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_matches_reference_spec(name):
    _, meta = fixture()
    cfg = fixture_config(meta, name)
    m = make_model(cfg)
    assert m.upscale_factor == 8
    spec = O.state_dict_spec(cfg)
    sd = m.state_dict()
    assert list(sd.keys()) == list(spec.keys())
    for k, (shape, _) in spec.items():
        assert tuple(sd[k].shape) == tuple(shape), k
    kw = 8 if cfg.circular_padding else cfg.patch_size[1]
    assert tuple(sd["patch_embed.proj.weight"].shape) == (cfg.embed_dim, cfg.in_chans, cfg.patch_size[0], kw)
    assert tuple(sd[UC.expand_key(cfg)].shape)[0] == 64 * cfg.embed_dim
    m.load_state_dict(O.key_seeded_state_dict(cfg, seed=meta["seed"]), strict=True)


def test_seeded_init_matches_reference_at_patch_2x8():
    z, meta = fixture()
    cfg = fixture_config(meta, "ps8_p2x8")
    torch.manual_seed(0)
    sd = make_model(cfg).state_dict()
    step = meta["init_row_step"]
    for k in ("patch_embed.proj.weight", "ps_head.conv_expand.0.weight"):
        want = torch.from_numpy(z[f"init_ps8_p2x8::{k}"])
        got = sd[k][::step] if sd[k].shape[0] > 48 else sd[k]
        assert torch.equal(got, want), k


@pytest.mark.parametrize("name", NAMES)
def test_engine_builds_without_gpu(name):
    from tulip_amd.engine import TulipEngine
    _, meta = fixture()
    cfg = fixture_config(meta, name)
    m = make_model(cfg)
    m.load_state_dict(O.key_seeded_state_dict(cfg, seed=meta["seed"]), strict=True)
    eng = TulipEngine(m)
    assert eng.model.upscale_factor == 8
    assert eng.output_shape(2) == (2, cfg.in_chans) + UC.output_size(cfg)


def test_constructor_defaults_engine_builds():
    """TULIP() as the reference constructs it by default: (4, 4) patches, 32x2048 -> an 8x512 grid -> a 64x4096 output image
    (not target_img_size (128, 2048): the target tensor decides)"""
    from tulip_amd.engine import TulipEngine
    from tulip_amd.model import tulip as T
    m = T.TULIP()
    assert m.upscale_factor == 8 and not m.pixel_shuffle
    eng = TulipEngine(m)
    assert eng.grid == (8, 512) and eng.output_shape(2) == (2, 1, 64, 4096)


@pytest.mark.parametrize("kind", ["kitti_base", "durlar_large"])
def test_full_size_2x8_engines_build(kind):
    from tulip_amd.engine import TulipEngine
    from tulip_amd.model import tulip as T
    kw = dict(patch_size=(2, 8), window_size=(2, 8), pixel_shuffle=True, circular_padding=True, log_transform=True,
              patch_unmerging=True)
    if kind == "kitti_base":
        m = T.tulip_base(img_size=(16, 1024), target_img_size=(64, 1024), **kw)
        grid = (8, 128)
    else:
        m = T.tulip_large(img_size=(32, 2048), target_img_size=(128, 2048), **kw)
        grid = (16, 256)
    eng = TulipEngine(m)
    assert eng.grid == grid and eng.output_shape(1)[2:] == tuple(m.target_img_size)


def test_upscale_16_refused_naming_the_supported_set():
    cfg = O.tiny_config(patch_size=(4, 16), img_size=(16, 512), target_img_size=(64, 512), circular_padding=False)
    assert cfg.upscale_factor == 16
    with pytest.raises(NotImplementedError, match="upscale_factor 4 and 8"):
        make_model(cfg).engine()


def test_upscale_2_refused_naming_the_supported_set():
    cfg = O.tiny_config(patch_size=(2, 2), img_size=(16, 128), target_img_size=(16, 128), circular_padding=False)
    assert cfg.upscale_factor == 2
    with pytest.raises(NotImplementedError, match="upscale_factor 4 and 8"):
        make_model(cfg).engine()


@pytest.mark.parametrize("kw, taps", [
    (dict(patch_size=(4, 4), circular_padding=True, embed_dim=64, num_heads=(2, 4)), 32),     # 32 taps outside E = 48 / 96
    (dict(patch_size=(2, 8), circular_padding=True, in_chans=3), 48),                           # more than 32 taps
    (dict(patch_size=(4, 4), circular_padding=True, in_chans=2), 64),
])
def test_tap_limit_refused_at_engine_build(kw, taps):
    cfg = O.tiny_config(img_size=(16, 512), target_img_size=(64, 512), **kw)
    with pytest.raises(NotImplementedError, match=f"{taps} taps"):
        make_model(cfg).engine()


def test_4x4_circular_single_channel_builds_at_embed_48():
    """(4, 4) patches with circular padding: kernel (4, 8), 32 taps -- covered at embed_dim 48 / 96 (the backward's 16-lane form)"""
    cfg = O.tiny_config(patch_size=(4, 4), img_size=(16, 256), target_img_size=(32, 512), circular_padding=True)
    make_model(cfg).engine()


def test_new_symbols_exported():
    lib = _lib.load()
    assert lib.tulip_abi_version() == 6
    for s in NEW_SYMBOLS:
        assert s in _lib.SIGNATURES, s
        assert getattr(lib, s) is not None, s


def test_abi_refuses_unbuilt_factors_and_widths_before_launching():
    """argument checks run on the host before any launch: no GPU needed"""
    lib = _lib.load()
    fake = 4096
    ln = (fake, fake, fake, 1e-6, fake, fake, fake, fake, fake, fake, fake, None, None, 0)
    dln = (fake, fake, fake, fake, fake, fake, 2, 8, 64)
    dln2 = (None, None, 1.0, fake, fake, fake, fake, fake, None, None, 1, None, None)
    for r, E, c in [(2, 96, 1), (16, 96, 1), (0, 96, 1), (6, 96, 2), (8, 136, 1), (8, 0, 1), (8, 96, 0), (8, 96, 5), (4, 96, 5)]:
        assert lib.tulip_tail_fwd_r(fake, fake, fake, fake, fake, 2, 8, 64, E, None, c, r) == -1, (r, E, c)
        assert lib.tulip_tail_bwd_r(fake, fake, fake, fake, fake, fake, fake, 2, 8, 64, E, None, None, 1.0, None, c, r) == -1
        assert lib.tulip_tail_bwd_dgrad_r(fake, fake, fake, fake, fake, fake, fake, 2, 8, 64, E, None, None, 1.0, None, c, r) == -1
        assert lib.tulip_tail_bwd_dgrad_ln_r(*dln, E, *dln2, c, r) == -1
        assert lib.tulip_tail_wgrad_r(fake, fake, fake, fake, fake, fake, fake, 2, 8, 64, E, None, None, 1.0, None, c, r) == -1
        assert lib.tulip_tail_fwd_ln_r(*ln, 2, 8, 64, E, None, c, r) == -1
        assert lib.tulip_tail_wgrad_splits_r(2, 8, 64, E, c, r) == 0
    # the fused backward pair needs E % 16 == 0 at either factor
    assert lib.tulip_tail_fused_bwd_supported_r(96, 8) == 1 and lib.tulip_tail_fused_bwd_supported_r(96, 4) == 1
    assert lib.tulip_tail_fused_bwd_supported_r(40, 8) == 0 and lib.tulip_tail_fused_bwd_supported_r(96, 2) == 0
    assert lib.tulip_tail_bwd_dgrad_r(fake, fake, fake, fake, fake, fake, fake, 2, 8, 64, 40, None, None, 1.0, None, 1, 8) == -1
    # the r = 4 plan is what the old query reports; r = 8 slices 4E virtual channels
    assert lib.tulip_tail_wgrad_splits_r(8, 16, 256, 96, 1, 4) == lib.tulip_tail_wgrad_splits(8, 16, 256, 96) == 64
    assert lib.tulip_tail_wgrad_splits_r(8, 8, 128, 96, 1, 8) == 16
    # empty batches are accepted (no launch) at r = 8
    assert lib.tulip_tail_fwd_r(fake, fake, fake, fake, fake, 0, 8, 64, 96, None, 4, 8) == 0
    # patch embedding: circular padding with 8-wide patches is kernel width 8; other widths stay refused
    pe = lambda p1, kw: lib.tulip_patch_embed_fwd(fake, fake, fake, fake, fake, fake, 0, 1, 16, 512, 48, 2, p1, kw, 1, 1e-6, None, 0, None)
    assert pe(8, 8) == 0 and pe(4, 8) == 0 and pe(8, 12) == -1 and pe(16, 8) == -1


@pytest.mark.parametrize("name", ["ps8_p4x4", "fe8_defaults"])
def test_wrongly_shaped_target_is_a_value_error(name):
    cfg = UC.config(name)
    eng = make_model(cfg).engine()
    good = torch.zeros(2, cfg.in_chans, *UC.output_size(cfg))
    eng.check_target(2, good)
    for bad in (torch.zeros(2, cfg.in_chans, *cfg.target_img_size) if tuple(cfg.target_img_size) != UC.output_size(cfg) else None,
                good.reshape(2, cfg.in_chans, good.shape[3], good.shape[2]), good[:, :, ::2], good[0]):
        if bad is None:
            continue
        with pytest.raises(ValueError, match="output shape") as e:
            eng.check_target(2, bad)
        assert str(tuple(bad.shape)) in str(e.value) and str(tuple(good.shape)) in str(e.value)

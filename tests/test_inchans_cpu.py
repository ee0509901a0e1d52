"""CPU: multi-channel images (in_chans 2 to 4).

  1. the oracle reproduces the reference fixture g16_inchans (tests/golden/make_golden_inchans.py) for in_chans 2, 3, 4;
  2. the drop-in TULIP has the reference's state_dict shapes and seeded initialisation at these channel counts;
  3. its engine builds without a GPU, and in_chans > 4 is refused when the engine is built, naming the limit;
  4. the library exports the head / FinalPatchExpanding entry points with a trailing in_chans, and they refuse what is
     not built before any launch.
"""
import json
import os
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import tulip_oracle as O
from tulip_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
NAMES = ("c2", "c3", "c4")
NEW_SYMBOLS = ("tulip_tail_fwd_c", "tulip_tail_fwd_ln_c", "tulip_tail_bwd_c", "tulip_tail_bwd_dgrad_c",
               "tulip_tail_bwd_dgrad_ln_c", "tulip_tail_wgrad_c", "tulip_expand_norm_fwd_c", "tulip_expand_norm_bwd_c")


def fixture():
    z = np.load(os.path.join(GOLD, "g16_inchans.npz"), allow_pickle=False)
    with open(os.path.join(GOLD, "g16_inchans.json")) as f:
        return z, json.load(f)


def fixture_config(meta, name) -> O.TulipConfig:
    return O.TulipConfig(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in meta["configs"][name]["cfg"].items()})


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def make_model(cfg: O.TulipConfig, **kw):
    from tulip_amd.model import tulip as T
    return T.TULIP(img_size=cfg.img_size, target_img_size=cfg.target_img_size, patch_size=cfg.patch_size,
                   in_chans=cfg.in_chans, embed_dim=cfg.embed_dim, window_size=list(cfg.window_size), depths=cfg.depths,
                   num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio, drop_path_rate=cfg.drop_path_rate,
                   norm_layer=partial(nn.LayerNorm, eps=cfg.ln_eps), pixel_shuffle=cfg.pixel_shuffle,
                   circular_padding=cfg.circular_padding, log_transform=cfg.log_transform,
                   patch_unmerging=cfg.patch_unmerging, **kw)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_reference_fixture(name):
    z, meta = fixture()
    cfg = fixture_config(meta, name)
    sd = O.key_seeded_state_dict(cfg, seed=meta["seed"])
    lo, hi = O.synthetic_batch(cfg, meta["batch"], seed=1234 + meta["seed"])
    pred, loss, pix, grads = O.tulip_loss_and_grads(sd, cfg, lo, hi)
    assert tuple(pred.shape) == tuple(z[f"{name}::pred_shape"].tolist())
    assert pred.shape[1] == cfg.in_chans
    assert abs(loss.item() - float(z[f"{name}::loss"])) <= 1e-5 * float(z[f"{name}::loss"])
    assert abs(pix.item() - float(z[f"{name}::pixel_loss"])) <= 1e-5 * float(z[f"{name}::pixel_loss"])
    got = pred.reshape(-1)[torch.from_numpy(z[f"{name}::pred_index"])].numpy()
    assert np.abs(got - z[f"{name}::pred"]).max() <= 1e-5
    for k in meta["configs"][name]["grad_keys"]:
        assert rel_l2(grads[k], z[f"{name}::grad::{k}"]) <= 1e-4, k
    for k, step in meta["configs"][name]["grad_rows"].items():
        assert rel_l2(grads[k][::step], z[f"{name}::grad_rows::{k}"]) <= 1e-4, k


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_shapes_match_reference(name):
    _, meta = fixture()
    cfg = fixture_config(meta, name)
    m = make_model(cfg)
    spec = O.state_dict_spec(cfg)
    sd = m.state_dict()
    assert list(sd.keys()) == list(spec.keys())
    for k, (shape, _) in spec.items():
        assert tuple(sd[k].shape) == tuple(shape), k
    kw = 8 if cfg.circular_padding else cfg.patch_size[1]
    assert tuple(sd["patch_embed.proj.weight"].shape) == (cfg.embed_dim, cfg.in_chans, cfg.patch_size[0], kw)
    assert tuple(sd["decoder_pred.weight"].shape) == (cfg.in_chans, cfg.embed_dim, 1, 1)
    m.load_state_dict(O.key_seeded_state_dict(cfg, seed=meta["seed"]), strict=True)


def test_seeded_init_matches_reference_at_in_chans_2():
    z, meta = fixture()
    cfg = fixture_config(meta, "c2")
    torch.manual_seed(0)
    sd = make_model(cfg).state_dict()
    for k in ("patch_embed.proj.weight", "decoder_pred.weight"):
        assert torch.equal(sd[k], torch.from_numpy(z[f"init_c2::{k}"])), k


@pytest.mark.parametrize("name", NAMES)
def test_engine_builds_without_gpu(name):
    from tulip_amd.engine import TulipEngine
    _, meta = fixture()
    cfg = fixture_config(meta, name)
    m = make_model(cfg)
    m.load_state_dict(O.key_seeded_state_dict(cfg, seed=meta["seed"]), strict=True)
    eng = TulipEngine(m)
    assert eng.model.in_chans == cfg.in_chans


def test_kitti_base_in_chans_2_engine_builds():
    from tulip_amd.engine import TulipEngine
    from tulip_amd.model import tulip as T
    m = T.tulip_base(img_size=(16, 1024), target_img_size=(64, 1024), patch_size=(1, 4), window_size=(2, 8),
                     pixel_shuffle=True, circular_padding=True, log_transform=True, patch_unmerging=True, in_chans=2)
    TulipEngine(m)


def test_in_chans_5_refused_naming_the_limit():
    from tulip_amd.engine import TulipEngine
    cfg = O.tiny_config(in_chans=5)
    with pytest.raises(NotImplementedError, match="in_chans 1 to 4"):
        TulipEngine(make_model(cfg))


def test_new_symbols_exported():
    lib = _lib.load()
    assert lib.tulip_abi_version() == 6
    for s in NEW_SYMBOLS:
        assert s in _lib.SIGNATURES, s
        assert getattr(lib, s) is not None, s


def test_abi_refuses_unbuilt_channel_counts_before_launching():
    """argument checks run on the host before any launch: no GPU needed"""
    lib = _lib.load()
    fake = 4096
    for c in (0, 5):
        assert lib.tulip_tail_fwd_c(fake, fake, fake, fake, fake, 2, 8, 64, 96, None, c) == -1
        assert lib.tulip_tail_bwd_c(fake, fake, fake, fake, fake, fake, fake, 2, 8, 64, 96, None, None, 1.0, None, c) == -1
        assert lib.tulip_tail_bwd_dgrad_c(fake, fake, fake, fake, fake, fake, fake, 2, 8, 64, 96, None, None, 1.0, None, c) == -1
        assert lib.tulip_tail_wgrad_c(fake, fake, fake, fake, fake, fake, fake, 2, 8, 64, 96, None, None, 1.0, None, c) == -1
        assert lib.tulip_tail_fwd_ln_c(fake, fake, fake, 1e-6, fake, fake, fake, fake, fake, fake, fake, None, None, 0,
                                       2, 8, 64, 96, None, c) == -1
        assert lib.tulip_expand_norm_fwd_c(fake, fake, fake, None, 0, fake, fake, fake, fake, 2, 8, 64, 4, 96, 1e-6, None, c) == -1
    # in_chans > 1 in FinalPatchExpanding needs the decoder_pred dot (dotw) and Cn <= 256
    assert lib.tulip_expand_norm_fwd_c(fake, fake, fake, fake, 96, None, None, fake, fake, 2, 8, 64, 2, 96, 1e-6, None, 2) == -1
    assert lib.tulip_expand_norm_fwd_c(fake, fake, fake, None, 0, fake, fake, fake, fake, 2, 8, 64, 4, 384, 1e-6, None, 2) == -1
    # empty batches are accepted (no launch) at the new channel counts
    assert lib.tulip_tail_fwd_c(fake, fake, fake, fake, fake, 0, 8, 64, 96, None, 4) == 0


def test_evaluate_refuses_multichannel_models():
    from tulip_amd import evaluation as EV
    m = make_model(O.tiny_config(in_chans=2))
    with pytest.raises(ValueError, match="in_chans"):
        EV.evaluate([], m, torch.device("cpu"), args=None)
    with pytest.raises(ValueError, match="in_chans"):
        EV.MCdrop([], m, torch.device("cpu"), args=None)

"""CPU: element dropout (drop_rate / attn_drop_rate) -- the drop-in constructor accepts it, the host definition of the
counter-based keep mask (tulip_amd/dropout.py) reproduces the fixture's masks and keeps the right fraction, and the new
C-ABI entry points are declared, bound and refuse what they do not support without launching anything."""
import json
import os
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn as nn

from tulip_amd import _lib
from tulip_amd import dropout as D

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def test_tulip_constructs_with_element_dropout():
    from tulip_amd.model import tulip as T
    m = T.TULIP(img_size=(8, 256), target_img_size=(32, 256), patch_size=(1, 4), embed_dim=48, window_size=[2, 8],
                depths=(2, 2), num_heads=(3, 6), drop_rate=0.1, attn_drop_rate=0.2,
                norm_layer=partial(nn.LayerNorm, eps=1e-6), pixel_shuffle=True, circular_padding=True,
                log_transform=True, patch_unmerging=True)
    blk = m.layers[0].blocks[1]
    assert m.pos_drop.p == 0.1 and blk.attn.attn_drop.p == 0.2 and blk.attn.proj_drop.p == 0.1
    assert blk.mlp.drop1.p == 0.1 and blk.mlp.drop2.p == 0.1
    eng = m.engine()
    # the torch rule: active iff p > 0 and the module is in training mode (MC dropout: eval() then Dropout.train())
    m.train()
    st = eng.dropout_state()
    assert st[0] == 0.1 and len(st[1]) == len(eng.blocks) and all(b == (0.2, 0.1, 0.1, 0.1) for b in st[1])
    m.eval()
    assert eng.dropout_state() == ()
    from tulip_amd.evaluation import enable_dropout
    enable_dropout(m)
    assert not m.training and eng.dropout_state() == st
    m.eval()
    m.layers[0].blocks[0].mlp.drop1.train()
    st = eng.dropout_state()
    assert st[0] == 0.0 and st[1][0] == (0.0, 0.0, 0.1, 0.0) and not any(any(b) for b in st[1][1:])


def test_reference_configs_keep_dropout_off():
    from tulip_amd.model import tulip as T
    m = T.tulip_base(img_size=(32, 2048), target_img_size=(128, 2048), patch_size=(1, 4), window_size=[2, 8],
                     pixel_shuffle=True, circular_padding=True, log_transform=True, patch_unmerging=True)
    m.train()
    assert m.engine().dropout_state() == ()


def _fixture():
    z = np.load(os.path.join(GOLD, "g14_tiny_dropout.npz"), allow_pickle=False)
    with open(os.path.join(GOLD, "g14_tiny_dropout.json")) as f:
        return z, json.load(f)


def test_mask_function_reproduces_fixture():
    z, meta = _fixture()
    n = meta["mask_n"]
    sites = [0] + [D.site(0, k) for k in (D.ATTN, D.PROJ, D.DROP1, D.DROP2)]
    for p in meta["mask_ps"]:
        for s in sites:
            want = np.unpackbits(z[f"mask::{s}::{p}"])[:n].astype(bool)
            got = D.keep(meta["mask_seed"], meta["mask_counter"], s, p, np.arange(n))
            assert np.array_equal(got, want), (s, p)
    # sites and counters give independent streams
    a = D.keep(meta["mask_seed"], meta["mask_counter"], 1, 0.5, np.arange(n))
    assert not np.array_equal(a, D.keep(meta["mask_seed"], meta["mask_counter"], 2, 0.5, np.arange(n)))
    assert not np.array_equal(a, D.keep(meta["mask_seed"], meta["mask_counter"] + 1, 1, 0.5, np.arange(n)))


def test_mask_function_definition():
    # splitmix64 finaliser on known inputs (reference values of the published constants)
    assert int(D.mix64(np.uint64(0))) == 0
    z = 0x9E3779B97F4A7C15
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & ((1 << 64) - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & ((1 << 64) - 1)
    assert int(D.mix64(np.uint64(0x9E3779B97F4A7C15))) == z ^ (z >> 31)
    assert D.threshold(0.1) == int(np.rint(np.float32(0.1) * 2 ** 24)) and D.threshold(0.0) == 0
    assert D.scale(0.1) == np.float32(1) / np.float32(np.float32(1) - np.float32(0.1))
    m = D.multiplier(3, 4, 5, 0.25, np.arange(16))
    assert m.dtype == np.float32 and set(np.unique(m)) <= {np.float32(0), D.scale(0.25)}
    assert D.keep(3, 4, 5, 0.0, np.arange(1 << 12)).all()


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_fraction(p):
    n = 1 << 22
    k = D.keep(0x1234, 99, 7, p, np.arange(n)).mean()
    sigma = np.sqrt(p * (1 - p) / n)
    assert abs(k - (1 - p)) <= 5 * sigma, (k, 1 - p)


def test_attention_and_window_index_maps():
    idx = D.attn_index(2, 4, 16, 3, (2, 8))
    assert idx.shape == (2 * 2 * 2, 3, 16, 16)
    win, h, q, k = 5, 2, 7, 11
    assert idx[win, h, q, k] == ((win * 3 + h) * 16 + q) * 16 + k
    rows = D.window_rows(1, 4, 16, (2, 8), (1, 4))
    # slot (i, j) of window (wy, wx) in the rolled image is natural token ((wy*2 + i + 1) % 4, (wx*8 + j + 4) % 16)
    assert rows[0, 0] == 1 * 16 + 4 and rows[3, 15] == ((2 + 1 + 1) % 4) * 16 + (8 + 7 + 4) % 16
    assert np.array_equal(np.sort(rows.reshape(-1)), np.arange(64))


NEW = {"tulip_dropout_begin": 4, "tulip_dropout_mask": 7, "tulip_dropout_scale": 10, "tulip_dropout_resid_ln": 19,
       "tulip_dropout_cast": 11, "tulip_window_attn_fwd_drop": 19, "tulip_window_attn_bwd_drop": 21}


def test_new_symbols_declared_and_bound():
    src = open(os.path.join(os.path.dirname(HERE), "include", "tulip_hip.h")).read()
    lib = _lib.load()
    assert lib.tulip_abi_version() == 6
    for name, nargs in NEW.items():
        assert f" {name}(" in src, name
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name]) == nargs, name
    from tulip_amd.csrc.build import SOURCES
    assert "dropout.hip" in SOURCES


def test_entry_points_refuse_before_launching():
    """argument checks run on the host before any launch: no GPU needed"""
    lib = _lib.load()
    fake = 4096
    # attn_drop with fp8 scores (TULIP_ATTN_FP8) is not built
    assert lib.tulip_window_attn_fwd_drop(fake, fake, fake, fake, 1, 2, 16, 96, 3, 2, 8, 0, 0, 2, fake, 1, 1, 0.1, None) == -1
    assert lib.tulip_window_attn_bwd_drop(fake, fake, fake, fake, fake, fake, 1, 2, 16, 96, 3, 2, 8, 0, 0, 2, fake, 1, 1,
                                          0.1, None) == -1
    # p outside [0, 1), missing key word, bad widths
    assert lib.tulip_dropout_mask(fake, 1, 0, 1.0, 16, fake, None) == -1
    assert lib.tulip_dropout_mask(None, 1, 0, 0.1, 16, fake, None) == -1
    assert lib.tulip_dropout_scale(fake, 0, 4, 6, 6, fake, 1, 0, 0.1, None) == -1
    assert lib.tulip_dropout_cast(fake, fake, 4, 8, None, 1, fake, 1, 0, -0.5, None) == -1
    assert lib.tulip_dropout_resid_ln(fake, fake, None, 1, fake, None, fake, None, None, None, None, 1e-6, 4, 8, fake, 1, 0,
                                      0.1, None) == -1
    assert lib.tulip_dropout_begin(None, fake, 1, None) == -1
    # empty work is a no-op
    assert lib.tulip_dropout_mask(fake, 1, 0, 0.1, 0, fake, None) == 0
    assert lib.tulip_dropout_scale(fake, 1, 0, 8, 8, fake, 1, 0, 0.1, None) == 0


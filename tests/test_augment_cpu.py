"""The per-sample range-image augmentation without a GPU, RangePrep(augment=...): the host definition (tulip_amd/augment.py)
against known answers and a pure-int restatement, the properties of `apply`, the constructor and call rules, the loader's sample
ids, and the new entry point in the header, both libraries and the bindings with its refusals before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tulip_amd import _lib
from tulip_amd import augment as A
from tulip_amd import data as D
from tulip_amd.dropout import threshold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = (1 << 64) - 1
NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------------- the table, in Python ints
def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def K(seed, i):
    return mix((seed & M) ^ 0x52414E4745415547 ^ mix(i & M))


def draw(k, n):
    return mix((k + n) & M)


def sfp(seed, i, W, f):
    k = K(seed, i)
    return ((draw(k, 0) >> 32) * W) >> 32, draw(k, 1) >> 63, ((draw(k, 2) >> 32) * f) >> 32


def beam_dropped(seed, i, il, p):
    return (draw(K(seed, i), (1 << 20) + il) >> 40) < threshold(p)


def point_dropped(seed, i, il, jl, Wl, p):
    return (draw(K(seed, i), (1 << 32) + il * Wl + jl) >> 40) < threshold(p)


# ---------------------------------------------------------------------------------------------------- 1. the definition
def test_known_answers():
    assert K(0, 0) == 0x973d1ff43a2ada07
    assert draw(K(0, 0), 0) == 0x7fddd9e4193143f1
    assert sfp(0, 0, 16, 4) == (7, 0, 0)
    assert sfp(7, 123456789012, 1024, 4) == (715, 0, 0)
    assert int(A.key(0, [0])[0]) == 0x973d1ff43a2ada07
    assert int(A.draw(A.key(0, [0]), 0)[0]) == 0x7fddd9e4193143f1
    assert A.params(0, [0], 16, 4).tolist() == [[7, 0, 0]]
    assert A.params(7, [123456789012], 1024, 4).tolist() == [[715, 0, 0]]
    assert A.DOMAIN == 0x52414E4745415547 == int.from_bytes(b"RANGEAUG", "big")


def test_module_matches_the_pure_int_restatement():
    rng = np.random.default_rng(0)
    cases = [(0, 0, 16, 4), (0, 63, 16, 4), (-1, -1, 18, 4), (1 << 64, 1 << 63, 72, 2), ((1 << 64) - 1, (1 << 63) - 1, 2048, 4)]
    for _ in range(300):
        cases.append((int(rng.integers(-2**63, 2**63)), int(rng.integers(-2**63, 2**63)), int(rng.integers(1, 5000)),
                      int(rng.integers(1, 9))))
    for seed, i, W, f in cases:
        want = sfp(seed, i, W, f)
        assert 0 <= want[0] < W and want[1] in (0, 1) and 0 <= want[2] < f
        assert tuple(A.params(seed, [i], W, f)[0]) == want, (seed, i, W, f)
        assert tuple(A.params(seed, [i], W, f, roll=False, flip=False, row_phase=3)[0]) == (0, 0, 3)
        assert tuple(A.params(seed, [i], W, f, roll=False, row_phase=False)[0]) == (0, want[1], 0)
    # vectorised over ids, of any integer dtype
    ids = np.arange(-5, 200, dtype=np.int64)
    got = A.params(3, ids, 72, 4)
    assert got.shape == (205, 3) and got.tolist() == [list(sfp(3, int(i), 72, 4)) for i in ids]
    # the drop masks
    for seed, p_b, p_p in ((0, 0.25, 0.5), (9, 0.1, 0.05), (5, 0.0, 0.0)):
        bm, pm = A.beam_mask(seed, ids[:20], 3, p_b), A.point_mask(seed, ids[:20], 3, 7, p_p)
        assert bm.shape == (20, 3) and pm.shape == (20, 3, 7) and bm.dtype == pm.dtype == bool
        for b, i in enumerate(ids[:20]):
            for il in range(3):
                assert bm[b, il] == beam_dropped(seed, int(i), il, p_b)
                for jl in range(7):
                    assert pm[b, il, jl] == point_dropped(seed, int(i), il, jl, 7, p_p)
    assert not A.beam_mask(5, ids, 4, 0.0).any() and not A.point_mask(5, ids, 4, 4, 0.0).any()


def test_coverage_sets_of_the_gpu_tests():
    """what tests/test_augment_gpu.py relies on, at seed 0"""
    p = A.params(0, np.arange(64), 16, 4)
    assert set(p[:, 0]) == set(range(16)) and set(p[:, 1]) == {0, 1} and set(p[:, 2]) == set(range(4))
    assert {(s % 4, fl) for s, fl, _ in p.tolist()} == {(r, fl) for r in range(4) for fl in (0, 1)}
    assert set(A.params(0, np.arange(128), 32, 4)[:, 0]) == set(range(32))
    assert {(s, fl) for s, fl, _ in A.params(0, np.arange(128), 18, 4).tolist()} == {(s, fl) for s in range(18) for fl in (0, 1)}
    assert set(A.params(0, np.arange(512), 72, 4)[:, 0]) == set(range(72))
    assert not A.params(0, np.arange(8), 16, 4)[:, 1].any()
    bm, pm = A.beam_mask(0, np.arange(64), 2, 0.25), A.point_mask(0, np.arange(64), 2, 16, 0.5)
    assert int(bm.sum()) == 33 and int(bm.all(1).sum()) == 4 and int((~bm.any(1)).sum()) == 35 and int(pm.sum()) == 1003


# ---------------------------------------------------------------------------------------------------- 2. apply
def plain_pair(hi0, f, fw=1, p=0, cp=0):
    return hi0[:, :, p::f, cp::fw], hi0


def test_apply_properties():
    rng = np.random.default_rng(1)
    B, H, W, f = 40, 8, 18, 4
    hi0 = rng.random((B, 1, H, W)).astype(np.float32)
    ids = np.arange(100, 100 + B)
    for fw, cp in ((1, 0), (2, 1), (3, 2)):
        lo, hi = A.apply(hi0, 0, ids, f, fw, cp)
        assert lo.shape == (B, 1, H // f, W // fw) and hi.shape == hi0.shape and lo.dtype == hi.dtype == np.float32
        par = A.params(0, ids, W, f)
        assert len(set(par[:, 0])) > 10 and set(par[:, 1]) == {0, 1} and len(set(par[:, 2])) == 4
        for b in range(B):
            s, fl, p = par[b]
            for i in range(H):
                assert np.array_equal(np.sort(hi[b, 0, i]), np.sort(hi0[b, 0, i]))          # a permutation of the row
            row = hi0[b, 0, :, ::-1] if fl else hi0[b, 0]
            assert np.array_equal(hi[b, 0], np.roll(row, s, axis=-1))                        # mirrored, then rotated
            assert np.array_equal(lo[b], hi[b, :, p::f, cp::fw])                             # drops off: the pair is consistent
    # element by element against the formula
    lo, hi = A.apply(hi0, 4, ids, f, 2, 1, beam_drop=0.25, point_drop=0.5)
    par = A.params(4, ids, W, f)
    src = lambda b, j: (W - 1 - (j - par[b, 0]) % W) if par[b, 1] else (j - par[b, 0]) % W
    n_drop = 0
    for b in range(B):
        for il in range(H // f):
            for jl in range(W // 2):
                dropped = beam_dropped(4, int(ids[b]), il, 0.25) or point_dropped(4, int(ids[b]), il, jl, W // 2, 0.5)
                n_drop += dropped
                want = 0.0 if dropped else hi0[b, 0, par[b, 2] + f * il, src(b, 1 + 2 * jl)]
                assert lo[b, 0, il, jl] == want and not np.signbit(lo[b, 0, il, jl])
    assert 0.4 * lo.size < n_drop < 0.8 * lo.size
    assert np.array_equal(hi, A.apply(hi0, 4, ids, f, 2, 1)[1])                              # the target is never dropped
    # all flags off: the plain pair, at a fixed row phase too
    for p in (0, 3):
        lo, hi = A.apply(hi0, 0, ids, f, 2, 1, roll=False, flip=False, row_phase=p)
        wl, wh = plain_pair(hi0, f, 2, p, 1)
        assert np.array_equal(lo, wl) and np.array_equal(hi, wh)
    with pytest.raises(ValueError):
        A.apply(hi0, 0, ids[:3], f)


# ---------------------------------------------------------------------------------------------------- 3. constructor and call rules
def test_range_augment_is_validated_and_frozen():
    a = A.RangeAugment()
    assert (a.seed, a.roll, a.flip, a.row_phase, a.beam_drop, a.point_drop) == (0, True, True, True, 0.0, 0.0)
    assert a.flags == 7 == _lib.AUG_ROLL | _lib.AUG_FLIP | _lib.AUG_ROW_PHASE and a.thresholds == (0, 0)
    b = A.RangeAugment(seed=5, roll=False, beam_drop=0.25, point_drop=np.float32(0.5))
    assert b.flags == 6 and b.thresholds == (1 << 22, 1 << 23) and type(b.point_drop) is float
    assert A.RangeAugment(flip=False, row_phase=False).flags == 1
    with pytest.raises(Exception):
        a.seed = 1
    for name in ("beam_drop", "point_drop"):
        for bad in (True, False, NAN, -0.1, 1.0, 1.5, INF, "0.1", None, np.bool_(True)):
            with pytest.raises(ValueError, match=name):
                A.RangeAugment(**{name: bad})
        assert getattr(A.RangeAugment(**{name: 0}), name) == 0.0
    for bad in (0.5, "1", None, True):
        with pytest.raises(ValueError, match="seed"):
            A.RangeAugment(seed=bad)
    assert A.RangeAugment(seed=np.int64(-3)).seed == -3


def test_range_prep_rules_raise_before_the_device_is_touched():
    aug = A.RangeAugment()
    plain = D.RangePrep("kitti", (2, 16), (8, 16), True)
    assert plain.augment is None and D.RangePrep("kitti", (2, 16), (8, 16), True, augment=None).augment is None
    prep = D.RangePrep("kitti", (2, 16), (8, 16), True, augment=aug)
    assert prep.augment is aug
    raw = torch.zeros(3, 8, 16)
    rimg = torch.zeros(3, 16, 8, dtype=torch.float16)
    with pytest.raises(ValueError, match="sample_ids"):
        prep(raw)                                                                   # augment set and no ids
    with pytest.raises(ValueError, match="sample_ids"):
        prep.from_rimg(rimg)
    with pytest.raises(ValueError, match="sample_ids"):
        plain(raw, sample_ids=[0, 1, 2])                                            # ids without augment
    with pytest.raises(ValueError, match="sample_ids"):
        plain.from_rimg(rimg, sample_ids=torch.arange(3))
    for bad in ([0, 1], [0, 1, 2, 3], torch.arange(2), torch.arange(4)):            # a wrong id count
        with pytest.raises(ValueError, match="sample ids|sample_ids"):
            prep(raw, sample_ids=bad)
        with pytest.raises(ValueError, match="sample ids|sample_ids"):
            prep.from_rimg(rimg, sample_ids=bad)
    with pytest.raises(ValueError, match="sample_ids"):
        prep(raw, sample_ids=torch.arange(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="roll_shift"):
        D.RangePrep("kitti", (2, 16), (8, 16), True, roll_shift=3, augment=aug)
    with pytest.raises(ValueError, match="row_phase"):
        D.RangePrep("kitti", (2, 16), (8, 16), True, row_phase=1, augment=aug)
    with pytest.raises(ValueError, match="augment"):
        D.RangePrep("kitti", (2, 16), (8, 16), True, augment=dict(seed=0))
    ok = D.RangePrep("kitti", (2, 16), (8, 16), True, row_phase=1, augment=A.RangeAugment(row_phase=False))
    assert ok.row_phase == 1
    # the right arguments get as far as the device check: there is no CPU fallback
    with pytest.raises(RuntimeError, match="GPU only"):
        prep(raw, sample_ids=[0, 1, 2])
    with pytest.raises(RuntimeError, match="GPU only"):
        plain(raw)


# ---------------------------------------------------------------------------------------------------- 4. the loader's ids
def test_loader_sample_ids(tmp_path):
    for i in range(5):
        np.save(tmp_path / f"{i:06d}.npy", np.zeros((8, 16, 2), np.float32))
    prep = D.RangePrep("kitti", (2, 16), (8, 16), True, augment=A.RangeAugment())
    ld = D.DeviceRangeLoader(str(tmp_path), prep, 2, device="cpu", drop_last=False)
    assert ld.batches() == [([0, 1], [0, 1]), ([2, 3], [2, 3]), ([4], [4])]
    ld.set_epoch(1)
    assert ld.batches() == [([0, 1], [5, 6]), ([2, 3], [7, 8]), ([4], [9])]
    # DistributedSampler: 5 files padded to 6, strided by rank -- the padded repeat of file 0 carries file 0's id
    r0, r1 = (D.DeviceRangeLoader(str(tmp_path), prep, 2, device="cpu", drop_last=False, rank=r, world_size=2) for r in (0, 1))
    assert r0.batches() == [([0, 2], [0, 2]), ([4], [4])] and r1.batches() == [([1, 3], [1, 3]), ([0], [0])]
    r0.set_epoch(1), r1.set_epoch(1)
    assert r0.batches() == [([0, 2], [5, 7]), ([4], [9])] and r1.batches() == [([1, 3], [6, 8]), ([0], [5])]
    # drop_last, another batch size: the same id for the same (epoch, file)
    ld3 = D.DeviceRangeLoader(str(tmp_path), prep, 3, device="cpu", drop_last=True)
    ld3.set_epoch(1)
    assert ld3.batches() == [([0, 1, 2], [5, 6, 7])] and len(ld3) == 1
    # shuffled: ids follow the files
    sh = D.DeviceRangeLoader(str(tmp_path), prep, 2, device="cpu", shuffle=True, drop_last=False, seed=3)
    sh.set_epoch(2)
    flat = [(i, s) for idx, ids in sh.batches() for i, s in zip(idx, ids)]
    assert sorted(flat) == [(i, 10 + i) for i in range(5)] and [i for i, _ in flat] == sh._order()


# ---------------------------------------------------------------------------------------------------- 5. library, bindings
NARGS = 27


def test_symbol_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "tulip_hip.h")).read()
    for name, val in (("TULIP_AUG_ROLL", 1), ("TULIP_AUG_FLIP", 2), ("TULIP_AUG_ROW_PHASE", 4)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), hdr)
    assert re.search(r"#define\s+TULIP_ABI_VERSION\s+6\b", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+tulip_range_prep_aug\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m, "tulip_range_prep_aug is not declared in include/tulip_hip.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    plain = re.search(r"\bint\s+tulip_range_prep\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    pargs = [" ".join(a.split()) for a in plain.group(1).split(",")]
    assert pargs[-2:] == ["int roll_shift", "hipStream_t stream"] and len(pargs) == 22                 # the plain call is as it was
    assert args[:20] == pargs[:20] and args[20:] == ["const int64_t* sample_ids", "uint64_t seed", "int flags",
                                                    "uint32_t beam_threshold", "uint32_t point_threshold",
                                                    "int32_t* params_out", "hipStream_t stream"]
    assert len(args) == NARGS == len(_lib.SIGNATURES["tulip_range_prep_aug"])
    assert _lib.SIGNATURES["tulip_range_prep_aug"][:20] == _lib.SIGNATURES["tulip_range_prep"][:20]
    assert _lib.SIGNATURES["tulip_range_prep_aug"][20:] == [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint32,
                                                           ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    from tulip_amd.csrc.build import build
    build(force=False, verbose=False)
    lib = _lib.load()
    assert lib.tulip_abi_version() == 6 == _lib.ABI_VERSION                                            # additive: the ABI version stays
    with _lib.dev_library() as dev:
        assert dev is not lib and hasattr(dev, "tulip_range_prep_aug") and dev.tulip_abi_version() == 6
    assert hasattr(lib, "tulip_range_prep_aug")
    from tulip_amd import ops
    assert callable(ops.range_prep_aug)


def test_bad_arguments_are_refused_on_the_host():
    """TULIP_ERR_ARG comes back before any launch: these calls need no GPU."""
    lib = _lib.load()
    buf = (ctypes.c_float * 1024)()
    a = (ctypes.addressof(buf) + 15) & ~15

    def call(raw=a, dt=0, sb=128, si=16, sj=1, base=0, hi=a + 1024, lo=a + 2048, B=1, H=8, W=16, f=4, fw=1, rp=0, cp=0, ids=a + 3072,
             seed=0, flags=7, bt=0, pt=0, par=None):
        return lib.tulip_range_prep_aug(raw, dt, sb, si, sj, base, hi, lo, B, H, W, f, fw, rp, cp, 1.0, 0, 0.0, 0.0, 1, ids, seed, flags,
                                        bt, pt, par, None)
    with _lib.dev_library() as dev:
        libs = (lib, dev)
    for L_ in libs:
        lib = L_
        assert call(ids=None) == -1                                                  # the new arguments
        assert call(ids=a + 3076) == -1
        for flags in (8, 15, 16, -1, 1 << 20):
            assert call(flags=flags) == -1
        for t in ((1 << 24) + 1, 1 << 25, (1 << 32) - 1):
            assert call(bt=t) == -1 and call(pt=t) == -1
        # ... and everything the plain call refuses
        assert call(raw=None) == -1 and call(hi=None, lo=None) == -1
        assert call(B=0) == -1 and call(H=0) == -1 and call(W=0) == -1 and call(f=0) == -1 and call(fw=0) == -1
        assert call(H=7) == -1 and call(fw=3) == -1 and call(rp=-1) == -1 and call(rp=4) == -1
        assert call(fw=2, cp=2) == -1 and call(cp=-1) == -1 and call(dt=2) == -1 and call(dt=-1) == -1
    assert not any(buf)                                                              # nothing was written

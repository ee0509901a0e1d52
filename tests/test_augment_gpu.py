"""The per-sample augmentation on the GPU: tulip_range_prep_aug (through RangePrep(augment=...) and the ops-level call) is bit for
bit `augment.apply` -- the host definition's gather -- of the plain tulip_range_prep output of the same library, for every shift
residue, both mirror states and every row phase, on both kernel families; the plain output itself is held to the data oracle by the
rule of tests/test_data_gpu.py.  Each test first asserts on the host that its ids draw what it means to cover."""
import numpy as np
import pytest
import torch

from oracle import data_oracle as DO
from tulip_amd import augment as A
from tulip_amd import data as D
from tulip_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOG_ATOL = 2.4e-7          # tests/test_data_gpu.py


def close(got: torch.Tensor, ref, log_t: bool):
    ref = torch.as_tensor(np.ascontiguousarray(ref))
    got = got.cpu()
    assert got.shape == ref.shape
    if not log_t:
        assert torch.equal(got, ref)
    else:
        assert torch.equal(got == 0, ref == 0)
        assert (got - ref).abs().max().item() <= LOG_ATOL


def same_bits(got: torch.Tensor, want: np.ndarray):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def check(ds, lo_size, hi_size, log_t, raw_cpu, ids, aug, col_phase=0, run=None, plain_run=None):
    """plain output vs the oracle; augmented output (and params_out) vs the definition applied to the plain output"""
    B = len(ids)
    plain = D.RangePrep(ds, lo_size, hi_size, log_t, col_phase=col_phase)
    prep = D.RangePrep(ds, lo_size, hi_size, log_t, col_phase=col_phase, augment=aug)
    lo0, hi0 = plain_run(plain)
    if raw_cpu is not None:
        olo, ohi = DO.range_prep(raw_cpu, DO.DATASETS[ds], lo_size, hi_size, log_t, None, col_phase=col_phase)
        close(lo0, olo, log_t)
        close(hi0, ohi, log_t)
    par = torch.full((B, 4), -1, dtype=torch.int32, device=DEV)
    lo, hi = run(prep, torch.as_tensor(np.asarray(ids), dtype=torch.int64).to(DEV), par)
    f, fw = prep.f, prep.fw
    want = A.params(aug.seed, ids, hi_size[1], f, aug.roll, aug.flip, True if aug.row_phase else 0)
    assert np.array_equal(par.cpu().numpy(), np.concatenate([want, np.zeros((B, 1), np.int64)], 1))
    wlo, whi = A.apply(hi0.cpu().numpy(), aug.seed, ids, f, fw, col_phase, aug.roll, aug.flip, True if aug.row_phase else 0,
                       aug.beam_drop, aug.point_drop)
    same_bits(hi, whi)
    same_bits(lo, wlo)
    return lo, hi, lo0, hi0


# ---------------------------------------------------------------------------------------------------- 1. draws
def test_params_out_is_the_host_draw():
    ids = np.arange(64)
    want = A.params(0, ids, 16, 4)
    assert set(want[:, 0]) == set(range(16)) and set(want[:, 1]) == {0, 1} and set(want[:, 2]) == set(range(4))
    prep = D.RangePrep("kitti", (2, 16), (8, 16), True, augment=A.RangeAugment(seed=0))
    raw = DO.synthetic_raw(64, 8, 16, seed=1).to(DEV)
    par = torch.full((64, 4), -1, dtype=torch.int32, device=DEV)
    prep(raw, sample_ids=torch.arange(64, device=DEV), params_out=par)
    assert np.array_equal(par.cpu().numpy()[:, :3], want) and not par[:, 3].any().item()
    # other seeds, negative and large ids, one flag at a time; the generic kernel writes them too
    ids = [-1, -2**63, 2**63 - 1, 123456789012, 0, 7]
    for seed, kw in ((7, {}), (-3, dict(roll=False)), (2**64 - 1, dict(flip=False)), (1, dict(row_phase=False))):
        aug = A.RangeAugment(seed=seed, **kw)
        want = A.params(seed, ids, 18, 4, aug.roll, aug.flip, True if aug.row_phase else 0)
        prep = D.RangePrep("kitti", (2, 18), (8, 18), True, augment=aug)
        par = torch.full((6, 4), -1, dtype=torch.int32, device=DEV)
        prep(DO.synthetic_raw(6, 8, 18, seed=1).to(DEV), sample_ids=ids, params_out=par)
        assert np.array_equal(par.cpu().numpy()[:, :3], want)


# ---------------------------------------------------------------------------------------------------- 2. row-major fast path
@pytest.fixture(scope="module")
def case2():
    """(8,16) -> (2,16), B = 64, ids 0..63 at seed 0: raw, and the augmented outputs of one 64-sample call"""
    ids = np.arange(64)
    par = A.params(0, ids, 16, 4)
    assert set(par[:, 0]) == set(range(16)) and 0 in par[:, 0] and 15 in par[:, 0]
    assert set(par[:, 1]) == {0, 1} and set(par[:, 2]) == set(range(4))
    assert {(s % 4, fl) for s, fl, _ in par.tolist()} == {(r, fl) for r in range(4) for fl in (0, 1)}
    raw = DO.synthetic_raw(64, 8, 16, seed=21)
    prep = D.RangePrep("durlar", (2, 16), (8, 16), True, augment=A.RangeAugment(seed=0))
    lo, hi = prep(raw.to(DEV), sample_ids=ids.tolist())
    return ids, raw, prep, lo, hi


@pytest.mark.parametrize("log_t", [True, False])
def test_rows_kernel_plain_source(case2, log_t):
    ids, raw, _, lo2, hi2 = case2
    lo, hi, _, _ = check("durlar", (2, 16), (8, 16), log_t, raw, ids, A.RangeAugment(seed=0),
                         run=lambda p, i, par: p(raw.to(DEV), sample_ids=i, params_out=par), plain_run=lambda p: p(raw.to(DEV)))
    if log_t:
        assert torch.equal(lo, lo2) and torch.equal(hi, hi2)


def test_rows_kernel_interleaved_payload(case2):
    ids, raw, _, lo2, hi2 = case2
    payload = torch.stack([raw, torch.full_like(raw, float("nan"))], -1).contiguous().to(DEV)      # channel 1 is never read
    lo, hi, _, _ = check("durlar", (2, 16), (8, 16), True, raw, ids, A.RangeAugment(seed=0),
                         run=lambda p, i, par: p(payload, sample_ids=i, params_out=par), plain_run=lambda p: p(payload))
    assert torch.isfinite(lo).all().item() and torch.isfinite(hi).all().item()
    assert torch.equal(lo, lo2) and torch.equal(hi, hi2)


# ---------------------------------------------------------------------------------------------------- 3. width subsampling
def test_width_subsampling_any_shift():
    ids = np.arange(128)
    par = A.params(0, ids, 32, 4)
    assert set(par[:, 0]) == set(range(32)) and set(par[:, 1]) == {0, 1}
    raw = DO.synthetic_raw(128, 8, 32, seed=22)
    for src in (raw.to(DEV), torch.stack([raw, torch.rand_like(raw)], -1).contiguous().to(DEV)):
        lo, hi, _, _ = check("durlar", (2, 16), (8, 32), True, raw, ids, A.RangeAugment(seed=0), col_phase=1,
                             run=lambda p, i, q: p(src, sample_ids=i, params_out=q), plain_run=lambda p: p(src))
        lo, hi = lo.cpu(), hi.cpu()
        for b in range(128):                                                        # drops off: lo == hi[:, :, p::f, cp::fw]
            assert torch.equal(lo[b], hi[b, :, int(par[b, 2])::4, 1::2])


# ---------------------------------------------------------------------------------------------------- 4. generic (LDS) path
def test_generic_kernel_float32_odd_width():
    ids = np.arange(128)
    par = A.params(0, ids, 18, 4)
    assert {(s, fl) for s, fl, _ in par.tolist()} == {(s, fl) for s in range(18) for fl in (0, 1)}
    raw = DO.synthetic_raw(128, 8, 18, seed=23)
    check("carla", (2, 18), (8, 18), True, raw, ids, A.RangeAugment(seed=0),
          run=lambda p, i, q: p(raw.to(DEV), sample_ids=i, params_out=q), plain_run=lambda p: p(raw.to(DEV)))


def test_generic_kernel_rimg_payload_crosses_both_tile_edges():
    s0, s1, f = 40, 72, 4                                          # H = 40 > TI = 32, W = 72 > TJ = 64
    ids = np.arange(512)
    par = A.params(0, ids, s1, f)
    assert set(par[:, 0]) == set(range(s1)) and set(par[:, 1]) == {0, 1} and set(par[:, 2]) == set(range(f))
    g = torch.Generator().manual_seed(5)
    pay = (torch.rand(512, s1, s0, generator=g) * 90).half()
    ref = torch.flip(pay.transpose(1, 2), dims=(1, 2)).float()                     # datasets.py:190-193
    check("carla", (s0 // f, s1), (s0, s1), True, ref, ids, A.RangeAugment(seed=0),
          run=lambda p, i, q: p.from_rimg(pay.to(DEV), sample_ids=i, params_out=q), plain_run=lambda p: p.from_rimg(pay.to(DEV)))


# ---------------------------------------------------------------------------------------------------- 5. drops
def test_beam_and_point_drops(case2):
    ids, raw, _, _, hi2 = case2
    bm, pm = A.beam_mask(0, ids, 2, 0.25), A.point_mask(0, ids, 2, 16, 0.5)
    assert int(bm.sum()) == 33 and int(bm.all(1).sum()) == 4 and int((~bm.any(1)).sum()) == 35 and int(pm.sum()) == 1003
    aug = A.RangeAugment(seed=0, beam_drop=0.25, point_drop=0.5)
    for src in (raw.to(DEV), torch.stack([raw, raw], -1).contiguous().to(DEV)):
        lo, hi, _, _ = check("durlar", (2, 16), (8, 16), True, raw, ids, aug,
                             run=lambda p, i, q: p(src, sample_ids=i, params_out=q), plain_run=lambda p: p(src))
        assert torch.equal(hi, hi2)                                                 # the target is never dropped
        dropped = torch.as_tensor(bm[:, :, None] | pm)[:, None]
        assert not lo.cpu()[dropped].any().item() and not torch.signbit(lo.cpu()[dropped]).any().item()
    # the generic kernel draws the same masks
    raw18 = DO.synthetic_raw(64, 8, 18, seed=24)
    check("durlar", (2, 18), (8, 18), True, raw18, ids, aug,
          run=lambda p, i, q: p(raw18.to(DEV), sample_ids=i, params_out=q), plain_run=lambda p: p(raw18.to(DEV)))


# ---------------------------------------------------------------------------------------------------- 6. identity
@pytest.mark.parametrize("shape", [((2, 16), (8, 16)), ((2, 16), (8, 32)), ((2, 18), (8, 18))])
def test_all_off_is_the_plain_entry_point(shape):
    lo_size, hi_size = shape
    raw = DO.synthetic_raw(5, *hi_size, seed=25).to(DEV)
    off = A.RangeAugment(seed=9, roll=False, flip=False, row_phase=False)
    for rp in (0, 3):
        cp = 1 if hi_size[1] != lo_size[1] else 0
        plain = D.RangePrep("durlar", lo_size, hi_size, True, row_phase=rp, col_phase=cp)
        prep = D.RangePrep("durlar", lo_size, hi_size, True, row_phase=rp, col_phase=cp, augment=off)
        par = torch.full((5, 4), -1, dtype=torch.int32, device=DEV)
        lo, hi = prep(raw, sample_ids=[3, 1, 4, 1, 5], params_out=par)
        lo0, hi0 = plain(raw)
        assert torch.equal(lo, lo0) and torch.equal(hi, hi0)
        assert par.cpu().tolist() == [[0, 0, rp, 0]] * 5


# ---------------------------------------------------------------------------------------------------- 7. batch independence
def test_a_sample_does_not_depend_on_its_batch(case2):
    ids, raw, prep, lo, hi = case2
    dev_raw = raw.to(DEV)
    one_lo, one_hi = zip(*(prep(dev_raw[b:b + 1], sample_ids=[int(ids[b])]) for b in (0, 17, 63)))
    for k, b in enumerate((0, 17, 63)):
        assert torch.equal(one_lo[k][0], lo[b]) and torch.equal(one_hi[k][0], hi[b])
    for s in range(0, 63, 3):
        l3, h3 = prep(dev_raw[s:s + 3], sample_ids=ids[s:s + 3].tolist())
        assert torch.equal(l3, lo[s:s + 3]) and torch.equal(h3, hi[s:s + 3])
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(0))
    lp, hp = prep(dev_raw[perm.to(DEV)].contiguous(), sample_ids=torch.as_tensor(ids)[perm].to(DEV))
    assert torch.equal(lp, lo[perm.to(DEV)]) and torch.equal(hp, hi[perm.to(DEV)])
    lo_only, none = prep(dev_raw, sample_ids=ids.tolist(), want_hi=False)
    assert none is None and torch.equal(lo_only, lo)
    # the generic kernel's inference form
    raw18 = DO.synthetic_raw(64, 8, 18, seed=26).to(DEV)
    p18 = D.RangePrep("durlar", (2, 18), (8, 18), True, augment=A.RangeAugment(seed=0, beam_drop=0.25, point_drop=0.5))
    l18, _ = p18(raw18, sample_ids=ids.tolist())
    lo_only, none = p18(raw18, sample_ids=ids.tolist(), want_hi=False)
    assert none is None and torch.equal(lo_only, l18)


# ---------------------------------------------------------------------------------------------------- 8. graph
def test_captured_call_reads_the_ids_at_replay():
    B, H, W, f = 16, 8, 16, 4
    raw = DO.synthetic_raw(B, H, W, seed=27).to(DEV)
    first, second = np.arange(8, 8 + B), np.arange(40, 40 + B)
    pa, pb = A.params(0, first, W, f), A.params(0, second, W, f)
    assert (pa != pb).any(1).all() and set(pa[:, 1]) == set(pb[:, 1]) == {0, 1}
    plain = D.RangePrep("kitti", (2, 16), (8, 16), True)
    _, hi0 = plain(raw)
    ids = torch.as_tensor(first, dtype=torch.int64).to(DEV)
    hi = torch.zeros(B, 1, H, W, device=DEV)
    lo = torch.zeros(B, 1, H // f, W, device=DEV)
    par = torch.zeros(B, 4, dtype=torch.int32, device=DEV)
    aug = A.RangeAugment(seed=0, beam_drop=0.25, point_drop=0.5)

    def launch():
        ops.range_prep_aug(raw, 0, H * W, W, 1, 0, hi, lo, B, H, W, f, 1, 0, 0, plain.scale, False, 0.0, 0.0, True, ids, aug.seed,
                           aug.flags, *aug.thresholds, par)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for these, want_par in ((first, pa), (second, pb)):
        ids.copy_(torch.as_tensor(these, dtype=torch.int64))
        hi.zero_(), lo.zero_(), par.zero_()
        graph.replay()
        torch.cuda.synchronize()
        wlo, whi = A.apply(hi0.cpu().numpy(), 0, these, f, beam_drop=0.25, point_drop=0.5)
        same_bits(hi, whi)
        same_bits(lo, wlo)
        assert np.array_equal(par.cpu().numpy()[:, :3], want_par)


# ---------------------------------------------------------------------------------------------------- 9. loader
def test_loader_draws_by_epoch_and_file(tmp_path):
    rng = np.random.default_rng(0)
    root = tmp_path / "train"
    root.mkdir()
    raws = []
    for i in range(5):
        a = (rng.random((64, 256, 2)) * 100).astype(np.float32)
        np.save(root / f"{i:06d}.npy", a)
        raws.append(torch.from_numpy(a[..., 0].copy()))
    par = A.params(3, np.arange(10), 256, 4)
    assert set(par[:, 1]) == {0, 1} and len(set(par[:, 0])) == 10
    aug = A.RangeAugment(seed=3, beam_drop=0.1, point_drop=0.05)
    prep = D.RangePrep("kitti", (16, 256), (64, 256), True, augment=aug)
    plain = D.RangePrep("kitti", (16, 256), (64, 256), True)
    _, hi0 = plain(torch.stack(raws).to(DEV))
    olo, ohi = DO.range_prep(torch.stack(raws), DO.DATASETS["kitti"], (16, 256), (64, 256), True)
    close(hi0, ohi, True)
    hi0 = hi0.cpu().numpy()
    ld = D.DeviceRangeLoader(str(root), prep, 2, drop_last=False)
    by_epoch = []
    for epoch in (0, 1):
        ld.set_epoch(epoch)
        out, seen = {}, 0
        for lo, hi in ld:
            n = lo.shape[0]
            files = list(range(seen, seen + n))
            wlo, whi = A.apply(hi0[files], 3, [epoch * 5 + i for i in files], 4, beam_drop=0.1, point_drop=0.05)
            same_bits(lo, wlo)
            same_bits(hi, whi)
            for k, i in enumerate(files):
                out[i] = (lo[k].clone(), hi[k].clone())
            seen += n
        assert seen == 5
        by_epoch.append(out)
    assert all(not torch.equal(by_epoch[0][i][1], by_epoch[1][i][1]) for i in range(5))            # fresh draws per epoch
    # two ranks reproduce the single-rank outputs file by file (the padded repeat of file 0 included)
    for epoch in (0, 1):
        for rank in (0, 1):
            r = D.DeviceRangeLoader(str(root), prep, 2, drop_last=False, rank=rank, world_size=2)
            r.set_epoch(epoch)
            got = list(r)
            files = [i for idx, _ in r.batches() for i in idx]
            assert files == ([0, 2, 4] if rank == 0 else [1, 3, 0])
            k = 0
            for lo, hi in got:
                for b in range(lo.shape[0]):
                    assert torch.equal(lo[b], by_epoch[epoch][files[k]][0]) and torch.equal(hi[b], by_epoch[epoch][files[k]][1])
                    k += 1
            assert k == 3
    # a loader on a RangePrep without augment is the loader of before
    seen = 0
    for lo, hi in D.DeviceRangeLoader(str(root), plain, 2, drop_last=False):
        n = lo.shape[0]
        close(lo, olo[seen:seen + n], True)
        close(hi, ohi[seen:seen + n], True)
        seen += n
    assert seen == 5


# ---------------------------------------------------------------------------------------------------- 10. one full size
def test_full_size_kitti_payload():
    ids = np.arange(100, 108)
    par = A.params(0, ids, 1024, 4)
    assert set(par[:, 1]) == {0, 1} and len(set(par[:, 0] % 4)) >= 3 and len(set(par[:, 2])) >= 3
    rng = DO.synthetic_raw(8, 64, 1024, seed=11)
    payload = torch.stack([rng, torch.rand_like(rng)], dim=-1).contiguous().to(DEV)
    aug = A.RangeAugment(seed=0, beam_drop=0.1, point_drop=0.05)
    check("kitti", (16, 1024), (64, 1024), True, rng, ids, aug,
          run=lambda p, i, q: p(payload, sample_ids=i, params_out=q), plain_run=lambda p: p(payload))

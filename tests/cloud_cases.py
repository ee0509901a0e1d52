"""Shared builders of the dense-cloud tests (tests/test_cloud_cpu.py, tests/test_cloud_gpu.py): synthetic (pred, lo) batches whose
kept pixels follow a chosen pattern over the destination slots, the host definition's answer for them (computed once per case and
left unchanged), guarded device buffers, and the comparison of a launch's outputs against that answer.

A case fixes the dataset tables ("carla" allows any H, W; one "durlar" case crosses the row end with its rotation), B, C, (H, W),
(h, w), the keep pattern, and whether the planes are stored as log1p.  With T = tulip_cloud_tile():
    H*W < T;  H*W == 2T;  H*W == T + 476 (a partial last tile that is no multiple of 64);  B*tiles > 256 (B = 5, H*W = 64T).

Values.  A kept slot holds a range inside the gate; a slot that is not kept holds, in turn, +0.0, -0.0, a NaN, a value under the
gate, a value over it, -inf, +inf (prediction rows) or +0.0, -0.0, a NaN, a negative value (restored rows, which are not gated).
Log cases store log1p of those values; every prediction value of a log case has a float64 expm1 at least 4 fp32 ulp from both gate
bounds (`assert_gate_margin`), so an expm1 that is 2 ulp off cannot change a keep decision.  keep_close is only used without log.
"""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional, Tuple

import numpy as np

from tulip_amd import cloud as CL
from tulip_amd import evaluation as EV

F32 = np.float32
PATTERNS = ("all", "none", "none_middle", "alternating", "lane63", "tile_first", "last_pixel", "random")


class Case(NamedTuple):
    name: str
    dataset: str
    B: int
    C: int
    H: int
    W: int
    h: int
    w: int
    pattern: str
    log: bool = False
    channel_log: Tuple[bool, ...] = ()
    keep_close: float = 0.0
    seed: int = 0

    @property
    def gate(self):
        return EV.pred_gate(self.dataset, False)


def shapes(T: int):
    """(H, W, h) of the four sizes; W follows the tile so that every size stays what its name says"""
    return {"small": (4, 100, 2), "two_tiles": (8, T // 4, 2), "partial": (4, (T + 476) // 4, 2), "scan2": (64, T, 16)}


def kernel_cases(T: int):
    S = shapes(T)
    out = []

    def add(name, shape, B, C, pattern, dataset="carla", restore=True, **kw):
        H, W, h = S[shape] if isinstance(shape, str) else shape
        out.append(Case(name, dataset, B, C, H, W, h, W if restore else W // 2, pattern, seed=len(out) + 1, **kw))

    # every keep pattern on the partial-tile size, three images (none_middle needs them)
    for p in PATTERNS:
        add(f"partial-B3-C1-{p}", "partial", 3, 1, p)
    # sizes x B x C
    add("small-B1-C1-random", "small", 1, 1, "random")
    add("small-B3-C2-alternating", "small", 3, 2, "alternating")
    add("small-B1-C4-random-norestore", "small", 1, 4, "random", restore=False)
    add("two_tiles-B1-C2-lane63", "two_tiles", 1, 2, "lane63")
    add("two_tiles-B3-C4-tile_first", "two_tiles", 3, 4, "tile_first")
    add("two_tiles-B3-C1-all", "two_tiles", 3, 1, "all")
    add("partial-B1-C4-last_pixel", "partial", 1, 4, "last_pixel")
    add("partial-B3-C2-random-keep_close", "partial", 3, 2, "random", keep_close=0.25)
    add("partial-B1-C1-random-norestore", "partial", 1, 1, "random", restore=False)
    add("scan2-B5-C1-random", "scan2", 5, 1, "random")
    add("scan2-B5-C2-tile_first", "scan2", 5, 2, "tile_first")
    # DurLAR tables: offsets 48, 32, 16, 0 at W = 96 rotate across the row end
    add("durlar-B2-C1-random", (8, 96, 2), 2, 1, "random", dataset="durlar")
    add("durlar-B3-C2-alternating", (8, 96, 2), 3, 2, "alternating", dataset="durlar")
    add("durlar-B1-C4-lane63", (8, 96, 4), 1, 4, "lane63", dataset="durlar")
    # planes stored as log1p
    add("partial-B3-C1-random-log", "partial", 3, 1, "random", log=True)
    add("two_tiles-B1-C4-random-log", "two_tiles", 1, 4, "random", log=True, channel_log=(True, False, True))
    add("small-B3-C2-alternating-log", "small", 3, 2, "alternating", log=True, channel_log=(False,))
    add("durlar-B2-C2-random-log", (8, 96, 2), 2, 2, "random", dataset="durlar", log=True, channel_log=(True,))
    return out


def keep_mask(case: Case, T: int, pattern: Optional[str] = None) -> np.ndarray:
    """(B, H*W) bool over the destination slots"""
    p = pattern or case.pattern
    n = case.H * case.W
    d = np.arange(n)
    rng = np.random.default_rng(1000 + case.seed)
    one = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "none_middle": np.ones(n, bool), "alternating": d % 2 == 0,
           "lane63": d % 64 == 63, "tile_first": d % T == 0, "last_pixel": np.zeros(n, bool)}.get(p)
    if p == "random":
        return rng.random((case.B, n)) < 0.5
    if p == "sparser":          # the second call into the same buffers: a subset of nothing in particular
        return rng.random((case.B, n)) < 0.1
    m = np.tile(one, (case.B, 1))
    if p == "none_middle":
        m[case.B // 2] = False
    if p == "last_pixel":
        m[-1, -1] = True
    return m


def _source_order(case: Case, planes_dst: np.ndarray) -> np.ndarray:
    """(..., H, W) in destination order -> pixel order (the inverse of cloud.to_destination)"""
    cols = CL.destination_columns(case.dataset, case.H, case.W)
    return np.take_along_axis(planes_dst, np.broadcast_to(cols, planes_dst.shape), axis=-1)


class Problem(NamedTuple):
    case: Case
    pred: np.ndarray            # (B, C, H, W) float32, the model's value space
    lo: np.ndarray              # (B, C, h, w) float32
    keep: np.ndarray            # (B, H*W) bool over the destination slots: what the builder planted
    points: np.ndarray          # the host definition's answer
    offsets: np.ndarray
    planes: np.ndarray          # (B, C, H, W), destination order
    counts: np.ndarray          # (B * tiles,) int32
    planes64: Optional[np.ndarray]      # log cases: the chain with float64 expm1, destination order


def build(case: Case, T: int, pattern: Optional[str] = None) -> Problem:
    B, C, H, W, h, w = case.B, case.C, case.H, case.W, case.h, case.w
    f, restore = H // h, w == W
    gmin, gmax = (F32(v) for v in case.gate)
    rng = np.random.default_rng(case.seed * 7919 + (0 if pattern is None else 13))
    keep = keep_mask(case, T, pattern)
    top = F32(0.2) if case.keep_close > 0 else gmax
    # final range per destination slot: inside the gate (and under keep_close) where kept ...
    want = (gmin + (top - gmin) * rng.random((B, H, W))).astype(F32)
    if case.log:                # clear of both bounds by far more than the 4 ulp assert_gate_margin asks for
        want = np.minimum(np.maximum(want, gmin * F32(1.001)), top * F32(0.999))
    k3 = keep.reshape(B, H, W)
    if not case.log:        # exact hits on both gate bounds among the kept values (inclusive gate)
        hit = rng.random((B, H, W))
        want = np.where(hit < 0.02, gmin, np.where((hit < 0.04) & (case.keep_close == 0), gmax, want)).astype(F32)
    # ... and one of the values that are not kept elsewhere
    over = [F32(1.5)] if case.keep_close == 0 else [F32(0.2500001), F32(0.9)]      # keep_close zeroes what passes the gate above it
    bad_pred = np.array([0.0, -0.0, np.nan, float(gmin) * 0.5, -0.3, -np.inf, np.inf] + over, dtype=F32)
    bad_lo = np.array([0.0, -0.0, np.nan, -0.3] + ([0.9] if case.keep_close > 0 else []), dtype=F32)
    row_restored = np.zeros((1, H, 1), bool)
    if restore:
        row_restored[0, 0::f, 0] = True
    bad = np.where(row_restored, bad_lo[rng.integers(0, bad_lo.size, (B, H, W))],
                   bad_pred[rng.integers(0, bad_pred.size, (B, H, W))])
    plane0 = np.where(k3, want, bad).astype(F32)
    if restore and case.keep_close == 0 and not case.log:
        plane0[:, 0, 0] = np.where(k3[:, 0, 0], F32(1.5), plane0[:, 0, 0])      # a restored row is not gated: 1.5 is kept
    # attribute channels: anything, with NaN / inf planted in the holes of the prediction
    attrs = rng.random((B, max(C - 1, 0), H, W)).astype(F32)
    if C > 1:
        junk = np.array([np.nan, np.inf, -np.inf, 7.0], dtype=F32)[rng.integers(0, 4, attrs.shape)]
        attrs = np.where(~k3[:, None] & (rng.random(attrs.shape) < 0.5), junk, attrs).astype(F32)
    planes_dst = np.concatenate([plane0[:, None], attrs], axis=1)
    src = _source_order(case, planes_dst)
    logs = [case.log] + list(case.channel_log or [False] * (C - 1))
    with np.errstate(all="ignore"):
        for c in range(C):
            if logs[c]:
                src[:, c] = np.log1p(np.maximum(src[:, c], F32(-0.5)))
    pred = np.ascontiguousarray(src)
    lo = np.ascontiguousarray(src[:, :, 0::f, :] if restore else src[:, :, 0::f, 0:w])
    if restore:                 # what the restore overwrites is never read: make it something that would be kept
        pred[:, :, 0::f, :] = F32(0.5)
    kw = dict(log_transform=case.log, channel_log=case.channel_log or None, gate=case.gate, keep_close=case.keep_close)
    points, offsets, planes = CL.batch_cloud(pred, lo, case.dataset, **kw)
    tiles = -(-(H * W) // T)
    kept = planes[:, 0].reshape(B, -1) > 0
    pad = np.zeros((B, tiles * T), bool)
    pad[:, :H * W] = kept
    counts = pad.reshape(B * tiles, T).sum(axis=1).astype(np.int32)
    planes64 = None
    if case.log or any(case.channel_log):
        planes64 = np.stack([CL.to_destination(CL.range_planes(p, l, case.log, case.channel_log or None, case.gate,
                                                               case.keep_close, wide=True), case.dataset)
                             for p, l in zip(pred, lo)])
    return Problem(case, pred, lo, keep, points, offsets, planes, counts, planes64)


def assert_gate_margin(pb: Problem):
    """log cases: the float64 expm1 of every prediction value lies at least 4 fp32 ulp from both gate bounds"""
    if not pb.case.log:
        return
    with np.errstate(all="ignore"):
        e = np.expm1(pb.pred[:, 0].astype(np.float64))
    e = e[np.isfinite(e)]
    for g in pb.case.gate:
        g32 = F32(g)
        margin = 4.0 * float(np.spacing(g32))
        near = np.abs(e - float(g32)) < margin
        assert not near.any(), (pb.case.name, g, e[near][:4])


def assert_planted(pb: Problem):
    """the host definition keeps exactly the slots the builder planted (so the patterns are what their names say)"""
    kept = pb.planes[:, 0].reshape(pb.case.B, -1) > 0
    assert np.array_equal(kept, pb.keep), pb.case.name
    assert pb.offsets[-1] == pb.keep.sum() == pb.points.shape[0]


@functools.lru_cache(maxsize=None)
def problem(name: str, T: int, pattern: Optional[str] = None) -> Problem:
    case = {c.name: c for c in kernel_cases(T)}[name]
    pb = build(case, T, pattern)
    for a in pb[1:]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return pb


def case_names(T: int = 1024):
    return [c.name for c in kernel_cases(T)]


# ------------------------------------------------------------------------------------------------ device buffers and the comparison
def _bits(a: np.ndarray) -> np.ndarray:
    assert a.dtype == np.float32
    return np.ascontiguousarray(a).view(np.uint32)


def alloc_outputs(case: Case, T: int, device):
    """rng, counts, tile_offsets, offsets, points as eval_exact.Guarded allocations: NaN (0xFF for integers) between guard words"""
    import torch
    from tests.eval_exact import Guarded
    B, C, n = case.B, case.C, case.H * case.W
    tiles = -(-n // T)
    return {"rng": Guarded(B * C * n, torch.float32, device), "counts": Guarded(B * tiles, torch.int32, device),
            "tile_offsets": Guarded(B * tiles, torch.int64, device), "offsets": Guarded(B + 1, torch.int64, device),
            "points": Guarded(B * n * (3 + C - 1), torch.float32, device)}


def launch(pb: Problem, bufs, device):
    import torch
    from tulip_amd import ops
    c = pb.case
    geo = EV.sensor_geometry(c.dataset, c.H, c.W)
    pred, lo = torch.tensor(pb.pred, device=device), torch.tensor(pb.lo, device=device)      # copies: the problem stays read-only
    common = (pred, lo, c.B, c.C, c.H, c.W, c.h, c.w, c.log, c.channel_log, c.gate[0], c.gate[1], c.keep_close,
              EV.MAX_RANGE[c.dataset])
    outs = tuple(bufs[k].body for k in ("rng", "counts", "tile_offsets", "offsets", "points"))
    if geo.f64:
        ops.cloud_durlar(*common, torch.from_numpy(geo.colt).to(device), torch.from_numpy(geo.rowt).to(device),
                         torch.tensor(EV.DURLAR_PIXEL_OFFSET[:c.H], dtype=torch.int32, device=device), EV.DURLAR_ORIGIN_OFFSET,
                         EV.DURLAR_Z_OFFSET, *outs)
    else:
        ops.cloud_spherical(*common, *(torch.from_numpy(t).to(device) for t in geo.tables), *outs)
    torch.cuda.synchronize()


def check(pb: Problem, bufs, untouched_from: Optional[int] = None):
    """Every element of every output against the host definition; returns a list of failure strings.
    untouched_from: the first row of `points` that must still hold the pre-fill (default: offsets[B] of this problem)."""
    from tests.eval_exact import GUARD32
    c = pb.case
    n, RW = c.H * c.W, 3 + c.C - 1
    bad = []
    for name, b in bufs.items():
        v = b.guard_violation(name)
        if v:
            bad.append(v)
    counts, offsets = bufs["counts"].arr(), bufs["offsets"].arr()
    tile_offsets = bufs["tile_offsets"].arr()
    rng = bufs["rng"].arr().reshape(c.B, c.C, c.H, c.W)
    points = bufs["points"].arr().reshape(c.B * n, RW)
    if not np.array_equal(counts, pb.counts):
        bad.append(f"counts differ at {np.flatnonzero(counts != pb.counts)[:4]}")
    if not np.array_equal(offsets, pb.offsets):
        bad.append(f"offsets {offsets} != {pb.offsets}")
    want_to = np.concatenate([[0], np.cumsum(pb.counts.astype(np.int64))[:-1]])
    if not np.array_equal(tile_offsets, want_to):
        bad.append("tile_offsets are not the exclusive scan of the counts")
    N = int(pb.offsets[-1])
    if pb.planes64 is None:
        if not np.array_equal(_bits(rng), _bits(pb.planes)):
            bad.append(f"rng: {int((_bits(rng) != _bits(pb.planes)).sum())} elements differ in bits")
        if not np.array_equal(_bits(points[:N]), _bits(pb.points)):
            bad.append(f"rows: {int((_bits(points[:N]) != _bits(pb.points)).any(axis=1).sum())} rows differ in bits")
    else:
        ref = pb.planes64
        with np.errstate(all="ignore"):
            same_class = (np.isnan(rng) == np.isnan(ref)) & (np.isinf(rng) == np.isinf(ref))
            fin = np.isfinite(ref)
            err = np.abs(rng.astype(np.float64) - ref)
            budget = 2.0 * np.spacing(np.abs(ref).astype(F32)).astype(np.float64)
            ok = same_class & np.where(fin, err <= budget, np.where(np.isinf(ref), rng == ref, True))
        if not ok.all():
            bad.append(f"rng: {int((~ok).sum())} elements beyond 2 ulp of the float64 chain")
        rows = [CL.project_planes(rng[b], c.dataset) for b in range(c.B)]
        own = np.concatenate(rows, axis=0)
        if own.shape[0] != N or not np.array_equal(_bits(points[:N]), _bits(own)):
            bad.append("rows are not the host projection of the device's own rng, bit for bit")
    start = N if untouched_from is None else untouched_from
    tail = _bits(points[start:])
    if not (tail == np.uint32(GUARD32 & 0xFFFFFFFF)).all():
        bad.append(f"{int((tail != np.uint32(GUARD32 & 0xFFFFFFFF)).sum())} words at or beyond row {start} lost their pre-fill")
    return bad

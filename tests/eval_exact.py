"""Adversarial small-cloud tests of the evaluation kernels (csrc/evalpost.hip): case lists, builders, float64 references, checkers
and a numpy emulation of every launch with switchable defects (test_eval_exact_cpu.py proves the checkers sharp, the routes reached
and the refusals; test_eval_exact_gpu.py applies the checkers to the kernels through tulip_amd.ops).  Plain numpy / torch; no kernel
code and nothing of the oracle.

Every buffer a launch writes is a `Guarded` allocation: 64 guard words in front and behind, the body prefilled with a fixed NaN
pattern (0xFF bytes for integers) unless the launch needs it zero; the checkers compare the guards bit for bit.  Inputs sit inside
the same NaN guards, so a read outside an operand poisons the result.  (gemm_exact's Buf / Out / check_out describe pitched fp32 /
bf16 matrices compared whole as 32-bit words; these buffers are flat, float64 and integer among them, and most are compared to a
budget, so `Guarded` carries the same idea -- gemm_exact's guard pattern included -- in one dimension and any element size.)

1. Chamfer: per element within 6 x 2^-24 relative of the float64 nearest-neighbour distance of the float32 coordinates (derivation
   at CHAMFER_BUDGET), an exact 0 exactly 0, out[0] against the float64 sum of the launch's own dist arrays (1e-12) and against the
   reference (6 x 2^-24).  Small cases by float64 brute force; the planted case by construction (build_planted).
2. Voxel metrics: `==` (or both NaN) against a dense-grid restatement of voxelize_point_cloud / calculate_metrics in the cloud's type.
3. Post-processing: images bit for bit and both MAE within one fp32 ulp on pixel values that make every |p - t| exact in fp32.
4. Projections bit for bit against numpy in the reference's product order; the MC aggregate through numerics_domain.check_mc."""
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from tests import numerics_domain as ND
from tests.gemm_exact import GUARD32
from tests.numerics_domain import Report
from tulip_amd import evaluation as EV

F64, F32 = torch.float64, torch.float32
GUARD64 = 0x7FF8A5A5A5A5A5A5
NG = 64                                 # guard words on either side of every allocation
U = 2.0 ** -24                          # unit roundoff of fp32
# one rounding in each of dx, dy, dz (1 + u), squared (1 + u)^2, one rounding per square (1 + u), two additions of non-negative
# terms (1 + u)^2: every term of the sum carries at most (1 + u)^5 - 1 < 6u, and so does the sum; the minimum over targets of
# values each within 6u of its exact distance is within 6u of the exact minimum.  Fused multiply-adds only remove roundings.
CHAMFER_BUDGET = 6 * U
CT, CQ, RB = 1024, 4, 1024              # target points per LDS tile, query points per thread, cap of the reduction grids
MAX_BUFFER_BYTES = 16 << 20


# ------------------------------------------------------------------ allocations
class Guarded:
    """n elements of `dtype` between two runs of NG guard words.  body=None leaves the body as the guard pattern (NaN / 0xFF)."""

    def __init__(self, n, dtype, device="cpu", body=None):
        self.n, self.dtype = int(n), dtype
        if dtype == F32:
            flat = torch.full((n + 2 * NG,), GUARD32, dtype=torch.int32).view(F32)
        elif dtype == F64:
            flat = torch.full((n + 2 * NG,), GUARD64, dtype=torch.int64).view(F64)
        else:
            flat = torch.full((n + 2 * NG,), -1, dtype=dtype)
        if body is not None:
            flat[NG:NG + n] = torch.as_tensor(body, dtype=dtype).reshape(-1) if not np.isscalar(body) else body
        self.flat = flat.to(device)

    @property
    def body(self):
        return self.flat[NG:NG + self.n]

    def arr(self):
        """the body as numpy: a view for a host allocation (the emulation writes through it), a copy for a device one"""
        return self.body.cpu().numpy()

    def bytes(self):
        return self.flat.numel() * self.flat.element_size()

    def guard_violation(self, name):
        f = self.flat.cpu()
        bits = f.view(torch.int64 if f.element_size() == 8 else torch.int32)
        want = Guarded(0, self.dtype).flat
        want = want.view(bits.dtype)
        bad = torch.cat([bits[:NG] != want[:NG], bits[NG + self.n:] != want[NG:]])
        if bool(bad.any()):
            pos = int(bad.nonzero()[0])
            side = f"{NG - pos} words in front of" if pos < NG else f"{pos - NG} words behind"
            return f"{name}: {int(bad.sum())} guard words changed; first {side} the buffer"
        return None


def check_guards(rep, bufs):
    for name, b in bufs.items():
        v = b.guard_violation(name)
        if v:
            rep.violations.append(v)
            rep.worst = math.inf


def _ulp32(x):
    return ND.ulp_f32(torch.as_tensor(np.asarray(x, dtype=np.float64))).numpy()


def _worst(rep, err, budget, where):
    """max err / budget into the report; a positive error on a zero budget and a non-finite error count as infinite"""
    err, budget = np.asarray(err, dtype=np.float64).reshape(-1), np.asarray(budget, dtype=np.float64).reshape(-1)
    if not err.size:
        return np.zeros(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(budget > 0, err / np.where(budget > 0, budget, 1.0), np.where(err > 0, np.inf, 0.0))
    r = np.where(np.isfinite(err), r, np.inf)
    i = int(r.argmax())
    if r[i] >= rep.worst:
        rep.worst, rep.where = float(r[i]), f"{where}[{i}]"
    return r


def failures(reps):
    return [str(r) for r in reps if not r.ok]


# ================================================================== 1. Chamfer
def nn_route(nq, nt):
    """launch_nn's documented rule, stated once: query blocks of 256 x 4 points; enough (query block, target slice) pairs to fill the
    chip a few times over (2048 / query blocks), slices of whole 1024-point tiles.  -> (query blocks, slices, tiles per slice, points of
    the last slice)"""
    qblocks = -(-nq // (256 * CQ))
    splits = -(-2048 // qblocks)
    tiles = -(-nt // CT)
    splits = max(1, min(splits, tiles))
    chunk = -(-tiles // splits) * CT
    splits = -(-nt // chunk)
    return qblocks, splits, chunk // CT, nt - (splits - 1) * chunk


def route_traits(nq, nt):
    qb, sl, tps, last = nn_route(nq, nt)
    t = set()
    t.add("full-tile" if last % CT == 0 else "partial-tile")
    if sl > 1 and last == 1:
        t.add("one-point-last-slice")
    if tps >= 2 and last % CT:
        t.add("two-tiles-ragged")
    if tps >= 2 and last % CT == 0:
        t.add("two-tiles-full")
    if qb > 1:
        t.add("many-query-blocks")
    return t


def reduction_blocks(na, nb):
    return -(-max(na, nb) // 256)         # chamfer_partial_kernel / fill_u32_kernel before the cap of RB


@dataclass(frozen=True)
class ChamferCase:
    name: str
    na: int
    nb: int
    route_ab: tuple                       # nn_route(na, nb): a's points query b
    route_ba: tuple                       # nn_route(nb, na)
    kind: str = "uniform"                 # uniform | origin | far | ring | planted | single
    f64: bool = False
    seed: int = 0


def _both_types(name, na, nb, rab, rba, kind="uniform", seed=0):
    return [ChamferCase(f"{name}-f32", na, nb, rab, rba, kind, False, seed), ChamferCase(f"{name}-f64", na, nb, rab, rba, kind, True, seed)]


def chamfer_cases():
    c = []
    c += _both_types("1x1", 1, 1, (1, 1, 1, 1), (1, 1, 1, 1))                                  # smallest possible
    c += _both_types("1x1024", 1, 1024, (1, 1, 1, 1024), (1, 1, 1, 1))                          # one exactly full tile
    c += _both_types("1x1025", 1, 1025, (1, 2, 1, 1), (2, 1, 1, 1))                             # 2 slices, the last of one point
    c += _both_types("255x1023", 255, 1023, (1, 1, 1, 1023), (1, 1, 1, 255))                    # one partial tile
    c += _both_types("1024x2048", 1024, 2048, (1, 2, 1, 1024), (2, 1, 1, 1024))                 # full query block, two full slices
    c += _both_types("1025x3073", 1025, 3073, (2, 4, 1, 1), (4, 2, 1, 1))                       # 2 query blocks, 4 slices, last of 1
    c += _both_types("origin-600x1300", 600, 1300, (1, 2, 1, 276), (2, 1, 1, 600), "origin", 3)  # half of both clouds at 0: distance 0
    c += _both_types("far-700x1100", 700, 1100, (1, 2, 1, 76), (2, 1, 1, 700), "far", 4)         # +/-100 m, |delta| 1e-3 .. 1e-2 m
    c += _both_types("ring-300x700", 300, 700, (1, 1, 1, 700), (1, 1, 1, 300), "ring", 8)          # a at the origin, b far: padding read as points
    # 27 slices of 2 tiles, the last of 1025 points (its second tile holds one) / 20 slices of 2 full tiles
    c.append(ChamferCase("planted-40960x54273", 40960, 54273, (40, 27, 2, 1025), (54, 20, 2, 2048), "planted", False, 5))
    # 257 query blocks, 1026 > 1024 reduction blocks / 257 one-tile slices, the last of 300 points
    c += _both_types("stride-262444x1", 262444, 1, (257, 1, 1, 1), (1, 257, 1, 300), "single", 6)
    c += _both_types("stride-1x262444", 1, 262444, (1, 257, 1, 300), (257, 1, 1, 1), "single", 7)
    return c


@dataclass
class ChamferProblem:
    case: ChamferCase
    a: np.ndarray                         # [na][3] in the cloud's type
    b: np.ndarray
    a32: np.ndarray                       # the float32 coordinates the distances are defined on
    b32: np.ndarray
    dist_a: np.ndarray                    # float64 reference, [na]
    dist_b: np.ndarray
    out: float
    cand_a: tuple = None                  # planted: (partner list of every a point as CSR: starts, targets)
    cand_b: np.ndarray = None             # planted: sigma


def brute_nn(q64, t64, chunk=512):
    """float64 squared distance of every q to its nearest t, direct form"""
    out = np.empty(q64.shape[0])
    for s in range(0, q64.shape[0], chunk):
        d = q64[s:s + chunk, None, :] - t64[None, :, :]
        out[s:s + chunk] = (d * d).sum(-1).min(1)
    return out


def _widen(x32, rng):
    """the float64 cloud of a float32 one: widened, plus a perturbation below a quarter of a float32 ulp (a quarter, not a half: the
    spacing halves just below a power of two), so the kernel's cast to float32 is exercised and must give x32 back"""
    x64 = x32.astype(np.float64) + rng.uniform(-0.24, 0.24, x32.shape) * np.spacing(np.abs(x32)).astype(np.float64)
    assert np.array_equal(x64.astype(np.float32), x32)
    assert x32.size < 4 or bool((x64 != x32).any())
    return x64


LATTICE, SPACING = (40, 32, 32), 0.5


def planted_specials(na, nb):
    """(query indices with exactly one partner, target indices that hold such an only partner): the edges of the 256-thread rows and
    1024-point query blocks on one side, of the tiles (1024 k) and slices (chunk m, multiples of the tile) on the other"""
    q = [0, na - 1] + [1024 * k + d for k in range(1, na // 1024 + 1) for d in (-1, 1)] + [256 * k + d for k in range(1, na // 256 + 1) for d in (-1, 1)]
    q = list(dict.fromkeys(i for i in q if 0 <= i < na))
    t = [0, nb - 1] + [1024 * k + d for k in range(1, nb // 1024 + 1) for d in (-1, 0)]
    t = list(dict.fromkeys(j for j in t if 0 <= j < nb))
    return q, t


def build_planted(case):
    """Nearest neighbours by construction: a = a shuffled cubic lattice of spacing s, b_j = a[sigma(j)] + delta_j with |delta_j| < 0.49 s
    (asserted in float64 from the stored float32 coordinates).  A ball of radius s/2 lies inside a lattice point's Voronoi cell, so a[sigma(j)]
    is b_j's nearest a, and every b_j' planted on another lattice point is farther than 0.51 s from a_i: dist_b[j] = |delta_j|^2 and
    dist_a[i] = the minimum over i's partners, both exact in float64."""
    rng = np.random.default_rng(case.seed)
    na, nb, s = case.na, case.nb, SPACING
    assert na == LATTICE[0] * LATTICE[1] * LATTICE[2] and nb >= na
    g = np.stack(np.meshgrid(*(np.arange(n) for n in LATTICE), indexing="ij"), -1).reshape(-1, 3)
    a32 = ((g - np.array(LATTICE) / 2) * s).astype(np.float32)[rng.permutation(na)]
    qs, ts = planted_specials(na, nb)
    assert len(ts) <= len(qs)
    single = np.zeros(na, dtype=bool)
    single[qs] = True
    sigma = np.full(nb, -1, dtype=np.int64)
    sigma[ts] = qs[:len(ts)]                                          # the only partner of these queries sits on a tile / slice edge
    rest = np.concatenate([np.setdiff1d(np.arange(na), qs[:len(ts)]), rng.choice(np.flatnonzero(~single), nb - na)])
    sigma[sigma < 0] = rng.permutation(rest)
    assert np.array_equal(np.unique(sigma), np.arange(na))            # every a has a partner
    assert bool((np.bincount(sigma, minlength=na)[qs] == 1).all())
    d = rng.normal(size=(nb, 3))
    d *= (rng.uniform(0.01, 0.45, nb) * s / np.linalg.norm(d, axis=1))[:, None]
    b32 = (a32[sigma].astype(np.float64) + d).astype(np.float32)
    delta = b32.astype(np.float64) - a32[sigma].astype(np.float64)
    dist_b = (delta * delta).sum(1)
    assert float(np.sqrt(dist_b.max())) < 0.49 * s and float(dist_b.min()) > 0
    dist_a = np.full(na, np.inf)
    np.minimum.at(dist_a, sigma, dist_b)
    order = np.argsort(sigma, kind="stable")
    starts = np.concatenate([[0], np.cumsum(np.bincount(sigma, minlength=na))])
    return ChamferProblem(case, a32, b32, a32, b32, dist_a, dist_b, dist_a.mean() + dist_b.mean(), (starts, order), sigma)


def build_chamfer(case) -> ChamferProblem:
    if case.kind == "planted":
        assert not case.f64
        return build_planted(case)
    rng = np.random.default_rng(100 + case.seed + 7 * case.na + 13 * case.nb)
    na, nb = case.na, case.nb
    if case.kind == "uniform":
        a32 = rng.uniform(-50, 50, (na, 3)).astype(np.float32)
        b32 = rng.uniform(-50, 50, (nb, 3)).astype(np.float32)
    elif case.kind == "origin":                                       # range images: gated-out pixels all project to the origin
        a32 = rng.uniform(-50, 50, (na, 3)).astype(np.float32)
        b32 = rng.uniform(-50, 50, (nb, 3)).astype(np.float32)
        a32[rng.permutation(na)[:na // 2]] = 0
        b32[rng.permutation(nb)[:nb // 2]] = 0
    elif case.kind == "far":                                          # the cancellation regime of the |a|^2 + |b|^2 - 2ab form
        a32 = (rng.choice([-100.0, 100.0], (na, 3)) + rng.uniform(-2, 2, (na, 3))).astype(np.float32)
        d = rng.normal(size=(nb, 3))
        d *= (rng.uniform(1e-3, 1e-2, nb) / np.linalg.norm(d, axis=1))[:, None]
        b32 = (a32[rng.integers(0, na, nb)].astype(np.float64) + d).astype(np.float32)
    elif case.kind == "ring":                                         # a ragged tile's padding, read as points at the origin, would win
        a32 = rng.uniform(-1, 1, (na, 3)).astype(np.float32)
        d = rng.normal(size=(nb, 3))
        b32 = (d * (rng.uniform(30, 60, nb) / np.linalg.norm(d, axis=1))[:, None]).astype(np.float32)
    elif case.kind == "single":
        a32 = rng.uniform(-50, 50, (na, 3)).astype(np.float32)
        b32 = rng.uniform(-50, 50, (nb, 3)).astype(np.float32)
    else:
        raise AssertionError(case.kind)
    a64, b64 = a32.astype(np.float64), b32.astype(np.float64)
    if min(na, nb) == 1:                                              # the reference computed directly
        one, many = (a64, b64) if na == 1 else (b64, a64)
        dm = ((many - one) ** 2).sum(1)
        dist_a, dist_b = (np.array([dm.min()]), dm) if na == 1 else (dm, np.array([dm.min()]))
    else:
        dist_a, dist_b = brute_nn(a64, b64), brute_nn(b64, a64)
    if case.kind == "origin":
        assert int((dist_a == 0).sum()) == na // 2 and int((dist_b == 0).sum()) == nb // 2
    if case.kind == "far":
        r = np.sqrt(dist_b)
        assert float(np.abs(a32).min()) > 97 and float(r.max()) < 1.1e-2 and float(np.median(r)) > 5e-4
    a, b = (a32, b32) if not case.f64 else (_widen(a32, rng), _widen(b32, rng))
    return ChamferProblem(case, a, b, a32, b32, dist_a, dist_b, dist_a.mean() + dist_b.mean())


def stale_pair():
    """two problems of the same sizes for one pair of dist buffers: small distances first, then distances that are all larger"""
    rng = np.random.default_rng(11)
    na, nb = 300, 1500
    a32 = rng.uniform(-20, 20, (na, 3)).astype(np.float32)
    idx = np.concatenate([np.arange(na), rng.integers(0, na, nb - na)])
    b1 = (a32[idx] + rng.uniform(-1e-2, 1e-2, (nb, 3))).astype(np.float32)
    b2 = (a32[idx] + rng.uniform(200, 300, (nb, 3))).astype(np.float32)
    out = []
    for k, b32 in enumerate((b1, b2)):
        c = ChamferCase(f"stale-{k}", na, nb, nn_route(na, nb), nn_route(nb, na), "uniform")
        da, db = brute_nn(a32.astype(np.float64), b32.astype(np.float64)), brute_nn(b32.astype(np.float64), a32.astype(np.float64))
        out.append(ChamferProblem(c, a32, b32, a32, b32, da, db, da.mean() + db.mean()))
    assert out[0].dist_a.max() < out[1].dist_a.min() and out[0].dist_b.max() < out[1].dist_b.min()
    return out


def alloc_chamfer(pb, device="cpu"):
    """inputs inside NaN guards, outputs NaN-prefilled inside guards"""
    t = F64 if pb.case.f64 else F32
    return {"a": Guarded(pb.a.size, t, device, pb.a), "b": Guarded(pb.b.size, t, device, pb.b),
            "dist_a": Guarded(pb.case.na, F32, device), "dist_b": Guarded(pb.case.nb, F32, device),
            "scratch": Guarded(2 * RB, F64, device, 0.0), "out": Guarded(1, F64, device)}


def check_chamfer(pb, bufs) -> Report:
    rep = Report(f"chamfer {pb.case.name}")
    sums = []
    for name, ref in (("dist_a", pb.dist_a), ("dist_b", pb.dist_b)):
        got = bufs[name].arr().astype(np.float64)
        err = np.abs(got - ref)
        r = _worst(rep, err, CHAMFER_BUDGET * ref, name)
        bad = ~(r <= 1)
        if bad.any():
            i = int(bad.argmax())
            what = "an exact 0 is not 0" if ref[i] == 0 else "more than 6 x 2^-24 from the float64 distance"
            rep.violations.append(f"{name}: {int(bad.sum())} of {ref.size} elements; first [{i}] = {got[i]!r}, expected {ref[i]!r} ({what})")
        sums.append(got.sum() / ref.size)
    out = float(bufs["out"].arr()[0])
    own = sums[0] + sums[1]
    if not (math.isfinite(out) and math.isfinite(own) and abs(out - own) <= 1e-12 * abs(own)):
        rep.violations.append(f"out[0] = {out!r} is not mean(dist_a) + mean(dist_b) of the launch's own arrays ({own!r})")
    r = _worst(rep, [abs(out - pb.out)], [CHAMFER_BUDGET * pb.out], "out")
    if not r[0] <= 1:
        rep.violations.append(f"out[0] = {out!r}, reference {pb.out!r}")
    check_guards(rep, {k: bufs[k] for k in ("dist_a", "dist_b", "scratch", "out")})
    return rep


CHAMFER_DEFECTS = ("drop_last_target", "pad_origin", "skip_tile2", "queries_256", "swap_dist", "swap_inv", "gemm_form", "f64_as_f32",
                   "stale_min")


def _d32(q, t, gemm=False):
    """[nq][nt] float32 squared distances in the kernel's order of operations"""
    if gemm:
        qq, tt = (q * q).sum(1, dtype=np.float32), (t * t).sum(1, dtype=np.float32)
        return np.maximum(qq[:, None] + tt[None, :] - np.float32(2) * (q @ t.T), np.float32(0))
    dx, dy, dz = (q[:, None, k] - t[None, :, k] for k in range(3))
    return dx * dx + dy * dy + dz * dz


def _nn32(q, t, vis, extra, cand, gemm):
    """float32 minimum over the visible targets (and `extra` padding points); cand: per query candidate targets (planted case) --
    queries whose candidates are all invisible fall back to every visible target"""
    nq = q.shape[0]
    out = np.full(nq, np.inf, dtype=np.float32)
    tv = t[vis]
    if extra is not None:
        tv = np.concatenate([tv, extra])
    if cand is None:
        if tv.shape[0]:
            for s in range(0, nq, 256):
                out[s:s + 256] = _d32(q[s:s + 256], tv, gemm).min(1)
        return out
    qi, tj = cand                                                     # pairs (query, target)
    keep = vis[tj]
    qi, tj = qi[keep], tj[keep]
    d = q[qi] - t[tj]
    d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    np.minimum.at(out, qi, d2)
    lost = np.flatnonzero(np.isinf(out))
    if lost.size and tv.shape[0]:
        tt = torch.from_numpy(tv)
        for s in range(0, lost.size, 128):
            d = torch.from_numpy(q[lost[s:s + 128]])[:, None, :] - tt[None, :, :]
            out[lost[s:s + 128]] = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]).min(1).values.numpy()
    if extra is not None:
        out = np.minimum(out, _d32(q, extra, gemm).min(1))
    return out


def _as_kernel_reads(x, n, f64, defect):
    if f64 and defect == "f64_as_f32":
        return np.frombuffer(x.tobytes(), dtype=np.float32)[:3 * n].reshape(n, 3).copy()
    return x.astype(np.float32).reshape(n, 3)


def emulate_chamfer(pb, bufs, defect=None):
    """what tulip_chamfer_sq leaves in `bufs` (host allocations): minima reset, both sweeps in fp32 over the slices and tiles of
    nn_route, the two means in double"""
    assert defect is None or defect in CHAMFER_DEFECTS
    c = pb.case
    a = _as_kernel_reads(bufs["a"].arr(), c.na, c.f64, defect)
    b = _as_kernel_reads(bufs["b"].arr(), c.nb, c.f64, defect)

    def sweep(q, t, cand, prev):
        nq, nt = q.shape[0], t.shape[0]
        _, _, tps, last = nn_route(nq, nt)
        j = np.arange(nt)
        vis = np.ones(nt, dtype=bool)
        if defect == "drop_last_target":
            vis[nt - 1] = False
        if defect == "skip_tile2":
            vis &= (j % (tps * CT)) < CT
        extra = np.zeros((1, 3), dtype=np.float32) if defect == "pad_origin" and last % CT else None
        with np.errstate(invalid="ignore", over="ignore"):
            m = _nn32(q, t, vis, extra, cand, defect == "gemm_form")
        if defect == "queries_256":
            m[(np.arange(nq) % (256 * CQ)) >= 256] = np.inf
        if defect == "stale_min":                                     # atomicMin on the bit patterns of what the buffer held
            old = prev.view(np.uint32)
            m = np.where(old < m.view(np.uint32), old, m.view(np.uint32)).view(np.float32)
        return m

    ca = cb = None
    if pb.cand_a is not None:
        starts, order = pb.cand_a
        ca = (np.repeat(np.arange(c.na), np.diff(starts)), order)
        cb = (np.arange(c.nb), pb.cand_b)
    da = sweep(a, b, ca, bufs["dist_a"].arr().copy())
    db = sweep(b, a, cb, bufs["dist_b"].arr().copy())
    if defect == "swap_dist":                                         # each sweep writes the other cloud's buffer
        n = min(c.na, c.nb)
        da2, db2 = np.full(c.na, np.inf, np.float32), np.full(c.nb, np.inf, np.float32)
        da2[:n], db2[:n] = db[:n], da[:n]
        da, db = da2, db2
    bufs["dist_a"].arr()[:] = da
    bufs["dist_b"].arr()[:] = db
    sa, sb = da.astype(np.float64).sum(), db.astype(np.float64).sum()
    inv_a, inv_b = (1.0 / c.nb, 1.0 / c.na) if defect == "swap_inv" else (1.0 / c.na, 1.0 / c.nb)
    bufs["out"].arr()[0] = sa * inv_a + sb * inv_b
    return bufs


# ================================================================== 2. voxel metrics
GRID = 0.1
SCRATCH_DOUBLES = 6 * RB + 16             # partials, min/max, the four counters at word 6 RB + 8
COUNTERS_AT = 6 * RB + 8


@dataclass
class VoxelProblem:
    name: str
    pred: np.ndarray
    gt: np.ndarray
    words: int
    ref: np.ndarray                       # the eight doubles of `out`: iou, precision, recall, f1, dims x 3, status
    after: str = None                     # name of the problem run just before on the same scratch and bitmaps


def dense_grid(points, grid, lo, hi):
    """the occupancy grid of one cloud: a boolean array of ((hi - lo) / grid).astype(int) + 1 cells per axis, True where
    ((p - lo) / grid).astype(int) of some point falls -- all in the arrays' own type"""
    occ = np.zeros(((hi - lo) / grid).astype(int) + 1, dtype=bool)
    i, j, k = ((points - lo) / grid).astype(int).T
    occ[i, j, k] = True
    return occ


def grid_metrics(occ_p, occ_g):
    """IoU = |P & G| / |P | G|, precision = tp / (tp + fp), recall = tp / (tp + fn), F1 = 2 p r / (p + r) with numpy scalars: 0 / 0 is
    NaN, not an exception"""
    with np.errstate(invalid="ignore", divide="ignore"):
        tp = np.sum(occ_p & occ_g)
        iou = tp / np.sum(occ_p | occ_g)
        fp, fn = np.sum(occ_p) - tp, np.sum(occ_g) - tp
        precision, recall = tp / (tp + fp), tp / (tp + fn)
        f1 = 2 * (precision * recall) / (precision + recall)
    return iou, precision, recall, f1


def voxel_ref(pred, gt, words):
    """the reference's own steps on dense grids, in the clouds' type, grid = 0.1 in that type; a grid of more cells than the bitmaps
    hold is refused (status 1, NaN metrics, dims still reported)"""
    assert pred.dtype == gt.dtype and pred.dtype in (np.float32, np.float64)
    grid = pred.dtype.type(GRID)
    both = np.vstack((pred, gt))
    mn, mx = np.min(both, axis=0), np.max(both, axis=0)
    dims = ((mx - mn) / grid).astype(int) + 1
    cells = int(dims[0]) * int(dims[1]) * int(dims[2])
    assert cells <= 1 << 22
    if cells > 32 * words:
        return np.array([np.nan] * 4 + list(dims) + [1.0])
    m = grid_metrics(dense_grid(pred, grid, mn, mx), dense_grid(gt, grid, mn, mx))
    return np.array(list(m) + list(dims) + [0.0], dtype=np.float64)


def _lattice(t, mn, axis, ks, others):
    """points mn + k * grid computed in type t: k from `ks` on `axis`, from `others` (small) on the two other axes"""
    g, m = t(GRID), t(mn)
    p = np.empty((len(ks), 3), dtype=t)
    p[:, axis] = m + ks.astype(t) * g
    for c, o in zip([x for x in range(3) if x != axis], others):
        p[:, c] = m + o.astype(t) * g
    return p


def _box(rng, t, n, lo, hi):
    return rng.uniform(lo, hi, (n, 3)).astype(t)


def _dims_box(t, dims, rng, n):
    """n points at voxel centres of a grid of exactly `dims` voxels; the first two are the corners, a quarter of a voxel inside it, so
    (max - min) / grid = dims - 1/2 and every other point sits a quarter of a voxel from a face: no index here depends on a rounding"""
    idx = np.stack([rng.integers(0, d, n) for d in dims], 1) + 0.5
    idx[0], idx[1] = 0.25, np.array(dims) - 0.25
    return (idx * GRID).astype(t)


def voxel_problems():
    """every case in float32 and float64; a list of VoxelProblem (references included), in the order the sequences need"""
    out = []
    for t in (np.float32, np.float64):
        tn = "f32" if t == np.float32 else "f64"
        rng = np.random.default_rng(21)

        def add(name, pred, gt, words=None, after=None):
            pred, gt = np.ascontiguousarray(pred, dtype=t), np.ascontiguousarray(gt, dtype=t)
            if words is None:
                both = np.vstack((pred, gt))
                d = ((both.max(0) - both.min(0)) / t(GRID)).astype(int) + 1
                words = (int(d.prod()) + 31) // 32 + 3                # a few spare words: the capacity cases set their own
            out.append(VoxelProblem(f"{name}-{tn}", pred, gt, words, voxel_ref(pred, gt, words), after and f"{after}-{tn}"))
            return out[-1]

        # faces: every coordinate sits on a voxel face, where the index depends on the division being the correctly rounded one
        k = np.arange(1601)
        for mn in (0.0, -79.3, -12.625):
            for axis in range(3):
                kp, kg = k[k % 3 != 1], k[k % 2 == 0]
                pred = _lattice(t, mn, axis, kp, (kp % 4, (kp // 4) % 3))
                gt = _lattice(t, mn, axis, kg, (kg % 3, (kg // 3) % 4))
                off = lambda ks: (t(mn) + (ks.astype(t) + t(0.37)) * t(GRID))[:, None].repeat(3, 1)
                pred = np.vstack((pred, off(np.array([1, 2, 3]))))
                gt = np.vstack((gt, off(np.array([2, 3, 0]))))
                add(f"faces-min{mn}-axis{axis}", pred, gt)
        # the point at the maximum of each axis: index dims - 1
        p = add("axis-maximum", _box(rng, t, 400, -3, 3), _box(rng, t, 300, -3, 3))
        both = np.vstack((p.pred, p.gt))
        top = ((both.max(0) - both.min(0)) / t(GRID)).astype(int)
        assert np.array_equal(top + 1, p.ref[4:7].astype(int))
        one = np.array([[1.23, -4.56, 0.789]])
        add("one-point-same-voxel", one, one + 0.01)
        add("one-point-different-voxels", one, one + np.array([[0.31, 0.0, -0.22]]))
        p = add("all-identical", one.repeat(5, 0), one.repeat(3, 0))
        assert list(p.ref[4:7]) == [1, 1, 1] and list(p.ref[:4]) == [1, 1, 1, 1]
        big = _box(rng, t, 900, -2, 2)
        small = big[::7]
        add("pred-inside-gt", small, big)
        add("gt-inside-pred", big, small)
        p = add("disjoint", _box(rng, t, 200, -2, -1.05), _box(rng, t, 150, 1.05, 2))
        assert list(p.ref[:3]) == [0, 0, 0] and np.isnan(p.ref[3]) and p.ref[7] == 0
        p = add("unequal-3000-700", _box(rng, t, 3000, -1.5, 1.5), _box(rng, t, 700, -1.0, 1.2))
        assert p.ref[1] != p.ref[2]                                   # P != G: a precision / recall swap shows
        cells = _dims_box(t, (5, 5, 4), rng, 50)
        p = add("duplicates", cells[np.concatenate([[0, 1], rng.integers(0, 50, 9998)])], cells[rng.integers(0, 40, 6000)])
        assert p.pred.shape[0] == 10000 and len(np.unique(p.pred, axis=0)) <= 50 and p.ref[1] != p.ref[2]
        p = add("minimum-from-gt", _box(rng, t, 500, 0.5, 2), np.vstack((_box(rng, t, 200, 0.2, 1.5), [[-1.0, -1.1, -0.7]])))
        assert bool((p.gt.min(0) < p.pred.min(0)).all())
        # capacity: cells == 32 words is accepted, one more cell is refused, the call after a refusal is right (the counters reset)
        a448, b448 = _dims_box(t, (4, 4, 8), rng, 60), _dims_box(t, (4, 4, 8), rng, 40)
        p = add("capacity-4x4x8-4words", a448, b448, words=4)
        assert list(p.ref[4:]) == [4, 4, 8, 0]
        a457, b457 = _dims_box(t, (4, 5, 7), rng, 60), _dims_box(t, (4, 5, 7), rng, 40)
        p = add("capacity-4x5x7-4words", a457, b457, words=4)
        assert list(p.ref[4:]) == [4, 5, 7, 1] and np.isnan(p.ref[:4]).all()
        p = add("capacity-4x5x7-5words", a457, b457, words=5, after="capacity-4x5x7-4words")
        assert list(p.ref[4:]) == [4, 5, 7, 0]
        a129, b129 = _dims_box(t, (1, 3, 43), rng, 60), _dims_box(t, (1, 3, 43), rng, 40)
        p = add("capacity-129cells-4words", a129, b129, words=4)       # cells == 32 words + 1
        assert list(p.ref[4:]) == [1, 3, 43, 1]
        add("capacity-4x4x8-after-refusal", a448, b448, words=4, after="capacity-129cells-4words")
        add("stride-262444x5", _box(rng, t, 262444, -2, 2), _box(rng, t, 5, -2, 2))
    return out


def alloc_voxel(pb, device="cpu", scratch=None):
    t = F64 if pb.pred.dtype == np.float64 else F32
    return {"pred": Guarded(pb.pred.size, t, device, pb.pred), "gt": Guarded(pb.gt.size, t, device, pb.gt),
            "bm_pred": Guarded(pb.words, torch.int32, device, 0), "bm_gt": Guarded(pb.words, torch.int32, device, 0),
            "scratch": scratch if scratch is not None else Guarded(SCRATCH_DOUBLES, F64, device, 0.0), "out": Guarded(8, F64, device)}


def check_voxel(pb, bufs) -> Report:
    rep = Report(f"voxel {pb.name}")
    got = bufs["out"].arr()
    names = ("iou", "precision", "recall", "f1", "dims[0]", "dims[1]", "dims[2]", "status")
    for k, n in enumerate(names):
        if not (got[k] == pb.ref[k] or (np.isnan(got[k]) and np.isnan(pb.ref[k]))):
            rep.violations.append(f"{n} = {got[k]!r}, reference {pb.ref[k]!r}")
            rep.worst = math.inf
    for n in ("bm_pred", "bm_gt"):
        nz = int(np.count_nonzero(bufs[n].arr()))
        if nz:
            rep.violations.append(f"{n}: {nz} words are not zero after the call")
    counters = bufs["scratch"].arr()[COUNTERS_AT:COUNTERS_AT + 4].view(np.int64)
    if counters.any():
        rep.violations.append(f"counters left at {counters.tolist()}")
    check_guards(rep, {k: bufs[k] for k in ("bm_pred", "bm_gt", "scratch", "out")})
    return rep


VOXEL_DEFECTS = ("mul_inv_grid", "f64_on_f32", "f32_on_f64", "minmax_one_cloud", "count_duplicates", "dims_no_plus1", "round_not_trunc",
                 "capacity_ge", "dirty_bitmap", "swap_pr")


def emulate_voxel(pb, bufs, defect=None):
    """what tulip_voxel_metrics leaves in `bufs`: min / max over both clouds, keys in the clouds' own arithmetic, first-point-per-voxel
    counts through the bitmaps, the metrics in double, bitmaps and counters handed back clean"""
    assert defect is None or defect in VOXEL_DEFECTS
    pred = bufs["pred"].arr().reshape(-1, 3)
    gt = bufs["gt"].arr().reshape(-1, 3)
    t = pred.dtype.type
    at = t
    if defect == "f64_on_f32" and t == np.float32:
        at = np.float64
    if defect == "f32_on_f64" and t == np.float64:
        at = np.float32
    both = pred if defect == "minmax_one_cloud" else np.vstack((pred, gt))
    mn, mx = both.min(0).astype(at), both.max(0).astype(at)
    grid = at(GRID)

    def index(x):
        with np.errstate(invalid="ignore"):
            q = x * (at(1) / grid) if defect == "mul_inv_grid" else x / grid
            return (np.rint(q) if defect == "round_not_trunc" else np.trunc(q)).astype(np.int64)

    dims = index(mx - mn) + (0 if defect == "dims_no_plus1" else 1)
    cells = int(dims[0]) * int(dims[1]) * int(dims[2])
    cap = 32 * pb.words
    over = cells >= cap if defect == "capacity_ge" else cells > cap
    counters = bufs["scratch"].arr()[COUNTERS_AT:COUNTERS_AT + 4].view(np.int64)
    sets, bad = [], over
    for cloud in (pred, gt):
        idx = index(cloud.astype(at) - mn)
        key = (idx[:, 0] * dims[1] + idx[:, 1]) * dims[2] + idx[:, 2]
        ok = (key >= 0) & (key < cells) & (not over)
        bad = bad or not bool(ok.all())
        sets.append((np.unique(key[ok]), int(ok.sum())))
    (kp, n_p), (kg, n_g) = sets
    P, G = (n_p, n_g) if defect == "count_duplicates" else (kp.size, kg.size)
    inter = np.intersect1d(kp, kg).size
    counters += np.array([P, G, inter, int(bad)])
    P, G, I = (np.float64(v) for v in counters[:3])
    with np.errstate(invalid="ignore", divide="ignore"):
        iou, precision, recall = I / (P + G - I), I / (I + (P - I)), I / (I + (G - I))
        f1 = 2.0 * (precision * recall) / (precision + recall)
    if defect == "swap_pr":
        precision, recall = recall, precision
    out = bufs["out"].arr()
    out[:4] = np.nan if counters[3] else (iou, precision, recall, f1)
    out[4:7] = dims
    out[7] = 1.0 if counters[3] else 0.0
    counters[:] = 0
    if defect == "dirty_bitmap":
        for keys, bm in ((kp, bufs["bm_pred"].arr()), (kg, bufs["bm_gt"].arr())):
            np.bitwise_or.at(bm.view(np.uint32), keys >> 5, (np.uint32(1) << (keys & 31).astype(np.uint32)))
    return bufs


# ================================================================== 3. post-processing
EXACT_GATE = (2.0 ** -5, 1.0)            # multiples of 2^-10: a pixel exactly on an edge keeps |p - t| exact
LOG_GATE = (2 / 80, 1.0)
KEEP = 0.25
Q = 2.0 ** -10


@dataclass(frozen=True)
class PostCase:
    name: str
    H: int
    h: int
    W: int
    w: int = 0                            # 0: w == W
    logt: bool = False

    @property
    def lw(self):
        return self.w or self.W


def post_cases():
    return [PostCase("4x1x3", 4, 1, 3), PostCase("4x4x5-every-row-restored", 4, 4, 5), PostCase("6x2x255", 6, 2, 255),
            PostCase("8x2x257", 8, 2, 257), PostCase("8x4x64-power-of-two-divisors", 8, 4, 64),
            PostCase("132x33x2048-stride", 132, 33, 2048), PostCase("8x2x256-w128-nothing-restored", 8, 2, 256, 128),
            PostCase("8x2x257-log", 8, 2, 257, 0, True)]


@dataclass
class PostProblem:
    case: PostCase
    pred: np.ndarray                      # [H][W] float32
    hi: np.ndarray
    lo: np.ndarray                        # [h][w]
    gate: tuple
    probes: dict = field(default_factory=dict)


def _up(x):
    return np.nextafter(np.float32(x), np.float32(np.inf))


def _down(x):
    return np.nextafter(np.float32(x), np.float32(-np.inf))


def build_post(case) -> PostProblem:
    rng = np.random.default_rng(31 + case.H * 7 + case.W)
    H, W, h, w = case.H, case.W, case.h, case.lw
    f = H // h
    if case.logt:
        gate = LOG_GATE
        pred = rng.uniform(0, math.log1p(1.3), (H, W)).astype(np.float32)
        hi = rng.uniform(0, math.log1p(1.0), (H, W)).astype(np.float32)
        lo = rng.uniform(0, math.log1p(1.0), (h, w)).astype(np.float32)
        pred.reshape(-1)[::5] = np.float32(0.001)                      # below the gate after expm1
        pb = PostProblem(case, pred, hi, lo, gate)
        e = np.expm1(pred.astype(np.float64))
        for edge in gate:                                             # nothing within 4 fp32 ulp of a gate edge: no pixel is excluded
            assert float(np.abs(e - np.float32(edge)).min()) > 4 * float(_ulp32(edge))
        return pb
    gate = EXACT_GATE
    gmin, gmax = np.float32(gate[0]), np.float32(gate[1])
    pred = (rng.integers(0, 2048, (H, W)) * Q).astype(np.float32)
    hi = (rng.integers(0, 2048, (H, W)) * Q).astype(np.float32)
    lo = (rng.integers(0, 2048, (h, w)) * Q).astype(np.float32)
    restore = w == W
    free = [(i, j) for i in range(H) for j in range(W) if i % f or not restore][::max(1, (H * W) // 64)]
    rest = [(i, j) for i in range(H) for j in range(W) if i % f == 0][::max(1, (h * W) // 32)] if restore else []
    probes = {}
    # (pred, hi) anywhere outside the restored rows -- or inside them where every row is restored: the gate and the first MAE still see them
    anywhere = [("gate_min_kept", gmin, 0.5), ("gate_max_kept", gmax, 0.5), ("below_gate_min", _down(gmin), 0.5),
                ("above_gate_max", _up(gmax), 0.5), ("negative", -0.5, 0.25), ("keep_edge_pred", KEEP, _up(KEEP)),
                ("above_keep_pred", _up(KEEP), KEEP)]
    spots = free if free else rest[len(rest) // 2:]
    assert len(spots) >= len(anywhere), case
    for (name, p, t), (i, j) in zip(anywhere, spots):
        pred[i, j], hi[i, j] = p, t
        if restore and i % f == 0:
            lo[i // f, j] = t                                         # (a restored pixel: |p - lo| exact like |p - hi|)
        probes[name] = (i, j)
    if restore:
        # (pred, lo) in a restored row: a gated-out pred counts as 0 and is replaced; lo outside the gate survives; keep_close acts on lo
        rows = [("gated_out_restored_lo_below_gate", -1.0, Q), ("lo_above_keep", KEEP, _up(KEEP)), ("lo_keep_edge", 0.5, KEEP),
                ("lo_above_gate", 3.0, 1.5)]
        spots = [s for s in rest if s not in probes.values()]
        assert len(spots) >= 3, case
        for (name, p, l), (i, j) in zip(rows, spots):
            pred[i, j], lo[i // f, j] = p, l
            probes[name] = (i, j)
    pb = PostProblem(case, pred, hi, lo, gate, probes)
    # every |p - t| and |p - l| the kernel forms is exact in fp32
    r = post_ref(pb, 0.0)
    for d in (r["d_all"], r["d_low"]):
        assert np.array_equal(d.astype(np.float32).astype(np.float64), d)
    return pb


def post_ref(pb, keep):
    """engine:176-251 in float64: expm1, gate (inclusive, pred only), MAE, low-res MAE and row restore (only if w == W), keep_close"""
    c = pb.case
    H, W, h = c.H, c.W, c.h
    f = H // h
    p, t, l = pb.pred.astype(np.float64), pb.hi.astype(np.float64), pb.lo.astype(np.float64)
    if c.logt:
        p, t, l = np.expm1(p), np.expm1(t), np.expm1(l)
    else:
        p = p.astype(np.float32).astype(np.float64)
    kept = (p >= np.float32(pb.gate[0])) & (p <= np.float32(pb.gate[1]))
    p = np.where(kept, p, 0.0)
    d_all = np.abs(p - t)
    out = {"d_all": d_all, "mae": d_all.mean(), "kept": kept, "restored": np.zeros((H, W), dtype=bool), "p_mae": p.copy(), "t": t.copy()}
    if c.lw == W:
        d_low = np.abs(p[::f] - l)
        out["d_low"], out["mae_low"] = d_low, d_low.mean()
        p[::f] = l
        out["restored"][::f] = True
    else:
        out["d_low"], out["mae_low"] = np.zeros((h, W)), 0.0
    if keep > 0:
        p = np.where(p > np.float32(keep), 0.0, p)
        t = np.where(t > np.float32(keep), 0.0, t)
    out["pred_img"], out["hi_img"] = p, t
    return out


def alloc_post(pb, device="cpu"):
    c = pb.case
    n = c.H * c.W
    return {"pred": Guarded(n, F32, device, pb.pred), "hi": Guarded(n, F32, device, pb.hi), "lo": Guarded(c.h * c.lw, F32, device, pb.lo),
            "pred_img": Guarded(n, F32, device), "hi_img": Guarded(n, F32, device), "partials": Guarded(2 * RB, F64, device),
            "mae": Guarded(2, F32, device)}


def _pow2(n):
    return n & (n - 1) == 0


def check_post(pb, bufs, keep) -> Report:
    c = pb.case
    rep = Report(f"post {c.name} keep_close {keep}")
    ref = post_ref(pb, keep)
    mae = bufs["mae"].arr().astype(np.float64)
    if not c.logt:
        for name in ("pred_img", "hi_img"):
            got, want = bufs[name].arr(), ref[name].astype(np.float32).reshape(-1)
            bad = got.view(np.int32) != want.view(np.int32)
            if bad.any():
                k = int(bad.argmax())
                rep.violations.append(f"{name}: {int(bad.sum())} pixels differ; first ({k // c.W}, {k % c.W}) = {got[k]!r}, expected {want[k]!r}")
                rep.worst = math.inf
        for k, (name, div) in enumerate((("mae", c.H * c.W), ("mae_low", c.h * c.W))):
            want = ref[name]
            budget = float(_ulp32(want))
            if _pow2(div) or want == 0:                               # sum x 2^-k is exact in double: the one rounding to the fp32 output
                want, budget = float(np.float32(want)), 0.0
            r = _worst(rep, [abs(mae[k] - want)], [budget], name)
            if not r[0] <= 1:
                rep.violations.append(f"mae_out[{k}] = {mae[k]!r}, float64 mean {want!r}" + (" (must be equal: the divisor is a power of two)" if budget == 0 else ""))
    else:
        tol_p, tol_t = 2 * _ulp32(ref["pred_img"]), 2 * _ulp32(ref["hi_img"])
        for name, tol in (("pred_img", tol_p), ("hi_img", tol_t)):
            got, want = bufs[name].arr().astype(np.float64), ref[name].reshape(-1)
            r = _worst(rep, np.abs(got - want), np.where(want == 0, 0.0, tol.reshape(-1)), name)
            if not (r <= 1).all():
                rep.violations.append(f"{name}: {int((~(r <= 1)).sum())} pixels more than 2 fp32 ulp from float64 expm1 (gated-out pixels: not 0)")
        # per pixel: 2 ulp of each operand the kernel computed (a gated-out pred is an exact 0) and one ulp for the fp32 subtraction of
        # the perturbed operands; the sums are in double; the mean's one rounding to fp32 is one ulp of the result
        u_p = np.where(ref["kept"], 2 * _ulp32(ref["p_mae"]), 0.0)
        u_t = 2 * _ulp32(ref["t"])
        px = u_p + u_t + _ulp32(ref["d_all"])
        budgets = [px.mean() + float(_ulp32(ref["mae"]))]
        f = c.H // c.h
        l64 = np.expm1(pb.lo.astype(np.float64))
        budgets.append((u_p[::f] + 2 * _ulp32(l64) + _ulp32(ref["d_low"])).mean() + float(_ulp32(ref["mae_low"])))
        for k, name in enumerate(("mae", "mae_low")):
            r = _worst(rep, [abs(mae[k] - ref[name])], [budgets[k]], name)
            if not r[0] <= 1:
                rep.violations.append(f"mae_out[{k}] = {mae[k]!r}, float64 {ref[name]!r}, budget {budgets[k]:.3e}")
    check_guards(rep, {k: bufs[k] for k in ("pred_img", "hi_img", "partials", "mae")})
    return rep


POST_DEFECTS = ("mae_after_restore", "gate_exclusive", "restored_gated", "keep_before_mae", "lo_row_mod", "low_div_hw", "restore_when_w_differs")


def emulate_post(pb, bufs, keep, defect=None):
    """post_kernel + post_final_kernel in fp32 / double as the kernel orders them; lo is fetched by ADDRESS from its allocation"""
    assert defect is None or defect in POST_DEFECTS
    c = pb.case
    H, W, h = c.H, c.W, c.h
    f = H // h
    restore = c.lw == W or defect == "restore_when_w_differs"
    e32 = (lambda x: np.expm1(x.astype(np.float64)).astype(np.float32)) if c.logt else (lambda x: x)
    p, t = e32(bufs["pred"].arr().reshape(H, W).copy()), e32(bufs["hi"].arr().reshape(H, W).copy())
    gmin, gmax, kc = np.float32(pb.gate[0]), np.float32(pb.gate[1]), np.float32(keep)
    with np.errstate(invalid="ignore"):
        gate = (lambda x: (x > gmin) & (x < gmax)) if defect == "gate_exclusive" else (lambda x: (x >= gmin) & (x <= gmax))
        p = np.where(gate(p), p, np.float32(0))
        if defect == "keep_before_mae" and keep > 0:
            p, t = np.where(p > kc, np.float32(0), p), np.where(t > kc, np.float32(0), t)
        e_all = np.abs(p - t).astype(np.float64)
        e_low = 0.0
        if restore:
            rows = np.arange(0, H, f)
            lo_flat = bufs["lo"].flat.numpy()
            src = (rows % f if defect == "lo_row_mod" else rows // f)[:, None] * W + np.arange(W)[None, :]
            l = e32(lo_flat[np.minimum(NG + src, lo_flat.size - 1)])   # (past the allocation: the NaN of its last guard word)
            if defect == "restored_gated":
                l = np.where(gate(l), l, np.float32(0))
            e_low = np.abs(p[rows] - l).astype(np.float64).sum()
            p[rows] = l
            if defect == "mae_after_restore":
                e_all = np.abs(p - t).astype(np.float64)
        if keep > 0:
            p, t = np.where(p > kc, np.float32(0), p), np.where(t > kc, np.float32(0), t)
    bufs["pred_img"].arr()[:] = p.reshape(-1)
    bufs["hi_img"].arr()[:] = t.reshape(-1)
    inv_low = (1.0 / (H * W) if defect == "low_div_hw" else 1.0 / (h * W)) if restore else 0.0
    bufs["mae"].arr()[:] = (np.float32(e_all.sum() * (1.0 / (H * W))), np.float32(e_low * inv_low))
    nb = min(RB, -(-H * W // 256))
    bufs["partials"].arr()[:2 * nb] = 0.0
    return bufs


# ================================================================== 4. projections and the MC aggregate
XYZ_SHAPES = ((1, 1), (3, 5), (7, 257), (130, 2048))          # 130 x 2048 > 262144: the second trip of the grid-stride loop
DURLAR_SHAPES = ((4, 48), (5, 64), (128, 2056))                # W = 48: the row offset 48 == W; 128 x 2056 > 262144
MC_N, MC_T = 1048576 + 257, 2


@dataclass
class XyzProblem:
    name: str
    H: int
    W: int
    img: np.ndarray
    tables: tuple                         # spherical: sin_h, cos_h [W], sin_v, cos_v [H] float32; durlar: colt [4 W], rowt [2 H] float64, row_offset int32
    max_range: float
    ref: np.ndarray                       # [H W][3]
    durlar: bool = False


def _image(rng, H, W):
    img = rng.uniform(0, 1, (H, W)).astype(np.float32)
    img.reshape(-1)[::7] = 0
    return img


def build_xyz(H, W) -> XyzProblem:
    rng = np.random.default_rng(41 + H + W)
    img = _image(rng, H, W)
    sh, ch = (rng.uniform(-1, 1, W).astype(np.float32) for _ in range(2))
    sv, cv = (rng.uniform(-1, 1, H).astype(np.float32) for _ in range(2))
    r = img * np.float32(80)
    ref = np.stack([(sh[None, :] * cv[:, None]) * r, (ch[None, :] * cv[:, None]) * r, sv[:, None] * r], -1)
    assert ref.dtype == np.float32
    return XyzProblem(f"xyz-{H}x{W}", H, W, img, (sh, ch, sv, cv), 80.0, ref.reshape(-1, 3))


def durlar_tables(H, W):
    """the tables RangeEvaluator builds for DurLAR (evaluation.py), from the module's own sensor constants"""
    u = np.arange(W)
    enc = 2.0 * math.pi - (((W + u) % W) * (math.pi * 2.0 / W))
    el = math.pi * np.array(EV.DURLAR_ELEVATION_DEG[:H], dtype=np.float64) / 180.
    colt = np.concatenate([np.cos(enc + EV.DURLAR_ANGLE_OFF), np.sin(enc + EV.DURLAR_ANGLE_OFF),
                           EV.DURLAR_ORIGIN_OFFSET * np.cos(enc), EV.DURLAR_ORIGIN_OFFSET * np.sin(enc)])
    return colt, np.concatenate([np.cos(el), np.sin(el)]), np.array(EV.DURLAR_PIXEL_OFFSET[:H], dtype=np.int32)


def _fma64(a, b, c):
    """a b + c with (almost always) one rounding: Dekker's exact product, then a compensated sum"""
    split = 134217729.0
    p = a * b
    ah = a * split
    ah = ah - (ah - a)
    al = a - ah
    bh = b * split
    bh = bh - (bh - b)
    bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    s = p + c
    bb = s - p
    return s + (((p - (s - bb)) + (c - bb)) + e)


def durlar_points(pb_img, tables, H, W, max_range, defect=None):
    """evaluation.py:21-50 as numpy evaluates it: float32 (r - origin offset), float64 multiply-then-add, scattered to the
    staggered-beam pixel; -> ([H W][3] float64 by destination, the destination of every source pixel)"""
    colt, rowt, off = tables
    if defect == "t_in_f64":
        t = pb_img.astype(np.float64) * max_range - EV.DURLAR_ORIGIN_OFFSET
    else:
        t = (pb_img * np.float32(max_range) - np.float32(EV.DURLAR_ORIGIN_OFFSET)).astype(np.float64)
    cr, sr = rowt[:H, None], rowt[H:, None]
    if defect == "fma":
        x, y = _fma64(t * colt[None, :W], cr, colt[None, 2 * W:3 * W]), _fma64(t * colt[None, W:2 * W], cr, colt[None, 3 * W:])
    else:
        x, y = (t * colt[None, :W]) * cr + colt[None, 2 * W:3 * W], (t * colt[None, W:2 * W]) * cr + colt[None, 3 * W:]
    z = t * sr + EV.DURLAR_Z_OFFSET
    sign = 1 if defect == "offset_sign" else -1
    dst = np.arange(H)[:, None] * W + (np.arange(W)[None, :] + W + sign * off[:, None]) % W
    out = np.full((H * W, 3), np.nan)
    out[dst.reshape(-1)] = np.stack([-x, -y, z], -1).reshape(-1, 3)
    return out, dst.reshape(-1)


def build_durlar(H, W) -> XyzProblem:
    rng = np.random.default_rng(51 + H + W)
    img = _image(rng, H, W)
    tables = durlar_tables(H, W)
    ref, dst = durlar_points(img, tables, H, W, 120.0)
    assert np.array_equal(np.sort(dst), np.arange(H * W)) and not np.isnan(ref).any()       # the scatter is a permutation
    assert int(tables[2].max()) <= W
    return XyzProblem(f"durlar-{H}x{W}", H, W, img, tables, 120.0, ref, True)


def alloc_xyz(pb, device="cpu"):
    d = {"img": Guarded(pb.img.size, F32, device, pb.img), "xyz": Guarded(pb.H * pb.W * 3, F64 if pb.durlar else F32, device)}
    if pb.durlar:
        d.update(colt=Guarded(4 * pb.W, F64, device, pb.tables[0]), rowt=Guarded(2 * pb.H, F64, device, pb.tables[1]),
                 row_offset=Guarded(pb.H, torch.int32, device, pb.tables[2]))
    else:
        for k, n in enumerate(("sin_h", "cos_h", "sin_v", "cos_v")):
            d[n] = Guarded(pb.tables[k].size, F32, device, pb.tables[k])
    return d


def check_xyz(pb, bufs) -> Report:
    rep = Report(pb.name)
    got = bufs["xyz"].arr().reshape(-1, 3)
    nan = int(np.isnan(got).any(1).sum())
    if nan:
        rep.violations.append(f"{nan} points were never written (NaN left from the prefill)")
    it = np.int64 if pb.durlar else np.int32
    bad = (got.view(it) != np.ascontiguousarray(pb.ref).view(it)).any(1)
    if bad.any():
        k = int(bad.argmax())
        rep.violations.append(f"{int(bad.sum())} of {bad.size} points differ in some bit; first point {k} (row {k // pb.W}, column {k % pb.W}) = "
                              f"{got[k].tolist()}, expected {pb.ref[k].tolist()}")
        rep.worst = math.inf
    check_guards(rep, {"xyz": bufs["xyz"]})
    return rep


XYZ_DEFECTS = ("product_order", "fma", "offset_sign", "t_in_f64")


def emulate_xyz(pb, bufs, defect=None):
    assert defect is None or defect in XYZ_DEFECTS
    img = bufs["img"].arr().reshape(pb.H, pb.W)
    if pb.durlar:
        tabs = (bufs["colt"].arr(), bufs["rowt"].arr(), bufs["row_offset"].arr())
        out, _ = durlar_points(img, tabs, pb.H, pb.W, pb.max_range, defect)
        written = ~np.isnan(out).any(1)
        bufs["xyz"].arr().reshape(-1, 3)[written] = out[written]
        return bufs
    sh, ch, sv, cv = (bufs[n].arr() for n in ("sin_h", "cos_h", "sin_v", "cos_v"))
    r = img * np.float32(pb.max_range)
    if defect == "product_order":
        x, y = sh[None, :] * (cv[:, None] * r), ch[None, :] * (cv[:, None] * r)
    else:
        x, y = (sh[None, :] * cv[:, None]) * r, (ch[None, :] * cv[:, None]) * r
    bufs["xyz"].arr()[:] = np.stack([x, y, sv[:, None] * r], -1).reshape(-1)
    return bufs


def mc_stride_case():
    """(preds [T][n] float32, threshold): n beyond 4096 blocks x 256, the second trip of mc_aggregate's grid-stride loop"""
    g = torch.Generator().manual_seed(61)
    base = torch.rand(MC_N, generator=g) * 80
    return torch.stack([base, base + torch.randn(MC_N, generator=g) * 0.05 * base]).contiguous(), 0.03


def largest_buffer_bytes():
    """the largest single allocation of any case, from the case lists alone"""
    n = [MC_T * MC_N * 4]
    n += [max(c.na, c.nb) * 3 * (8 if c.f64 else 4) for c in chamfer_cases()]
    n += [c.H * c.W * 4 for c in post_cases()] + [H * W * 12 for H, W in XYZ_SHAPES] + [H * W * 24 for H, W in DURLAR_SHAPES]
    n += [262444 * 3 * 8, 2 * RB * 8]
    return max(n) + 2 * NG * 8

"""Dense point clouds from the model on the device: `CloudUpsampler`, and the host (numpy) definition of what it computes --
what tulip_cloud_spherical / tulip_cloud_durlar compute (include/tulip_hip.h; csrc/cloud.hip).  The numpy functions are used by the
tests; nothing on the hot path calls them.

One image: pred (C, H, W) and lo (C, h, w), float32 in the model's value space, C = 1..4; f = H // h; rows are restored iff w == W.

    range plane   the chain of tulip_eval_postprocess without a target: p = expm1(pred_0) if log_transform (float32);
                  p = (gmin <= p <= gmax) ? p : 0 (inclusive; a NaN fails it);  rows 0::f: p = the inverse-transformed lo_0 iff
                  w == W;  keep_close > 0: p above it becomes 0
    hole          p == 0.0 after the gate, before the rows are restored (true for -0.0 and for what failed the gate)
    channel c>=1  the prediction side of eval_channels.py: a = expm1(pred_c) if channel_log[c-1];  a = hole ? +0.0 : a (a select:
                  a NaN or an infinity in a hole yields +0.0);  restored rows: a = the inverse of lo_c;  0 where keep_close zeroed
                  the pixel
    kept          a pixel is kept iff its final range r > 0.0: false for -0.0, +0.0 and a NaN, true for +inf (which only a
                  restored row can hold: the gate removes it from a prediction)
    coordinates   float32.  kitti / carla: r' = r * max_range; x = (sin_h[j] * cos_v[i]) * r'; y = (cos_h[j] * cos_v[i]) * r';
                  z = sin_v[i] * r' -- float32 products in that order (tulip_range_to_xyz).  durlar: t = float32(r * max_range) -
                  origin_offset in float32, then the unfused float64 expressions of tulip_range_to_xyz_durlar, rounded once to
                  float32
    order         the row order of the evaluator's pcd_pred with the rows that are not kept removed: row-major pixel order, and for
                  durlar the staggered index v*W + (u + W - row_offset[v]) % W ("destination order")
    row           (x, y, z, a_1 .. a_{C-1})

A batch is the concatenation of its images in order; offsets has B+1 int64 entries, offsets[0] = 0, image b owns rows
offsets[b]:offsets[b+1]; an image with no kept pixel gives two equal offsets.  The post-processed planes (`range_images`) are kept
in destination order, so that row k of an image's cloud is the k-th positive element of its flattened range plane.
"""
from __future__ import annotations

import numbers
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import evaluation as EV
from . import ops
from .infer import GraphedForward

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- host definition
def _flags(C: int, channel_log: Optional[Sequence[bool]]):
    lg = [False] * (C - 1) if channel_log is None else [bool(v) for v in channel_log]
    if len(lg) != C - 1:
        raise ValueError(f"{C} channels take {C - 1} log flags")
    return lg


def _expm1(a: np.ndarray) -> np.ndarray:
    """float32: torch's expm1, which is what the reference's evaluate() applies (numpy's float32 expm1 is up to 2 ulp off)"""
    if a.dtype == np.float32:
        return torch.expm1(torch.from_numpy(np.ascontiguousarray(a))).numpy()
    return np.expm1(a)


def range_planes(pred, lo, log_transform: bool, channel_log: Optional[Sequence[bool]], gate: Tuple[float, float],
                 keep_close: float = 0.0, wide: bool = False) -> np.ndarray:
    """The post-processed planes (C, H, W) float32 of one image, in pixel order.  wide=True: the same chain on the float64 values
    of the inputs (expm1 in float64), returned as float64 -- what a test measures a device expm1 against."""
    pred, lo = np.asarray(pred), np.asarray(lo)
    if pred.dtype != np.float32 or lo.dtype != np.float32 or pred.ndim != 3 or lo.ndim != 3 or lo.shape[0] != pred.shape[0]:
        raise ValueError("pred must be (C, H, W) and lo (C, h, w) float32 arrays")
    C, H, W = pred.shape
    h, w = lo.shape[1:]
    if not 1 <= C <= 4 or h <= 0 or H % h:
        raise ValueError("C must be 1..4 and H a multiple of h")
    lg = [bool(log_transform)] + _flags(C, channel_log)
    f, restore = H // h, w == W
    gmin, gmax, kc, zero = F32(gate[0]), F32(gate[1]), F32(keep_close), F32(0.0)
    with np.errstate(all="ignore"):
        inv = lambda a, c: _expm1(a) if lg[c] else a.copy()
        if wide:
            pred, lo = pred.astype(np.float64), lo.astype(np.float64)
        p = [inv(pred[c], c) for c in range(C)]
        p[0] = np.where((p[0] >= gmin) & (p[0] <= gmax), p[0], zero)
        hole = p[0] == zero
        for c in range(C):
            if c:
                p[c] = np.where(hole, zero, p[c])
            if restore:
                p[c][0::f] = inv(lo[c], c)
        if kc > 0:
            far = p[0] > kc
            for c in range(C):
                p[c][far] = zero
    return np.stack(p) if wide else np.stack(p).astype(np.float32, copy=False)


def _row_offset(dataset_select: str, H: int) -> np.ndarray:
    return np.asarray(EV.DURLAR_PIXEL_OFFSET[:H], dtype=np.int64) if dataset_select == "durlar" else np.zeros(H, dtype=np.int64)


def destination_columns(dataset_select: str, H: int, W: int) -> np.ndarray:
    """(H, W) int64: the destination column of pixel (v, u); the identity except for durlar's staggered beams"""
    u = np.arange(W)[None, :]
    return (u + W - _row_offset(dataset_select, H)[:, None]) % W


def to_destination(planes: np.ndarray, dataset_select: str) -> np.ndarray:
    """(..., H, W) planes in pixel order -> in destination order"""
    H, W = planes.shape[-2:]
    out = np.empty_like(planes)
    np.put_along_axis(out, np.broadcast_to(destination_columns(dataset_select, H, W), planes.shape), planes, axis=-1)
    return out


def project_planes(planes_dst: np.ndarray, dataset_select: str) -> np.ndarray:
    """Post-processed planes (C, H, W) in destination order -> the cloud (kept, 3 + C - 1) float32"""
    planes_dst = np.asarray(planes_dst)
    C, H, W = planes_dst.shape
    geo = EV.sensor_geometry(dataset_select, H, W)
    R = EV.MAX_RANGE[dataset_select]
    r = planes_dst[0]
    with np.errstate(all="ignore"):
        if geo.f64:
            src = (np.arange(W)[None, :] + _row_offset(dataset_select, H)[:, None]) % W      # source column of every slot
            t = (r * F32(R) - F32(EV.DURLAR_ORIGIN_OFFSET)).astype(np.float64)
            assert (r * F32(R)).dtype == np.float32
            c0, c1, c2, c3 = (geo.colt[k * W:(k + 1) * W][src] for k in range(4))
            cos_el, sin_el = geo.rowt[:H][:, None], geo.rowt[H:][:, None]
            x = (t * c0) * cos_el + c2
            y = (t * c1) * cos_el + c3
            z = t * sin_el
            xyz = np.stack((-x, -y, z + EV.DURLAR_Z_OFFSET), axis=-1).astype(np.float32)
        else:
            sh, ch, sv, cv = geo.tables
            rr = r * F32(R)
            xyz = np.stack(((sh[None, :] * cv[:, None]) * rr, (ch[None, :] * cv[:, None]) * rr,
                            np.broadcast_to(sv[:, None], rr.shape) * rr), axis=-1)
            assert xyz.dtype == np.float32
        keep = (r > F32(0.0)).reshape(-1)
    rows = np.concatenate([xyz.reshape(-1, 3)] + [planes_dst[c].reshape(-1, 1) for c in range(1, C)], axis=1)
    return np.ascontiguousarray(rows[keep])


def image_cloud(pred, lo, dataset_select: str, log_transform: bool = False, channel_log: Optional[Sequence[bool]] = None,
                gate: Optional[Tuple[float, float]] = None, keep_close: float = 0.0):
    """One image: (cloud (kept, 3 + C - 1) float32, planes (C, H, W) float32 in destination order)"""
    gate = EV.pred_gate(dataset_select, False) if gate is None else gate
    planes = to_destination(range_planes(pred, lo, log_transform, channel_log, gate, keep_close), dataset_select)
    return project_planes(planes, dataset_select), planes


def batch_cloud(pred, lo, dataset_select: str, log_transform: bool = False, channel_log: Optional[Sequence[bool]] = None,
                gate: Optional[Tuple[float, float]] = None, keep_close: float = 0.0):
    """pred (B, C, H, W), lo (B, C, h, w) -> (points (N, 3 + C - 1) float32, offsets (B + 1,) int64, planes (B, C, H, W))"""
    clouds, planes = zip(*(image_cloud(p, l, dataset_select, log_transform, channel_log, gate, keep_close)
                           for p, l in zip(np.asarray(pred), np.asarray(lo))))
    offsets = np.zeros(len(clouds) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([c.shape[0] for c in clouds])
    return np.concatenate(clouds, axis=0), offsets, np.stack(planes)


# ---------------------------------------------------------------------------------------------------------------- the device path
class _ForwardThenCloud(GraphedForward):
    """GraphedForward whose captured work ends with the owner's three cloud launches"""

    def __init__(self, model, batch_size, device, tail):
        super().__init__(model, batch_size, device)
        self._tail = tail

    def _forward(self):
        super()._forward()
        self._tail(self.P.pred, self.P.x_in)


def _check_gate(gate):
    if isinstance(gate, (str, bytes)) or not hasattr(gate, "__len__") or len(gate) != 2 or \
            not all(isinstance(v, numbers.Real) and not isinstance(v, (bool, np.bool_)) for v in gate):
        raise ValueError(f"gate must be (gmin, gmax), got {gate!r}")
    return float(gate[0]), float(gate[1])


class CloudUpsampler:
    """Low-resolution batches in, dense point clouds out, without leaving the device.

    `up(lo)` takes the (B, C, h, w) float32 device batch RangePrep / DeviceRangeLoader / KittiRangeProjector produce, runs the
    model's eval forward and the cloud stretch (post-processing, projection, ordered compaction; module docstring) as one HIP graph
    and returns (points, offsets): the (B*H*W, 3+C-1) float32 capacity buffer whose first offsets[B] rows are the batch's clouds,
    and the (B+1,) int64 offsets.  Nothing synchronises with the host; both tensors are static buffers, valid until the next call.
    `clouds()` synchronises once and returns the B views points[offsets[b]:offsets[b+1]].  `from_pred(pred, lo)` is the same
    stretch for a prediction the caller made, e.g. an mc_aggregate result.  `range_images` holds the (B, C, H, W) post-processed
    planes of the last call in the clouds' row order.  As with GraphedForward the Dropout flags in force are part of the graph:
    changing them re-captures."""

    def __init__(self, model, dataset_select: str, batch_size: int, log_transform: bool = False, channel_log=None,
                 keep_close: float = 0.0, gate=None, device=None):
        self.ds = dataset_select
        self.gate = EV.pred_gate(dataset_select, False) if gate is None else _check_gate(gate)    # unknown dataset: NotImplementedError
        if isinstance(batch_size, (bool, np.bool_)) or not isinstance(batch_size, numbers.Integral) or batch_size < 1:
            raise ValueError(f"batch_size must be a positive int, got {batch_size!r}")
        self.B = int(batch_size)
        C = getattr(model, "in_chans", 1)
        if C == 1:
            if channel_log is not None and len(channel_log):
                raise ValueError("in_chans == 1 has no channel_log entries")
            self.in_chans, self.channel_log = 1, ()
        else:
            self.in_chans, self.channel_log = EV._check_channels(C, channel_log)
        if isinstance(keep_close, (bool, np.bool_)) or not isinstance(keep_close, numbers.Real) or not keep_close >= 0.0:
            raise ValueError(f"keep_close must be a number >= 0 (0: off), got {keep_close!r}")
        self.keep_close, self.log_transform = float(keep_close), bool(log_transform)
        self.h, self.w = (int(v) for v in model.img_size)
        self.H, self.W = (int(v) for v in model.target_img_size)
        if self.h <= 0 or self.H % self.h:
            raise ValueError(f"target height {self.H} is not a multiple of the input height {self.h}")
        geo = EV.sensor_geometry(dataset_select, self.H, self.W)      # the KITTI size check and the DurLAR row limit
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise RuntimeError("tulip_amd.cloud runs on the GPU only (HIP kernels, no CPU fallback)")
        dev, B, C, H, W = self.device, self.B, self.in_chans, self.H, self.W
        self.f64 = geo.f64
        if geo.f64:
            self.colt = torch.from_numpy(geo.colt).to(dev)
            self.rowt = torch.from_numpy(geo.rowt).to(dev)
            self.row_offset = torch.tensor(EV.DURLAR_PIXEL_OFFSET[:H], dtype=torch.int32, device=dev)
        else:
            self.tables = [torch.from_numpy(t).to(dev) for t in geo.tables]
        tiles = -(-(H * W) // ops.cloud_tile())
        self.rng = torch.zeros(B, C, H, W, dtype=torch.float32, device=dev)
        self.counts = torch.zeros(B * tiles, dtype=torch.int32, device=dev)
        self.tile_offsets = torch.zeros(B * tiles, dtype=torch.int64, device=dev)
        self.offsets = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        self.points = torch.zeros(B * H * W, 3 + C - 1, dtype=torch.float32, device=dev)
        self.forward = _ForwardThenCloud(model, B, dev, self._cloud)

    def _cloud(self, pred, lo):
        """the three launches on the current stream: pred (B,C,H,W), lo (B,C,h,w) -> rng, counts, tile_offsets, offsets, points"""
        common = (pred, lo, self.B, self.in_chans, self.H, self.W, self.h, self.w, self.log_transform, self.channel_log,
                  self.gate[0], self.gate[1], self.keep_close, EV.MAX_RANGE[self.ds])
        outs = (self.rng, self.counts, self.tile_offsets, self.offsets, self.points)
        if self.f64:
            ops.cloud_durlar(*common, self.colt, self.rowt, self.row_offset, EV.DURLAR_ORIGIN_OFFSET, EV.DURLAR_Z_OFFSET, *outs)
        else:
            ops.cloud_spherical(*common, *self.tables, *outs)

    def _check(self, t, shape, name):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or tuple(t.shape) != shape:
            raise ValueError(f"{name}: expected a float32 device tensor of shape {shape}")
        return t.contiguous()

    @property
    def range_images(self) -> torch.Tensor:
        return self.rng

    @torch.no_grad()
    def __call__(self, lo: torch.Tensor):
        lo = self._check(lo, (self.B, self.in_chans, self.h, self.w), "lo")
        self.forward(lo)
        return self.points, self.offsets

    @torch.no_grad()
    def from_pred(self, pred: torch.Tensor, lo: torch.Tensor):
        pred = self._check(pred, (self.B, self.in_chans, self.H, self.W), "pred")
        lo = self._check(lo, (self.B, self.in_chans, self.h, self.w), "lo")
        self._cloud(pred, lo)
        return self.points, self.offsets

    def clouds(self) -> List[torch.Tensor]:
        """the clouds of the last call as B views of the capacity buffer (the one host synchronisation: reading the offsets)"""
        off = self.offsets.tolist()
        return [self.points[off[b]:off[b + 1]] for b in range(self.B)]

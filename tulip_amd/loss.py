"""The training loss, TULIP(loss="l1" | "l2" | "berhu", loss_edge_weight=w) -- the host definition of what csrc/loss.hip computes on the device.

The reference's forward_loss is L1 (tulip.py:690-700), and that stays the default.  The alternative it imports and leaves unused
(tulip.py:11, util/evaluation.py:177-180, inverse_huber_loss) is berHu, the usual depth-regression loss; L2 is its other half.
With d = pred - target and n = pred.numel():

    l1      loss = mean |d|                                   gradient  sign(d) / n
    l2      loss = mean d^2                                   gradient  2 d / n
    berhu   C = 0.2 * max |d|                                 (read with .item() in the reference: a constant under autograd)
            value_i = |d_i| where |d_i| < C, else (d_i^2 + C^2) / (2 C)
            loss = mean value_i                               (the reference function returns the elementwise tensor; the mean is
                                                               how forward_loss would use it)
            gradient  sign(d_i) / n where |d_i| < C, else d_i / (C n)           -- nothing flows through C

One departure from the reference: C == 0 (pred equals target everywhere) makes its formula 0/0 = NaN; here loss and gradient are 0,
so that a perfect prediction is not a non-finite step.  A NaN or an infinity anywhere in pred or target makes the loss non-finite
and at least the affected gradient elements with it (numpy's max keeps a NaN; the device's max is written to do the same), so the
non-finite guard and train_one_epoch's abort still see it.  `pixel_loss`, the second value the model returns, keeps its meaning for
every kind: the L1 metric, mean |expm1(pred) - expm1(target)| with log_transform and mean |pred - target| without.

The functions below are that table in numpy float64 (the device works in float32: C there is the float32 product
float32(0.2) * float32(max |d|), `berhu_c32`).  With world > 1 and with accum_iter > 1 C is per rank and per micro-batch, as in the
reference, where every rank computes its own loss on its own batch.

The valid-pixel mask, TULIP(loss_valid_min=v) -- `valid_min=v` below.  A range image has pixels with no return, written as 0
(util/datasets.py:143-150; log1p keeps them 0).  With target of shape (B, C, ...), pixel (b, y, x) is valid iff
target[b, 0, y, x] > v: the rule reads channel 0, the range (a hole has no intensity either, while a valid return may have
intensity 0), and the comparison is false for a NaN.  All C elements of a valid pixel count, n_v = C * (valid pixels), and every
row of the table above is that loss over the valid elements with n_v in place of n (berHu's C: the max over the valid |d|);
pixel_loss likewise.  The gradient at an invalid element is +0.  n_v == 0 gives loss 0, pixel_loss 0, C 0 and all gradients 0
(a second departure from 0/0).  Whatever pred or any channel of target holds at an invalid pixel -- a NaN, an infinity -- changes
nothing; a non-finite value at a valid element propagates as above.  n_v and C are per call.  valid_min=None (the default): every
element counts, and each function returns what it returns without the keyword, bit for bit.

The edge term, TULIP(loss_edge_weight=w) -- `edge_weight=w` below.  Every loss above is a per-pixel function of d; an upsampler
smears depth discontinuities, and a gradient term beside the pixel loss is the usual remedy.  The reference ships the two filters
(tulip.py:9 imports util/filter.py: HorizontalEdgeDetectionCNN and VerticalEdgeDetectionCNN, each a fixed 3x3 Sobel filter in a
Conv2d(1, 1, 3, padding=1, bias=False)) and leaves them unused; the loss built from them is this project's.  With d (B, C, H, W):

    K_h = [[-1,-2,-1],[0,0,0],[1,2,1]]     K_v = K_h transposed
    e_h[b,c,y,x] = sum_{i,j in 0..2} K_h[i,j] d[b,c,y+i-1,x+j-1]      (0 outside the H x W plane, the conv's zero padding; every
    e_v likewise with K_v                                              (b, c) plane on its own; the columns do not wrap)
    edge  = (1/n) sum (|e_h| + |e_v|)
    total = base(kind, valid_min) + w * edge                          (base: loss_value)
    k[b,c,p,q] = sum_{i,j} K_h[i,j] sign(e_h[b,c,p-i+1,q-j+1]) + the same with K_v       (sign(0) = 0, the torch subgradient;
    d total / d pred = base gradient + w * k / n                       terms whose centre is outside the plane: 0)

k is an integer in [-16, 16].  With the mask: d is +0 at an invalid pixel (by selection: a NaN or an infinity there reaches
nothing), a response counts only where its centre pixel is valid (and contributes 0 to k elsewhere), the normaliser is n_v
(n_v == 0: edge 0, gradient 0) and the gradient at an invalid element stays +0.  pixel_loss does not change, log_transform plays
no part, and the term is per rank and per micro-batch, as berHu's C is.  A NaN response contributes 0 to k and makes the edge sum,
and the loss with it, NaN.  The device's float32 arithmetic (csrc/loss.hip, tulip_loss_edge_*) is restated by the *32 functions:
d32 = fl32(pred - target); e_h = ((d[+1,-1] - d[-1,-1]) + 2 (d[+1,0] - d[-1,0])) + (d[+1,+1] - d[-1,+1]), one rounding per
operation (d[dy,dx]; e_v: the transposed pattern); ge = fl32(fl32(w) * g) with g the base gradient's fl32(gscale / n) (n_v with
the mask); dpred = fl32(base_grad + fl32(ge * k)); edge32 = fl32(sum / n), the sum folded in double;
total32 = fl32(base32 + fl32(fl32(w) * edge32)).  edge_weight=0.0 (the default): every function returns what it returns without
the keyword, bit for bit.

The channel weights, TULIP(loss_channel_weights=(w_0, ..., w_{C-1})) -- `channel_weights=` below.  Range, intensity and the other
channels of a multi-channel image have other scales and other noise.  With pred, target (B, C, ...), element (b, c, ...) is COUNTED
iff its pixel is valid (above; always without a mask) and w_c > 0; S is the set of counted elements and n_S their number:

    loss     = (1/n_S) sum_{i in S} w_c(i) f_kind(d_i)               f: |d|, d^2 or the berHu value
    gradient   w_c f'(d_i) / n_S on S, +0 off S
    berHu      one C = 0.2 * max_{i in S} |d_i|: unweighted, shared by the channels, NaN-keeping, a constant under differentiation
    pixel_loss the unweighted L1 metric over S, with n_S (the rule the mask follows)
    edge     = (1/n_S) sum_{(b,c,y,x) in S} w_c (|e_h| + |e_v|)      responses per plane, d +0 at an invalid pixel; a plane with
               gradient w_e w_c k / n_S                              w_c == 0 contributes nothing and gets gradient +0

A weight of 0 removes a channel by selection, as the mask removes a pixel: a NaN or an infinity in pred or target of a w_c == 0
channel changes no value and no gradient -- except that channel 0 of target decides validity even where w_0 == 0.  n_S == 0 gives
zeros.  (1, 0, ...) is the single-channel loss of channel 0, all ones the loss without the keyword.  The device's float32
arithmetic (csrc/loss.hip, the _w entry points; loss_grad32 / loss_values32 / edge_grad32 / edge_total32 restate it): g =
fl32(gscale / n_S) as without weights, then g_c = fl32(fl32(w_c) * g) once per channel, which stands wherever g stands in the
gradient; the edge gradient uses ge_c = fl32(fl32(w_e) * g_c); value terms are fl32(fl32(w_c) * term), summed as before, the fold in
double.  With every w_c == 1.0 each product is exact.  channel_weights=None (the default): every function returns what it returns
without the keyword, bit for bit.
"""
from __future__ import annotations

import numpy as np

KINDS = ("l1", "l2", "berhu")
BERHU_FRACTION = 0.2


def check_loss(name) -> str:
    """The loss of TULIP(loss=...): "l1", "l2" or "berhu" (ValueError for anything else)."""
    if not isinstance(name, str) or name not in KINDS:
        raise ValueError(f"loss must be one of {KINDS}, got {name!r}")
    return name


def check_valid_min(v):
    """The threshold of TULIP(loss_valid_min=...): None (no mask) or a finite float, returned as a Python float (ValueError for a
    bool, a NaN, an infinity or any other type -- an int among them: the value is in the target's units, write 0.0)."""
    if v is None:
        return None
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (float, np.floating)) or not np.isfinite(v):
        raise ValueError(f"loss_valid_min must be None or a finite float, got {v!r}")
    return float(v)


def check_channel_weights(w, in_chans):
    """The weights of TULIP(loss_channel_weights=...): None (no weights), or a tuple or list of exactly in_chans finite floats >= 0
    with at least one > 0, returned as a tuple of Python floats (ValueError for anything else -- a bool, an int, a NaN, an infinity,
    a negative value, a wrong length, all zeros: check_edge_weight's strictness).  in_chans == 1 with (w,) is a plain scale."""
    if w is None:
        return None
    if not isinstance(w, (tuple, list)) or len(w) != in_chans:
        raise ValueError(f"loss_channel_weights must be None or a tuple of in_chans = {in_chans} floats, got {w!r}")
    for v in w:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (float, np.floating)) or not np.isfinite(v) or v < 0:
            raise ValueError(f"loss_channel_weights must be finite floats >= 0, got {w!r}")
    if not any(v > 0 for v in w):
        raise ValueError(f"loss_channel_weights needs at least one weight > 0, got {w!r}")
    return tuple(float(v) for v in w)


def _weights_like(target, channel_weights, dtype=np.float64) -> np.ndarray:
    """w_c broadcast to target's shape (B, C, ...)"""
    target = np.asarray(target)
    if target.ndim < 2:
        raise ValueError(f"channel_weights needs arrays of shape (B, C, ...), got {target.shape}")
    w = np.asarray(check_channel_weights(tuple(channel_weights), target.shape[1]), dtype=dtype)
    return np.broadcast_to(w.reshape((1, -1) + (1,) * (target.ndim - 2)), target.shape)


def counted_mask(target, valid_min=None, channel_weights=None) -> np.ndarray:
    """S as a bool array of target's shape: the valid elements (valid_mask) of the channels with w_c > 0."""
    m = valid_mask(target, valid_min)
    return m if channel_weights is None else m & (_weights_like(target, channel_weights) > 0)


def _counted(pred, target, valid_min, channel_weights):
    """(pred, target, weights) compressed to S, and S"""
    m = counted_mask(target, valid_min, channel_weights)
    return np.asarray(pred)[m], np.asarray(target)[m], _weights_like(target, channel_weights)[m], m


def valid_mask(target, valid_min) -> np.ndarray:
    """The valid elements of target (B, C, ...) as a bool array of its shape: target[b, 0, ...] > valid_min, broadcast over the
    channels (false for a NaN); all true for valid_min=None."""
    target = np.asarray(target)
    valid_min = check_valid_min(valid_min)
    if valid_min is None:
        return np.ones(target.shape, dtype=bool)
    if target.ndim < 2:
        raise ValueError(f"valid_mask needs a target of shape (B, C, ...), got {target.shape}")
    with np.errstate(all="ignore"):
        return np.broadcast_to(target[:, :1] > valid_min, target.shape).copy()


def _valid(pred, target, valid_min):
    """(pred, target) compressed to the valid elements, and the mask"""
    m = valid_mask(target, valid_min)
    return np.asarray(pred)[m], np.asarray(target)[m], m


def _diff(pred, target):
    pred, target = np.asarray(pred, dtype=np.float64), np.asarray(target, dtype=np.float64)
    with np.errstate(all="ignore"):
        return pred - target


def berhu_c(pred, target, valid_min=None, channel_weights=None) -> np.float64:
    """C = 0.2 * max |pred - target| in float64 (NaN when any difference is NaN); over the valid elements with valid_min (0 when
    there is none); over S with channel_weights."""
    if channel_weights is not None:
        p, t, _, _ = _counted(pred, target, valid_min, channel_weights)
        return np.float64(0.0) if p.size == 0 else berhu_c(p, t)
    if valid_min is not None:
        p, t, _ = _valid(pred, target, valid_min)
        return np.float64(0.0) if p.size == 0 else berhu_c(p, t)
    with np.errstate(all="ignore"):
        return np.float64(BERHU_FRACTION) * np.max(np.abs(_diff(pred, target)))


def berhu_c32(pred, target, valid_min=None, channel_weights=None) -> np.float32:
    """The device's C: float32(0.2) * float32(max |d|), d formed in float32 -- one float32 product."""
    if channel_weights is not None:
        p, t, _, _ = _counted(pred, target, valid_min, channel_weights)
        return np.float32(0.0) if p.size == 0 else berhu_c32(p, t)
    if valid_min is not None:
        p, t, _ = _valid(pred, target, valid_min)
        return np.float32(0.0) if p.size == 0 else berhu_c32(p, t)
    with np.errstate(all="ignore"):
        d = np.asarray(pred, dtype=np.float32) - np.asarray(target, dtype=np.float32)
        return np.float32(BERHU_FRACTION) * np.float32(np.max(np.abs(d)))


def berhu_values(pred, target, c=None, valid_min=None, channel_weights=None) -> np.ndarray:
    """The elementwise berHu values (what inverse_huber_loss returns) for the threshold c (default: berhu_c); with valid_min the
    values of the valid elements (c's default: the masked berhu_c) and 0 at the others; with channel_weights the UNWEIGHTED values
    on S (c's default: the max over S) and 0 off it."""
    if channel_weights is not None:
        p, t, _, m = _counted(pred, target, valid_min, channel_weights)
        out = np.zeros(m.shape, dtype=np.float64)
        if p.size:
            out[m] = berhu_values(p, t, c)
        return out
    if valid_min is not None:
        p, t, m = _valid(pred, target, valid_min)
        out = np.zeros(m.shape, dtype=np.float64)
        if p.size:
            out[m] = berhu_values(p, t, c)
        return out
    d = _diff(pred, target)
    c = berhu_c(pred, target) if c is None else np.float64(c)
    if c == 0.0:
        return np.zeros_like(d)
    a = np.abs(d)
    with np.errstate(all="ignore"):
        return np.where(a < c, a, (a * a + c * c) / (2.0 * c))


def loss_value(kind: str, pred, target, valid_min=None, channel_weights=None) -> np.float64:
    """The scalar training loss of `kind` in float64; over the valid elements with valid_min (0 when there is none); with
    channel_weights (1/n_S) sum_S w_c f(d)."""
    kind = check_loss(kind)
    if channel_weights is not None:
        p, t, w, _ = _counted(pred, target, valid_min, channel_weights)
        if p.size == 0:
            return np.float64(0.0)
        d = _diff(p, t)
        with np.errstate(all="ignore"):
            f = np.abs(d) if kind == "l1" else d * d if kind == "l2" else berhu_values(p, t)
            return np.sum(w * f) / f.size
    if valid_min is not None:
        p, t, _ = _valid(pred, target, valid_min)
        return np.float64(0.0) if p.size == 0 else loss_value(kind, p, t)
    d = _diff(pred, target)
    with np.errstate(all="ignore"):
        if kind == "l1":
            return np.mean(np.abs(d))
        if kind == "l2":
            return np.mean(d * d)
        return np.mean(berhu_values(pred, target))


def loss_grad(kind: str, pred, target, gscale: float = 1.0, valid_min=None, channel_weights=None) -> np.ndarray:
    """gscale * d(loss_value) / d(pred) in float64, the shape of pred; +0 at the invalid elements with valid_min; with
    channel_weights w_c times the gradient over S, +0 off S."""
    kind = check_loss(kind)
    if channel_weights is not None:
        p, t, w, m = _counted(pred, target, valid_min, channel_weights)
        out = np.zeros(m.shape, dtype=np.float64)
        if p.size:
            with np.errstate(all="ignore"):
                out[m] = w * loss_grad(kind, p, t, gscale)
        return out
    if valid_min is not None:
        p, t, m = _valid(pred, target, valid_min)
        out = np.zeros(m.shape, dtype=np.float64)
        if p.size:
            out[m] = loss_grad(kind, p, t, gscale)
        return out
    d = _diff(pred, target)
    n = d.size
    with np.errstate(all="ignore"):
        if kind == "l1":
            g = np.sign(d) / n
        elif kind == "l2":
            g = 2.0 * d / n
        else:
            c = berhu_c(pred, target)
            g = np.zeros_like(d) if c == 0.0 else np.where(np.abs(d) < c, np.sign(d) / n, d / (c * n))
        return np.float64(gscale) * g


def pixel_loss(pred, target, log_transform: bool, valid_min=None, channel_weights=None) -> np.float64:
    """The logged L1 metric, the same for every kind (tulip.py:695-698); over the valid elements with valid_min (0 when there is
    none); with channel_weights over S, unweighted."""
    if channel_weights is not None:
        p, t, _, _ = _counted(pred, target, valid_min, channel_weights)
        return np.float64(0.0) if p.size == 0 else pixel_loss(p, t, log_transform)
    if valid_min is not None:
        p, t, _ = _valid(pred, target, valid_min)
        return np.float64(0.0) if p.size == 0 else pixel_loss(p, t, log_transform)
    pred, target = np.asarray(pred, dtype=np.float64), np.asarray(target, dtype=np.float64)
    with np.errstate(all="ignore"):
        if log_transform:
            return np.mean(np.abs(np.expm1(pred) - np.expm1(target)))
        return np.mean(np.abs(pred - target))


def _weights32(target, channel_weights) -> np.ndarray:
    """fl32(w_c) broadcast to target's shape; ones without weights"""
    if channel_weights is None:
        return np.ones(np.shape(target), dtype=np.float32)
    return _weights_like(target, channel_weights, np.float32)


def loss_grad32(kind: str, pred, target, gscale: float = 1.0, valid_min=None, channel_weights=None) -> np.ndarray:
    """The device's dpred behind tulip_loss_bwd(_m / _w), in float32: d = fl32(pred - target), g = fl32(fl32(gscale) / fl32(n_S)) (0
    when n_S == 0), g_c = fl32(fl32(w_c) * g) (g itself without weights), then l1: +-g_c by the sign of d (0 at 0 and at a NaN);
    l2: fl32(fl32(2 d) * g_c); berhu with C = berhu_c32 over S: +-g_c where |d| < C, 0 where C == 0, else fl32(fl32(d / C) * g_c);
    +0 off S."""
    kind = check_loss(kind)
    m = counted_mask(target, valid_min, channel_weights)
    ns = int(m.sum())
    with np.errstate(all="ignore"):
        d = np.asarray(pred, dtype=np.float32) - np.asarray(target, dtype=np.float32)
        g = np.float32(gscale) / np.float32(ns) if ns else np.float32(0.0)
        gc = (_weights32(target, channel_weights) * g).astype(np.float32)
        sign = np.where(d > 0, gc, np.where(d < 0, -gc, np.float32(0.0)))
        if kind == "l1":
            out = sign
        elif kind == "l2":
            out = (np.float32(2.0) * d) * gc
        else:
            c = berhu_c32(pred, target, valid_min, channel_weights) if channel_weights is not None else berhu_c32(pred, target, valid_min)
            if c == 0.0:
                out = np.where(np.abs(d) < c, sign, np.float32(0.0))
            else:
                out = np.where(np.abs(d) < c, sign, (d / c) * gc)
    return np.where(m, out, np.float32(0.0)).astype(np.float32)


def loss_values32(kind: str, pred, target, log_transform: bool = False, valid_min=None, channel_weights=None):
    """(loss32, pixel32) as the device's final fold forms them: the float32 terms fl32(fl32(w_c) * term) (l1: |d|; l2: fl32(fl32(w_c
    d) * d); berhu: the float32 value for C = berhu_c32) and, for pixel32, the unweighted metric terms, each summed in double over
    S and multiplied by 1 / n_S (0 when n_S == 0), then rounded.  (The device sums a workgroup's terms in float32 first: the same
    bits wherever those sums are exact, integer-valued terms for instance.)"""
    kind = check_loss(kind)
    m = counted_mask(target, valid_min, channel_weights)
    ns = int(m.sum())
    w = _weights32(target, channel_weights)[m]
    with np.errstate(all="ignore"):
        p, t = np.asarray(pred, dtype=np.float32)[m], np.asarray(target, dtype=np.float32)[m]
        d = p - t
        a = np.abs(d)
        if kind == "l1":
            terms = w * a
        elif kind == "l2":
            terms = (w * d) * d
        else:
            c = berhu_c32(p, t) if ns else np.float32(0.0)
            v = np.zeros_like(a) if c == 0.0 else np.where(a < c, a, (a * a + c * c) / (np.float32(2.0) * c))
            terms = w * v.astype(np.float32)
        metric = np.abs(np.expm1(p) - np.expm1(t)) if log_transform else a
        inv = 1.0 / ns if ns else 0.0
        return (np.float32(np.sum(terms.astype(np.float64)) * inv), np.float32(np.sum(metric.astype(np.float64)) * inv))


def check_edge_weight(w) -> float:
    """The weight of TULIP(loss_edge_weight=...): a finite float >= 0, returned as a Python float (ValueError for a bool, an int,
    a NaN, an infinity, a negative value or any other type: check_valid_min's strictness)."""
    if isinstance(w, (bool, np.bool_)) or not isinstance(w, (float, np.floating)) or not np.isfinite(w) or w < 0:
        raise ValueError(f"loss_edge_weight must be a finite float >= 0, got {w!r}")
    return float(w)


def _shifted(a: np.ndarray, dy: int, dx: int) -> np.ndarray:
    """s[..., y, x] = a[..., y + dy, x + dx], 0 outside the plane (the last two axes); dy, dx in -1..1"""
    H, W = a.shape[-2:]
    p = np.zeros(a.shape[:-2] + (H + 2, W + 2), dtype=a.dtype)
    p[..., 1:H + 1, 1:W + 1] = a
    return p[..., 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def _responses(d: np.ndarray):
    """(e_h, e_v) of d (..., H, W) in d's dtype, in the device's order of operations"""
    s = lambda dy, dx: _shifted(d, dy, dx)
    with np.errstate(all="ignore"):
        two = d.dtype.type(2)
        e_h = ((s(1, -1) - s(-1, -1)) + two * (s(1, 0) - s(-1, 0))) + (s(1, 1) - s(-1, 1))
        e_v = ((s(-1, 1) - s(-1, -1)) + two * (s(0, 1) - s(0, -1))) + (s(1, 1) - s(1, -1))
    return e_h, e_v


def _plane_check(a: np.ndarray) -> np.ndarray:
    if a.ndim < 2:
        raise ValueError(f"the edge term needs planes (..., H, W), got {a.shape}")
    return a


def edge_responses(d):
    """(e_h, e_v): the two Sobel responses of d (..., H, W) in float64, every plane on its own, zero outside it -- what the
    reference's HorizontalEdgeDetectionCNN / VerticalEdgeDetectionCNN return for d."""
    return _responses(_plane_check(np.asarray(d, dtype=np.float64)))


def edge_responses32(d):
    """edge_responses in float32 with the device's roundings (d: float32 already, or rounded to it here)"""
    return _responses(_plane_check(np.asarray(d, dtype=np.float32)))


def _edge_diff(pred, target, valid_min, dtype, channel_weights=None):
    """(d, mask): d = pred - target in dtype, +0 by selection at the invalid pixels (with channel_weights: off S -- the planes are
    independent, so a w_c == 0 plane's d reaches nothing either way)"""
    m = counted_mask(target, valid_min, channel_weights)
    with np.errstate(all="ignore"):
        d = np.asarray(pred, dtype=dtype) - np.asarray(target, dtype=dtype)
    return _plane_check(np.where(m, d, dtype(0))), m


def _adjoint(s_h: np.ndarray, s_v: np.ndarray) -> np.ndarray:
    """k[p, q] = sum_{i,j} K_h[i,j] s_h[p-i+1, q-j+1] + K_v[i,j] s_v[p-i+1, q-j+1] (0 outside the plane)"""
    h, v = (lambda dy, dx: _shifted(s_h, dy, dx)), (lambda dy, dx: _shifted(s_v, dy, dx))
    k_h = (h(-1, 1) + 2 * h(-1, 0) + h(-1, -1)) - (h(1, 1) + 2 * h(1, 0) + h(1, -1))
    k_v = (v(1, -1) + 2 * v(0, -1) + v(-1, -1)) - (v(1, 1) + 2 * v(0, 1) + v(-1, 1))
    return k_h + k_v


def _sign(e: np.ndarray) -> np.ndarray:
    with np.errstate(all="ignore"):
        return (e > 0).astype(np.int64) - (e < 0).astype(np.int64)           # a NaN: 0


def _edge_k(d: np.ndarray, m: np.ndarray, responses) -> np.ndarray:
    e_h, e_v = responses(d)
    k = _adjoint(np.where(m, _sign(e_h), 0), np.where(m, _sign(e_v), 0))
    return np.where(m, k, 0)


def edge_value(pred, target, valid_min=None, channel_weights=None) -> np.float64:
    """edge = (1/n) sum (|e_h| + |e_v|) of d = pred - target in float64; with valid_min over the responses centred on a valid
    pixel, with n_v (0 when there is none); with channel_weights (1/n_S) sum_S w_c (|e_h| + |e_v|)."""
    d, m = _edge_diff(pred, target, valid_min, np.float64, channel_weights)
    nv = int(m.sum())
    if nv == 0:
        return np.float64(0.0)
    e_h, e_v = _responses(d)
    with np.errstate(all="ignore"):
        if channel_weights is not None:
            return np.sum((_weights_like(target, channel_weights) * (np.abs(e_h) + np.abs(e_v)))[m]) / nv
        return np.sum((np.abs(e_h) + np.abs(e_v))[m]) / nv


def edge_grad_int(pred, target, valid_min=None, channel_weights=None) -> np.ndarray:
    """k = n * d(edge) / d(pred): an int64 array of pred's shape, every value in [-16, 16]; 0 at the invalid elements.  With
    channel_weights: n_S * d(edge) / d(pred) = w_c * k, and k is 0 off S."""
    d, m = _edge_diff(pred, target, valid_min, np.float64, channel_weights)
    return _edge_k(d, m, _responses)


def edge_grad32(pred, target, base_grad32, weight, gscale: float = 1.0, valid_min=None, channel_weights=None) -> np.ndarray:
    """The device's dpred behind tulip_loss_edge_bwd, in float32: fl32(base_grad32 + fl32(ge * k)), ge = fl32(fl32(weight) * g),
    g = fl32(gscale / n) (n_v with valid_min, 0 when there is none); +0 at the invalid elements.  With channel_weights: n_S, and
    ge_c = fl32(fl32(weight) * fl32(fl32(w_c) * g)) per plane; +0 off S."""
    d, m = _edge_diff(pred, target, valid_min, np.float32, channel_weights)
    k = _edge_k(d, m, _responses).astype(np.float32)
    nv = int(m.sum())
    with np.errstate(all="ignore"):
        g = np.float32(gscale) / np.float32(nv) if nv else np.float32(0.0)
        if channel_weights is not None:
            g = (_weights32(target, channel_weights) * g).astype(np.float32)
        ge = np.float32(check_edge_weight(float(weight))) * g
        out = np.asarray(base_grad32, dtype=np.float32) + ge * k
    return np.where(m, out, np.float32(0.0)) if (valid_min is not None or channel_weights is not None) else out


def edge_total32(pred, target, base32, weight, valid_min=None, channel_weights=None):
    """(edge32, total32) as the device forms them: edge32 = fl32(sum * (1 / n)) with the float32 terms fl32(|e_h| + |e_v|) summed
    in double (the device sums a workgroup's terms in float32 first: the same bits wherever those sums are exact, integer
    inputs for instance), total32 = fl32(base32 + fl32(fl32(weight) * edge32)).  With channel_weights: the terms
    fl32(fl32(w_c) * fl32(|e_h| + |e_v|)) over S, and n_S."""
    d, m = _edge_diff(pred, target, valid_min, np.float32, channel_weights)
    nv = int(m.sum())
    e_h, e_v = _responses(d)
    with np.errstate(all="ignore"):
        terms = np.abs(e_h) + np.abs(e_v)
        if channel_weights is not None:
            terms = (_weights32(target, channel_weights) * terms).astype(np.float32)
        s = np.sum(terms[m].astype(np.float64))
        edge32 = np.float32(s * (1.0 / nv if nv else 0.0))
        total32 = np.float32(base32) + np.float32(check_edge_weight(float(weight))) * edge32
    return edge32, total32


def _torch_edge(d):
    """sum (|e_h| + |e_v|) of d (B, C, H, W) on torch tensors"""
    import torch
    import torch.nn.functional as F
    k_h = torch.tensor([[-1.0, -2.0, -1.0], [0.0, 0.0, 0.0], [1.0, 2.0, 1.0]], dtype=d.dtype, device=d.device)
    planes = d.reshape(-1, 1, *d.shape[-2:])
    e_h = F.conv2d(planes, k_h[None, None], padding=1)
    e_v = F.conv2d(planes, k_h.t()[None, None], padding=1)
    return (e_h.abs() + e_v.abs()).reshape(d.shape)


def _torch_counted(target, valid_min, channel_weights):
    """(S as a bool tensor, w_c broadcast to target's shape) on torch tensors"""
    import torch
    w = check_channel_weights(tuple(channel_weights), target.shape[1])
    wt = torch.tensor(w, dtype=target.dtype, device=target.device).reshape((1, -1) + (1,) * (target.dim() - 2)).expand_as(target)
    m = wt > 0
    if check_valid_min(valid_min) is not None:
        m = m & (target[:, :1] > valid_min).expand_as(target)
    return m, wt


def _torch_loss_weighted(kind: str, pred, target, valid_min, edge_weight, channel_weights):
    """torch_loss with channel_weights: everything by indexing with S, so that nothing off S reaches the value or the gradient"""
    import torch
    kind = check_loss(kind)
    m, wt = _torch_counted(target, valid_min, channel_weights)
    ns = int(m.sum())
    full = pred - target
    d, w = full[m], wt[m]
    if ns == 0:
        return d.sum()
    a = d.abs()
    if kind == "l1":
        f = a
    elif kind == "l2":
        f = d * d
    else:
        c = (BERHU_FRACTION * a.detach().max()).item()
        f = a * 0.0 if c == 0.0 else torch.where(a < c, a, (a * a + c * c) / (2.0 * c))
    total = (w * f).sum() / ns
    if edge_weight != 0.0:
        total = total + edge_weight * ((wt * _torch_edge(torch.where(m, full, torch.zeros_like(full))))[m].sum() / ns)
    return total


def torch_loss(kind: str, pred, target, valid_min=None, edge_weight=0.0, channel_weights=None):
    """The same definition on torch tensors, differentiable in pred (C detached, as the reference's .item() leaves it): what a
    test or a CPU experiment back-propagates through an autograd model.  With valid_min: over the valid elements (indexing, not
    a product with the mask: a NaN at an invalid pixel reaches neither the value nor the gradient).  edge_weight > 0 adds the
    edge term (pred, target: (B, C, H, W)); 0.0 returns the value without it, bit for bit.  channel_weights: the weighted
    definition over S; None returns the value without the keyword, bit for bit."""
    import torch
    edge_weight = check_edge_weight(edge_weight)
    if channel_weights is not None:
        return _torch_loss_weighted(kind, pred, target, valid_min, edge_weight, channel_weights)
    if edge_weight != 0.0:
        base = torch_loss(kind, pred, target, valid_min)
        d = pred - target
        if check_valid_min(valid_min) is None:
            return base + edge_weight * (_torch_edge(d).sum() / d.numel())
        m = (target[:, :1] > valid_min).expand_as(target)
        nv = int(m.sum())
        if nv == 0:
            return base
        return base + edge_weight * (_torch_edge(torch.where(m, d, torch.zeros_like(d)))[m].sum() / nv)
    kind = check_loss(kind)
    d = pred - target
    if check_valid_min(valid_min) is not None:
        d = d[(target[:, :1] > valid_min).expand_as(target)]
        if d.numel() == 0:
            return d.sum()                               # no valid pixel: 0, with a zero gradient
    if kind == "l1":
        return d.abs().mean()
    if kind == "l2":
        return (d * d).mean()
    a = d.abs()
    c = (BERHU_FRACTION * a.detach().max()).item()
    if c == 0.0:
        return (a * 0.0).mean()
    return torch.where(a < c, a, (a * a + c * c) / (2.0 * c)).mean()

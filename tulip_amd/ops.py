"""Tensor-level wrappers over the C ABI (tulip_amd/_lib.py).  Outputs are caller-allocated; every
call is asynchronous on torch's current HIP stream (so it is captured by torch.cuda.graph)."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib
from ._lib import (EPI_BF16, EPI_F32, EPI_GELU_BWD, EPI_GELU_DUAL,  # noqa: F401
                   EPI_PIXSHUF2_F32, EPI_RESID_F32, EPI_SPLIT_F32, EPI_UNSHUF2_BF16, check)

BF16 = torch.bfloat16
F32 = torch.float32


def _p(t):
    """tensor -> device address; ints (precomputed addresses) and None pass through."""
    if t is None or isinstance(t, int):
        return t
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk(t: torch.Tensor, dtype, name: str):
    if t.dtype != dtype or not t.is_cuda or not t.is_contiguous():
        raise TypeError(f"{name}: expected contiguous {dtype} device tensor, got {t.dtype} "
                        f"{'cuda' if t.is_cuda else 'cpu'} contiguous={t.is_contiguous()}")


def _gemm_flags(accumulate, touch, checked, mid, b_packed):
    """the `accumulate` flag word of tulip_gemm_bf16"""
    accumulate = int(bool(accumulate)) | (0 if touch else _lib.GEMM_NO_TOUCH) | (_lib.GEMM_CHECKED if checked else 0)
    accumulate |= 0 if mid is None else (_lib.GEMM_MID if mid else _lib.GEMM_NO_MID)     # the 192 x 192 mid-size kernel: forced / never
    accumulate |= _lib.GEMM_B_PACKED if b_packed else 0      # B = the fragment-major copy of the [N][K] matrix: the small-K form
    return accumulate


def gemm_route(M, N, K, *, a_trans=False, b_trans=False, epi=EPI_BF16, accumulate=False, splits=1, touch=True, checked=False,
               mid=None, b_packed=False) -> int:
    """tulip_gemm_route: the kernel gemm(...) launches for these arguments as the TULIP_ROUTE_* bit field of tulip_hip.h
    (_lib.ROUTE_*); host code only, needs no GPU.  Raises where gemm(...) refuses the shape or the flags."""
    r = _lib.load().tulip_gemm_route(M, N, K, int(a_trans), int(b_trans), epi, _gemm_flags(accumulate, touch, checked, mid, b_packed),
                                     splits)
    check(min(r, 0), "tulip_gemm_route")
    return r


def gemm(A, B, M, N, K, *, lda, ldb, a_trans=False, b_trans=False, epi=EPI_BF16, bias=None, out=None, ldo=None,
         out2=None, ldo2=0, aux=None, ldaux=0, rowscale=None, rows_per_sample=1, accumulate=False, psH=0, psW=0,
         splits=1, workspace=None, workspace_bytes=0, touch=True, checked=False, mid=None, b_packed=False):
    """C[M,N] = opA . opB^T with a fused epilogue (see include/tulip_hip.h).  A/B/out may be views
    with an element offset (row strides passed as lda/ldb/ldo).  touch=False / checked=True: TULIP_GEMM_NO_TOUCH /
    TULIP_GEMM_CHECKED (measurement and bit-compare switches, per call)."""
    lib = _lib.load()
    accumulate = _gemm_flags(accumulate, touch, checked, mid, b_packed)
    rc = lib.tulip_gemm_bf16(_p(A), lda, int(a_trans), _p(B), ldb, int(b_trans), M, N, K, epi, _p(bias), _p(out),
                             ldo if ldo is not None else N, _p(out2), ldo2, _p(aux), ldaux, _p(rowscale),
                             rows_per_sample, int(accumulate), psH, psW, splits, _p(workspace), workspace_bytes,
                             _stream())
    check(rc, "tulip_gemm_bf16")


def layernorm_fwd(x, gamma, beta, y, mean, rstd, rows, C, eps, merge=False, B=0, H=0, W=0):
    rc = _lib.load().tulip_layernorm_fwd(_p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), rows, C, eps,
                                         int(merge), B, H, W, _stream())
    check(rc, "tulip_layernorm_fwd")


def layernorm_bwd(dy, x, mean, rstd, gamma, dres, dx, rows, C, merge=False, B=0, H=0, W=0, param_partials=None,
                  dx_bf16=None, cast_rowscale=None, cast_rows_per_sample=1):
    rc = _lib.load().tulip_layernorm_bwd(_p(dy), _p(x), _p(mean), _p(rstd), _p(gamma), _p(dres), _p(dx), rows, C,
                                         int(merge), B, H, W, _p(param_partials), _p(dx_bf16), _p(cast_rowscale),
                                         cast_rows_per_sample, _stream())
    check(rc, "tulip_layernorm_bwd")


def layernorm_bwd_splitk(slabs, nslab, x, mean, rstd, gamma, dres, dx, rows, C, merge=False, B=0, H=0, W=0,
                         param_partials=None, dx_bf16=None, cast_rowscale=None, cast_rows_per_sample=1):
    """layernorm_bwd on the raw split-K slabs of the data-gradient GEMM in front (tulip_layernorm_bwd_splitk)."""
    rc = _lib.load().tulip_layernorm_bwd_splitk(_p(slabs), nslab, _p(x), _p(mean), _p(rstd), _p(gamma), _p(dres), _p(dx),
                                                rows, C, int(merge), B, H, W, _p(param_partials), _p(dx_bf16),
                                                _p(cast_rowscale), cast_rows_per_sample, _stream())
    check(rc, "tulip_layernorm_bwd_splitk")


def splitk_resid_ln_supported(N):
    return bool(_lib.load().tulip_splitk_resid_ln_supported(N))


def splitk_resid_ln(slabs, nslab, M, N, bias, aux, ldaux, rowscale, rows_per_sample, out, ldo, out_bf16, ldo2, gamma, beta,
                    ln_out, mean, rstd, eps):
    """Split-K fold + residual epilogue + the following LayerNorm in one launch (tulip_splitk_resid_ln)."""
    check(_lib.load().tulip_splitk_resid_ln(_p(slabs), nslab, M, N, _p(bias), _p(aux), ldaux, _p(rowscale), rows_per_sample,
                                            _p(out), ldo, _p(out_bf16), ldo2, _p(gamma), _p(beta), _p(ln_out), _p(mean),
                                            _p(rstd), eps, _stream()), "tulip_splitk_resid_ln")


def layernorm_bwd_partial_rows(rows, C):
    return _lib.load().tulip_layernorm_bwd_partial_rows(rows, C)


def reduce_rows2(part0, stride0, out0, n0, part1, stride1, out1, n1, nrows):
    check(_lib.load().tulip_reduce_rows2(_p(part0), stride0, _p(out0), n0, _p(part1), stride1, _p(out1), n1, nrows,
                                         _stream()), "tulip_reduce_rows2")


def reduce_region(part, stride, out, n, rows, overwrite=False, scatter_index=None, scatter_nh=0, scatter_len=0, adamw=False):
    """One tulip_reduce_region: out[i] (+)= sum_s part[s*stride + i]; see include/tulip_hip.h.  adamw: the fold takes the
    optimizer step of out[0..n) instead of storing the sum (reduce_rows_multi(..., adam=adamw_ref(...)))."""
    return _lib.ReduceRegion(_p(part), _p(out), stride, n, rows, int(overwrite), _p(scatter_index), scatter_nh,
                             scatter_len, int(adamw))


def wgrad_item(dY, ldy, X, ldx, Nw, Kw, Mtok, dW, db=None, splits=1, overwrite=False, adamw=False):
    return _lib.WgradItem(_p(dY), _p(X), _p(dW), _p(db), ldy, ldx, Nw, Kw, Mtok, splits, int(overwrite), int(adamw))


def adamw_ref(hyper, grad, param, exp_avg, exp_avg_sq, param_bf16, decay_mask64=None, lr_scale64=None):
    """tulip_adamw_ref: the flat buffers tulip_wgrad_group_adamw / tulip_reduce_rows_multi_adamw step in (all laid out like
    `grad`); decay_mask64: tulip_adamw's mask (bit 0: weight decay for these 64 elements; None: everywhere).
    lr_scale64 (needs the mask): the 64-float table of per-group learning-rate scales, group = mask byte >> 2 -- it rides on the
    returned object and sends wgrad_group / reduce_rows_multi to the `_s` entry points."""
    if lr_scale64 is not None and decay_mask64 is None:
        raise ValueError("lr_scale64 needs decay_mask64: the group index lives in bits 2-7 of the mask bytes")
    ref = _lib.AdamwRef(_p(hyper), _p(grad), _p(param), _p(exp_avg), _p(exp_avg_sq), _p(param_bf16), _p(decay_mask64))
    ref.lr_scale64 = _p(lr_scale64)
    return ref


def pack_lr_groups(decay_mask64: torch.Tensor, block_scale) -> tuple:
    """The carrier of per-parameter learning-rate scales: (mask bytes, table).  `block_scale`: one float per 64-float block
    (a sequence or 1-d tensor as long as the mask).  The scales are quantised to float32 and their distinct values numbered --
    1.0 is always group 0 --; a block's group goes into bits 2-7 of its mask byte, bits 0 (decay) and 1 (stepped elsewhere) stay
    as they are, and table[group] is the scale (64 float32 on the CPU, unused entries 1.0).  More than 64 distinct scales:
    ValueError."""
    sc = torch.as_tensor(block_scale, dtype=torch.float32).reshape(-1).cpu()
    mask = decay_mask64.detach().cpu()
    if mask.dtype != torch.uint8 or mask.numel() != sc.numel():
        raise ValueError("pack_lr_groups: one uint8 mask byte and one scale per 64-float block")
    if not bool(torch.isfinite(sc).all()) or bool((sc < 0).any()):
        raise ValueError("learning-rate scales must be finite and >= 0")
    values = [1.0] + sorted(set(sc.tolist()) - {1.0}, reverse=True)
    if len(values) > _lib.LR_GROUPS_MAX:
        raise ValueError(f"{len(values)} distinct learning-rate scales (1.0 included): the fused AdamW carries at most "
                         f"{_lib.LR_GROUPS_MAX} groups (bits 2-7 of the decay mask bytes)")
    table = torch.ones(_lib.LR_GROUPS_MAX, dtype=torch.float32)
    table[:len(values)] = torch.tensor(values, dtype=torch.float32)
    group = torch.zeros_like(mask)
    for gi, val in enumerate(values):
        group[sc == val] = gi
    return (mask & 3) | (group << _lib.LR_GROUP_SHIFT), table


def reduce_rows_multi(regions, adam=None):
    if len(regions) > _lib.REDUCE_REGIONS_MAX:
        raise ValueError("too many regions for one launch")
    arr = (_lib.ReduceRegion * max(len(regions), 1))(*regions)
    if adam is None:
        check(_lib.load().tulip_reduce_rows_multi(arr, len(regions), _stream()), "tulip_reduce_rows_multi")
    elif getattr(adam, "lr_scale64", None) is not None:
        check(_lib.load().tulip_reduce_rows_multi_adamw_s(arr, len(regions), ctypes.byref(adam), adam.lr_scale64, _stream()),
              "tulip_reduce_rows_multi_adamw_s")
    else:
        check(_lib.load().tulip_reduce_rows_multi_adamw(arr, len(regions), ctypes.byref(adam), _stream()),
              "tulip_reduce_rows_multi_adamw")


def wgrad_tiles(Nw, Kw, small_tiles=False):
    """Workgroup tiles per token split of a [Nw][Kw] weight gradient in the grouped launch (tulip_wgrad_tiles)."""
    return _lib.load().tulip_wgrad_tiles(Nw, Kw, _lib.WGRAD_SMALL_TILES if small_tiles else 0)


def wgrad_group_profiled(items, workspace, workspace_bytes, stamps, small_tiles=False):
    """tulip_wgrad_group_profiled: the grouped launch alone; stamps = int64 device tensor [workgroups, 4] (phase stamps)."""
    ia = (_lib.WgradItem * max(len(items), 1))(*items)
    check(_lib.load().tulip_wgrad_group_profiled(ia, len(items), _p(workspace), workspace_bytes,
                                                 _lib.WGRAD_SMALL_TILES if small_tiles else 0, _p(stamps), _stream()),
          "tulip_wgrad_group_profiled")


def wgrad_group(items, extra, workspace, workspace_bytes, fold=True, adam=None, small_tiles=False):
    """tulip_wgrad_group: grouped weight-gradient GEMM + one fold launch that also carries the `extra` regions.
    adam (ops.adamw_ref): items built with adamw=True take their optimizer step in the write-out (tulip_wgrad_group_adamw).
    small_tiles: TULIP_WGRAD_SMALL_TILES (the 64 x 96 tile everywhere; A/B measurements)."""
    ia = (_lib.WgradItem * max(len(items), 1))(*items)
    ea = (_lib.ReduceRegion * max(len(extra), 1))(*extra)
    fold = int(bool(fold)) | (_lib.WGRAD_SMALL_TILES if small_tiles else 0)
    if adam is None:
        check(_lib.load().tulip_wgrad_group(ia, len(items), ea, len(extra), _p(workspace), workspace_bytes, int(fold),
                                            _stream()), "tulip_wgrad_group")
    elif getattr(adam, "lr_scale64", None) is not None:
        check(_lib.load().tulip_wgrad_group_adamw_s(ia, len(items), ea, len(extra), _p(workspace), workspace_bytes, int(fold),
                                                    ctypes.byref(adam), adam.lr_scale64, _stream()), "tulip_wgrad_group_adamw_s")
    else:
        check(_lib.load().tulip_wgrad_group_adamw(ia, len(items), ea, len(extra), _p(workspace), workspace_bytes, int(fold),
                                                  ctypes.byref(adam), _stream()), "tulip_wgrad_group_adamw")


def wgrad_group_regions(items, workspace):
    """The fold regions of a grouped launch issued with fold=False (tulip_wgrad_group_regions)."""
    ia = (_lib.WgradItem * max(len(items), 1))(*items)
    out = (_lib.ReduceRegion * _lib.REDUCE_REGIONS_MAX)()
    n = _lib.load().tulip_wgrad_group_regions(ia, len(items), _p(workspace), out, _lib.REDUCE_REGIONS_MAX)
    check(min(n, 0), "tulip_wgrad_group_regions")
    return [out[i] for i in range(n)]


def layernorm_bwd_params(dy, x, mean, rstd, dgamma, dbeta, rows, C, merge=False, B=0, H=0, W=0):
    rc = _lib.load().tulip_layernorm_bwd_params(_p(dy), _p(x), _p(mean), _p(rstd), _p(dgamma), _p(dbeta), rows, C,
                                                int(merge), B, H, W, _stream())
    check(rc, "tulip_layernorm_bwd_params")


def patch_embed_fwd(img, w, b, gamma, beta, out, B, Cin, Hin, Win, E, p0, p1, kw, circular, eps, out_bf16=None,
                    ld_bf16=0, draw=None):
    """draw = (keep, scale, u_out, nslots, B, seed, counter): the step's DropPath draws (drop_path_scales) ride in this launch."""
    if draw is None:
        rc = _lib.load().tulip_patch_embed_fwd(_p(img), _p(w), _p(b), _p(gamma), _p(beta), _p(out), B, Cin, Hin, Win, E,
                                               p0, p1, kw, int(circular), eps, _p(out_bf16), ld_bf16, _stream())
        check(rc, "tulip_patch_embed_fwd")
        return
    keep, scale, u_out, nslots, Bd, seed, counter = draw
    dd = _lib.DropDraw(_p(keep), _p(scale), _p(u_out), nslots, Bd, int(seed) & (2 ** 64 - 1), _p(counter))
    rc = _lib.load().tulip_patch_embed_fwd_draw(_p(img), _p(w), _p(b), _p(gamma), _p(beta), _p(out), B, Cin, Hin, Win, E,
                                                p0, p1, kw, int(circular), eps, _p(out_bf16), ld_bf16, ctypes.byref(dd),
                                                _stream())
    check(rc, "tulip_patch_embed_fwd_draw")


def patch_embed_bwd(img, w, b, gamma, dout, dw, db, dgamma, dbeta, B, Cin, Hin, Win, E, p0, p1, kw, circular, eps,
                    partial_stride=0):
    rc = _lib.load().tulip_patch_embed_bwd(_p(img), _p(w), _p(b), _p(gamma), _p(dout), _p(dw), _p(db), _p(dgamma),
                                           _p(dbeta), B, Cin, Hin, Win, E, p0, p1, kw, int(circular), eps,
                                           partial_stride, _stream())
    check(rc, "tulip_patch_embed_bwd")


def patch_embed_bwd_blocks(ntok):
    return _lib.load().tulip_patch_embed_bwd_blocks(ntok)


def window_attn_bwd_partial_rows(B, H, W, nh, win):
    return _lib.load().tulip_window_attn_bwd_partial_rows(B, H, W, nh, win[0], win[1])


def window_attn_fwd(qkv, bias_table, rel_index, out, B, H, W, C, nh, win, shift, masked):
    rc = _lib.load().tulip_window_attn_fwd(_p(qkv), _p(bias_table), _p(rel_index), _p(out), B, H, W, C, nh, win[0],
                                           win[1], shift[0], shift[1], int(masked), _stream())
    check(rc, "tulip_window_attn_fwd")


def window_attn_bwd(qkv, dout, bias_table, rel_index, dqkv, dbias_dense, B, H, W, C, nh, win, shift, masked):
    rc = _lib.load().tulip_window_attn_bwd(_p(qkv), _p(dout), _p(bias_table), _p(rel_index), _p(dqkv),
                                           _p(dbias_dense), B, H, W, C, nh, win[0], win[1], shift[0], shift[1],
                                           int(masked), _stream())
    check(rc, "tulip_window_attn_bwd")


def cast_f32_bf16(x, y, rows, cols, rowscale=None, rows_per_sample=1):
    check(_lib.load().tulip_cast_f32_bf16(_p(x), _p(y), rows, cols, _p(rowscale), rows_per_sample, _stream()),
          "tulip_cast_f32_bf16")


def reduce_splits(slabs, out, n, splits):
    check(_lib.load().tulip_reduce_splits(_p(slabs), _p(out), n, splits, _stream()), "tulip_reduce_splits")


def gemm_packed_supported(M, N, K, splits=1) -> bool:
    return bool(_lib.load().tulip_gemm_packed_supported(M, N, K, splits))


def gemm_effective_splits(K, splits):
    return _lib.load().tulip_gemm_effective_splits(K, splits)


def cast_flat(x, y, n):
    check(_lib.load().tulip_cast_flat(_p(x), _p(y), n, _stream()), "tulip_cast_flat")


def cast_bf16_f32(x, y, n):
    check(_lib.load().tulip_cast_bf16_f32(_p(x), _p(y), n, _stream()), "tulip_cast_bf16_f32")


def tail_fwd(xn, We, be, wd, pred, B, H, W, E, in_chans=1, r=4):
    """r: the head's upscale factor (4 or 8; pred is (B, in_chans, r H, r W), We [r*r*E][E]) -- of every tail_* call below"""
    check(_lib.load().tulip_tail_fwd_r(_p(xn), _p(We), _p(be), _p(wd), _p(pred), B, H, W, E, _stream(), int(in_chans), int(r)),
          "tulip_tail_fwd_r")


def tail_bwd(xn, We, be, wd, dpred, dz, dwd, B, H, W, E, target=None, gscale_dev=None, gscale=1.0, in_chans=1, r=4):
    check(_lib.load().tulip_tail_bwd_r(_p(xn), _p(We), _p(be), _p(wd), _p(dpred), _p(dz), _p(dwd), B, H, W, E,
                                       _p(target), _p(gscale_dev), float(gscale), _stream(), int(in_chans), int(r)),
          "tulip_tail_bwd_r")


def tail_fused_bwd_supported(E, r=4):
    return bool(_lib.load().tulip_tail_fused_bwd_supported_r(int(E), int(r)))


def tail_bwd_dgrad(xn, We, be, wd, dpred, dxn, dwd, B, H, W, E, target=None, gscale_dev=None, gscale=1.0, in_chans=1, r=4):
    """Head backward on the chain: dxn (bf16 [M][E]) and the decoder_pred partial rows; d(expand) is never written."""
    check(_lib.load().tulip_tail_bwd_dgrad_r(_p(xn), _p(We), _p(be), _p(wd), _p(dpred), _p(dxn), _p(dwd), B, H, W, E,
                                             _p(target), _p(gscale_dev), float(gscale), _stream(), int(in_chans), int(r)),
          "tulip_tail_bwd_dgrad_r")


def tail_bwd_dgrad_ln(xn, We, be, wd, dpred, dwd, B, H, W, E, x, mean, rstd, gamma, dx, ln_partials, dx_bf16=None,
                      cast_rowscale=None, cast_rows_per_sample=1, target=None, gscale_dev=None, gscale=1.0, in_chans=1, r=4):
    """tail_bwd_dgrad with norm_up's backward in the epilogue: dx / dx_bf16 / [dgamma | dbeta] partial rows (one per 32 tokens)."""
    check(_lib.load().tulip_tail_bwd_dgrad_ln_r(_p(xn), _p(We), _p(be), _p(wd), _p(dpred), _p(dwd), B, H, W, E, _p(target),
                                                _p(gscale_dev), float(gscale), _p(x), _p(mean), _p(rstd), _p(gamma), _p(dx),
                                                _p(dx_bf16), _p(cast_rowscale), cast_rows_per_sample, _p(ln_partials),
                                                _stream(), int(in_chans), int(r)), "tulip_tail_bwd_dgrad_ln_r")


def tail_fwd_ln(x, gamma, beta, eps, xn, mean, rstd, We, be, wd, pred, B, H, W, E, target=None, loss_partials=None,
                log_transform=False, in_chans=1, r=4):
    """norm_up + fused head (+ the L1 / pixel loss partial sums per 32 tokens) in one launch."""
    check(_lib.load().tulip_tail_fwd_ln_r(_p(x), _p(gamma), _p(beta), float(eps), _p(xn), _p(mean), _p(rstd), _p(We), _p(be),
                                          _p(wd), _p(pred), _p(target), _p(loss_partials), int(log_transform), B, H, W, E,
                                          _stream(), int(in_chans), int(r)), "tulip_tail_fwd_ln_r")


def l1_loss_final(partials, losses, nblocks, n, log_transform):
    check(_lib.load().tulip_l1_loss_final(_p(partials), _p(losses), nblocks, n, int(log_transform), _stream()),
          "tulip_l1_loss_final")


def tail_wgrad_splits(B, H, W, E, in_chans=1, r=4):
    return _lib.load().tulip_tail_wgrad_splits_r(B, H, W, E, int(in_chans), int(r))


def tail_wgrad(xn, We, be, wd, dpred, slabs_w, slabs_b, B, H, W, E, target=None, gscale_dev=None, gscale=1.0, in_chans=1, r=4):
    """Expand-conv weight / bias gradient of the head as token-split slabs, d(expand) recomputed channel-sliced."""
    check(_lib.load().tulip_tail_wgrad_r(_p(xn), _p(We), _p(be), _p(wd), _p(dpred), _p(slabs_w), _p(slabs_b), B, H, W, E,
                                         _p(target), _p(gscale_dev), float(gscale), _stream(), int(in_chans), int(r)),
          "tulip_tail_wgrad_r")


def expand_norm_fwd(y, gamma, beta, mean, rstd, B, H, W, P, Cn, eps, out_bf16=None, ld=0, dotw=None, pred=None, in_chans=1):
    """PatchExpanding / FinalPatchExpanding rearrange + LayerNorm (+ decoder_pred dot), see include/tulip_hip.h."""
    check(_lib.load().tulip_expand_norm_fwd_c(_p(y), _p(gamma), _p(beta), _p(out_bf16), ld, _p(dotw), _p(pred), _p(mean),
                                              _p(rstd), B, H, W, P, Cn, eps, _stream(), int(in_chans)), "tulip_expand_norm_fwd_c")


def expand_norm_bwd(y, mean, rstd, gamma, dy_nat, partials, B, H, W, P, Cn, dy_fine=None, ld=0, dpred=None, dotw=None,
                    beta=None, in_chans=1):
    """partials: rows of [dgamma | dbeta | d(dotw) x in_chans] (stride (2 + in_chans) Cn, d(dotw) only with dotw)."""
    check(_lib.load().tulip_expand_norm_bwd_c(_p(dy_fine), ld, _p(dpred), _p(dotw), _p(y), _p(mean), _p(rstd), _p(gamma),
                                              _p(beta), _p(dy_nat), _p(partials), B, H, W, P, Cn, _stream(), int(in_chans)),
          "tulip_expand_norm_bwd_c")


def expand_norm_bwd_partial_rows(B, H, W, P):
    return _lib.load().tulip_expand_norm_bwd_partial_rows(B, H, W, P)


def l1_loss_fwd(pred, target, partials, losses, n, log_transform):
    check(_lib.load().tulip_l1_loss_fwd(_p(pred), _p(target), _p(partials), _p(losses), n, int(log_transform),
                                        _stream()), "tulip_l1_loss_fwd")


def l1_loss_bwd(pred, target, gscale_dev, gscale, dpred, n):
    check(_lib.load().tulip_l1_loss_bwd(_p(pred), _p(target), _p(gscale_dev), float(gscale), _p(dpred), n,
                                        _stream()), "tulip_l1_loss_bwd")


LOSS_KINDS = {"l1": _lib.LOSS_L1, "l2": _lib.LOSS_L2, "berhu": _lib.LOSS_BERHU}      # tulip_amd/loss.py names -> TULIP_LOSS_*


def _loss_kind(kind) -> int:
    return LOSS_KINDS[kind] if isinstance(kind, str) else int(kind)


def loss_blocks(n):
    """workgroups of the tulip_loss_* launches over n elements: the rows of `stats` (4 floats each) and of `value_partials`"""
    return _lib.load().tulip_loss_blocks(n)


def loss_stats(pred, target, stats, n, log_transform):
    """stats (4 * LOSS_BLOCKS_MAX floats): per workgroup [sum |d|, sum |expm1 p - expm1 t|, sum d^2, max |d|]."""
    check(_lib.load().tulip_loss_stats(_p(pred), _p(target), _p(stats), n, int(log_transform), _stream()), "tulip_loss_stats")


def loss_bwd(kind, pred, target, stats, gscale_dev, gscale, dpred, loss_c, n):
    """dpred = gscale * d(loss of `kind`) / d(pred) (tulip_amd/loss.py); berhu reads stats' maxima and writes loss_c[0] = C."""
    check(_lib.load().tulip_loss_bwd(_loss_kind(kind), _p(pred), _p(target), _p(stats), _p(gscale_dev), float(gscale), _p(dpred),
                                     _p(loss_c), n, _stream()), "tulip_loss_bwd")


def loss_value(pred, target, stats, value_partials, n):
    """berhu's second pass: value_partials (LOSS_BLOCKS_MAX floats) = per-workgroup sums of the elementwise values."""
    check(_lib.load().tulip_loss_value(_p(pred), _p(target), _p(stats), _p(value_partials), n, _stream()), "tulip_loss_value")


def loss_final(kind, stats, value_partials, losses, n, log_transform):
    """losses[0] = the loss of `kind`, losses[1] = pixel_loss (the L1 metric), from the partials of loss_stats / loss_value."""
    check(_lib.load().tulip_loss_final(_loss_kind(kind), _p(stats), _p(value_partials), _p(losses), n, int(log_transform),
                                       _stream()), "tulip_loss_final")


def loss_stats_m(pred, target, stats, n, log_transform, chans, chan_stride, valid_min, counts):
    """loss_stats over the valid elements (target[b, 0, pix] > valid_min; tulip_amd/loss.py), and counts (LOSS_BLOCKS_MAX uint32,
    held in an int32 tensor): the valid elements per workgroup."""
    check(_lib.load().tulip_loss_stats_m(_p(pred), _p(target), _p(stats), n, int(log_transform), int(chans), int(chan_stride),
                                         float(valid_min), _p(counts), _stream()), "tulip_loss_stats_m")


def loss_bwd_m(kind, pred, target, stats, gscale_dev, gscale, dpred, loss_c, n, chans, chan_stride, valid_min, counts, n_valid):
    """loss_bwd with n_v = sum(counts) in place of n and +0 at the invalid elements; n_valid (one int64) receives n_v."""
    check(_lib.load().tulip_loss_bwd_m(_loss_kind(kind), _p(pred), _p(target), _p(stats), _p(gscale_dev), float(gscale), _p(dpred),
                                       _p(loss_c), n, int(chans), int(chan_stride), float(valid_min), _p(counts), _p(n_valid),
                                       _stream()), "tulip_loss_bwd_m")


def loss_value_m(pred, target, stats, value_partials, n, chans, chan_stride, valid_min, counts):
    """berhu's second pass over the valid elements."""
    check(_lib.load().tulip_loss_value_m(_p(pred), _p(target), _p(stats), _p(value_partials), n, int(chans), int(chan_stride),
                                         float(valid_min), _p(counts), _stream()), "tulip_loss_value_m")


def loss_edge_blocks(planes, H, W):
    """workgroups of the tulip_loss_edge_* launches over `planes` planes of H x W: the entries of `edge_partials` in use"""
    return _lib.load().tulip_loss_edge_blocks(int(planes), int(H), int(W))


def loss_edge_stats(pred, target, edge_partials, planes, H, W, mask=None, counts=None):
    """edge_partials[wg] = the workgroup's sum of |e_h| + |e_v| of d = pred - target (tulip_amd/loss.py, the edge term); mask:
    (chans, valid_min) -- the responses centred on a valid pixel only (`counts` is not read by this launch)."""
    lib = _lib.load()
    if mask is None:
        check(lib.tulip_loss_edge_stats(_p(pred), _p(target), _p(edge_partials), int(planes), int(H), int(W), _stream()),
              "tulip_loss_edge_stats")
    else:
        check(lib.tulip_loss_edge_stats_m(_p(pred), _p(target), _p(edge_partials), int(planes), int(H), int(W), int(mask[0]),
                                          float(mask[1]), _stream()), "tulip_loss_edge_stats_m")


def loss_edge_bwd(pred, target, gscale_dev, gscale, weight, dpred, planes, H, W, mask=None, counts=None):
    """dpred += weight * gscale * d(edge) / d(pred) in place, behind the base gradient; mask: (chans, valid_min) with `counts` --
    n_v in place of n, +0 at the invalid elements."""
    lib = _lib.load()
    if mask is None:
        check(lib.tulip_loss_edge_bwd(_p(pred), _p(target), _p(gscale_dev), float(gscale), float(weight), _p(dpred), int(planes),
                                      int(H), int(W), _stream()), "tulip_loss_edge_bwd")
    else:
        check(lib.tulip_loss_edge_bwd_m(_p(pred), _p(target), _p(gscale_dev), float(gscale), float(weight), _p(dpred), int(planes),
                                        int(H), int(W), int(mask[0]), float(mask[1]), _p(counts), _stream()), "tulip_loss_edge_bwd_m")


def loss_edge_final(edge_partials, edge_out, losses, weight, planes, H, W, mask=None, counts=None):
    """edge_out[0] = the edge term, losses[0] += weight * edge_out[0], behind the base loss's final launch; mask: 1 / n_v from
    `counts`."""
    lib = _lib.load()
    if mask is None:
        check(lib.tulip_loss_edge_final(_p(edge_partials), _p(edge_out), _p(losses), float(weight), int(planes), int(H), int(W),
                                        _stream()), "tulip_loss_edge_final")
    else:
        check(lib.tulip_loss_edge_final_m(_p(edge_partials), _p(edge_out), _p(losses), float(weight), int(planes), int(H), int(W),
                                          _p(counts), _stream()), "tulip_loss_edge_final_m")


def loss_final_m(kind, stats, value_partials, losses, n, log_transform, counts, n_valid):
    """loss_final with 1 / n_v formed on the device from counts (both losses 0 when n_v == 0); n_valid receives n_v."""
    check(_lib.load().tulip_loss_final_m(_loss_kind(kind), _p(stats), _p(value_partials), _p(losses), n, int(log_transform),
                                         _p(counts), _p(n_valid), _stream()), "tulip_loss_final_m")


def adamw(p, g, m, v, p_bf16, n, hyper, decay_mask64=None, zero_grad=False, lr_scale64=None, skip=None):
    """lr_scale64: per-group learning-rate scales (pack_lr_groups; tulip_adamw_s) -- None: tulip_adamw.
    skip: the non-finite guard's device flag (step_guard; tulip_adamw_g) -- None: the entry points without it."""
    if skip is not None:
        check(_lib.load().tulip_adamw_g(_p(p), _p(g), _p(m), _p(v), _p(p_bf16), n, _p(hyper), _p(decay_mask64),
                                        _p(lr_scale64), int(zero_grad), _p(skip), _stream()), "tulip_adamw_g")
        return
    if lr_scale64 is not None:
        check(_lib.load().tulip_adamw_s(_p(p), _p(g), _p(m), _p(v), _p(p_bf16), n, _p(hyper), _p(decay_mask64),
                                        _p(lr_scale64), int(zero_grad), _stream()), "tulip_adamw_s")
        return
    check(_lib.load().tulip_adamw(_p(p), _p(g), _p(m), _p(v), _p(p_bf16), n, _p(hyper), _p(decay_mask64),
                                  int(zero_grad), _stream()), "tulip_adamw")


def adamw_blocks(p, g, m, v, p_bf16, blocks, nblocks, hyper, decay_mask64=None, zero_grad=False, lr_scale64=None, skip=None):
    """tulip_adamw over the listed 64-float blocks only (blocks: int32 device tensor of block indices); skip: as in adamw."""
    if skip is not None:
        check(_lib.load().tulip_adamw_blocks_g(_p(p), _p(g), _p(m), _p(v), _p(p_bf16), _p(blocks), nblocks, _p(hyper),
                                               _p(decay_mask64), _p(lr_scale64), int(zero_grad), _p(skip), _stream()),
              "tulip_adamw_blocks_g")
        return
    if lr_scale64 is not None:
        check(_lib.load().tulip_adamw_blocks_s(_p(p), _p(g), _p(m), _p(v), _p(p_bf16), _p(blocks), nblocks, _p(hyper),
                                               _p(decay_mask64), _p(lr_scale64), int(zero_grad), _stream()),
              "tulip_adamw_blocks_s")
        return
    check(_lib.load().tulip_adamw_blocks(_p(p), _p(g), _p(m), _p(v), _p(p_bf16), _p(blocks), nblocks, _p(hyper),
                                         _p(decay_mask64), int(zero_grad), _stream()), "tulip_adamw_blocks")


def grad_norm(g, n, partials, out, scale_dev=None, scale=1.0):
    check(_lib.load().tulip_grad_norm(_p(g), n, _p(partials), _p(scale_dev), float(scale), _p(out), _stream()),
          "tulip_grad_norm")


def grad_clip(g, n, partials, grad_scale, max_norm_dev, out):
    """tulip_grad_clip: out[0] = the pre-clip norm sqrt(sum g^2) * grad_scale[0], out[1] = clip_grad_norm_'s coefficient for the
    device float max_norm_dev, grad_scale[0] *= coefficient (tulip_amd/clip.py is the host definition).  g is only read."""
    check(_lib.load().tulip_grad_clip(_p(g), n, _p(partials), _p(grad_scale), _p(max_norm_dev), _p(out), _stream()),
          "tulip_grad_clip")


def range_prep(raw, raw_dtype, batch_stride, row_stride, col_stride, base_offset, hi, lo, B, H, W, row_factor,
               col_factor, row_phase, col_phase, scale, gate, min_range, max_range, log_transform, roll_shift):
    check(_lib.load().tulip_range_prep(_p(raw), raw_dtype, batch_stride, row_stride, col_stride, base_offset, _p(hi),
                                       _p(lo), B, H, W, row_factor, col_factor, row_phase, col_phase, float(scale),
                                       int(gate), float(min_range), float(max_range), int(log_transform),
                                       int(roll_shift), _stream()), "tulip_range_prep")


def range_prep_aug(raw, raw_dtype, batch_stride, row_stride, col_stride, base_offset, hi, lo, B, H, W, row_factor,
                   col_factor, row_phase, col_phase, scale, gate, min_range, max_range, log_transform, sample_ids, seed,
                   flags, beam_threshold, point_threshold, params_out=None):
    """tulip_range_prep_aug: the transforms of range_prep with the per-sample augmentation the kernel draws from (seed,
    sample_ids[b]); sample_ids: B device int64 words, params_out: (B,4) device int32 or None (tulip_amd/augment.py is the host
    definition)."""
    check(_lib.load().tulip_range_prep_aug(_p(raw), raw_dtype, batch_stride, row_stride, col_stride, base_offset, _p(hi),
                                           _p(lo), B, H, W, row_factor, col_factor, row_phase, col_phase, float(scale),
                                           int(gate), float(min_range), float(max_range), int(log_transform),
                                           _p(sample_ids), int(seed) & 0xFFFFFFFFFFFFFFFF, int(flags), int(beam_threshold),
                                           int(point_threshold), _p(params_out), _stream()), "tulip_range_prep_aug")


def _chan_args(C, chan_stride, chan_scale, chan_log):
    """the trailing (C, chan_stride, chan_scale, chan_log) of the multi-channel calls: the C-1 scales as a host float array (the
    entry point copies them into the kernel arguments before it returns), the C-1 log flags as a bit mask"""
    scales = (ctypes.c_float * max(1, C - 1))(*[float(s) for s in chan_scale])
    mask = sum(1 << k for k, on in enumerate(chan_log) if on)
    return int(C), int(chan_stride), scales, mask


def range_prep_c(raw, raw_dtype, batch_stride, row_stride, col_stride, base_offset, hi, lo, B, H, W, row_factor,
                 col_factor, row_phase, col_phase, scale, gate, min_range, max_range, log_transform, roll_shift, C, chan_stride,
                 chan_scale, chan_log):
    """tulip_range_prep_c: range_prep for C-channel pixels into (B,C,..) planes; chan_scale / chan_log: the C-1 scales and log
    flags of channels 1..C-1 (tulip_amd/prep_channels.py is the host definition)."""
    check(_lib.load().tulip_range_prep_c(_p(raw), raw_dtype, batch_stride, row_stride, col_stride, base_offset, _p(hi),
                                         _p(lo), B, H, W, row_factor, col_factor, row_phase, col_phase, float(scale),
                                         int(gate), float(min_range), float(max_range), int(log_transform),
                                         int(roll_shift), _stream(), *_chan_args(C, chan_stride, chan_scale, chan_log)),
          "tulip_range_prep_c")


def range_prep_aug_c(raw, raw_dtype, batch_stride, row_stride, col_stride, base_offset, hi, lo, B, H, W, row_factor,
                     col_factor, row_phase, col_phase, scale, gate, min_range, max_range, log_transform, sample_ids, seed,
                     flags, beam_threshold, point_threshold, params_out, C, chan_stride, chan_scale, chan_log):
    """tulip_range_prep_aug_c: range_prep_aug for C-channel pixels; every channel shares the sample's draws."""
    check(_lib.load().tulip_range_prep_aug_c(_p(raw), raw_dtype, batch_stride, row_stride, col_stride, base_offset, _p(hi),
                                             _p(lo), B, H, W, row_factor, col_factor, row_phase, col_phase, float(scale),
                                             int(gate), float(min_range), float(max_range), int(log_transform),
                                             _p(sample_ids), int(seed) & 0xFFFFFFFFFFFFFFFF, int(flags), int(beam_threshold),
                                             int(point_threshold), _p(params_out), _stream(),
                                             *_chan_args(C, chan_stride, chan_scale, chan_log)), "tulip_range_prep_aug_c")


# ---- evaluation post-processing / metrics (csrc/evalpost.hip)
def mc_aggregate(preds, passes, n, noise_threshold, out):
    check(_lib.load().tulip_mc_aggregate(_p(preds), passes, n, float(noise_threshold), _p(out), _stream()),
          "tulip_mc_aggregate")


def eval_postprocess(pred, hi, lo, pred_img, hi_img, partials, mae_out, H, W, h, w, log_transform, gate_min, gate_max,
                     keep_close):
    check(_lib.load().tulip_eval_postprocess(_p(pred), _p(hi), _p(lo), _p(pred_img), _p(hi_img), _p(partials),
                                             _p(mae_out), H, W, h, w, int(log_transform), float(gate_min),
                                             float(gate_max), float(keep_close), _stream()), "tulip_eval_postprocess")


def mc_aggregate_c(preds, passes, C, n, noise_threshold, out):
    """tulip_mc_aggregate_c: preds (passes, C, n) -> out (C, n); channel 0 decides the drop for all C channels."""
    check(_lib.load().tulip_mc_aggregate_c(_p(preds), passes, int(C), n, float(noise_threshold), _p(out), _stream()),
          "tulip_mc_aggregate_c")


def eval_postprocess_c(pred, hi, lo, pred_img, hi_img, partials, metrics, H, W, h, w, C, log_transform, chan_log, gate_min,
                       gate_max, keep_close):
    """tulip_eval_postprocess_c: eval_postprocess for (C,H,W) images (tulip_amd/eval_channels.py is the host definition).
    chan_log: the C-1 log flags of channels 1..C-1; metrics: 3*C+1 floats; partials: (3*C+1)*1024 doubles."""
    mask = sum(1 << k for k, on in enumerate(chan_log) if on)
    check(_lib.load().tulip_eval_postprocess_c(_p(pred), _p(hi), _p(lo), _p(pred_img), _p(hi_img), _p(partials), _p(metrics),
                                               H, W, h, w, int(C), int(log_transform), mask, float(gate_min), float(gate_max),
                                               float(keep_close), _stream()), "tulip_eval_postprocess_c")


def range_to_xyz(img, sin_h, cos_h, sin_v, cos_v, max_range, H, W, xyz):
    check(_lib.load().tulip_range_to_xyz(_p(img), _p(sin_h), _p(cos_h), _p(sin_v), _p(cos_v), float(max_range), H, W,
                                         _p(xyz), _stream()), "tulip_range_to_xyz")


def range_to_xyz_durlar(img, col_tables, row_tables, row_offset, max_range, origin_offset, z_offset, H, W, xyz):
    check(_lib.load().tulip_range_to_xyz_durlar(_p(img), _p(col_tables), _p(row_tables), _p(row_offset),
                                                float(max_range), float(origin_offset), float(z_offset), H, W,
                                                _p(xyz), _stream()), "tulip_range_to_xyz_durlar")


# ---- dense point clouds (csrc/cloud.hip; tulip_amd/cloud.py is the host definition)
def cloud_tile() -> int:
    """tulip_cloud_tile: destination slots per block; counts / tile_offsets hold B * ceil(H*W / cloud_tile()) entries"""
    return _lib.load().tulip_cloud_tile()


def _cloud_common(pred, lo, B, C, H, W, h, w, log_transform, chan_log, gate_min, gate_max, keep_close, max_range):
    mask = sum(1 << k for k, on in enumerate(chan_log or ()) if on)
    return (_p(pred), _p(lo), int(B), int(C), int(H), int(W), int(h), int(w), int(log_transform), mask, float(gate_min),
            float(gate_max), float(keep_close), float(max_range))


def cloud_spherical(pred, lo, B, C, H, W, h, w, log_transform, chan_log, gate_min, gate_max, keep_close, max_range, sin_h, cos_h,
                    sin_v, cos_v, rng, counts, tile_offsets, offsets, points):
    """tulip_cloud_spherical: pred (B,C,H,W), lo (B,C,h,w) -> rng (B,C,H,W), counts int32 / tile_offsets int64 (B*tiles),
    offsets int64 (B+1), points float32 (B*H*W, 3+C-1).  chan_log: the C-1 log flags of channels 1..C-1."""
    check(_lib.load().tulip_cloud_spherical(*_cloud_common(pred, lo, B, C, H, W, h, w, log_transform, chan_log, gate_min,
                                                            gate_max, keep_close, max_range),
                                            _p(sin_h), _p(cos_h), _p(sin_v), _p(cos_v), _p(rng), _p(counts), _p(tile_offsets),
                                            _p(offsets), _p(points), _stream()), "tulip_cloud_spherical")


def cloud_durlar(pred, lo, B, C, H, W, h, w, log_transform, chan_log, gate_min, gate_max, keep_close, max_range, col_tables,
                 row_tables, row_offset, origin_offset, z_offset, rng, counts, tile_offsets, offsets, points):
    """tulip_cloud_durlar: cloud_spherical with the DurLAR tables; rows and rng are in the staggered destination order."""
    check(_lib.load().tulip_cloud_durlar(*_cloud_common(pred, lo, B, C, H, W, h, w, log_transform, chan_log, gate_min, gate_max,
                                                         keep_close, max_range),
                                         _p(col_tables), _p(row_tables), _p(row_offset), float(origin_offset), float(z_offset),
                                         _p(rng), _p(counts), _p(tile_offsets), _p(offsets), _p(points), _stream()),
          "tulip_cloud_durlar")


def voxel_metrics(pcd_pred, n_pred, pcd_gt, n_gt, is_f64, grid_size, bitmap_pred, bitmap_gt, bitmap_words, scratch,
                  out):
    check(_lib.load().tulip_voxel_metrics(_p(pcd_pred), n_pred, _p(pcd_gt), n_gt, int(is_f64), float(grid_size),
                                          _p(bitmap_pred), _p(bitmap_gt), bitmap_words, _p(scratch), _p(out),
                                          _stream()), "tulip_voxel_metrics")


def chamfer_sq(a, na, b, nb, is_f64, dist_a, dist_b, scratch, out):
    check(_lib.load().tulip_chamfer_sq(_p(a), na, _p(b), nb, int(is_f64), _p(dist_a), _p(dist_b), _p(scratch),
                                       _p(out), _stream()), "tulip_chamfer_sq")


def step_guard(norm, state, skip_flag, hyper, beta1, beta2):
    """tulip_step_guard: the non-finite guard's decision from the float32 device norm (tulip_amd/guard.py is the host definition).
    state: int64[3] device words {applied, skipped_total, skipped_consecutive}; skip_flag: one uint32 device word (1 = skip);
    hyper: the AdamW block, whose bias corrections [5], [6] a taken step rewrites for the applied count."""
    check(_lib.load().tulip_step_guard(_p(norm), _p(state), _p(skip_flag), _p(hyper), float(beta1), float(beta2), _stream()),
          "tulip_step_guard")


def ema_update(p, shadow, n, decay, num_updates, omd_slot, skip=None):
    """tulip_ema_update: shadow -= omd * (shadow - p) over n floats; num_updates: int64 device word (None: no warm-up, no counter),
    omd_slot: one float32 device word the launch pair hands the coefficient through.  skip: the non-finite guard's device flag
    (tulip_ema_update_g: set, neither the counter nor the shadow changes) -- None: tulip_ema_update."""
    if skip is not None:
        check(_lib.load().tulip_ema_update_g(_p(p), _p(shadow), int(n), float(decay), _p(num_updates), _p(omd_slot), _p(skip),
                                             _stream()), "tulip_ema_update_g")
        return
    check(_lib.load().tulip_ema_update(_p(p), _p(shadow), int(n), float(decay), _p(num_updates), _p(omd_slot), _stream()),
          "tulip_ema_update")


def drop_path_scales(keep, scale, u_out, nslots, B, seed, counter):
    check(_lib.load().tulip_drop_path_scales(_p(keep), _p(scale), _p(u_out), nslots, B, int(seed) & (2 ** 64 - 1),
                                             _p(counter), _stream()), "tulip_drop_path_scales")


# ---- element dropout (include/tulip_hip.h, "Element dropout"); `key` is the step's counter word (int64 device tensor or address)
def _seed(seed):
    return int(seed) & (2 ** 64 - 1)


def dropout_begin(counter, key, advance):
    check(_lib.load().tulip_dropout_begin(_p(counter), _p(key), int(bool(advance)), _stream()), "tulip_dropout_begin")


def dropout_mask(key, seed, site, p, n, out):
    check(_lib.load().tulip_dropout_mask(_p(key), _seed(seed), int(site), float(p), int(n), _p(out), _stream()),
          "tulip_dropout_mask")


def dropout_scale(x, is_bf16, rows, cols, key, seed, site, p, ld=None):
    check(_lib.load().tulip_dropout_scale(_p(x), int(bool(is_bf16)), rows, cols, cols if ld is None else ld, _p(key),
                                          _seed(seed), int(site), float(p), _stream()), "tulip_dropout_scale")


def dropout_resid_ln(y, aux, rowscale, rows_per_sample, out, out_bf16, ln, eps, rows, C, key, seed, site, p):
    """ln = (gamma, beta, xn, mean, rstd) or None"""
    g, b, xn, mean, rstd = ln if ln is not None else (None,) * 5
    check(_lib.load().tulip_dropout_resid_ln(_p(y), _p(aux), _p(rowscale), rows_per_sample, _p(out), _p(out_bf16), _p(g),
                                             _p(b), _p(xn), _p(mean), _p(rstd), float(eps), rows, C, _p(key), _seed(seed),
                                             int(site), float(p), _stream()), "tulip_dropout_resid_ln")


def dropout_cast(dx, y, rows, cols, rowscale, rows_per_sample, key, seed, site, p):
    check(_lib.load().tulip_dropout_cast(_p(dx), _p(y), rows, cols, _p(rowscale), rows_per_sample, _p(key), _seed(seed),
                                         int(site), float(p), _stream()), "tulip_dropout_cast")


def window_attn_fwd_drop(qkv, bias_table, rel_index, out, B, H, W, C, nh, win, shift, masked, key, seed, site, p):
    rc = _lib.load().tulip_window_attn_fwd_drop(_p(qkv), _p(bias_table), _p(rel_index), _p(out), B, H, W, C, nh, win[0],
                                                win[1], shift[0], shift[1], int(masked), _p(key), _seed(seed), int(site),
                                                float(p), _stream())
    check(rc, "tulip_window_attn_fwd_drop")


def window_attn_bwd_drop(qkv, dout, bias_table, rel_index, dqkv, dbias_dense, B, H, W, C, nh, win, shift, masked, key, seed,
                         site, p):
    rc = _lib.load().tulip_window_attn_bwd_drop(_p(qkv), _p(dout), _p(bias_table), _p(rel_index), _p(dqkv),
                                                _p(dbias_dense), B, H, W, C, nh, win[0], win[1], shift[0], shift[1],
                                                int(masked), _p(key), _seed(seed), int(site), float(p), _stream())
    check(rc, "tulip_window_attn_bwd_drop")


def kitti_range_map(points, n, rows, cols, ang_start_y, ang_res_y, ang_res_x, max_range, min_range, winner, out):
    check(_lib.load().tulip_kitti_range_map(_p(points), n, rows, cols, float(ang_start_y), float(ang_res_y),
                                            float(ang_res_x), float(max_range), float(min_range), _p(winner), _p(out),
                                            _stream()), "tulip_kitti_range_map")


def _fill(cls, kw, numbers, default=None):
    """cls() from keyword arguments named like its fields: tensors or addresses for the pointer fields (missing: NULL), plain values
    for the fields in `numbers`.  default: what a missing number becomes -- None: nothing, the assignment raises (the geometry of a
    Swin block descriptor must be given); 0 for the stage-boundary descriptors.  A keyword that is no field is a TypeError."""
    d, kw = cls(), dict(kw)
    for name, _t in cls._fields_:
        v = kw.pop(name, None)
        setattr(d, name, (default if v is None else v) if name in numbers else _p(v))
    if kw:
        raise TypeError(f"unknown fields {sorted(kw)}")
    return d


_SWIN_NUMBERS = ("B", "H", "W", "shift_h", "shift_w", "masked", "eps")      # of tulip_swin96_desc / tulip_swin96_bwd_desc


def swin96_block_fwd(stamps=None, **kw):
    """tulip_swin96_block_fwd: keyword arguments are the fields of tulip_swin96_desc (tensors or addresses).
    stamps (int64 device tensor): the profiled twin."""
    d = _swin96_desc(kw)
    if stamps is not None:
        check(_lib.load().tulip_swin96_block_fwd_profiled(ctypes.byref(d), _p(stamps), _stream()), "tulip_swin96_block_fwd_profiled")
        return
    check(_lib.load().tulip_swin96_block_fwd(ctypes.byref(d), _stream()), "tulip_swin96_block_fwd")


def _swin96_desc(kw):
    return _fill(_lib.Swin96Desc, kw, _SWIN_NUMBERS)


def swin96_pair_sync_bytes(B, H, W) -> int:
    return int(_lib.load().tulip_swin96_pair_sync_bytes(B, H, W))


def swin96_pair_fwd(first: dict, second: dict, sync):
    """tulip_swin96_pair_fwd: two consecutive C = 96 blocks in one launch; first / second hold the fields of tulip_swin96_desc,
    sync is the zero-initialised uint8 / int32 device tensor of swin96_pair_sync_bytes that these launches own."""
    d0, d1 = _swin96_desc(first), _swin96_desc(second)
    check(_lib.load().tulip_swin96_pair_fwd(ctypes.byref(d0), ctypes.byref(d1), _p(sync), sync.numel() * sync.element_size(),
                                            _stream()), "tulip_swin96_pair_fwd")


def swinw_supported(C, H, W) -> bool:
    return bool(_lib.load().tulip_swinw_supported(C, H, W))


def swinw_block_fwd(C, out_bf16=None, stamps=None, exchange=None, **kw):
    """tulip_swinw_block_fwd (C = 192 / 384): keyword arguments are the fields of tulip_swin96_desc.
    stamps (int64 device tensor): the profiled twin, per-wave shader-clock stamps at the phase boundaries.
    exchange (zeroed uint8 device tensor of swinw_split_bytes): tulip_swinw_block_fwd_split, two workgroups per window."""
    d = _swin96_desc(kw)
    if exchange is not None:
        check(_lib.load().tulip_swinw_block_fwd_split(ctypes.byref(d), C, _p(out_bf16), _p(exchange),
                                                      exchange.numel() * exchange.element_size(), _p(stamps), _stream()),
              "tulip_swinw_block_fwd_split")
        return
    if stamps is not None:
        check(_lib.load().tulip_swinw_block_fwd_profiled(ctypes.byref(d), C, _p(out_bf16), _p(stamps), _stream()),
              "tulip_swinw_block_fwd_profiled")
        return
    check(_lib.load().tulip_swinw_block_fwd(ctypes.byref(d), C, _p(out_bf16), _stream()), "tulip_swinw_block_fwd")


def swinw_split_bytes(C, B, H, W) -> int:
    """tulip_swinw_split_bytes: size of the exchange buffer of the two-workgroups-per-window form, 0 where it does not exist."""
    return _lib.load().tulip_swinw_split_bytes(C, B, H, W)


def stamp_realtime(dst) -> None:
    """tulip_stamp_realtime: dst (int64 device tensor element) = the 100 MHz device clock at this point of the stream."""
    check(_lib.load().tulip_stamp_realtime(_p(dst), _stream()), "tulip_stamp_realtime")


def swinw_bwd_partial_rows(C, B, H, W) -> int:
    return _lib.load().tulip_swinw_bwd_partial_rows(C, B, H, W)


def swinw_block_bwd(C, exchange=None, **kw):
    """tulip_swinw_block_bwd: fields of tulip_swin96_bwd_desc; w_* are the TRANSPOSED bf16 weights.
    exchange: tulip_swinw_block_bwd_split (see swinw_block_fwd)."""
    d = _fill(_lib.Swin96BwdDesc, kw, _SWIN_NUMBERS)
    if exchange is not None:
        check(_lib.load().tulip_swinw_block_bwd_split(ctypes.byref(d), C, _p(exchange), exchange.numel() * exchange.element_size(),
                                                      _stream()), "tulip_swinw_block_bwd_split")
        return
    check(_lib.load().tulip_swinw_block_bwd(ctypes.byref(d), C, _stream()), "tulip_swinw_block_bwd")


def swind_supported(C, H, W, win) -> bool:
    return bool(_lib.load().tulip_swind_supported(C, H, W, int(win[0]), int(win[1])))


def swind_groups(C, B, H, W, win) -> int:
    """tulip_swind_groups: window groups of a deep-stage block launch = partial rows of its backward."""
    return _lib.load().tulip_swind_groups(C, B, H, W, int(win[0]), int(win[1]))


def swind_block_fwd(C, win, out_bf16=None, phases=15, stamps=None, **kw):
    """tulip_swind_block_fwd (C = 768 / 1536): keyword arguments are the fields of tulip_swin96_desc; w_* fragment-major copies."""
    d = _swin96_desc(kw)
    check(_lib.load().tulip_swind_block_fwd(ctypes.byref(d), C, int(win[0]), int(win[1]), _p(out_bf16), phases, _p(stamps),
                                            _stream()), "tulip_swind_block_fwd")


def swind_block_bwd(C, win, d_norm_out, phases=15, stamps=None, **kw):
    """tulip_swind_block_bwd: fields of tulip_swin96_bwd_desc; w_* fragment-major copies of the TRANSPOSED weights; d_norm_out:
    fp32 [M][C] scratch that phases 2 / 8 fill for tulip_layernorm_bwd_splitk."""
    d = _fill(_lib.Swin96BwdDesc, kw, _SWIN_NUMBERS)
    check(_lib.load().tulip_swind_block_bwd(ctypes.byref(d), C, int(win[0]), int(win[1]), _p(d_norm_out), phases, _p(stamps),
                                            _stream()), "tulip_swind_block_bwd")


def pack_items(entries):
    """[(src address, dst address, rows, cols, transpose)] -> ctypes array for pack_bf16_multi (build once, launch often)."""
    return ((_lib.PackItem * max(len(entries), 1))(*[_lib.PackItem(_p(s), _p(d), r, c, int(t)) for s, d, r, c, t in entries]),
            len(entries))


def pack_bf16_multi(items, n):
    """Fragment-major bf16 copies (optionally of the transpose) of a list of matrices, see include/tulip_hip.h."""
    for k in range(0, n, _lib.PACK_MAX):
        cnt = min(_lib.PACK_MAX, n - k)
        check(_lib.load().tulip_pack_bf16_multi(ctypes.byref(items, k * ctypes.sizeof(_lib.PackItem)), cnt, _stream()),
              "tulip_pack_bf16_multi")


def swin96_bwd_partial_rows(B, H, W) -> int:
    return _lib.load().tulip_swin96_bwd_partial_rows(B, H, W)


def swin96_block_bwd(stamps=None, **kw):
    """tulip_swin96_block_bwd: keyword arguments are the fields of tulip_swin96_bwd_desc (tensors or addresses)."""
    d = _fill(_lib.Swin96BwdDesc, kw, _SWIN_NUMBERS)
    if stamps is not None:
        check(_lib.load().tulip_swin96_block_bwd_profiled(ctypes.byref(d), _p(stamps), _stream()), "tulip_swin96_block_bwd_profiled")
        return
    check(_lib.load().tulip_swin96_block_bwd(ctypes.byref(d), _stream()), "tulip_swin96_block_bwd")


# ---- the stage boundaries as one launch each (csrc/glue.hip): keyword arguments are the descriptor's fields
def merge_fwd_supported(Cin, B, H, W) -> bool:
    return bool(_lib.load().tulip_merge_fwd_supported(Cin, B, H, W))


def merge_fwd(**kw):
    """tulip_merge_fwd: PatchMerging.forward (2x2 gather + LayerNorm + reduction GEMM) in one launch."""
    d = _fill(_lib.MergeFwdDesc, kw, ("ld_bf16", "B", "H", "W", "Cin", "eps"), default=0)
    check(_lib.load().tulip_merge_fwd(ctypes.byref(d), _stream()), "tulip_merge_fwd")


def merge_bwd_supported(Cp, B, H, W) -> bool:
    return bool(_lib.load().tulip_merge_bwd_supported(Cp, B, H, W))


def merge_bwd_partial_rows(Cp, B, H, W) -> int:
    return _lib.load().tulip_merge_bwd_partial_rows(Cp, B, H, W)


def merge_bwd(**kw):
    """tulip_merge_bwd: [x_save half of the skip Linear's data gradient +] reduction data gradient + LayerNorm backward."""
    d = _fill(_lib.MergeBwdDesc, kw, ("cast_rows_per_sample", "B", "H", "W", "Cp"), default=0)
    check(_lib.load().tulip_merge_bwd(ctypes.byref(d), _stream()), "tulip_merge_bwd")


def unmerge_skip_supported(C, B, H, W) -> bool:
    return bool(_lib.load().tulip_unmerge_skip_supported(C, B, H, W))


def unmerge_skip_fwd(**kw):
    """tulip_unmerge_skip_fwd: PatchUnmerging.forward -> skip Linear(cat[...]) in one launch."""
    d = _fill(_lib.UnmergeSkipDesc, kw, ("B", "H", "W", "C"), default=0)
    check(_lib.load().tulip_unmerge_skip_fwd(ctypes.byref(d), _stream()), "tulip_unmerge_skip_fwd")


def skip_unmerge_bwd(**kw):
    """tulip_skip_unmerge_bwd: the skip Linear's data gradient (unmerged half) -> PatchUnmerging's data gradient."""
    d = _fill(_lib.SkipUnmergeBwdDesc, kw, ("cast_rows_per_sample", "B", "H", "W", "C"), default=0)
    check(_lib.load().tulip_skip_unmerge_bwd(ctypes.byref(d), _stream()), "tulip_skip_unmerge_bwd")


def _chan_weights(weights):
    """the host array of a _w launch (None: NULL, which the library refuses)"""
    import ctypes
    return None if weights is None else (ctypes.c_float * len(weights))(*[float(w) for w in weights])


def _w_mask(valid_min) -> tuple:
    """(masked, valid_min) of a _w launch: valid_min None is the unmasked case"""
    return (0, 0.0) if valid_min is None else (1, float(valid_min))


def loss_stats_w(pred, target, stats, n, log_transform, chans, chan_stride, weights, valid_min, counts):
    """loss_stats over the COUNTED elements (TULIP(loss_channel_weights=...), tulip_amd/loss.py: w_c > 0 and, valid_min not None,
    a valid pixel): per workgroup [sum w_c |d|, the unweighted metric sum, sum w_c d^2, max |d|], and counts as in loss_stats_m.
    weights: `chans` Python floats, passed by value in the launch arguments."""
    check(_lib.load().tulip_loss_stats_w(_p(pred), _p(target), _p(stats), n, int(log_transform), int(chans), int(chan_stride),
                                         _chan_weights(weights), *_w_mask(valid_min), _p(counts), _stream()), "tulip_loss_stats_w")


def loss_bwd_w(kind, pred, target, stats, gscale_dev, gscale, dpred, loss_c, n, chans, chan_stride, weights, valid_min, counts,
               n_valid):
    """loss_bwd with g_c = w_c * gscale / n_S per channel, n_S = sum(counts), and +0 at the elements that are not counted; n_valid
    (one int64) receives n_S."""
    check(_lib.load().tulip_loss_bwd_w(_loss_kind(kind), _p(pred), _p(target), _p(stats), _p(gscale_dev), float(gscale), _p(dpred),
                                       _p(loss_c), n, int(chans), int(chan_stride), _chan_weights(weights), *_w_mask(valid_min),
                                       _p(counts), _p(n_valid), _stream()), "tulip_loss_bwd_w")


def loss_value_w(pred, target, stats, value_partials, n, chans, chan_stride, weights, valid_min, counts):
    """berhu's second pass over the counted elements, every value times its channel's weight."""
    check(_lib.load().tulip_loss_value_w(_p(pred), _p(target), _p(stats), _p(value_partials), n, int(chans), int(chan_stride),
                                         _chan_weights(weights), *_w_mask(valid_min), _p(counts), _stream()), "tulip_loss_value_w")


def loss_final_w(kind, stats, value_partials, losses, n, counts, n_valid):
    """losses[0] = the weighted loss of `kind`, losses[1] = the unweighted L1 metric over the counted elements (loss_stats_w's second
    sums, whatever log_transform was), both over n_S = sum(counts); n_valid receives n_S."""
    check(_lib.load().tulip_loss_final_w(_loss_kind(kind), _p(stats), _p(value_partials), _p(losses), n, _p(counts), _p(n_valid),
                                         _stream()), "tulip_loss_final_w")


def loss_edge_stats_w(pred, target, edge_partials, planes, H, W, chans, weights, valid_min):
    """loss_edge_stats with every response times its plane's weight (plane p: channel p % chans); a plane of weight 0 is not read."""
    check(_lib.load().tulip_loss_edge_stats_w(_p(pred), _p(target), _p(edge_partials), int(planes), int(H), int(W), int(chans),
                                              _chan_weights(weights), *_w_mask(valid_min), _stream()), "tulip_loss_edge_stats_w")


def loss_edge_bwd_w(pred, target, gscale_dev, gscale, weight, dpred, planes, H, W, chans, weights, valid_min, counts):
    """loss_edge_bwd with ge_c = weight * w_c * gscale / n_S per plane, n_S from `counts` (loss_stats_w's); a plane of weight 0 is
    neither read nor written."""
    check(_lib.load().tulip_loss_edge_bwd_w(_p(pred), _p(target), _p(gscale_dev), float(gscale), float(weight), _p(dpred), int(planes),
                                            int(H), int(W), int(chans), _chan_weights(weights), *_w_mask(valid_min), _p(counts),
                                            _stream()), "tulip_loss_edge_bwd_w")


def loss_edge_final_w(edge_partials, edge_out, losses, weight, planes, H, W, counts):
    """loss_edge_final with 1 / n_S from `counts`."""
    check(_lib.load().tulip_loss_edge_final_w(_p(edge_partials), _p(edge_out), _p(losses), float(weight), int(planes), int(H), int(W),
                                              _p(counts), _stream()), "tulip_loss_edge_final_w")

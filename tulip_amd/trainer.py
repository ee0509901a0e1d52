"""The training step of the reference's hot loop (engine_upsampling.py:66-100, misc.py:294-308,
lr_sched.py:9-21, main_lidar_upsampling.py:282-283) as ONE fixed launch sequence on one MI355X:

    zero grads -> DropPath draws -> forward -> L1 loss -> backward -> [bucketed RCCL all-reduce,
    overlapped] -> fused AdamW (fp32 master + bf16 shadow)

captured once into HIP graphs (torch.cuda.CUDAGraph) and replayed; the host only refreshes the
8-float hyper-parameter block (lr and bias corrections) per step.  With world_size > 1 the sequence
is cut into graph segments at the bucket boundaries and the all-reduces are issued between replays
(collectives are deliberately NOT captured).  bf16 needs no GradScaler (misc.py:288-308 exists for
fp16).  Gradient accumulation (`accum_iter`, engine:90-97) runs the forward/backward sequence with
d(loss/accum_iter) accumulating into the flat gradient buffer; only the last micro-step of a window
all-reduces (the sum of the per-micro-step all-reduces the reference issues) and applies AdamW.
`train_one_epoch` is the reference's loop around it (per-iteration LR, non-finite-loss abort).
`Trainer(ema_decay=...)` keeps an exponential moving average of the weights (tulip_amd.ema.ParamEMA): one more launch pair
behind the last optimizer write of every optimizer step, inside the captured graphs.
`Trainer(clip_grad=...)` clips the gradients by their global norm (misc.py:299-300; tulip_amd/clip.py): the norm and the coefficient in
front of one end-of-step AdamW, inside the captured graphs, the coefficient folded into the gradient scale that launch reads.
`Trainer(skip_nonfinite=True)` drops the optimizer step whose gradient norm is not finite (GradScaler.step(), misc.py:288-308;
tulip_amd/guard.py): one single-workgroup launch behind the norm decides, AdamW and the EMA update behind it read its flag -- no host
synchronisation, no re-capture, no extra collective.
"""
from __future__ import annotations

import gc
import math
import os
import sys
from typing import Iterable, Optional

import torch
import torch.distributed as dist

from . import knobs, ops
from .clip import check_clip_grad
from .ddp import GradBucketer
from .ema import ParamEMA, check_decay
from .guard import check_skip_nonfinite
from .loss import check_channel_weights, check_edge_weight, check_loss, check_valid_min
from .engine import ALIGN


def cosine_lr(epoch_float: float, lr: float, min_lr: float, warmup_epochs: float, epochs: float) -> float:
    """Per-iteration warm-up + half-cosine (lr_sched.py:9-21)."""
    if epoch_float < warmup_epochs:
        return lr * epoch_float / warmup_epochs
    return min_lr + (lr - min_lr) * 0.5 * (1.0 + math.cos(math.pi * (epoch_float - warmup_epochs)
                                                          / (epochs - warmup_epochs)))


def layer_decay_scales(model, layer_decay: float = 0.75, layers_per_group: int = 12) -> dict:
    """{parameter name: lr_scale} of layer-wise learning-rate decay, for `Trainer(lr_scales=...)`: the reference builds its
    optimizer from timm's `optim_factory.param_groups_layer_decay(model, weight_decay)` (main_lidar_upsampling.py:282, timm's
    default layer_decay = 0.75) and its schedule sets `lr * lr_scale` per group at every iteration (util/lr_sched.py:16-20).
    The rule, for a model without a `group_matcher` and without a `pretrained_cfg` classifier (TULIP has neither):
      1. the names of the parameters with requires_grad, in named_parameters() order;
      2. consecutive chunks of `layers_per_group` names are the groups (the last may be shorter), G groups in all;
      3. group i gets layer_decay ** (G - 1 - i).
    tulip_base: 212 names, 18 groups, 0.75**17 = 0.0075 for the first 12 tensors up to 1.0 for the last 8.
    CAVEAT: timm is neither installed beside this package nor part of the reference tree; the rule is restated from timm's
    source from memory and is not pinned by any test against timm itself.  The function is pure in its three arguments: with
    another timm version, pass that version's own groups (`Trainer(lr_scales=param_groups)`) instead."""
    if layers_per_group < 1:
        raise ValueError("layers_per_group must be >= 1")
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    G = (len(names) + layers_per_group - 1) // layers_per_group
    return {n: float(layer_decay) ** (G - 1 - i // layers_per_group) for i, n in enumerate(names)}


class Trainer:
    def __init__(self, model, batch_size: int, lr: float = 5e-4, betas=(0.9, 0.95), eps: float = 1e-8,
                 weight_decay: float = 0.01, device=None, use_graph: bool = True, process_group=None,
                 bucket_mb: float = 16.0, accum_iter: int = 1, track_grad_norm: bool = False,
                 force_segments: bool = False, bucket_adamw: Optional[bool] = None, grad_dtype: str = "fp32",
                 attn_fp8: Optional[bool] = None, exchange: str = "allreduce", lr_scales=None,
                 ema_decay: Optional[float] = None, ema_use_num_updates: bool = True, clip_grad: Optional[float] = None,
                 skip_nonfinite: bool = False):
        """force_segments: run the N>1 step structure (graph segments cut at the bucket points, one all-reduce per
        bucket between replays) in a one-rank process group too -- how the RCCL path is exercised on a single GPU.
        bucket_adamw: None = environment default (TULIP_BUCKET_ADAMW, off).
        grad_dtype: "fp32" (DistributedDataParallel's exchange, main_lidar_upsampling.py:277) or "bf16": every bucket is
        cast to bf16 before its all-reduce (half the bytes on the xGMI links) and back into the fp32 gradient buffer in
        front of AdamW, whose moments and master weights stay fp32.
        exchange: "allreduce" (default) or "sharded" (tulip_amd.ddp.ShardedExchange, round 5; optional, never measured on more
        than one GPU): per bucket reduce-scatter -> AdamW on the owned shard and on the parameters the kernels read in fp32 ->
        all-gather of the bf16 shadow, on the optimizer stream beside the rest of the backward.  The fp32 master and the moments
        are then current only where this rank steps them: gather_state() (called by state_dict()) makes them whole.
        lr_scales: per-parameter learning-rate scales (layer-wise lr decay; `layer_decay_scales(model)` is the reference's
        recipe): {parameter name: float} -- names left out get 1.0, unknown names raise KeyError -- or a list of torch-style
        param groups carrying `lr_scale`.  Every AdamW site steps a tensor at fl32(lr * scale); at most 64 distinct scales
        (ValueError beyond); exchange="sharded" with scales other than 1.0 raises ValueError (that plan is optional and
        unmeasured).  `step(lr=...)` keeps setting the unscaled rate.
        ema_decay: None (default): no average -- no buffer, no launch, the captured graphs and state_dict() are the ones without
        it.  A float in [0, 1] (ValueError otherwise): `self.ema` is a tulip_amd.ema.ParamEMA over this model (ema_use_num_updates:
        its warm-up, torch_ema's default) and its update runs once per OPTIMIZER step behind every optimizer write of that step,
        inside the captured graphs.  One deviation from the reference's hook (engine_upsampling.py:94-95), which fires at every
        iteration -- also at the accumulation micro-steps, where the parameters did not change: at accum_iter == 1 the two are
        identical; for the per-iteration form leave ema_decay None and call a ParamEMA's update() yourself (train_one_epoch(ema=...)
        does).  world > 1 needs no communication: every rank holds the same parameters and therefore the same average.
        exchange="sharded" with ema_decay raises ValueError (the master is partial there; that plan is optional and unmeasured).
        clip_grad: None (default): no clipping -- no buffer, no launch, the captured graphs and state_dict() are the ones without
        it.  A float >= 0 (ValueError for a negative value or NaN): misc.py:299-300, `clip_grad_norm_(parameters, clip_grad)` in
        front of every optimizer step (tulip_amd/clip.py is the definition): the step takes the norm-first plan of track_grad_norm
        -- no AdamW beside the backward, none per bucket, tulip_grad_clip in front of the one end-of-step launch, inside the
        captured graphs -- and the coefficient goes into the gradient scale that launch reads (hyper[7]), not into the gradients.
        `grad_norm` holds the pre-clip norm (what clip_grad_norm_ returns), `clip_coef` the coefficient, both device floats;
        `trainer.clip_grad = x` between steps uploads one float (no re-capture).  exchange="sharded" with clip_grad raises
        ValueError (every rank would need the norm over all shards before its first bucket steps).
        skip_nonfinite: False (default): no guard -- no buffer, no launch, the captured graphs and state_dict() are the ones without
        it.  True (ValueError for a non-bool): GradScaler.step()'s behaviour (misc.py:288-308; tulip_amd/guard.py is the definition):
        the step takes the norm-first plan, computes the norm (also without track_grad_norm / clip_grad), and tulip_step_guard behind
        it decides on the device: a NaN or infinite norm leaves parameters, bf16 copy, moments, EMA shadow and EMA counter as they
        are (the gradients are still cleared where a taken step clears them) and counts the step as skipped; the optimizer's step
        count and the bias corrections follow the APPLIED steps, on the device.  With world > 1 the norm is that of the all-reduced
        gradient: every rank decides alike.  Read-outs: last_step_skipped (device uint32, no sync), skipped_steps, applied_steps,
        consecutive_skips (ints, one host sync each).  exchange="sharded" with skip_nonfinite raises ValueError.
        The training loss is the model's (TULIP(loss="l1" | "l2" | "berhu"), tulip_amd/loss.py): no argument here.  `losses[0]` is
        that loss, `losses[1]` stays the L1 metric.  berHu's threshold C is formed on the device inside the captured graphs, per
        micro-batch under accum_iter > 1 and per rank with world > 1 (as in the reference, where every rank computes its own
        loss); `loss_c` is the device float of the last backward.  exchange="sharded" with a loss other than "l1" raises
        ValueError (that plan is optional and unmeasured).
        The valid-pixel mask is the model's too (TULIP(loss_valid_min=...)): the loss, `losses[1]` and berHu's C are then over the
        pixels whose target range exceeds the threshold, n_v of them counted on the device per micro-batch and per rank;
        `loss_valid` is the device int64 of the last backward.  A NaN in a target pixel that the mask drops costs no step under
        skip_nonfinite.  exchange="sharded" with a mask raises ValueError; state_dict() does not carry the setting.
        The edge term is the model's as well (TULIP(loss_edge_weight=w)): with w > 0 `losses[0]` is the total, the loss above plus
        w times the mean Sobel response of pred - target, formed on the device inside the captured graphs per micro-batch and
        per rank; `edge_loss` is the device float of the last forward's term (AttributeError at w == 0).  exchange="sharded" with
        w > 0 raises ValueError; state_dict() records w as "loss_edge_weight".
        The channel weights are the model's (TULIP(loss_channel_weights=(w_0, ..))): the loss, its gradient and the edge term then
        weigh channel c by w_c over the counted elements (valid pixels of the channels with w_c > 0), n_S of them counted on the
        device per micro-batch and per rank (`loss_valid` is that count); `losses[1]` stays the unweighted L1 metric over them.  A
        NaN in a w_c == 0 channel costs no step under skip_nonfinite.  exchange="sharded" with weights raises ValueError;
        state_dict() records them as "loss_channel_weights", only when they are set."""
        skip_nonfinite = check_skip_nonfinite(skip_nonfinite)
        self.loss = check_loss(getattr(model, "loss", "l1"))
        self.loss_valid_min = check_valid_min(getattr(model, "loss_valid_min", None))
        if self.loss != "l1" and exchange == "sharded":
            raise ValueError("exchange='sharded' with a loss other than 'l1' is not supported: use exchange='allreduce'")
        if self.loss_valid_min is not None and exchange == "sharded":
            raise ValueError("exchange='sharded' with loss_valid_min is not supported: use exchange='allreduce'")
        self.loss_edge_weight = check_edge_weight(getattr(model, "loss_edge_weight", 0.0))
        if self.loss_edge_weight != 0.0 and exchange == "sharded":
            raise ValueError("exchange='sharded' with loss_edge_weight is not supported: use exchange='allreduce'")
        cw = getattr(model, "loss_channel_weights", None)
        self._loss_channel_weights = None if cw is None else check_channel_weights(tuple(cw), model.in_chans)
        if self._loss_channel_weights is not None and exchange == "sharded":
            raise ValueError("exchange='sharded' with loss_channel_weights is not supported: use exchange='allreduce'")
        if skip_nonfinite and exchange == "sharded":
            raise ValueError("exchange='sharded' with skip_nonfinite is not supported (the per-bucket optimizer steps before the "
                             "global norm exists): use exchange='allreduce'")
        if clip_grad is not None:
            clip_grad = check_clip_grad(clip_grad)
            if exchange == "sharded":
                raise ValueError("exchange='sharded' with clip_grad is not supported (the per-bucket optimizer steps before the "
                                 "global norm exists): use exchange='allreduce'")
        if ema_decay is not None:
            ema_decay = check_decay(ema_decay)
            if exchange == "sharded":
                raise ValueError("exchange='sharded' with ema_decay is not supported (the fp32 master is partial between "
                                 "gather_state() calls): use exchange='allreduce'")
        self.model = model
        device = device or torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self.eng = model.engine()
        if attn_fp8 is not None:      # BASELINE configs[4]: attention scores from e4m3 q, k (default: env TULIP_ATTN_FP8, off)
            self.eng.attn_fp8 = bool(attn_fp8)
        self.eng.check_attn_fp8()
        self.eng.bind(device)
        self.P = self.eng.plan(batch_size)
        W = self.eng.params
        self.g = torch.zeros(W.total, dtype=torch.float32, device=device)
        self.m = torch.zeros_like(self.g)
        self.v = torch.zeros_like(self.g)
        self.hyper = torch.zeros(8, dtype=torch.float32, device=device)
        # the host runs several steps ahead of the GPU: each upload of the hyper block reads its own pinned slot, and a
        # slot is rewritten only after the copy that last read it has executed
        self._hyper_slots = [torch.zeros(8, dtype=torch.float32).pin_memory() for _ in range(4)]
        self._hyper_events = [None] * 4
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.t = 0
        self.accum_iter, self.micro = int(accum_iter), 0
        if self.accum_iter < 1:
            raise ValueError("accum_iter must be >= 1")
        # misc.py:303 get_grad_norm_ (the reference computes it at every update and drops the value)
        self.track_grad_norm = track_grad_norm
        self.grad_norm = torch.zeros(1, dtype=torch.float32, device=device)
        self._norm_part = torch.zeros(1024, dtype=torch.float64, device=device)
        # misc.py:299-300 clip_grad_norm_: the norm first, like the read-out; [norm, coef] and the device float max_norm
        self._clip_grad = clip_grad
        self.clip_coef = None
        if clip_grad is not None:
            self._clip_out = torch.zeros(2, dtype=torch.float32, device=device)
            self.grad_norm, self.clip_coef = self._clip_out[0:1], self._clip_out[1:2]
            self._clip_max = torch.full((1,), clip_grad, dtype=torch.float32, device=device)
        # GradScaler.step() (misc.py:288-308): the device words of the non-finite guard -- {applied, skipped_total,
        # skipped_consecutive} and the flag the launches behind the decision read
        self.skip_nonfinite = skip_nonfinite
        self._guard_state = self._skip_flag = None
        if skip_nonfinite:
            self._guard_state = torch.zeros(3, dtype=torch.int64, device=device)
            self._skip_flag = torch.zeros(1, dtype=torch.int32, device=device).view(torch.uint32)
        norm_first = track_grad_norm or clip_grad is not None or skip_nonfinite      # the optimizer waits for the norm over ALL gradients
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        self.bucketer = GradBucketer(W.groups, W.total, bucket_mb, process_group, force=force_segments)
        self.segmented = self.bucketer.active          # the step is cut at the bucket points
        if grad_dtype not in ("fp32", "bf16"):
            raise ValueError("grad_dtype must be 'fp32' or 'bf16'")
        self.grad_dtype = grad_dtype
        self.gb = (torch.zeros(W.total, dtype=torch.bfloat16, device=device)
                   if (grad_dtype == "bf16" and self.segmented) else None)
        self.use_graph = use_graph
        # N > 1: each bucket is updated (fused AdamW on its slice) on a separate stream as soon as ITS all-reduce has
        # finished, beside the rest of the backward, instead of one update after the last bucket; nothing later in
        # the step reads a finished bucket's parameters or gradients.  The grad-norm read-out needs all gradients.
        # Opt-in (TULIP_BUCKET_ADAMW=1): it relies on RCCL's stream-ordered work.wait(); the default is one update
        # after the last bucket, the order the reference's DDP + optimizer.step() has.
        if bucket_adamw is None:
            bucket_adamw = knobs.is_one("TULIP_BUCKET_ADAMW")
        if exchange not in ("allreduce", "sharded"):
            raise ValueError("exchange must be 'allreduce' or 'sharded'")
        self.exchange = exchange if self.segmented else "allreduce"
        if self.exchange == "sharded" and (model.drop_rate > 0.0 or model.attn_drop_rate > 0.0):
            raise ValueError("exchange='sharded' with element dropout (drop_rate / attn_drop_rate > 0) is not supported: "
                             "use exchange='allreduce'")
        if self.exchange == "sharded":
            if norm_first or grad_dtype != "fp32" or self.accum_iter != 1:
                raise ValueError("exchange='sharded': fp32 gradients, no gradient-norm read-out, accum_iter == 1")
            bucket_adamw = True                      # the plan IS a per-bucket optimizer
        self.bucket_adamw = self.segmented and not norm_first and bool(bucket_adamw)
        self._opt_stream = torch.cuda.Stream(device=device) if self.bucket_adamw else None
        self._sharded = None                         # built at the first bucket (FlatParams.fp32_read is complete by then)
        # (FlatParams groups every parameter where it is last READ in the backward -- the skip Linears sit in their
        # encoder stage's group -- so a bucket's weights are dead once the bucket's hook has fired)
        self._segments = None     # {is_update_step: [(CUDAGraph, tag or None)]}
        self._pack_epoch = -1
        self._seg_drop = None        # the element-dropout sites active when the step was captured (TulipEngine.dropout_state)
        # the fragment-major weight copies of the fused wide blocks (one ~25-us launch) are rewritten at the START of the
        # next step, beside the forward's first kernels, instead of on the chain behind AdamW
        self.pack_at_step_start = True
        # round 5 (TULIP_PACK_AT_END=0: off): the copies rewritten at the END of the step, on the chain's own queue while it waits for the
        # side queue's last groups (TulipEngine.run_backward) -- no forks or joins beside the forward, no pack traffic beside its
        # kernels: 1.9107 -> 1.8941 ms at batch 8, 9.054 -> 9.017 at batch 64 (four interleaved same-box runs each,
        # profiles/r5_ab_pack_at_end.txt; identical losses: the same arithmetic).  Needs every packed weight stepped beside the backward
        # (decided in _plan_fused_adamw: one GPU, captured step); otherwise the pieces beside the forward stay
        self._want_pack_at_end = knobs.on("TULIP_PACK_AT_END", True)
        self._pack_at_end = False
        # without gradient accumulation the backward WRITES every gradient (one producer per parameter and step) instead of adding
        # to a buffer AdamW has to clear: TulipEngine.grad_overwrite (TULIP_GRAD_OVERWRITE=0: accumulate + clear, as with accum_iter > 1)
        self.grad_overwrite = (self.accum_iter == 1 and knobs.on("TULIP_GRAD_OVERWRITE", True)
                               and self.eng.overwrite_supported(batch_size))
        if self.exchange == "sharded" and not self.grad_overwrite:
            # the sharded plan clears nothing outside the blocks this rank steps: an accumulating (+=) backward would feed the stale
            # running sums of the other ranks' shards into the next reduce-scatter
            raise ValueError("exchange='sharded' needs the overwriting backward (accum_iter == 1, TULIP_GRAD_OVERWRITE on, grouped "
                             "weight gradients)")
        # ... and where a weight-gradient workgroup holds a tensor's COMPLETE gradient tile (no token split: the deep stages, 90 %
        # of the parameters), the optimizer step is taken right there, in the write-out, beside the backward instead of behind it
        # (TULIP_FUSE_ADAMW=0: one AdamW launch over everything at the end of the step).  Captured steps on one GPU only: a
        # gradient all-reduce, the gradient-norm read-out, clipping and accumulation need the gradients themselves.
        self.fuse_adamw = (self.grad_overwrite and use_graph and not self.segmented and not norm_first
                           and knobs.on("TULIP_FUSE_ADAMW", True))
        self._adam_mask = None
        self._adam_blocks = None
        # per-parameter learning-rate scales: the group of every 64-float block in bits 2-7 of this Trainer's copy of the decay mask,
        # the scales in a 64-float device table (None while every scale is 1.0: the launches then are the ones without a table)
        self.lr_scales = {n: 1.0 for n in W.names}
        self._mask, self._lr_table = W.decay_mask, None
        self._adam_ctx, self._adam_fused = None, frozenset()
        self._adam_names, self._adam_sites = {}, {}
        self.fused_adamw_params = 0
        # parity tests: explicit DropPath uniforms [n_drop_slots][B] (device tensor) instead of the counter-based draws;
        # set before the first step (the choice is baked into the captured graphs)
        self.inject_drop_u: Optional[torch.Tensor] = None
        # (optimizer step, what the host issued last): read by bench.py's watchdog thread to say WHERE a multi-rank
        # step stopped making progress (a hung collective shows as the segment tag it followed)
        self.progress = (0, "init")
        self._side = torch.cuda.Stream(device=device) if use_graph else None
        # N > 1, captured steps: the last side group of every bucket but the final one is a graph of its own on this stream (own
        # split-K workspace), so that a cut of the step graph does not make the chain wait for it (TULIP_DETACH_BUCKETS=0: the
        # group is forked inside the segment and joined at the cut, one block late)
        self.detach_buckets = bool(use_graph and self.segmented and knobs.on("TULIP_DETACH_BUCKETS", True))
        self._det_stream = torch.cuda.Stream(device=device) if self.detach_buckets else None
        self._ws_det = (torch.empty(self.eng.WS_ELEMS + (1 << 20), dtype=torch.float32, device=device)
                        if self.detach_buckets else None)
        self._det_graphs, self._det_events = {}, {}
        # round 6 (TULIP_GRAPH_COLLECTIVES=0: off): the N > 1 step as ONE captured graph -- every bucket's all-reduce is captured as a
        # branch off the side queue behind the bucket's last weight-gradient group (TulipEngine.run_backward(bucket_on_side=True)),
        # AdamW behind the last of them -- instead of graph segments cut at the bucket points with eager collectives in between (each
        # cut costs the chain ~20 us on one GPU: tools/exp_segments.py).  RCCL only (gloo cannot be captured); a capture that raises
        # falls back to the segmented form (self.step_form says which one runs).  Never run on more than one GPU.
        backend = dist.get_backend(process_group) if dist.is_initialized() else ""
        self.graph_collectives = bool(use_graph and self.segmented and self.exchange == "allreduce" and backend == "nccl"
                                      and knobs.on("TULIP_GRAPH_COLLECTIVES", True))
        self.step_form = "unset"
        self.process_group = process_group
        if self.world > 1:
            # DistributedDataParallel's constructor broadcasts rank 0's parameters and buffers (main_lidar_upsampling.py:277
            # after per-rank seeds `args.seed + rank`, :155): without it every rank would start from its own init and
            # apply identical averaged gradients to different weights.
            src = 0 if process_group is None else dist.get_global_rank(process_group, 0)
            dist.broadcast(W.flat, src=src, group=process_group)
            self.eng.wgrad_ctas = self.eng.WGRAD_DDP_CTAS      # leave the CUs RCCL's channels sit on out of a round
        if lr_scales is not None:
            self.set_lr_scales(lr_scales)
        # the weight average starts as a copy of the parameters this Trainer starts from (behind the broadcast above)
        self.ema = ParamEMA(model, ema_decay, ema_use_num_updates, device) if ema_decay is not None else None
        if self.ema is not None:
            self.ema.skip_flag = self._skip_flag        # (None without the guard)
        W.refresh_shadow()

    # ------------------------------------------------------------------ per-parameter learning-rate scales
    def _scales_by_name(self, lr_scales) -> dict:
        W = self.eng.params
        out = {n: 1.0 for n in W.names}
        if isinstance(lr_scales, dict):
            unknown = [n for n in lr_scales if n not in out]
            if unknown:
                raise KeyError(f"lr_scales names {len(unknown)} parameters this model does not have, e.g. {unknown[:3]}")
            out.update({n: float(v) for n, v in lr_scales.items()})
            return out
        by_ptr = self._param_names_by_ptr()
        for grp in lr_scales:                      # torch-style param groups
            for p in grp["params"]:
                n = by_ptr.get(p.data_ptr())
                if n is None:
                    raise KeyError("lr_scales holds a parameter that is not one of this model's (was the model moved?)")
                out[n] = float(grp.get("lr_scale", 1.0))
        return out

    def set_lr_scales(self, lr_scales) -> None:
        """Install per-parameter learning-rate scales (see __init__; None: all 1.0): quantised to float32, numbered, written
        into the mask bytes and the device table once.  A captured step is captured again."""
        W = self.eng.params
        by_name = self._scales_by_name(lr_scales if lr_scales is not None else {})
        blocks = torch.ones(W.total // ALIGN, dtype=torch.float32)
        for n in W.names:
            blocks[W.offset[n] // ALIGN:(W.offset[n] + W.numel[n] + ALIGN - 1) // ALIGN] = by_name[n]
        mask, table = ops.pack_lr_groups(W.decay_mask, blocks)
        trivial = bool((mask >> 2 == 0).all())
        if not trivial and self.exchange == "sharded":
            raise ValueError("exchange='sharded' with learning-rate scales other than 1.0 is not supported: use exchange='allreduce'")
        self.lr_scales = {n: float(torch.tensor(by_name[n], dtype=torch.float32)) for n in W.names}
        self._mask = W.decay_mask if trivial else mask.to(self.device)
        self._lr_table = None if trivial else table.to(self.device)
        # the fused plan's mask and table are launch arguments baked into the captured graphs
        self._adam_mask, self._adam_blocks, self._adam_ctx, self._adam_fused = None, None, None, frozenset()
        self._adam_names, self._adam_sites = {}, {}
        self._segments = None

    # ------------------------------------------------------------------ gradient clipping
    @property
    def clip_grad(self) -> Optional[float]:
        return self._clip_grad

    @clip_grad.setter
    def clip_grad(self, max_norm) -> None:
        """A new max_norm for the next optimizer step: one float uploaded on the current stream, the captured graphs stay (they
        read it from device memory).  Switching clipping on or off changes the step plan: build another Trainer."""
        if (max_norm is None) != (self._clip_grad is None):
            raise ValueError("clip_grad cannot be switched on or off after construction (the step plan differs): "
                             "build the Trainer with the clip_grad it is to run with")
        if max_norm is not None:
            self._clip_grad = check_clip_grad(max_norm)
            self._clip_max.copy_(torch.full((1,), self._clip_grad, dtype=torch.float32))

    # ------------------------------------------------------------------ non-finite guard
    @property
    def loss_c(self) -> torch.Tensor:
        """berHu's threshold C = 0.2 max|pred - target| of the last backward: a device float (no sync); loss="berhu" only."""
        if self.loss != "berhu":
            raise AttributeError("this Trainer's model has no berHu threshold: build the model with loss='berhu'")
        return self.P.loss_c

    @property
    def loss_valid(self) -> torch.Tensor:
        """n_v, the valid elements (in_chans per valid pixel) of the last backward's loss: a device int64 (no sync); models built
        with loss_valid_min only -- or with loss_channel_weights: n_S, the counted elements."""
        if self.loss_valid_min is None and self._loss_channel_weights is None:
            raise AttributeError("this Trainer's model has no valid-pixel mask: build the model with loss_valid_min=...")
        return self.P.loss_valid

    @property
    def loss_channel_weights(self):
        """The model's channel weights (TULIP(loss_channel_weights=...)): None or a tuple of in_chans floats."""
        return self._loss_channel_weights

    @property
    def edge_loss(self) -> torch.Tensor:
        """The edge term mean(|e_h| + |e_v|) of the last forward, before its weight: a device float (no sync); models built with
        loss_edge_weight > 0 only."""
        if self.loss_edge_weight == 0.0:
            raise AttributeError("this Trainer's model has no edge term: build the model with loss_edge_weight > 0")
        return self.P.loss_edge

    def _guard_word(self, k: int) -> int:
        if self._guard_state is None:
            raise AttributeError("this Trainer has no non-finite guard: build it with skip_nonfinite=True")
        return int(self._guard_state[k].item())

    @property
    def last_step_skipped(self) -> torch.Tensor:
        """The flag of the last optimizer step (device uint32[1], 1 = skipped; no host sync)."""
        if self._skip_flag is None:
            raise AttributeError("this Trainer has no non-finite guard: build it with skip_nonfinite=True")
        return self._skip_flag

    @property
    def applied_steps(self) -> int:
        """Optimizer steps actually taken (one host sync): the optimizer's step count."""
        return self._guard_word(0)

    @property
    def skipped_steps(self) -> int:
        """Optimizer steps skipped in all (one host sync)."""
        return self._guard_word(1)

    @property
    def consecutive_skips(self) -> int:
        """The current run of skipped optimizer steps (one host sync); 0 after a taken step."""
        return self._guard_word(2)

    def _set_guard_counters(self, applied: int, skipped: int = 0, consecutive: int = 0) -> None:
        self._guard_state.copy_(torch.tensor([int(applied), int(skipped), int(consecutive)], dtype=torch.int64))
        self.t = int(applied)

    def _set_betas(self, betas) -> None:
        betas = tuple(betas)
        if self.skip_nonfinite and betas != tuple(self.betas):
            self._segments = None          # the guard's betas are launch arguments baked into the captured graphs: re-capture
        self.betas = betas

    # ------------------------------------------------------------------ pieces
    def _set_hyper(self):
        self.t += 1
        b1, b2 = self.betas
        k = self.t % len(self._hyper_slots)
        if self._hyper_events[k] is not None:
            self._hyper_events[k].synchronize()
        h = self._hyper_slots[k]
        h[0] = self.lr
        h[1], h[2], h[3], h[4] = b1, b2, self.eps, self.wd
        h[5], h[6] = 1.0 - b1 ** self.t, 1.0 - b2 ** self.t
        h[7] = 1.0 / self.world
        self.hyper.copy_(h, non_blocking=True)
        if self._hyper_events[k] is None:
            self._hyper_events[k] = torch.cuda.Event()
        self._hyper_events[k].record()

    def _fwd_bwd(self, hook, update: bool = True, apply_adamw: bool = False, bucket_on_side: bool = False):
        eng, P = self.eng, self.P
        # the fused-AdamW plan points at THIS trainer's gradient / moment / mask buffers: a second Trainer on the same model
        # (another batch size, a rebuild) must not leave its own on the engine for this one's launches or captures
        if getattr(self, "_adam_ctx", None) is not None:
            eng.adam_fused, eng.adam_ctx, eng.adam_sites = self._adam_fused, self._adam_ctx, self._adam_sites
        elif eng.adam_probe is None:
            eng.adam_fused, eng.adam_ctx, eng.adam_sites = frozenset(), None, None
        # (the flat gradient buffer is cleared by the fused AdamW right after it consumed it)
        eng.draw_drop_scales(P, self.model.training, self.inject_drop_u)
        eng.run_forward(P, pack_on_side=self.pack_at_step_start, defer_loss_final=True)
        eng.run_backward(P, self.g, gscale=1.0 / self.accum_iter, bucket_hook=hook,
                         join_tags=set(self.bucketer.by_tag) if (self.segmented and update) else None,
                         overwrite=self.grad_overwrite, apply_adamw=apply_adamw, pack_at_end=self._pack_at_end and apply_adamw,
                         bucket_on_side=bucket_on_side)

    def _adamw_range(self, lo: int, hi: int):
        W = self.eng.params
        ops.adamw(W.base32 + 4 * lo, self.g.data_ptr() + 4 * lo, self.m.data_ptr() + 4 * lo,
                  self.v.data_ptr() + 4 * lo, W.base16 + 2 * lo, hi - lo, self.hyper,
                  self._mask.data_ptr() + lo // 64, zero_grad=not self.grad_overwrite, lr_scale64=self._lr_table)

    def _cast_bucket_down(self, tag):
        """grad_dtype bf16: the bucket's gradients -> the bf16 exchange buffer (captured at the end of the bucket's graph
        segment; issued right before the all-reduce in eager mode)."""
        if self.gb is not None and tag in self.bucketer.by_tag:
            a, b = self.bucketer.by_tag[tag]
            ops.cast_flat(self.g.data_ptr() + 4 * a, self.gb.data_ptr() + 2 * a, b - a)

    def _bucket_done(self, tag, cast: bool = False):
        """All-reduce of the bucket that `tag` completes; with bucket_adamw also its optimizer update, ordered behind
        the collective on the optimizer stream (work.wait() is a stream-level dependency for RCCL)."""
        if cast:
            self._cast_bucket_down(tag)
        if self.exchange == "sharded":
            if tag in self.bucketer.by_tag:
                self._sharded_bucket(tag)
            return
        r = self.bucketer.on_group_done(tag, self.g if self.gb is None else self.gb, keep=not self.bucket_adamw)
        if r is None or not self.bucket_adamw:
            return
        work, a, b = r
        ev = torch.cuda.Event()
        ev.record()                      # (the collective implies this order; a dry run and a capture need it said)
        with torch.cuda.stream(self._opt_stream):
            self._opt_stream.wait_event(ev)
            work.wait()
            if self.gb is not None:
                ops.cast_bf16_f32(self.gb.data_ptr() + 2 * a, self.g.data_ptr() + 4 * a, b - a)
            self._adamw_range(a, b)

    def _sharded_bucket(self, tag):
        """exchange="sharded": reduce-scatter -> AdamW on what this rank steps -> all-gather of the bf16 shadow, all on the
        optimizer stream behind the bucket's last producer (the caller's stream position)."""
        W = self.eng.params
        if self._sharded is None:
            from .ddp import ShardedExchange
            rep = sorted((W.offset[n], W.offset[n] + W.numel[n]) for n in W.fp32_read)
            self._sharded = ShardedExchange(self.bucketer.buckets, rep, self.device, self.process_group)
        ev = torch.cuda.Event()
        ev.record()
        with torch.cuda.stream(self._opt_stream):
            self._opt_stream.wait_event(ev)
            dry = self.bucketer.dry              # (bench.py's re-timing with the collectives skipped: the local work stays)
            blocks = self._sharded.plan[tag]["blocks"] if dry else self._sharded.reduce(tag, self.g)
            ops.adamw_blocks(W.flat, self.g, self.m, self.v, W.shadow, blocks, blocks.numel(), self.hyper, W.decay_mask,
                             zero_grad=not self.grad_overwrite)
            if not dry:
                self._sharded.gather_shadow(tag, W.shadow)
        if self.world > 1:
            # the fp32 master (what model.parameters() / state_dict() view) is now current only on the shards this rank owns:
            # nobody may re-derive the bf16 shadow from it until gather_state() has run on every rank
            W.master_partial = True

    def gather_state(self):
        """exchange="sharded": fp32 master and both moments whole on every rank again (checkpoints, state_dict(), evaluation
        through anything that re-derives the shadow from the master).  A COLLECTIVE: every rank of the process group must call it
        (and therefore Trainer.state_dict()) together -- a call guarded by `if rank == 0` deadlocks.  A no-op for the all-reduce plans.
        Until it has run, FlatParams.master_partial makes every path that would rebuild the bf16 shadow from the stale master
        (model(x) through the module, GraphedForward.weights_changed, load_state_dict -> refresh_shadow) raise instead."""
        if self._sharded is not None:
            torch.cuda.current_stream().wait_stream(self._opt_stream)
            self._sharded.gather_state(self.eng.params.flat, self.m, self.v)
            self.eng.params.master_partial = False

    def _finish_buckets(self):
        if self.bucket_adamw:
            torch.cuda.current_stream().wait_stream(self._opt_stream)
            if not self.pack_at_step_start:
                self.eng.params.refresh_transposes()
            self._ema_update()                        # behind the wait: every bucket's optimizer launch is in front of it
        else:
            self.bucketer.wait_all()
            self._adamw()

    def _ema_update(self):
        """The weight average's update (Trainer(ema_decay=...)), at the one point of each step form that is behind EVERY optimizer
        write of the step: the end of _adamw() -- the end-of-step launch in the eager step, in the one-GPU graph (run_backward has
        joined the side queue, whose write-outs and fold launches take the fused steps, before it returns), in the "adamw" graph of
        the segmented form and in the one graph with captured collectives -- and, with bucket_adamw, behind the wait for the
        optimizer stream in _finish_buckets().  On the chain's own queue: never beside a fold launch."""
        if self.ema is not None:
            self.ema.update()

    def _adamw(self):
        W = self.eng.params
        if self.gb is not None:                       # the summed bf16 gradients come back into the fp32 buffer
            ops.cast_bf16_f32(self.gb, self.g, W.total)
        if self._clip_grad is not None:
            # the pre-clip norm of DDP's mean gradient into grad_norm, the coefficient into clip_coef and into hyper[7]: the launch
            # below steps on g * fl32(1/world * coef); the host uploads 1/world again at the next optimizer step (_set_hyper)
            ops.grad_clip(self.g, W.total, self._norm_part, self.hyper[7:8], self._clip_max, self._clip_out)
        elif self.track_grad_norm or self.skip_nonfinite:
            # g holds the SUM over ranks here; hyper[7] = 1/world turns it into DDP's mean
            ops.grad_norm(self.g, W.total, self._norm_part, self.grad_norm, scale_dev=self.hyper[7:8])
        if self.skip_nonfinite:
            # the decision, from the norm just written (with world > 1: of the all-reduced gradient, the same on every rank): the
            # counters, the flag and -- on a taken step -- the bias corrections of the applied count over the host's upload.  The
            # AdamW launch and the average's update behind it read the flag
            ops.step_guard(self.grad_norm, self._guard_state, self._skip_flag, self.hyper, self.betas[0], self.betas[1])
        mask = self._adam_mask if self._adam_mask is not None else self._mask         # (bit 1: stepped beside the backward)
        if self._adam_blocks is not None:
            # most tensors were stepped where their gradient was completed: the few blocks left, by index (nothing scanned)
            ops.adamw_blocks(W.flat, self.g, self.m, self.v, W.shadow, self._adam_blocks, self._adam_blocks.numel(), self.hyper,
                             mask, zero_grad=not self.grad_overwrite, lr_scale64=self._lr_table, skip=self._skip_flag)
        else:
            ops.adamw(W.flat, self.g, self.m, self.v, W.shadow, W.total, self.hyper, mask, zero_grad=not self.grad_overwrite,
                      lr_scale64=self._lr_table, skip=self._skip_flag)
        if self._pack_at_end:
            if W.pk_late:
                W.refresh_transposes(late=True)
        elif not self.pack_at_step_start:
            W.refresh_transposes()
        self._ema_update()

    # ------------------------------------------------------------------ checkpoint (misc.save_model / load_model keep
    # {'model', 'optimizer', 'epoch', ...}: this is the 'optimizer' entry of the fused AdamW)
    def state_dict(self) -> dict:
        W = self.eng.params
        self.gather_state()
        cut = lambda flat, n: flat[W.offset[n]:W.offset[n] + W.numel[n]].view(W.shape[n]).clone()
        applied = self.t
        if self.skip_nonfinite:                    # the optimizer's step count is the APPLIED count, which only the device knows
            applied, skipped, consecutive = (int(x) for x in self._guard_state.tolist())
        sd = {"step": applied, "micro": self.micro, "lr": self.lr, "betas": tuple(self.betas), "eps": self.eps,
              "weight_decay": self.wd, "accum_iter": self.accum_iter, "loss_edge_weight": self.loss_edge_weight, "lr_scales": dict(self.lr_scales),
              "exp_avg": {n: cut(self.m, n) for n in W.names}, "exp_avg_sq": {n: cut(self.v, n) for n in W.names},
              "grad": {n: cut(self.g, n) for n in W.names} if self.micro % self.accum_iter else None,
              "drop_seed": int(self.eng._drop_seed), "drop_counter": int(self.eng._drop_counter.item()),
              # the DropPath stream is seeded per rank (main_lidar_upsampling.py:155: args.seed + rank); a checkpoint is
              # written by rank 0 and read by every rank, which re-derives its own seed from the saver's
              "rank": dist.get_rank(self.process_group) if dist.is_initialized() else 0}
        if self.ema is not None:                   # (no key without the average: the dictionary of a Trainer that keeps none is unchanged)
            sd["ema"] = self.ema.state_dict()
        if self._clip_grad is not None:            # (likewise)
            sd["clip_grad"] = self._clip_grad
        if self.skip_nonfinite:                    # (likewise)
            sd["guard"] = {"applied": applied, "skipped": skipped, "consecutive": consecutive}
        if self._loss_channel_weights is not None:
            sd["loss_channel_weights"] = tuple(self._loss_channel_weights)
        return sd

    def _report_saved_edge_weight(self, sd: dict) -> bool:
        """The edge term is the model's setting, fixed at its construction: a state saved under another weight (a dictionary without
        the key: 0.0) is loaded all the same, and the difference is reported on stderr -- the run continues with another loss than it
        was saved with.  True when they differ."""
        saved = float(sd.get("loss_edge_weight", 0.0))
        if saved == self.loss_edge_weight:
            return False
        sys.stderr.write(f"tulip_amd.Trainer: the optimizer state was saved with loss_edge_weight={saved!r} and this Trainer's model "
                         f"was built with {self.loss_edge_weight!r}: the model's value stays\n")
        return True

    def _report_saved_channel_weights(self, sd: dict) -> bool:
        """The channel weights are the model's setting too, and follow the edge weight's rule: a state saved under other weights (a
        dictionary without the key: None) is loaded all the same and the difference is reported on stderr.  True when they differ."""
        saved = sd.get("loss_channel_weights")
        saved = None if saved is None else tuple(float(w) for w in saved)
        if saved == self._loss_channel_weights:
            return False
        sys.stderr.write(f"tulip_amd.Trainer: the optimizer state was saved with loss_channel_weights={saved!r} and this Trainer's "
                         f"model was built with {self._loss_channel_weights!r}: the model's value stays\n")
        return True

    def load_state_dict(self, sd: dict) -> None:
        W = self.eng.params
        missing = [n for n in W.names if n not in sd["exp_avg"] or n not in sd["exp_avg_sq"]]
        if missing:
            raise KeyError(f"optimizer state lacks {len(missing)} parameters, e.g. {missing[:3]}")
        if self.ema is not None:
            if "ema" not in sd:
                raise KeyError("this Trainer keeps a weight average (ema_decay) and the optimizer state has no 'ema' entry")
            decay = self.ema.decay
            self.ema.load_state_dict(sd["ema"])
            if self.ema.decay != decay:
                self._segments = None          # the decay is a launch argument baked into the captured graphs: re-capture
        elif "ema" in sd:
            sys.stderr.write("tulip_amd.Trainer: the optimizer state holds a weight average ('ema') and this Trainer keeps none "
                             "(ema_decay=None): ignored\n")
        # clipping: the saved max_norm where both clip; a dictionary without the key (or from a run that did not clip) leaves the
        # constructor's value, and a Trainer built without clipping stays without
        if self._clip_grad is not None and sd.get("clip_grad") is not None:
            self.clip_grad = sd["clip_grad"]
        elif self._clip_grad is None and sd.get("clip_grad") is not None:
            sys.stderr.write("tulip_amd.Trainer: the optimizer state was saved with gradient clipping ('clip_grad') and this Trainer "
                             "clips nothing (clip_grad=None): ignored\n")
        self._report_saved_edge_weight(sd)
        self._report_saved_channel_weights(sd)
        put = lambda flat, n, t: flat[W.offset[n]:W.offset[n] + W.numel[n]].copy_(t.reshape(-1).to(flat.dtype))
        for n in W.names:
            put(self.m, n, sd["exp_avg"][n])
            put(self.v, n, sd["exp_avg_sq"][n])
        self.g.zero_()
        if sd.get("grad") is not None:
            for n in W.names:
                put(self.g, n, sd["grad"][n])
        self.t, self.micro, self.lr = int(sd["step"]), int(sd["micro"]), float(sd["lr"])
        self._set_betas(sd["betas"])
        self.eps, self.wd = float(sd["eps"]), float(sd["weight_decay"])
        if self.skip_nonfinite:
            # the device counters; a dictionary without the entry (an unguarded run's): every step so far was applied
            gd = sd.get("guard") or {"applied": int(sd["step"]), "skipped": 0, "consecutive": 0}
            self._set_guard_counters(gd["applied"], gd["skipped"], gd["consecutive"])
        elif sd.get("guard") is not None:
            sys.stderr.write("tulip_amd.Trainer: the optimizer state was saved with the non-finite guard ('guard') and this Trainer "
                             "has none (skip_nonfinite=False): the skip counters are ignored\n")
        saved = sd.get("lr_scales")                # (a dictionary saved before the scales existed: all ones)
        if (saved if saved is not None else {n: 1.0 for n in W.names}) != self.lr_scales:
            self.set_lr_scales(saved)
        # DropPath stream.  Same rank as the one that saved (or a checkpoint without a rank): the saved seed -- the resume then
        # continues the uninterrupted run's draws.  Another rank: the reference seeds rank r with seed + r (main_lidar_upsampling.py:
        # 155); when this engine's own seed sits at exactly that distance from the saved one the convention holds and the own seed
        # IS the shifted one -- otherwise (one manual_seed everywhere, unseeded runs, a sub-group that this process is not a member
        # of: get_rank() == -1) the engine keeps the seed it was built with.
        my_rank = dist.get_rank(self.process_group) if dist.is_initialized() else 0
        saved_rank, own = sd.get("rank"), int(self.eng._drop_seed)
        if saved_rank is None or my_rank == int(saved_rank):
            seed = int(sd["drop_seed"])
        else:
            seed = own
        if seed != own:
            self.eng._drop_seed = seed
            self._segments = None          # the seed is a launch argument baked into the captured graphs: re-capture
        self.eng._drop_counter.fill_(int(sd["drop_counter"]))
        W.master_partial = False       # (the model's load_state_dict wrote the whole master and this call the whole moments)
        W.shadow_dirty = True          # the model's own load_state_dict normally precedes this; refresh either way

    def _plan_fused_adamw(self, eligible):
        """Which tensors take their optimizer step where their gradient is completed, beside the backward, instead of in the
        AdamW launch at the end of the step: `eligible` = {gradient address: elements} of the producers the warm-up pass saw --
        un-split large-tile weight-gradient items (step in the write-out), token-split items and partial-row folds (step in
        the fold launch).  Left out: weights the backward reads again AFTER their gradient is complete (the skip Linears: the
        x_save half of their input gradient is formed when the encoder stage is reached, see FlatParams._completion_order),
        and ranges that do not cover whole tensors."""
        W = self.eng.params
        gbase = self.g.data_ptr()
        by_off = {W.offset[n]: n for n in W.names}
        fused, mask, count = set(), self._mask.clone(), 0
        self._adam_names, self._adam_sites = {}, {}
        cand, rejected_modules = [], set()
        module_of = lambda n: n.rsplit(".", 1)[0]
        for ptr, cnt in eligible.items():
            a = (ptr - gbase) // 4
            names, o = [], a
            while o < a + cnt and o in by_off:             # the tensors the range covers, in flat order
                names.append(by_off[o])
                o = (o + W.numel[by_off[o]] + ALIGN - 1) // ALIGN * ALIGN
            whole = bool(names) and W.offset[names[-1]] + W.numel[names[-1]] <= a + cnt <= o
            if not whole or any(n.startswith("skip_connection_layers.") for n in names):
                rejected_modules.update(module_of(n) for n in names)
                continue
            cand.append((ptr, a, cnt, names))
        for ptr, a, cnt, names in cand:
            # a token-split Linear is stepped by its fold launch only when weight AND bias are fused (TulipEngine._issue_pending):
            # a tensor whose partner of the same module was left out stays with the end-of-step launch too -- masking it here
            # would leave it stepped by nobody
            if any(module_of(n) in rejected_modules for n in names):
                continue
            fused.add(ptr)
            self._adam_names[ptr] = list(names)
            mask[a // 64:(a + cnt + 63) // 64] |= 2
            count += sum(W.numel[n] for n in names)
        if fused:
            self._adam_fused = frozenset(fused)
            self._adam_mask = mask
            self._adam_ctx = ops.adamw_ref(self.hyper, self.g, W.flat, self.m, self.v, W.shadow, decay_mask64=mask,
                                           lr_scale64=self._lr_table)
            self.eng.adam_fused, self.eng.adam_ctx, self.eng.adam_sites = self._adam_fused, self._adam_ctx, self._adam_sites
            self.fused_adamw_params = count
            if self._want_pack_at_end and getattr(W, "pk_offset", None):
                packed = W.packed_names()
                stepped = lambda n: bool((mask[W.offset[n] // 64:(W.offset[n] + W.numel[n] + 63) // 64] & 2).all())
                late = [n for n in packed if not stepped(n)]
                # the copies of weights the END-of-step AdamW launch steps (the skip Linears: read again after their gradient is
                # complete, so never stepped beside the backward) are rewritten by a small launch of their own behind that launch
                if packed and all(n.startswith("skip_connection_layers.") for n in late):
                    self._pack_at_end, self.pack_at_step_start = True, False
                    W.pk_late = frozenset(late)
                    self.eng._pack_mark_tag_ = None
            left = torch.nonzero((mask[:(W.total + 63) // 64] & 2) == 0).flatten().to(torch.int32)
            if 0 < left.numel() * 64 <= W.total // 4:       # (a long list gains nothing over the scan)
                self._adam_blocks = left.contiguous()

    def adamw_sites(self) -> dict:
        """{parameter name: site} of the plan the last optimizer step ran: which of the four places that take the AdamW step
        stepped the tensor -- "writeout" (tulip_wgrad_group_adamw: the weight-gradient write-out), "fold"
        (tulip_reduce_rows_multi_adamw), "blocks" (tulip_adamw_blocks) or "scan" (tulip_adamw).  exchange="sharded" steps
        through tulip_adamw_blocks on every rank's own shard and is not described here."""
        W = self.eng.params
        rest = "blocks" if self._adam_blocks is not None else "scan"
        out = {n: rest for n in W.names}
        for ptr, names in self._adam_names.items():
            if ptr in self._adam_fused and ptr in self._adam_sites:
                out.update({n: self._adam_sites[ptr] for n in names})
        return out

    # ------------------------------------------------------------------ torch.optim.AdamW <-> fused AdamW state
    def _param_names_by_ptr(self):
        W = self.eng.params
        return {W.base32 + 4 * W.offset[n]: n for n in W.names}

    def import_torch_optimizer(self, optimizer: "torch.optim.Optimizer") -> None:
        """Continue a run of the reference's optimizer (main_lidar_upsampling.py:283: torch.optim.AdamW over the module's
        parameters; a reference checkpoint's 'optimizer' entry after `optimizer.load_state_dict`, misc.py:386-390) with the
        fused step: exp_avg / exp_avg_sq / step of every parameter, lr, betas, eps and the weight decay of the decaying
        group.  Parameters are matched by storage (the module's parameters are views of the flat buffer).
        Learning rates: every group's `lr_scale` (timm's param_groups_layer_decay) becomes the scale of its parameters and
        self.lr the unscaled rate, lr / lr_scale of the group with the largest scale; groups without `lr_scale` get their lr
        relative to the largest group lr, which becomes self.lr."""
        W, by_ptr = self.eng.params, self._param_names_by_ptr()
        seen, steps, wds, scales = set(), set(), set(), {}
        groups = optimizer.param_groups
        if any("lr_scale" in grp for grp in groups):
            top = max(groups, key=lambda grp: float(grp.get("lr_scale", 1.0)))
            top_scale = float(top.get("lr_scale", 1.0))
            base_lr = float(top["lr"]) / top_scale if top_scale > 0.0 else float(top["lr"])
            scale_of = lambda grp: float(grp.get("lr_scale", 1.0))
        else:
            base_lr = max(float(grp["lr"]) for grp in groups)
            scale_of = lambda grp: float(grp["lr"]) / base_lr if base_lr > 0.0 else 1.0
        for grp in groups:
            for p in grp["params"]:
                n = by_ptr.get(p.data_ptr())
                if n is None:
                    raise KeyError("optimizer holds a parameter that is not one of this model's (was the model moved?)")
                st = optimizer.state.get(p, {})
                sl = slice(W.offset[n], W.offset[n] + W.numel[n])
                if st:
                    self.m[sl].copy_(st["exp_avg"].reshape(-1).to(self.m.dtype))
                    self.v[sl].copy_(st["exp_avg_sq"].reshape(-1).to(self.v.dtype))
                    steps.add(int(st["step"].item()) if torch.is_tensor(st["step"]) else int(st["step"]))
                else:
                    self.m[sl].zero_(); self.v[sl].zero_(); steps.add(0)
                if p.ndim > 1:
                    wds.add(float(grp["weight_decay"]))
                elif float(grp["weight_decay"]) != 0.0:
                    raise ValueError("the fused AdamW decays ndim > 1 parameters only (timm's grouping, main:282)")
                seen.add(n)
                scales[n] = scale_of(grp)
        if seen != set(W.names) or len(steps) != 1 or len(wds) > 1:
            raise ValueError(f"cannot import: {len(W.names) - len(seen)} parameters missing, steps {sorted(steps)}, decays {sorted(wds)}")
        g0 = optimizer.param_groups[0]
        self.set_lr_scales(scales)
        self.t, self.lr, self.eps = steps.pop(), base_lr, float(g0["eps"])
        self._set_betas(g0["betas"])
        if self.skip_nonfinite:                    # the imported step count is the applied count; the skip counters keep theirs
            self._set_guard_counters(self.t, self.skipped_steps, self.consecutive_skips)
        if wds:
            self.wd = wds.pop()
        self.g.zero_()
        self.micro = 0
        self.eng.params.shadow_dirty = True

    def export_torch_optimizer(self, optimizer: "torch.optim.Optimizer") -> None:
        """The reverse: write the fused optimizer's moments and step count into a torch.optim.AdamW built over the module's
        parameters (so that `optimizer.state_dict()` is what misc.save_model stores, misc.py:339-345).  Every group gets
        lr = lr * lr_scale (what the reference's schedule leaves there, util/lr_sched.py:16-20) and, where the scale is not 1.0
        or the group already has the key, `lr_scale`; a group whose parameters do not share one scale raises ValueError."""
        W, by_ptr = self.eng.params, self._param_names_by_ptr()
        step_count = self.applied_steps if self.skip_nonfinite else self.t
        for grp in optimizer.param_groups:
            sc = {self.lr_scales[by_ptr[p.data_ptr()]] for p in grp["params"]}
            if len(sc) > 1:
                raise ValueError(f"cannot export: a param group mixes the learning-rate scales {sorted(sc)[:4]}; build the "
                                 "optimizer over groups that share one scale (e.g. one group per lr_scale and weight decay)")
            scale = sc.pop() if sc else 1.0
            grp["lr"], grp["betas"], grp["eps"] = self.lr * scale, tuple(self.betas), self.eps
            if scale != 1.0 or "lr_scale" in grp:
                grp["lr_scale"] = scale
            for p in grp["params"]:
                n = by_ptr[p.data_ptr()]
                sl = slice(W.offset[n], W.offset[n] + W.numel[n])
                optimizer.state[p] = {"step": torch.tensor(float(step_count)), "exp_avg": self.m[sl].view(W.shape[n]).clone(),
                                      "exp_avg_sq": self.v[sl].view(W.shape[n]).clone()}

    # ------------------------------------------------------------------ graph capture
    def _abort_capture(self, g, origin):
        """Leave capture mode after an exception inside a capture (the caller captures again in another form).  HIP keeps EVERY
        stream of a capture in capture mode when hipStreamEndCapture finds forked work that was never joined (CUDA ends the
        capture there), so: back on the stream the capture began on -- the engine may have been on its side stream when the
        exception passed through --, join every stream the capture forked into, then end it.  The graph is dropped."""
        torch.cuda.set_stream(origin)
        for st in (getattr(self.eng, "_side_stream", None), self._opt_stream, self._det_stream):
            if st is None or st == origin:
                continue
            with torch.cuda.stream(st):
                forked = torch.cuda.is_current_stream_capturing()
            if forked:
                origin.wait_stream(st)
        try:
            self.bucketer.wait_all()         # (collectives captured before the failure: their stream joins through work.wait())
        except Exception:                    # noqa: BLE001
            self.bucketer.pending.clear()
        try:
            g.capture_end()
        except Exception as e:               # noqa: BLE001
            sys.stderr.write(f"tulip_amd.Trainer: ending the failed capture: {type(e).__name__}: {str(e)[:200]}\n")

    def _capture_one_graph(self):
        """The N > 1 optimizer step as ONE graph: collectives captured as branches off the side queue (graph_collectives)."""
        side = self._side
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            g = torch.cuda.CUDAGraph()
            g.capture_begin(capture_error_mode="thread_local")
            self.eng.detach_buckets = False
            try:
                self._fwd_bwd(lambda tag: self._bucket_done(tag, cast=True), True, bucket_on_side=True)
                self._finish_buckets()       # joins the collectives (and the per-bucket optimizer) / the end-of-step AdamW
            except BaseException:
                self._abort_capture(g, side)
                raise
            g.capture_end()
        torch.cuda.current_stream().wait_stream(side)
        return [(g, None)]

    def _capture(self, update: bool):
        """Capture one step as graph segments cut at the all-reduce points.  update=False is a
        gradient-accumulation micro-step: forward + backward only, no all-reduce, no AdamW.
        Capture mode is thread-local: HIP calls of other threads (the RCCL watchdog polling its events) must not
        invalidate the capture."""
        if update and self.graph_collectives:
            try:
                segs = self._capture_one_graph()
                self.step_form = "one_graph_captured_collectives"
                return segs
            except Exception as e:      # noqa: BLE001  (a backend / runtime that cannot capture the collective: today's segmented form)
                sys.stderr.write(f"tulip_amd.Trainer: capturing the collectives failed ({type(e).__name__}: {e}); "
                                 "falling back to graph segments with eager collectives\n")
                self.graph_collectives = False
                self.bucketer.pending.clear()
                self.P.reset_exchange()
                torch.cuda.synchronize()
        if update:
            self.step_form = "segments" if self.segmented else "one_graph"
        segs = []
        if update:
            self._det_graphs = {}
        side = self._side
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            cur = torch.cuda.CUDAGraph()
            cur.capture_begin(capture_error_mode="thread_local")

            def hook(tag):
                nonlocal cur
                if update and self.segmented and tag in self.bucketer.by_tag:
                    det = self.eng.take_detached()
                    if det is None:
                        self._cast_bucket_down(tag)
                    cur.capture_end()
                    if det is not None:
                        # the bucket's last side group as a graph of its own (TulipEngine.detach_buckets): replayed behind this
                        # segment on the detached stream, the all-reduce behind it; the chain's next segment does not wait for it
                        sg = torch.cuda.CUDAGraph()
                        with torch.cuda.stream(self._det_stream):
                            sg.capture_begin(capture_error_mode="thread_local")
                            self.eng.issue_detached(det, self._ws_det.data_ptr())
                            self._cast_bucket_down(tag)
                            sg.capture_end()
                        self._det_graphs[tag] = sg
                    segs.append((cur, tag))
                    cur = torch.cuda.CUDAGraph()
                    cur.capture_begin(capture_error_mode="thread_local")

            self.eng.detach_buckets = bool(update and self.segmented and self.detach_buckets)
            try:
                self._fwd_bwd(hook, update, apply_adamw=update and self._adam_mask is not None)
            except BaseException:
                self._abort_capture(cur, side)      # (the caller sees the exception; the streams are out of capture mode)
                raise
            finally:
                self.eng.detach_buckets = False
            if not update:
                cur.capture_end()
                segs.append((cur, None))
            elif not self.segmented:
                self._adamw()
                cur.capture_end()
                segs.append((cur, None))
            else:
                # the last bucket closes with the backward's final hook ("embed"): the piece opened after it is
                # empty and is not replayed
                cur.capture_end()
                if not (segs and segs[-1][1] == self.bucketer.buckets[-1][0]):
                    segs.append((cur, None))
                else:
                    self._empty_tail = cur          # keep the (empty) graph object alive
                if not self.bucket_adamw:
                    g2 = torch.cuda.CUDAGraph()
                    g2.capture_begin(capture_error_mode="thread_local")
                    self._adamw()
                    g2.capture_end()
                    segs.append((g2, "adamw"))
        torch.cuda.current_stream().wait_stream(side)
        return segs

    # ------------------------------------------------------------------ public
    def load_batch(self, x: torch.Tensor, target: torch.Tensor):
        self.eng.check_target(self.P.B, target)
        self.P.x_in.copy_(x.reshape(self.P.x_in.shape), non_blocking=True)
        self.P.target.copy_(target.reshape(self.P.target.shape), non_blocking=True)

    def set_dry(self, dry: bool):
        """Measurement switch (tools/exp_segments.py, bench.py's comm report): keep the step structure, skip the collectives.  The
        one-graph form bakes the collectives into its capture, so the step is re-captured."""
        if self.bucketer.dry != bool(dry):
            self.bucketer.dry = bool(dry)
            if self.graph_collectives:
                self._segments = None

    def zero_grad(self):
        """optimizer.zero_grad() at the top of an epoch (engine_upsampling.py:61): drops the gradients of
        an unfinished accumulation window."""
        self.g.zero_()
        self.micro = 0

    def step(self, x: Optional[torch.Tensor] = None, target: Optional[torch.Tensor] = None,
             lr: Optional[float] = None) -> torch.Tensor:
        """One micro-step on the batch (or on the batch already resident in the plan); every
        `accum_iter`-th call is an optimizer step.  `lr` (if given) becomes the learning rate of the
        next optimizer step.  Returns the device tensor [loss, pixel_loss] (no host sync)."""
        if x is not None:
            self.load_batch(x, target)
        if lr is not None:
            self.lr = lr
        self.micro += 1
        update = self.micro % self.accum_iter == 0
        if update:
            self._set_hyper()
        if update and self.pack_at_step_start:
            # after this step the bf16 shadow is new and the wide blocks' copies are not (this Trainer's next step rewrites
            # them first thing; any other forward in between must, too)
            mark_pack_dirty = True
        else:
            mark_pack_dirty = False
        if self.eng.params.shadow_dirty:
            # parameters were written from outside (load_state_dict / misc.load_model after construction, a foreign
            # optimizer): the bf16 GEMM operands are rebuilt here, outside the captured graphs
            self.eng.params.refresh_shadow()
        if not self.use_graph:
            if update:
                self._fwd_bwd(lambda tag: self._bucket_done(tag, cast=True))
                if self.segmented:
                    self._finish_buckets()
                else:
                    self._adamw()
            else:
                self._fwd_bwd(lambda tag: None, update=False)
            self.eng.params.pack_dirty = self.eng.params.pack_dirty or mark_pack_dirty
            return self.P.losses
        if self._segments is not None and self._pack_epoch != self.eng.params.pack_epoch:
            self._segments = None       # another plan activated the weight copies of a width this capture does not rewrite
        if self._segments is not None and self._seg_drop != self.eng.dropout_state():
            self._segments = None       # Dropout modules switched train / eval: another launch sequence
        if self._segments is None:
            # load every kernel once outside capture, without touching parameters, optimizer state, the gradients of an
            # open accumulation window or the DropPath stream (the pass below accumulates into g and draws once)
            keep_g, keep_c = self.g.clone(), self.eng._drop_counter.clone()
            if self.fuse_adamw:
                self.eng.adam_probe = {}
            self._fwd_bwd(lambda tag: None)
            if self.fuse_adamw:
                self._plan_fused_adamw(self.eng.adam_probe)
                self.eng.adam_probe = None
            if self.exchange == "allreduce":     # the collectives once outside capture too (g is restored below, gb is scratch)
                self.bucketer.prime(self.g if self.gb is None else self.gb)
            scratch = torch.zeros(64, dtype=torch.float32, device=self.device)
            ops.adamw(scratch, scratch.clone(), scratch.clone(), scratch.clone(), None, 64, self.hyper, None)
            if self._lr_table is not None:
                ops.adamw(scratch, scratch.clone(), scratch.clone(), scratch.clone(), None, 64, self.hyper,
                          torch.zeros(1, dtype=torch.uint8, device=self.device), lr_scale64=self._lr_table)
            ops.grad_norm(scratch, 64, self._norm_part, self.grad_norm)
            if self._clip_grad is not None:      # ... and the clip's pair, with a scale and an output of its own (hyper stays as uploaded)
                ops.grad_clip(scratch, 64, self._norm_part, torch.ones(1, dtype=torch.float32, device=self.device), self._clip_max,
                              torch.zeros(2, dtype=torch.float32, device=self.device))
            flag = None
            if self.skip_nonfinite:              # the guard's launch and the gated AdamW forms, on counters, a flag and a hyper block of their own
                flag = torch.zeros(1, dtype=torch.int32, device=self.device).view(torch.uint32)
                ops.step_guard(torch.ones(1, dtype=torch.float32, device=self.device),
                               torch.zeros(3, dtype=torch.int64, device=self.device), flag, self.hyper.clone(), *self.betas)
                ops.adamw(scratch, scratch.clone(), scratch.clone(), scratch.clone(), None, 64, self.hyper,
                          None if self._lr_table is None else torch.zeros(1, dtype=torch.uint8, device=self.device),
                          lr_scale64=self._lr_table, skip=flag)
            if self.ema is not None:             # the average's kernels on scratch too: its shadow and counter stay as they are
                ops.ema_update(scratch, scratch.clone(), 64, self.ema.decay,
                               None if self.ema.counter is None else torch.zeros(1, dtype=torch.int64, device=self.device),
                               torch.zeros(1, dtype=torch.float32, device=self.device), skip=flag)
            self.g.copy_(keep_g)
            self.eng._drop_counter.copy_(keep_c)
            del keep_g
            torch.cuda.synchronize()
            self._pack_epoch = self.eng.params.pack_epoch
            self._seg_drop = self.eng.dropout_state()
            # no cyclic garbage collection inside the captures: a dead reference cycle that holds a CUDAGraph of an earlier Trainer
            # (a test's saved exception info, a local class) is collected wherever the collector happens to run, and on ROCm
            # ~CUDAGraph synchronises the device -- not permitted while this thread captures: the process aborts
            gc_on = gc.isenabled()
            gc.disable()
            try:
                self._segments = {True: self._capture(True)}
                if self.accum_iter > 1:
                    self._segments[False] = self._capture(False)
            except BaseException:
                self._segments = None
                self.P.reset_exchange()       # a launch sequence cut short may have left an arrival ticket half-counted
                raise
            finally:
                if gc_on:
                    gc.enable()
        for graph, tag in self._segments[update]:
            self.progress = (self.t, f"segment:{tag}")
            if tag == "adamw":
                self.bucketer.wait_all()
                graph.replay()
            else:
                graph.replay()
                if tag is not None:
                    self.progress = (self.t, f"all_reduce:{tag}")
                    sg = self._det_graphs.get(tag) if update else None
                    if sg is None:
                        self._bucket_done(tag)
                    else:
                        ev = self._det_events.get(tag)
                        if ev is None:
                            ev = self._det_events[tag] = torch.cuda.Event()
                        ev.record()
                        with torch.cuda.stream(self._det_stream):
                            self._det_stream.wait_event(ev)
                            sg.replay()
                            self._bucket_done(tag)
        if update and self.bucket_adamw and not self.graph_collectives:
            self._finish_buckets()
        self.eng.params.pack_dirty = self.eng.params.pack_dirty or mark_pack_dirty
        return self.P.losses


def train_one_epoch(trainer: Trainer, data_loader: Iterable, epoch: int, args, log_every: int = 0, ema=None) -> dict:
    """engine_upsampling.py:46-124 around the fused step: the learning rate is set from
    `data_iter_step / len(data_loader) + epoch` at the first micro-step of every accumulation window
    (engine:68-69), a non-finite loss prints both losses and exits with status 1 (engine:85-88), and
    the returned dict holds the epoch averages of `loss` and the last `lr` (engine:124).
    `args` needs lr, min_lr, warmup_epochs, epochs (lr_sched.py:9-21); batches are
    (low_res, high_res) tensors or the reference's ({'sample': ...}, {'sample': ...}) dicts.
    Like the reference, the loss is read back every iteration (one host sync per step).
    ema: an object of the caller's with torch_ema's `update()` (a tulip_amd.ema.ParamEMA, say): called after EVERY trainer.step()
    call, the reference's placement (engine:94-95).  The average a Trainer keeps itself (Trainer(ema_decay=...)) needs nothing
    here: it is updated inside the step.
    A guarded trainer (Trainer(skip_nonfinite=True)): the skip flag of every optimizer step is read along with the loss (the same
    host sync).  A skipped step prints one line, its loss (and those of its accumulation window) stays out of the epoch average,
    and the loop exits with status 1 only when `getattr(args, "max_skipped_steps", 10)` optimizer steps in a row were skipped.  A
    non-finite loss of a step that was NOT skipped (a NaN target pixel: NaN loss, zero gradient there) still exits, as in the
    reference; inside an accumulation window that verdict waits for the window's optimizer step."""
    trainer.model.train(True)
    trainer.zero_grad()
    n = len(data_loader)
    tot, cnt, lr = 0.0, 0, trainer.lr
    guarded = bool(getattr(trainer, "skip_nonfinite", False))
    max_skips = int(getattr(args, "max_skipped_steps", 10))
    window = []                  # guarded: the (reduced) losses of the open accumulation window and its first non-finite pair
    window_bad = None
    for it, (lo, hi) in enumerate(data_loader):
        if it % trainer.accum_iter == 0:
            lr = cosine_lr(it / n + epoch, args.lr, args.min_lr, args.warmup_epochs, args.epochs)
        if isinstance(lo, dict):
            lo, hi = lo["sample"], hi["sample"]
        losses = trainer.step(lo.to(trainer.device, non_blocking=True), hi.to(trainer.device, non_blocking=True),
                              lr=lr).tolist()
        if ema is not None:
            ema.update()
        if guarded:
            if not math.isfinite(losses[0]) and window_bad is None:
                window_bad = losses
            if trainer.micro % trainer.accum_iter != 0:
                losses = [0.0, 0.0] if not math.isfinite(losses[0]) else losses      # (the window's verdict is pending)
            elif int(trainer.last_step_skipped.item()):
                run = trainer.consecutive_skips
                print(f"Epoch: [{epoch}]  [{it + 1}/{n}]  non-finite gradient norm: optimizer step skipped "
                      f"({run} in a row, {trainer.skipped_steps} in all; loss {(window_bad or losses)[0]})")
                if run >= max_skips:
                    print("{} optimizer steps skipped in a row, stopping training".format(run))
                    sys.exit(1)
                window, window_bad = [], None
                continue
            elif window_bad is not None:
                print("Total Loss is {}, stopping training".format(window_bad[0]))
                print("Pixel Loss is {}, stopping training".format(window_bad[1]))
                sys.exit(1)
        elif not math.isfinite(losses[0]):
            print("Total Loss is {}, stopping training".format(losses[0]))
            print("Pixel Loss is {}, stopping training".format(losses[1]))
            sys.exit(1)
        if trainer.world > 1:
            # misc.all_reduce_mean on the logged values (engine_upsampling.py:107-109): one 2-float collective
            red = torch.tensor(losses, dtype=torch.float32, device=trainer.device)
            dist.all_reduce(red, group=trainer.process_group)
            losses = (red / trainer.world).tolist()
        if guarded:
            # a window's losses enter the average when its optimizer step was taken
            window.append(losses[0])
            if trainer.micro % trainer.accum_iter == 0:
                tot, cnt = tot + sum(window), cnt + len(window)
                window = []
        else:
            tot, cnt = tot + losses[0], cnt + 1
        if log_every and (it + 1) % log_every == 0:
            print(f"Epoch: [{epoch}]  [{it + 1}/{n}]  lr: {lr:.6f}  loss: {losses[0]:.4f}")
    return {"loss": tot / max(cnt, 1), "lr": lr}

/* tulip_hip.h -- C ABI of libtulip_hip.so: the MI355X (gfx950) kernels behind the TULIP Swin hot path.
 *
 * The reference (ethz-asl/TULIP) is pure Python and defines no FFI; the boundary it exposes for
 * this path is the nn.Module in tulip/model/tulip.py.  Each entry point below replaces the ATen
 * op sequence of the cited reference lines (paths relative to the reference repo).  The Python
 * host (tulip_amd/model/tulip.py) binds them with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - plain pointers + sizes; every buffer is owned by the caller and lives in device memory.
 *   - bf16 tensors are uint16_t (raw bits), row-major, innermost dimension contiguous.
 *   - every call is asynchronous on `stream`, allocates nothing, keeps no global state (the library has no mutable
 *     globals, no setters and reads no environment variable: measurement switches are per-call flag bits), performs
 *     no synchronisation, is re-entrant and is legal under HIP-graph capture.
 *   - return value: 0 on success, TULIP_ERR_ARG (-1) for an unsupported argument combination, TULIP_ERR_NOT_BUILT (-3)
 *     for a form that exists only in the development build (below), -(1000 + hipError_t) if the launch failed.
 *     Nothing throws, nothing exits.
 *   - TWO builds of one symbol set: libtulip_hip.so carries what a training / inference step launches; libtulip_hip_dev.so
 *     (-DTULIP_DEV_VARIANTS=1; tulip_dev_variants() == 1) additionally the forms that were built, bit-tested and measured but
 *     are not on the path -- the *_profiled twins (in-kernel clock stamps), the recomputing C = 96 backward (qkv = fc1_pre = NULL
 *     with the other saved tensors given), tulip_swinw_block_bwd_split, and tulip_swinw_block_fwd / _bwd in their training
 *     forms WITHOUT TULIP_BLOCK_FC1_GRAD.  The product library answers those calls with TULIP_ERR_NOT_BUILT.
 *   - "stream" tensors (the residual stream) are fp32 (B,H,W,C); GEMM operands are bf16 with
 *     fp32 accumulation (the autocast contract of engine_upsampling.py:77, bf16 instead of fp16).
 */
#ifndef TULIP_HIP_H_
#define TULIP_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP_PLATFORM_AMD__
typedef struct ihipStream_t* hipStream_t;
#endif

/* GEMM epilogues */
#define TULIP_EPI_BF16 0         /* out_bf16 = acc + bias                                             */
#define TULIP_EPI_GELU_DUAL 1    /* out = bf16(acc+bias) ; out2 = bf16(gelu_erf(out))  (tulip.py:195-196) */
#define TULIP_EPI_GELU_BWD 2     /* out_bf16 = acc * gelu'(aux_bf16)                                    */
#define TULIP_EPI_F32 3          /* out_f32 (+)= acc + bias                                             */
#define TULIP_EPI_RESID_F32 4    /* out_f32 = aux_f32 + rowscale[m/rows_per_sample]*(acc+bias) (tulip.py:343-344,350-351) */
#define TULIP_EPI_PIXSHUF2_F32 5 /* PatchUnmerging scatter: PixelShuffle(2) + BCHW->BHWC (tulip.py:120-122) */
/* (6: retired) */
#define TULIP_EPI_SPLIT_F32 7    /* out_f32[split][M][ldo] = acc : split-K partial slabs (deterministic) */
#define TULIP_EPI_UNSHUF2_BF16 8 /* inverse of 5, bf16: row m = fine token (b,2h+i,2w+j), column c -> out[(b,h,w)][4c+2i+j]
                                    with psH, psW = the COARSE grid, N = fine channels (backward of PixelShuffle(2)) */
/* TULIP_EPI_F32 with out2 != NULL and ldo2 > 0 additionally stores bf16(result * rowscale[m/rows_per_sample]) at
 * out2[m*ldo2 + n] (the operand of the next GEMM on the path, entering a DropPath branch); TULIP_EPI_RESID_F32 stores
 * bf16(result) there (the row scale is already inside the result); TULIP_EPI_PIXSHUF2_F32 stores fp32 to `out`
 * and/or bf16 to `out2` (row pitch ldo2), whichever is non-NULL. */

/* C[M,N] = opA[M,K] . opB[N,K]^T, bf16 in / fp32 accumulate on v_mfma_f32_16x16x32_bf16.
 * a_trans=0: A is [M][lda]; a_trans=1: A is [K][lda] (A^T stored).  Same for B ([N][ldb] / [K][ldb]).
 * Replaces nn.Linear / 1x1 nn.Conv2d forward (tulip.py:298,318,195,198,105,119,716,175) and their
 * autograd dgrad/wgrad.  Requirements: K%8==0, N%8==0, lda%8==0, ldb%8==0 (and M%8 / N%8 for the
 * transposed operands).  splits>1: the K range is cut across workgroups (for launches too small to fill 256
 * CUs).  With TULIP_EPI_SPLIT_F32 the raw partials go to `out`; with any other epilogue
 * the partial slabs go to `workspace` (>= effective_splits*M*N*4 bytes) and a second kernel folds them and
 * applies the epilogue.  workspace may be NULL when splits == 1.
 * Weight-gradient form (a_trans=1, epi SPLIT_F32 or F32): if out2 != NULL it additionally receives
 * the row sums of opA, i.e. sum over tokens of dY = the bias gradient, as fp32 [splits][M] (SPLIT) or
 * [M] (F32, += when accumulate) -- computed by one extra MFMA per fragment against an all-ones operand.  They come out of the
 * GEMM kernel's own k loop: TULIP_EPI_F32 with out2 (ldo2 = 0) and an effective split count above 1 is TULIP_ERR_ARG (take the
 * slabs with TULIP_EPI_SPLIT_F32 and fold them).
 * `accumulate` is a flag word: TULIP_GEMM_ACCUMULATE (bit 0, the 0 / 1 of earlier versions); TULIP_GEMM_NO_TOUCH: skip the
 * split first touch of the cold [96][k range] weight panel that the M-tile workgroups of an N panel perform before their k
 * loops (forward / data-gradient form); TULIP_GEMM_CHECKED: the bounds-checked kernels even where whole tiles allow the
 * unchecked ones.  The last two are measurement / bit-compare switches: results are identical either way. */
#define TULIP_GEMM_ACCUMULATE 1
#define TULIP_GEMM_NO_TOUCH 0x100
#define TULIP_GEMM_CHECKED 0x200
/* TULIP_GEMM_MID: run the 192 x 192 loader-wave kernel (csrc/gemm.hip, gemm_mid_tile) wherever it fits (a_trans = 0, K range per
 * split a multiple of 64, M, N >= 96, not the PixelShuffle epilogues) -- the caller's choice, for narrow outputs over a deep K at
 * M >= 4096 with the K split that fills the chip; bit-identical results (both kernels sum k in the same order per output element).
 * TULIP_GEMM_NO_MID is accepted and means the default (never, unless asked). */
#define TULIP_GEMM_NO_MID 0x400
#define TULIP_GEMM_MID 0x800
/* TULIP_GEMM_B_PACKED: B is the FRAGMENT-MAJOR copy (tulip_pack_bf16_multi) of the [N][K] matrix -- for a data gradient, of the
 * transposed weight -- and the launch is the small-K form (csrc/gemm.hip, gemm_stream_kernel): 32 x 96 output tiles, the whole K
 * range of a split in flight at once.  a_trans = b_trans = 0, ldb ignored; tulip_gemm_packed_supported(M, N, K, splits) says where
 * it exists (M % 32 == 0, N % 96 == 0, K per split in {96, 384, 768, 1536}), TULIP_ERR_ARG elsewhere.  Same epilogues, same bits as the
 * plain call on the row-major matrix. */
#define TULIP_GEMM_B_PACKED 0x1000
int tulip_gemm_bf16(const void* A, int lda, int a_trans, const void* B, int ldb, int b_trans, int M, int N, int K,
                    int epi, const float* bias, void* out, int ldo, void* out2, int ldo2, const void* aux, int ldaux,
                    const float* rowscale, int rows_per_sample, int accumulate, int psH, int psW, int splits,
                    void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* Up to TULIP_REDUCE_REGIONS_MAX row reductions in one launch:  out[i] (+)= sum_{s<rows} partials[s*stride + i],
 * i < n (n, stride multiples of 4).  With scatter_index != NULL the region is the dense [scatter_nh][scatter_len]
 * relative-position-bias gradient and its sums are added to out[scatter_index[ij]*scatter_nh + h] instead
 * (tulip.py:304-308 backwards; deterministic, no atomics, for scatter_len 256 / 1024 / 4096 -- the 16- / 32- / 64-token
 * windows; 1024 / 4096 take one more launch, one workgroup per head; other lengths add atomically).  A scatter region
 * never takes the AdamW step. */
#define TULIP_REDUCE_REGIONS_MAX 48
typedef struct tulip_reduce_region {
    const float* partials; float* out;
    int64_t stride; int64_t n;
    int rows; int overwrite;
    const int32_t* scatter_index; int scatter_nh; int scatter_len;
    int adamw;      /* 1: tulip_reduce_rows_multi_adamw takes the optimizer step of out[0..n) instead of storing the sum */
} tulip_reduce_region;
int tulip_reduce_rows_multi(const tulip_reduce_region* regions, int n, hipStream_t stream);

/* The weight (and bias) gradients of up to TULIP_WGRAD_GROUP_MAX Linear layers in TWO launches (autograd of
 * nn.Linear, tulip.py:298,318,195,198):  dW[Nw][Kw] += dY[Mtok][Nw]^T . X[Mtok][Kw],  db[Nw] += sum_tokens dY.
 * One grouped GEMM launch covers all items (token dimension cut `splits` ways into fp32 slabs in `workspace`, or
 * accumulated in place when splits == 1), one tulip_reduce_rows_multi launch folds the slabs -- and the `extra`
 * regions (LayerNorm / bias-table partial rows of the same block) ride along in that launch.  `fold` is a flag word:
 * without TULIP_WGRAD_FOLD (bit 0, the 0 / 1 of earlier versions) the second launch is skipped and the slabs stay in the
 * workspace; TULIP_WGRAD_SMALL_TILES forces the 64 x 96 tile everywhere (A/B measurements; tulip_wgrad_tiles takes the
 * same word).  A launch is sized by its caller to
 * about one workgroup per CU in total (`splits`), so the slab traffic is per LAUNCH, not per linear: the engine puts a
 * whole stage (two Swin blocks + boundary linears, up to 12 items) into one. */
#define TULIP_WGRAD_GROUP_MAX 16
#define TULIP_WGRAD_FOLD 1
#define TULIP_WGRAD_SMALL_TILES 0x100
typedef struct tulip_wgrad_item {
    const void* dY; const void* X; float* dW; float* db;
    int ldy; int ldx; int Nw; int Kw; int Mtok; int splits;
    int overwrite;      /* 0: dW += ..., db += ... (autograd's accumulation); 1: dW = ..., db = ... (the caller guarantees this is the
                           only contribution of the step: the gradient buffer then needs no clearing) */
    int reserved_;      /* tulip_wgrad_group_adamw: 1 = apply the optimizer step in the write-out (see there); else 0 */
} tulip_wgrad_item;
int tulip_wgrad_group(const tulip_wgrad_item* items, int n, const tulip_reduce_region* extra, int n_extra,
                      void* workspace, int64_t workspace_bytes, int fold, hipStream_t stream);
/* tulip_wgrad_group that also takes the optimizer step of the items marked reserved_ = 1 (and overwrite = 1, large tiles, no
 * token split: the workgroup holds the complete gradient tile) in its write-out -- torch.optim.AdamW.step (main_lidar_upsampling.py:283)
 * on fp32 master weights + bf16 shadow, same arithmetic as tulip_adamw, decoupled decay on -- instead of storing the gradient:
 * param / exp_avg / exp_avg_sq / param_bf16 are flat buffers laid out like `grad` (an element is addressed by its gradient's
 * offset from `grad`), hyper as in tulip_adamw.  The caller's end-of-step tulip_adamw must skip those tensors (mask bit 1).
 * adam == NULL: exactly tulip_wgrad_group. */
typedef struct tulip_adamw_ref {
    const float* hyper; const float* grad; float* param; float* exp_avg; float* exp_avg_sq; uint16_t* param_bf16;
    const uint8_t* decay_mask64;    /* tulip_adamw's mask (bit 0 = weight decay applies to these 64 elements); NULL: everywhere */
} tulip_adamw_ref;
int tulip_wgrad_group_adamw(const tulip_wgrad_item* items, int n, const tulip_reduce_region* extra, int n_extra,
                            void* workspace, int64_t workspace_bytes, int fold, const tulip_adamw_ref* adam, hipStream_t stream);
/* tulip_reduce_rows_multi whose regions marked adamw = 1 (overwrite = 1, no scatter: the sum is the complete gradient of
 * out[0..n), a range of `adam->grad`) take the optimizer step in place of storing the sum -- same arithmetic as tulip_adamw,
 * decay per 64 elements from adam->decay_mask64; the caller's end-of-step tulip_adamw must skip those ranges (mask bit 1).
 * tulip_wgrad_group_adamw marks the fold regions of its token-split items with reserved_ = 1 this way (weight and bias).
 * adam == NULL: exactly tulip_reduce_rows_multi (a marked region is then an argument error). */
int tulip_reduce_rows_multi_adamw(const tulip_reduce_region* regions, int n, const tulip_adamw_ref* adam, hipStream_t stream);
/* Per-group learning-rate scales (layer-wise lr decay: timm's `lr_scale`, applied by the reference's schedule as
 * lr * lr_scale, util/lr_sched.py:16-20).  The `_s` twins of the four entry points that take the AdamW step read the group of
 * every 64-float block from bits 2-7 of its decay_mask64 byte (bit 0: decay, bit 1: stepped elsewhere) and step it with
 * lr_g = fl32(hyper[0] * lr_scale64[group]) in place of hyper[0], in 1 - lr wd and in lr / bias_corr1 alike.  lr_scale64: a
 * device table of 64 floats whose entry 0 is 1.0f (blocks with bits 2-7 clear keep hyper[0]: x * 1.0f is exact).
 * lr_scale64 == NULL: exactly the entry point without the suffix, which never reads bits 2-7.  lr_scale64 without a mask
 * (decay_mask64 / adam->decay_mask64 NULL, or adam NULL) is TULIP_ERR_ARG before any launch.  A weight-gradient write-out steps
 * one tensor per item and takes the group from the mask byte of the tensor's first block, decay_mask64[(dW - adam->grad) / 64].
 * REQUIREMENT with a table: every stepped item's dW starts on a 64-float boundary of adam->grad and no 64-float block holds
 * elements of two groups (the host cannot check the latter: a tensor that starts inside a block is stepped at the rate of the
 * tensor the block begins with).  An item whose dW is not 64-float aligned to adam->grad is TULIP_ERR_ARG before any launch. */
int tulip_wgrad_group_adamw_s(const tulip_wgrad_item* items, int n, const tulip_reduce_region* extra, int n_extra,
                              void* workspace, int64_t workspace_bytes, int fold, const tulip_adamw_ref* adam,
                              const float* lr_scale64, hipStream_t stream);
int tulip_reduce_rows_multi_adamw_s(const tulip_reduce_region* regions, int n, const tulip_adamw_ref* adam,
                                    const float* lr_scale64, hipStream_t stream);
/* The fold regions tulip_wgrad_group(fold = 1) would hand to tulip_reduce_rows_multi for these items and this workspace (host
 * code only): for a caller that launches with fold = 0 and folds later, in one launch with regions that become ready in
 * between (the engine: the patch-embedding partial rows ride in the fold of the backward's last weight-gradient group).
 * Returns the number of regions written to `out` (<= max), or a negative error. */
int tulip_wgrad_group_regions(const tulip_wgrad_item* items, int n, void* workspace, tulip_reduce_region* out, int max);

/* Workgroup tiles per token split the grouped launch uses for a [Nw][Kw] weight gradient (192 x 192 per workgroup where
 * both dimensions are multiples of 192, 384 x 96 / 96 x 384 for the 96-wide stage, else 64 x 96): what a caller sizes
 * `splits` with.  flags: the `fold` word of the launch it is sized for (TULIP_WGRAD_SMALL_TILES matters). */
int tulip_wgrad_tiles(int Nw, int Kw, int flags);
/* Profiling twin (tools/wgrad_phases.py): the grouped launch alone -- no fold, no optimizer step -- writing 4 x uint64 per
 * workgroup of a large-tile launch into `stamps` (shader clock: start, end of the pipeline prologue, end of the k loop, end
 * of the write-out). */
int tulip_wgrad_group_profiled(const tulip_wgrad_item* items, int n, void* workspace, int64_t workspace_bytes, int flags,
                               void* stamps, hipStream_t stream);

/* number of K-splits tulip_gemm_bf16 actually launches for (K, splits): K is cut in multiples of 32 */
int tulip_gemm_effective_splits(int K, int splits);
int tulip_gemm_packed_supported(int M, int N, int K, int splits);
/* Which kernel tulip_gemm_bf16 launches for these arguments (host code only; `accumulate` is the call's flag word, of which
 * TULIP_GEMM_CHECKED, TULIP_GEMM_MID and TULIP_GEMM_B_PACKED matter): the launcher takes its decision from the same function, so
 * the answer cannot drift from the dispatch.  Returns TULIP_ERR_ARG where tulip_gemm_bf16 refuses on shape or flag grounds (K % 8,
 * N % 8, M % 8 with a_trans, a packed B where the small-K form does not exist, a fold of 2^31 or more 8-column chunks) and for an
 * empty shape (nothing is launched); pitches and pointers are not its business.  Otherwise a non-negative bit field:
 *   bits 0-1  family   TULIP_ROUTE_TILE   gemm_kernel: BM x 96 tiles, bounds-checked loads and stores
 *                      TULIP_ROUTE_FULL   gemm_kernel_full: the same tiles unchecked (whole tiles, a_trans = 0)
 *                      TULIP_ROUTE_MID    gemm_mid_kernel: 192 x 192, 64-deep stages (TULIP_GEMM_MID where it fits)
 *                      TULIP_ROUTE_STREAM gemm_stream_kernel: 32 x 96, the packed-B small-K form
 *   bits 2-3  variant  tile families: tile rows 0 = 64, 1 = 128, 2 = 256 (256 only with a_trans = 0); stream: K per split
 *                      0 = 96, 1 = 384, 2 = 768, 3 = 1536; mid: 0
 *   bit  4    TULIP_ROUTE_DEEP     128-deep k stages instead of 32-deep ones (64-row tiles only)
 *   bit  5    TULIP_ROUTE_A_TRANS  bit 6  TULIP_ROUTE_B_TRANS   the operand layouts the kernel is instantiated for
 *   bit  7    TULIP_ROUTE_FOLD     splitk_epilogue_kernel follows (splits > 1 with an epilogue other than TULIP_EPI_SPLIT_F32)
 *   bits 8-30 the K splits launched (= tulip_gemm_effective_splits(K, splits)) */
#define TULIP_ROUTE_TILE 0
#define TULIP_ROUTE_FULL 1
#define TULIP_ROUTE_MID 2
#define TULIP_ROUTE_STREAM 3
#define TULIP_ROUTE_FAMILY(r) ((r) & 3)
#define TULIP_ROUTE_VARIANT(r) (((r) >> 2) & 3)
#define TULIP_ROUTE_DEEP 0x10
#define TULIP_ROUTE_A_TRANS 0x20
#define TULIP_ROUTE_B_TRANS 0x40
#define TULIP_ROUTE_FOLD 0x80
#define TULIP_ROUTE_SPLITS_SHIFT 8
#define TULIP_ROUTE_SPLITS(r) ((r) >> TULIP_ROUTE_SPLITS_SHIFT)
int tulip_gemm_route(int M, int N, int K, int a_trans, int b_trans, int epi, int accumulate, int splits);

/* REDUCTIONS.  No kernel in this library funnels many workgroups into same-address atomics (on gfx950 a
 * chain of same-address device-scope fp32 atomics costs ~0.1-0.5 us per link).  Every cross-workgroup sum
 * (split-K weight gradients, bias / LayerNorm / relative-position-bias / patch-embed / decoder_pred
 * gradients) is written as per-workgroup PARTIAL ROWS with plain stores and folded, deterministically, by:
 *   out_r[i] += sum_{s<nrows} part_r[s*stride_r + i],  i < n_r,   for two regions r = 0,1 in one launch.
 * n, stride multiples of 4; a region with n<=0 is skipped. */
int tulip_reduce_rows2(const float* part0, int64_t stride0, float* out0, int64_t n0, const float* part1,
                       int64_t stride1, float* out1, int64_t n1, int nrows, hipStream_t stream);
/* out[i] += sum_s slabs[s*n + i]  (= tulip_reduce_rows2 with one region of stride n) */
int tulip_reduce_splits(const float* slabs, float* out, int64_t n, int splits, hipStream_t stream);

/* LayerNorm over the last dim of an fp32 stream tensor -> bf16 (the next op is always a GEMM).
 * merge=0: x is [rows][C].  merge=1 (PatchMerging, tulip.py:92-105): x is (B,H,W,C/4) and row
 * (b,h',w') is the concat [x(2h',2w'), x(2h'+1,2w'), x(2h',2w'+1), x(2h'+1,2w'+1)]; rows=B*H/2*W/2.
 * Saves mean/rstd per row for the backward.  Replaces tulip.py:340,347,104,720. */
int tulip_layernorm_fwd(const float* x, const float* gamma, const float* beta, uint16_t* y, float* mean, float* rstd,
                        int rows, int C, float eps, int merge, int B, int H, int W, hipStream_t stream);

/* dx = dres + LayerNorm-backward(dy) in the layout of x (scatter for merge=1).  dres may be NULL
 * (treated as zero) or alias dx.  param_partials (may be NULL): receives
 * tulip_layernorm_bwd_partial_rows(rows, C) partial rows of [dgamma[C] | dbeta[C]] (stride 2C), to be
 * folded with tulip_reduce_rows2 -- the parameter gradients cost no second pass over dy and x.
 * dx_bf16 (may be NULL): additionally receives bf16(dx * cast_rowscale[token / cast_rows_per_sample]) in the
 * layout of dx -- the operand of the next dgrad/wgrad GEMM on the backward chain (DropPath scale of the branch
 * it enters, tulip.py:25-29), so no separate cast pass is needed. */
int tulip_layernorm_bwd(const uint16_t* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                        const float* dres, float* dx, int rows, int C, int merge, int B, int H, int W,
                        float* param_partials, uint16_t* dx_bf16, const float* cast_rowscale,
                        int cast_rows_per_sample, hipStream_t stream);
/* tulip_layernorm_bwd whose incoming gradient is still the `nslab` raw split-K slabs [nslab][rows][C] of the data-gradient
 * GEMM in front (tulip_gemm_bf16 with TULIP_EPI_SPLIT_F32): folded in slab order and rounded to bf16 exactly as that
 * GEMM's own fold launch would have stored them -- one launch less on the backward chain. */
int tulip_layernorm_bwd_splitk(const float* slabs, int nslab, const float* x, const float* mean, const float* rstd,
                               const float* gamma, const float* dres, float* dx, int rows, int C, int merge, int B, int H,
                               int W, float* param_partials, uint16_t* dx_bf16, const float* cast_rowscale,
                               int cast_rows_per_sample, hipStream_t stream);
/* Split-K fold + residual epilogue + the LayerNorm that follows (proj -> norm2, fc2 -> next block's norm1, tulip.py:344-347)
 * in one launch, for a GEMM that left raw slabs [nslab][M][N]: out = aux + rowscale[row / rows_per_sample] * (sum slabs +
 * bias) (aux NULL: no residual), optional bf16 copy, then ln_out = bf16(LayerNorm(out row)), mean, rstd.  N % 256 == 0,
 * N <= 2048 (tulip_splitk_resid_ln_supported). */
int tulip_splitk_resid_ln_supported(int N);
int tulip_splitk_resid_ln(const float* slabs, int nslab, int M, int N, const float* bias, const float* aux, int ldaux,
                          const float* rowscale, int rows_per_sample, float* out, int ldo, uint16_t* out_bf16, int ldo2,
                          const float* gamma, const float* beta, uint16_t* ln_out, float* mean, float* rstd, float eps,
                          hipStream_t stream);
/* partial rows tulip_layernorm_bwd writes for (rows, C); 0 if C is too wide for the fused form (C > 2048) */
int tulip_layernorm_bwd_partial_rows(int rows, int C);

/* stand-alone dgamma[c] += sum_rows dy*xhat ; dbeta[c] += sum_rows dy (atomic; only for C > 2048) */
int tulip_layernorm_bwd_params(const uint16_t* dy, const float* x, const float* mean, const float* rstd, float* dgamma,
                               float* dbeta, int rows, int C, int merge, int B, int H, int W, hipStream_t stream);

/* PatchEmbedding (tulip.py:63-73): optional circular W padding by (2,2), Conv2d(Cin->E,(p0,kw),
 * stride (p0,p1)), BCHW->BHWC, LayerNorm(E).  img (B,Cin,Hin,Win) fp32 -> out (B,Hin/p0,Win/p1,E).
 * out_bf16 (optional): the same rows in bf16 with row pitch ld_bf16 (x_save half of the first skip concat, tulip.py:715). */
int tulip_patch_embed_fwd(const float* img, const float* w, const float* b, const float* gamma, const float* beta,
                          float* out, int B, int Cin, int Hin, int Win, int E, int p0, int p1, int kw, int circular,
                          float eps, uint16_t* out_bf16, int ld_bf16, hipStream_t stream);
/* The same launch also drawing the step's DropPath multipliers (tulip_drop_path_scales below: same generator, same counter
 * update) in its first workgroup -- nothing in this launch reads them, every later kernel of the step is ordered behind it -- so a
 * training step does not begin with a launch of its own for a few hundred numbers.  draw == NULL: exactly tulip_patch_embed_fwd.
 * Shapes the row kernel does not cover issue the draw as its own launch first. */
typedef struct tulip_drop_draw {
    const float* keep; float* scale; float* u_out; int nslots; int B; uint64_t seed; uint64_t* counter;
} tulip_drop_draw;
int tulip_patch_embed_fwd_draw(const float* img, const float* w, const float* b, const float* gamma, const float* beta,
                               float* out, int B, int Cin, int Hin, int Win, int E, int p0, int p1, int kw, int circular,
                               float eps, uint16_t* out_bf16, int ld_bf16, const tulip_drop_draw* draw, hipStream_t stream);
/* parameter gradients of the above (the input image needs no gradient).  partial_stride > 0: dw/db/dgamma/
 * dbeta point into row 0 of a [tulip_patch_embed_bwd_blocks(ntok)][partial_stride] partial buffer (plain
 * stores; fold with tulip_reduce_rows2); partial_stride == 0: accumulate atomically into the gradients.
 * Partial rows cover Cin * p0 * kw <= 16 taps at any E, and up to 32 taps (Cin 2 .. 4) at E = 48 / 96. */
int tulip_patch_embed_bwd(const float* img, const float* w, const float* b, const float* gamma, const float* dout,
                          float* dw, float* db, float* dgamma, float* dbeta, int B, int Cin, int Hin, int Win, int E,
                          int p0, int p1, int kw, int circular, float eps, int partial_stride, hipStream_t stream);
int tulip_patch_embed_bwd_blocks(int ntok);

/* Shifted-window attention core (tulip.py:289-323 minus the two Linears): cyclic shift, window
 * partition, q*scale, QK^T, + relative-position bias gathered through rel_index, + shift mask
 * (0/-100 from region labels, tulip.py:254-280), softmax, PV, window reverse, reverse shift -- all
 * as address arithmetic on natural-order tokens.  qkv is [B*H*W][3C] with channel order (T,Nh,P)
 * (tulip.py:298); out is [B*H*W][C] with channel order (Nh,P).  L = wh*ww must be 16; head dim P
 * in {16,32}.  rel_index is the module's (L,L) relative_position_index buffer as int32.
 * `masked` (here and in the block descriptors below) is a bit set: bit 0 (TULIP_ATTN_MASKED) = shifted block, apply the
 * region mask; bit 1 (TULIP_ATTN_FP8) = BASELINE configs[4] "fp8 MFMA attention": the scores Q.K^T are computed by
 * v_mfma_f32_16x16x32_fp8_fp8 from q, k rounded bf16 -> OCP e4m3 (round to nearest even); softmax, P.V and all
 * stored tensors stay as they are, and the backward multiplies dS with the same rounded q, k (it differentiates the
 * function the forward ran).  Default 0/1: the reference's bf16 / fp16 scores. */
#define TULIP_ATTN_MASKED 1
#define TULIP_ATTN_FP8 2
/* bit 2, the fused block kernels (tulip_swin96_block_fwd / _bwd, tulip_swinw_block_fwd / _bwd) only: the fc1_pre buffer carries bf16(gelu'(h)) from the forward to the backward instead
 * of the fc1 pre-activation h itself -- the derivative is all the backward wants from h (autograd of tulip.py:196), and the
 * forward has erf and the Gaussian at hand.  Forward and backward of a block must agree on it. */
#define TULIP_BLOCK_FC1_GRAD 4
/* bit 3, tulip_swinw_block_fwd / _bwd (+ split forms) only: skip the L2 warm-up at the head of the launch (below; measurement
 * and the bit-compare test only, results are identical either way) */
#define TULIP_BLOCK_NO_WARM 8
/* Shifted-window attention core on the [B*H*W][3C] qkv rows: windows of L = wh*ww tokens, L in {16, 32, 64} (2x8 / 1x16;
 * 4x8, 2x16, 1x32; 8x8, 4x16, 2x32, 1x64), head dim C/nh in {16, 32}, rel_index the module's [L][L] index.  Any other L,
 * or `masked` bit 1 (fp8 scores) with L != 16, returns TULIP_ERR_ARG before anything is launched. */
int tulip_window_attn_fwd(const uint16_t* qkv, const float* bias_table, const int32_t* rel_index, uint16_t* out, int B,
                          int H, int W, int C, int nh, int wh, int ww, int sh, int sw, int masked, hipStream_t stream);
/* dqkv from dout.  d(bias) leaves as R = tulip_window_attn_bwd_partial_rows(...) partial rows per head:
 * dbias_partials[(j*nh + h)*L*L + i*L + k], j < R  ==  a [R][nh*L*L] matrix whose column sums are the dense
 * [nh][L][L] gradient (fold + scatter into the table: tulip_reduce_rows_multi with scatter_index, scatter_len L*L).
 * L = 32 / 64: R <= max(1, 512 / nh), so the partial buffer R*nh*L*L floats is at most 2 MiB (L = 32) / 8 MiB (L = 64)
 * for nh <= 512. */
int tulip_window_attn_bwd(const uint16_t* qkv, const uint16_t* dout, const float* bias_table, const int32_t* rel_index,
                          uint16_t* dqkv, float* dbias_partials, int B, int H, int W, int C, int nh, int wh, int ww,
                          int sh, int sw, int masked, hipStream_t stream);
int tulip_window_attn_bwd_partial_rows(int B, int H, int W, int nh, int wh, int ww);

/* y_bf16 = bf16(x * rowscale[row/rows_per_sample]) ; rowscale may be NULL. x is [rows][cols]. */
int tulip_cast_f32_bf16(const float* x, uint16_t* y, int rows, int cols, const float* rowscale, int rows_per_sample,
                        hipStream_t stream);
/* flat fp32 -> bf16 copy (weight shadow refresh) */
int tulip_cast_flat(const float* x, uint16_t* y, int64_t n, hipStream_t stream);
/* flat bf16 -> fp32 copy (gradients all-reduced in bf16 come back into the fp32 gradient buffer of the optimizer) */
int tulip_cast_bf16_f32(const uint16_t* x, float* y, int64_t n, hipStream_t stream);

/* Fused head (tulip.py:724-731): conv1x1 E->16E (+bias), LeakyReLU(0.01), PixelShuffle(4),
 * conv1x1 E->in_chans (no bias, wd [in_chans][E]); xn is norm_up's bf16 output [B*H*W][E]; pred is (B,in_chans,4H,4W)
 * fp32.  The (B,16E,H,W) intermediate (100 MB at B=8) is never materialised.  upscale factor 4 (8: the _r forms below).
 * Every head entry point has a _c form with a trailing int in_chans (1 .. 4; anything else: TULIP_ERR_ARG); the form
 * without it is in_chans 1.  With in_chans > 1 the decoder_pred partial rows are [row][in_chans][128] and the L1
 * gradient divides by numel = in_chans * 16 * B*H*W. */
int tulip_tail_fwd(const uint16_t* xn, const uint16_t* We, const float* be, const float* wd, float* pred, int B, int H,
                   int W, int E, hipStream_t stream);
int tulip_tail_fwd_c(const uint16_t* xn, const uint16_t* We, const float* be, const float* wd, float* pred, int B, int H,
                     int W, int E, hipStream_t stream, int in_chans);
/* backward of the head w.r.t. the expand pre-activation: dz[B*H*W][16E] (bf16), and decoder_pred's weight
 * gradient as ceil(B*H*W/32) partial rows dwd_partials[row][128] (first E valid; fold with
 * tulip_reduce_rows2).  target == NULL: dpred is the upstream gradient of pred.  target != NULL: dpred is the
 * forward's pred and the L1 gradient gscale*sign(pred-target)/numel (forward_loss backward, tulip.py:692-693;
 * gscale read from gscale_dev if non-NULL) is formed inside the kernel. */
int tulip_tail_bwd(const uint16_t* xn, const uint16_t* We, const float* be, const float* wd, const float* dpred,
                   uint16_t* dz, float* dwd_partials, int B, int H, int W, int E, const float* target,
                   const float* gscale_dev, float gscale, hipStream_t stream);
int tulip_tail_bwd_c(const uint16_t* xn, const uint16_t* We, const float* be, const float* wd, const float* dpred,
                     uint16_t* dz, float* dwd_partials, int B, int H, int W, int E, const float* target,
                     const float* gscale_dev, float gscale, hipStream_t stream, int in_chans);
/* The same backward WITHOUT the (B,16E,H,W) gradient tensor (100 MB at batch 8, written once and read twice): both
 * consumers recompute it.  tulip_tail_bwd_dgrad (the chain): dxn[B*H*W][E] (bf16) = dz . We, the input of norm_up's
 * backward (autograd of tulip.py:724-731), and the decoder_pred partial rows exactly as tulip_tail_bwd writes them.
 * tulip_tail_wgrad (beside the chain): the expand conv's weight / bias gradient as tulip_tail_wgrad_splits(B,H,W,E) plain
 * slabs slabs_w[split][16E*E], slabs_b[split][16E] (fold with tulip_reduce_rows_multi, stride 16E*E resp. 16E).
 * dpred / target / gscale as in tulip_tail_bwd.  E % 16 == 0, E <= 128 (tulip_tail_fused_bwd_supported). */
int tulip_tail_fused_bwd_supported(int E);
int tulip_tail_bwd_dgrad(const uint16_t* xn, const uint16_t* We, const float* be, const float* wd, const float* dpred,
                         uint16_t* dxn, float* dwd_partials, int B, int H, int W, int E, const float* target,
                         const float* gscale_dev, float gscale, hipStream_t stream);
int tulip_tail_bwd_dgrad_c(const uint16_t* xn, const uint16_t* We, const float* be, const float* wd, const float* dpred,
                           uint16_t* dxn, float* dwd_partials, int B, int H, int W, int E, const float* target,
                           const float* gscale_dev, float gscale, hipStream_t stream, int in_chans);
/* tulip_tail_bwd_dgrad with norm_up's backward (autograd of tulip.py:720) in its epilogue: instead of dxn it writes what
 * tulip_layernorm_bwd would -- dx[B*H*W][E] (fp32, overwritten), optionally dx_bf16 = bf16(dx * cast_rowscale[token /
 * cast_rows_per_sample]) and ceil(B*H*W/32) partial rows ln_partials[row][2E] = [dgamma | dbeta] (fold with
 * tulip_reduce_rows_multi).  x / mean / rstd / gamma: the LayerNorm's input rows, saved statistics and weight. */
int tulip_tail_bwd_dgrad_ln(const uint16_t* xn, const uint16_t* We, const float* be, const float* wd, const float* dpred,
                            float* dwd_partials, int B, int H, int W, int E, const float* target, const float* gscale_dev,
                            float gscale, const float* x, const float* mean, const float* rstd, const float* gamma,
                            float* dx, uint16_t* dx_bf16, const float* cast_rowscale, int cast_rows_per_sample,
                            float* ln_partials, hipStream_t stream);
int tulip_tail_bwd_dgrad_ln_c(const uint16_t* xn, const uint16_t* We, const float* be, const float* wd, const float* dpred,
                              float* dwd_partials, int B, int H, int W, int E, const float* target, const float* gscale_dev,
                              float gscale, const float* x, const float* mean, const float* rstd, const float* gamma,
                              float* dx, uint16_t* dx_bf16, const float* cast_rowscale, int cast_rows_per_sample,
                              float* ln_partials, hipStream_t stream, int in_chans);
/* tulip_tail_fwd with norm_up (tulip.py:720: LayerNorm(E) of the fp32 rows x, eps) in front -- xn / mean / rstd are written
 * for the backward -- and, when loss_partials != NULL, the partial sums of forward_loss (tulip.py:690-700) behind it:
 * loss_partials[2*wg] = sum |pred - target|, [2*wg+1] = sum |expm1(pred) - expm1(target)| (log_transform) over the
 * workgroup's 32 tokens, wg < ceil(B*H*W/32); tulip_l1_loss_final folds them into losses[2] (mean over n elements). */
int tulip_tail_fwd_ln(const float* x, const float* gamma, const float* beta, float eps, uint16_t* xn, float* mean,
                      float* rstd, const uint16_t* We, const float* be, const float* wd, float* pred, const float* target,
                      float* loss_partials, int log_transform, int B, int H, int W, int E, hipStream_t stream);
int tulip_tail_fwd_ln_c(const float* x, const float* gamma, const float* beta, float eps, uint16_t* xn, float* mean,
                        float* rstd, const uint16_t* We, const float* be, const float* wd, float* pred, const float* target,
                        float* loss_partials, int log_transform, int B, int H, int W, int E, hipStream_t stream,
                        int in_chans);
int tulip_l1_loss_final(const float* partials, float* losses, int nblocks, int64_t n, int log_transform,
                        hipStream_t stream);
int tulip_tail_wgrad_splits(int B, int H, int W, int E);
int tulip_tail_wgrad(const uint16_t* xn, const uint16_t* We, const float* be, const float* wd, const float* dpred,
                     float* slabs_w, float* slabs_b, int B, int H, int W, int E, const float* target,
                     const float* gscale_dev, float gscale, hipStream_t stream);
int tulip_tail_wgrad_c(const uint16_t* xn, const uint16_t* We, const float* be, const float* wd, const float* dpred,
                       float* slabs_w, float* slabs_b, int B, int H, int W, int E, const float* target,
                       const float* gscale_dev, float gscale, hipStream_t stream, int in_chans);
/* Upscale factor r (PixelShuffle(r); tulip.py:577: r = int(sqrt(target area / image area)) * 2 * int(sqrt(patch area // 4)),
 * 4 for patches of 4 .. 15 pixels, 8 for 16-pixel patches such as (2, 8) and (4, 4)).  Every head entry point has an _r form
 * with trailing (int in_chans, int r), r in {4, 8} (anything else: TULIP_ERR_ARG, before any launch); the forms above are
 * r = 4.  At r = 8 the expand conv is E -> 64E: We [64E][E], be [64E], output column oc = c*64 + i*8 + j (four MFMA column
 * tiles per channel), pred / target / dpred are (B,in_chans,8H,8W), dz is [B*H*W][64E], the wgrad slabs are
 * slabs_w[split][64E*E], slabs_b[split][64E] with tulip_tail_wgrad_splits_r(B,H,W,E,in_chans,r) splits, and the L1 gradient divides by
 * numel = in_chans * 64 * B*H*W.  As at r = 4, only tulip_tail_bwd_r materialises the (B,r*r*E,H,W) gradient.  The partial
 * rows (decoder_pred, norm_up, loss) keep their r = 4 layout: one row per 32 tokens. */
int tulip_tail_fwd_r(const uint16_t* xn, const uint16_t* We, const float* be, const float* wd, float* pred, int B, int H,
                     int W, int E, hipStream_t stream, int in_chans, int r);
int tulip_tail_bwd_r(const uint16_t* xn, const uint16_t* We, const float* be, const float* wd, const float* dpred,
                     uint16_t* dz, float* dwd_partials, int B, int H, int W, int E, const float* target,
                     const float* gscale_dev, float gscale, hipStream_t stream, int in_chans, int r);
int tulip_tail_fused_bwd_supported_r(int E, int r);
int tulip_tail_bwd_dgrad_r(const uint16_t* xn, const uint16_t* We, const float* be, const float* wd, const float* dpred,
                           uint16_t* dxn, float* dwd_partials, int B, int H, int W, int E, const float* target,
                           const float* gscale_dev, float gscale, hipStream_t stream, int in_chans, int r);
int tulip_tail_bwd_dgrad_ln_r(const uint16_t* xn, const uint16_t* We, const float* be, const float* wd, const float* dpred,
                              float* dwd_partials, int B, int H, int W, int E, const float* target, const float* gscale_dev,
                              float gscale, const float* x, const float* mean, const float* rstd, const float* gamma,
                              float* dx, uint16_t* dx_bf16, const float* cast_rowscale, int cast_rows_per_sample,
                              float* ln_partials, hipStream_t stream, int in_chans, int r);
int tulip_tail_fwd_ln_r(const float* x, const float* gamma, const float* beta, float eps, uint16_t* xn, float* mean,
                        float* rstd, const uint16_t* We, const float* be, const float* wd, float* pred, const float* target,
                        float* loss_partials, int log_transform, int B, int H, int W, int E, hipStream_t stream,
                        int in_chans, int r);
int tulip_tail_wgrad_splits_r(int B, int H, int W, int E, int in_chans, int r);
int tulip_tail_wgrad_r(const uint16_t* xn, const uint16_t* We, const float* be, const float* wd, const float* dpred,
                       float* slabs_w, float* slabs_b, int B, int H, int W, int E, const float* target,
                       const float* gscale_dev, float gscale, hipStream_t stream, int in_chans, int r);


/* The non-default decoder alternates PatchExpanding (tulip.py:126-140, patch_unmerging=False; P = 2, Cn = C/2) and
 * FinalPatchExpanding (tulip.py:144-159, pixel_shuffle=False; P = upscale_factor, Cn = embed_dim):
 * Linear(no bias) -> 'B H W (P1 P2 C) -> B (H P1) (W P2) C' -> LayerNorm(Cn).  The Linear is tulip_gemm_bf16 with
 * TULIP_EPI_F32 into y [B*H*W][P*P*Cn] fp32; a fine token is a contiguous Cn-slice of a row of y, so the rearrange is
 * the OUTPUT addressing of these kernels.  fwd: LayerNorm of every slice -> out_bf16 (optional; fine-token order,
 * row pitch ld, e.g. the first half of a skip-concat buffer, tulip.py:715) and/or pred[fine token] =
 * sum_c dotw[c] * bf16(LayerNorm out)[c] (optional: decoder_pred, tulip.py:731, the (B,PH,PW,Cn) tensor is never
 * stored; the _c forms take a trailing in_chans 1 .. 4: dotw [in_chans][Cn], pred (B,in_chans,PH,PW), Cn <= 256 when
 * in_chans > 1).  mean / rstd: [B*H*W*P*P] in the (coarse token, p) order of y.
 * bwd: upstream gradient either as bf16 rows dy_fine (fine-token order, row pitch ld) or, when dotw != NULL, as
 * dpred[fine token] (then d(LayerNorm out)[c] = dpred * dotw[c]) -> dy_nat = bf16 d(y) in y's layout (operand of the
 * Linear's dgrad / wgrad GEMMs) and tulip_expand_norm_bwd_partial_rows(...) partial rows of
 * [dgamma[Cn] | dbeta[Cn] | d(dotw)[in_chans][Cn]] (stride (2 + in_chans)*Cn; fold with tulip_reduce_rows_multi).
 * Cn % 4 == 0, Cn <= 768. */
int tulip_expand_norm_fwd(const float* y, const float* gamma, const float* beta, uint16_t* out_bf16, int ld,
                          const float* dotw, float* pred, float* mean, float* rstd, int B, int H, int W, int P, int Cn,
                          float eps, hipStream_t stream);
int tulip_expand_norm_bwd(const uint16_t* dy_fine, int ld, const float* dpred, const float* dotw, const float* y,
                          const float* mean, const float* rstd, const float* gamma, const float* beta, uint16_t* dy_nat,
                          float* partials, int B, int H, int W, int P, int Cn, hipStream_t stream);
int tulip_expand_norm_fwd_c(const float* y, const float* gamma, const float* beta, uint16_t* out_bf16, int ld,
                            const float* dotw, float* pred, float* mean, float* rstd, int B, int H, int W, int P, int Cn,
                            float eps, hipStream_t stream, int in_chans);
int tulip_expand_norm_bwd_c(const uint16_t* dy_fine, int ld, const float* dpred, const float* dotw, const float* y,
                            const float* mean, const float* rstd, const float* gamma, const float* beta, uint16_t* dy_nat,
                            float* partials, int B, int H, int W, int P, int Cn, hipStream_t stream, int in_chans);
int tulip_expand_norm_bwd_partial_rows(int B, int H, int W, int P);

/* forward_loss (tulip.py:690-700): losses[0]=mean|pred-target|, losses[1]=mean|expm1(pred)-expm1(target)|
 * (or a copy of losses[0] when log_transform==0).  partials: scratch of 2*1024 floats. Deterministic. */
int tulip_l1_loss_fwd(const float* pred, const float* target, float* partials, float* losses, int64_t n,
                      int log_transform, hipStream_t stream);
/* dpred = gscale * sign(pred-target)/n ; gscale read from device memory if gscale_dev!=NULL */
int tulip_l1_loss_bwd(const float* pred, const float* target, const float* gscale_dev, float gscale, float* dpred,
                      int64_t n, hipStream_t stream);

/* The selectable training loss, TULIP(loss="l1" | "l2" | "berhu") (host definition: tulip_amd/loss.py).  With d = pred - target
 * over n elements:
 *   TULIP_LOSS_L2     loss = mean d^2,  d(loss)/d(pred) = 2 d / n
 *   TULIP_LOSS_BERHU  C = 0.2f * max|d| (fp32, constant under differentiation: util/evaluation.py:177-180, inverse_huber_loss);
 *                     value |d| where |d| < C, (d^2 + C^2) / (2 C) elsewhere; loss = the mean of the values; gradient sign(d) / n
 *                     where |d| < C, d / (C n) elsewhere.  C == 0 (pred == target everywhere, 0/0 in the reference): loss and
 *                     gradient are 0.  A NaN in d reaches C (the max keeps it), every value and every gradient element.
 *   TULIP_LOSS_L1     tulip_l1_loss_fwd / _bwd's arithmetic (the training step keeps calling those)
 * Flat kernels: tulip_loss_blocks(n) = min(1024, ceil(ceil(n / 4) / 256)) workgroups of 256 threads, float4 loads where pred,
 * target (and dpred) are 16-byte aligned and a scalar tail, every reduction in a fixed order (deterministic), plain stores, no
 * atomics, graph-capturable.  losses[1] stays the L1 metric of tulip_l1_loss_fwd for every kind.
 *   tulip_loss_stats  one pass: stats[4 wg + {0, 1, 2, 3}] = {sum |d|, sum |expm1(pred) - expm1(target)| (log_transform, else 0),
 *                     sum d^2, max |d| (NaN-keeping)} per workgroup; stats: 4 * TULIP_LOSS_BLOCKS_MAX floats, 16-byte aligned
 *   tulip_loss_bwd    dpred[i] = g * grad_kind(d_i; C), g = fl32((gscale_dev ? gscale_dev[0] : gscale) / n).  BERHU: every workgroup
 *                     folds the maxima of `stats` itself (max is exact: the same C everywhere) and loss_c[0] = C is written;
 *                     other kinds read neither stats nor loss_c (both may be NULL)
 *   tulip_loss_value  BERHU's second pass (the sum needs C): value_partials[wg] = the workgroup's sum of the elementwise values;
 *                     value_partials: TULIP_LOSS_BLOCKS_MAX floats
 *   tulip_loss_final  one workgroup, the partials folded in double: losses[0] = the loss of `kind`, losses[1] = the mean of
 *                     stats' second sums (log_transform) or of the first.  value_partials is read for BERHU only
 * TULIP_ERR_ARG before any launch: an unknown kind, n <= 0, a NULL required pointer, a misaligned stats. */
#define TULIP_LOSS_L1 0
#define TULIP_LOSS_L2 1
#define TULIP_LOSS_BERHU 2
#define TULIP_LOSS_BLOCKS_MAX 1024
int tulip_loss_blocks(int64_t n);
int tulip_loss_stats(const float* pred, const float* target, float* stats, int64_t n, int log_transform, hipStream_t stream);
int tulip_loss_bwd(int kind, const float* pred, const float* target, const float* stats, const float* gscale_dev, float gscale,
                   float* dpred, float* loss_c, int64_t n, hipStream_t stream);
int tulip_loss_value(const float* pred, const float* target, const float* stats, float* value_partials, int64_t n,
                     hipStream_t stream);
int tulip_loss_final(int kind, const float* stats, const float* value_partials, float* losses, int64_t n, int log_transform,
                     hipStream_t stream);

/* The masked forms, TULIP(loss_valid_min=v) (host definition: tulip_amd/loss.py): the same four launches over the VALID elements.
 * pred / target are (B, chans, chan_stride) with n = B * chans * chan_stride; pixel (b, pix) is valid iff
 * target[b, 0, pix] > valid_min -- channel 0, the range; false for a NaN -- and all `chans` elements of a valid pixel count:
 * n_v = chans * (valid pixels) stands where n stands above (L1: sum|d| / n_v, gradient sign(d) / n_v; L2: sum d^2 / n_v, 2 d / n_v;
 * BERHU: C = 0.2f * max over the valid |d|, values and gradient as above with n_v; losses[1]: the L1 metric over the valid
 * elements).  The gradient at an invalid element is +0.0f.  n_v == 0: losses, C and every gradient are 0.  Whatever pred or any
 * channel of target holds at an invalid pixel (a NaN, an infinity; a NaN in target[b, 0, pix] makes the pixel invalid) changes
 * nothing; a non-finite value at a valid element propagates as above.  For chans == 1 the mask is the element's own target value
 * (no second load); for chans > 1 the kernels read target[b, 0, pix].  Same grid, same fixed reduction orders, plain stores, no
 * atomics; float4 loads only where pred, target (and dpred) are 16-byte aligned AND chan_stride % 4 == 0 (a group then never
 * straddles a channel, and target's channel-0 rows are aligned too), the scalar route otherwise.
 *   tulip_loss_stats_m  stats as above over the valid elements (the NaN-keeping max too), and counts[wg] = the workgroup's number
 *                       of valid elements (integers: per thread, the wave tree, four wave results); counts:
 *                       TULIP_LOSS_BLOCKS_MAX uint32
 *   tulip_loss_bwd_m    every workgroup folds `counts` itself (integer addition is exact in any order: the same n_v everywhere);
 *                       g = fl32(gscale / (float)n_v), one rounding; n_valid[0] = n_v.  stats / loss_c as in tulip_loss_bwd
 *   tulip_loss_value_m  BERHU's second pass over the valid elements (n_v == 0: zeros, nothing read)
 *   tulip_loss_final_m  1 / (double)n_v formed on the device (0 when n_v == 0); n_valid[0] = n_v
 * TULIP_ERR_ARG before any launch, besides the cases above: chans < 1, chan_stride < 1, n no multiple of chans * chan_stride,
 * n >= 2^41, a NaN or infinite valid_min, a NULL or misaligned counts / n_valid. */
int tulip_loss_stats_m(const float* pred, const float* target, float* stats, int64_t n, int log_transform, int chans,
                       int64_t chan_stride, float valid_min, uint32_t* counts, hipStream_t stream);
int tulip_loss_bwd_m(int kind, const float* pred, const float* target, const float* stats, const float* gscale_dev, float gscale,
                     float* dpred, float* loss_c, int64_t n, int chans, int64_t chan_stride, float valid_min,
                     const uint32_t* counts, int64_t* n_valid, hipStream_t stream);
int tulip_loss_value_m(const float* pred, const float* target, const float* stats, float* value_partials, int64_t n, int chans,
                       int64_t chan_stride, float valid_min, const uint32_t* counts, hipStream_t stream);
int tulip_loss_final_m(int kind, const float* stats, const float* value_partials, float* losses, int64_t n, int log_transform,
                       const uint32_t* counts, int64_t* n_valid, hipStream_t stream);

/* The edge term, TULIP(loss_edge_weight=w) (host definition: tulip_amd/loss.py): w * mean(|e_h| + |e_v|) beside the loss above,
 * e_h / e_v the 3x3 Sobel responses of d = pred - target (the reference's util/filter.py, zero padding) on each of the `planes`
 * = B * C planes of H x W on its own: nothing is read across a row end, a plane or a sample, and the columns do not wrap.
 * fp32 order: e_h = ((d[+1,-1] - d[-1,-1]) + 2 (d[+1,0] - d[-1,0])) + (d[+1,+1] - d[-1,+1]) (d[dy,dx]), e_v the transposed
 * pattern; sign(e) = (e > 0) - (e < 0), 0 for a NaN.  One workgroup of 256 threads per 8 x 128 tile, the tile and its halo
 * staged in LDS, workgroup-strided over the tiles: tulip_loss_edge_blocks(planes, H, W) = min(TULIP_LOSS_BLOCKS_MAX, tiles)
 * workgroups (host-only).  Fixed reduction orders, plain stores, no atomics, graph-capturable, 64-bit element offsets.
 *   tulip_loss_edge_stats  edge_partials[wg] = the workgroup's sum of |e_h| + |e_v| (per thread, the wave tree, four wave results);
 *                          edge_partials: TULIP_LOSS_BLOCKS_MAX floats
 *   tulip_loss_edge_bwd    dpred[e] = fl32(dpred[e] + fl32(ge * k[e])) in place behind the base gradient, with
 *                          g = fl32((gscale_dev ? gscale_dev[0] : gscale) / n) as in tulip_loss_bwd, ge = fl32(weight * g) and
 *                          k[p,q] = sum_{i,j} K_h[i,j] sign(e_h[p-i+1,q-j+1]) + the same with K_v (an integer in [-16, 16];
 *                          terms whose centre is outside the plane: 0).  A multiply, then an add: no fma
 *   tulip_loss_edge_final  one workgroup behind the base loss's final launch: the partials folded in double,
 *                          edge_out[0] = edge32 = fl32(sum / n), losses[0] = fl32(losses[0] + fl32(weight * edge32))
 * The _m forms (TULIP(loss_valid_min=v)): pixel (b, y, x) is valid iff target[b, 0, y, x] > valid_min, plane p belonging to sample
 * p / chans.  d is +0 at an invalid pixel (by selection: a NaN there reaches nothing), a response counts -- in the sum and in k --
 * only where its centre is valid, n_v = the sum of the counts tulip_loss_stats_m wrote stands where n stands (n_v == 0: edge 0,
 * gradient 0), and dpred is +0 at the invalid elements.
 * TULIP_ERR_ARG before any launch: a non-positive planes / H / W (or n >= 2^41, H or W within 144 of INT_MAX, 2^31 or more
 * tiles in one plane: the kernels' tile and pixel coordinates are 32-bit, only the element offsets 64-bit), a NULL pred / target / dpred / edge_partials /
 * edge_out / losses, a misaligned edge_partials, a negative, NaN or infinite weight; _m: chans < 1, planes no multiple of chans,
 * a NaN or infinite valid_min, a NULL or misaligned counts. */
int tulip_loss_edge_blocks(int64_t planes, int H, int W);
int tulip_loss_edge_stats(const float* pred, const float* target, float* edge_partials, int64_t planes, int H, int W,
                          hipStream_t stream);
int tulip_loss_edge_bwd(const float* pred, const float* target, const float* gscale_dev, float gscale, float weight, float* dpred,
                        int64_t planes, int H, int W, hipStream_t stream);
int tulip_loss_edge_final(const float* edge_partials, float* edge_out, float* losses, float weight, int64_t planes, int H, int W,
                          hipStream_t stream);
int tulip_loss_edge_stats_m(const float* pred, const float* target, float* edge_partials, int64_t planes, int H, int W, int chans,
                            float valid_min, hipStream_t stream);
int tulip_loss_edge_bwd_m(const float* pred, const float* target, const float* gscale_dev, float gscale, float weight,
                          float* dpred, int64_t planes, int H, int W, int chans, float valid_min, const uint32_t* counts,
                          hipStream_t stream);
int tulip_loss_edge_final_m(const float* edge_partials, float* edge_out, float* losses, float weight, int64_t planes, int H, int W,
                            const uint32_t* counts, hipStream_t stream);

/* The channel weights, TULIP(loss_channel_weights=(w_0, .., w_{chans-1})) (host definition: tulip_amd/loss.py): the launches above
 * with element e of channel c = (e / chan_stride) % chans COUNTED iff w_c > 0 and -- masked != 0 -- its pixel is valid
 * (target[b, 0, pix] > valid_min, channel 0 even where w_0 == 0; masked == 0: valid_min is not read).  n_S, the number of counted
 * elements, stands where n / n_v stand above: loss = (1 / n_S) sum_S w_c f(d), gradient g_c f'(d) with g = fl32(gscale / n_S) and
 * g_c = fl32(w_c * g) once per channel, +0.0f at the elements that are not counted; BERHU: one C = 0.2f * max over S of |d|,
 * unweighted; n_S == 0: zeros.  An element that is not counted enters nothing: a NaN or an infinity in a w_c == 0 channel of pred
 * or target changes no bit.  `weights` is a HOST array of `chans` floats read during the call and passed to the kernels by value
 * in the launch arguments: no device buffer holds them, and a captured graph keeps the values it was captured with.  One family
 * for the masked and the unmasked case; counts / n_valid as in the _m forms, always.
 *   tulip_loss_stats_w  stats[4 wg + {0, 1, 2, 3}] = {sum w_c |d|, the UNWEIGHTED metric sum -- |expm1(pred) - expm1(target)| with
 *                       log_transform, |d| without --, sum w_c d^2, max |d|} over the workgroup's counted elements (value terms
 *                       fl32(w_c * term), then the sums above; d^2 as fl32(w_c * d) * d into the accumulator), counts[wg] = how
 *                       many there were.  The weighted L1 value and the metric are different sums: slot 1 is always filled
 *   tulip_loss_bwd_w    as tulip_loss_bwd_m with g_c where g stands; n_valid[0] = n_S
 *   tulip_loss_value_w  BERHU's second pass: the sums of fl32(w_c * value) over the counted elements
 *   tulip_loss_final_w  losses[0] = the weighted loss of `kind`, losses[1] = slot 1's sum / n_S (the L1 metric over S); n_valid[0] = n_S
 *   tulip_loss_edge_stats_w  the sums of fl32(w_c * fl32(|e_h| + |e_v|)), c = plane % chans; a plane with w_c == 0 is not read
 *   tulip_loss_edge_bwd_w    ge_c = fl32(weight * g_c) where ge stands, n_S from `counts` (masked or not); a plane with w_c == 0
 *                            is neither read nor written: dpred keeps the +0.0f tulip_loss_bwd_w wrote there
 *   tulip_loss_edge_final_w  tulip_loss_edge_final_m's fold with n_S
 * Same grids as above; every thread takes the elements the unweighted kernel of the same case gives it (groups of four where the
 * pointers are 16-byte aligned -- masked: and chan_stride % 4 == 0 --, a scalar tail), so with every w_c == 1.0f the results are
 * that kernel's, bit for bit.  A group is loaded as a float4 only where chan_stride % 4 == 0 (it then lies in one channel);
 * elsewhere by four scalar loads, every element with its own channel.  Fixed reduction orders, plain stores, no atomics, 64-bit
 * element offsets, graph-capturable.
 * TULIP_ERR_ARG before any launch, besides the cases of the _m forms: chans outside 1..4, a NULL weights, a negative, NaN or
 * infinite weight, all weights 0. */
int tulip_loss_stats_w(const float* pred, const float* target, float* stats, int64_t n, int log_transform, int chans,
                       int64_t chan_stride, const float* weights, int masked, float valid_min, uint32_t* counts, hipStream_t stream);
int tulip_loss_bwd_w(int kind, const float* pred, const float* target, const float* stats, const float* gscale_dev, float gscale,
                     float* dpred, float* loss_c, int64_t n, int chans, int64_t chan_stride, const float* weights, int masked,
                     float valid_min, const uint32_t* counts, int64_t* n_valid, hipStream_t stream);
int tulip_loss_value_w(const float* pred, const float* target, const float* stats, float* value_partials, int64_t n, int chans,
                       int64_t chan_stride, const float* weights, int masked, float valid_min, const uint32_t* counts,
                       hipStream_t stream);
int tulip_loss_final_w(int kind, const float* stats, const float* value_partials, float* losses, int64_t n, const uint32_t* counts,
                       int64_t* n_valid, hipStream_t stream);
int tulip_loss_edge_stats_w(const float* pred, const float* target, float* edge_partials, int64_t planes, int H, int W, int chans,
                            const float* weights, int masked, float valid_min, hipStream_t stream);
int tulip_loss_edge_bwd_w(const float* pred, const float* target, const float* gscale_dev, float gscale, float weight,
                          float* dpred, int64_t planes, int H, int W, int chans, const float* weights, int masked,
                          float valid_min, const uint32_t* counts, hipStream_t stream);
int tulip_loss_edge_final_w(const float* edge_partials, float* edge_out, float* losses, float weight, int64_t planes, int H, int W,
                            const uint32_t* counts, hipStream_t stream);

/* Fused AdamW over a flat parameter buffer (torch.optim.AdamW semantics, main_lidar_upsampling.py:283):
 * hyper (device, 8 floats) = {lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2, grad_scale}.
 * decay_mask64[i/64] bit 0 selects weight decay for elements of 64-float block i/64 (timm's grouping,
 * main:282: decay only for ndim>1 parameters), bit 1 SKIPS the block (its step was taken elsewhere:
 * tulip_wgrad_group_adamw); NULL = decay everywhere, skip nothing.  Also refreshes the bf16 shadow.
 * zero_grad != 0: g is cleared after it has been consumed (optimizer.zero_grad(), engine_upsampling.py:97). */
int tulip_adamw(float* p, float* g, float* m, float* v, uint16_t* p_bf16, int64_t n, const float* hyper,
                const uint8_t* decay_mask64, int zero_grad, hipStream_t stream);
/* The same step for the 64-float blocks blocks[0..nblocks) only (device int32 block indices; decay_mask64 is indexed by block,
 * bit 1 is ignored): the end-of-step launch when most tensors were stepped where their gradient was completed
 * (tulip_wgrad_group_adamw, tulip_reduce_rows_multi_adamw) -- nothing is scanned. */
int tulip_adamw_blocks(float* p, float* g, float* m, float* v, uint16_t* p_bf16, const int32_t* blocks, int nblocks,
                       const float* hyper, const uint8_t* decay_mask64, int zero_grad, hipStream_t stream);
/* tulip_adamw / tulip_adamw_blocks with per-group learning-rate scales (see tulip_wgrad_group_adamw_s): block i/64 is stepped
 * with lr_g = fl32(hyper[0] * lr_scale64[decay_mask64[i/64] >> 2]); bits 0 and 1 of the mask byte keep their meaning.
 * lr_scale64 == NULL: exactly tulip_adamw / tulip_adamw_blocks; lr_scale64 with decay_mask64 == NULL: TULIP_ERR_ARG. */
int tulip_adamw_s(float* p, float* g, float* m, float* v, uint16_t* p_bf16, int64_t n, const float* hyper,
                  const uint8_t* decay_mask64, const float* lr_scale64, int zero_grad, hipStream_t stream);
int tulip_adamw_blocks_s(float* p, float* g, float* m, float* v, uint16_t* p_bf16, const int32_t* blocks, int nblocks,
                         const float* hyper, const uint8_t* decay_mask64, const float* lr_scale64, int zero_grad,
                         hipStream_t stream);
/* tulip_adamw_s / tulip_adamw_blocks_s behind the non-finite guard (tulip_step_guard below): skip[0] != 0 (device word, one
 * launch-uniform load) leaves p, m, v and p_bf16 unread and unwritten; with zero_grad the launch still clears the gradients the
 * step would have cleared, and does nothing else.  skip[0] == 0 or skip == NULL: the bits of the _s entry. */
int tulip_adamw_g(float* p, float* g, float* m, float* v, uint16_t* p_bf16, int64_t n, const float* hyper,
                  const uint8_t* decay_mask64, const float* lr_scale64, int zero_grad, const uint32_t* skip, hipStream_t stream);
int tulip_adamw_blocks_g(float* p, float* g, float* m, float* v, uint16_t* p_bf16, const int32_t* blocks, int nblocks,
                         const float* hyper, const uint8_t* decay_mask64, const float* lr_scale64, int zero_grad,
                         const uint32_t* skip, hipStream_t stream);

/* Weight EMA: one update of an exponential moving average `shadow` of the parameters `p` (n floats, n % 4 == 0, both 16-byte
 * aligned), torch_ema's ExponentialMovingAverage.update() as tulip_amd/ema.py restates it:
 *   num_updates != NULL:  *num_updates += 1 (device word);  d = min(decay, (1 + *num_updates) / (10 + *num_updates))   [float64]
 *   num_updates == NULL:  d = decay                                                                  (no warm-up, no counter)
 *   omd = (float)(1.0 - d), written to omd_slot[0] (device)
 *   per element, float32, three separately rounded operations, no fused multiply-add:  t = s - p;  t = omd * t;  s = s - t
 * Two launches in stream order: the coefficient (one workgroup; the counter and omd live in device memory, so a captured graph
 * replays the warm-up schedule with no host upload), then one streaming pass.  Bit-identical to the host definition.
 * n <= 0: TULIP_OK, nothing launched.  n % 4 != 0, p / shadow / omd_slot NULL or misaligned, decay outside [0, 1] (NaN included):
 * TULIP_ERR_ARG before any launch. */
int tulip_ema_update(const float* p, float* shadow, int64_t n, double decay, uint64_t* num_updates, float* omd_slot,
                     hipStream_t stream);
/* ... behind the non-finite guard: skip[0] != 0 (device word) -- the counter does not advance, omd_slot and the shadow are not
 * touched (the streaming kernel returns at entry; NOT omd = 0, which would turn a shadow of -0 over a parameter of +0 into +0).
 * skip[0] == 0 or skip == NULL: the bits of tulip_ema_update. */
int tulip_ema_update_g(const float* p, float* shadow, int64_t n, double decay, uint64_t* num_updates, float* omd_slot,
                       const uint32_t* skip, hipStream_t stream);

/* DropPath multipliers of one step (tulip.py:25-29; timm drop_path: keep a sample's residual branch with
 * probability keep, scale kept branches by 1/keep): scale[slot*B+b] = floor(keep[slot] + u)/keep[slot] with
 * u ~ U[0,1) from a counter-based generator keyed by (seed, *counter, index).  *counter is advanced by one:
 * replaying the launch from a HIP graph draws fresh numbers every step.  u_out (optional) receives the draws. */
int tulip_drop_path_scales(const float* keep, float* scale, float* u_out, int nslots, int B, uint64_t seed,
                           uint64_t* counter, hipStream_t stream);

/* Element dropout (nn.Dropout, tulip.py:190-192, 315, 319, 705): y = x * m / (1-p), m a Bernoulli(1-p) keep mask that is
 * counter-based -- nothing is stored, the backward regenerates it.  The mask function, bit for bit (host code reproduces it):
 *   mix64(z)        = splitmix64 finaliser: z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB;
 *                     z ^= z >> 31  (uint64 arithmetic)
 *   key             = mix64(seed ^ mix64(counter * 2^20 + site))
 *   u(index)        = mix64(key + index) >> 40                  (top 24 bits)
 *   kept(index)     = u(index) >= rint(p * 2^24)                (p as fp32, rint = round half to even)
 *   scale           = 1.0f / (1.0f - p)                          (fp32, correctly rounded)
 * seed: the engine's DropPath seed; counter: *key_ptr, a device word the forward records once per step (tulip_dropout_begin),
 * read through the pointer by every dropout launch of that forward and of its backward, so graph replays draw fresh masks;
 * site: 0 = pos_drop, block i (engine order) 1 + 4 i + {0 attn_drop, 1 proj_drop, 2 mlp.drop1, 3 mlp.drop2};
 * index: row * cols + c over natural token rows (pos_drop, proj_drop, drop2: cols = C; drop1: cols = hidden), and for
 * attn_drop ((((b * nWy + wy) * nWx + wx) * nh + head) * L + q) * L + k, L = wh * ww the window's tokens, (wy, wx) the window of
 * the rolled image, q / k the in-window slots i * ww + j -- the flattening of the reference's [B * nW, nh, N, N] probability
 * tensor.  p in [0, 1). */
/* *key_out = *counter; advance != 0: *counter += 1 (a forward whose DropPath draw does not advance it already) */
int tulip_dropout_begin(uint64_t* counter, uint64_t* key_out, int advance, hipStream_t stream);
/* mask read-out: out[i] = kept(i) ? scale : 0, i < n (fp32) */
int tulip_dropout_mask(const uint64_t* key_ptr, uint64_t seed, int site, float p, int64_t n, float* out, hipStream_t stream);
/* in place: x[r * ld + c] *= kept(r * cols + c) ? scale : 0, x fp32 (is_bf16 = 0) or bf16 (is_bf16 = 1, rounded to nearest
 * even); cols % 4 == 0, ld % 4 == 0 */
int tulip_dropout_scale(void* x, int is_bf16, int rows, int cols, int ld, const uint64_t* key_ptr, uint64_t seed, int site,
                        float p, hipStream_t stream);
/* residual with dropout (proj_drop / drop2 of a block; y = the fp32 Linear output incl. bias, TULIP_EPI_F32):
 * out = aux + rowscale[r / rows_per_sample] * (y * (kept ? scale : 0)) ([rows][C], y may alias out), out_bf16 (optional)
 * = bf16(out), and, gamma != NULL, the LayerNorm behind it exactly as tulip_layernorm_fwd computes it (xn, mean, rstd).
 * rowscale may be NULL.  C % 4 == 0. */
int tulip_dropout_resid_ln(const float* y, const float* aux, const float* rowscale, int rows_per_sample, float* out,
                           uint16_t* out_bf16, const float* gamma, const float* beta, uint16_t* xn, float* mean, float* rstd,
                           float eps, int rows, int C, const uint64_t* key_ptr, uint64_t seed, int site, float p,
                           hipStream_t stream);
/* backward of the above: y = bf16(dx * rowscale[r / rows_per_sample] * (kept ? scale : 0)), [rows][cols]; rowscale may be NULL */
int tulip_dropout_cast(const float* dx, uint16_t* y, int rows, int cols, const float* rowscale, int rows_per_sample,
                       const uint64_t* key_ptr, uint64_t seed, int site, float p, hipStream_t stream);
/* tulip_window_attn_fwd / _bwd with attn_drop on the softmax probabilities (P.V from the dropped probabilities; backward:
 * dV from the dropped probabilities, dP = (dO.V^T) * mask * scale, dS = P * (dP - rowsum(dP * P))).  `masked` bit 1 (fp8
 * scores) is refused with TULIP_ERR_ARG before anything is launched. */
int tulip_window_attn_fwd_drop(const uint16_t* qkv, const float* bias_table, const int32_t* rel_index, uint16_t* out, int B,
                               int H, int W, int C, int nh, int wh, int ww, int sh, int sw, int masked,
                               const uint64_t* key_ptr, uint64_t seed, int site, float p, hipStream_t stream);
int tulip_window_attn_bwd_drop(const uint16_t* qkv, const uint16_t* dout, const float* bias_table, const int32_t* rel_index,
                               uint16_t* dqkv, float* dbias_partials, int B, int H, int W, int C, int nh, int wh, int ww,
                               int sh, int sw, int masked, const uint64_t* key_ptr, uint64_t seed, int site, float p,
                               hipStream_t stream);

/* Gradient L2 norm read-out (misc.py:317-329 get_grad_norm_, taken before the optimizer step, misc.py:303):
 * out[0] = sqrt(sum g[i]^2) * scale * (scale_dev ? scale_dev[0] : 1).  partials: scratch of 1024 doubles.
 * Fixed partition and fold order: deterministic. */
int tulip_grad_norm(const float* g, int64_t n, double* partials, const float* scale_dev, float scale, float* out,
                    hipStream_t stream);

/* Gradient clipping by global norm (misc.py:299-300: torch.nn.utils.clip_grad_norm_(parameters, clip_grad) in front of
 * optimizer.step()), folded into the gradient scale the AdamW launches behind it read (hyper[7] of tulip_adamw):
 *   t = sum g[i]^2 (tulip_grad_norm's partition and fold order);  base = grad_scale[0];
 *   norm = (float)(sqrt(t) * (double)base)     -- what tulip_grad_norm(g, n, partials, grad_scale, 1.0f, out) writes
 *   c = max_norm_dev[0] / (norm + 1e-6f);  coef = c > 1.0f ? 1.0f : c    (fp32, one rounding per operation; a NaN norm gives
 *                                                                          a NaN coef, an infinite norm gives 0)
 *   out[0] = norm, out[1] = coef, grad_scale[0] = base * coef            (coef == 1.0f: grad_scale keeps its bits)
 * Two launches in stream order, graph-capturable, nothing allocated.  g is only read and 16-byte aligned; partials: scratch of
 * 1024 doubles.  TULIP_ERR_ARG before any launch: n <= 0, a NULL pointer, a misaligned g.  Host definition:
 * tulip_amd/clip.py. */
int tulip_grad_clip(const float* g, int64_t n, double* partials, float* grad_scale, const float* max_norm_dev, float* out,
                    hipStream_t stream);

/* Non-finite guard (GradScaler.step()'s behaviour, misc.py:288-308: no optimizer step on Inf / NaN gradients), decided on the
 * device from the norm tulip_grad_norm / tulip_grad_clip wrote (norm[0], float32).  state = {applied, skipped_total,
 * skipped_consecutive}, three 64-bit device words; hyper = tulip_adamw's block.
 *   norm is NaN or +-Inf:  skipped_total += 1, skipped_consecutive += 1, skip_flag[0] = 1; applied and hyper stay
 *   otherwise:             applied += 1, skipped_consecutive = 0, skip_flag[0] = 0,
 *                          hyper[5] = (float)(1 - beta1^applied), hyper[6] = (float)(1 - beta2^applied)
 * with the power by binary exponentiation in float64 (r = 1, x = beta; while t: if t & 1: r *= x; t >>= 1; if t: x *= x), one
 * rounding per multiplication: no transcendental function, bit-identical to the host definition (tulip_amd/guard.py).
 * One workgroup, one working lane, plain stores; graph-capturable (a replayed graph advances the counters itself).  The launches
 * behind it (tulip_adamw_g, tulip_adamw_blocks_g, tulip_ema_update_g) read skip_flag.  A NULL pointer or a state that is not
 * 8-byte aligned: TULIP_ERR_ARG before any launch. */
int tulip_step_guard(const float* norm, uint64_t* state, uint32_t* skip_flag, float* hyper, double beta1, double beta2,
                     hipStream_t stream);

/* Range-image input transforms in one pass (util/datasets.py): ScaleTensor :138-142, FilterInvalidPixels
 * :144-151, DownsampleTensor :117-125, DownsampleTensorWidth :127-135, LogTransform :68-70,
 * RandomRollRangeMap :96-107, composed as build_{durlar,kitti,carla}_upsampling_dataset do (:244-340).
 * raw: B sensor images in metres, element type float32 (raw_dtype 0) or float16 (raw_dtype 1); pixel (i,j) of
 * image b is raw[b*batch_stride + base_offset + i*row_stride + j*col_stride] (strides in elements, may be
 * negative), so the (H,W,2) .npy payload is read in place with col_stride 2 (npy_loader :175-179 takes channel 0)
 * and the .rimg payload with row_stride -1, col_stride -s0, base_offset s0*s1-1 (rimg_loader :181-193:
 * transpose + flip).  hi (B,1,H,W) and/or lo (B,1,H/row_factor,W/col_factor); either may be NULL.
 *   v = raw*scale; if gate: v = (min_range<=v<=max_range) ? v : 0; if log_transform: v = log1p(v);
 *   hi[i][(j+roll)%W] = v;  lo[(i-row_phase)/row_factor][((j-col_phase)/col_factor+roll)%(W/col_factor)] = v
 *   for rows/columns with (i-row_phase)%row_factor==0, (j-col_phase)%col_factor==0. */
int tulip_range_prep(const void* raw, int raw_dtype, int64_t batch_stride, int64_t row_stride, int64_t col_stride,
                     int64_t base_offset, float* hi, float* lo, int B, int H, int W, int row_factor, int col_factor,
                     int row_phase, int col_phase, float scale, int gate, float min_range, float max_range,
                     int log_transform, int roll_shift, hipStream_t stream);

/* The same transforms with a per-sample augmentation drawn on the device from (seed, sample_ids[b]) and nothing else (host
 * definition: tulip_amd/augment.py).  Arguments up to log_transform as above (no roll_shift); sample_ids: B device int64 words,
 * read by the kernel, so a captured call replayed after the ids were rewritten in place draws for the new ids.
 *   mix64 = the splitmix64 finaliser of "Element dropout";  K = mix64(seed ^ 0x52414E4745415547 ^ mix64(id));  draw(n) = mix64(K + n)
 *   s    = ((draw(0) >> 32) * W) >> 32            in [0, W)            with TULIP_AUG_ROLL, else 0
 *   flip = draw(1) >> 63                                               with TULIP_AUG_FLIP, else 0
 *   p    = ((draw(2) >> 32) * row_factor) >> 32   in [0, row_factor)   with TULIP_AUG_ROW_PHASE, else row_phase
 *   beam il dropped      iff (draw(2^20 + il) >> 40) < beam_threshold            (thresholds: rint(p * 2^24), at most 2^24)
 *   point (il,jl) dropped iff (draw(2^32 + il*(W/col_factor) + jl) >> 40) < point_threshold
 * The scan is mirrored, then rotated, and the pair is taken from it afterwards: with v0(i,j) the value tulip_range_prep forms
 * for pixel (i,j) (the kernels share that expression: the outputs are bit for bit this gather of the plain outputs),
 * c = (j - s) mod W and src(j) = flip ? W-1-c : c,
 *   hi[i][j]   = v0(i, src(j))
 *   lo[il][jl] = dropped ? +0.0f : v0(p + row_factor*il, src(col_phase + col_factor*jl))          (the target is never dropped)
 * so any s is legal when the widths differ.  Every thread owns output pixels: stores are the plain call's aligned, coalesced
 * ones for every draw, reads stay along the source's unit-stride axis.  params_out (B,4) int32 {s, flip, p, 0} per sample, or NULL.
 * One launch, nothing allocated, no host state, graph-capturable.  TULIP_ERR_ARG before any launch: whatever tulip_range_prep
 * refuses, sample_ids NULL or not 8-byte aligned, flag bits other than the three below, a threshold above 2^24. */
#define TULIP_AUG_ROLL 1
#define TULIP_AUG_FLIP 2
#define TULIP_AUG_ROW_PHASE 4
int tulip_range_prep_aug(const void* raw, int raw_dtype, int64_t batch_stride, int64_t row_stride, int64_t col_stride,
                         int64_t base_offset, float* hi, float* lo, int B, int H, int W, int row_factor, int col_factor,
                         int row_phase, int col_phase, float scale, int gate, float min_range, float max_range,
                         int log_transform, const int64_t* sample_ids, uint64_t seed, int flags, uint32_t beam_threshold,
                         uint32_t point_threshold, int32_t* params_out, hipStream_t stream);

/* Multi-channel batches: the two calls above with trailing (C, chan_stride, chan_scale, chan_log), for raw images of C in 1..4
 * channels ([range, intensity, ...]; float32 only).  Channel c of pixel (i,j) of image b is raw[b*batch_stride + base_offset +
 * i*row_stride + j*col_stride + c*chan_stride]; hi (B,C,H,W) and/or lo (B,C,H/row_factor,W/col_factor), planes.  chan_scale:
 * HOST pointer to C-1 floats, the scale s_c of channels 1..C-1 (read during the call, passed to the kernel by value; may be NULL
 * at C == 1); chan_log bit c-1: log1p on channel c.  Host definition: tulip_amd/prep_channels.py.
 *   channel 0:  v0 = the value of tulip_range_prep (raw0*scale -> gate -> log1p if log_transform), and nothing else: bit for bit
 *               the single-channel output.
 *   hole:       the pixel is a hole iff raw0*scale after the gate, BEFORE the log, == 0.0f (true for -0.0, false for a NaN).
 *   channel c:  u = raw_c * s_c (one float32 multiply);  u = hole ? +0.0f : u  (a select: a NaN, infinite or negative raw_c in a
 *               hole gives +0.0f);  u = log1pf(u) if bit c-1 of chan_log.
 * Subsampling, phases and roll_shift (tulip_range_prep_c), and the rotation, mirror, start row and beam / point drops
 * (tulip_range_prep_aug_c; the draws do not depend on C) apply to every channel alike: output channel c of the augmented call is
 * bit for bit the gather of tulip_range_prep_aug's comment applied to plain channel c, a dropped low-res pixel is +0.0f in all C
 * channels, the target is never dropped.  The interleaved row-major payload (chan_stride 1, col_stride 2 or 4 >= C, the
 * alignment of the single-channel 16-byte kernels) is read once with 16-byte loads, a thread owning 4 output pixels of all C
 * planes; anything else goes through the LDS-tile form.  One launch each, nothing allocated, no host state, graph-capturable.
 * TULIP_ERR_ARG before any launch: whatever the call above refuses, raw_dtype != 0, C < 1, C > 4, chan_scale NULL at C > 1,
 * chan_log bits at or above C-1. */
int tulip_range_prep_c(const void* raw, int raw_dtype, int64_t batch_stride, int64_t row_stride, int64_t col_stride,
                       int64_t base_offset, float* hi, float* lo, int B, int H, int W, int row_factor, int col_factor,
                       int row_phase, int col_phase, float scale, int gate, float min_range, float max_range,
                       int log_transform, int roll_shift, hipStream_t stream, int C, int64_t chan_stride,
                       const float* chan_scale, uint32_t chan_log);
int tulip_range_prep_aug_c(const void* raw, int raw_dtype, int64_t batch_stride, int64_t row_stride, int64_t col_stride,
                           int64_t base_offset, float* hi, float* lo, int B, int H, int W, int row_factor, int col_factor,
                           int row_phase, int col_phase, float scale, int gate, float min_range, float max_range,
                           int log_transform, const int64_t* sample_ids, uint64_t seed, int flags, uint32_t beam_threshold,
                           uint32_t point_threshold, int32_t* params_out, hipStream_t stream, int C, int64_t chan_stride,
                           const float* chan_scale, uint32_t chan_log);

/* ---- evaluation post-processing and 3-D metrics (engine_upsampling.py:126-355,361-608; util/evaluation.py) ---- */

/* MC-dropout aggregate (engine_upsampling.py:421-426): preds (passes, n) -> out (n):
 * mean over the passes, zeroed where the unbiased std exceeds noise_threshold*mean. */
int tulip_mc_aggregate(const float* preds, int passes, int64_t n, float noise_threshold, float* out,
                       hipStream_t stream);

/* One image (engine_upsampling.py:176-251): pred/hi (H,W), lo (h,w) in the model's value space.
 * expm1 of all three when log_transform (:178-181); pred = (gate_min<=pred<=gate_max) ? pred : 0 (:183-190);
 * mae_out[0] = mean|pred-hi| (:192-193); when w==W: mae_out[1] = mean over rows 0::H/h of |pred-lo| (:226-228) and
 * those rows of pred are replaced by lo (:230), else mae_out[1] = 0 (:208-209); keep_close>0 zeroes pixels of both
 * images above it (:247-249).  pred_img/hi_img (H,W): the images the point clouds are made from.
 * partials: scratch of 2*1024 doubles. */
int tulip_eval_postprocess(const float* pred, const float* hi, const float* lo, float* pred_img, float* hi_img,
                           double* partials, float* mae_out, int H, int W, int h, int w, int log_transform,
                           float gate_min, float gate_max, float keep_close, hipStream_t stream);

/* ---- the two above for images of C = 2..4 channels ([range, intensity, ...] planes; the reference evaluates one channel only, so
 * the definition is this project's: tulip_amd/eval_channels.py is its host form) ----
 *
 * tulip_eval_postprocess_c: pred/hi (C,H,W), lo (C,h,w), pred_img/hi_img (C,H,W).  Channel 0 is tulip_eval_postprocess on the
 * channel-0 planes, expression for expression (its planes are bit-identical).  A pixel is a prediction hole iff channel 0 is
 * == 0.0f after the gate, before the rows are restored (true for -0.0f; a NaN fails the gate); a valid target pixel iff the
 * target's channel 0 is > 0 after the expm1 (false for a NaN).  Channel c >= 1: expm1 of pred, hi and lo when bit c-1 of
 * chan_log_bits is set (RangePrep(channel_log=...)); pred = hole ? +0.0f : pred (a select); sum|pred-hi| before the restore;
 * when w==W rows 0::H/h give sum|pred-lo| and are replaced by lo; keep_close>0: where the final channel 0 of an image exceeds
 * it, all C channels of that image's pixel become 0.  metrics (3*C+1 floats) = {mae[C], mae_low_res[C], mae_valid[C], n_valid}:
 * float64 sums, float32(sum * inv); mae_valid[c] = sum over the valid target pixels / n_valid (0 when there is none), taken
 * before the restore.  partials: scratch of (3*C+1)*1024 doubles.  One grid-stride launch and a single-block fold.
 *
 * tulip_mc_aggregate_c: preds (passes, C, n) -> out (C, n): per channel the float64 mean rounded to float32; the drop decision
 * is channel 0's (sd0 > noise_threshold*mean0, unbiased std) and zeroes the pixel in all C channels; out[0:n] is bit for bit
 * tulip_mc_aggregate of preds[:, 0].
 *
 * TULIP_ERR_ARG before any launch: what the single-channel calls refuse, C outside 2..4, w <= 0, chan_log_bits at or above bit
 * C-1. */
int tulip_mc_aggregate_c(const float* preds, int passes, int C, int64_t n, float noise_threshold, float* out,
                         hipStream_t stream);
int tulip_eval_postprocess_c(const float* pred, const float* hi, const float* lo, float* pred_img, float* hi_img,
                             double* partials, float* metrics, int H, int W, int h, int w, int C, int log_transform,
                             uint32_t chan_log_bits, float gate_min, float gate_max, float keep_close, hipStream_t stream);

/* Range image -> (H*W,3) float32 points, row-major pixel order (evaluation.py img_to_pcd_kitti :52-87 and
 * img_to_pcd_carla :90-116): r = img*max_range; x = (sin_h[j]*cos_v[i])*r; y = (cos_h[j]*cos_v[i])*r;
 * z = sin_v[i]*r, float32 products in that order (bit exact against numpy given the same tables). */
int tulip_range_to_xyz(const float* img, const float* sin_h, const float* cos_h, const float* sin_v,
                       const float* cos_v, float max_range, int H, int W, float* xyz, hipStream_t stream);

/* DurLAR / OS1-128 (evaluation.py img_to_pcd_durlar :21-50) -> (H*W,3) float64 points:
 * t = float32(img*max_range) - origin_offset (float32); col_tables = [cos(enc+az) | sin(enc+az) | o*cos(enc) |
 * o*sin(enc)] (4*W), row_tables = [cos(el) | sin(el)] (2*H); x = -((t*c0[u])*cos_el[v] + c2[u]),
 * y = -((t*c1[u])*cos_el[v] + c3[u]), z = t*sin_el[v] + z_offset, unfused float64; pixel (v,u) is written at
 * index v*W + (u + W - row_offset[v]) % W (idx_from_px :21-24). */
int tulip_range_to_xyz_durlar(const float* img, const double* col_tables, const double* row_tables,
                              const int32_t* row_offset, float max_range, float origin_offset, double z_offset, int H,
                              int W, double* xyz, hipStream_t stream);

/* ---- dense point clouds from a batch of predictions (csrc/cloud.hip; tulip_amd/cloud.py is the host definition) ----
 *
 * pred (B,C,H,W), lo (B,C,h,w), C = 1..4.  Per image: the prediction side of tulip_eval_postprocess (C = 1) /
 * tulip_eval_postprocess_c (C >= 2) without a target -- expm1, inclusive gate, rows 0::H/h restored from lo iff w == W,
 * keep_close -- then the projection of tulip_range_to_xyz / tulip_range_to_xyz_durlar (the float64 DurLAR point rounded once to
 * float32), and an ordered compaction that keeps the pixels whose final range is > 0.0f (false for -0.0f, +0.0f and a NaN).
 * Row order: the row order of the projection's output (row-major; DurLAR: the staggered index v*W + (u + W - row_offset[v]) % W)
 * with the other rows removed; images concatenated.  A row is (x, y, z, a_1 .. a_{C-1}), a_c = the final value of channel c.
 *
 * Outputs: rng (B,C,H,W) the post-processed planes in that row ("destination") order -- for the spherical sensors the planes
 * tulip_eval_postprocess(_c) writes to pred_img; counts (B*tiles int32, tiles = ceil(H*W / tulip_cloud_tile())) the kept slots of
 * every tile; tile_offsets (B*tiles int64) their exclusive scan; offsets (B+1 int64): image b owns rows offsets[b] ..
 * offsets[b+1]-1, offsets[0] = 0; points (capacity B*H*W rows of 3+C-1 floats): rows at or beyond offsets[B] are not written.
 * Three stream-ordered launches (post-process + count, scan by one block, write); no block waits for another.
 *
 * TULIP_ERR_ARG before any launch: a null pointer, C outside 1..4, B, H, W, h or w <= 0, B > 65535, H % h, chan_log_bits at or
 * above bit C-1. */
int tulip_cloud_tile(void);
int tulip_cloud_spherical(const float* pred, const float* lo, int B, int C, int H, int W, int h, int w, int log_transform,
                          uint32_t chan_log_bits, float gate_min, float gate_max, float keep_close, float max_range,
                          const float* sin_h, const float* cos_h, const float* sin_v, const float* cos_v, float* rng,
                          int32_t* counts, int64_t* tile_offsets, int64_t* offsets, float* points, hipStream_t stream);
int tulip_cloud_durlar(const float* pred, const float* lo, int B, int C, int H, int W, int h, int w, int log_transform,
                       uint32_t chan_log_bits, float gate_min, float gate_max, float keep_close, float max_range,
                       const double* col_tables, const double* row_tables, const int32_t* row_offset, float origin_offset,
                       double z_offset, float* rng, int32_t* counts, int64_t* tile_offsets, int64_t* offsets, float* points,
                       hipStream_t stream);

/* Voxel IoU / precision / recall / F1 of two clouds (engine_upsampling.py:254-271; evaluation.py
 * voxelize_point_cloud :148-160, calculate_metrics :162-175).  Points (n,3) float32 (is_f64=0) or float64; voxel
 * of p = ((p - min)/grid_size).astype(int) with min/max over BOTH clouds, evaluated in the clouds' own type.
 * The two occupancy grids are bitmaps of bitmap_words 32-bit words each, all zero on entry and on exit (cleared
 * again point by point); out = {iou, precision, recall, f1, dims0, dims1, dims2, status}; status 1 (metrics NaN)
 * when dims0*dims1*dims2 exceeds 32*bitmap_words.  scratch: 6*1024+16 doubles, zero before first use. */
int tulip_voxel_metrics(const void* pcd_pred, int64_t n_pred, const void* pcd_gt, int64_t n_gt, int is_f64,
                        double grid_size, uint32_t* bitmap_pred, uint32_t* bitmap_gt, int64_t bitmap_words,
                        double* scratch, double* out, hipStream_t stream);

/* Chamfer distance as the reference reduces it (evaluation.py:125-135): out[0] = mean(dist_a) + mean(dist_b),
 * dist_a[i] = min_j |a_i - b_j|^2 and dist_b[j] = min_i |b_j - a_i|^2 in float32 (float64 clouds are cast), the
 * semantics of the ChamferDistance CUDA extension the reference imports (not vendored there).
 * scratch: 2*1024 doubles. */
int tulip_chamfer_sq(const void* a, int64_t na, const void* b, int64_t nb, int is_f64, float* dist_a, float* dist_b,
                     double* scratch, double* out, hipStream_t stream);

/* KITTI point cloud -> range image, the producer of the .npy files the loaders read
 * (kitti_utils/sample_kitti_dataset.py create_range_map :24-66, parameters :139-145): points (n,4) float32
 * [x,y,z,intensity]; row = rint((atan2(z,sqrt(x^2+y^2))*180/pi + ang_start_y)/ang_res_y),
 * col = -trunc((atan2(x,y)*180/pi - 90)/ang_res_x) + cols/2 (wrapped once), all float32 in numpy's op order; a pixel
 * keeps the LAST point (in point order) that falls into it; range outside [min_range,max_range] -> 0, the
 * intensity of such a point is kept (as in the reference); out (rows,cols,2) float32 [range, intensity].
 * winner: scratch of rows*cols int32, all -1 on entry and on exit. */
int tulip_kitti_range_map(const float* points, int64_t n, int rows, int cols, float ang_start_y, float ang_res_y,
                          float ang_res_x, float max_range, float min_range, int32_t* winner, float* out,
                          hipStream_t stream);

/* Forward of one whole Swin block at embed width 96 (3 heads x 32, window 2x8, MLP 96->384->96) in ONE launch:
 * SwinTransformerBlock.forward (tulip.py:338-352) = norm1 -> WindowAttention.forward (:282-324, shifted when
 * shift_h/shift_w != 0, mask when `masked`) -> +DropPath residual -> norm2 -> Mlp.forward (:194-200) -> +residual.
 * Tokens (B,H,W,96) fp32, H even, W % 64 == 0.  Every tensor the backward reads is written exactly as the separate
 * kernels write it: xn1 [M][96] bf16, qkv [M][288] bf16, attn_out [M][96] bf16, x1 [M][96] fp32, xn2 [M][96] bf16,
 * fc1_pre / fc1_act [M][384] bf16, mean/rstd [M] fp32.  drop_scale_* : per-sample DropPath multipliers or NULL.
 * Inference form: ALL eleven saved-activation pointers (x1, xn1, qkv, attn_out, xn2, fc1_pre, fc1_act, mean1, rstd1, mean2,
 * rstd2) NULL -- only x_out (and the wide kernels' out_bf16) is written.  tulip_swin96_block_fwd only: qkv and fc1_pre
 * (both) NULL with the other nine given -- the lean training form for the recomputing backward (tulip_swin96_bwd_desc).
 * Any other mix of NULL and non-NULL is an argument error. */
typedef struct tulip_swin96_desc {
    const float* x_in; float* x1; float* x_out;
    void* xn1; void* qkv; void* attn_out; void* xn2; void* fc1_pre; void* fc1_act;
    float* mean1; float* rstd1; float* mean2; float* rstd2;
    const void* w_qkv; const void* w_proj; const void* w_fc1; const void* w_fc2;
    const float* b_qkv; const float* b_proj; const float* b_fc1; const float* b_fc2;
    const float* norm1_weight; const float* norm1_bias; const float* norm2_weight; const float* norm2_bias;
    const float* bias_table; const int32_t* rel_index; const float* drop_scale_attn; const float* drop_scale_mlp;
    int B; int H; int W; int shift_h; int shift_w; int masked; float eps;
} tulip_swin96_desc;
int tulip_swin96_block_fwd(const tulip_swin96_desc* d, hipStream_t stream);
/* diagnostic twins (tools/swin96_phases.py): stamps[(workgroup * 8 + wave) * 16 + k] = s_memtime (shader clock) at phase
 * boundary k of every wave; workgroups = tulip_swin96_bwd_partial_rows(B, H, W) */
int tulip_swin96_block_fwd_profiled(const tulip_swin96_desc* d, uint64_t* stamps, hipStream_t stream);
/* Two consecutive blocks of the stage (tulip.py:399-436: the un-shifted block d0, then the shifted block d1 on its output) in ONE
 * launch: a workgroup runs its tile of d0, publishes the 49-KB output tile (write-through stores + one flag per tile), waits for
 * the <= 4 tiles of d0 that its tile of d1 reads, and runs d1 -- no grid barrier; first-block tiles never wait.  d0->x_out must be
 * d1->x_in; B (H/2) (W/64) <= the number of CUs (one workgroup per tile, all resident; TULIP_ERR_ARG beyond); both descriptors in the same form (inference, or training with TULIP_BLOCK_FC1_GRAD); same tensors and bits as the
 * two launches.  sync: tulip_swin96_pair_sync_bytes(B, H, W) bytes, 16-byte aligned, ZERO before the first launch and owned by
 * these launches from then on (epoch-stamped flags: nothing to clear between launches or graph replays; words 2 / 3 are a test
 * hook that holds the tiles of one parity back, see csrc/swin96.hip; word 4 counts polls that gave up after ~0.5 s -- it stays 0 unless
 * a producer never ran, and the results of such a launch are undefined). */
int tulip_swin96_pair_sync_bytes(int B, int H, int W);
int tulip_swin96_pair_fwd(const tulip_swin96_desc* d0, const tulip_swin96_desc* d1, void* sync, size_t sync_bytes,
                          hipStream_t stream);

/* Backward of the same block in ONE launch (replaces, for C = 96, the chain tulip_gemm_bf16(EPI_GELU_BWD) ->
 * tulip_gemm_bf16 -> tulip_layernorm_bwd -> tulip_gemm_bf16 -> tulip_window_attn_bwd -> tulip_gemm_bf16 ->
 * tulip_layernorm_bwd; autograd of tulip.py:338-352).  dx holds d(block output) on entry and d(block input) on
 * return.  The kernel also writes the bf16 operands of the four weight-gradient GEMMs -- d_out_mlp = bf16(dx*s_mlp)
 * [M][96], d_fc1_pre [M][384], d_out_attn = bf16(d(x1)*s_attn) [M][96], d_qkv [M][288] -- and ONE partial row per
 * workgroup (tulip_swin96_bwd_partial_rows of them) for each of: norm1 / norm2 affine gradients ([rows][192] =
 * d(weight) | d(bias), folded by tulip_reduce_rows2) and the dense relative-position-bias gradient ([rows][3*256],
 * folded and scattered by tulip_reduce_rows_multi).  dx_bf16 (optional): bf16(dx * dx_bf16_scale[sample]). */
typedef struct tulip_swin96_bwd_desc {
    float* dx; const float* x_in; const float* x1;
    const void* qkv; const void* fc1_pre;
    const float* mean1; const float* rstd1; const float* mean2; const float* rstd2;
    const void* w_qkv; const void* w_proj; const void* w_fc1; const void* w_fc2;
    const float* norm1_weight; const float* norm2_weight;
    const float* bias_table; const int32_t* rel_index; const float* drop_scale_attn; const float* drop_scale_mlp;
    void* d_out_mlp; void* d_fc1_pre; void* d_out_attn; void* d_qkv;
    void* dx_bf16; const float* dx_bf16_scale;
    float* norm1_partials; float* norm2_partials; float* bias_partials;
    int B; int H; int W; int shift_h; int shift_w; int masked;
    /* Recomputation form (C = 96 only, round 4): qkv == NULL and fc1_pre == NULL -- the forward was launched without them
     * (tulip_swin96_block_fwd with qkv = fc1_pre = NULL writes 2.1 instead of 3.5 KB per token) and the backward recomputes
     * both from x_in / x1, the saved statistics and the weights it holds in LDS anyway, with the forward's own operand
     * fragments and accumulation order (the forward's bits).  Needs the four bias vectors the forward added; ignored (may be
     * NULL) when qkv / fc1_pre are given.  tulip_swinw_block_bwd does not read them. */
    const float* b_qkv; const float* b_fc1; const float* norm1_bias; const float* norm2_bias;
} tulip_swin96_bwd_desc;
int tulip_swin96_bwd_partial_rows(int B, int H, int W);
int tulip_swin96_block_bwd(const tulip_swin96_bwd_desc* d, hipStream_t stream);
int tulip_swin96_block_bwd_profiled(const tulip_swin96_bwd_desc* d, uint64_t* stamps, hipStream_t stream);

/* The same two launches for the wider stages, C = 192 and C = 384 (heads of 32, window 2x8, MLP C -> 4C -> C; H even,
 * W % 16 == 0; tulip_swinw_supported): a workgroup owns 2 or 4 neighbouring windows with one wave per head, every GEMM
 * of the block is split along its output channels across the waves, weights stream from L2 straight into MFMA
 * operand registers, activations pass through LDS (csrc/swinw.hip).  Descriptors, saved tensors and partial rows are
 * those of the C = 96 entry points with 96 -> C, 288 -> 3C, 384 -> 4C, 3*256 -> (C/32)*256 and partial rows of
 * [d(weight)[C] | d(bias)[C]].  out_bf16 (optional): bf16 copy of the block output [M][C].
 * WEIGHTS are read in fragment-major ("packed") order, written by tulip_pack_bf16_multi: the 16 x 32 block (rows 16 nt..,
 * columns 32 ks..) of a [N][K] matrix is the 1-KiB block nt*K/32 + ks, and inside it element (n, k) sits at
 * ((n%16) + 16*((k%32)/8))*8 + k%8 -- one MFMA A operand = one contiguous 1-KiB wave load (4x the L2 -> register rate
 * of row-major fragments on this chip).  Forward: w_qkv / w_proj / w_fc1 / w_fc2 = packed copies of the weights as
 * they are ([3C][C], [C][C], [4C][C], [C][4C]); backward: packed copies of their TRANSPOSES (item.transpose = 1).
 * rows % 16 == 0 and cols % 32 == 0 of the matrix being packed (after the transpose, if any); up to TULIP_PACK_MAX
 * matrices per launch. */
#define TULIP_PACK_MAX 64
typedef struct tulip_pack_item { const void* src; void* dst; int rows; int cols; int transpose; } tulip_pack_item;
int tulip_swinw_supported(int C, int H, int W);
int tulip_swinw_block_fwd(const tulip_swin96_desc* d, int C, void* out_bf16, hipStream_t stream);
/* diagnostic twin of tulip_swinw_block_fwd: stamps[(workgroup * waves + wave) * 16 + k] = s_memtime (shader clock) at
 * phase boundary k of every wave (waves = C/32; workgroups = tulip_swinw_bwd_partial_rows); tools/swinw_phases.py */
int tulip_swinw_block_fwd_profiled(const tulip_swin96_desc* d, int C, void* out_bf16, uint64_t* stamps,
                                   hipStream_t stream);
/* Split form of the forward (round 4; C = 384 where a workgroup owns ONE window, i.e. few windows: batch 8 at stage 2 is 128
 * workgroups on 256 CUs, each streaming the block's 3.5 MB of weights): two workgroups per window.  Both run the attention
 * half, each takes half of the MLP's hidden channels; the two fc2 partial sums meet in `exchange` (tulip_swinw_split_bytes
 * bytes, 16-byte aligned, zero before the first launch, left zeroed; its last 4 bytes per window are arrival tickets): the
 * last-arriving workgroup of a pair adds its partner's partial and writes the block output, nobody waits.  Same arguments,
 * tensors and results (the fc2 sum is formed as two halves: last-bit differences) as tulip_swinw_block_fwd in its training
 * form with TULIP_BLOCK_FC1_GRAD or in its inference form; stamps optional (the profiled twin).  tulip_swinw_split_bytes returns 0 where the form
 * does not exist (then call tulip_swinw_block_fwd). */
int tulip_swinw_split_bytes(int C, int B, int H, int W);
int tulip_swinw_block_fwd_split(const tulip_swin96_desc* d, int C, void* out_bf16, void* exchange, size_t exchange_bytes,
                                uint64_t* stamps, hipStream_t stream);
int tulip_swinw_bwd_partial_rows(int C, int B, int H, int W);
/* Launches of at most 256 workgroups (the whole grid resident at once) start by spreading the block's weights over the
 * L2 of each XCD (every wave touches a few KiB nobody else touches): in a training step the weights are cold, and the
 * per-wave streams would otherwise run at miss latency (tools/cold_probe.py).  TULIP_BLOCK_NO_WARM in d->masked switches
 * that off for one launch.  (tulip_gemm_bf16 has the same first touch of its weight panel: TULIP_GEMM_NO_TOUCH.) */
int tulip_swinw_block_bwd(const tulip_swin96_bwd_desc* d, int C, hipStream_t stream);
/* split form of the backward (see tulip_swinw_block_fwd_split; the same exchange buffer may serve both directions of a block):
 * the MLP half's hidden channels are halved between the two workgroups of a window, the partial sums of d(norm2 output) meet in
 * `exchange`, the last arriver runs norm2' .. norm1' alone.  Needs TULIP_BLOCK_FC1_GRAD in d->masked.  Partial rows: one per
 * WINDOW, tulip_swinw_bwd_partial_rows as for tulip_swinw_block_bwd. */
int tulip_swinw_block_bwd_split(const tulip_swin96_bwd_desc* d, int C, void* exchange, size_t exchange_bytes, hipStream_t stream);
int tulip_pack_bf16_multi(const tulip_pack_item* items, int n, hipStream_t stream);

/* The same block at the DEEP widths, C = 768 (stage 3) and C = 1536 (stage 4 of tulip_large) -- replaces, per direction, the 15 / 16
 * launch sequence tulip_layernorm_fwd -> tulip_gemm_bf16 -> tulip_window_attn_fwd -> ... of tulip.py:338-352 -- as a chain of SLICED
 * launches (csrc/swind.hip): eight workgroups per group of 1-2 windows, workgroup (group, slice) on XCD `slice`, every CU streaming
 * one eighth of a fragment-major weight matrix; the slicing alternates between heads / hidden channels and output channels, so no
 * launch holds a partial sum.  Window wh x ww = 2 x 8 or the 1 x 16 backup window (tulip.py:284-287).  Descriptors, saved tensors and
 * weight copies (fragment-major; backward: of the transposes) are those of tulip_swinw_block_fwd / _bwd.
 * Forward, `phases` bits: 1 norm1 + qkv + attention (by heads) -> attn_out; 2 proj + residual (by output channels) -> x1;
 * 4 norm2 + fc1 + GELU (by hidden channels) -> fc1_act; 8 fc2 + residual -> x_out (+ out_bf16).  The training form needs
 * TULIP_BLOCK_FC1_GRAD in d->masked (the fc1_pre buffer carries gelu'(h)); the inference form is xn1, qkv, xn2, fc1_pre and the
 * four statistics NULL -- attn_out, x1 and fc1_act pass from launch to launch and must always be given.
 * Backward, `phases` bits: 1 fc2' + GELU' (by hidden channels): d->dx (read only) -> d_out_mlp, d_fc1_pre; 2 fc1' -> d_norm_out =
 * fp32 d(norm2 output) [M][C]; the caller then runs tulip_layernorm_bwd_splitk(d_norm_out, 1, x1, mean2, rstd2, ...) (norm2',
 * residual, d_out_attn); 4 proj' + attention' (by heads): d_out_attn -> d_qkv, bias_partials [tulip_swind_groups][heads * 256];
 * 8 qkv' -> d_norm_out = fp32 d(norm1 output); the caller runs tulip_layernorm_bwd_splitk again (norm1', residual).  The
 * descriptor's norm partials, dx_bf16, x_in, x1 and statistics fields are not read by these launches.
 * stamps (optional): s_memtime per wave at the phase boundaries, [launch 0..3][workgroup][wave][16]. */
int tulip_swind_supported(int C, int H, int W, int wh, int ww);
int tulip_swind_groups(int C, int B, int H, int W, int wh, int ww);
int tulip_swind_block_fwd(const tulip_swin96_desc* d, int C, int wh, int ww, void* out_bf16, int phases, uint64_t* stamps,
                          hipStream_t stream);
int tulip_swind_block_bwd(const tulip_swin96_bwd_desc* d, int C, int wh, int ww, float* d_norm_out, int phases, uint64_t* stamps,
                          hipStream_t stream);

/* ---- the stage boundaries of the U-Net as ONE launch each (csrc/glue.hip, round 6) -------------------------------------
 * A workgroup owns a block of 16 / 32 rows for the whole boundary: the row block's activations sit in LDS as the MFMA B operand,
 * the weights stream from their FRAGMENT-MAJOR copies (tulip_pack_bf16_multi: `*_packed` = the matrix as it is, `*_t_packed` =
 * its transpose), and what the launch sequences below pass through HBM passes through LDS.  bf16 rounding points are those of
 * the sequences they replace (every GEMM operand bf16, every accumulator fp32, LayerNorm in fp32): results agree with them to
 * fp32 summation order.  Every *_supported() is 0 where the form does not exist; the caller then issues the sequence. */

/* PatchMerging.forward (tulip.py:101-106) = tulip_layernorm_fwd(merge = 1) + tulip_gemm_bf16(TULIP_EPI_F32): x (B,H,W,Cin) fp32
 * -> 2x2 gather -> LayerNorm(4 Cin) -> xm bf16 [rows][4 Cin], mean, rstd [rows] (saved for the backward) -> y fp32 [rows][2 Cin]
 * = xm . W^T (no bias); y_bf16 (optional, row pitch ld_bf16 elements): bf16 copy of y (x_save half of the next level's skip
 * concat, tulip.py:715).  rows = B H/2 W/2.  Cin in {96, 192, 384}, rows % 32 == 0. */
typedef struct tulip_merge_fwd_desc {
    const float* x; const float* gamma; const float* beta;
    const void* w_packed;          /* reduction.weight [2 Cin][4 Cin], fragment-major */
    void* xm; float* mean; float* rstd; float* y;
    void* y_bf16; int ld_bf16;
    int B, H, W, Cin; float eps;
} tulip_merge_fwd_desc;
int tulip_merge_fwd_supported(int Cin, int B, int H, int W);
int tulip_merge_fwd(const tulip_merge_fwd_desc* d, hipStream_t stream);

/* Backward of the same boundary (autograd of tulip.py:101-106, and of the x_save half of tulip.py:715 in front of it) =
 * [tulip_gemm_bf16(dy_skip . W_skip[:, Cs:], TULIP_EPI_F32 accumulate + bf16 copy)] + tulip_gemm_bf16(dyb . W_red, TULIP_EPI_BF16)
 * + tulip_layernorm_bwd(merge = 1).  (B,H,W,Cp) is the FINER stage (the LayerNorm's input x_prev), Cs = 2 Cp, rows = B H/2 W/2.
 * dy_skip != NULL: dyb = bf16(dx_in + dy_skip . W_skip[:, Cs:2Cs]) is formed and WRITTEN (operand of the reduction's weight
 * gradient; w_skip_t_packed = packed W_skip^T, a [2 Cs][Cs] matrix); dy_skip == NULL: dyb is READ (the bottleneck stage: no skip).
 * dx_prev (B,H,W,Cp) fp32 is overwritten with the LayerNorm backward's result scattered through the gather; dx_bf16 (optional) =
 * bf16(dx_prev * cast_rowscale[token / cast_rows_per_sample]); param_partials: tulip_merge_bwd_partial_rows() rows of
 * [dgamma[4 Cp] | dbeta[4 Cp]] (fold with tulip_reduce_rows_multi).  Cp in {96, 192}, rows % 32 == 0. */
typedef struct tulip_merge_bwd_desc {
    const float* dx_in; const void* dy_skip; const void* w_skip_t_packed;
    void* dyb;
    const void* w_red_t_packed;    /* packed reduction.weight^T: a [4 Cp][2 Cp] matrix */
    const float* x_prev; const float* mean; const float* rstd; const float* gamma;
    float* dx_prev; float* param_partials;
    void* dx_bf16; const float* cast_rowscale; int cast_rows_per_sample;
    int B, H, W, Cp;
} tulip_merge_bwd_desc;
int tulip_merge_bwd_supported(int Cp, int B, int H, int W);
int tulip_merge_bwd_partial_rows(int Cp, int B, int H, int W);
int tulip_merge_bwd(const tulip_merge_bwd_desc* d, hipStream_t stream);

/* PatchUnmerging.forward -> skip Linear(cat[...]) (tulip.py:117-123, :713-716) = tulip_gemm_bf16(TULIP_EPI_PIXSHUF2_F32) +
 * tulip_gemm_bf16(TULIP_EPI_F32).  x_bf16 [M][C], M = B H W coarse tokens; cat bf16 [4M][C] (fine-token order): its first half
 * [:, :C/2] = bf16(PixelShuffle(2)(x . We^T + be)) is WRITTEN (operand of the skip weight gradient), its second half (x_save)
 * is READ; out fp32 [4M][C/2] = cat . Ws^T + bs.  C in {192, 384}, M % 16 == 0. */
typedef struct tulip_unmerge_skip_desc {
    const void* x_bf16;
    const void* w_expand_packed; const float* b_expand;     /* expand.weight [2C][C] fragment-major, bias [2C] */
    void* cat;
    const void* w_skip_packed; const float* b_skip;         /* skip weight [C/2][C] fragment-major, bias [C/2] */
    float* out;
    int B, H, W, C;
} tulip_unmerge_skip_desc;
int tulip_unmerge_skip_supported(int C, int B, int H, int W);
int tulip_unmerge_skip_fwd(const tulip_unmerge_skip_desc* d, hipStream_t stream);

/* Its backward along the unmerged stream = tulip_gemm_bf16(dy_skip . W_skip[:, :C/2], TULIP_EPI_UNSHUF2_BF16) +
 * tulip_gemm_bf16(dz . We, TULIP_EPI_F32 + bf16 copy): dy_skip bf16 [4M][C/2]; dz bf16 [M][2C] is WRITTEN (operand of the expand
 * weight / bias gradient); dx fp32 [M][C] overwritten; dx_bf16 (optional) = bf16(dx * cast_rowscale[m / cast_rows_per_sample]).
 * w_skip_t_packed = packed W_skip^T ([C][C/2], rows 0 .. C/2-1 used), w_expand_t_packed = packed We^T ([C][2C]). */
typedef struct tulip_skip_unmerge_bwd_desc {
    const void* dy_skip; const void* w_skip_t_packed;
    void* dz;
    const void* w_expand_t_packed;
    float* dx; void* dx_bf16; const float* cast_rowscale; int cast_rows_per_sample;
    int B, H, W, C;
} tulip_skip_unmerge_bwd_desc;
int tulip_skip_unmerge_bwd(const tulip_skip_unmerge_bwd_desc* d, hipStream_t stream);

/* library self-description */
/* diagnostics: *dst = the 100 MHz constant device clock (s_memrealtime) when the stream reaches this point; capturable
 * (tools/step_stamps.py time-lines a captured training step with it, no tracer attached) */
int tulip_stamp_realtime(uint64_t* dst, hipStream_t stream);
/* Layout version of the structs and signatures in this header (round 3: tulip_wgrad_item, tulip_reduce_region and tulip_adamw_ref grew
 * fields, entry points were added): a caller built against another version must not bind. */
#define TULIP_ABI_VERSION 6
int tulip_abi_version(void);
const char* tulip_build_arch(void);
int tulip_dev_variants(void);      /* 1: the development build (see the conventions at the top) */

#ifdef __cplusplus
}
#endif
#endif /* TULIP_HIP_H_ */

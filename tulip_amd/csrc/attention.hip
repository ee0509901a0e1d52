// Shifted-window attention core for 16-token windows (2x8, or the 1x16 backup window), forward and
// backward, and for 32- / 64-token windows (section "32- and 64-token windows" below).   gfx950 only.
//
// One wave owns one (window, head) pair at a time.  Cyclic shift, window partition and their
// inverses (tulip.py:289-290, 248-252, 320-323) are pure address arithmetic: the 16 token rows of a
// window are gathered from / scattered to their natural (b,h,w) positions in the [B*H*W][3C] qkv
// tensor, so no roll / permute copies exist.
//
// A 16x16 score tile with head_dim 32 is exactly one v_mfma_f32_16x16x32_bf16 (head_dim 16: upper
// k-half zero).  The MFMA is issued as K.Q^T so lane l holds S[query=l&15][key=4*(l>>4)+r]: the
// row softmax is 4 in-lane values + two cross-lane steps (xor 16, 32), and the probabilities are
// already the B operand of the 16x16x16 P.V MFMA.  V / K / Q / dO tiles that must be consumed
// "token-major" go through a 1 KiB per-wave LDS tile and ds_read_b64_tr_b16 (LDS transpose read).
#include "common.h"
#include "tulip_hip.h"

namespace {

struct AttnGeom {
    int B, H, W, C, nh;
    int wh, ww, sh, sw, masked, fp8;
    int nWy, nWx;
    float scale;
};

__device__ __forceinline__ int region(int x, int X, int wsz, int ssz) {
    // create_mask slices (tulip.py:261-266): [0:-wsz]=0, [-wsz:-ssz]=1, [-ssz:]=2; later wins, and
    // ssz==0 makes the last slice [0:] (Python -0) cover everything.
    return (ssz == 0 || x >= X - ssz) ? 2 : (x >= X - wsz ? 1 : 0);
}

__device__ __forceinline__ void slot_info(const AttnGeom& g, int b, int wy, int wx, int s, int& row, int& label) {
    const int i = fast_div(s, g.ww), j = s - i * g.ww;
    const int hs = wy * g.wh + i, ws = wx * g.ww + j;  // coordinates in the rolled image
    int h = hs + g.sh; if (h >= g.H) h -= g.H;         // rolled[hs] = x[(hs+sh) mod H]
    int w = ws + g.sw; if (w >= g.W) w -= g.W;
    row = (b * g.H + h) * g.W + w;
    label = 3 * region(hs, g.H, g.wh, g.sh) + region(ws, g.W, g.ww, g.sw);
}

// ds_read_b64_tr_b16 through the builtin: the compiler batches the waits of consecutive reads
__device__ __forceinline__ bf16x4 tr_read(const unsigned char* p) {
    typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4_t;
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4_t*)p);
}

__device__ __forceinline__ bf16x4 pack4(float a, float b, float c, float d) {
    typedef __attribute__((ext_vector_type(2))) uint32_t u32x2_t;
    return __builtin_bit_cast(bf16x4, (u32x2_t){pack_bf16x2(a, b), pack_bf16x2(c, d)});
}

__device__ __forceinline__ void store4(bf16_t* p, f32x4 v, float s) {
    *(uint2*)p = make_uint2(pack_bf16x2(v[0] * s, v[1] * s), pack_bf16x2(v[2] * s, v[3] * s));
}

// wave -> (head, window group); every wave keeps one head so d(bias) accumulates in registers
struct WaveMap {
    int h, grp, ngrp;
};
__device__ __forceinline__ WaveMap wave_map(int nh, int ngrp) {
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
    WaveMap m;
    m.h = wave % nh; m.grp = wave / nh; m.ngrp = ngrp;
    return m;
}

// DROP: attn_drop on the probabilities (tulip.py:315), mask element ((window * nh + head) * 16 + query) * 16 + key of the
// counter-based mask (include/tulip_hip.h, "Element dropout"); DROP = false is the kernel the step runs without it.
template <int P, bool DROP = false>
__global__ __launch_bounds__(256, 2) void attn_fwd_kernel(const bf16_t* __restrict__ qkv,
                                                       const float* __restrict__ bias_table,
                                                       const int* __restrict__ rel_index, bf16_t* __restrict__ out,
                                                       AttnGeom g, int ngrp, DropoutArg da = DropoutArg{}) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * 16 * P * 2];
    const int lane = threadIdx.x & 63, li = lane & 15, gq = lane >> 4;
    unsigned char* ldsV = smem + (threadIdx.x >> 6) * (16 * P * 2);
    const WaveMap wm = wave_map(g.nh, ngrp);
    if (wm.grp >= ngrp) return;
    const int h = wm.h;
    const int nW = g.nWy * g.nWx, total = g.B * nW;
    const bool dvalid = gq * 8 < P;
    const int C3 = 3 * g.C;

    float bias[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bias[r] = bias_table[rel_index[li * 16 + gq * 4 + r] * g.nh + h];

    uint64_t dkey = 0;
    uint32_t dthr = 0;
    float dscale = 0.f;
    if constexpr (DROP) { dkey = dropout_key(da); dthr = dropout_thr(da.p); dscale = dropout_inv_keep(da.p); }

    for (int win = wm.grp; win < total; win += ngrp) {
        const int b = fast_div(win, nW), wloc = win - b * nW;
        const int wy = fast_div(wloc, g.nWx), wx = wloc - wy * g.nWx;
        int row, lab;
        slot_info(g, b, wy, wx, li, row, lab);
        const bf16_t* src = qkv + (size_t)row * C3 + h * P + gq * 8;
        bf16x8 q = {0, 0, 0, 0, 0, 0, 0, 0}, k = q, v = q;
        if (dvalid) {
            q = *(const bf16x8*)src;
            k = *(const bf16x8*)(src + g.C);
            v = *(const bf16x8*)(src + 2 * g.C);
            *(bf16x8*)(ldsV + li * (P * 2) + gq * 16) = v;
        }
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        if (g.fp8) s = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(bf16x8_to_fp8(k), bf16x8_to_fp8(q), s, 0, 0, 0);
        else s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k, q, s, 0, 0, 0);  // s[r] = q_li . k_(4gq+r)
        float mx = -3.0e38f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float x = s[r] * g.scale + bias[r];
            if (g.masked) {
                const int kl = __shfl(lab, gq * 4 + r, 64);
                if (kl != lab) x += -100.0f;
            }
            s[r] = x;
            mx = fmaxf(mx, x);
        }
        mx = rows_max(mx);
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) { s[r] = __expf(s[r] - mx); sum += s[r]; }
        sum = rows_sum(sum);
        const float inv = __builtin_amdgcn_rcpf(sum);
        if constexpr (DROP) {           // lane (query li, key 4gq+r)
            const uint64_t base = ((uint64_t)win * g.nh + h) * 256 + li * 16 + gq * 4;
#pragma unroll
            for (int r = 0; r < 4; ++r) s[r] *= dropout_mul(dkey, base + r, dthr, dscale);
        }
        const bf16x4 pb = pack4(s[0] * inv, s[1] * inv, s[2] * inv, s[3] * inv);
        bf16_t* dst = out + (size_t)row * g.C + h * P + gq * 4;
#pragma unroll
        for (int dc = 0; dc < P / 16; ++dc) {
            const bf16x4 vt = tr_read(ldsV + (gq * 4 + (li >> 2)) * (P * 2) + dc * 32 + (li & 3) * 8);
            f32x4 o = {0.f, 0.f, 0.f, 0.f};
            o = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(vt, pb, o, 0, 0, 0);  // o[r] = O[li][16dc+4gq+r]
            store4(dst + dc * 16, o, 1.0f);
        }
    }
}

// DROP: the backward of attn_drop -- dV from the dropped probabilities, dP = (dO.V^T) * mask * scale ahead of the softmax
// backward, whose row term sum_key P * dP then equals rowsum(dO * O) of the dropped forward.
template <int P, bool DROP = false>
__global__ __launch_bounds__(256, 2) void attn_bwd_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                       const float* __restrict__ bias_table,
                                                       const int* __restrict__ rel_index, bf16_t* __restrict__ dqkv,
                                                       float* dbias_part, AttnGeom g, int ngrp, DropoutArg da = DropoutArg{}) {
    // All 4 waves of a workgroup serve the SAME head (blockIdx.x % nh), so d(bias) is summed over the
    // workgroup in LDS and leaves as one plain 256-float partial row per workgroup:
    // dbias_part[blockIdx.x][i*16+j].  Rows of one head are nh apart -> viewed as [gridDim.x/nh][nh*256]
    // the partials fold into the dense [nh][16][16] gradient with a single row reduction.
    constexpr int TILE = 16 * P * 2;
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * 3 * TILE];
    __shared__ float red[4][256];
    const int lane = threadIdx.x & 63, li = lane & 15, gq = lane >> 4, wid = threadIdx.x >> 6;
    unsigned char* ldsQ = smem + wid * (3 * TILE);
    unsigned char* ldsK = ldsQ + TILE;
    unsigned char* ldsD = ldsK + TILE;
    const int h = blockIdx.x % g.nh;
    WaveMap wm;
    wm.h = h; wm.grp = (blockIdx.x / g.nh) * 4 + wid; wm.ngrp = ngrp;
    const int nW = g.nWy * g.nWx, total = g.B * nW;
    const bool dvalid = gq * 8 < P;
    const int C3 = 3 * g.C;

    float bias_q[4], bias_k[4];  // Lq: (query li, key 4gq+r)   Lk: (query 4gq+r, key li)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        bias_q[r] = bias_table[rel_index[li * 16 + gq * 4 + r] * g.nh + h];
        bias_k[r] = bias_table[rel_index[(gq * 4 + r) * 16 + li] * g.nh + h];
    }
    float dbacc[4] = {0.f, 0.f, 0.f, 0.f};
    uint64_t dkey = 0;
    uint32_t dthr = 0;
    float dscale = 0.f;
    if constexpr (DROP) { dkey = dropout_key(da); dthr = dropout_thr(da.p); dscale = dropout_inv_keep(da.p); }

    for (int win = wm.grp; win < total; win += ngrp) {
        const int b = fast_div(win, nW), wloc = win - b * nW;
        const int wy = fast_div(wloc, g.nWx), wx = wloc - wy * g.nWx;
        int row, lab;
        slot_info(g, b, wy, wx, li, row, lab);
        const bf16_t* src = qkv + (size_t)row * C3 + h * P + gq * 8;
        bf16x8 q = {0, 0, 0, 0, 0, 0, 0, 0}, k = q, v = q, d = q;
        if (dvalid) {
            q = *(const bf16x8*)src;
            k = *(const bf16x8*)(src + g.C);
            v = *(const bf16x8*)(src + 2 * g.C);
            d = *(const bf16x8*)(dout + (size_t)row * g.C + h * P + gq * 8);
            if (g.fp8) { q = round_through_fp8(q); k = round_through_fp8(k); }     // the values the forward's scores saw
            const int off = li * (P * 2) + gq * 16;
            *(bf16x8*)(ldsQ + off) = q;
            *(bf16x8*)(ldsK + off) = k;
            *(bf16x8*)(ldsD + off) = d;
        }
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        f32x4 sq = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k, q, z, 0, 0, 0);   // Lq: S[li][4gq+r]
        f32x4 sk = __builtin_amdgcn_mfma_f32_16x16x32_bf16(q, k, z, 0, 0, 0);   // Lk: S[4gq+r][li]
        f32x4 dpq = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v, d, z, 0, 0, 0);  // Lq: dP[li][4gq+r] = dO_li . V_key
        f32x4 dpk = __builtin_amdgcn_mfma_f32_16x16x32_bf16(d, v, z, 0, 0, 0);  // Lk: dP[4gq+r][li]
        float mk[4] = {1.f, 1.f, 1.f, 1.f};
        if constexpr (DROP) {
            const uint64_t base = ((uint64_t)win * g.nh + h) * 256;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                dpq[r] *= dropout_mul(dkey, base + li * 16 + gq * 4 + r, dthr, dscale);     // Lq: (query li, key 4gq+r)
                mk[r] = dropout_mul(dkey, base + (gq * 4 + r) * 16 + li, dthr, dscale);    // Lk: (query 4gq+r, key li)
                dpk[r] *= mk[r];
            }
        }

        float mx = -3.0e38f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ol = __shfl(lab, gq * 4 + r, 64);
            float xq = sq[r] * g.scale + bias_q[r];
            float xk = sk[r] * g.scale + bias_k[r];
            if (g.masked && ol != lab) { xq += -100.0f; xk += -100.0f; }
            sq[r] = xq; sk[r] = xk;
            mx = fmaxf(mx, xq);
        }
        mx = rows_max(mx);
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) sum += __expf(sq[r] - mx);
        sum = rows_sum(sum);
        const float lse = mx + __logf(sum);  // for query li
        float pq[4], pk[4], delta = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            pq[r] = __expf(sq[r] - lse);
            pk[r] = __expf(sk[r] - __shfl(lse, gq * 4 + r, 64));
            delta += pq[r] * dpq[r];
        }
        delta = rows_sum(delta);  // sum_key P*dP for query li
        float dsq[4], dsk[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            dsq[r] = pq[r] * (dpq[r] - delta);
            dsk[r] = pk[r] * (dpk[r] - __shfl(delta, gq * 4 + r, 64));
            dbacc[r] += dsq[r];
        }
        const bf16x4 dsq_b = pack4(dsq[0], dsq[1], dsq[2], dsq[3]);
        const bf16x4 dsk_b = pack4(dsk[0], dsk[1], dsk[2], dsk[3]);
        const bf16x4 pk_b = DROP ? pack4(pk[0] * mk[0], pk[1] * mk[1], pk[2] * mk[2], pk[3] * mk[3])
                                 : pack4(pk[0], pk[1], pk[2], pk[3]);
        bf16_t* dst = dqkv + (size_t)row * C3 + h * P + gq * 4;
        const int troff = (gq * 4 + (li >> 2)) * (P * 2) + (li & 3) * 8;
#pragma unroll
        for (int dc = 0; dc < P / 16; ++dc) {
            const bf16x4 kt = tr_read(ldsK + troff + dc * 32);  // K[4gq+jj][16dc+li]
            const bf16x4 qt = tr_read(ldsQ + troff + dc * 32);  // Q[4gq+jj][16dc+li]
            const bf16x4 dt = tr_read(ldsD + troff + dc * 32);  // dO[4gq+jj][16dc+li]
            // dQ[li][d] = scale * sum_key dS[li][key] K[key][d]
            f32x4 dq = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(kt, dsq_b, z, 0, 0, 0);
            // dK[li][d] = scale * sum_q dS[q][li] Q[q][d]
            f32x4 dk = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(qt, dsk_b, z, 0, 0, 0);
            // dV[li][d] = sum_q P[q][li] dO[q][d]
            f32x4 dv = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(dt, pk_b, z, 0, 0, 0);
            store4(dst + dc * 16, dq, g.scale);
            store4(dst + g.C + dc * 16, dk, g.scale);
            store4(dst + 2 * g.C + dc * 16, dv, 1.0f);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wid][li * 16 + gq * 4 + r] = dbacc[r];
    __syncthreads();
    dbias_part[(size_t)blockIdx.x * 256 + threadIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// ---------------------------------------------------------------- 32- and 64-token windows
// (4x8, 2x16, 8x8, 4x16, 2x32 and the (1, L) backup windows).  A workgroup is one wave and serves one head; its 64 lanes are
// 64 / L windows of that head side by side, lane = token slot in its window.  The K / V rows (backward: Q, K, V, dO) of those
// windows are staged in LDS as bf16 and read back as broadcasts; a lane keeps the L scores of its row in registers, so the
// softmax is in-lane.  Scores, P.V and the gradients are fp32 FMA; P is rounded to bf16 ahead of P.V as the 16-token kernel
// rounds its MFMA operand.  The (query, key) bias of the head sits in LDS with a padded row (L + 1 floats: conflict-free
// by row and by column).  Same semantics as above: q.scale + bias + 0/-100 shift mask, softmax, (attn_drop,) P.V, window
// reverse / reverse shift as addressing.
template <int P>
__device__ __forceinline__ void load_row(const bf16_t* p, float (&x)[P]) {
#pragma unroll
    for (int c = 0; c < P / 8; ++c) {
        const bf16x8 v = *(const bf16x8*)(p + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) x[c * 8 + e] = bf2f((bf16_t)v[e]);
    }
}

template <int P>
__device__ __forceinline__ void copy_row(unsigned char* lds, const bf16_t* p) {
#pragma unroll
    for (int c = 0; c < P / 8; ++c) *(bf16x8*)(lds + c * 16) = *(const bf16x8*)(p + c * 8);
}

template <int P>
__device__ __forceinline__ float dot_lds(const float (&x)[P], const unsigned char* row) {
    float a = 0.f;
#pragma unroll
    for (int c = 0; c < P / 8; ++c) {
        const bf16x8 v = *(const bf16x8*)(row + c * 16);
#pragma unroll
        for (int e = 0; e < 8; ++e) a = fmaf(x[c * 8 + e], bf2f((bf16_t)v[e]), a);
    }
    return a;
}

template <int P>
__device__ __forceinline__ void axpy_lds(float (&y)[P], float s, const unsigned char* row) {
#pragma unroll
    for (int c = 0; c < P / 8; ++c) {
        const bf16x8 v = *(const bf16x8*)(row + c * 16);
#pragma unroll
        for (int e = 0; e < 8; ++e) y[c * 8 + e] = fmaf(s, bf2f((bf16_t)v[e]), y[c * 8 + e]);
    }
}

template <int P>
__device__ __forceinline__ void store_row(bf16_t* p, const float (&x)[P], float s) {
#pragma unroll
    for (int c = 0; c < P / 8; ++c)
        *(uint4*)(p + c * 8) = make_uint4(pack_bf16x2(x[c * 8] * s, x[c * 8 + 1] * s), pack_bf16x2(x[c * 8 + 2] * s, x[c * 8 + 3] * s),
                                          pack_bf16x2(x[c * 8 + 4] * s, x[c * 8 + 5] * s), pack_bf16x2(x[c * 8 + 6] * s, x[c * 8 + 7] * s));
}

__device__ __forceinline__ float round_bf16(float x) { return bf2f(f2bf(x)); }

// the head's [L][L] bias (query i, key j) -> LDS rows of L + 1 floats
template <int L>
__device__ __forceinline__ void stage_bias(float* sbias, const float* bias_table, const int* rel_index, int nh, int h) {
    for (int e = threadIdx.x; e < L * L; e += 64) {
        const int i = e / L, j = e - i * L;
        sbias[i * (L + 1) + j] = bias_table[rel_index[e] * nh + h];
    }
}

// workgroup = (head blockIdx.x % nh, group blockIdx.x / nh); group grp takes windows grp * IT + item, stepping ngrp * IT.
// The score / probability row of each lane lives in LDS (srow: [64][L + 1] fp32, conflict-free both ways), so the loops over
// keys are not unrolled into registers.  DROP: mask element ((window * nh + head) * L + query) * L + key.
template <int L, int P, bool DROP = false>
__global__ __launch_bounds__(64) void attn_fwd_wide_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ bias_table,
                                                           const int* __restrict__ rel_index, bf16_t* __restrict__ out,
                                                           AttnGeom g, int ngrp, DropoutArg da = DropoutArg{}) {
    constexpr int IT = 64 / L, LP = L + 1, ROW = P * 2;
    __shared__ __attribute__((aligned(16))) unsigned char ldsK[64 * ROW];
    __shared__ __attribute__((aligned(16))) unsigned char ldsV[64 * ROW];
    __shared__ float sbias[L * LP];
    __shared__ float srow[64 * LP];
    __shared__ int slab[64];
    const int lane = threadIdx.x, s = lane % L, item = lane / L;
    const int h = blockIdx.x % g.nh, grp = blockIdx.x / g.nh;
    const int nW = g.nWy * g.nWx, total = g.B * nW;
    const int C3 = 3 * g.C;
    stage_bias<L>(sbias, bias_table, rel_index, g.nh, h);
    const unsigned char* Kw = ldsK + item * L * ROW;
    const unsigned char* Vw = ldsV + item * L * ROW;
    const float* brow = sbias + s * LP;
    const int* lw = slab + item * L;
    float* sr = srow + lane * LP;
    uint64_t dkey = 0;
    uint32_t dthr = 0;
    float dscale = 0.f;
    if constexpr (DROP) { dkey = dropout_key(da); dthr = dropout_thr(da.p); dscale = dropout_inv_keep(da.p); }

    for (int base = grp * IT; base < total; base += ngrp * IT) {    // wave-uniform trip count
        const int win = base + item;
        const bool valid = win < total;
        int row = 0, lab = 0;
        float q[P];
#pragma unroll
        for (int d = 0; d < P; ++d) q[d] = 0.f;
        if (valid) {
            const int b = fast_div(win, nW), wloc = win - b * nW;
            const int wy = fast_div(wloc, g.nWx), wx = wloc - wy * g.nWx;
            slot_info(g, b, wy, wx, s, row, lab);
            const bf16_t* src = qkv + (size_t)row * C3 + h * P;
            load_row<P>(src, q);
            copy_row<P>(ldsK + lane * ROW, src + g.C);
            copy_row<P>(ldsV + lane * ROW, src + 2 * g.C);
        }
        slab[lane] = lab;
        __syncthreads();
        float mx = -3.0e38f;
#pragma unroll 2
        for (int k = 0; k < L; ++k) {
            float x = dot_lds<P>(q, Kw + k * ROW) * g.scale + brow[k];
            if (g.masked && lw[k] != lab) x += -100.0f;
            sr[k] = x;
            mx = fmaxf(mx, x);
        }
        float sum = 0.f;
#pragma unroll 4
        for (int k = 0; k < L; ++k) { const float e = __expf(sr[k] - mx); sr[k] = e; sum += e; }
        const float inv = __builtin_amdgcn_rcpf(sum);
        const uint64_t mb = (((uint64_t)win * g.nh + h) * L + s) * L;
        float o[P];
#pragma unroll
        for (int d = 0; d < P; ++d) o[d] = 0.f;
#pragma unroll 2
        for (int k = 0; k < L; ++k) {
            float e = sr[k];
            if constexpr (DROP) e *= dropout_mul(dkey, mb + k, dthr, dscale);
            axpy_lds<P>(o, round_bf16(e * inv), Vw + k * ROW);
        }
        if (valid) store_row<P>(out + (size_t)row * g.C + h * P, o, 1.0f);
        __syncthreads();                                            // the rows are restaged for the next windows
    }
}

// Backward, two phases per group of windows.  Phase A, lane = query: P from the recomputed scores, the row term
// delta = sum_key P * dP with dP = (dO . V) * mask, summed as the 16-token kernel sums it (the algebraically equal dO . O
// cancels across channels: its rounding error is not bounded by sum_key P |dP|, and a row whose dP are all 0 did not get 0),
// dS = P (dP - delta) and dQ = scale dS.K; dS and the (dropped) P, rounded to bf16 as the forward rounds it ahead of P.V (and
// as the 16-token kernel rounds its dV operand), stay in LDS ([item][query][key]).  Phase B, lane = key:
// dK = scale dS^T.Q and dV = P^T.dO.  d(bias) leaves as one [L*L] partial row per workgroup, dbias_part[blockIdx.x][i*L+j]
// (rows of one head nh apart): the workgroup owns its row and adds the dS of every trip to it (plain load / store, the
// first trip stores; every group has at least one trip, wide_groups).
template <int L, int P, bool DROP = false>
__global__ __launch_bounds__(64) void attn_bwd_wide_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                           const float* __restrict__ bias_table,
                                                           const int* __restrict__ rel_index, bf16_t* __restrict__ dqkv,
                                                           float* __restrict__ dbias_part, AttnGeom g, int ngrp,
                                                           DropoutArg da = DropoutArg{}) {
    constexpr int IT = 64 / L, LP = L + 1, ROW = P * 2;
    __shared__ __attribute__((aligned(16))) unsigned char ldsQ[64 * ROW];
    __shared__ __attribute__((aligned(16))) unsigned char ldsK[64 * ROW];
    __shared__ __attribute__((aligned(16))) unsigned char ldsV[64 * ROW];
    __shared__ __attribute__((aligned(16))) unsigned char ldsD[64 * ROW];
    __shared__ float sbias[L * LP];
    __shared__ float sds[64 * LP];          // lane (item, query) row: scores, then P, then dS
    __shared__ float spm[64 * LP];          // P, dropped
    __shared__ int slab[64];
    const int lane = threadIdx.x, s = lane % L, item = lane / L;
    const int h = blockIdx.x % g.nh, grp = blockIdx.x / g.nh;
    const int nW = g.nWy * g.nWx, total = g.B * nW;
    const int C3 = 3 * g.C;
    stage_bias<L>(sbias, bias_table, rel_index, g.nh, h);
    const unsigned char* Qw = ldsQ + item * L * ROW;
    const unsigned char* Kw = ldsK + item * L * ROW;
    const unsigned char* Vw = ldsV + item * L * ROW;
    const unsigned char* Dw = ldsD + item * L * ROW;
    const float* brow = sbias + s * LP;
    const int* lw = slab + item * L;
    float* dsr = sds + lane * LP;
    float* pmr = spm + lane * LP;
    const float* dsc = sds + item * L * LP + s;     // column s of the item's rows (phase B)
    const float* pmc = spm + item * L * LP + s;
    float* dpart = dbias_part + (size_t)blockIdx.x * (L * L) + s;
    uint64_t dkey = 0;
    uint32_t dthr = 0;
    float dscale = 0.f;
    if constexpr (DROP) { dkey = dropout_key(da); dthr = dropout_thr(da.p); dscale = dropout_inv_keep(da.p); }

    for (int base = grp * IT; base < total; base += ngrp * IT) {    // wave-uniform trip count
        const int win = base + item;
        const bool valid = win < total;
        int row = 0, lab = 0;
        float x[P], dor[P];
#pragma unroll
        for (int d = 0; d < P; ++d) { x[d] = 0.f; dor[d] = 0.f; }
        if (valid) {
            const int b = fast_div(win, nW), wloc = win - b * nW;
            const int wy = fast_div(wloc, g.nWx), wx = wloc - wy * g.nWx;
            slot_info(g, b, wy, wx, s, row, lab);
            const bf16_t* src = qkv + (size_t)row * C3 + h * P;
            const bf16_t* dsrc = dout + (size_t)row * g.C + h * P;
            load_row<P>(src, x);
            load_row<P>(dsrc, dor);
            copy_row<P>(ldsQ + lane * ROW, src);
            copy_row<P>(ldsK + lane * ROW, src + g.C);
            copy_row<P>(ldsV + lane * ROW, src + 2 * g.C);
            copy_row<P>(ldsD + lane * ROW, dsrc);
        }
        slab[lane] = lab;
        __syncthreads();
        // ---- phase A: lane = query s
        float mx = -3.0e38f;
#pragma unroll 2
        for (int k = 0; k < L; ++k) {
            float v = dot_lds<P>(x, Kw + k * ROW) * g.scale + brow[k];
            if (g.masked && lw[k] != lab) v += -100.0f;
            dsr[k] = v;
            mx = fmaxf(mx, v);
        }
        float sum = 0.f;
#pragma unroll 4
        for (int k = 0; k < L; ++k) sum += __expf(dsr[k] - mx);
        const float lse = mx + __logf(sum);
        const uint64_t mb = (((uint64_t)win * g.nh + h) * L + s) * L;
        float delta = 0.f;
#pragma unroll 2
        for (int k = 0; k < L; ++k) {
            const float p = __expf(dsr[k] - lse);
            float pm = p;
            if constexpr (DROP) pm *= dropout_mul(dkey, mb + k, dthr, dscale);
            dsr[k] = p;
            pmr[k] = valid ? round_bf16(pm) : 0.f;                  // dV takes the P the forward's P.V took
            delta = fmaf(pm, dot_lds<P>(dor, Vw + k * ROW), delta);
        }
#pragma unroll
        for (int d = 0; d < P; ++d) x[d] = 0.f;                     // x: dQ from here
#pragma unroll 2
        for (int k = 0; k < L; ++k) {
            float dp = dot_lds<P>(dor, Vw + k * ROW);
            if constexpr (DROP) dp *= dropout_mul(dkey, mb + k, dthr, dscale);
            const float ds = dsr[k] * (dp - delta);
            dsr[k] = valid ? ds : 0.f;
            axpy_lds<P>(x, ds, Kw + k * ROW);
        }
        if (valid) store_row<P>(dqkv + (size_t)row * C3 + h * P, x, g.scale);
        __syncthreads();
        // ---- phase B: lane = key s
        float dk[P], dv[P];
#pragma unroll
        for (int d = 0; d < P; ++d) { dk[d] = 0.f; dv[d] = 0.f; }
#pragma unroll 2
        for (int i = 0; i < L; ++i) {
            axpy_lds<P>(dk, dsc[i * LP], Qw + i * ROW);
            axpy_lds<P>(dv, pmc[i * LP], Dw + i * ROW);
        }
        if (valid) {
            bf16_t* dst = dqkv + (size_t)row * C3 + h * P;
            store_row<P>(dst + g.C, dk, g.scale);
            store_row<P>(dst + 2 * g.C, dv, 1.0f);
        }
        if (item == 0) {                                            // d(bias): the column s of every item, in item order
            const bool first = base == grp * IT;
#pragma unroll 4
            for (int i = 0; i < L; ++i) {
                float a = dsc[i * LP];
                if constexpr (IT == 2) a += dsc[(L + i) * LP];
                dpart[i * L] = first ? a : dpart[i * L] + a;
            }
        }
        __syncthreads();                                            // the rows are restaged for the next windows
    }
}

bool make_geom(AttnGeom& g, int B, int H, int W, int C, int nh, int wh, int ww, int sh, int sw, int masked) {
    const int L = wh * ww;
    if ((L != 16 && L != 32 && L != 64) || nh <= 0 || C % nh) return false;
    if (L != 16 && (masked & TULIP_ATTN_FP8)) return false;        // fp8 scores: 16-token windows only
    const int P = C / nh;
    if (P != 16 && P != 32) return false;
    if (H % wh || W % ww || sh >= H + (sh == 0) || sw >= W + (sw == 0)) return false;
    g.B = B; g.H = H; g.W = W; g.C = C; g.nh = nh; g.wh = wh; g.ww = ww; g.sh = sh; g.sw = sw;
    g.masked = masked & TULIP_ATTN_MASKED; g.fp8 = (masked & TULIP_ATTN_FP8) ? 1 : 0;
    g.nWy = H / wh; g.nWx = W / ww;
    g.scale = 1.0f / sqrtf((float)P);
    return true;
}

int pick_groups(const AttnGeom& g) {
    const int total = g.B * g.nWy * g.nWx;
    int ngrp = (256 * 16 + g.nh - 1) / g.nh;  // ~16 waves per CU
    if (ngrp > total) ngrp = total;
    if (ngrp < 1) ngrp = 1;
    return ngrp;
}


// 32 / 64-token windows: workgroups per head (one wave each, 64 / L windows per trip).  The forward fills ~8 waves per CU;
// the backward's groups are its d(bias) partial rows: R <= max(1, 512 / nh) per head, so the partial buffer
// R * nh * L * L floats stays under 2 MiB (L = 32) / 8 MiB (L = 64) for nh <= 512.
int wide_groups(int total, int L, int nh, int cap_waves) {
    const int need = (total + 64 / L - 1) / (64 / L);
    int ngrp = cap_waves / nh;
    if (ngrp > need) ngrp = need;
    return ngrp < 1 ? 1 : ngrp;
}
int wide_fwd_groups(const AttnGeom& g) { return wide_groups(g.B * g.nWy * g.nWx, g.wh * g.ww, g.nh, 2048); }
int wide_bwd_groups(int total, int L, int nh) { return wide_groups(total, L, nh, 512); }

template <bool DROP>
void launch_fwd_wide(const AttnGeom& g, const uint16_t* qkv, const float* bias_table, const int32_t* rel_index, uint16_t* out,
                     DropoutArg da, hipStream_t stream) {
    const int ngrp = wide_fwd_groups(g);
    const dim3 grid(ngrp * g.nh), block(64);
    const int L = g.wh * g.ww, P = g.C / g.nh;
#define TULIP_FWD_WIDE(LL, PP) \
    hipLaunchKernelGGL((attn_fwd_wide_kernel<LL, PP, DROP>), grid, block, 0, stream, qkv, bias_table, rel_index, out, g, ngrp, da)
    if (L == 32) { if (P == 32) TULIP_FWD_WIDE(32, 32); else TULIP_FWD_WIDE(32, 16); }
    else         { if (P == 32) TULIP_FWD_WIDE(64, 32); else TULIP_FWD_WIDE(64, 16); }
#undef TULIP_FWD_WIDE
}

template <bool DROP>
void launch_bwd_wide(const AttnGeom& g, const uint16_t* qkv, const uint16_t* dout, const float* bias_table,
                     const int32_t* rel_index, uint16_t* dqkv, float* dbias_partials, DropoutArg da, hipStream_t stream) {
    const int L = g.wh * g.ww, P = g.C / g.nh;
    const int ngrp = wide_bwd_groups(g.B * g.nWy * g.nWx, L, g.nh);
    const dim3 grid(ngrp * g.nh), block(64);
#define TULIP_BWD_WIDE(LL, PP)                                                                                            \
    hipLaunchKernelGGL((attn_bwd_wide_kernel<LL, PP, DROP>), grid, block, 0, stream, qkv, dout, bias_table, rel_index, dqkv, \
                       dbias_partials, g, ngrp, da)
    if (L == 32) { if (P == 32) TULIP_BWD_WIDE(32, 32); else TULIP_BWD_WIDE(32, 16); }
    else         { if (P == 32) TULIP_BWD_WIDE(64, 32); else TULIP_BWD_WIDE(64, 16); }
#undef TULIP_BWD_WIDE
}

}  // namespace

extern "C" int tulip_window_attn_fwd(const uint16_t* qkv, const float* bias_table, const int32_t* rel_index,
                                     uint16_t* out, int B, int H, int W, int C, int nh, int wh, int ww, int sh, int sw,
                                     int masked, hipStream_t stream) {
    AttnGeom g;
    if (!make_geom(g, B, H, W, C, nh, wh, ww, sh, sw, masked)) return TULIP_ERR_ARG;
    if (B <= 0) return TULIP_OK;
    if (wh * ww != 16) {
        launch_fwd_wide<false>(g, qkv, bias_table, rel_index, out, DropoutArg{}, stream);
        TULIP_CHECK_LAUNCH();
        return TULIP_OK;
    }
    const int ngrp = pick_groups(g);
    const int blocks = (ngrp * nh + 3) / 4;
    if (C / nh == 32)
        hipLaunchKernelGGL(attn_fwd_kernel<32>, dim3(blocks), dim3(256), 0, stream, qkv, bias_table, rel_index, out, g,
                           ngrp);
    else
        hipLaunchKernelGGL(attn_fwd_kernel<16>, dim3(blocks), dim3(256), 0, stream, qkv, bias_table, rel_index, out, g,
                           ngrp);
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

// workgroups per head of the backward launch (each emits one 256-float d(bias) partial row)
static int bwd_blocks_per_head(int windows_total, int nh) {
    int ngrp = (256 * 8 + nh - 1) / nh;  // ~8 waves per CU
    if (ngrp > windows_total) ngrp = windows_total;
    if (ngrp < 1) ngrp = 1;
    return (ngrp + 3) / 4;
}

extern "C" int tulip_window_attn_bwd_partial_rows(int B, int H, int W, int nh, int wh, int ww) {
    if (B <= 0 || nh <= 0 || wh <= 0 || ww <= 0) return 0;
    if (wh * ww == 32 || wh * ww == 64) return wide_bwd_groups(B * (H / wh) * (W / ww), wh * ww, nh);
    return bwd_blocks_per_head(B * (H / wh) * (W / ww), nh);
}

extern "C" int tulip_window_attn_bwd(const uint16_t* qkv, const uint16_t* dout, const float* bias_table,
                                     const int32_t* rel_index, uint16_t* dqkv, float* dbias_partials, int B, int H,
                                     int W, int C, int nh, int wh, int ww, int sh, int sw, int masked,
                                     hipStream_t stream) {
    AttnGeom g;
    if (!make_geom(g, B, H, W, C, nh, wh, ww, sh, sw, masked)) return TULIP_ERR_ARG;
    if (B <= 0) return TULIP_OK;
    if (wh * ww != 16) {
        launch_bwd_wide<false>(g, qkv, dout, bias_table, rel_index, dqkv, dbias_partials, DropoutArg{}, stream);
        TULIP_CHECK_LAUNCH();
        return TULIP_OK;
    }
    const int bph = bwd_blocks_per_head(g.B * g.nWy * g.nWx, nh);
    const int blocks = bph * nh, ngrp = bph * 4;
    if (C / nh == 32)
        hipLaunchKernelGGL(attn_bwd_kernel<32>, dim3(blocks), dim3(256), 0, stream, qkv, dout, bias_table, rel_index,
                           dqkv, dbias_partials, g, ngrp);
    else
        hipLaunchKernelGGL(attn_bwd_kernel<16>, dim3(blocks), dim3(256), 0, stream, qkv, dout, bias_table, rel_index,
                           dqkv, dbias_partials, g, ngrp);
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

extern "C" int tulip_window_attn_fwd_drop(const uint16_t* qkv, const float* bias_table, const int32_t* rel_index,
                                          uint16_t* out, int B, int H, int W, int C, int nh, int wh, int ww, int sh, int sw,
                                          int masked, const uint64_t* key_ptr, uint64_t seed, int site, float p,
                                          hipStream_t stream) {
    AttnGeom g;
    if (!make_geom(g, B, H, W, C, nh, wh, ww, sh, sw, masked)) return TULIP_ERR_ARG;
    if (g.fp8 || !key_ptr || !(p >= 0.0f && p < 1.0f)) return TULIP_ERR_ARG;      // attn_drop with fp8 scores: not built
    if (B <= 0) return TULIP_OK;
    const DropoutArg da{(const unsigned long long*)key_ptr, (unsigned long long)seed, site, p};
    if (wh * ww != 16) {
        launch_fwd_wide<true>(g, qkv, bias_table, rel_index, out, da, stream);
        TULIP_CHECK_LAUNCH();
        return TULIP_OK;
    }
    const int ngrp = pick_groups(g);
    const int blocks = (ngrp * nh + 3) / 4;
    if (C / nh == 32)
        hipLaunchKernelGGL((attn_fwd_kernel<32, true>), dim3(blocks), dim3(256), 0, stream, qkv, bias_table, rel_index, out, g,
                           ngrp, da);
    else
        hipLaunchKernelGGL((attn_fwd_kernel<16, true>), dim3(blocks), dim3(256), 0, stream, qkv, bias_table, rel_index, out, g,
                           ngrp, da);
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

extern "C" int tulip_window_attn_bwd_drop(const uint16_t* qkv, const uint16_t* dout, const float* bias_table,
                                          const int32_t* rel_index, uint16_t* dqkv, float* dbias_partials, int B, int H,
                                          int W, int C, int nh, int wh, int ww, int sh, int sw, int masked,
                                          const uint64_t* key_ptr, uint64_t seed, int site, float p, hipStream_t stream) {
    AttnGeom g;
    if (!make_geom(g, B, H, W, C, nh, wh, ww, sh, sw, masked)) return TULIP_ERR_ARG;
    if (g.fp8 || !key_ptr || !(p >= 0.0f && p < 1.0f)) return TULIP_ERR_ARG;
    if (B <= 0) return TULIP_OK;
    const DropoutArg da{(const unsigned long long*)key_ptr, (unsigned long long)seed, site, p};
    if (wh * ww != 16) {
        launch_bwd_wide<true>(g, qkv, dout, bias_table, rel_index, dqkv, dbias_partials, da, stream);
        TULIP_CHECK_LAUNCH();
        return TULIP_OK;
    }
    const int bph = bwd_blocks_per_head(g.B * g.nWy * g.nWx, nh);
    const int blocks = bph * nh, ngrp = bph * 4;
    if (C / nh == 32)
        hipLaunchKernelGGL((attn_bwd_kernel<32, true>), dim3(blocks), dim3(256), 0, stream, qkv, dout, bias_table, rel_index,
                           dqkv, dbias_partials, g, ngrp, da);
    else
        hipLaunchKernelGGL((attn_bwd_kernel<16, true>), dim3(blocks), dim3(256), 0, stream, qkv, dout, bias_table, rel_index,
                           dqkv, dbias_partials, g, ngrp, da);
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

// Range-image input transforms as one pass (util/datasets.py:68-70,96-151,175-193,244-340):
// raw sensor image (metres; float32 or float16, any element strides so the interleaved (H,W,2) .npy payload
// and the transposed+flipped .rimg payload are read in place) -> high-res target (B,1,H,W) and low-res input
// (B,1,H/f,W/fw): x*scale -> range gate -> row/column subsample -> log1p -> roll along W.
// HBM-bound byte work: every raw element is read once, every output written once, tiles go through LDS so
// that both the read (along the source's unit-stride axis) and the write (along W) are coalesced.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "common.h"
#include "tulip_hip.h"

namespace {

constexpr int TI = 32, TJ = 64;

struct PrepArgs {
    int64_t sb, si, sj, base;      // element strides of the raw image and offset of pixel (0,0)
    float* hi;
    float* lo;
    int H, W, f, fw, rp, cp;
    float scale, gmin, gmax;
    int gate, logt, shift_hi, shift_lo, along_i;
};

template <typename T>
__device__ __forceinline__ float raw_to_float(T v);
template <>
__device__ __forceinline__ float raw_to_float<float>(float v) { return v; }
template <>
__device__ __forceinline__ float raw_to_float<__half>(__half v) { return __half2float(v); }

// The value of one pixel; every kernel of this file, plain or augmented, forms it with this one expression, so an
// augmented output is bit for bit a gather of the plain one.
// (prep_gated is that expression before its log: the multi-channel kernels call a pixel a hole where it is zero)
__device__ __forceinline__ float prep_gated(float raw, const PrepArgs& a) {
    float v = raw * a.scale;                                                                // ScaleTensor
    if (a.gate) v = (v >= a.gmin && v <= a.gmax) ? v : 0.f;                                 // FilterInvalidPixels
    return v;
}
__device__ __forceinline__ float prep_value(float raw, const PrepArgs& a) {
    float v = prep_gated(raw, a);
    if (a.logt) v = log1pf(v);                                                              // LogTransform
    return v;
}

template <typename T>
__global__ __launch_bounds__(256) void range_prep_kernel(const T* __restrict__ raw, PrepArgs a) {
    __shared__ float tile[TI][TJ + 1];
    const int b = blockIdx.z, i0 = blockIdx.y * TI, j0 = blockIdx.x * TJ, t = threadIdx.x;
    const T* src = raw + (int64_t)b * a.sb + a.base;
#pragma unroll
    for (int k = 0; k < TI * TJ / 256; ++k) {
        // fast thread index along the source's unit-stride axis
        const int ii = a.along_i ? (t & (TI - 1)) : (t / TJ + k * (256 / TJ));
        const int jj = a.along_i ? (t / TI + k * (256 / TI)) : (t & (TJ - 1));
        const int i = i0 + ii, j = j0 + jj;
        float v = 0.f;
        const bool need = a.hi || ((i - a.rp) % a.f == 0);
        if (i < a.H && j < a.W && need) {
            v = prep_value(raw_to_float<T>(src[(int64_t)i * a.si + (int64_t)j * a.sj]), a);
        }
        tile[ii][jj] = v;
    }
    __syncthreads();
    const int Hl = a.H / a.f, Wl = a.W / a.fw;
#pragma unroll
    for (int k = 0; k < TI * TJ / 256; ++k) {
        const int ii = t / TJ + k * (256 / TJ), jj = t & (TJ - 1);
        const int i = i0 + ii, j = j0 + jj;
        if (i >= a.H || j >= a.W) continue;
        const float v = tile[ii][jj];
        if (a.hi) {
            int jo = j + a.shift_hi;                                                        // torch.roll along W
            if (jo >= a.W) jo -= a.W;
            a.hi[((int64_t)b * a.H + i) * a.W + jo] = v;
        }
        if (a.lo && i >= a.rp && j >= a.cp && (i - a.rp) % a.f == 0 && (j - a.cp) % a.fw == 0) {
            const int il = (i - a.rp) / a.f;
            int jl = (j - a.cp) / a.fw + a.shift_lo;
            if (jl >= Wl) jl -= Wl;
            if (il < Hl) a.lo[((int64_t)b * Hl + il) * Wl + jl] = v;
        }
    }
}

// Row-major float32 sources (plain (B,H,W) or the interleaved (B,H,W,2) .npy payload): no transpose needed, so
// each thread takes 4 consecutive pixels of one row: 16-byte loads, 16-byte stores when the roll keeps alignment.
template <int SJ>
__global__ __launch_bounds__(256) void range_prep_rows_kernel(const float* __restrict__ raw, PrepArgs a) {
    const int W4 = a.W >> 2;
    const int64_t n4 = (int64_t)a.H * W4;
    const int b = blockIdx.y;
    const int Hl = a.H / a.f, Wl = a.W / a.fw;
    const float* src = raw + (int64_t)b * a.sb;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n4; k += (int64_t)gridDim.x * 256) {
        const int i = (int)(k / W4), j = (int)(k - (int64_t)i * W4) * 4;
        const bool lo_row = a.lo && i >= a.rp && (i - a.rp) % a.f == 0;
        if (!a.hi && !lo_row) continue;
        float v[4];
        const float* p = src + (int64_t)i * a.si + (int64_t)j * SJ;
        if (SJ == 1) {
            const float4 q = *(const float4*)p;
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            const float4 q0 = *(const float4*)p, q1 = *(const float4*)(p + 4);
            v[0] = q0.x; v[1] = q0.z; v[2] = q1.x; v[3] = q1.z;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = prep_value(v[c], a);
        if (a.hi) {
            float* dst = a.hi + ((int64_t)b * a.H + i) * a.W;
            int jo = j + a.shift_hi;
            if (jo >= a.W) jo -= a.W;
            if ((a.shift_hi & 3) == 0) {
                *(float4*)(dst + jo) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) { dst[jo] = v[c]; if (++jo == a.W) jo = 0; }
            }
        }
        if (lo_row) {
            float* dst = a.lo + ((int64_t)b * Hl + (i - a.rp) / a.f) * Wl;
            if (a.fw == 1 && (a.shift_lo & 3) == 0) {
                int jl = j + a.shift_lo;
                if (jl >= Wl) jl -= Wl;
                *(float4*)(dst + jl) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int jj = j + c;
                    if (jj >= a.cp && (jj - a.cp) % a.fw == 0) {
                        int jl = (jj - a.cp) / a.fw + a.shift_lo;
                        if (jl >= Wl) jl -= Wl;
                        dst[jl] = v[c];
                    }
                }
            }
        }
    }
}

// ---- per-sample augmentation (tulip_range_prep_aug; host definition tulip_amd/augment.py) -------------------------------
// Gather formulation: a thread owns OUTPUT pixels, so every store is the plain kernels' aligned, coalesced one whatever the
// sample drew; the rotation and the mirror only move where the (read-only, cache-served) source is read.  All draws come from
// (seed, sample_ids[b]) with the counter-based generator of the dropout masks: key = mix64(seed ^ DOMAIN ^ mix64(id)),
// draw(n) = mix64(key + n).
struct AugArgs {
    const long long* ids;
    unsigned long long seed;
    int flags;
    uint32_t beam_thr, point_thr;
    int32_t* params;
};
struct AugDraw {
    uint64_t key;
    int s, flip, p;
};
constexpr uint64_t AUG_DOMAIN = 0x52414E4745415547ull, AUG_BEAM = 1ull << 20, AUG_POINT = 1ull << 32;

__device__ __forceinline__ AugDraw aug_draw(const AugArgs& g, int b, const PrepArgs& a) {
    AugDraw d;
    d.key = drop_mix64(g.seed ^ AUG_DOMAIN ^ drop_mix64((uint64_t)g.ids[b]));
    d.s = (g.flags & TULIP_AUG_ROLL) ? (int)(((drop_mix64(d.key) >> 32) * (uint64_t)a.W) >> 32) : 0;
    d.flip = (g.flags & TULIP_AUG_FLIP) ? (int)(drop_mix64(d.key + 1) >> 63) : 0;
    d.p = (g.flags & TULIP_AUG_ROW_PHASE) ? (int)(((drop_mix64(d.key + 2) >> 32) * (uint64_t)a.f) >> 32) : a.rp;
    return d;
}
__device__ __forceinline__ void aug_write_params(const AugArgs& g, const AugDraw& d, int b) {
    int32_t* q = g.params + (int64_t)b * 4;
    q[0] = d.s; q[1] = d.flip; q[2] = d.p; q[3] = 0;
}
// the source column of output column j: the scan is mirrored, then rotated by s
__device__ __forceinline__ int aug_src(int j, const AugDraw& d, int W) {
    int c = j - d.s;
    if (c < 0) c += W;
    return d.flip ? W - 1 - c : c;
}
__device__ __forceinline__ bool aug_dropped(uint64_t key, uint64_t n, uint32_t thr) {
    return thr && (uint32_t)(drop_mix64(key + n) >> 40) < thr;
}

template <typename T>
__global__ __launch_bounds__(256) void range_prep_aug_kernel(const T* __restrict__ raw, PrepArgs a, AugArgs g) {
    __shared__ float tile[TI][TJ + 1];
    const int b = blockIdx.z, i0 = blockIdx.y * TI, j0 = blockIdx.x * TJ, t = threadIdx.x;
    const AugDraw d = aug_draw(g, b, a);
    if (g.params && blockIdx.x == 0 && blockIdx.y == 0 && t == 0) aug_write_params(g, d, b);
    const T* src = raw + (int64_t)b * a.sb + a.base;
#pragma unroll
    for (int k = 0; k < TI * TJ / 256; ++k) {
        // fast thread index along the source's unit-stride axis; the tile's columns are OUTPUT columns, read at their sources
        // (an ascending or descending run of source columns with at most one wrap)
        const int ii = a.along_i ? (t & (TI - 1)) : (t / TJ + k * (256 / TJ));
        const int jj = a.along_i ? (t / TI + k * (256 / TI)) : (t & (TJ - 1));
        const int i = i0 + ii, j = j0 + jj;
        float v = 0.f;
        const bool need = a.hi || (i >= d.p && (i - d.p) % a.f == 0);
        if (i < a.H && j < a.W && need)
            v = prep_value(raw_to_float<T>(src[(int64_t)i * a.si + (int64_t)aug_src(j, d, a.W) * a.sj]), a);
        tile[ii][jj] = v;
    }
    __syncthreads();
    const int Hl = a.H / a.f, Wl = a.W / a.fw;
#pragma unroll
    for (int k = 0; k < TI * TJ / 256; ++k) {
        const int ii = t / TJ + k * (256 / TJ), jj = t & (TJ - 1);
        const int i = i0 + ii, j = j0 + jj;
        if (i >= a.H || j >= a.W) continue;
        const float v = tile[ii][jj];
        if (a.hi) a.hi[((int64_t)b * a.H + i) * a.W + j] = v;
        if (a.lo && i >= d.p && j >= a.cp && (i - d.p) % a.f == 0 && (j - a.cp) % a.fw == 0) {
            const int il = (i - d.p) / a.f, jl = (j - a.cp) / a.fw;
            const bool drop = aug_dropped(d.key, AUG_BEAM + (uint64_t)il, g.beam_thr) ||
                              aug_dropped(d.key, AUG_POINT + (uint64_t)il * Wl + jl, g.point_thr);
            if (il < Hl && jl < Wl) a.lo[((int64_t)b * Hl + il) * Wl + jl] = drop ? 0.f : v;
        }
    }
}

// 4 consecutive pixels of a row-major float32 row from the 16-byte aligned group at pixel g4 (a multiple of 4)
template <int SJ>
__device__ __forceinline__ void load_group4(const float* __restrict__ row, int g4, float* e) {
    const float* p = row + (int64_t)g4 * SJ;
    if (SJ == 1) {
        const float4 q = *(const float4*)p;
        e[0] = q.x; e[1] = q.y; e[2] = q.z; e[3] = q.w;
    } else {
        const float4 q0 = *(const float4*)p, q1 = *(const float4*)(p + 4);
        e[0] = q0.x; e[1] = q0.z; e[2] = q1.x; e[3] = q1.z;
    }
}

// Row-major float32 sources: a thread owns 4 consecutive OUTPUT pixels of one row (one 16-byte store to hi, one to lo when the
// widths agree).  Their sources are 4 consecutive pixels (mod W), descending under a mirror; they start at a0 with a0 % 4 ==
// (-s) % 4 either way, so a sample whose shift is a multiple of 4 reads one aligned group like the plain kernel and any other
// sample reads the two aligned groups around them (the second one is its neighbour's first: served by the cache).
template <int SJ>
__global__ __launch_bounds__(256) void range_prep_rows_aug_kernel(const float* __restrict__ raw, PrepArgs a, AugArgs g) {
    const int W4 = a.W >> 2;
    const int64_t n4 = (int64_t)a.H * W4;
    const int b = blockIdx.y;
    const int Hl = a.H / a.f, Wl = a.W / a.fw;
    const AugDraw d = aug_draw(g, b, a);
    if (g.params && blockIdx.x == 0 && threadIdx.x == 0) aug_write_params(g, d, b);
    const float* src = raw + (int64_t)b * a.sb;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n4; k += (int64_t)gridDim.x * 256) {
        const int i = (int)(k / W4), j = (int)(k - (int64_t)i * W4) * 4;
        const bool lo_row = a.lo && i >= d.p && (i - d.p) % a.f == 0;
        if (!a.hi && !lo_row) continue;
        int c = j - d.s;
        if (c < 0) c += a.W;
        int a0 = d.flip ? a.W - 4 - c : c;                  // the lowest of the 4 source pixels (mod W)
        if (a0 < 0) a0 += a.W;
        const int r = a0 & 3, g0 = a0 - r;
        const float* row = src + (int64_t)i * a.si;
        float e[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        load_group4<SJ>(row, g0, e);
        if (r) load_group4<SJ>(row, g0 + 4 == a.W ? 0 : g0 + 4, e + 4);
        float u[4], v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) u[q] = r == 0 ? e[q] : r == 1 ? e[q + 1] : r == 2 ? e[q + 2] : e[q + 3];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = prep_value(d.flip ? u[3 - q] : u[q], a);
        if (a.hi) *(float4*)(a.hi + ((int64_t)b * a.H + i) * a.W + j) = make_float4(v[0], v[1], v[2], v[3]);
        if (lo_row) {
            const int il = (i - d.p) / a.f;
            if (il >= Hl) continue;
            float* dst = a.lo + ((int64_t)b * Hl + il) * Wl;
            const bool beam = aug_dropped(d.key, AUG_BEAM + (uint64_t)il, g.beam_thr);
            if (a.fw == 1) {
                float w[4];         // a select into a fresh array: as `if (drop) v[q] = 0.f` the compiled kernel kept the point-dropped values
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const bool drop = beam || aug_dropped(d.key, AUG_POINT + (uint64_t)il * Wl + (j + q), g.point_thr);
                    w[q] = drop ? 0.f : v[q];
                }
                *(float4*)(dst + j) = make_float4(w[0], w[1], w[2], w[3]);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int jj = j + q;
                    if (jj >= a.cp && (jj - a.cp) % a.fw == 0) {
                        const int jl = (jj - a.cp) / a.fw;
                        const bool drop = beam || aug_dropped(d.key, AUG_POINT + (uint64_t)il * Wl + jl, g.point_thr);
                        dst[jl] = drop ? 0.f : v[q];
                    }
                }
            }
        }
    }
}

// ---- multi-channel batches (tulip_range_prep_c / tulip_range_prep_aug_c; host definition tulip_amd/prep_channels.py) -------
// Channel 0 is the range and goes through prep_value; a pixel whose range is zero after scale and gate is a hole, and a hole has
// no other channel either.  Outputs are planes: hi (B,C,H,W), lo (B,C,H/f,W/fw).  One template per kernel family, AUG = the
// per-sample augmentation (the draws and the drops are per pixel: every channel shares them); the plain form is the augmented
// one with s = 0, no mirror and p = row_phase, plus the roll of the stores.
struct ChanArgs {
    int64_t sc;                    // element stride from a pixel's channel c to its channel c + 1
    int C, logmask;                // logmask bit c - 1: log1p on channel c
    float scale[3];                // the scale of channels 1 .. 3
};

// The value of channel c >= 1 of one pixel; all four multi-channel kernels form it with this one expression.  A select, not a
// multiply: whatever the raw value of a hole is, the result is +0.0.
__device__ __forceinline__ float chan_value(float raw, float s, bool logc, bool hole) {
    float u = raw * s;
    u = hole ? 0.f : u;
    if (logc) u = log1pf(u);
    return u;
}
// every channel of one pixel from its N >= C raw channels
template <int N>
__device__ __forceinline__ void pixel_values(const float (&r)[N], const PrepArgs& a, const ChanArgs& ch, float (&v)[4]) {
    const bool hole = prep_gated(r[0], a) == 0.f;
    v[0] = prep_value(r[0], a);
#pragma unroll
    for (int c = 1; c < 4; ++c)
        v[c] = (c < N && c < ch.C) ? chan_value(r[c < N ? c : 0], ch.scale[c - 1], (ch.logmask >> (c - 1)) & 1, hole) : 0.f;
}

template <bool AUG>
__global__ __launch_bounds__(256) void range_prep_c_kernel(const float* __restrict__ raw, PrepArgs a, ChanArgs ch, AugArgs g) {
    __shared__ float tile[4][TI][TJ + 1];
    const int b = blockIdx.z, i0 = blockIdx.y * TI, j0 = blockIdx.x * TJ, t = threadIdx.x;
    AugDraw d{0, 0, 0, a.rp};
    if (AUG) {
        d = aug_draw(g, b, a);
        if (g.params && blockIdx.x == 0 && blockIdx.y == 0 && t == 0) aug_write_params(g, d, b);
    }
    const float* src = raw + (int64_t)b * a.sb + a.base;
#pragma unroll
    for (int k = 0; k < TI * TJ / 256; ++k) {
        // as in range_prep_aug_kernel: the tile's columns are OUTPUT columns (before the roll), read at their sources
        const int ii = a.along_i ? (t & (TI - 1)) : (t / TJ + k * (256 / TJ));
        const int jj = a.along_i ? (t / TI + k * (256 / TI)) : (t & (TJ - 1));
        const int i = i0 + ii, j = j0 + jj;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        const bool need = a.hi || (i >= d.p && (i - d.p) % a.f == 0);
        if (i < a.H && j < a.W && need) {
            const float* p = src + (int64_t)i * a.si + (int64_t)(AUG ? aug_src(j, d, a.W) : j) * a.sj;
            float r[4] = {p[0], 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 1; c < 4; ++c)
                if (c < ch.C) r[c] = p[c * ch.sc];
            pixel_values<4>(r, a, ch, v);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < ch.C) tile[c][ii][jj] = v[c];
    }
    __syncthreads();
    const int Hl = a.H / a.f, Wl = a.W / a.fw;
#pragma unroll
    for (int k = 0; k < TI * TJ / 256; ++k) {
        const int ii = t / TJ + k * (256 / TJ), jj = t & (TJ - 1);
        const int i = i0 + ii, j = j0 + jj;
        if (i >= a.H || j >= a.W) continue;
        int jo = j + a.shift_hi;                                                            // torch.roll along W (0 under AUG)
        if (jo >= a.W) jo -= a.W;
        const bool lo_px = a.lo && i >= d.p && j >= a.cp && (i - d.p) % a.f == 0 && (j - a.cp) % a.fw == 0;
        const int il = (i - d.p) / a.f, jl0 = (j - a.cp) / a.fw;
        int jl = jl0 + a.shift_lo;
        if (jl >= Wl) jl -= Wl;
        bool drop = false;
        if (AUG && lo_px)
            drop = aug_dropped(d.key, AUG_BEAM + (uint64_t)il, g.beam_thr) ||
                   aug_dropped(d.key, AUG_POINT + (uint64_t)il * Wl + jl0, g.point_thr);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c >= ch.C) continue;
            const float v = tile[c][ii][jj];
            if (a.hi) a.hi[(((int64_t)b * ch.C + c) * a.H + i) * a.W + jo] = v;
            if (lo_px && il < Hl && jl0 < Wl) a.lo[(((int64_t)b * ch.C + c) * Hl + il) * Wl + jl] = drop ? 0.f : v;
        }
    }
}

// 4 consecutive pixels, CR interleaved channels each, from the 16-byte aligned group at pixel g4 (a multiple of 4): the two
// loads of load_group4<2> at CR = 2 (now both halves are kept), one float4 per pixel at CR = 4
template <int CR>
__device__ __forceinline__ void load_group4c(const float* __restrict__ row, int g4, float (*e)[CR]) {
    const float4* p = (const float4*)(row + (int64_t)g4 * CR);
    if constexpr (CR == 2) {
        const float4 q0 = p[0], q1 = p[1];
        e[0][0] = q0.x; e[0][1] = q0.y; e[1][0] = q0.z; e[1][1] = q0.w;
        e[2][0] = q1.x; e[2][1] = q1.y; e[3][0] = q1.z; e[3][1] = q1.w;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 x = p[q];
            e[q][0] = x.x; e[q][1] = x.y; e[q][2] = x.z; e[q][3] = x.w;
        }
    }
}

// The interleaved row-major float32 payload with CR in {2, 4} raw channels: a thread owns 4 consecutive OUTPUT pixels of one row
// for all C channels.  It reads them once (the aligned group, or under AUG the two aligned groups around their sources, rotated
// in registers as in range_prep_rows_aug_kernel) and issues C 16-byte plane stores to hi and C to lo.
template <int CR, bool AUG>
__global__ __launch_bounds__(256) void range_prep_rows_c_kernel(const float* __restrict__ raw, PrepArgs a, ChanArgs ch,
                                                                AugArgs g) {
    const int W4 = a.W >> 2;
    const int64_t n4 = (int64_t)a.H * W4;
    const int b = blockIdx.y;
    const int Hl = a.H / a.f, Wl = a.W / a.fw;
    AugDraw d{0, 0, 0, a.rp};
    if (AUG) {
        d = aug_draw(g, b, a);
        if (g.params && blockIdx.x == 0 && threadIdx.x == 0) aug_write_params(g, d, b);
    }
    const float* src = raw + (int64_t)b * a.sb;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n4; k += (int64_t)gridDim.x * 256) {
        const int i = (int)(k / W4), j = (int)(k - (int64_t)i * W4) * 4;
        const bool lo_row = a.lo && i >= d.p && (i - d.p) % a.f == 0 && (i - d.p) / a.f < Hl;
        if (!a.hi && !lo_row) continue;
        const float* row = src + (int64_t)i * a.si;
        float u[4][CR];                                     // [output pixel][raw channel]
        if (AUG) {
            int c = j - d.s;
            if (c < 0) c += a.W;
            int a0 = d.flip ? a.W - 4 - c : c;              // the lowest of the 4 source pixels (mod W)
            if (a0 < 0) a0 += a.W;
            const int r = a0 & 3, g0 = a0 - r;
            float e[8][CR];
#pragma unroll
            for (int q = 4; q < 8; ++q)
#pragma unroll
                for (int x = 0; x < CR; ++x) e[q][x] = 0.f;
            load_group4c<CR>(row, g0, e);
            if (r) load_group4c<CR>(row, g0 + 4 == a.W ? 0 : g0 + 4, e + 4);
            float s[4][CR];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int x = 0; x < CR; ++x) s[q][x] = r == 0 ? e[q][x] : r == 1 ? e[q + 1][x] : r == 2 ? e[q + 2][x] : e[q + 3][x];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int x = 0; x < CR; ++x) u[q][x] = d.flip ? s[3 - q][x] : s[q][x];
        } else {
            load_group4c<CR>(row, j, u);
        }
        float v[4][4];                                      // [output pixel][channel]
#pragma unroll
        for (int q = 0; q < 4; ++q) pixel_values<CR>(u[q], a, ch, v[q]);
        const int il = (i - d.p) / a.f;
        bool sel[4], drop[4];                               // low-res: is pixel q a sampled column, did it lose its return
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int jj = j + q;
            sel[q] = lo_row && jj >= a.cp && (jj - a.cp) % a.fw == 0;
            drop[q] = false;
        }
        if (AUG && lo_row) {
            const bool beam = aug_dropped(d.key, AUG_BEAM + (uint64_t)il, g.beam_thr);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (sel[q])
                    drop[q] = beam || aug_dropped(d.key, AUG_POINT + (uint64_t)il * Wl + (j + q - a.cp) / a.fw, g.point_thr);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c >= ch.C) continue;
            if (a.hi) {
                float* dst = a.hi + (((int64_t)b * ch.C + c) * a.H + i) * a.W;
                int jo = j + a.shift_hi;
                if (jo >= a.W) jo -= a.W;
                if ((a.shift_hi & 3) == 0) {
                    *(float4*)(dst + jo) = make_float4(v[0][c], v[1][c], v[2][c], v[3][c]);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) { dst[jo] = v[q][c]; if (++jo == a.W) jo = 0; }
                }
            }
            if (lo_row) {
                float* dst = a.lo + (((int64_t)b * ch.C + c) * Hl + il) * Wl;
                float w[4];                                 // a select into a fresh array, as in range_prep_rows_aug_kernel
#pragma unroll
                for (int q = 0; q < 4; ++q) w[q] = drop[q] ? 0.f : v[q][c];
                if (a.fw == 1 && (a.shift_lo & 3) == 0) {
                    int jl = j + a.shift_lo;
                    if (jl >= Wl) jl -= Wl;
                    *(float4*)(dst + jl) = make_float4(w[0], w[1], w[2], w[3]);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (sel[q]) {
                            int jl = (j + q - a.cp) / a.fw + a.shift_lo;
                            if (jl >= Wl) jl -= Wl;
                            dst[jl] = w[q];
                        }
                    }
                }
            }
        }
    }
}

// ---- KITTI point cloud -> range image(kitti_utils/sample_kitti_dataset.py:24-66), float32 in numpy's op order
struct KittiProj {
    int rows, cols;
    float ang_start_y, ang_res_y, ang_res_x, max_range, min_range, half_cols;
};
__device__ __forceinline__ bool kitti_pixel(const float* __restrict__ p, const KittiProj& k, int& row, int& col) {
#pragma clang fp contract(off)
    const float x = p[0], y = p[1], z = p[2];
    const float deg = 180.0f, pi = 3.14159274101257324f;                       // float32(180.0), float32(np.pi)
    const float vert = atan2f(z, sqrtf(x * x + y * y)) * deg / pi;              // :32
    const float r = rintf((vert + k.ang_start_y) / k.ang_res_y);                // :33-34 (round half to even)
    const float hor = atan2f(x, y) * deg / pi;                                  // :36
    const float c = truncf((hor - 90.0f) / k.ang_res_x);                        // :38 np.int_ truncates
    if (!(fabsf(r) < 1e9f) || !(fabsf(c) < 1e9f)) return false;
    long long ci = -(long long)c + (long long)k.half_cols;
    if (ci >= k.cols) ci -= k.cols;                                             // :40-41
    const long long ri = (long long)r;
    row = (int)ri; col = (int)ci;
    return ri >= 0 && ri < k.rows && ci >= 0 && ci < k.cols;                    // :49
}
__global__ __launch_bounds__(256) void kitti_mark_kernel(const float* __restrict__ pts, int64_t n, KittiProj k,
                                                         int* __restrict__ winner) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        int row, col;
        if (kitti_pixel(pts + i * 4, k, row, col)) atomicMax(&winner[row * k.cols + col], (int)i);   // last point wins
    }
}
__global__ __launch_bounds__(256) void kitti_resolve_kernel(const float* __restrict__ pts, KittiProj k,
                                                            int* __restrict__ winner, float* __restrict__ out) {
#pragma clang fp contract(off)
    const int npix = k.rows * k.cols;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) {
        const int w = winner[i];
        float rng = 0.f, inten = 0.f;
        if (w >= 0) {
            const float* p = pts + (int64_t)w * 4;
            rng = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);               // :43
            if (rng > k.max_range || rng < k.min_range) rng = 0.f;               // :44-45
            inten = p[3];                                                        // :47-48 never fire (range already 0)
        }
        out[(int64_t)i * 2] = rng;
        out[(int64_t)i * 2 + 1] = inten;
        winner[i] = -1;                                                          // scratch handed back reset
    }
}

inline int64_t iabs64(int64_t v) { return v < 0 ? -v : v; }

// The argument checks and the kernel arguments both entry points share; false: TULIP_ERR_ARG.  rows16: the source is row-major
// float32 and everything is aligned for the 16-byte kernels.
bool prep_setup(const void* raw, int raw_dtype, int64_t batch_stride, int64_t row_stride, int64_t col_stride,
                int64_t base_offset, float* hi, float* lo, int B, int H, int W, int row_factor, int col_factor, int row_phase,
                int col_phase, float scale, int gate, float min_range, float max_range, int log_transform, int roll_shift,
                PrepArgs& a, bool& rows16) {
    if (!raw || (!hi && !lo) || B <= 0 || H <= 0 || W <= 0 || row_factor < 1 || col_factor < 1) return false;
    if (H % row_factor || W % col_factor || row_phase < 0 || row_phase >= row_factor || col_phase < 0 ||
        col_phase >= col_factor || (raw_dtype != 0 && raw_dtype != 1))
        return false;
    a.sb = batch_stride; a.si = row_stride; a.sj = col_stride; a.base = base_offset;
    a.hi = hi; a.lo = lo;
    a.H = H; a.W = W; a.f = row_factor; a.fw = col_factor; a.rp = row_phase; a.cp = col_phase;
    a.scale = scale; a.gmin = min_range; a.gmax = max_range; a.gate = gate; a.logt = log_transform;
    const int Wl = W / col_factor;
    a.shift_hi = ((roll_shift % W) + W) % W;
    a.shift_lo = ((roll_shift % Wl) + Wl) % Wl;
    a.along_i = iabs64(row_stride) < iabs64(col_stride);
    rows16 = raw_dtype == 0 && (W & 3) == 0 && base_offset == 0 && (col_stride == 1 || col_stride == 2) &&
             row_stride == (int64_t)W * col_stride && (batch_stride & 3) == 0 &&
             ((uintptr_t)raw & 15) == 0 && (!hi || ((uintptr_t)hi & 15) == 0) && (!lo || ((uintptr_t)lo & 15) == 0) &&
             (Wl & 3) == 0;
    return true;
}
inline int prep_rows_blocks(int H, int W) {
    int64_t nb = ((int64_t)H * (W / 4) + 255) / 256;
    return nb > 2048 ? 2048 : (int)nb;
}

// The multi-channel entry points' own checks and arguments, after prep_setup; false: TULIP_ERR_ARG.  rows16: prep_setup's
// alignment conditions for the interleaved payload, whose pixel stride is its channel count (2 or 4) and channel stride 1.
bool chan_setup(const void* raw, int raw_dtype, int64_t batch_stride, int64_t row_stride, int64_t col_stride,
                int64_t base_offset, const PrepArgs& a, int C, int64_t chan_stride, const float* chan_scale, uint32_t chan_log,
                ChanArgs& ch, bool& rows16) {
    if (raw_dtype != 0 || C < 1 || C > 4 || (C > 1 && !chan_scale) || (chan_log >> (C - 1))) return false;
    ch.sc = chan_stride; ch.C = C; ch.logmask = (int)chan_log;
    for (int c = 1; c < 4; ++c) ch.scale[c - 1] = c < C ? chan_scale[c - 1] : 1.f;
    const int Wl = a.W / a.fw;
    rows16 = (a.W & 3) == 0 && base_offset == 0 && (col_stride == 2 || col_stride == 4) && C <= col_stride &&
             (C == 1 || chan_stride == 1) && row_stride == (int64_t)a.W * col_stride && (batch_stride & 3) == 0 &&
             ((uintptr_t)raw & 15) == 0 && (!a.hi || ((uintptr_t)a.hi & 15) == 0) && (!a.lo || ((uintptr_t)a.lo & 15) == 0) &&
             (Wl & 3) == 0;
    return true;
}
template <bool AUG>
int launch_prep_c(const float* raw, const PrepArgs& a, const ChanArgs& ch, const AugArgs& g, bool rows16, int B,
                  hipStream_t stream) {
    if (rows16) {
        const dim3 grid(prep_rows_blocks(a.H, a.W), B);
        if (a.sj == 2)
            hipLaunchKernelGGL((range_prep_rows_c_kernel<2, AUG>), grid, dim3(256), 0, stream, raw, a, ch, g);
        else
            hipLaunchKernelGGL((range_prep_rows_c_kernel<4, AUG>), grid, dim3(256), 0, stream, raw, a, ch, g);
    } else {
        const dim3 grid((a.W + TJ - 1) / TJ, (a.H + TI - 1) / TI, B);
        hipLaunchKernelGGL(range_prep_c_kernel<AUG>, grid, dim3(256), 0, stream, raw, a, ch, g);
    }
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

}  // namespace

extern "C" int tulip_range_prep(const void* raw, int raw_dtype, int64_t batch_stride, int64_t row_stride,
                                int64_t col_stride, int64_t base_offset, float* hi, float* lo, int B, int H, int W,
                                int row_factor, int col_factor, int row_phase, int col_phase, float scale, int gate,
                                float min_range, float max_range, int log_transform, int roll_shift,
                                hipStream_t stream) {
    PrepArgs a;
    bool rows16;
    if (!prep_setup(raw, raw_dtype, batch_stride, row_stride, col_stride, base_offset, hi, lo, B, H, W, row_factor, col_factor,
                    row_phase, col_phase, scale, gate, min_range, max_range, log_transform, roll_shift, a, rows16))
        return TULIP_ERR_ARG;
    if (rows16) {
        const dim3 grid(prep_rows_blocks(H, W), B);
        if (col_stride == 1)
            hipLaunchKernelGGL(range_prep_rows_kernel<1>, grid, dim3(256), 0, stream, (const float*)raw, a);
        else
            hipLaunchKernelGGL(range_prep_rows_kernel<2>, grid, dim3(256), 0, stream, (const float*)raw, a);
        TULIP_CHECK_LAUNCH();
        return TULIP_OK;
    }
    const dim3 grid((W + TJ - 1) / TJ, (H + TI - 1) / TI, B);
    if (raw_dtype == 0)
        hipLaunchKernelGGL(range_prep_kernel<float>, grid, dim3(256), 0, stream, (const float*)raw, a);
    else
        hipLaunchKernelGGL(range_prep_kernel<__half>, grid, dim3(256), 0, stream, (const __half*)raw, a);
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

extern "C" int tulip_range_prep_aug(const void* raw, int raw_dtype, int64_t batch_stride, int64_t row_stride,
                                    int64_t col_stride, int64_t base_offset, float* hi, float* lo, int B, int H, int W,
                                    int row_factor, int col_factor, int row_phase, int col_phase, float scale, int gate,
                                    float min_range, float max_range, int log_transform, const int64_t* sample_ids,
                                    uint64_t seed, int flags, uint32_t beam_threshold, uint32_t point_threshold,
                                    int32_t* params_out, hipStream_t stream) {
    PrepArgs a;
    bool rows16;
    if (!prep_setup(raw, raw_dtype, batch_stride, row_stride, col_stride, base_offset, hi, lo, B, H, W, row_factor, col_factor,
                    row_phase, col_phase, scale, gate, min_range, max_range, log_transform, 0, a, rows16))
        return TULIP_ERR_ARG;
    if (!sample_ids || ((uintptr_t)sample_ids & 7) || ((uintptr_t)params_out & 3) ||
        (flags & ~(TULIP_AUG_ROLL | TULIP_AUG_FLIP | TULIP_AUG_ROW_PHASE)) || beam_threshold > (1u << 24) ||
        point_threshold > (1u << 24))
        return TULIP_ERR_ARG;
    AugArgs g;
    g.ids = (const long long*)sample_ids; g.seed = seed; g.flags = flags;
    g.beam_thr = beam_threshold; g.point_thr = point_threshold; g.params = params_out;
    if (rows16) {
        const dim3 grid(prep_rows_blocks(H, W), B);
        if (col_stride == 1)
            hipLaunchKernelGGL(range_prep_rows_aug_kernel<1>, grid, dim3(256), 0, stream, (const float*)raw, a, g);
        else
            hipLaunchKernelGGL(range_prep_rows_aug_kernel<2>, grid, dim3(256), 0, stream, (const float*)raw, a, g);
        TULIP_CHECK_LAUNCH();
        return TULIP_OK;
    }
    const dim3 grid((W + TJ - 1) / TJ, (H + TI - 1) / TI, B);
    if (raw_dtype == 0)
        hipLaunchKernelGGL(range_prep_aug_kernel<float>, grid, dim3(256), 0, stream, (const float*)raw, a, g);
    else
        hipLaunchKernelGGL(range_prep_aug_kernel<__half>, grid, dim3(256), 0, stream, (const __half*)raw, a, g);
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

extern "C" int tulip_range_prep_c(const void* raw, int raw_dtype, int64_t batch_stride, int64_t row_stride,
                                  int64_t col_stride, int64_t base_offset, float* hi, float* lo, int B, int H, int W,
                                  int row_factor, int col_factor, int row_phase, int col_phase, float scale, int gate,
                                  float min_range, float max_range, int log_transform, int roll_shift, hipStream_t stream,
                                  int C, int64_t chan_stride, const float* chan_scale, uint32_t chan_log) {
    PrepArgs a;
    ChanArgs ch;
    bool rows16;
    if (!prep_setup(raw, raw_dtype, batch_stride, row_stride, col_stride, base_offset, hi, lo, B, H, W, row_factor, col_factor,
                    row_phase, col_phase, scale, gate, min_range, max_range, log_transform, roll_shift, a, rows16) ||
        !chan_setup(raw, raw_dtype, batch_stride, row_stride, col_stride, base_offset, a, C, chan_stride, chan_scale, chan_log, ch,
                    rows16))
        return TULIP_ERR_ARG;
    return launch_prep_c<false>((const float*)raw, a, ch, AugArgs{}, rows16, B, stream);
}

extern "C" int tulip_range_prep_aug_c(const void* raw, int raw_dtype, int64_t batch_stride, int64_t row_stride,
                                      int64_t col_stride, int64_t base_offset, float* hi, float* lo, int B, int H, int W,
                                      int row_factor, int col_factor, int row_phase, int col_phase, float scale, int gate,
                                      float min_range, float max_range, int log_transform, const int64_t* sample_ids,
                                      uint64_t seed, int flags, uint32_t beam_threshold, uint32_t point_threshold,
                                      int32_t* params_out, hipStream_t stream, int C, int64_t chan_stride,
                                      const float* chan_scale, uint32_t chan_log) {
    PrepArgs a;
    ChanArgs ch;
    bool rows16;
    if (!prep_setup(raw, raw_dtype, batch_stride, row_stride, col_stride, base_offset, hi, lo, B, H, W, row_factor, col_factor,
                    row_phase, col_phase, scale, gate, min_range, max_range, log_transform, 0, a, rows16) ||
        !chan_setup(raw, raw_dtype, batch_stride, row_stride, col_stride, base_offset, a, C, chan_stride, chan_scale, chan_log, ch,
                    rows16))
        return TULIP_ERR_ARG;
    if (!sample_ids || ((uintptr_t)sample_ids & 7) || ((uintptr_t)params_out & 3) ||
        (flags & ~(TULIP_AUG_ROLL | TULIP_AUG_FLIP | TULIP_AUG_ROW_PHASE)) || beam_threshold > (1u << 24) ||
        point_threshold > (1u << 24))
        return TULIP_ERR_ARG;
    AugArgs g;
    g.ids = (const long long*)sample_ids; g.seed = seed; g.flags = flags;
    g.beam_thr = beam_threshold; g.point_thr = point_threshold; g.params = params_out;
    return launch_prep_c<true>((const float*)raw, a, ch, g, rows16, B, stream);
}

extern "C" int tulip_kitti_range_map(const float* points, int64_t n, int rows, int cols, float ang_start_y,
                                     float ang_res_y, float ang_res_x, float max_range, float min_range,
                                     int32_t* winner, float* out, hipStream_t stream) {
    if (!points || !winner || !out || n < 0 || n > 0x7fffffff || rows <= 0 || cols <= 0 || !(ang_res_y > 0.f) ||
        !(ang_res_x > 0.f))
        return TULIP_ERR_ARG;
    KittiProj k{rows, cols, ang_start_y, ang_res_y, ang_res_x, max_range, min_range, (float)cols / 2.0f};
    if (n > 0) {
        int64_t nb = (n + 255) / 256;
        if (nb > 4096) nb = 4096;
        hipLaunchKernelGGL(kitti_mark_kernel, dim3((int)nb), dim3(256), 0, stream, points, n, k, winner);
    }
    hipLaunchKernelGGL(kitti_resolve_kernel, dim3((rows * cols + 255) / 256), dim3(256), 0, stream, points, k, winner,
                       out);
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

// The selectable training loss, TULIP(loss="l2" | "berhu") (tulip_amd/loss.py is the host definition): four flat, HBM-bound
// kernels over n = pred.numel() elements, and their masked forms (TULIP(loss_valid_min=...), the _m entry points: LossMask
// below).  float4 loads where pred / target (/ dpred) are 16-byte aligned, a scalar tail behind them; at most 1024 workgroups of 256 threads; every reduction in a fixed order (per-thread grid-stride sums, the wave tree,
// four wave results in a fixed bracket, the final fold in double by one workgroup): the same bits run to run.  Plain vector
// stores only, no atomics.   gfx950 only.
#include "common.h"
#include "tulip_hip.h"

namespace {

constexpr int LOSS_BLOCKS = TULIP_LOSS_BLOCKS_MAX;

// max that keeps a NaN: fmaxf drops it, and a NaN anywhere in (pred, target) has to reach C, the loss and the gradient
__device__ __forceinline__ float nan_max(float a, float b) { return (b > a || b != b) ? b : a; }

__device__ __forceinline__ float block_sum(float v, float (*red)[4], int k) {
    v = group_sum<64>(v);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v;
    return v;
}

// berHu (util/evaluation.py:177-180) with C fixed: |d| below C, (d^2 + C^2) / (2 C) from C on.  C == 0 (pred == target
// everywhere, where the reference's formula is 0/0): 0.  A NaN C fails both tests and gives NaN.
__device__ __forceinline__ float berhu_value(float d, float C) {
    const float a = fabsf(d);
    if (a < C) return a;
    if (C == 0.f) return 0.f;
    return (a * a + C * C) / (2.f * C);
}

// d(loss)/d(pred) * n / g: sign(d) below C, d / C from C on (no gradient through C); C == 0: 0
__device__ __forceinline__ float berhu_grad(float d, float C, float g) {
    if (fabsf(d) < C) return d > 0.f ? g : (d < 0.f ? -g : 0.f);
    if (C == 0.f) return 0.f;
    return (d / C) * g;
}

// C = 0.2f * max|d| from the per-workgroup maxima of loss_stats_kernel (stats[4 wg + 3], wg < nb <= 1024), folded by every
// workgroup itself: max is exact and order-independent, so every workgroup forms the same bits
__device__ __forceinline__ float berhu_threshold(const float* __restrict__ stats, int nb, float* red) {
    float m = 0.f;
    for (int i = threadIdx.x; i < nb; i += 256) m = nan_max(m, stats[4 * i + 3]);
    m = group_reduce<64>(m, [](float a, float b) { return nan_max(a, b); });
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = nan_max(nan_max(red[0], red[1]), nan_max(red[2], red[3]));
    return 0.2f * m;
}

// The valid-pixel mask of the _m entry points (TULIP(loss_valid_min=...)): element e = (b * chans + c) * chan_stride + pix of
// (pred, target) counts iff target[b, 0, pix] > valid_min (false for a NaN) -- channel 0, the range.  chans == 1: that is the
// element's own target value, no second load.  The kernels take this struct as a trailing parameter pack K..., LossMask for the
// masked instantiations and empty for the unmasked ones, whose arguments and code are thereby what they were without it.
struct LossMask {
    int64_t chan_stride;       // H * W
    int chans;
    int narrow;                // n < 2^32: the index arithmetic in 32 bits
    float valid_min;
    uint32_t* counts;          // [TULIP_LOSS_BLOCKS_MAX]: the valid elements each workgroup of loss_stats_kernel saw
    int64_t* n_valid;          // n_v = their sum, as the bwd / final kernel formed it
};

__device__ __forceinline__ LossMask mask_arg() { return LossMask{}; }
__device__ __forceinline__ LossMask mask_arg(const LossMask& k) { return k; }

// the index of target[b, 0, pix] for element e.  On the float4 route (chan_stride % 4 == 0) e is a multiple of 4 and so is the
// result: a group never straddles a channel
__device__ __forceinline__ int64_t chan0_index(int64_t e, const LossMask& k) {
    if (k.narrow) {
        const uint32_t hw = (uint32_t)k.chan_stride, cs = hw * (uint32_t)k.chans, u = (uint32_t)e, base = u - u % cs;
        return base + (u - base) % hw;
    }
    const int64_t cs = k.chan_stride * k.chans, base = e - e % cs;
    return base + (e - base) % k.chan_stride;
}
// the mask values of the float4 group at element e, whose own target values are t / of the single element e
__device__ __forceinline__ float4 mask_src4(const float* __restrict__ tgt, int64_t e, float4 t, const LossMask& k) {
    if (k.chans != 1) t = *(const float4*)(tgt + chan0_index(e, k));
    return t;
}
__device__ __forceinline__ float mask_src(const float* __restrict__ tgt, int64_t e, float t, const LossMask& k) {
    if (k.chans != 1) t = tgt[chan0_index(e, k)];
    return t;
}

// n_v = the sum of the per-workgroup counts (counts[wg], wg < nb <= 1024), folded by every workgroup itself: integer addition is
// exact in any order, so every workgroup holds the same n_v
__device__ __forceinline__ int64_t valid_count(const uint32_t* __restrict__ counts, int nb, long long* red) {
    long long c = 0;
    for (int i = threadIdx.x; i < nb; i += 256) c += counts[i];
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

struct LossAcc {
    float abs = 0.f, pix = 0.f, sq = 0.f, mx = 0.f;
    uint32_t cnt = 0;          // the valid elements (masked kernels only)
    __device__ __forceinline__ void add(float p, float t, int log_transform) {
        const float d = p - t, a = fabsf(d);
        abs += a;
        if (log_transform) pix += fabsf(expm1f(p) - expm1f(t));
        sq += d * d;
        mx = nan_max(mx, a);
    }
    // an invalid element enters nothing: whatever p and t hold there (a NaN, an infinity) stays out of the sums and the max
    __device__ __forceinline__ void add_if(bool valid, float p, float t, int log_transform) {
        if (valid) {
            add(p, t, log_transform);
            ++cnt;
        }
    }
};

// stats[4 wg + {0, 1, 2, 3}] = {sum |d|, sum |expm1 p - expm1 t| (log_transform, else 0), sum d^2, max |d|} of the workgroup;
// MASK: over the valid elements, and k.counts[wg] = how many there were
template <class... K>
__global__ __launch_bounds__(256) void loss_stats_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                         float* __restrict__ stats, int64_t n, int64_t n4, int log_transform,
                                                         K... kk) {
    constexpr bool MASK = sizeof...(K) != 0;
    const LossMask k = mask_arg(kk...);
    __shared__ float red[4][4];
    LossAcc s;
    const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = first; i < n4; i += stride) {
        const float4 p = *(const float4*)(pred + i * 4), t = *(const float4*)(tgt + i * 4);
        if constexpr (MASK) {
            const float4 z = mask_src4(tgt, i * 4, t, k);
            s.add_if(z.x > k.valid_min, p.x, t.x, log_transform); s.add_if(z.y > k.valid_min, p.y, t.y, log_transform);
            s.add_if(z.z > k.valid_min, p.z, t.z, log_transform); s.add_if(z.w > k.valid_min, p.w, t.w, log_transform);
        } else {
            s.add(p.x, t.x, log_transform); s.add(p.y, t.y, log_transform);
            s.add(p.z, t.z, log_transform); s.add(p.w, t.w, log_transform);
        }
    }
    for (int64_t i = n4 * 4 + first; i < n; i += stride) {
        if constexpr (MASK) s.add_if(mask_src(tgt, i, tgt[i], k) > k.valid_min, pred[i], tgt[i], log_transform);
        else s.add(pred[i], tgt[i], log_transform);
    }
    if constexpr (MASK) {
        // integers: per thread, the wave tree, four wave results
        __shared__ uint32_t cred[4];
        uint32_t c = s.cnt;
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if ((threadIdx.x & 63) == 0) cred[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) k.counts[blockIdx.x] = (cred[0] + cred[1]) + (cred[2] + cred[3]);
    }
    block_sum(s.abs, red, 0);
    block_sum(s.pix, red, 1);
    block_sum(s.sq, red, 2);
    const float m = group_reduce<64>(s.mx, [](float a, float b) { return nan_max(a, b); });
    if ((threadIdx.x & 63) == 0) red[3][threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        *(float4*)(stats + 4 * (size_t)blockIdx.x) =
            make_float4((red[0][0] + red[0][1]) + (red[0][2] + red[0][3]), (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]),
                        (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]),
                        nan_max(nan_max(red[3][0], red[3][1]), nan_max(red[3][2], red[3][3])));
    }
}

template <int KIND>
__device__ __forceinline__ float loss_grad(float p, float t, float C, float g) {
    const float d = p - t;
    if constexpr (KIND == TULIP_LOSS_L1) return d > 0.f ? g : (d < 0.f ? -g : 0.f);
    else if constexpr (KIND == TULIP_LOSS_L2) return (2.f * d) * g;
    else return berhu_grad(d, C, g);
}

// dpred[i] = g * grad_kind(d_i; C), g = gscale / n (one rounding, as in tulip_l1_loss_bwd).  MASK: n_v (folded here, written to
// k.n_valid) in place of n, C from the valid maxima, +0 at the invalid elements -- and everywhere when n_v == 0
template <int KIND, class... K>
__global__ __launch_bounds__(256) void loss_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                       const float* __restrict__ stats, int nb,
                                                       const float* __restrict__ gscale_dev, float gscale,
                                                       float* __restrict__ dpred, float* __restrict__ loss_c, int64_t n,
                                                       int64_t n4, K... kk) {
    constexpr bool MASK = sizeof...(K) != 0;
    const LossMask k = mask_arg(kk...);
    __shared__ float red[4];
    float C = 0.f;
    if constexpr (KIND == TULIP_LOSS_BERHU) {
        C = berhu_threshold(stats, nb, red);
        if (blockIdx.x == 0 && threadIdx.x == 0) loss_c[0] = C;
    }
    float g;
    if constexpr (MASK) {
        __shared__ long long cred[4];
        const int64_t nv = valid_count(k.counts, nb, cred);
        if (blockIdx.x == 0 && threadIdx.x == 0) k.n_valid[0] = nv;
        g = nv ? (gscale_dev ? gscale_dev[0] : gscale) / (float)nv : 0.f;
    } else {
        g = (gscale_dev ? gscale_dev[0] : gscale) / (float)n;
    }
    const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = first; i < n4; i += stride) {
        const float4 p = *(const float4*)(pred + i * 4), t = *(const float4*)(tgt + i * 4);
        float4 d = make_float4(loss_grad<KIND>(p.x, t.x, C, g), loss_grad<KIND>(p.y, t.y, C, g),
                               loss_grad<KIND>(p.z, t.z, C, g), loss_grad<KIND>(p.w, t.w, C, g));
        if constexpr (MASK) {
            const float4 z = mask_src4(tgt, i * 4, t, k);
            d = make_float4(z.x > k.valid_min ? d.x : 0.f, z.y > k.valid_min ? d.y : 0.f, z.z > k.valid_min ? d.z : 0.f,
                            z.w > k.valid_min ? d.w : 0.f);
        }
        *(float4*)(dpred + i * 4) = d;
    }
    for (int64_t i = n4 * 4 + first; i < n; i += stride) {
        const float d = loss_grad<KIND>(pred[i], tgt[i], C, g);
        if constexpr (MASK) dpred[i] = mask_src(tgt, i, tgt[i], k) > k.valid_min ? d : 0.f;
        else dpred[i] = d;
    }
}

// berHu's second pass: vpart[wg] = the workgroup's sum of the elementwise values (the sum needs C); MASK: of the valid elements
// (n_v == 0: nothing is read)
template <class... K>
__global__ __launch_bounds__(256) void loss_value_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                         const float* __restrict__ stats, int nb, float* __restrict__ vpart,
                                                         int64_t n, int64_t n4, K... kk) {
    constexpr bool MASK = sizeof...(K) != 0;
    const LossMask k = mask_arg(kk...);
    __shared__ float red[4];
    __shared__ float sum[1][4];
    if constexpr (MASK) {
        __shared__ long long cred[4];
        if (valid_count(k.counts, nb, cred) == 0) {       // (the same n_v in every thread: a uniform exit)
            if (threadIdx.x == 0) vpart[blockIdx.x] = 0.f;
            return;
        }
    }
    const float C = berhu_threshold(stats, nb, red);
    float s = 0.f;
    const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = first; i < n4; i += stride) {
        const float4 p = *(const float4*)(pred + i * 4), t = *(const float4*)(tgt + i * 4);
        if constexpr (MASK) {
            const float4 z = mask_src4(tgt, i * 4, t, k);
            if (z.x > k.valid_min) s += berhu_value(p.x - t.x, C);
            if (z.y > k.valid_min) s += berhu_value(p.y - t.y, C);
            if (z.z > k.valid_min) s += berhu_value(p.z - t.z, C);
            if (z.w > k.valid_min) s += berhu_value(p.w - t.w, C);
        } else {
            s += berhu_value(p.x - t.x, C); s += berhu_value(p.y - t.y, C);
            s += berhu_value(p.z - t.z, C); s += berhu_value(p.w - t.w, C);
        }
    }
    for (int64_t i = n4 * 4 + first; i < n; i += stride) {
        if constexpr (MASK) {
            if (mask_src(tgt, i, tgt[i], k) > k.valid_min) s += berhu_value(pred[i] - tgt[i], C);
        } else {
            s += berhu_value(pred[i] - tgt[i], C);
        }
    }
    block_sum(s, sum, 0);
    __syncthreads();
    if (threadIdx.x == 0) vpart[blockIdx.x] = (sum[0][0] + sum[0][1]) + (sum[0][2] + sum[0][3]);
}

// one workgroup: the partials folded in double (l1_final_kernel's order); losses[0] = the chosen loss, losses[1] = pixel_loss.
// MASK: inv_n = 1 / n_v formed here from the counts (0 when n_v == 0: both losses 0), n_v written to k.n_valid
template <class... K>
__global__ __launch_bounds__(256) void loss_final_kernel(int kind, const float* __restrict__ stats,
                                                         const float* __restrict__ vpart, float* __restrict__ losses, int nb,
                                                         double inv_n, int log_transform, K... kk) {
    constexpr bool MASK = sizeof...(K) != 0;
    const LossMask k = mask_arg(kk...);
    __shared__ double red[3][4];
    if constexpr (MASK) {
        __shared__ long long cred[4];
        const int64_t nv = valid_count(k.counts, nb, cred);
        if (threadIdx.x == 0) k.n_valid[0] = nv;
        inv_n = nv ? 1.0 / (double)nv : 0.0;
    }
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) {
        s0 += stats[4 * i];
        s1 += stats[4 * i + 1];
        s2 += kind == TULIP_LOSS_BERHU ? vpart[i] : stats[4 * i + 2];
    }
    for (int o = 32; o > 0; o >>= 1) { s0 += __shfl_xor(s0, o, 64); s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s0; red[1][threadIdx.x >> 6] = s1; red[2][threadIdx.x >> 6] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double a = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        const double b = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
        const double c = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
        losses[0] = (float)((kind == TULIP_LOSS_L1 ? a : c) * inv_n);
        losses[1] = log_transform ? (float)(b * inv_n) : (float)(a * inv_n);
    }
}

inline bool bad_kind(int kind) { return kind != TULIP_LOSS_L1 && kind != TULIP_LOSS_L2 && kind != TULIP_LOSS_BERHU; }

// float4 groups in front of the scalar tail: all of n / 4 when every pointer is 16-byte aligned, none otherwise
inline int64_t vec_groups(int64_t n, const void* a, const void* b, const void* c = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) ? 0 : n >> 2;
}

// the mask of an _m call, checked: false for what TULIP_ERR_ARG refuses.  (n < 2^41: a workgroup's count fits its uint32)
inline bool make_mask(LossMask& k, int64_t n, int chans, int64_t chan_stride, float valid_min, const uint32_t* counts,
                      int64_t* n_valid, bool wants_n_valid) {
    if (chans < 1 || chan_stride < 1 || n <= 0 || n >= ((int64_t)1 << 41) || chan_stride > n / chans ||
        n % (chans * chan_stride) != 0)
        return false;
    if (!(valid_min - valid_min == 0.f) || !counts || ((uintptr_t)counts & 3)) return false;       // NaN, infinities
    if (wants_n_valid && (!n_valid || ((uintptr_t)n_valid & 7))) return false;
    k = LossMask{chan_stride, chans, n < ((int64_t)1 << 32), valid_min, const_cast<uint32_t*>(counts), n_valid};
    return true;
}

// the masked float4 route needs chan_stride % 4 == 0 besides the alignment (with target 16-byte aligned, its channel-0 rows then
// are too): a group then never straddles a channel
inline int64_t vec_groups_m(const LossMask* k, int64_t n, const void* a, const void* b, const void* c = nullptr) {
    return (k && (k->chan_stride & 3)) ? 0 : vec_groups(n, a, b, c);
}

int launch_stats(const float* pred, const float* target, float* stats, int64_t n, int log_transform, const LossMask* k,
                 hipStream_t stream) {
    if (n <= 0 || !pred || !target || !stats || ((uintptr_t)stats & 15)) return TULIP_ERR_ARG;
    const dim3 grid(tulip_loss_blocks(n)), block(256);
    const int64_t n4 = vec_groups_m(k, n, pred, target);
    if (k) hipLaunchKernelGGL(loss_stats_kernel<LossMask>, grid, block, 0, stream, pred, target, stats, n, n4, log_transform, *k);
    else hipLaunchKernelGGL(loss_stats_kernel<>, grid, block, 0, stream, pred, target, stats, n, n4, log_transform);
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

template <class... K>
void launch_bwd_kind(int kind, dim3 grid, hipStream_t stream, const float* pred, const float* target, const float* stats, int nb,
                     const float* gscale_dev, float gscale, float* dpred, float* loss_c, int64_t n, int64_t n4, K... k) {
    const dim3 block(256);
    if (kind == TULIP_LOSS_L1)
        hipLaunchKernelGGL((loss_bwd_kernel<TULIP_LOSS_L1, K...>), grid, block, 0, stream, pred, target, stats, nb, gscale_dev, gscale,
                           dpred, loss_c, n, n4, k...);
    else if (kind == TULIP_LOSS_L2)
        hipLaunchKernelGGL((loss_bwd_kernel<TULIP_LOSS_L2, K...>), grid, block, 0, stream, pred, target, stats, nb, gscale_dev, gscale,
                           dpred, loss_c, n, n4, k...);
    else
        hipLaunchKernelGGL((loss_bwd_kernel<TULIP_LOSS_BERHU, K...>), grid, block, 0, stream, pred, target, stats, nb, gscale_dev,
                           gscale, dpred, loss_c, n, n4, k...);
}

int launch_bwd(int kind, const float* pred, const float* target, const float* stats, const float* gscale_dev, float gscale,
               float* dpred, float* loss_c, int64_t n, const LossMask* k, hipStream_t stream) {
    if (bad_kind(kind) || n <= 0 || !pred || !target || !dpred) return TULIP_ERR_ARG;
    if (kind == TULIP_LOSS_BERHU && (!stats || !loss_c)) return TULIP_ERR_ARG;
    const int nb = tulip_loss_blocks(n);
    const int64_t n4 = vec_groups_m(k, n, pred, target, dpred);
    if (k) launch_bwd_kind(kind, dim3(nb), stream, pred, target, stats, nb, gscale_dev, gscale, dpred, loss_c, n, n4, *k);
    else launch_bwd_kind(kind, dim3(nb), stream, pred, target, stats, nb, gscale_dev, gscale, dpred, loss_c, n, n4);
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

int launch_value(const float* pred, const float* target, const float* stats, float* value_partials, int64_t n, const LossMask* k,
                 hipStream_t stream) {
    if (n <= 0 || !pred || !target || !stats || !value_partials) return TULIP_ERR_ARG;
    const int nb = tulip_loss_blocks(n);
    const int64_t n4 = vec_groups_m(k, n, pred, target);
    if (k) hipLaunchKernelGGL(loss_value_kernel<LossMask>, dim3(nb), dim3(256), 0, stream, pred, target, stats, nb, value_partials, n,
                              n4, *k);
    else hipLaunchKernelGGL(loss_value_kernel<>, dim3(nb), dim3(256), 0, stream, pred, target, stats, nb, value_partials, n, n4);
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

int launch_final(int kind, const float* stats, const float* value_partials, float* losses, int64_t n, int log_transform,
                 const LossMask* k, hipStream_t stream) {
    if (bad_kind(kind) || n <= 0 || !stats || !losses) return TULIP_ERR_ARG;
    if (kind == TULIP_LOSS_BERHU && !value_partials) return TULIP_ERR_ARG;
    const int nb = tulip_loss_blocks(n);
    if (k) hipLaunchKernelGGL(loss_final_kernel<LossMask>, dim3(1), dim3(256), 0, stream, kind, stats, value_partials, losses, nb, 0.0,
                              log_transform, *k);
    else hipLaunchKernelGGL(loss_final_kernel<>, dim3(1), dim3(256), 0, stream, kind, stats, value_partials, losses, nb,
                            1.0 / (double)n, log_transform);
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

// ---- the edge term, TULIP(loss_edge_weight=...) (tulip_amd/loss.py): the two 3x3 Sobel responses of d = pred - target per
// (b, c) plane, zero outside the plane, and their adjoint for the gradient.  Not element-wise: one workgroup of 256 threads takes
// one EDGE_TH x EDGE_TW tile of one plane (rows of 128 floats: coalesced along W), stages d for the tile plus its halo in LDS
// (a few KB) and loops workgroup-strided over the remaining tiles.  Thread t owns column t & 127 and the four rows 4 (t >> 7) + r
// of the tile.  Scalar loads and stores (the halo is unaligned anyway): one route whatever the pointers' alignment.
constexpr int EDGE_TH = 8, EDGE_TW = 128;

struct EdgeMask {
    int chans;                 // plane p belongs to sample p / chans, whose channel-0 plane decides validity
    float valid_min;
};

// The channel weights of the _w entry points (TULIP(loss_channel_weights=...)), by value in the launch arguments: w[c] of channel
// c < chans, 0 behind them.  Nothing on the device holds them, so nothing can rewrite them under a captured graph.
struct ChanW {
    float w0, w1, w2, w3;
};
// (a select chain, not an index: the argument stays in scalar registers)
__device__ __forceinline__ float chan_weight(int c, const ChanW& w) { return c == 0 ? w.w0 : c == 1 ? w.w1 : c == 2 ? w.w2 : w.w3; }

struct EdgeGeom {
    int H, W, tiles_x, tiles_y;
    int64_t tiles;             // planes * tiles_y * tiles_x
};

inline EdgeGeom edge_geom(int64_t planes, int H, int W) {
    EdgeGeom g{H, W, (W + EDGE_TW - 1) / EDGE_TW, (H + EDGE_TH - 1) / EDGE_TH, 0};
    g.tiles = planes * g.tiles_y * g.tiles_x;
    return g;
}

// d of tile (plane, y0, x0) with a HALO-pixel border into sd, row pitch EDGE_TW + 2 HALO: pred - target inside the plane, +0
// outside it -- the neighbouring row, plane and sample lie adjacent in memory and are never read for it -- and, MASK, +0 by
// selection at an invalid pixel.  ok[i] = 1 where entry i is inside the plane (MASK: and valid).  64-bit element offsets.
template <int HALO, bool MASK>
__device__ __forceinline__ void edge_stage(float* sd, uint8_t* ok, const float* __restrict__ pred, const float* __restrict__ tgt,
                                           int64_t plane, int y0, int x0, const EdgeGeom& g, const EdgeMask& k) {
    constexpr int PW = EDGE_TW + 2 * HALO, PH = EDGE_TH + 2 * HALO;
    const int64_t hw = (int64_t)g.H * g.W, base = plane * hw;
    int64_t base0 = base;
    if constexpr (MASK) base0 = (plane / k.chans) * k.chans * hw;
    for (int i = threadIdx.x; i < PW * PH; i += 256) {
        const int ly = i / PW, lx = i - ly * PW;
        const int gy = y0 + ly - HALO, gx = x0 + lx - HALO;
        float d = 0.f;
        uint8_t v = 0;
        if (gy >= 0 && gy < g.H && gx >= 0 && gx < g.W) {
            const int64_t off = (int64_t)gy * g.W + gx;
            if constexpr (MASK) v = tgt[base0 + off] > k.valid_min;
            else v = 1;
            if (v) d = pred[base + off] - tgt[base + off];
        }
        sd[i] = d;
        ok[i] = v;
    }
}

// the two responses centred on entry c of a staged tile of row pitch PW, in the fixed order of tulip_amd/loss.py (2 a is exact:
// an fma contraction of 2 a + b rounds as the two operations do)
template <int PW>
__device__ __forceinline__ void edge_responses(const float* sd, int c, float& eh, float& ev) {
    const float a = sd[c - PW - 1], b = sd[c - PW], cc = sd[c - PW + 1], l = sd[c - 1], r = sd[c + 1], e = sd[c + PW - 1],
                f = sd[c + PW], h = sd[c + PW + 1];
    eh = ((e - a) + 2.f * (f - b)) + (h - cc);
    ev = ((cc - a) + 2.f * (r - l)) + (h - e);
}

// fl32(c + fl32(a * b)): a multiply, then an add -- two roundings, as tulip_amd/loss.py states them.  (__fmul_rn / __fadd_rn are
// plain operators in HIP's headers and contract into an fma like any others; the pragma is what keeps them apart.)
__device__ __forceinline__ float mul_then_add(float a, float b, float c) {
#pragma clang fp contract(off)
    const float p = a * b;
    return c + p;
}

__device__ __forceinline__ void edge_tile(int64_t t, const EdgeGeom& g, int64_t& plane, int& y0, int& x0) {
    const int per = g.tiles_y * g.tiles_x;
    plane = t / per;
    const int r = (int)(t - plane * per), ty = r / g.tiles_x;
    y0 = ty * EDGE_TH;
    x0 = (r - ty * g.tiles_x) * EDGE_TW;
}

// edge_partials[wg] = the workgroup's sum of |e_h| + |e_v| over its tiles (MASK: over the responses centred on a valid pixel):
// per thread over its tiles and rows in order, the wave tree, four wave results.  WT: the terms fl32(w_c * fl32(|e_h| + |e_v|)), c
// the plane's channel (plane % k.chans); a plane with w_c == 0 is skipped -- nothing of it is read
template <bool MASK, bool WT>
__global__ __launch_bounds__(256) void edge_stats_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                         float* __restrict__ edge_partials, EdgeGeom g, EdgeMask k, ChanW cw) {
    constexpr int PW = EDGE_TW + 2;
    __shared__ float sd[(EDGE_TH + 2) * PW];
    __shared__ uint8_t ok[(EDGE_TH + 2) * PW];
    __shared__ float red[1][4];
    const int col = threadIdx.x & (EDGE_TW - 1), row0 = (threadIdx.x >> 7) * 4;
    float s = 0.f;
    for (int64_t t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        int64_t plane;
        int y0, x0;
        edge_tile(t, g, plane, y0, x0);
        float w = 1.f;
        if constexpr (WT) {
            w = chan_weight((int)(plane % k.chans), cw);
            if (!(w > 0.f)) continue;                  // (the same plane in every thread: a uniform skip)
        }
        edge_stage<1, MASK>(sd, ok, pred, tgt, plane, y0, x0, g, k);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = (row0 + r + 1) * PW + col + 1;
            if (ok[c]) {                               // inside the plane (and valid)
                float eh, ev;
                edge_responses<PW>(sd, c, eh, ev);
                if constexpr (WT) s = mul_then_add(w, fabsf(eh) + fabsf(ev), s);
                else s += fabsf(eh) + fabsf(ev);
            }
        }
        __syncthreads();
    }
    block_sum(s, red, 0);
    __syncthreads();
    if (threadIdx.x == 0) edge_partials[blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
}

// dpred[e] = fl32(dpred[e] + fl32(ge * k[e])), ge = fl32(weight * g) with g the base gradient's fl32(gscale / n) (MASK: n_v folded
// here from the counts; g = 0 when n_v == 0), k the adjoint taps over the two sign maps -- signs zeroed where their centre is
// outside the plane (MASK: or invalid); a NaN response has sign 0.  MASK: +0 at the invalid elements.  Every thread reads and
// writes its own elements of dpred only.  WT: n_S from the counts (masked or not), ge_c = fl32(weight * fl32(w_c * g)) per plane,
// and a plane with w_c == 0 is skipped: nothing of it is read, and dpred keeps the +0 the base gradient's launch wrote there.
template <bool MASK, bool WT>
__global__ __launch_bounds__(256) void edge_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                       const float* __restrict__ gscale_dev, float gscale, float weight,
                                                       float* __restrict__ dpred, int64_t n, const uint32_t* __restrict__ counts,
                                                       int nb_counts, EdgeGeom g, EdgeMask k, ChanW cw) {
    constexpr int PW2 = EDGE_TW + 4, PW1 = EDGE_TW + 2, N1 = (EDGE_TH + 2) * PW1;
    __shared__ float sd[(EDGE_TH + 4) * PW2];
    __shared__ uint8_t ok[(EDGE_TH + 4) * PW2];
    __shared__ int8_t sh[N1], sv[N1];
    float gg;
    if constexpr (MASK || WT) {
        __shared__ long long cred[4];
        const int64_t nv = valid_count(counts, nb_counts, cred);
        gg = nv ? (gscale_dev ? gscale_dev[0] : gscale) / (float)nv : 0.f;
    } else {
        gg = (gscale_dev ? gscale_dev[0] : gscale) / (float)n;
    }
    float ge = weight * gg;
    const int col = threadIdx.x & (EDGE_TW - 1), row0 = (threadIdx.x >> 7) * 4;
    const int64_t hw = (int64_t)g.H * g.W;
    for (int64_t t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        int64_t plane;
        int y0, x0;
        edge_tile(t, g, plane, y0, x0);
        if constexpr (WT) {
            const float w = chan_weight((int)(plane % k.chans), cw);
            if (!(w > 0.f)) continue;                  // (uniform)
            const float gc = w * gg;
            ge = weight * gc;
        }
        edge_stage<2, MASK>(sd, ok, pred, tgt, plane, y0, x0, g, k);
        __syncthreads();
        for (int i = threadIdx.x; i < N1; i += 256) {
            const int ly = i / PW1, lx = i - ly * PW1, c = (ly + 1) * PW2 + lx + 1;
            int8_t a = 0, b = 0;
            if (ok[c]) {
                float eh, ev;
                edge_responses<PW2>(sd, c, eh, ev);
                a = (int8_t)((eh > 0.f) - (eh < 0.f));
                b = (int8_t)((ev > 0.f) - (ev < 0.f));
            }
            sh[i] = a;
            sv[i] = b;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int y = y0 + row0 + r, x = x0 + col;
            if (y < g.H && x < g.W) {
                const int c = (row0 + r + 1) * PW1 + col + 1;
                const int kh = ((int)sh[c - PW1 + 1] + 2 * (int)sh[c - PW1] + (int)sh[c - PW1 - 1]) -
                               ((int)sh[c + PW1 + 1] + 2 * (int)sh[c + PW1] + (int)sh[c + PW1 - 1]);
                const int kv = ((int)sv[c + PW1 - 1] + 2 * (int)sv[c - 1] + (int)sv[c - PW1 - 1]) -
                               ((int)sv[c + PW1 + 1] + 2 * (int)sv[c + 1] + (int)sv[c - PW1 + 1]);
                const int64_t e = plane * hw + (int64_t)y * g.W + x;
                float out = mul_then_add(ge, (float)(kh + kv), dpred[e]);
                if constexpr (MASK) {
                    if (!ok[(row0 + r + 2) * PW2 + col + 2]) out = 0.f;
                }
                dpred[e] = out;
            }
        }
        __syncthreads();                               // the next tile's staging rewrites ok, which the taps above still read
    }
}

// one workgroup: the partials folded in double (loss_final_kernel's order); edge_out[0] = edge32 = fl32(sum * inv_n) and
// losses[0] = fl32(losses[0] + fl32(weight * edge32)) behind the base loss's final launch.  MASK: inv_n = 1 / n_v from the counts
template <bool MASK>
__global__ __launch_bounds__(256) void edge_final_kernel(const float* __restrict__ edge_partials, int nb, float* __restrict__ edge_out,
                                                         float* __restrict__ losses, float weight, double inv_n,
                                                         const uint32_t* __restrict__ counts, int nb_counts) {
    __shared__ double red[4];
    if constexpr (MASK) {
        __shared__ long long cred[4];
        const int64_t nv = valid_count(counts, nb_counts, cred);
        inv_n = nv ? 1.0 / (double)nv : 0.0;
    }
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) s += edge_partials[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float edge32 = (float)(((red[0] + red[1]) + (red[2] + red[3])) * inv_n);
        edge_out[0] = edge32;
        losses[0] = mul_then_add(weight, edge32, losses[0]);
    }
}

inline bool bad_weight(float w) { return !(w >= 0.f) || !(w - w == 0.f); }       // negative, NaN, infinite

// the geometry of an edge call, checked (n = planes * H * W < 2^41 as in make_mask: planes * tiles per plane then fits int64 too)
inline bool make_edge(EdgeGeom& g, int64_t& n, int64_t planes, int H, int W) {
    if (planes <= 0 || H <= 0 || W <= 0) return false;
    if (planes > (((int64_t)1 << 41) - 1) / H / W) return false;
    // the kernels' tile and pixel coordinates are 32-bit: the halo must not carry y0 + ly or x0 + lx past INT_MAX, and the
    // tiles of one plane must be countable in an int
    if (H > INT_MAX - 16 || W > INT_MAX - EDGE_TW - 16) return false;
    if ((int64_t)((H + EDGE_TH - 1) / EDGE_TH) * ((W + EDGE_TW - 1) / EDGE_TW) >= ((int64_t)1 << 31)) return false;
    n = planes * H * W;
    g = edge_geom(planes, H, W);
    return true;
}

inline bool make_edge_mask(EdgeMask& k, int64_t planes, int chans, float valid_min) {
    if (chans < 1 || planes % chans != 0 || !(valid_min - valid_min == 0.f)) return false;
    k = EdgeMask{chans, valid_min};
    return true;
}

inline int edge_grid(const EdgeGeom& g) { return (int)(g.tiles > LOSS_BLOCKS ? LOSS_BLOCKS : g.tiles); }

// cw: the weighted kernels (k then carries the channel count whether `masked` or not)
int launch_edge_stats(const float* pred, const float* target, float* edge_partials, int64_t planes, int H, int W,
                      const EdgeMask* k, hipStream_t stream, const ChanW* cw = nullptr, bool masked = true) {
    EdgeGeom g;
    int64_t n;
    if (!make_edge(g, n, planes, H, W) || !pred || !target || !edge_partials || ((uintptr_t)edge_partials & 3)) return TULIP_ERR_ARG;
    const dim3 grid(edge_grid(g)), block(256);
    if (cw && masked) hipLaunchKernelGGL((edge_stats_kernel<true, true>), grid, block, 0, stream, pred, target, edge_partials, g, *k, *cw);
    else if (cw) hipLaunchKernelGGL((edge_stats_kernel<false, true>), grid, block, 0, stream, pred, target, edge_partials, g, *k, *cw);
    else if (k) hipLaunchKernelGGL((edge_stats_kernel<true, false>), grid, block, 0, stream, pred, target, edge_partials, g, *k, ChanW{});
    else hipLaunchKernelGGL((edge_stats_kernel<false, false>), grid, block, 0, stream, pred, target, edge_partials, g, EdgeMask{1, 0.f},
                            ChanW{});
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

int launch_edge_bwd(const float* pred, const float* target, const float* gscale_dev, float gscale, float weight, float* dpred,
                    int64_t planes, int H, int W, const EdgeMask* k, const uint32_t* counts, hipStream_t stream,
                    const ChanW* cw = nullptr, bool masked = true) {
    EdgeGeom g;
    int64_t n;
    if (!make_edge(g, n, planes, H, W) || !pred || !target || !dpred || bad_weight(weight)) return TULIP_ERR_ARG;
    if (k && (!counts || ((uintptr_t)counts & 3))) return TULIP_ERR_ARG;
    const dim3 grid(edge_grid(g)), block(256);
    if (cw && masked) hipLaunchKernelGGL((edge_bwd_kernel<true, true>), grid, block, 0, stream, pred, target, gscale_dev, gscale, weight,
                                         dpred, n, counts, tulip_loss_blocks(n), g, *k, *cw);
    else if (cw) hipLaunchKernelGGL((edge_bwd_kernel<false, true>), grid, block, 0, stream, pred, target, gscale_dev, gscale, weight,
                                    dpred, n, counts, tulip_loss_blocks(n), g, *k, *cw);
    else if (k) hipLaunchKernelGGL((edge_bwd_kernel<true, false>), grid, block, 0, stream, pred, target, gscale_dev, gscale, weight, dpred,
                                   n, counts, tulip_loss_blocks(n), g, *k, ChanW{});
    else hipLaunchKernelGGL((edge_bwd_kernel<false, false>), grid, block, 0, stream, pred, target, gscale_dev, gscale, weight, dpred, n,
                            (const uint32_t*)nullptr, 0, g, EdgeMask{1, 0.f}, ChanW{});
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

int launch_edge_final(const float* edge_partials, float* edge_out, float* losses, float weight, int64_t planes, int H, int W,
                      bool masked, const uint32_t* counts, hipStream_t stream) {
    EdgeGeom g;
    int64_t n;
    if (!make_edge(g, n, planes, H, W) || !edge_partials || ((uintptr_t)edge_partials & 3) || !edge_out || !losses || bad_weight(weight))
        return TULIP_ERR_ARG;
    if (masked && (!counts || ((uintptr_t)counts & 3))) return TULIP_ERR_ARG;
    if (masked) hipLaunchKernelGGL(edge_final_kernel<true>, dim3(1), dim3(256), 0, stream, edge_partials, edge_grid(g), edge_out, losses,
                                   weight, 0.0, counts, tulip_loss_blocks(n));
    else hipLaunchKernelGGL(edge_final_kernel<false>, dim3(1), dim3(256), 0, stream, edge_partials, edge_grid(g), edge_out, losses,
                            weight, 1.0 / (double)n, (const uint32_t*)nullptr, 0);
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

// ---- the channel weights, TULIP(loss_channel_weights=(w_0, ..)) (tulip_amd/loss.py): the flat kernels again with element e of
// channel c = (e / chan_stride) % chans COUNTED iff w_c > 0 and (masked) its pixel is valid.  One family for the unmasked and the
// masked case (`masked` at run time); the counted elements are always counted in integers (k.m.counts), and n_S, their sum, stands
// where n / n_v stand above.  stats[4 wg + {0, 1, 2, 3}] = {sum w_c |d|, the UNWEIGHTED metric sum (|expm1 p - expm1 t| with
// log_transform, |d| without), sum w_c d^2, max |d|} over the counted elements: the weighted L1 value and the metric are different
// sums now, so the second slot is always filled and the final fold (loss_final_kernel<LossMask>) always reads it.
// Threads take the elements the kernels above give them -- groups of four where the pointers are 16-byte aligned (masked: and
// chan_stride % 4 == 0), a scalar tail -- so that the reduction orders, and with all weights 1 every bit, are theirs.  A group is
// loaded as a float4 only where it lies in one channel (vec: chan_stride % 4 == 0); elsewhere by four scalar loads, each element
// with its own channel.
struct LossW {
    LossMask m;
    ChanW w;
    int masked;
    int vec;
};

__device__ __forceinline__ float weight_at(int64_t e, const LossW& k) {
    int c;
    if (k.m.narrow) c = (int)(((uint32_t)e / (uint32_t)k.m.chan_stride) % (uint32_t)k.m.chans);
    else c = (int)((e / k.m.chan_stride) % k.m.chans);
    return chan_weight(c, k.w);
}
__device__ __forceinline__ float4 weights4(int64_t e, const LossW& k) {
    if (k.vec) {
        const float w = weight_at(e, k);
        return make_float4(w, w, w, w);
    }
    return make_float4(weight_at(e, k), weight_at(e + 1, k), weight_at(e + 2, k), weight_at(e + 3, k));
}
__device__ __forceinline__ float4 load4(const float* __restrict__ a, int64_t e, const LossW& k) {
    if (k.vec) return *(const float4*)(a + e);
    return make_float4(a[e], a[e + 1], a[e + 2], a[e + 3]);
}
// counted: w > 0 and, masked, the pixel valid (a masked group is always a float4 group: vec_groups_m)
struct Counted {
    bool x, y, z, w;
};
__device__ __forceinline__ Counted counted4(const float* __restrict__ tgt, int64_t e, float4 t, float4 w, const LossW& k) {
    Counted c{w.x > 0.f, w.y > 0.f, w.z > 0.f, w.w > 0.f};
    if (k.masked) {
        const float4 z = mask_src4(tgt, e, t, k.m);
        c = Counted{c.x && z.x > k.m.valid_min, c.y && z.y > k.m.valid_min, c.z && z.z > k.m.valid_min, c.w && z.w > k.m.valid_min};
    }
    return c;
}
__device__ __forceinline__ bool counted1(const float* __restrict__ tgt, int64_t e, float t, float w, const LossW& k) {
    return w > 0.f && (!k.masked || mask_src(tgt, e, t, k.m) > k.m.valid_min);
}

struct LossAccW {
    float abs = 0.f, pix = 0.f, sq = 0.f, mx = 0.f;
    uint32_t cnt = 0;
    // an element that is not counted enters nothing, whatever p and t hold there
    __device__ __forceinline__ void add_if(bool counted, float w, float p, float t, int log_transform) {
        if (counted) {
            const float d = p - t, a = fabsf(d);
            abs = mul_then_add(w, a, abs);
            pix += log_transform ? fabsf(expm1f(p) - expm1f(t)) : a;
            sq += (w * d) * d;
            mx = nan_max(mx, a);
            ++cnt;
        }
    }
};

__global__ __launch_bounds__(256) void loss_stats_w_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                           float* __restrict__ stats, int64_t n, int64_t n4, int log_transform,
                                                           LossW k) {
    __shared__ float red[4][4];
    __shared__ uint32_t cred[4];
    LossAccW s;
    const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = first; i < n4; i += stride) {
        const float4 p = load4(pred, i * 4, k), t = load4(tgt, i * 4, k), w = weights4(i * 4, k);
        const Counted c = counted4(tgt, i * 4, t, w, k);
        s.add_if(c.x, w.x, p.x, t.x, log_transform); s.add_if(c.y, w.y, p.y, t.y, log_transform);
        s.add_if(c.z, w.z, p.z, t.z, log_transform); s.add_if(c.w, w.w, p.w, t.w, log_transform);
    }
    for (int64_t i = n4 * 4 + first; i < n; i += stride) {
        const float w = weight_at(i, k), t = tgt[i];
        s.add_if(counted1(tgt, i, t, w, k), w, pred[i], t, log_transform);
    }
    uint32_t c = s.cnt;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) cred[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) k.m.counts[blockIdx.x] = (cred[0] + cred[1]) + (cred[2] + cred[3]);
    block_sum(s.abs, red, 0);
    block_sum(s.pix, red, 1);
    block_sum(s.sq, red, 2);
    const float m = group_reduce<64>(s.mx, [](float a, float b) { return nan_max(a, b); });
    if ((threadIdx.x & 63) == 0) red[3][threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        *(float4*)(stats + 4 * (size_t)blockIdx.x) =
            make_float4((red[0][0] + red[0][1]) + (red[0][2] + red[0][3]), (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]),
                        (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]),
                        nan_max(nan_max(red[3][0], red[3][1]), nan_max(red[3][2], red[3][3])));
    }
}

// dpred[i] = grad_kind(d_i; C) with g_c = fl32(w_c * g) where g stands above, g = fl32(gscale / n_S) (0 when n_S == 0); +0 at the
// elements that are not counted.  n_S is written to k.m.n_valid
template <int KIND>
__global__ __launch_bounds__(256) void loss_bwd_w_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                         const float* __restrict__ stats, int nb,
                                                         const float* __restrict__ gscale_dev, float gscale,
                                                         float* __restrict__ dpred, float* __restrict__ loss_c, int64_t n,
                                                         int64_t n4, LossW k) {
    __shared__ float red[4];
    __shared__ long long cred[4];
    float C = 0.f;
    if constexpr (KIND == TULIP_LOSS_BERHU) {
        C = berhu_threshold(stats, nb, red);
        if (blockIdx.x == 0 && threadIdx.x == 0) loss_c[0] = C;
    }
    const int64_t nv = valid_count(k.m.counts, nb, cred);
    if (blockIdx.x == 0 && threadIdx.x == 0) k.m.n_valid[0] = nv;
    const float g = nv ? (gscale_dev ? gscale_dev[0] : gscale) / (float)nv : 0.f;
    const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = first; i < n4; i += stride) {
        const float4 p = load4(pred, i * 4, k), t = load4(tgt, i * 4, k), w = weights4(i * 4, k);
        const Counted c = counted4(tgt, i * 4, t, w, k);
        const float4 d = make_float4(c.x ? loss_grad<KIND>(p.x, t.x, C, w.x * g) : 0.f, c.y ? loss_grad<KIND>(p.y, t.y, C, w.y * g) : 0.f,
                                     c.z ? loss_grad<KIND>(p.z, t.z, C, w.z * g) : 0.f, c.w ? loss_grad<KIND>(p.w, t.w, C, w.w * g) : 0.f);
        if (k.vec) {
            *(float4*)(dpred + i * 4) = d;
        } else {
            dpred[i * 4] = d.x; dpred[i * 4 + 1] = d.y; dpred[i * 4 + 2] = d.z; dpred[i * 4 + 3] = d.w;
        }
    }
    for (int64_t i = n4 * 4 + first; i < n; i += stride) {
        const float w = weight_at(i, k), t = tgt[i];
        dpred[i] = counted1(tgt, i, t, w, k) ? loss_grad<KIND>(pred[i], t, C, w * g) : 0.f;
    }
}

// berHu's second pass: vpart[wg] = the workgroup's sum of fl32(w_c * value) over the counted elements (n_S == 0: nothing is read)
__global__ __launch_bounds__(256) void loss_value_w_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                           const float* __restrict__ stats, int nb, float* __restrict__ vpart,
                                                           int64_t n, int64_t n4, LossW k) {
    __shared__ float red[4];
    __shared__ float sum[1][4];
    __shared__ long long cred[4];
    if (valid_count(k.m.counts, nb, cred) == 0) {          // (the same n_S in every thread: a uniform exit)
        if (threadIdx.x == 0) vpart[blockIdx.x] = 0.f;
        return;
    }
    const float C = berhu_threshold(stats, nb, red);
    float s = 0.f;
    const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = first; i < n4; i += stride) {
        const float4 p = load4(pred, i * 4, k), t = load4(tgt, i * 4, k), w = weights4(i * 4, k);
        const Counted c = counted4(tgt, i * 4, t, w, k);
        if (c.x) s = mul_then_add(w.x, berhu_value(p.x - t.x, C), s);
        if (c.y) s = mul_then_add(w.y, berhu_value(p.y - t.y, C), s);
        if (c.z) s = mul_then_add(w.z, berhu_value(p.z - t.z, C), s);
        if (c.w) s = mul_then_add(w.w, berhu_value(p.w - t.w, C), s);
    }
    for (int64_t i = n4 * 4 + first; i < n; i += stride) {
        const float w = weight_at(i, k), t = tgt[i];
        if (counted1(tgt, i, t, w, k)) s = mul_then_add(w, berhu_value(pred[i] - t, C), s);
    }
    block_sum(s, sum, 0);
    __syncthreads();
    if (threadIdx.x == 0) vpart[blockIdx.x] = (sum[0][0] + sum[0][1]) + (sum[0][2] + sum[0][3]);
}

// the weights of a _w call, checked: false for what TULIP_ERR_ARG refuses
inline bool make_chan_w(ChanW& cw, const float* weights, int chans) {
    if (chans < 1 || chans > 4 || !weights) return false;
    float w[4] = {0.f, 0.f, 0.f, 0.f};
    bool any = false;
    for (int c = 0; c < chans; ++c) {
        if (bad_weight(weights[c])) return false;
        w[c] = weights[c];
        any = any || w[c] > 0.f;
    }
    if (!any) return false;
    cw = ChanW{w[0], w[1], w[2], w[3]};
    return true;
}

inline bool make_loss_w(LossW& k, int64_t n, int chans, int64_t chan_stride, const float* weights, int masked, float valid_min,
                        const uint32_t* counts, int64_t* n_valid, bool wants_n_valid) {
    ChanW cw;
    if (!make_chan_w(cw, weights, chans)) return false;
    LossMask m;
    if (!make_mask(m, n, chans, chan_stride, masked ? valid_min : 0.f, counts, n_valid, wants_n_valid)) return false;
    k = LossW{m, cw, masked != 0, (chan_stride & 3) == 0};
    return true;
}

// the groups of the kernels above for the same pointers: masked the _m rule, unmasked the alignment alone
inline int64_t groups_w(const LossW& k, int64_t n, const void* a, const void* b, const void* c = nullptr) {
    return k.masked ? vec_groups_m(&k.m, n, a, b, c) : vec_groups(n, a, b, c);
}

int launch_stats_w(const float* pred, const float* target, float* stats, int64_t n, int log_transform, const LossW& k,
                   hipStream_t stream) {
    if (n <= 0 || !pred || !target || !stats || ((uintptr_t)stats & 15)) return TULIP_ERR_ARG;
    hipLaunchKernelGGL(loss_stats_w_kernel, dim3(tulip_loss_blocks(n)), dim3(256), 0, stream, pred, target, stats, n,
                       groups_w(k, n, pred, target), log_transform, k);
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

int launch_bwd_w(int kind, const float* pred, const float* target, const float* stats, const float* gscale_dev, float gscale,
                 float* dpred, float* loss_c, int64_t n, const LossW& k, hipStream_t stream) {
    if (bad_kind(kind) || n <= 0 || !pred || !target || !dpred) return TULIP_ERR_ARG;
    if (kind == TULIP_LOSS_BERHU && (!stats || !loss_c)) return TULIP_ERR_ARG;
    const int nb = tulip_loss_blocks(n);
    const int64_t n4 = groups_w(k, n, pred, target, dpred);
    const dim3 grid(nb), block(256);
    if (kind == TULIP_LOSS_L1)
        hipLaunchKernelGGL(loss_bwd_w_kernel<TULIP_LOSS_L1>, grid, block, 0, stream, pred, target, stats, nb, gscale_dev, gscale, dpred,
                           loss_c, n, n4, k);
    else if (kind == TULIP_LOSS_L2)
        hipLaunchKernelGGL(loss_bwd_w_kernel<TULIP_LOSS_L2>, grid, block, 0, stream, pred, target, stats, nb, gscale_dev, gscale, dpred,
                           loss_c, n, n4, k);
    else
        hipLaunchKernelGGL(loss_bwd_w_kernel<TULIP_LOSS_BERHU>, grid, block, 0, stream, pred, target, stats, nb, gscale_dev, gscale,
                           dpred, loss_c, n, n4, k);
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

int launch_value_w(const float* pred, const float* target, const float* stats, float* value_partials, int64_t n, const LossW& k,
                   hipStream_t stream) {
    if (n <= 0 || !pred || !target || !stats || !value_partials) return TULIP_ERR_ARG;
    const int nb = tulip_loss_blocks(n);
    hipLaunchKernelGGL(loss_value_w_kernel, dim3(nb), dim3(256), 0, stream, pred, target, stats, nb, value_partials, n,
                       groups_w(k, n, pred, target), k);
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

}  // namespace

extern "C" int tulip_loss_blocks(int64_t n) {
    if (n <= 0) return 0;
    const int64_t b = ((n + 3) / 4 + 255) / 256;
    return (int)(b > LOSS_BLOCKS ? LOSS_BLOCKS : b);
}

extern "C" int tulip_loss_stats(const float* pred, const float* target, float* stats, int64_t n, int log_transform,
                                hipStream_t stream) {
    return launch_stats(pred, target, stats, n, log_transform, nullptr, stream);
}

extern "C" int tulip_loss_bwd(int kind, const float* pred, const float* target, const float* stats, const float* gscale_dev,
                              float gscale, float* dpred, float* loss_c, int64_t n, hipStream_t stream) {
    return launch_bwd(kind, pred, target, stats, gscale_dev, gscale, dpred, loss_c, n, nullptr, stream);
}

extern "C" int tulip_loss_value(const float* pred, const float* target, const float* stats, float* value_partials, int64_t n,
                                hipStream_t stream) {
    return launch_value(pred, target, stats, value_partials, n, nullptr, stream);
}

extern "C" int tulip_loss_final(int kind, const float* stats, const float* value_partials, float* losses, int64_t n,
                                int log_transform, hipStream_t stream) {
    return launch_final(kind, stats, value_partials, losses, n, log_transform, nullptr, stream);
}

// ---- the masked entry points: the same launches over the valid elements (LossMask above)
extern "C" int tulip_loss_stats_m(const float* pred, const float* target, float* stats, int64_t n, int log_transform, int chans,
                                  int64_t chan_stride, float valid_min, uint32_t* counts, hipStream_t stream) {
    LossMask k;
    if (!make_mask(k, n, chans, chan_stride, valid_min, counts, nullptr, false)) return TULIP_ERR_ARG;
    return launch_stats(pred, target, stats, n, log_transform, &k, stream);
}

extern "C" int tulip_loss_bwd_m(int kind, const float* pred, const float* target, const float* stats, const float* gscale_dev,
                                float gscale, float* dpred, float* loss_c, int64_t n, int chans, int64_t chan_stride,
                                float valid_min, const uint32_t* counts, int64_t* n_valid, hipStream_t stream) {
    LossMask k;
    if (!make_mask(k, n, chans, chan_stride, valid_min, counts, n_valid, true)) return TULIP_ERR_ARG;
    return launch_bwd(kind, pred, target, stats, gscale_dev, gscale, dpred, loss_c, n, &k, stream);
}

extern "C" int tulip_loss_value_m(const float* pred, const float* target, const float* stats, float* value_partials, int64_t n,
                                  int chans, int64_t chan_stride, float valid_min, const uint32_t* counts, hipStream_t stream) {
    LossMask k;
    if (!make_mask(k, n, chans, chan_stride, valid_min, counts, nullptr, false)) return TULIP_ERR_ARG;
    return launch_value(pred, target, stats, value_partials, n, &k, stream);
}

extern "C" int tulip_loss_final_m(int kind, const float* stats, const float* value_partials, float* losses, int64_t n,
                                  int log_transform, const uint32_t* counts, int64_t* n_valid, hipStream_t stream) {
    LossMask k;
    if (!make_mask(k, n, 1, 1, 0.f, counts, n_valid, true)) return TULIP_ERR_ARG;
    return launch_final(kind, stats, value_partials, losses, n, log_transform, &k, stream);
}

// ---- the edge term (TULIP(loss_edge_weight=...)): three launches behind the base loss's, each with a masked twin
extern "C" int tulip_loss_edge_blocks(int64_t planes, int H, int W) {
    EdgeGeom g;
    int64_t n;
    return make_edge(g, n, planes, H, W) ? edge_grid(g) : 0;
}

extern "C" int tulip_loss_edge_stats(const float* pred, const float* target, float* edge_partials, int64_t planes, int H, int W,
                                     hipStream_t stream) {
    return launch_edge_stats(pred, target, edge_partials, planes, H, W, nullptr, stream);
}

extern "C" int tulip_loss_edge_bwd(const float* pred, const float* target, const float* gscale_dev, float gscale, float weight,
                                   float* dpred, int64_t planes, int H, int W, hipStream_t stream) {
    return launch_edge_bwd(pred, target, gscale_dev, gscale, weight, dpred, planes, H, W, nullptr, nullptr, stream);
}

extern "C" int tulip_loss_edge_final(const float* edge_partials, float* edge_out, float* losses, float weight, int64_t planes, int H,
                                     int W, hipStream_t stream) {
    return launch_edge_final(edge_partials, edge_out, losses, weight, planes, H, W, false, nullptr, stream);
}

extern "C" int tulip_loss_edge_stats_m(const float* pred, const float* target, float* edge_partials, int64_t planes, int H, int W,
                                       int chans, float valid_min, hipStream_t stream) {
    EdgeMask k;
    if (!make_edge_mask(k, planes, chans, valid_min)) return TULIP_ERR_ARG;
    return launch_edge_stats(pred, target, edge_partials, planes, H, W, &k, stream);
}

extern "C" int tulip_loss_edge_bwd_m(const float* pred, const float* target, const float* gscale_dev, float gscale, float weight,
                                     float* dpred, int64_t planes, int H, int W, int chans, float valid_min,
                                     const uint32_t* counts, hipStream_t stream) {
    EdgeMask k;
    if (!make_edge_mask(k, planes, chans, valid_min)) return TULIP_ERR_ARG;
    return launch_edge_bwd(pred, target, gscale_dev, gscale, weight, dpred, planes, H, W, &k, counts, stream);
}

extern "C" int tulip_loss_edge_final_m(const float* edge_partials, float* edge_out, float* losses, float weight, int64_t planes,
                                       int H, int W, const uint32_t* counts, hipStream_t stream) {
    return launch_edge_final(edge_partials, edge_out, losses, weight, planes, H, W, true, counts, stream);
}

// ---- the weighted entry points (TULIP(loss_channel_weights=...)): `weights` is a HOST array of `chans` floats, copied into the
// launch arguments here
extern "C" int tulip_loss_stats_w(const float* pred, const float* target, float* stats, int64_t n, int log_transform, int chans,
                                  int64_t chan_stride, const float* weights, int masked, float valid_min, uint32_t* counts,
                                  hipStream_t stream) {
    LossW k;
    if (!make_loss_w(k, n, chans, chan_stride, weights, masked, valid_min, counts, nullptr, false)) return TULIP_ERR_ARG;
    return launch_stats_w(pred, target, stats, n, log_transform, k, stream);
}

extern "C" int tulip_loss_bwd_w(int kind, const float* pred, const float* target, const float* stats, const float* gscale_dev,
                                float gscale, float* dpred, float* loss_c, int64_t n, int chans, int64_t chan_stride,
                                const float* weights, int masked, float valid_min, const uint32_t* counts, int64_t* n_valid,
                                hipStream_t stream) {
    LossW k;
    if (!make_loss_w(k, n, chans, chan_stride, weights, masked, valid_min, counts, n_valid, true)) return TULIP_ERR_ARG;
    return launch_bwd_w(kind, pred, target, stats, gscale_dev, gscale, dpred, loss_c, n, k, stream);
}

extern "C" int tulip_loss_value_w(const float* pred, const float* target, const float* stats, float* value_partials, int64_t n,
                                  int chans, int64_t chan_stride, const float* weights, int masked, float valid_min,
                                  const uint32_t* counts, hipStream_t stream) {
    LossW k;
    if (!make_loss_w(k, n, chans, chan_stride, weights, masked, valid_min, counts, nullptr, false)) return TULIP_ERR_ARG;
    return launch_value_w(pred, target, stats, value_partials, n, k, stream);
}

// (stats' second slot is the metric sum whatever log_transform was: the masked fold, reading that slot)
extern "C" int tulip_loss_final_w(int kind, const float* stats, const float* value_partials, float* losses, int64_t n,
                                  const uint32_t* counts, int64_t* n_valid, hipStream_t stream) {
    LossMask k;
    if (!make_mask(k, n, 1, 1, 0.f, counts, n_valid, true)) return TULIP_ERR_ARG;
    return launch_final(kind, stats, value_partials, losses, n, 1, &k, stream);
}

inline bool make_edge_w(EdgeMask& k, ChanW& cw, int64_t planes, int chans, const float* weights, int masked, float valid_min) {
    return make_chan_w(cw, weights, chans) && make_edge_mask(k, planes, chans, masked ? valid_min : 0.f);
}

extern "C" int tulip_loss_edge_stats_w(const float* pred, const float* target, float* edge_partials, int64_t planes, int H, int W,
                                       int chans, const float* weights, int masked, float valid_min, hipStream_t stream) {
    EdgeMask k;
    ChanW cw;
    if (!make_edge_w(k, cw, planes, chans, weights, masked, valid_min)) return TULIP_ERR_ARG;
    return launch_edge_stats(pred, target, edge_partials, planes, H, W, &k, stream, &cw, masked != 0);
}

extern "C" int tulip_loss_edge_bwd_w(const float* pred, const float* target, const float* gscale_dev, float gscale, float weight,
                                     float* dpred, int64_t planes, int H, int W, int chans, const float* weights, int masked,
                                     float valid_min, const uint32_t* counts, hipStream_t stream) {
    EdgeMask k;
    ChanW cw;
    if (!make_edge_w(k, cw, planes, chans, weights, masked, valid_min)) return TULIP_ERR_ARG;
    return launch_edge_bwd(pred, target, gscale_dev, gscale, weight, dpred, planes, H, W, &k, counts, stream, &cw, masked != 0);
}

extern "C" int tulip_loss_edge_final_w(const float* edge_partials, float* edge_out, float* losses, float weight, int64_t planes,
                                       int H, int W, const uint32_t* counts, hipStream_t stream) {
    return launch_edge_final(edge_partials, edge_out, losses, weight, planes, H, W, true, counts, stream);
}

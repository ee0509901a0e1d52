// The selectable training loss, TULIP(loss="l2" | "berhu") (tulip_amd/loss.py is the host definition): four flat, HBM-bound
// kernels over n = pred.numel() elements.  float4 loads where pred / target (/ dpred) are 16-byte aligned, a scalar tail behind
// them; at most 1024 workgroups of 256 threads; every reduction in a fixed order (per-thread grid-stride sums, the wave tree,
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

struct LossAcc {
    float abs = 0.f, pix = 0.f, sq = 0.f, mx = 0.f;
    __device__ __forceinline__ void add(float p, float t, int log_transform) {
        const float d = p - t, a = fabsf(d);
        abs += a;
        if (log_transform) pix += fabsf(expm1f(p) - expm1f(t));
        sq += d * d;
        mx = nan_max(mx, a);
    }
};

// stats[4 wg + {0, 1, 2, 3}] = {sum |d|, sum |expm1 p - expm1 t| (log_transform, else 0), sum d^2, max |d|} of the workgroup
__global__ __launch_bounds__(256) void loss_stats_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                         float* __restrict__ stats, int64_t n, int64_t n4, int log_transform) {
    __shared__ float red[4][4];
    LossAcc s;
    const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = first; i < n4; i += stride) {
        const float4 p = *(const float4*)(pred + i * 4), t = *(const float4*)(tgt + i * 4);
        s.add(p.x, t.x, log_transform); s.add(p.y, t.y, log_transform);
        s.add(p.z, t.z, log_transform); s.add(p.w, t.w, log_transform);
    }
    for (int64_t i = n4 * 4 + first; i < n; i += stride) s.add(pred[i], tgt[i], log_transform);
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

// dpred[i] = g * grad_kind(d_i; C), g = gscale / n (one rounding, as in tulip_l1_loss_bwd)
template <int KIND>
__global__ __launch_bounds__(256) void loss_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                       const float* __restrict__ stats, int nb,
                                                       const float* __restrict__ gscale_dev, float gscale,
                                                       float* __restrict__ dpred, float* __restrict__ loss_c, int64_t n,
                                                       int64_t n4) {
    __shared__ float red[4];
    float C = 0.f;
    if constexpr (KIND == TULIP_LOSS_BERHU) {
        C = berhu_threshold(stats, nb, red);
        if (blockIdx.x == 0 && threadIdx.x == 0) loss_c[0] = C;
    }
    const float g = (gscale_dev ? gscale_dev[0] : gscale) / (float)n;
    const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = first; i < n4; i += stride) {
        const float4 p = *(const float4*)(pred + i * 4), t = *(const float4*)(tgt + i * 4);
        *(float4*)(dpred + i * 4) = make_float4(loss_grad<KIND>(p.x, t.x, C, g), loss_grad<KIND>(p.y, t.y, C, g),
                                                loss_grad<KIND>(p.z, t.z, C, g), loss_grad<KIND>(p.w, t.w, C, g));
    }
    for (int64_t i = n4 * 4 + first; i < n; i += stride) dpred[i] = loss_grad<KIND>(pred[i], tgt[i], C, g);
}

// berHu's second pass: vpart[wg] = the workgroup's sum of the elementwise values (the sum needs C)
__global__ __launch_bounds__(256) void loss_value_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                         const float* __restrict__ stats, int nb, float* __restrict__ vpart,
                                                         int64_t n, int64_t n4) {
    __shared__ float red[4];
    __shared__ float sum[1][4];
    const float C = berhu_threshold(stats, nb, red);
    float s = 0.f;
    const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = first; i < n4; i += stride) {
        const float4 p = *(const float4*)(pred + i * 4), t = *(const float4*)(tgt + i * 4);
        s += berhu_value(p.x - t.x, C); s += berhu_value(p.y - t.y, C);
        s += berhu_value(p.z - t.z, C); s += berhu_value(p.w - t.w, C);
    }
    for (int64_t i = n4 * 4 + first; i < n; i += stride) s += berhu_value(pred[i] - tgt[i], C);
    block_sum(s, sum, 0);
    __syncthreads();
    if (threadIdx.x == 0) vpart[blockIdx.x] = (sum[0][0] + sum[0][1]) + (sum[0][2] + sum[0][3]);
}

// one workgroup: the partials folded in double (l1_final_kernel's order); losses[0] = the chosen loss, losses[1] = pixel_loss
__global__ __launch_bounds__(256) void loss_final_kernel(int kind, const float* __restrict__ stats,
                                                         const float* __restrict__ vpart, float* __restrict__ losses, int nb,
                                                         double inv_n, int log_transform) {
    __shared__ double red[3][4];
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

}  // namespace

extern "C" int tulip_loss_blocks(int64_t n) {
    if (n <= 0) return 0;
    const int64_t b = ((n + 3) / 4 + 255) / 256;
    return (int)(b > LOSS_BLOCKS ? LOSS_BLOCKS : b);
}

extern "C" int tulip_loss_stats(const float* pred, const float* target, float* stats, int64_t n, int log_transform,
                                hipStream_t stream) {
    if (n <= 0 || !pred || !target || !stats || ((uintptr_t)stats & 15)) return TULIP_ERR_ARG;
    hipLaunchKernelGGL(loss_stats_kernel, dim3(tulip_loss_blocks(n)), dim3(256), 0, stream, pred, target, stats, n,
                       vec_groups(n, pred, target), log_transform);
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

extern "C" int tulip_loss_bwd(int kind, const float* pred, const float* target, const float* stats, const float* gscale_dev,
                              float gscale, float* dpred, float* loss_c, int64_t n, hipStream_t stream) {
    if (bad_kind(kind) || n <= 0 || !pred || !target || !dpred) return TULIP_ERR_ARG;
    if (kind == TULIP_LOSS_BERHU && (!stats || !loss_c)) return TULIP_ERR_ARG;
    const int nb = tulip_loss_blocks(n);
    const int64_t n4 = vec_groups(n, pred, target, dpred);
    const dim3 grid(nb), block(256);
    if (kind == TULIP_LOSS_L1)
        hipLaunchKernelGGL(loss_bwd_kernel<TULIP_LOSS_L1>, grid, block, 0, stream, pred, target, stats, nb, gscale_dev, gscale, dpred,
                           loss_c, n, n4);
    else if (kind == TULIP_LOSS_L2)
        hipLaunchKernelGGL(loss_bwd_kernel<TULIP_LOSS_L2>, grid, block, 0, stream, pred, target, stats, nb, gscale_dev, gscale, dpred,
                           loss_c, n, n4);
    else
        hipLaunchKernelGGL(loss_bwd_kernel<TULIP_LOSS_BERHU>, grid, block, 0, stream, pred, target, stats, nb, gscale_dev, gscale,
                           dpred, loss_c, n, n4);
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

extern "C" int tulip_loss_value(const float* pred, const float* target, const float* stats, float* value_partials, int64_t n,
                                hipStream_t stream) {
    if (n <= 0 || !pred || !target || !stats || !value_partials) return TULIP_ERR_ARG;
    const int nb = tulip_loss_blocks(n);
    hipLaunchKernelGGL(loss_value_kernel, dim3(nb), dim3(256), 0, stream, pred, target, stats, nb, value_partials, n,
                       vec_groups(n, pred, target));
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

extern "C" int tulip_loss_final(int kind, const float* stats, const float* value_partials, float* losses, int64_t n,
                                int log_transform, hipStream_t stream) {
    if (bad_kind(kind) || n <= 0 || !stats || !losses) return TULIP_ERR_ARG;
    if (kind == TULIP_LOSS_BERHU && !value_partials) return TULIP_ERR_ARG;
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(256), 0, stream, kind, stats, value_partials, losses, tulip_loss_blocks(n),
                       1.0 / (double)n, log_transform);
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

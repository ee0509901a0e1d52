// Element dropout (nn.Dropout: tulip.py:190-192 Mlp.drop1 / drop2, :319 proj_drop, :705 pos_drop; attn_drop lives in the
// attention kernels, csrc/attention.hip).  gfx950 only.
//
// The keep mask is counter-based (include/tulip_hip.h, "Element dropout"): every launch regenerates it from (seed, the step's
// counter word, site, element index), so nothing is stored between the forward and the backward and a replayed graph draws a
// fresh mask once tulip_dropout_begin has recorded the next counter value.  Everything here is elementwise over natural token
// rows, four elements per lane.
#include "common.h"
#include "tulip_hip.h"

namespace {

inline int grid_for(int64_t work, int cap = 256 * 8) {
    int64_t b = (work + 255) / 256;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

struct Mask {
    uint64_t key;
    uint32_t thr;
    float scale;
};
__device__ __forceinline__ Mask make_mask(const DropoutArg& d) {
    return Mask{dropout_key(d), dropout_thr(d.p), dropout_inv_keep(d.p)};
}
__device__ __forceinline__ float4 mask4(const Mask& m, uint64_t index) {
    return make_float4(dropout_mul(m.key, index, m.thr, m.scale), dropout_mul(m.key, index + 1, m.thr, m.scale),
                       dropout_mul(m.key, index + 2, m.thr, m.scale), dropout_mul(m.key, index + 3, m.thr, m.scale));
}

__global__ void begin_kernel(unsigned long long* counter, unsigned long long* key_out, int advance) {
    const unsigned long long c = *counter;
    *key_out = c;
    if (advance) *counter = c + 1;
}

__global__ __launch_bounds__(256) void mask_kernel(const DropoutArg d, int64_t n, float* __restrict__ out) {
    const Mask m = make_mask(d);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        out[i] = dropout_mul(m.key, (uint64_t)i, m.thr, m.scale);
}

// in place, fp32 or bf16 rows with pitch ld
template <bool BF16>
__global__ __launch_bounds__(256) void scale_kernel(void* __restrict__ x, int64_t n4, int cols4, int ld, const DropoutArg d) {
    const Mask m = make_mask(d);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / cols4;
        const int c = (int)(i - r * cols4) * 4;
        const float4 k = mask4(m, (uint64_t)(i * 4));
        if (BF16) {
            uint2* p = (uint2*)((bf16_t*)x + r * ld + c);
            const uint2 v = *p;
            const float a = __uint_as_float(v.x << 16), b = __uint_as_float(v.x & 0xffff0000u);
            const float e = __uint_as_float(v.y << 16), f = __uint_as_float(v.y & 0xffff0000u);
            *p = make_uint2(pack_bf16x2(a * k.x, b * k.y), pack_bf16x2(e * k.z, f * k.w));
        } else {
            float4* p = (float4*)((float*)x + r * ld + c);
            const float4 v = *p;
            *p = make_float4(v.x * k.x, v.y * k.y, v.z * k.z, v.w * k.w);
        }
    }
}

// out = aux + rowscale * (y * mask)  (+ bf16 copy)
__global__ __launch_bounds__(256) void resid_kernel(const float* y, const float* __restrict__ aux,
                                                    const float* __restrict__ rowscale, int rps, float* out,
                                                    bf16_t* __restrict__ out_bf16, int64_t n4, int cols4, const DropoutArg d) {
    const Mask m = make_mask(d);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / cols4;
        const float s = rowscale ? rowscale[r / rps] : 1.0f;
        const float4 k = mask4(m, (uint64_t)(i * 4));
        const float4 v = *(const float4*)(y + i * 4), a = *(const float4*)(aux + i * 4);
        const float4 o = make_float4(a.x + s * (v.x * k.x), a.y + s * (v.y * k.y), a.z + s * (v.z * k.z), a.w + s * (v.w * k.w));
        *(float4*)(out + i * 4) = o;
        if (out_bf16) *(uint2*)(out_bf16 + i * 4) = make_uint2(pack_bf16x2(o.x, o.y), pack_bf16x2(o.z, o.w));
    }
}

// y = bf16(dx * rowscale * mask)
__global__ __launch_bounds__(256) void cast_kernel(const float* __restrict__ dx, bf16_t* __restrict__ y,
                                                   const float* __restrict__ rowscale, int rps, int64_t n4, int cols4,
                                                   const DropoutArg d) {
    const Mask m = make_mask(d);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / cols4;
        const float s = rowscale ? rowscale[r / rps] : 1.0f;
        const float4 k = mask4(m, (uint64_t)(i * 4));
        const float4 v = *(const float4*)(dx + i * 4);
        *(uint2*)(y + i * 4) = make_uint2(pack_bf16x2(v.x * s * k.x, v.y * s * k.y), pack_bf16x2(v.z * s * k.z, v.w * s * k.w));
    }
}

bool p_ok(float p) { return p >= 0.0f && p < 1.0f; }

DropoutArg arg(const uint64_t* key_ptr, uint64_t seed, int site, float p) {
    return DropoutArg{(const unsigned long long*)key_ptr, (unsigned long long)seed, site, p};
}

}  // namespace

extern "C" int tulip_dropout_begin(uint64_t* counter, uint64_t* key_out, int advance, hipStream_t stream) {
    if (!counter || !key_out) return TULIP_ERR_ARG;
    hipLaunchKernelGGL(begin_kernel, dim3(1), dim3(1), 0, stream, (unsigned long long*)counter, (unsigned long long*)key_out,
                       advance);
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

extern "C" int tulip_dropout_mask(const uint64_t* key_ptr, uint64_t seed, int site, float p, int64_t n, float* out,
                                  hipStream_t stream) {
    if (!key_ptr || !out || !p_ok(p) || n < 0) return TULIP_ERR_ARG;
    if (n == 0) return TULIP_OK;
    hipLaunchKernelGGL(mask_kernel, dim3(grid_for(n)), dim3(256), 0, stream, arg(key_ptr, seed, site, p), n, out);
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

extern "C" int tulip_dropout_scale(void* x, int is_bf16, int rows, int cols, int ld, const uint64_t* key_ptr, uint64_t seed,
                                   int site, float p, hipStream_t stream) {
    if (!x || !key_ptr || !p_ok(p) || rows < 0 || cols <= 0 || (cols & 3) || (ld & 3) || ld < cols) return TULIP_ERR_ARG;
    if (rows == 0) return TULIP_OK;
    const int64_t n4 = (int64_t)rows * cols / 4;
    if (is_bf16)
        hipLaunchKernelGGL(scale_kernel<true>, dim3(grid_for(n4)), dim3(256), 0, stream, x, n4, cols / 4, ld,
                           arg(key_ptr, seed, site, p));
    else
        hipLaunchKernelGGL(scale_kernel<false>, dim3(grid_for(n4)), dim3(256), 0, stream, x, n4, cols / 4, ld,
                           arg(key_ptr, seed, site, p));
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

extern "C" int tulip_dropout_resid_ln(const float* y, const float* aux, const float* rowscale, int rows_per_sample, float* out,
                                      uint16_t* out_bf16, const float* gamma, const float* beta, uint16_t* xn, float* mean,
                                      float* rstd, float eps, int rows, int C, const uint64_t* key_ptr, uint64_t seed, int site,
                                      float p, hipStream_t stream) {
    if (!y || !aux || !out || !key_ptr || !p_ok(p) || rows < 0 || C <= 0 || (C & 3)) return TULIP_ERR_ARG;
    if (rowscale && rows_per_sample <= 0) return TULIP_ERR_ARG;
    if (gamma && (!beta || !xn || !mean || !rstd)) return TULIP_ERR_ARG;
    if (rows == 0) return TULIP_OK;
    const int64_t n4 = (int64_t)rows * C / 4;
    hipLaunchKernelGGL(resid_kernel, dim3(grid_for(n4)), dim3(256), 0, stream, y, aux, rowscale, rows_per_sample, out,
                       (bf16_t*)out_bf16, n4, C / 4, arg(key_ptr, seed, site, p));
    TULIP_CHECK_LAUNCH();
    if (!gamma) return TULIP_OK;
    // the LayerNorm behind the residual is the library's own launch: the same bits as the unmasked sequence's
    return tulip_layernorm_fwd(out, gamma, beta, xn, mean, rstd, rows, C, eps, 0, 0, 0, 0, stream);
}

extern "C" int tulip_dropout_cast(const float* dx, uint16_t* y, int rows, int cols, const float* rowscale, int rows_per_sample,
                                  const uint64_t* key_ptr, uint64_t seed, int site, float p, hipStream_t stream) {
    if (!dx || !y || !key_ptr || !p_ok(p) || rows < 0 || cols <= 0 || (cols & 3)) return TULIP_ERR_ARG;
    if (rowscale && rows_per_sample <= 0) return TULIP_ERR_ARG;
    if (rows == 0) return TULIP_OK;
    const int64_t n4 = (int64_t)rows * cols / 4;
    hipLaunchKernelGGL(cast_kernel, dim3(grid_for(n4)), dim3(256), 0, stream, dx, (bf16_t*)y, rowscale, rows_per_sample, n4,
                       cols / 4, arg(key_ptr, seed, site, p));
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

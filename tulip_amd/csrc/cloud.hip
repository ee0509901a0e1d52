// Dense point clouds from a batch of predictions (tulip_amd/cloud.py is the host definition): the prediction side of the
// evaluation post-processing (evalpost.hip post_kernel / post_c_kernel, expression for expression), the range image -> xyz
// projection (xyz_spherical_kernel / xyz_durlar_kernel) and an ordered stream compaction that drops the pixels without a return.
//
// Three stream-ordered launches over B*H*W destination slots, tiles of T = CLOUD_TILE consecutive slots of one image:
//   1. cloud_post_kernel   grid (tiles, B): post-processed planes rng (B,C,H,W) in destination order + the tile's kept count
//   2. cloud_scan_kernel   one block: exclusive scan of the B*tiles counts -> tile_offsets (int64), offsets[0..B]
//   3. cloud_write_kernel  grid (tiles, B): keep flags re-derived from rng, rank = wave-ballot prefix + totals of the waves before,
//                          rows (x, y, z, a_1..a_{C-1}) stored at tile_offsets + rank
// No block waits for another one: the order between the passes is the stream's.  A wave owns 256 consecutive slots of its tile
// (4 trips of 64 lanes), so the slot order within a tile is (wave, trip, lane) and one LDS exchange of four totals ranks a tile.
#include <hip/hip_runtime.h>

#include "common.h"
#include "tulip_hip.h"

namespace {

constexpr int CLOUD_TILE = 1024;                 // slots per block: 4 waves x CLOUD_TRIPS x 64 lanes
constexpr int CLOUD_TRIPS = CLOUD_TILE / 256;
static_assert(CLOUD_TILE % 256 == 0, "a tile is whole 256-thread trips");

struct CloudArgs {
    const float* pred; const float* lo;          // (B,C,H,W), (B,C,h,w)
    float* rng;                                  // (B,C,H,W), destination order
    int32_t* counts; int64_t* tile_offsets; int64_t* offsets; float* points;
    int B, H, W, h, w, f, restore_rows, logt, tiles;
    uint32_t chan_log;
    float gmin, gmax, keep_close, max_range;
    // spherical sensors: sin_h, cos_h over columns, sin_v, cos_v over rows
    const float* sh; const float* ch; const float* sv; const float* cv;
    // DurLAR: col tables (4*W), row tables (2*H), per-row pixel offset
    const double* colt; const double* rowt; const int32_t* row_offset;
    float origin_offset; double z_offset;
};

// destination slot d = v*W + j of an image -> its source column u (the row is v for every sensor)
template <bool DURLAR>
__device__ __forceinline__ int source_col(const CloudArgs& a, int v, int j) {
    if (!DURLAR) return j;
    int o = a.row_offset[v] % a.W;               // pixel (v,u) lands at column (u + W - o) % W: slot j holds u = (j + o) % W
    if (o < 0) o += a.W;
    const int u = j + o;
    return u >= a.W ? u - a.W : u;
}

template <int C, bool DURLAR>
__global__ __launch_bounds__(256) void cloud_post_kernel(CloudArgs a) {
    __shared__ int wave_total[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
    const int64_t n = (int64_t)a.H * a.W, lo_plane = (int64_t)a.h * a.w;
    const float* pred = a.pred + (int64_t)b * C * n;
    const float* lo = a.lo + (int64_t)b * C * lo_plane;
    float* rng = a.rng + (int64_t)b * C * n;
    int kept_total = 0;
#pragma unroll
    for (int t = 0; t < CLOUD_TRIPS; ++t) {
        const int64_t d = (int64_t)blockIdx.x * CLOUD_TILE + wave * (CLOUD_TRIPS * 64) + t * 64 + lane;
        bool kept = false;
        if (d < n) {
            const int v = (int)(d / a.W), j = (int)(d - (int64_t)v * a.W);
            const int u = source_col<DURLAR>(a, v, j);
            const int64_t k = (int64_t)v * a.W + u;
            float p = pred[k];
            if (a.logt) p = expm1f(p);
            p = (p >= a.gmin && p <= a.gmax) ? p : 0.f;
            const bool hole = p == 0.f;                       // after the gate, before the rows are restored
            const bool restore = a.restore_rows && v % a.f == 0;
            const int64_t kl = restore ? (int64_t)(v / a.f) * a.W + u : 0;
            if (restore) {
                float l = lo[kl];
                if (a.logt) l = expm1f(l);
                p = l;
            }
            bool zero_p = false;
            if (a.keep_close > 0.f) {
                zero_p = p > a.keep_close;
                if (zero_p) p = 0.f;
            }
            rng[d] = p;
            kept = p > 0.f;                                   // false for -0.0, +0.0 and a NaN
#pragma unroll
            for (int c = 1; c < C; ++c) {
                const bool lg = (a.chan_log >> (c - 1)) & 1u;
                float pc = pred[(int64_t)c * n + k];
                if (lg) pc = expm1f(pc);
                pc = hole ? 0.f : pc;                         // a select: a NaN or an infinity in a hole yields +0.0
                if (restore) {
                    float l = lo[(int64_t)c * lo_plane + kl];
                    if (lg) l = expm1f(l);
                    pc = l;
                }
                if (zero_p) pc = 0.f;
                rng[(int64_t)c * n + d] = pc;
            }
        }
        kept_total += __popcll(__ballot(kept));
    }
    if (lane == 0) wave_total[wave] = kept_total;
    __syncthreads();
    if (threadIdx.x == 0)
        a.counts[(int64_t)b * a.tiles + blockIdx.x] = (wave_total[0] + wave_total[1]) + (wave_total[2] + wave_total[3]);
}

// exclusive scan of n counts by one block, 256 per trip with a carry; offsets[b] = the first tile offset of image b
__global__ __launch_bounds__(256) void cloud_scan_kernel(const int32_t* __restrict__ counts, int64_t n, int tiles, int B,
                                                         int64_t* __restrict__ tile_offsets, int64_t* __restrict__ offsets) {
    __shared__ int wave_total[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t carry = 0;
    for (int64_t base = 0; base < n; base += 256) {
        const int64_t i = base + threadIdx.x;
        const int cnt = i < n ? counts[i] : 0;
        int incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        __syncthreads();                                      // the previous trip's totals have been read
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        int before = 0;
        for (int k = 0; k < wave; ++k) before += wave_total[k];
        const int64_t excl = carry + before + (incl - cnt);
        if (i < n) {
            tile_offsets[i] = excl;
            if (i % tiles == 0) offsets[i / tiles] = excl;
        }
        carry += (wave_total[0] + wave_total[1]) + (wave_total[2] + wave_total[3]);
    }
    if (threadIdx.x == 0) offsets[B] = carry;
}

template <int C, bool DURLAR>
__global__ __launch_bounds__(256) void cloud_write_kernel(CloudArgs a) {
#pragma clang fp contract(off)
    __shared__ int wave_total[4];
    constexpr int RW = 3 + C - 1;                             // floats per row
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
    const int64_t n = (int64_t)a.H * a.W;
    const float* rng = a.rng + (int64_t)b * C * n;
    const int64_t d0 = (int64_t)blockIdx.x * CLOUD_TILE + wave * (CLOUD_TRIPS * 64) + lane;
    float r[CLOUD_TRIPS];
    unsigned long long votes[CLOUD_TRIPS];
    int kept_total = 0;
#pragma unroll
    for (int t = 0; t < CLOUD_TRIPS; ++t) {
        const int64_t d = d0 + t * 64;
        r[t] = d < n ? rng[d] : 0.f;
        votes[t] = __ballot(r[t] > 0.f);
        kept_total += __popcll(votes[t]);
    }
    if (lane == 0) wave_total[wave] = kept_total;
    __syncthreads();
    int64_t row = a.tile_offsets[(int64_t)b * a.tiles + blockIdx.x];
    for (int k = 0; k < wave; ++k) row += wave_total[k];
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int t = 0; t < CLOUD_TRIPS; ++t) {
        if (r[t] > 0.f) {
            const int64_t d = d0 + t * 64;
            const int v = (int)(d / a.W), j = (int)(d - (int64_t)v * a.W);
            float* out = a.points + (row + __popcll(votes[t] & below)) * RW;
            if (DURLAR) {
                // xyz_durlar_kernel: float32 (r*max_range - origin_offset), unfused float64 after it, rounded once to float32
                const int u = source_col<DURLAR>(a, v, j);
                const float tf = r[t] * a.max_range - a.origin_offset;
                const double td = (double)tf;
                const double x = (td * a.colt[u]) * a.rowt[v] + a.colt[2 * a.W + u];
                const double y = (td * a.colt[a.W + u]) * a.rowt[v] + a.colt[3 * a.W + u];
                const double z = td * a.rowt[a.H + v];
                out[0] = (float)(-x);
                out[1] = (float)(-y);
                out[2] = (float)(z + a.z_offset);
            } else {
                // xyz_spherical_kernel: float32 products in the reference's order
                const float rr = r[t] * a.max_range;
                out[0] = (a.sh[j] * a.cv[v]) * rr;
                out[1] = (a.ch[j] * a.cv[v]) * rr;
                out[2] = a.sv[v] * rr;
            }
#pragma unroll
            for (int c = 1; c < C; ++c) out[2 + c] = rng[(int64_t)c * n + d];
        }
        row += __popcll(votes[t]);
    }
}

template <int C, bool DURLAR>
void launch_cloud(const CloudArgs& a, hipStream_t stream) {
    const dim3 grid(a.tiles, a.B), block(256);
    hipLaunchKernelGGL((cloud_post_kernel<C, DURLAR>), grid, block, 0, stream, a);
    hipLaunchKernelGGL(cloud_scan_kernel, dim3(1), block, 0, stream, (const int32_t*)a.counts, (int64_t)a.B * a.tiles, a.tiles,
                       a.B, a.tile_offsets, a.offsets);
    hipLaunchKernelGGL((cloud_write_kernel<C, DURLAR>), grid, block, 0, stream, a);
}

template <bool DURLAR>
int cloud_dispatch(const CloudArgs& a, int C, hipStream_t stream) {
    if (C == 1) launch_cloud<1, DURLAR>(a, stream);
    else if (C == 2) launch_cloud<2, DURLAR>(a, stream);
    else if (C == 3) launch_cloud<3, DURLAR>(a, stream);
    else launch_cloud<4, DURLAR>(a, stream);
    TULIP_CHECK_LAUNCH();
    return TULIP_OK;
}

// the arguments both entry points share; false: TULIP_ERR_ARG
bool cloud_args(CloudArgs& a, const float* pred, const float* lo, int B, int C, int H, int W, int h, int w, int log_transform,
                uint32_t chan_log_bits, float gate_min, float gate_max, float keep_close, float max_range, float* rng,
                int32_t* counts, int64_t* tile_offsets, int64_t* offsets, float* points) {
    if (!pred || !lo || !rng || !counts || !tile_offsets || !offsets || !points) return false;
    if (B <= 0 || B > 65535 || C < 1 || C > 4 || H <= 0 || W <= 0 || h <= 0 || w <= 0 || H % h) return false;
    if (chan_log_bits >> (C - 1)) return false;
    const int64_t tiles = ((int64_t)H * W + CLOUD_TILE - 1) / CLOUD_TILE;
    if (tiles > 0x7fffffff) return false;
    a = CloudArgs{};
    a.pred = pred; a.lo = lo; a.rng = rng; a.counts = counts; a.tile_offsets = tile_offsets; a.offsets = offsets;
    a.points = points;
    a.B = B; a.H = H; a.W = W; a.h = h; a.w = w; a.f = H / h; a.restore_rows = (w == W); a.logt = log_transform;
    a.tiles = (int)tiles;
    a.chan_log = chan_log_bits;
    a.gmin = gate_min; a.gmax = gate_max; a.keep_close = keep_close; a.max_range = max_range;
    return true;
}

}  // namespace

extern "C" int tulip_cloud_tile(void) { return CLOUD_TILE; }

extern "C" int tulip_cloud_spherical(const float* pred, const float* lo, int B, int C, int H, int W, int h, int w,
                                     int log_transform, uint32_t chan_log_bits, float gate_min, float gate_max,
                                     float keep_close, float max_range, const float* sin_h, const float* cos_h,
                                     const float* sin_v, const float* cos_v, float* rng, int32_t* counts,
                                     int64_t* tile_offsets, int64_t* offsets, float* points, hipStream_t stream) {
    CloudArgs a;
    if (!sin_h || !cos_h || !sin_v || !cos_v ||
        !cloud_args(a, pred, lo, B, C, H, W, h, w, log_transform, chan_log_bits, gate_min, gate_max, keep_close, max_range, rng,
                    counts, tile_offsets, offsets, points))
        return TULIP_ERR_ARG;
    a.sh = sin_h; a.ch = cos_h; a.sv = sin_v; a.cv = cos_v;
    return cloud_dispatch<false>(a, C, stream);
}

extern "C" int tulip_cloud_durlar(const float* pred, const float* lo, int B, int C, int H, int W, int h, int w,
                                  int log_transform, uint32_t chan_log_bits, float gate_min, float gate_max, float keep_close,
                                  float max_range, const double* col_tables, const double* row_tables,
                                  const int32_t* row_offset, float origin_offset, double z_offset, float* rng,
                                  int32_t* counts, int64_t* tile_offsets, int64_t* offsets, float* points,
                                  hipStream_t stream) {
    CloudArgs a;
    if (!col_tables || !row_tables || !row_offset ||
        !cloud_args(a, pred, lo, B, C, H, W, h, w, log_transform, chan_log_bits, gate_min, gate_max, keep_close, max_range, rng,
                    counts, tile_offsets, offsets, points))
        return TULIP_ERR_ARG;
    a.colt = col_tables; a.rowt = row_tables; a.row_offset = row_offset;
    a.origin_offset = origin_offset; a.z_offset = z_offset;
    return cloud_dispatch<true>(a, C, stream);
}

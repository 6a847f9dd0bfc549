// adaptive.hip — the device side of adaptive sampling (rt_adaptive_*_async; the definition:
// include/rt_api.h, DESIGN.md §4 "Adaptive sampling"):
//
//   as_accumulate  a pass's run sums onto the accumulators of the tiles it rendered
//   as_metric      every tile's error from its accumulators
//   as_metric_rank the same with a ranked pixel error in place of the largest (by counting in LDS)
//   as_compact     the tiles still above the threshold, as a list in tile order, and `info`
//   as_resolve     accumulators / count -> the frame, row-major
//
// The state is the packed tile layout the path kernel writes: tile t is [256][3] f64 at
// double 768 * t, 6 KiB, 384 sixteen-byte words, 48 whole 128-byte lines; pixels outside the
// image are zeros.  Every kernel takes a tile a block and moves it by 16-byte words in
// address order, word w of the tile to lane w mod 64 of some wave, so each load or store
// instruction of a wave covers 1 KiB, eight whole lines (se_kernel's and dn_prepare's map for
// 24-byte pixels).
//
// as_accumulate is a function of words, not of pixels, so it needs no LDS: 192 lanes take
// two words of each array, add the pass's runs onto them in run order — acc = ((acc + r_0) +
// r_1) + ..., the association of oracle_render_chunked's sum over a longer frame's runs —
// and store them by the same map.  The r_k are read where the path kernel left them, in the
// scene's partials [slot][run][256][3] (a single-run pass writes its one undivided output
// there too), not through reduce_chunks_kernel, which would add the pass's runs to each
// other first.  A pass at sample base 0 starts its tiles: the accumulators are taken as zero
// instead of read (0 + r_0 is r_0: a run sum starts from +0 and is never -0), the count is
// the pass's, and the error is "not measured" (+inf, not flagged).
//
// as_metric and as_resolve need pixels.  They stage a tile's two arrays in LDS by the word
// map, 12 KiB a block, and lane l then picks pixel l's three doubles of each.  The pixel
// pitch is 3 doubles, 6 banks: an odd number of bank pairs, so the 32 lanes of a half-wave,
// which an 8-byte LDS read serves in one pass, fall on 32 different bank pairs with no
// padding (dn_prepare pads only its records of an even number of doubles, to 7 and 9).
//
// Reductions are max and or, which do not depend on order: __shfl_xor within the wave, the
// block's waves through LDS.  as_compact is one block: in a trip lane i looks at tile
// trip * 1024 + i, a wave's ballot and popcount rank its lanes, the 16 wave counts go through
// LDS (two buffers, so one barrier a trip), and a running base is carried in a register
// every lane holds.  The list is therefore in ascending tile order, the same on every run.
// No floating-point atomics, and no atomics at all.
//
// / and sqrt are the compiler's IEEE ones and nothing is contracted (the Makefile's flags), so
// tile_err is the float64 numpy restatement's, bit for bit (tests/test_gpu_adaptive.py).
#include <hip/hip_runtime.h>

#include "render.h"

namespace rt {
namespace {

constexpr double kLr = 0.2126, kLg = 0.7152, kLb = 0.0722;  // luminance (denoise.hip)
constexpr uint32_t kPixelDoubles = 3;                       // the LDS pitch of a pixel
constexpr uint32_t kTileWords = 256 * kPixelDoubles / 2;    // 16-byte words of a tile's array
constexpr uint32_t kAccThreads = 192, kAccWords = kTileWords / kAccThreads;
constexpr uint32_t kThreads = 256, kWaves = kThreads / 64;
constexpr uint32_t kCompactWaves = kCompactThreads / 64;
static_assert(kTileWords % kAccThreads == 0 && kAccThreads % 64 == 0, "whole waves, whole words");
static_assert(kPixelDoubles % 2 == 1, "a pixel pitch of an odd number of doubles: conflict-free 8-byte LDS reads");

__device__ __forceinline__ bool finite(double v) { return fabs(v) < INFINITY; }
__device__ __forceinline__ double wave_max(double m) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(m, off, 64);
        m = o > m ? o : m;
    }
    return m;
}

// ----------------------------------------------------------------- accumulate ----
__global__ __launch_bounds__(kAccThreads) void as_accumulate(double2* __restrict__ acc_sum, double2* __restrict__ acc_sq,
                                                             const double2* __restrict__ part,
                                                             const double2* __restrict__ part_sq,
                                                             const uint32_t* __restrict__ list, uint64_t n_tiles,
                                                             uint32_t chunks, uint32_t pass_spp, int first,
                                                             uint32_t* __restrict__ tile_count,
                                                             double* __restrict__ tile_err,
                                                             uint32_t* __restrict__ tile_flag) {
    const uint32_t slot = blockIdx.x;
    const uint64_t tile = list ? list[slot] : slot;
    if (tile >= n_tiles) return;  // a caller's list entry that names no tile
#pragma unroll
    for (uint32_t j = 0; j < kAccWords; ++j) {
        const uint32_t w = threadIdx.x + kAccThreads * j;
        const uint64_t i = tile * kTileWords + w;
        double2 a = make_double2(0.0, 0.0), q = a;
        if (!first) { a = acc_sum[i]; q = acc_sq[i]; }
        const uint64_t r0 = (uint64_t)slot * chunks * kTileWords + w;
        for (uint32_t k = 0; k < chunks; ++k) {
            const double2 r = part[r0 + (uint64_t)k * kTileWords], r2 = part_sq[r0 + (uint64_t)k * kTileWords];
            a.x = a.x + r.x; a.y = a.y + r.y;
            q.x = q.x + r2.x; q.y = q.y + r2.y;
        }
        acc_sum[i] = a; acc_sq[i] = q;
    }
    if (threadIdx.x == 0) {
        tile_count[tile] = (first ? 0u : tile_count[tile]) + pass_spp;
        if (first) { tile_err[tile] = INFINITY; tile_flag[tile] = 0u; }
    }
}

// the block's tile, both arrays, into LDS by 16-byte words
__device__ __forceinline__ void stage_tile(double2* s_sum, double2* s_sq, const double2* __restrict__ acc_sum,
                                           const double2* __restrict__ acc_sq, uint64_t tile) {
    for (uint32_t w = threadIdx.x; w < kTileWords; w += kThreads) {
        s_sum[w] = acc_sum[tile * kTileWords + w];
        s_sq[w] = acc_sq[tile * kTileWords + w];
    }
    __syncthreads();
}

// --------------------------------------------------------------------- metric ----
__global__ __launch_bounds__(kThreads) void as_metric(const double2* __restrict__ acc_sum,
                                                      const double2* __restrict__ acc_sq,
                                                      const uint32_t* __restrict__ tile_count, uint32_t max_spp,
                                                      double eps, double* __restrict__ tile_err,
                                                      uint32_t* __restrict__ tile_flag) {
    __shared__ double2 s_sum[kTileWords], s_sq[kTileWords];
    __shared__ double s_max[kWaves];
    __shared__ uint32_t s_bad[kWaves];
    const uint64_t tile = blockIdx.x;
    const uint32_t count = tile_count[tile];
    if (count >= max_spp) return;  // at the cap: it cannot be selected, its error stays (block-uniform)
    if (count < 2) {               // no variance yet
        if (threadIdx.x == 0) { tile_err[tile] = INFINITY; tile_flag[tile] = 0u; }
        return;
    }
    stage_tile(s_sum, s_sq, acc_sum, acc_sq, tile);
    const double* ps = (const double*)s_sum + kPixelDoubles * threadIdx.x;
    const double* pq = (const double*)s_sq + kPixelDoubles * threadIdx.x;
    const double n = (double)count, n1 = n - 1.0;
    double mean[3], v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        mean[c] = ps[c] / n;
        const double m2 = pq[c] / n;
        const double d = m2 - mean[c] * mean[c];  // below 0 by rounding only: clamped; a NaN stays
        v[c] = (d < 0.0 ? 0.0 : d) / n1;
    }
    const double var = ((kLr * kLr) * v[0] + (kLg * kLg) * v[1]) + (kLb * kLb) * v[2];
    const double lum = (kLr * mean[0] + kLg * mean[1]) + kLb * mean[2];
    const double e = sqrt(var) / (lum + eps);
    // a pixel whose e is not finite cannot be repaired by samples: it flags the tile and
    // holds nothing open; a NaN never compares greater, and +inf is rejected here
    const bool bad = !finite(e);
    const double m = wave_max(!bad && e > 0.0 ? e : 0.0);
    const bool any_bad = __ballot(bad) != 0;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) { s_max[wave] = m; s_bad[wave] = any_bad ? 1u : 0u; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = s_max[0];
        uint32_t f = s_bad[0];
        for (uint32_t k = 1; k < kWaves; ++k) { r = s_max[k] > r ? s_max[k] : r; f |= s_bad[k]; }
        tile_err[tile] = r;
        tile_flag[tile] = f;
    }
}

// as_metric with the (r + 1)-th largest of the tile's 256 values g in place of the largest,
// r = rank * m / 256 for a tile with m pixels inside the image (rt_adaptive_select_rank_async).
// g is finite and >= +0, so doubles order as their bit patterns and the keys are the u64s.
// Selection by counting, no sort: every lane puts its key into LDS, and after the one barrier
// (which the flags share) counts the keys that come before its own in the order "larger key
// first, equal keys by pixel index".  That order is total, so the 256 counts are a
// permutation of 0..255 and exactly one lane finds r: it writes its key, one of the inputs,
// unchanged.  The keys are read as 128 sixteen-byte words at addresses every lane shares:
// broadcasts, no bank conflicts, and no traffic beyond the 2 KiB of keys.
__global__ __launch_bounds__(kThreads) void as_metric_rank(const double2* __restrict__ acc_sum,
                                                           const double2* __restrict__ acc_sq,
                                                           const uint32_t* __restrict__ tile_count, uint32_t max_spp,
                                                           double eps, uint32_t W, uint32_t H, uint32_t tiles_x,
                                                           uint32_t rank, double* __restrict__ tile_err,
                                                           uint32_t* __restrict__ tile_flag) {
    __shared__ double2 s_sum[kTileWords], s_sq[kTileWords];
    __shared__ ulonglong2 s_key[kThreads / 2];
    __shared__ uint32_t s_bad[kWaves];
    const uint64_t tile = blockIdx.x;
    const uint32_t count = tile_count[tile];
    if (count >= max_spp) return;  // as as_metric: block-uniform exits
    if (count < 2) {
        if (threadIdx.x == 0) { tile_err[tile] = INFINITY; tile_flag[tile] = 0u; }
        return;
    }
    stage_tile(s_sum, s_sq, acc_sum, acc_sq, tile);
    // e as as_metric computes it, restated: sharing the lines through a function reorders
    // as_metric's own instructions, and that kernel stays as it was compiled
    const double* ps = (const double*)s_sum + kPixelDoubles * threadIdx.x;
    const double* pq = (const double*)s_sq + kPixelDoubles * threadIdx.x;
    const double n = (double)count, n1 = n - 1.0;
    double mean[3], v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        mean[c] = ps[c] / n;
        const double m2 = pq[c] / n;
        const double d = m2 - mean[c] * mean[c];
        v[c] = (d < 0.0 ? 0.0 : d) / n1;
    }
    const double var = ((kLr * kLr) * v[0] + (kLg * kLg) * v[1]) + (kLb * kLb) * v[2];
    const double lum = (kLr * mean[0] + kLg * mean[1]) + kLb * mean[2];
    const double e = sqrt(var) / (lum + eps);
    const bool bad = !finite(e);
    const unsigned long long key = (unsigned long long)__double_as_longlong(!bad && e > 0.0 ? e : 0.0);
    ((unsigned long long*)s_key)[threadIdx.x] = key;
    const bool any_bad = __ballot(bad) != 0;
    if ((threadIdx.x & 63u) == 0) s_bad[threadIdx.x >> 6] = any_bad ? 1u : 0u;
    __syncthreads();
    uint32_t before = 0;  // keys ahead of this lane's
#pragma unroll 8
    for (uint32_t j = 0; j < kThreads; j += 2) {
        const ulonglong2 k = s_key[j / 2];
        before += (k.x > key || (k.x == key && j < threadIdx.x)) ? 1u : 0u;
        before += (k.y > key || (k.y == key && j + 1 < threadIdx.x)) ? 1u : 0u;
    }
    // the tile's pixels inside the image scale the rank: a full tile uses rank itself
    const uint32_t x0 = (uint32_t)(tile % tiles_x) * RT_TILE, y0 = (uint32_t)(tile / tiles_x) * RT_TILE;
    const uint32_t m = min((uint32_t)RT_TILE, W - x0) * min((uint32_t)RT_TILE, H - y0);
    if (before == rank * m / 256u) {
        uint32_t f = s_bad[0];
        for (uint32_t k = 1; k < kWaves; ++k) f |= s_bad[k];
        tile_err[tile] = __longlong_as_double((long long)key);
        tile_flag[tile] = f;
    }
}

// -------------------------------------------------------------------- compact ----
struct AsInfo {
    uint32_t n_list, n_flagged;
    double max_err;
};
static_assert(sizeof(AsInfo) == 16, "rt_api.h: info is 16 bytes");

__global__ __launch_bounds__(kCompactThreads) void as_compact(const double* __restrict__ tile_err,
                                                              const uint32_t* __restrict__ tile_count,
                                                              const uint32_t* __restrict__ tile_flag, uint64_t n_tiles,
                                                              double threshold, uint32_t pass_spp, uint32_t max_spp,
                                                              uint32_t* __restrict__ list, AsInfo* __restrict__ info) {
    __shared__ uint32_t s_sel[2][kCompactWaves], s_flag[2][kCompactWaves];
    __shared__ double s_max[kCompactWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t base = 0, flagged = 0;  // block-uniform: tiles selected and flagged in the trips so far
    double m = 0.0;                  // this lane's largest finite error
    for (uint64_t t0 = 0, trip = 0; t0 < n_tiles; t0 += kCompactThreads, ++trip) {
        const uint64_t tile = t0 + threadIdx.x;
        bool sel = false, flag = false;
        if (tile < n_tiles) {
            const double e = tile_err[tile];
            sel = e > threshold && (uint64_t)tile_count[tile] + pass_spp <= max_spp;
            flag = tile_flag[tile] != 0;
            if (finite(e) && e > m) m = e;
        }
        const uint64_t b_sel = __ballot(sel), b_flag = __ballot(flag);
        if (lane == 0) {
            s_sel[trip & 1][wave] = (uint32_t)__popcll(b_sel);
            s_flag[trip & 1][wave] = (uint32_t)__popcll(b_flag);
        }
        __syncthreads();
        uint32_t before = 0, total = 0;  // selected by the waves before this one, and by all
#pragma unroll
        for (uint32_t k = 0; k < kCompactWaves; ++k) {
            const uint32_t c = s_sel[trip & 1][k];
            before += k < wave ? c : 0u;
            total += c;
            flagged += s_flag[trip & 1][k];
        }
        if (sel) list[base + before + (uint32_t)__popcll(b_sel & ((1ull << lane) - 1ull))] = (uint32_t)tile;
        base += total;
    }
    m = wave_max(m);
    if (lane == 0) s_max[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = s_max[0];
        for (uint32_t k = 1; k < kCompactWaves; ++k) r = s_max[k] > r ? s_max[k] : r;
        info->n_list = base;
        info->n_flagged = flagged;
        info->max_err = r;
    }
}

// -------------------------------------------------------------------- resolve ----
// The packed reads are whole lines (stage_tile); a lane writes its pixel's 24 bytes, a
// tile row of 16 lanes 384 contiguous bytes of the frame, as unpack_kernel's lanes do.
__global__ __launch_bounds__(kThreads) void as_resolve(const double2* __restrict__ acc_sum,
                                                       const double2* __restrict__ acc_sq,
                                                       const uint32_t* __restrict__ tile_count, uint32_t W, uint32_t H,
                                                       uint32_t tiles_x, double* __restrict__ mean,
                                                       double* __restrict__ sq, uint32_t* __restrict__ count) {
    __shared__ double2 s_sum[kTileWords], s_sq[kTileWords];
    const uint64_t tile = blockIdx.x;
    stage_tile(s_sum, s_sq, acc_sum, acc_sq, tile);
    const uint32_t x = (uint32_t)(tile % tiles_x) * RT_TILE + (threadIdx.x & 15u);
    const uint32_t y = (uint32_t)(tile / tiles_x) * RT_TILE + (threadIdx.x >> 4);
    if (x >= W || y >= H) return;
    const uint32_t c = tile_count[tile];
    const double n = (double)c;
    const double* ps = (const double*)s_sum + kPixelDoubles * threadIdx.x;
    const double* pq = (const double*)s_sq + kPixelDoubles * threadIdx.x;
    const uint64_t pix = (uint64_t)y * W + x;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        mean[3 * pix + k] = ps[k] / n;
        sq[3 * pix + k] = pq[k] / n;
    }
    if (count) count[pix] = c;
}

uint64_t up256(uint64_t b) { return (b + 255) / 256 * 256; }

}  // namespace

AdaptiveLayout adaptive_layout(uint64_t n_tiles) {
    AdaptiveLayout L;
    uint64_t o = 0;
    L.acc_sum = o;    o += up256(n_tiles * 256 * 3 * sizeof(double));
    L.acc_sq = o;     o += up256(n_tiles * 256 * 3 * sizeof(double));
    L.tile_count = o; o += up256(n_tiles * sizeof(uint32_t));
    L.tile_err = o;   o += up256(n_tiles * sizeof(double));
    L.tile_flag = o;  o += up256(n_tiles * sizeof(uint32_t));
    L.tile_list = o;  o += up256(n_tiles * sizeof(uint32_t));
    L.info = o;       o += up256(sizeof(AsInfo));
    L.bytes = o;
    return L;
}

hipError_t launch_adaptive_accumulate(void* ws, uint64_t n_tiles, const double* part, const double* part_sq,
                                      const uint32_t* list, uint32_t n_list, uint32_t chunks, uint32_t pass_spp,
                                      bool first, hipStream_t st) {
    const AdaptiveLayout L = adaptive_layout(n_tiles);
    char* b = (char*)ws;
    hipLaunchKernelGGL(as_accumulate, dim3(n_list), dim3(kAccThreads), 0, st, (double2*)(b + L.acc_sum),
                       (double2*)(b + L.acc_sq), (const double2*)part, (const double2*)part_sq, list, n_tiles, chunks,
                       pass_spp, first ? 1 : 0, (uint32_t*)(b + L.tile_count), (double*)(b + L.tile_err),
                       (uint32_t*)(b + L.tile_flag));
    return hipGetLastError();
}

static hipError_t launch_compact(char* b, const AdaptiveLayout& L, uint64_t n_tiles, double threshold,
                                 uint32_t pass_spp, uint32_t max_spp, hipStream_t st) {
    hipLaunchKernelGGL(as_compact, dim3(1), dim3(kCompactThreads), 0, st, (const double*)(b + L.tile_err),
                       (const uint32_t*)(b + L.tile_count), (const uint32_t*)(b + L.tile_flag), n_tiles, threshold,
                       pass_spp, max_spp, (uint32_t*)(b + L.tile_list), (AsInfo*)(b + L.info));
    return hipGetLastError();
}

hipError_t launch_adaptive_select(void* ws, uint64_t n_tiles, double threshold, double eps, uint32_t pass_spp,
                                  uint32_t max_spp, hipStream_t st) {
    const AdaptiveLayout L = adaptive_layout(n_tiles);
    char* b = (char*)ws;
    hipLaunchKernelGGL(as_metric, dim3((unsigned)n_tiles), dim3(kThreads), 0, st, (const double2*)(b + L.acc_sum),
                       (const double2*)(b + L.acc_sq), (const uint32_t*)(b + L.tile_count), max_spp, eps,
                       (double*)(b + L.tile_err), (uint32_t*)(b + L.tile_flag));
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : launch_compact(b, L, n_tiles, threshold, pass_spp, max_spp, st);
}

hipError_t launch_adaptive_select_rank(void* ws, uint32_t W, uint32_t H, double threshold, double eps,
                                       uint32_t pass_spp, uint32_t max_spp, uint32_t rank, hipStream_t st) {
    const uint32_t tiles_x = (W + RT_TILE - 1) / RT_TILE, tiles_y = (H + RT_TILE - 1) / RT_TILE;
    const uint64_t n_tiles = (uint64_t)tiles_x * tiles_y;
    const AdaptiveLayout L = adaptive_layout(n_tiles);
    char* b = (char*)ws;
    hipLaunchKernelGGL(as_metric_rank, dim3((unsigned)n_tiles), dim3(kThreads), 0, st, (const double2*)(b + L.acc_sum),
                       (const double2*)(b + L.acc_sq), (const uint32_t*)(b + L.tile_count), max_spp, eps, W, H, tiles_x,
                       rank, (double*)(b + L.tile_err), (uint32_t*)(b + L.tile_flag));
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : launch_compact(b, L, n_tiles, threshold, pass_spp, max_spp, st);
}

hipError_t launch_adaptive_resolve(const void* ws, uint32_t W, uint32_t H, double* mean, double* sq, uint32_t* count,
                                   hipStream_t st) {
    const uint32_t tiles_x = (W + RT_TILE - 1) / RT_TILE, tiles_y = (H + RT_TILE - 1) / RT_TILE;
    const uint64_t n_tiles = (uint64_t)tiles_x * tiles_y;
    const AdaptiveLayout L = adaptive_layout(n_tiles);
    const char* b = (const char*)ws;
    hipLaunchKernelGGL(as_resolve, dim3((unsigned)n_tiles), dim3(kThreads), 0, st, (const double2*)(b + L.acc_sum),
                       (const double2*)(b + L.acc_sq), (const uint32_t*)(b + L.tile_count), W, H, tiles_x, mean, sq,
                       count);
    return hipGetLastError();
}

}  // namespace rt

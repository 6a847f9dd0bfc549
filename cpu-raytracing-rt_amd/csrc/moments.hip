// moments.hip — from a frame's per-pixel mean and second moment (rt_render_moments) to the
// standard error of the mean and a frame summary (rt_error_estimate_async):
//
//   se_kernel       se = sqrt(max(m2 - mean * mean, 0) / (spp - 1)) per value, and per block
//                   one partial of the summary
//   se_counts_kernel  the same with (count of the value's pixel - 1) for (spp - 1)
//   se_fold_kernel  the partials, in block order, to the 8 doubles of the summary
//
// The arrays are [n_pixels][3] f64, interleaved.  A pixel is 24 bytes, so no 16-byte word
// per lane holds whole pixels — but se is a function of one (mean, m2) value pair, not of
// a pixel.  So the map is by word, not by pixel: in a trip a wave takes 3 KiB of each
// array, 192 sixteen-byte words, and lane l loads words l, 64 + l and 128 + l.  Each load
// instruction of the wave then reads 64 consecutive words, 1 KiB, eight whole 128-byte
// lines (the arrays are 16-byte aligned by contract and line-aligned as hipMalloc gives
// them); the two se values of a word are computed in the registers the loads filled and
// stored by the same map, whole lines again (tri_tile.h store_tile's way, without the trip
// through LDS that its items need).  3 KiB are 128 whole pixels, so no pixel straddles two
// trips or two waves.
//
// Only the summary asks for pixels: its sums run over the pixels whose three channels are
// all finite.  Each value's "not finite" flag goes to LDS as a byte (384 B a wave), and a
// lane reads the three flags of the pixel of each of its values.  Value x of a trip has
// channel x % 3 = (2 * lane + 2 * k + j) % 3 for word k, half j, so a lane adds into three
// accumulators indexed by (2 * k + j) % 3, known at compile time, and rotates them by
// (2 * lane) % 3 once at the end.
//
// The reduction has a fixed shape, and no floating-point atomics: a lane adds its values
// in trip order; the wave's lanes combine by __shfl_xor at distances 32, 16, .., 1 (every
// lane ends with the same bits, a + b being b + a); the block's four waves are folded in
// wave order through LDS; block b writes partial b; se_fold_kernel's lane l folds the
// partials of blocks [l * per, (l + 1) * per) in block order and the 64 lanes combine by
// the same __shfl_xor tree.  Block count and trips per block are functions of n_pixels
// alone, so the summary is the same bits on every run and every stream.
//
// sqrt and / are the compiler's IEEE ones (no fast-math; the Makefile's flags), which
// round as the host's do (tests/test_gpu_parity.py test_fp64_rounding_matches_host).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "render.h"

namespace rt {
namespace {

constexpr uint32_t kSeWaves = 4, kSeThreads = kSeWaves * 64;
constexpr uint32_t kSeWords = 3;                       // 16-byte words per lane, array and trip
constexpr uint32_t kSeVals = 64 * kSeWords * 2;        // values per wave and trip: 384 = 128 pixels
static_assert(kSeVals % 3 == 0 && (64 * 2) % 3 == 2, "the channel of a value as se_kernel derives it");

__device__ __forceinline__ bool finite(double v) { return fabs(v) < INFINITY; }

// `one`: spp == 1, where the estimate does not exist: +inf (NaN where an input is NaN)
__device__ __forceinline__ double se_of(double mean, double m2, double denom, bool one) {
    if (one) return (mean != mean || m2 != m2) ? NAN : INFINITY;
    const double d = m2 - mean * mean;  // below 0 by rounding only: clamped; a NaN stays
    return sqrt((d < 0.0 ? 0.0 : d) / denom);
}

// summary value i of two partial results: 0 the non-finite pixels, 1..3 the sums of se,
// 4..6 of the mean, 7 the max of se
__device__ __forceinline__ double se_join(int i, double a, double b) { return i == 7 ? fmax(a, b) : a + b; }

__device__ __forceinline__ void wave_join(double v[8]) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = se_join(i, v[i], __shfl_xor(v[i], off, 64));
}

__global__ __launch_bounds__(kSeThreads) void se_kernel(const double2* __restrict__ mean, const double2* __restrict__ sq,
                                                        uint64_t n_vals, uint64_t trips, double denom, int one,
                                                        double2* __restrict__ se, double* __restrict__ part) {
    // a value's flag: se or mean not finite; two buffers, so one barrier a trip is enough
    __shared__ uint16_t s_bad[2][kSeWaves][kSeVals / 2];
    __shared__ double s_red[kSeWaves][8];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    double a_se[3] = {0.0, 0.0, 0.0}, a_mean[3] = {0.0, 0.0, 0.0}, a_max = 0.0, a_bad = 0.0;
    for (uint64_t t = 0; t < trips; ++t) {
        const uint64_t v0 = ((blockIdx.x * trips + t) * kSeWaves + wave) * kSeVals;  // the wave's first value
        uint16_t* bad = s_bad[t & 1][wave];
        double m[2 * kSeWords], e[2 * kSeWords];
#pragma unroll
        for (uint32_t k = 0; k < kSeWords; ++k) {
            const uint64_t v = v0 + 2 * (64 * k + lane);
            double2 a = make_double2(0.0, 0.0), q = a;
            if (v + 1 < n_vals) {
                a = mean[v / 2]; q = sq[v / 2];
            } else if (v < n_vals) {  // the last value of an odd count
                a.x = ((const double*)mean)[v]; q.x = ((const double*)sq)[v];
            }
            const double2 r = make_double2(se_of(a.x, q.x, denom, one), se_of(a.y, q.y, denom, one));
            if (se && v + 1 < n_vals) se[v / 2] = r;
            else if (se && v < n_vals) ((double*)se)[v] = r.x;
            bad[64 * k + lane] = (uint16_t)((finite(r.x) && finite(a.x) ? 0u : 1u) | (finite(r.y) && finite(a.y) ? 0u : 0x100u));
            m[2 * k] = a.x; m[2 * k + 1] = a.y; e[2 * k] = r.x; e[2 * k + 1] = r.y;
        }
        __syncthreads();
        const uint8_t* flag = (const uint8_t*)bad;
#pragma unroll
        for (uint32_t i = 0; i < 2 * kSeWords; ++i) {
            const uint32_t x = 2 * (64 * (i / 2) + lane) + (i & 1u), p = x / 3 * 3;  // p: the pixel's first value
            if (v0 + x >= n_vals) continue;
            if (flag[p] | flag[p + 1] | flag[p + 2]) {
                if (x == p) a_bad += 1.0;  // counted once, by the lane of its first value
            } else {
                a_se[i % 3] += e[i]; a_mean[i % 3] += m[i];
                a_max = fmax(a_max, e[i]);
            }
        }
    }
    // accumulator r holds channel (c0 + r) % 3
    const uint32_t c0 = 2 * lane % 3;
    double v[8];
    v[0] = a_bad; v[7] = a_max;
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) {
        v[1 + c] = c0 == 0 ? a_se[c] : (c0 == 1 ? a_se[(c + 2) % 3] : a_se[(c + 1) % 3]);
        v[4 + c] = c0 == 0 ? a_mean[c] : (c0 == 1 ? a_mean[(c + 2) % 3] : a_mean[(c + 1) % 3]);
    }
    wave_join(v);
    if (lane == 0)
        for (int i = 0; i < 8; ++i) s_red[wave][i] = v[i];
    __syncthreads();
    if (threadIdx.x < 8) {
        double r = s_red[0][threadIdx.x];
        for (uint32_t w = 1; w < kSeWaves; ++w) r = se_join((int)threadIdx.x, r, s_red[w][threadIdx.x]);
        part[(uint64_t)blockIdx.x * 8 + threadIdx.x] = r;
    }
}

// se_kernel where every pixel has a sample count of its own (rt_error_estimate_counts_async): a
// value's denom and `one` come from its pixel's count.  The map, the flags and the fold are
// se_kernel's, restated line for line: shared through a function, se_kernel's own instructions
// come out in another order, and that kernel stays as it was compiled.  A wave's trip is 128
// whole pixels, 512 contiguous bytes of counts: the wave loads them as two coalesced 4-byte
// loads a lane (the array is only 4-byte aligned) into LDS, and a lane reads the count of each
// of its six values from there (neighbouring lanes read the same or the next word: no bank
// conflicts).  The counts are staged one trip ahead, into the buffer the flags' parity names,
// so the trip's one barrier orders them too and their load overlaps the trip's other loads;
// only the first trip pays a barrier of its own.
__global__ __launch_bounds__(kSeThreads) void se_counts_kernel(const double2* __restrict__ mean,
                                                               const double2* __restrict__ sq,
                                                               const uint32_t* __restrict__ count, uint64_t n_vals,
                                                               uint64_t trips, double2* __restrict__ se,
                                                               double* __restrict__ part) {
    // a value's flag: se or mean not finite; two buffers, so one barrier a trip is enough
    __shared__ uint16_t s_bad[2][kSeWaves][kSeVals / 2];
    __shared__ uint32_t s_cnt[2][kSeWaves][kSeVals / 3];
    __shared__ double s_red[kSeWaves][8];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    double a_se[3] = {0.0, 0.0, 0.0}, a_mean[3] = {0.0, 0.0, 0.0}, a_max = 0.0, a_bad = 0.0;
    const auto stage_counts = [&](uint64_t t) {
        const uint64_t p0 = ((blockIdx.x * trips + t) * kSeWaves + wave) * (kSeVals / 3);  // the wave's first pixel
#pragma unroll
        for (uint32_t k = 0; k < kSeVals / 3 / 64; ++k) {
            const uint64_t p = p0 + 64 * k + lane;
            s_cnt[t & 1][wave][64 * k + lane] = p < n_vals / 3 ? count[p] : 0u;
        }
    };
    stage_counts(0);
    __syncthreads();
    for (uint64_t t = 0; t < trips; ++t) {
        const uint64_t v0 = ((blockIdx.x * trips + t) * kSeWaves + wave) * kSeVals;  // the wave's first value
        uint16_t* bad = s_bad[t & 1][wave];
        if (t + 1 < trips) stage_counts(t + 1);
        double m[2 * kSeWords], e[2 * kSeWords];
#pragma unroll
        for (uint32_t k = 0; k < kSeWords; ++k) {
            const uint64_t v = v0 + 2 * (64 * k + lane);
            double2 a = make_double2(0.0, 0.0), q = a;
            if (v + 1 < n_vals) {
                a = mean[v / 2]; q = sq[v / 2];
            } else if (v < n_vals) {  // the last value of an odd count
                a.x = ((const double*)mean)[v]; q.x = ((const double*)sq)[v];
            }
            const uint32_t x = 2 * (64 * k + lane);  // the word's first value within the trip
            const uint32_t c0 = s_cnt[t & 1][wave][x / 3], c1 = s_cnt[t & 1][wave][(x + 1) / 3];
            const double2 r = make_double2(se_of(a.x, q.x, (double)c0 - 1.0, c0 < 2), se_of(a.y, q.y, (double)c1 - 1.0, c1 < 2));
            if (se && v + 1 < n_vals) se[v / 2] = r;
            else if (se && v < n_vals) ((double*)se)[v] = r.x;
            bad[64 * k + lane] = (uint16_t)((finite(r.x) && finite(a.x) ? 0u : 1u) | (finite(r.y) && finite(a.y) ? 0u : 0x100u));
            m[2 * k] = a.x; m[2 * k + 1] = a.y; e[2 * k] = r.x; e[2 * k + 1] = r.y;
        }
        __syncthreads();
        const uint8_t* flag = (const uint8_t*)bad;
#pragma unroll
        for (uint32_t i = 0; i < 2 * kSeWords; ++i) {
            const uint32_t x = 2 * (64 * (i / 2) + lane) + (i & 1u), p = x / 3 * 3;  // p: the pixel's first value
            if (v0 + x >= n_vals) continue;
            if (flag[p] | flag[p + 1] | flag[p + 2]) {
                if (x == p) a_bad += 1.0;  // counted once, by the lane of its first value
            } else {
                a_se[i % 3] += e[i]; a_mean[i % 3] += m[i];
                a_max = fmax(a_max, e[i]);
            }
        }
    }
    // accumulator r holds channel (c0 + r) % 3
    const uint32_t c0 = 2 * lane % 3;
    double v[8];
    v[0] = a_bad; v[7] = a_max;
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) {
        v[1 + c] = c0 == 0 ? a_se[c] : (c0 == 1 ? a_se[(c + 2) % 3] : a_se[(c + 1) % 3]);
        v[4 + c] = c0 == 0 ? a_mean[c] : (c0 == 1 ? a_mean[(c + 2) % 3] : a_mean[(c + 1) % 3]);
    }
    wave_join(v);
    if (lane == 0)
        for (int i = 0; i < 8; ++i) s_red[wave][i] = v[i];
    __syncthreads();
    if (threadIdx.x < 8) {
        double r = s_red[0][threadIdx.x];
        for (uint32_t w = 1; w < kSeWaves; ++w) r = se_join((int)threadIdx.x, r, s_red[w][threadIdx.x]);
        part[(uint64_t)blockIdx.x * 8 + threadIdx.x] = r;
    }
}

// One block of 8 waves, wave i for summary value i; n_blocks == 0 gives the empty frame's zeros.
__global__ __launch_bounds__(512) void se_fold_kernel(const double* __restrict__ part, uint32_t n_blocks,
                                                      double* __restrict__ summary) {
    const uint32_t lane = threadIdx.x & 63u;
    const int i = (int)(threadIdx.x >> 6);
    const uint32_t per = (n_blocks + 63u) / 64u;
    double r = 0.0;
    for (uint32_t b = lane * per; b < min(n_blocks, (lane + 1u) * per); ++b) r = se_join(i, r, part[(uint64_t)b * 8 + i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) r = se_join(i, r, __shfl_xor(r, off, 64));
    if (lane == 0) summary[i] = r;
}

}  // namespace

hipError_t launch_error_estimate(const double* mean, const double* sq, uint64_t n_pixels, uint32_t spp, double* se,
                                 double* summary, double* part, hipStream_t st, const uint32_t* count) {
    const uint64_t n_vals = n_pixels * 3, tiles = (n_vals + kSeVals - 1) / kSeVals;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(kSeMaxBlocks, (tiles + kSeWaves - 1) / kSeWaves);
    if (blocks) {
        const uint64_t trips = (tiles + (uint64_t)blocks * kSeWaves - 1) / ((uint64_t)blocks * kSeWaves);
        if (count)
            hipLaunchKernelGGL(se_counts_kernel, dim3(blocks), dim3(kSeThreads), 0, st, (const double2*)mean,
                               (const double2*)sq, count, n_vals, trips, (double2*)se, part);
        else
            hipLaunchKernelGGL(se_kernel, dim3(blocks), dim3(kSeThreads), 0, st, (const double2*)mean, (const double2*)sq,
                               n_vals, trips, (double)spp - 1.0, spp == 1 ? 1 : 0, (double2*)se, part);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(se_fold_kernel, dim3(1), dim3(512), 0, st, part, blocks, summary);
    return hipGetLastError();
}

}  // namespace rt

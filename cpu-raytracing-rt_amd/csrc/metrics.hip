// metrics.hip — the distance of a frame A to a reference frame B of the same scene
// (rt_image_metrics_async; the definition: include/rt_api.h, DESIGN.md §4 "Image metrics"):
//
//   im_tile<format>  per pixel squared error, relative squared error and largest difference, per
//                    11x11 window SSIM of the luminances, and per block one partial of the summary
//   im_fold          the partials, in block order, to the 8 doubles of the summary
//
// im_tile.  A block of 256 lanes owns a 32x16 core of pixels, and pixel (x, y) of the core is also
// the window whose top-left pixel is (x, y), so the halo lies to the right and below only: the
// block stages 42x26 pixels.  A pixel outside the image is staged as 0; only windows that do not
// exist read one.
//
// A staged row is 126 consecutive values of an image (42 pixels of 3), and the 26 rows fill a raw
// LDS buffer of 3,276 doubles: value v of the buffer belongs to lane v mod 256, so a load
// instruction of a wave reads 64 consecutive values, 512 B of f64 or 64 B of u8.  The loads are
// 8-byte (1-byte) ones: a row of f64 starts at 24 * (y * W + x0) bytes, which is only 8-aligned
// when W is odd, and a row of u8 anywhere.  A byte is widened to f64 as it is staged, which is
// exact, so everything behind the staging is one body.  Staged pixel k then reads raw[3k .. 3k + 2]:
// neighbouring lanes are 3 doubles apart, an odd number of bank pairs, so a pass of 32 lanes falls
// on 32 different pairs (as_metric's argument), and writes its luminance to plane[k], consecutive
// lanes to consecutive doubles.  The luminance planes have pitch 42, the staged width itself: every
// later read is by 32 lanes of one row at consecutive columns, one pass of 32 different bank pairs
// at any pitch, so a padded pitch would buy nothing and the dense one keeps plane[k] contiguous.
//
// A is staged first; a lane keeps the two core pixels it owns, (lx, ly) and (lx, ly + 8), in
// registers (6 doubles), and B is staged into the same raw buffer, which therefore holds one image
// (26,208 B), not two.  se, rel and the largest |d| of the two pixels are formed while B's values
// pass through registers.
//
// Horizontal pass: item (r, lx) of 26 rows x 32 columns, four trips (the last one a single wave),
// reads ya and yb at r, lx + i for i = 0..10, forms the five products and accumulates the five
// planes q = (ya, yb, ya*ya, yb*yb, ya*yb) in tap order into h[5][26][32] (33,280 B), which
// overlays the raw buffer, dead by then.  Vertical pass: lane (lx, ly) reads h_k[oy + j][lx] for
// j = 0..10 and its two outputs oy = ly, ly + 8, forms ssim and stores rows of 32 consecutive
// doubles.  LDS: 33,280 + 2 * 8,736 + 256 = 51,008 B, three blocks a CU.
//
// No matrix instruction: both passes are banded Toeplitz products that v_mfma_f64_16x16x4_f64
// could run, but its internal summation order is not the definition's tap order, and the
// definition pins bits.  Everything is VALU f64 in the definition's order, / is the compiler's
// IEEE one and nothing is contracted (the Makefile's flags), so the maps are numpy's bit for bit
// (tests/test_gpu_metrics.py).
//
// The summary has a fixed shape and no floating-point atomics: a lane combines its two pixels and
// its two windows in that order; the wave's lanes combine by __shfl_xor at 32, 16, .., 1; the
// block's four waves fold in wave order through LDS; block b = by * blocks_x + bx writes partial b;
// im_fold's wave i folds value i: lane l the blocks [l * per, (l + 1) * per) in block order, then
// the same tree (se_fold_kernel's shape, restated here: moments.hip stays as it is).  The block
// count depends on (W, H) alone, so the same bits come back on every call and stream.
#include <hip/hip_runtime.h>

#include "render.h"

namespace rt {
namespace {

constexpr double kLr = 0.2126, kLg = 0.7152, kLb = 0.0722;  // luminance, the denoiser's
constexpr uint32_t kThreads = 256;
constexpr uint32_t kTaps = 11;
constexpr uint32_t kCoreW = kMetricsCoreW, kCoreH = kMetricsCoreH;           // 32 x 16
constexpr uint32_t kStW = kCoreW + kTaps - 1, kStH = kCoreH + kTaps - 1;     // 42 x 26 staged pixels
constexpr uint32_t kRowVals = 3 * kStW, kRawVals = kStH * kRowVals;          // 126, 3,276
constexpr uint32_t kStaged = kStW * kStH;                                    // 1,092
constexpr uint32_t kHPlane = kStH * kCoreW;                                  // 832
static_assert(kCoreW == 32 && kCoreH == 16 && kThreads == kCoreW * kCoreH / 2, "two core pixels a lane");
static_assert(5 * kHPlane >= kRawVals, "the h planes overlay the raw buffer");

struct ImParams {
    uint32_t width, height;
    double eps, c1, c2;
    double w[kTaps];
};

__device__ __forceinline__ bool finite(double v) { return fabs(v) < INFINITY; }

// summary value i of two partial results: 3 is a max, 6 a min, the others sums (counts are exact)
__device__ __forceinline__ double im_join(int i, double a, double b) {
    return i == 3 ? fmax(a, b) : (i == 6 ? fmin(a, b) : a + b);
}

// the block's 26 rows of 126 values into raw, widened to f64; outside the image: 0
template <int FMT>
__device__ __forceinline__ void stage_image(double* raw, const void* __restrict__ img, uint32_t W, uint32_t H,
                                            uint32_t x0, uint32_t y0) {
    constexpr uint32_t kTrips = (kRawVals + kThreads - 1) / kThreads;  // 13
    double v[kTrips];
#pragma unroll
    for (uint32_t t = 0; t < kTrips; ++t) {
        const uint32_t k = t * kThreads + threadIdx.x;
        const uint32_t row = k / kRowVals, col = k - row * kRowVals;
        const uint32_t y = y0 + row, x = x0 + col / 3;
        v[t] = 0.0;
        if (k < kRawVals && y < H && x < W) {
            const uint64_t at = 3 * ((uint64_t)y * W + x0) + col;  // <= 3 * (y * W + x) + 2 < 3 * W * H
            if (FMT == RT_METRICS_F64) v[t] = ((const double*)img)[at];
            else v[t] = (double)((const uint8_t*)img)[at];
        }
    }
#pragma unroll
    for (uint32_t t = 0; t < kTrips; ++t) {
        const uint32_t k = t * kThreads + threadIdx.x;
        if (k < kRawVals) raw[k] = v[t];
    }
}

__device__ __forceinline__ void luminance(const double* raw, double* plane) {
#pragma unroll
    for (uint32_t t = 0; t < (kStaged + kThreads - 1) / kThreads; ++t) {
        const uint32_t k = t * kThreads + threadIdx.x;
        if (k < kStaged) plane[k] = (kLr * raw[3 * k] + kLg * raw[3 * k + 1]) + kLb * raw[3 * k + 2];
    }
}

template <int FMT>
__global__ __launch_bounds__(kThreads) void im_tile(ImParams P, const void* __restrict__ img_a,
                                                    const void* __restrict__ img_b, double* __restrict__ rel,
                                                    double* __restrict__ ssim, double* __restrict__ part) {
    __shared__ double s_buf[5 * kHPlane];  // the raw image, then the five h planes
    __shared__ double s_y[2][kStaged];     // ya, yb
    __shared__ double s_red[kThreads / 64][8];
    const uint32_t W = P.width, H = P.height;
    const uint32_t x0 = blockIdx.x * kCoreW, y0 = blockIdx.y * kCoreH;
    const uint32_t lx = threadIdx.x & 31u, ly = threadIdx.x >> 5;  // the lane's core pixels: (lx, ly), (lx, ly + 8)
    const uint32_t x = x0 + lx;

    stage_image<FMT>(s_buf, img_a, W, H, x0, y0);
    __syncthreads();
    luminance(s_buf, s_y[0]);
    double a[2][3];
#pragma unroll
    for (uint32_t i = 0; i < 2; ++i)
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) a[i][c] = s_buf[3 * ((ly + 8 * i) * kStW + lx) + c];
    __syncthreads();
    stage_image<FMT>(s_buf, img_b, W, H, x0, y0);
    __syncthreads();
    luminance(s_buf, s_y[1]);

    // summary values 0..7 of this lane
    double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, INFINITY, 0.0};
#pragma unroll
    for (uint32_t i = 0; i < 2; ++i) {
        const uint32_t y = y0 + ly + 8 * i;
        const double* b = s_buf + 3 * ((ly + 8 * i) * kStW + lx);
        const double br = b[0], bg = b[1], bb = b[2];
        const double dr = a[i][0] - br, dg = a[i][1] - bg, db = a[i][2] - bb;
        const double se = (dr * dr + dg * dg) + db * db;
        const double rl = (dr * dr / (br * br + P.eps) + dg * dg / (bg * bg + P.eps)) + db * db / (bb * bb + P.eps);
        if (x < W && y < H) {
            if (rel) rel[(uint64_t)y * W + x] = rl;
            if (finite(a[i][0]) && finite(a[i][1]) && finite(a[i][2]) && finite(br) && finite(bg) && finite(bb)) {
                v[1] = v[1] + se;
                v[2] = v[2] + rl;
                v[3] = fmax(v[3], fmax(fmax(fabs(dr), fabs(dg)), fabs(db)));
            } else {
                v[0] = v[0] + 1.0;
            }
        }
    }
    __syncthreads();

    // horizontal: h_k[r][c] over q_k(c + i, r), i = 0..10 in order
#pragma unroll
    for (uint32_t t = 0; t < (kHPlane + kThreads - 1) / kThreads; ++t) {
        const uint32_t k = t * kThreads + threadIdx.x;  // = r * 32 + c
        if (k < kHPlane) {
            const double* pa = s_y[0] + (k >> 5) * kStW + (k & 31u);
            const double* pb = s_y[1] + (k >> 5) * kStW + (k & 31u);
            double ya = pa[0], yb = pb[0];
            double h0 = P.w[0] * ya, h1 = P.w[0] * yb, h2 = P.w[0] * (ya * ya), h3 = P.w[0] * (yb * yb),
                   h4 = P.w[0] * (ya * yb);
#pragma unroll
            for (uint32_t i = 1; i < kTaps; ++i) {
                ya = pa[i]; yb = pb[i];
                h0 = h0 + P.w[i] * ya;
                h1 = h1 + P.w[i] * yb;
                h2 = h2 + P.w[i] * (ya * ya);
                h3 = h3 + P.w[i] * (yb * yb);
                h4 = h4 + P.w[i] * (ya * yb);
            }
            s_buf[k] = h0;
            s_buf[kHPlane + k] = h1;
            s_buf[2 * kHPlane + k] = h2;
            s_buf[3 * kHPlane + k] = h3;
            s_buf[4 * kHPlane + k] = h4;
        }
    }
    __syncthreads();

    // vertical: v_k over h_k[oy + j][lx], j = 0..10 in order, then ssim of the window at (x, y)
#pragma unroll
    for (uint32_t i = 0; i < 2; ++i) {
        const uint32_t oy = ly + 8 * i, y = y0 + oy;
        const double* h = s_buf + oy * kCoreW + lx;
        double m[5];
#pragma unroll
        for (uint32_t k = 0; k < 5; ++k) m[k] = P.w[0] * h[k * kHPlane];
#pragma unroll
        for (uint32_t j = 1; j < kTaps; ++j)
#pragma unroll
            for (uint32_t k = 0; k < 5; ++k) m[k] = m[k] + P.w[j] * h[k * kHPlane + j * kCoreW];
        const double ma = m[0], mb = m[1];
        const double sa = m[2] - ma * ma, sb = m[3] - mb * mb, sab = m[4] - ma * mb;
        const double s = (((2.0 * ma) * mb + P.c1) * (2.0 * sab + P.c2)) /
                         (((ma * ma + mb * mb) + P.c1) * ((sa + sb) + P.c2));
        if ((uint64_t)x + kTaps <= W && (uint64_t)y + kTaps <= H) {  // the window exists
            if (ssim) ssim[(uint64_t)y * (W - (kTaps - 1)) + x] = s;
            if (finite(s)) {
                v[4] = v[4] + 1.0;
                v[5] = v[5] + s;
                v[6] = fmin(v[6], s);
            } else {
                v[7] = v[7] + 1.0;
            }
        }
    }

#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = im_join(i, v[i], __shfl_xor(v[i], off, 64));
    if ((threadIdx.x & 63u) == 0)
        for (int i = 0; i < 8; ++i) s_red[threadIdx.x >> 6][i] = v[i];
    __syncthreads();
    if (threadIdx.x < 8) {
        double r = s_red[0][threadIdx.x];
        for (uint32_t w = 1; w < kThreads / 64; ++w) r = im_join((int)threadIdx.x, r, s_red[w][threadIdx.x]);
        part[((uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * 8 + threadIdx.x] = r;
    }
}

// One block of 8 waves, wave i for summary value i.  The loads of four partials are issued
// together; they are joined one by one in block order.
__global__ __launch_bounds__(512) void im_fold(const double* __restrict__ part, uint32_t n_blocks,
                                               double* __restrict__ summary) {
    const uint32_t lane = threadIdx.x & 63u;
    const int i = (int)(threadIdx.x >> 6);
    const uint32_t per = (n_blocks + 63u) / 64u;
    const uint32_t first = min(n_blocks, lane * per), last = min(n_blocks, first + per);
    double r = i == 6 ? INFINITY : 0.0;
    uint32_t b = first;
    for (; b + 4 <= last; b += 4) {
        double p[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) p[k] = part[(uint64_t)(b + k) * 8 + i];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) r = im_join(i, r, p[k]);
    }
    for (; b < last; ++b) r = im_join(i, r, part[(uint64_t)b * 8 + i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) r = im_join(i, r, __shfl_xor(r, off, 64));
    if (lane == 0) summary[i] = r;
}

}  // namespace

uint64_t metrics_blocks(uint32_t width, uint32_t height) {
    return (uint64_t)((width + kCoreW - 1) / kCoreW) * ((height + kCoreH - 1) / kCoreH);
}

hipError_t launch_image_metrics(const MetricsSettings& S, const void* a, const void* b, double* rel, double* ssim,
                                double* summary, double* part, hipStream_t st) {
    ImParams P;
    P.width = S.width; P.height = S.height;
    P.eps = S.eps;
    P.c1 = (0.01 * S.peak) * (0.01 * S.peak);
    P.c2 = (0.03 * S.peak) * (0.03 * S.peak);
    for (uint32_t i = 0; i < kTaps; ++i) P.w[i] = S.window[i];
    const dim3 grid((S.width + kCoreW - 1) / kCoreW, (S.height + kCoreH - 1) / kCoreH);
    const auto kernel = S.format == RT_METRICS_F64 ? im_tile<RT_METRICS_F64> : im_tile<RT_METRICS_U8>;
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, st, P, a, b, rel, ssim, part);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(im_fold, dim3(1), dim3(512), 0, st, (const double*)part, (uint32_t)(grid.x * grid.y), summary);
    return hipGetLastError();
}

}  // namespace rt

// denoise.hip — the variance-guided à-trous filter of rt_denoise_async and the pixel-centre
// camera rays of rt_camera_rays_async (the definition: include/rt_api.h):
//
//   dn_camera_rays  camera_dir's arithmetic (render.hip) at the pixel centres
//   dn_prepare      mean, second moment, rays and first hits -> the working records
//   dn_prepare_counts  the same with every pixel's own sample count (rt_denoise_counts_async)
//   dn_atrous       one iteration of the filter, launched once per step s = 2^i
//
// Working records, 96 B a pixel in the caller's workspace: two colour buffers of
// {r, g, b, var} f64 (32 B, read and written as two 16-byte words; the iterations ping-pong
// between them) and one guide of {nx, ny, nz, t, px, py, pz} f32 + flags (32 B, written once).
// Whether a pixel is "ok" changes from one iteration to the next (a missing pixel gets
// filled), so it travels with the colour: a pixel that is not ok carries kNotOk, one NaN
// bit pattern, in place of var.  No arithmetic makes that pattern: the hardware's own NaN is
// the canonical one, and a NaN of the inputs never reaches an ok pixel's var, since a
// pixel that is not ok is staged as zeros.  A pixel that is not ok has never been ok, so the
// var it passes through is its first one: dn_prepare writes that to out_var itself, and
// the last iteration leaves it alone.
//
// dn_prepare stages its four inputs through LDS: a block takes 256 pixels, whose mean, sq,
// rays and hits are contiguous ranges of 6, 6, 12 and 16 KiB; the lanes copy them by 16-byte
// words in address order (whole 128-byte lines per load instruction, and every byte of the
// 24-byte pixels and of the hits' lines is fetched once), then each lane picks its own
// pixel's fields out of LDS.  Records of an even number of doubles get one double of padding
// (strides 7 and 9), so that a half-wave's 8-byte reads fall on 32 different bank pairs, as
// the 3-double pixels do by themselves.  The records go out as two 16-byte stores a lane,
// neighbouring lanes to neighbouring records: a wave's two stores cover the same 2 KiB.
//
// dn_atrous.  For step s the pixels that agree in (x mod s, y mod s) form a lattice on which
// the filter is a dense 5x5.  A block takes a 16x16 tile of one lattice, one output pixel a
// lane, and stages the tile's 20x20 lattice points (halo 2) into LDS once, so a record is read
// from global memory once per block, not 25 times, and LDS footprint and code are the same
// for every step.  A point outside the image, or one that is not ok, is staged as zeros with
// its ok flag clear: its tap weight is then 0 by the definition itself, and the 25 unrolled
// taps have no bounds tests.
//
// LDS holds planes, not records: r, g, b, var as f64 and the guide's eight words as 32-bit.
// A wave's 64 lanes are 4 tile rows of 16, and a tap reads, per plane, element
// base + pitch * j + lx for row j = 0..3 and lx = 0..15.  With pitch 48 elements:
//   4-byte planes: 48 * j mod 64 = 0, 48, 32, 16, four disjoint runs of 16: the 64 lanes read 64
//     different banks (with 32 banks, a pass of 32 lanes: 48 mod 32 = 16, two disjoint runs);
//   8-byte planes: a pass serves 32 lanes, rows j and j + 1, and 48 mod 32 = 16: 32 different
//     bank pairs.
// A pitch has to be 16 mod 32 for this and at least 20, so 48 it is — and the 28 columns a
// 20-wide row leaves free hold a second plane, at column 24: the same banks, shifted.  So
// two planes share an array [20][2][24], 7,680 B for an f64 pair; two f64 arrays and four
// 32-bit arrays are 30,720 B a block.  (Records of 64 B would put the 16 lanes of a row on 4
// banks' worth of stride: 4-way conflicts on every tap.)
//
// The centre pixel's normal, position, sigma_z * t, luminance and sigma_l * sqrt(var) + eps
// stay in registers.  Arithmetic is f64 in the definition's order; / and sqrt are the
// compiler's IEEE ones and nothing is contracted (the Makefile's flags), which round as
// the host's do (tests/test_gpu_parity.py test_fp64_rounding_matches_host), so the output
// is numpy's, bit for bit (tests/test_gpu_denoise.py).
#include <hip/hip_runtime.h>

#include "render.h"
#include "rt_math.h"

namespace rt {
namespace {

constexpr double kLr = 0.2126, kLg = 0.7152, kLb = 0.0722;  // luminance
constexpr uint32_t kHit = 1u, kOk = 2u;                    // guide flags
constexpr unsigned long long kNotOk = 0x7ff8dead00000001ull;  // in place of var: the pixel is not ok
constexpr int kTile = 16, kHalo = 2, kSide = kTile + 2 * kHalo, kHalf = 24;
constexpr uint32_t kThreads = kTile * kTile;
static_assert((2 * kHalf) % 32 == 16 && kHalf >= kSide, "the bank argument above");

__device__ __forceinline__ bool finite(double v) { return fabs(v) < INFINITY; }
__device__ __forceinline__ bool is_ok(double var) { return (unsigned long long)__double_as_longlong(var) != kNotOk; }
__device__ __forceinline__ double lum(double r, double g, double b) { return (kLr * r + kLg * g) + kLb * b; }

// ---------------------------------------------------------------- camera rays ----
struct DnCamera {
    uint32_t width, height;
    double fw, fh, tan_x, tan_y;
    double pos[3], right[3], up[3], fwd[3];
};

// render.hip camera_dir with fx = px + 0.5, fy = py + 0.5 in place of the two draws
// (camera.rs:48-55), restated here so that the path kernels' code stays as it is; normalize
// is rt_math.h's v * (1 / |v|), whose bits camera_dir's nrm reproduces (rt_device.h).
__global__ __launch_bounds__(256) void dn_camera_rays(DnCamera C, double2* __restrict__ rays) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint64_t)C.width * C.height) return;
    const double fx = (double)(uint32_t)(i % C.width) + 0.5, fy = (double)(uint32_t)(i / C.width) + 0.5;
    const double x = (2.0 * fx / C.fw - 1.0) * C.tan_x;
    const double y = -(2.0 * fy / C.fh - 1.0) * C.tan_y;
    const V3 d = normalize((load3(C.right) * x + load3(C.up) * y) + load3(C.fwd) * 1.0);
    rays[3 * i] = make_double2(C.pos[0], C.pos[1]);
    rays[3 * i + 1] = make_double2(C.pos[2], d.x);
    rays[3 * i + 2] = make_double2(d.y, d.z);
}

// -------------------------------------------------------------------- prepare ----
// index of double d of a block's staged records of R doubles each
template <int R>
__device__ __forceinline__ uint32_t padded(uint32_t d) { return R % 2 ? d : d + d / R; }
template <int R>
constexpr uint32_t staged_doubles() { return kThreads * (R % 2 ? R : R + 1); }

// the block's 256 records of R doubles, of an array of n_doubles in all, by 16-byte words
template <int R>
__device__ __forceinline__ void stage_records(double* lds, const double* __restrict__ g, uint64_t n_doubles) {
    const uint64_t first = (uint64_t)blockIdx.x * (kThreads * R);
    for (uint32_t w = threadIdx.x; w < kThreads * R / 2; w += kThreads) {
        const uint64_t d = first + 2 * w;
        double2 a = make_double2(0.0, 0.0);
        if (d + 1 < n_doubles) a = *(const double2*)(g + d);
        else if (d < n_doubles) a.x = g[d];  // the last double of an odd count
        lds[padded<R>(2 * w)] = a.x;
        lds[padded<R>(2 * w + 1)] = a.y;
    }
}

__global__ __launch_bounds__(kThreads) void dn_prepare(const double* __restrict__ mean, const double* __restrict__ sq,
                                                       const double* __restrict__ rays, const double* __restrict__ hits,
                                                       uint64_t n, double denom, double2* __restrict__ colour,
                                                       uint4* __restrict__ guide, double* __restrict__ out_var) {
    __shared__ double s_mean[staged_doubles<3>()], s_sq[staged_doubles<3>()];
    __shared__ double s_ray[staged_doubles<6>()], s_hit[staged_doubles<8>()];
    stage_records<3>(s_mean, mean, n * 3);
    stage_records<3>(s_sq, sq, n * 3);
    stage_records<6>(s_ray, rays, n * 6);
    stage_records<8>(s_hit, hits, n * 8);
    __syncthreads();
    const uint32_t l = threadIdx.x;
    const uint64_t pix = (uint64_t)blockIdx.x * kThreads + l;
    if (pix >= n) return;
    double m[3], v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        m[c] = s_mean[3 * l + c];
        const double d = s_sq[3 * l + c] - m[c] * m[c];  // below 0 by rounding only: clamped; a NaN stays
        v[c] = (d < 0.0 ? 0.0 : d) / denom;
    }
    const double var = ((kLr * kLr) * v[0] + (kLg * kLg) * v[1]) + (kLb * kLb) * v[2];
    const bool ok = finite(m[0]) && finite(m[1]) && finite(m[2]) && finite(var);
    colour[2 * pix] = make_double2(m[0], m[1]);
    colour[2 * pix + 1] = make_double2(m[2], ok ? var : __longlong_as_double((long long)kNotOk));
    if (out_var) out_var[pix] = var;
    // rt_hit as 8 doubles: t, geometry_normal, shading_normal, {inside, prim}
    const double* h = s_hit + 9 * l;
    const double* r = s_ray + 7 * l;
    const double t = h[0];
    const bool hit = (int32_t)(__double_as_longlong(h[7]) >> 32) != RT_HIT_MISS;
    uint4 a, b;
    a.x = __float_as_uint((float)h[4]);
    a.y = __float_as_uint((float)h[5]);
    a.z = __float_as_uint((float)h[6]);
    a.w = __float_as_uint((float)t);
    b.x = __float_as_uint((float)(r[0] + t * r[3]));
    b.y = __float_as_uint((float)(r[1] + t * r[4]));
    b.z = __float_as_uint((float)(r[2] + t * r[5]));
    b.w = (hit ? kHit : 0u) | (ok ? kOk : 0u);
    guide[2 * pix] = a;
    guide[2 * pix + 1] = b;
}

// dn_prepare with the pixel's own sample count in place of the frame's (rt_denoise_counts_async):
// denom is count - 1, and a pixel with fewer than two samples is not ok.  The rest is dn_prepare's,
// restated: shared through a function, dn_prepare itself compiles to other registers, and that
// kernel stays as it was.  Lane l needs the count of pixel l and of no other, so the block's
// 1 KiB of counts is one 4-byte load a lane, whole lines a wave, started before the staging
// loops so that it is in flight with them; a trip through LDS would add a store and a load
// and move the same bytes.
__global__ __launch_bounds__(kThreads) void dn_prepare_counts(const double* __restrict__ mean,
                                                              const double* __restrict__ sq,
                                                              const double* __restrict__ rays,
                                                              const double* __restrict__ hits,
                                                              const uint32_t* __restrict__ count, uint64_t n,
                                                              double2* __restrict__ colour, uint4* __restrict__ guide,
                                                              double* __restrict__ out_var) {
    __shared__ double s_mean[staged_doubles<3>()], s_sq[staged_doubles<3>()];
    __shared__ double s_ray[staged_doubles<6>()], s_hit[staged_doubles<8>()];
    const uint64_t own = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint32_t cnt = own < n ? count[own] : 0u;
    const double denom = (double)cnt - 1.0;
    stage_records<3>(s_mean, mean, n * 3);
    stage_records<3>(s_sq, sq, n * 3);
    stage_records<6>(s_ray, rays, n * 6);
    stage_records<8>(s_hit, hits, n * 8);
    __syncthreads();
    const uint32_t l = threadIdx.x;
    const uint64_t pix = (uint64_t)blockIdx.x * kThreads + l;
    if (pix >= n) return;
    double m[3], v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        m[c] = s_mean[3 * l + c];
        const double d = s_sq[3 * l + c] - m[c] * m[c];  // below 0 by rounding only: clamped; a NaN stays
        v[c] = (d < 0.0 ? 0.0 : d) / denom;
    }
    const double var = ((kLr * kLr) * v[0] + (kLg * kLg) * v[1]) + (kLb * kLb) * v[2];
    const bool ok = cnt >= 2 && finite(m[0]) && finite(m[1]) && finite(m[2]) && finite(var);
    colour[2 * pix] = make_double2(m[0], m[1]);
    colour[2 * pix + 1] = make_double2(m[2], ok ? var : __longlong_as_double((long long)kNotOk));
    if (out_var) out_var[pix] = var;
    // rt_hit as 8 doubles: t, geometry_normal, shading_normal, {inside, prim}
    const double* h = s_hit + 9 * l;
    const double* r = s_ray + 7 * l;
    const double t = h[0];
    const bool hit = (int32_t)(__double_as_longlong(h[7]) >> 32) != RT_HIT_MISS;
    uint4 a, b;
    a.x = __float_as_uint((float)h[4]);
    a.y = __float_as_uint((float)h[5]);
    a.z = __float_as_uint((float)h[6]);
    a.w = __float_as_uint((float)t);
    b.x = __float_as_uint((float)(r[0] + t * r[3]));
    b.y = __float_as_uint((float)(r[1] + t * r[4]));
    b.z = __float_as_uint((float)(r[2] + t * r[5]));
    b.w = (hit ? kHit : 0u) | (ok ? kOk : 0u);
    guide[2 * pix] = a;
    guide[2 * pix + 1] = b;
}

// --------------------------------------------------------------------- filter ----
struct DnFilter {
    uint32_t width, height;
    uint32_t step;         // s = 2^i
    uint32_t lattices_x;   // min(s, width): blockIdx.x = tile_x * lattices_x + phase_x, and so for y
    uint32_t lattices_y;
    uint32_t squarings;
    double sigma_l, sigma_z, eps;
};

// h = (1/16, 1/4, 3/8, 1/4, 1/16); the taps are unrolled, so h[dy] * h[dx] folds to a literal
__device__ constexpr double tap_h(int i) { return i == 2 ? 3.0 / 8 : (i == 1 || i == 3 ? 1.0 / 4 : 1.0 / 16); }

// 5 waves a SIMD: five blocks' LDS (30,720 B each) fit a CU's 160 KiB.
// SQ >= 0: the squarings, a compile-time count (the default's instance); SQ < 0: P.squarings of them,
// as a chain of kMaxSquarings products each picked by a select (a loop with a uniform trip count
// would not diverge, but it cuts every tap into basic blocks, and the allocator then spills 327).
// out != nullptr: the last iteration, which writes [H][W][3] (and out_var where the pixel is ok)
// in place of dst.
template <int SQ>
__global__ __launch_bounds__(kThreads, 5) void dn_atrous(const double2* __restrict__ src, const uint4* __restrict__ guide,
                                                         double2* __restrict__ dst, double* __restrict__ out,
                                                         double* __restrict__ out_var, DnFilter P) {
    __shared__ double s_c[2][kSide][2][kHalf];    // planes r g | b var
    __shared__ uint32_t s_g[4][kSide][2][kHalf];  // planes nx ny | nz t | px py | pz flags
    const int step = (int)P.step;
    const int phx = (int)(blockIdx.x % P.lattices_x), phy = (int)(blockIdx.y % P.lattices_y);
    const int u0 = (int)(blockIdx.x / P.lattices_x) * kTile, v0 = (int)(blockIdx.y / P.lattices_y) * kTile;
    // the tile's first pixel is outside the image: a lattice with fewer points than the largest one
    if (phx + step * u0 >= (int)P.width || phy + step * v0 >= (int)P.height) return;

    for (int k = (int)threadIdx.x; k < kSide * kSide; k += (int)kThreads) {
        const int row = k / kSide, col = k % kSide;
        const int u = u0 - kHalo + col, v = v0 - kHalo + row;
        const int x = phx + step * u, y = phy + step * v;
        double2 c0 = make_double2(0.0, 0.0), c1 = c0;
        uint4 g0 = make_uint4(0u, 0u, 0u, 0u), g1 = g0;
        if (u >= 0 && v >= 0 && x < (int)P.width && y < (int)P.height) {
            const size_t pix = (size_t)y * P.width + (size_t)x;
            c0 = src[2 * pix]; c1 = src[2 * pix + 1];
            g0 = guide[2 * pix]; g1 = guide[2 * pix + 1];
            const bool ok = is_ok(c1.y);
            if (!ok) c0 = c1 = make_double2(0.0, 0.0);
            g1.w = (g1.w & kHit) | (ok ? kOk : 0u);
        }
        s_c[0][row][0][col] = c0.x; s_c[0][row][1][col] = c0.y;
        s_c[1][row][0][col] = c1.x; s_c[1][row][1][col] = c1.y;
        s_g[0][row][0][col] = g0.x; s_g[0][row][1][col] = g0.y;
        s_g[1][row][0][col] = g0.z; s_g[1][row][1][col] = g0.w;
        s_g[2][row][0][col] = g1.x; s_g[2][row][1][col] = g1.y;
        s_g[3][row][0][col] = g1.z; s_g[3][row][1][col] = g1.w;
    }
    __syncthreads();

    const int cx = (int)(threadIdx.x & 15u) + kHalo, cy = (int)(threadIdx.x >> 4) + kHalo;
    const int x = phx + step * (u0 + cx - kHalo), y = phy + step * (v0 + cy - kHalo);
    if (x >= (int)P.width || y >= (int)P.height) return;
    const size_t pix = (size_t)y * P.width + (size_t)x;

    const uint32_t fp = s_g[3][cy][1][cx];
    const bool ok_p = (fp & kOk) != 0;
    const V3 n_p = v3((double)__uint_as_float(s_g[0][cy][0][cx]), (double)__uint_as_float(s_g[0][cy][1][cx]),
                      (double)__uint_as_float(s_g[1][cy][0][cx]));
    const V3 x_p = v3((double)__uint_as_float(s_g[2][cy][0][cx]), (double)__uint_as_float(s_g[2][cy][1][cx]),
                      (double)__uint_as_float(s_g[3][cy][0][cx]));
    const double dz = P.sigma_z * (double)__uint_as_float(s_g[1][cy][1][cx]);
    const double lum_p = lum(s_c[0][cy][0][cx], s_c[0][cy][1][cx], s_c[1][cy][0][cx]);
    const double dl = P.sigma_l * sqrt(s_c[1][cy][1][cx]) + P.eps;

    double sw = 0.0, sr = 0.0, sg = 0.0, sb = 0.0, sv = 0.0;
#pragma unroll
    for (int dy = -kHalo; dy <= kHalo; ++dy) {
#pragma unroll
        for (int dx = -kHalo; dx <= kHalo; ++dx) {
            const int r = cy + dy, c = cx + dx;
            const uint32_t fq = s_g[3][r][1][c];
            const double qr = s_c[0][r][0][c], qg = s_c[0][r][1][c], qb = s_c[1][r][0][c], qv = s_c[1][r][1][c];
            const V3 n_q = v3((double)__uint_as_float(s_g[0][r][0][c]), (double)__uint_as_float(s_g[0][r][1][c]),
                              (double)__uint_as_float(s_g[1][r][0][c]));
            const V3 x_q = v3((double)__uint_as_float(s_g[2][r][0][c]), (double)__uint_as_float(s_g[2][r][1][c]),
                              (double)__uint_as_float(s_g[3][r][0][c]));
            // every value is computed whether it is needed or not and picked by a select, so the 25
            // taps are one straight line of code
            const double nn = dot(n_p, n_q);
            double wn = nn < 0.0 ? 0.0 : nn;
#pragma unroll
            for (uint32_t k = 0; k < (SQ < 0 ? kMaxSquarings : (uint32_t)SQ); ++k) {
                const double w2 = wn * wn;
                wn = SQ >= 0 || k < P.squarings ? w2 : wn;
            }
            const double xz = fabs(dot(n_p, x_q - x_p)) / dz;
            const double wz = 1.0 / (1.0 + xz * xz);
            const double wg_hits = wn * wz, wg_else = ((fp | fq) & kHit) ? 0.0 : 1.0;
            const double wg = (fp & fq & kHit) ? wg_hits : wg_else;
            const double xl_ok = (lum(qr, qg, qb) - lum_p) / dl;
            const double xl = ok_p ? xl_ok : 0.0;  // p not ok: w_l = 1 / (1 + 0) = 1
            const double wl = 1.0 / (1.0 + xl * xl);
            const double w_ok = (tap_h(dy + kHalo) * tap_h(dx + kHalo)) * (wg * wl);
            const double w = (fq & kOk) ? w_ok : 0.0;
            sw = sw + w;
            sr = sr + w * qr;
            sg = sg + w * qg;
            sb = sb + w * qb;
            sv = sv + (w * w) * qv;
        }
        // a row of taps at a time: without it the scheduler starts all 25 taps' loads at once
        // and spills; with it the kernel takes 96 VGPRs, which is the 5 waves a SIMD that LDS allows
        __builtin_amdgcn_sched_barrier(0);
    }

    // the quotients come first and the rare pass-through overwrites them: were they inside an
    // if (sw > 0), the compiler would move the sums in there too, and keep every tap's weight
    // and colours live until the end
    double2 c0 = make_double2(sr / sw, sg / sw);
    double2 c1 = make_double2(sb / sw, sv / (sw * sw));
    if (!(sw > 0.0)) {  // nothing to average (or a NaN weight): the pixel passes through as it is
        c0 = src[2 * pix];
        c1 = src[2 * pix + 1];
    }
    if (out) {
        out[3 * pix] = c0.x;
        out[3 * pix + 1] = c0.y;
        out[3 * pix + 2] = c1.x;
        if (out_var && is_ok(c1.y)) out_var[pix] = c1.y;  // not ok: dn_prepare's var stays
    } else {
        dst[2 * pix] = c0;
        dst[2 * pix + 1] = c1;
    }
}

}  // namespace

hipError_t launch_camera_rays(const KParams& k, double* rays, hipStream_t st) {
    DnCamera C;
    C.width = k.width; C.height = k.height;
    C.fw = k.fw; C.fh = k.fh; C.tan_x = k.tan_x; C.tan_y = k.tan_y;
    for (int i = 0; i < 3; ++i) {
        C.pos[i] = k.cam_pos[i]; C.right[i] = k.cam_right[i]; C.up[i] = k.cam_up[i]; C.fwd[i] = k.cam_fwd[i];
    }
    const uint64_t n = (uint64_t)k.width * k.height;
    hipLaunchKernelGGL(dn_camera_rays, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, C, (double2*)rays);
    return hipGetLastError();
}

uint64_t denoise_buffer_bytes(uint64_t n_pixels) { return (n_pixels * 32 + 255) / 256 * 256; }

hipError_t launch_denoise(const DenoiseSettings& S, const double* mean, const double* sq, const double* rays,
                          const rt_hit* hits, double* out, double* out_var, void* workspace, hipStream_t st,
                          const uint32_t* count) {
    const uint64_t n = (uint64_t)S.width * S.height, buf = denoise_buffer_bytes(n);
    double2* colour[2] = {(double2*)workspace, (double2*)((char*)workspace + buf)};
    uint4* guide = (uint4*)((char*)workspace + 2 * buf);
    const dim3 blocks((unsigned)((n + kThreads - 1) / kThreads));
    if (count)
        hipLaunchKernelGGL(dn_prepare_counts, blocks, dim3(kThreads), 0, st, mean, sq, rays, (const double*)hits, count,
                           n, colour[0], guide, out_var);
    else
        hipLaunchKernelGGL(dn_prepare, blocks, dim3(kThreads), 0, st, mean, sq, rays, (const double*)hits, n,
                           (double)S.spp - 1.0, colour[0], guide, out_var);
    hipError_t e = hipGetLastError();
    for (uint32_t i = 0; i < S.iterations && e == hipSuccess; ++i) {
        DnFilter P;
        P.width = S.width; P.height = S.height; P.step = 1u << i;
        P.lattices_x = P.step < S.width ? P.step : S.width;
        P.lattices_y = P.step < S.height ? P.step : S.height;
        P.squarings = S.squarings; P.sigma_l = S.sigma_l; P.sigma_z = S.sigma_z; P.eps = S.eps;
        // tiles of the largest lattice (phase 0) times the lattices; smaller lattices' spare tiles exit
        const uint32_t tiles_x = ((S.width + P.step - 1) / P.step + kTile - 1) / kTile;
        const uint32_t tiles_y = ((S.height + P.step - 1) / P.step + kTile - 1) / kTile;
        const bool last = i + 1 == S.iterations;
        const auto kernel = S.squarings == RT_DENOISE_NORMAL_SQUARINGS ? dn_atrous<(int)RT_DENOISE_NORMAL_SQUARINGS>
                                                                       : dn_atrous<-1>;
        hipLaunchKernelGGL(kernel, dim3(tiles_x * P.lattices_x, tiles_y * P.lattices_y), dim3(kThreads), 0, st,
                           colour[i & 1], guide, colour[(i + 1) & 1], last ? out : nullptr, last ? out_var : nullptr, P);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace rt

// temporal.hip — temporal accumulation, rt_temporal_accumulate_async (the definition: include/rt_api.h,
// DESIGN.md §4): every pixel of the current frame is reprojected into the previous camera, takes up
// to four taps of the previous frame's history there, and merges what they agree on with its own
// (mean, second moment, count).
//
//   tp_accumulate<true>   taps from a window of the history staged in LDS where the block's taps fit
//                         one, from global memory where they do not
//   tp_accumulate<false>  every tap from global memory (RT_TEMPORAL_NO_WINDOW): no window in LDS
//
// History, 80 B a pixel in the caller's block: a guide record of 32 B, {nx, ny, nz, px, py, pz} f32,
// count and flags u32 (two 16-byte words), and a colour record of 48 B, mean and sq as six f64
// (three 16-byte words); the two arrays follow each other, each rounded up to 256 B.
//
// A block takes one 16x16 tile of the current frame, one pixel a lane (lane l: column l & 15, row
// l >> 4, so a wave is four tile rows), and uses one piece of LDS three times over:
//
// 1. Inputs.  A tile row's mean, sq, rays and hits are contiguous runs of 384, 384, 768 and 1024 B.
//    The lanes copy them by 16-byte words in address order, as dn_prepare does (denoise.hip): a
//    wave's load covers 1 KiB of whole lines, and every byte of the 24-byte pixels is fetched once.
//    A row that starts on an odd double (odd widths) takes one word more, whose other half belongs
//    to the neighbouring tile.  Each lane then picks its pixel's 23 values out of LDS; records of
//    an even number of doubles are padded by one (strides 7 and 9), dn_prepare's bank argument.
//    The counts, 4 B a lane, are loaded directly before the staging so that they are in flight
//    with it.
//
// 2. Taps.  Each lane reprojects its pixel in f64 and, where it has a candidate, knows the 2x2
//    footprint (x0, y0) .. (x0 + 1, y0 + 1) of its taps.  Under coherent motion the footprints of
//    neighbouring lanes overlap almost entirely: four gathers a lane fetch each record about four
//    times.  So the block reduces the bounding box of its candidates' footprints (four
//    butterflies of wave shuffles, one exchange of the four waves' results through LDS), and when
//    the box is at most kSide = 24 columns and rows it stages the box's guide and colour records,
//    clipped to the image, into LDS once: row by row, each row a contiguous run of 16-byte words
//    that the lanes take in address order.  A static camera needs 17 or 18 columns, a pan the
//    same, so 24 leaves room for a mild zoom or roll; a block whose box does not fit (zoom, fast
//    rotation, parallax across a depth edge) reads its taps from global memory: the guide record
//    first, and the 48-byte colour record only for a valid tap.
//
//    LDS holds planes, not records, in denoise.hip's arrangement: the guide's eight 32-bit words
//    and the colour's six doubles, two planes to an array [24][2][24], so a plane's row pitch is
//    48 elements.  When the motion is a translation, a tap's 64 lanes read, per plane, element
//    base + 48 * j + lx for tile row j = 0..3 and lx = 0..15:
//      4-byte planes: 48 * j mod 64 = 0, 48, 32, 16, four disjoint runs of 16: 64 different banks
//        (with 32 banks, a pass of 32 lanes: 48 mod 32 = 16, two disjoint runs);
//      8-byte planes: a pass serves 32 lanes, rows j and j + 1, and 48 mod 32 = 16: 32 different
//        bank pairs.
//    (Records of 32 B and 48 B would put a row's 16 lanes on strides of 8 and 12 banks: 4-way
//    and 6-way conflicts on every read.)  Three f64 arrays and four 32-bit arrays are 46,080 B,
//    about what the inputs took (45,056 B): three blocks a CU, three waves a SIMD.
//
//    Both paths hand the same values to the same function in the same order, so they produce the
//    same bits (tests/test_gpu_temporal.py runs pan and zoom both ways).
//
// 3. Outputs.  The new history records go out as whole 16-byte words, neighbouring lanes to
//    neighbouring records (a tile row: 512 B of guide, 768 B of colour).  out_mean and out_sq are
//    24-byte pixels, so they go back through LDS and out by rows of 16-byte words, the way the
//    inputs came in; only a row's first or last double, where it shares its word with the
//    neighbouring tile, is stored alone.
//
// Arithmetic is f64 in the definition's order; / and floor are IEEE and nothing is contracted
// (the Makefile's flags), so the outputs are numpy's, bit for bit.
#include <hip/hip_runtime.h>

#include <climits>

#include "render.h"
#include "rt_math.h"

namespace rt {
namespace {

constexpr int kTile = 16, kSide = 24, kHalf = 24;
constexpr uint32_t kThreads = kTile * kTile;
constexpr uint32_t kHit = 1u;              // guide flags
constexpr uint32_t kMaxCount = 1u << 30;   // what a pixel's own count is clamped to
static_assert((2 * kHalf) % 32 == 16 && kHalf >= kSide && kSide >= kTile + 2 && kSide <= 32, "the bank argument above");

// doubles of LDS: the staged inputs (mean 3, sq 3, rays 6 + 1, hits 8 + 1 a pixel), and the window's planes
constexpr uint32_t kInDoubles = kThreads * (3 + 3 + 7 + 9);
constexpr uint32_t kWinDoubles = 3 * kSide * 2 * kHalf + 4 * kSide * 2 * kHalf / 2;

__device__ __forceinline__ bool finite(double v) { return fabs(v) < INFINITY; }

// index of double d of a tile's staged records of R doubles each (dn_prepare's padding)
template <int R>
__device__ __forceinline__ uint32_t padded(uint32_t d) { return R % 2 ? d : d + d / R; }

// f(row, word) for every 16-byte word of `rows` runs of `words` words each, lanes in address order
template <typename F>
__device__ __forceinline__ void for_words(uint32_t words, uint32_t rows, F f) {
    uint32_t row = threadIdx.x / words, word = threadIdx.x % words;
    const uint32_t rows_step = kThreads / words, words_step = kThreads % words;
    while (row < rows) {
        f(row, word);
        row += rows_step;
        word += words_step;
        if (word >= words) { word -= words; ++row; }
    }
}

// A tile's records of R doubles each, of an array [H][W][R] of n_doubles in all: tile row r is the
// doubles [d0, d1) from pixel first + r * width on, fetched as the 16-byte words that cover them.
template <int R>
__device__ __forceinline__ void stage_rows(double* lds, const double* __restrict__ g, uint64_t n_doubles, uint64_t first,
                                           uint32_t width, uint32_t cols, uint32_t rows) {
    constexpr uint32_t kWords = kTile * R / 2 + 1;  // one more for a row that starts on an odd double
    for (uint32_t k = threadIdx.x; k < rows * kWords; k += kThreads) {
        const uint32_t r = k / kWords, w = k % kWords;
        const uint64_t d0 = (first + (uint64_t)r * width) * R, d1 = d0 + (uint64_t)cols * R;
        const uint64_t e = (d0 & ~1ull) + 2 * w;
        if (e >= d1) continue;
        double2 a = make_double2(0.0, 0.0);
        if (e + 1 < n_doubles) a = *(const double2*)(g + e);
        else a.x = g[e];  // the last double of an odd count
        const uint32_t base = r * kTile * R;
        if (e >= d0) lds[padded<R>(base + (uint32_t)(e - d0))] = a.x;
        if (e + 1 < d1) lds[padded<R>(base + (uint32_t)(e + 1 - d0))] = a.y;
    }
}

// The way back for records of 3 doubles: whole words, but for a row's first or last double where the
// other half of its word is the neighbouring tile's.
__device__ __forceinline__ void unstage_rows(const double* lds, double* __restrict__ g, uint64_t first, uint32_t width,
                                             uint32_t cols, uint32_t rows) {
    constexpr uint32_t R = 3, kWords = kTile * R / 2 + 1;
    for (uint32_t k = threadIdx.x; k < rows * kWords; k += kThreads) {
        const uint32_t r = k / kWords, w = k % kWords;
        const uint64_t d0 = (first + (uint64_t)r * width) * R, d1 = d0 + (uint64_t)cols * R;
        const uint64_t e = (d0 & ~1ull) + 2 * w;
        if (e >= d1) continue;
        const uint32_t base = r * kTile * R;
        const bool lo = e >= d0, hi = e + 1 < d1;
        if (lo && hi) *(double2*)(g + e) = make_double2(lds[base + (uint32_t)(e - d0)], lds[base + (uint32_t)(e + 1 - d0)]);
        else if (lo) g[e] = lds[base + (uint32_t)(e - d0)];
        else if (hi) g[e + 1] = lds[base + (uint32_t)(e + 1 - d0)];
    }
}

// the centre pixel's side of a tap's test: its guide rounded to f32 and widened back
struct Centre {
    V3 n, x;
    double tol_t;  // plane_tol * t_p
    double normal_min;
};

// the sums over the valid taps, in tap order
struct Sums {
    double sw, sm[3], ss[3];
    uint32_t n_min;
};

__device__ __forceinline__ bool tap_valid(const Centre& C, uint4 g0, uint4 g1) {
    const V3 n_q = v3((double)__uint_as_float(g0.x), (double)__uint_as_float(g0.y), (double)__uint_as_float(g0.z));
    const V3 x_q = v3((double)__uint_as_float(g0.w), (double)__uint_as_float(g1.x), (double)__uint_as_float(g1.y));
    return g1.z >= 1u && (g1.w & kHit) != 0 && dot(C.n, n_q) >= C.normal_min && fabs(dot(C.n, x_q - C.x)) <= C.tol_t;
}

__device__ __forceinline__ void tap_add(Sums& S, bool valid, double b, double2 c0, double2 c1, double2 c2, uint32_t count) {
    S.sw = valid ? S.sw + b : S.sw;
    S.sm[0] = valid ? S.sm[0] + b * c0.x : S.sm[0];
    S.sm[1] = valid ? S.sm[1] + b * c0.y : S.sm[1];
    S.sm[2] = valid ? S.sm[2] + b * c1.x : S.sm[2];
    S.ss[0] = valid ? S.ss[0] + b * c1.y : S.ss[0];
    S.ss[1] = valid ? S.ss[1] + b * c2.x : S.ss[1];
    S.ss[2] = valid ? S.ss[2] + b * c2.y : S.ss[2];
    S.n_min = valid && count < S.n_min ? count : S.n_min;
}

template <bool kWindow>
__global__ __launch_bounds__(kThreads, 3) void tp_accumulate(TemporalSettings P, const double* __restrict__ mean,
                                                             const double* __restrict__ sq,
                                                             const uint32_t* __restrict__ count,
                                                             const double* __restrict__ rays,
                                                             const double* __restrict__ hits,
                                                             const uint4* __restrict__ guide_prev,
                                                             const double2* __restrict__ colour_prev,
                                                             uint4* __restrict__ guide_next, double2* __restrict__ colour_next,
                                                             double* __restrict__ out_mean, double* __restrict__ out_sq,
                                                             uint32_t* __restrict__ out_count) {
    __shared__ double s_raw[kWindow && kWinDoubles > kInDoubles ? kWinDoubles : kInDoubles];
    __shared__ int s_box[4][4];
    const uint32_t l = threadIdx.x, lx = l & 15u, ly = l >> 4;
    const uint32_t tx0 = blockIdx.x * kTile, ty0 = blockIdx.y * kTile;
    const uint32_t cols = min((uint32_t)kTile, P.width - tx0), rows = min((uint32_t)kTile, P.height - ty0);
    const bool active = lx < cols && ly < rows;
    const uint64_t n = (uint64_t)P.width * P.height, first = (uint64_t)ty0 * P.width + tx0;
    const uint64_t pix = first + (uint64_t)ly * P.width + lx;  // in the image when the lane is active

    // ---- 1. inputs ----
    const uint32_t cnt = !active ? 0u : count ? count[pix] : P.spp;
    double* s_mean = s_raw;
    double* s_sq = s_mean + kThreads * 3;
    double* s_ray = s_sq + kThreads * 3;
    double* s_hit = s_ray + kThreads * 7;
    stage_rows<3>(s_mean, mean, n * 3, first, P.width, cols, rows);
    stage_rows<3>(s_sq, sq, n * 3, first, P.width, cols, rows);
    stage_rows<6>(s_ray, rays, n * 6, first, P.width, cols, rows);
    stage_rows<8>(s_hit, hits, n * 8, first, P.width, cols, rows);
    __syncthreads();
    double cur[6];  // mean r g b, sq r g b; a lane that is not active reads what nobody staged and uses none of it
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        cur[c] = s_mean[3 * l + c];
        cur[3 + c] = s_sq[3 * l + c];
    }
    // rt_hit as 8 doubles: t, geometry_normal, shading_normal, {inside, prim}
    const double* h = s_hit + 9 * l;
    const double* r = s_ray + 7 * l;
    const double t = h[0];
    const V3 n_p = v3(h[4], h[5], h[6]);
    const bool hit = active && (int32_t)(__double_as_longlong(h[7]) >> 32) != RT_HIT_MISS;
    const V3 x_p = v3(r[0] + t * r[3], r[1] + t * r[4], r[2] + t * r[5]);
    const float nf[3] = {(float)n_p.x, (float)n_p.y, (float)n_p.z}, xf[3] = {(float)x_p.x, (float)x_p.y, (float)x_p.z};

    // ---- 2. reprojection and taps ----
    bool cand = false;
    int x0 = 0, y0 = 0;
    double ax = 0.0, ay = 0.0;
    if (P.has_prev && hit) {
        const V3 v = x_p - load3(P.pos);
        const double zc = dot(v, load3(P.fs)), xc = dot(v, load3(P.rs)), yc = dot(v, load3(P.us));
        const double gx = (((xc / zc) / P.tan_x + 1.0) * 0.5) * P.fw - 0.5;
        const double gy = (((-(yc / zc)) / P.tan_y + 1.0) * 0.5) * P.fh - 0.5;
        cand = zc > 0.0 && gx >= -1.0 && gx < P.fw && gy >= -1.0 && gy < P.fh;  // all false for a NaN
        if (cand) {
            const double fx = floor(gx), fy = floor(gy);
            x0 = (int)fx; y0 = (int)fy;
            ax = gx - fx; ay = gy - fy;
        }
    }
    Centre C;
    C.n = v3((double)nf[0], (double)nf[1], (double)nf[2]);
    C.x = v3((double)xf[0], (double)xf[1], (double)xf[2]);
    C.tol_t = P.plane_tol * (double)(float)t;
    C.normal_min = P.normal_min;
    Sums S;
    S.sw = 0.0;
    S.sm[0] = S.sm[1] = S.sm[2] = S.ss[0] = S.ss[1] = S.ss[2] = 0.0;
    S.n_min = 0xffffffffu;

    const int W = (int)P.width, H = (int)P.height;
    bool fits = false;
    int bx0 = INT_MAX, by0 = INT_MAX, bx1 = INT_MIN, by1 = INT_MIN;
    if (kWindow && P.has_prev) {  // the block's box of footprints
        if (cand) { bx0 = x0; by0 = y0; bx1 = x0 + 1; by1 = y0 + 1; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            bx0 = min(bx0, __shfl_xor(bx0, o)); by0 = min(by0, __shfl_xor(by0, o));
            bx1 = max(bx1, __shfl_xor(bx1, o)); by1 = max(by1, __shfl_xor(by1, o));
        }
        if ((l & 63u) == 0) {
            int* b = s_box[l >> 6];
            b[0] = bx0; b[1] = by0; b[2] = bx1; b[3] = by1;
        }
    }
    __syncthreads();  // the box is there, and every lane has taken its inputs out of s_raw
    if (kWindow && P.has_prev) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            bx0 = min(bx0, s_box[w][0]); by0 = min(by0, s_box[w][1]);
            bx1 = max(bx1, s_box[w][2]); by1 = max(by1, s_box[w][3]);
        }
        fits = bx0 <= bx1 && bx1 - bx0 < kSide && by1 - by0 < kSide;
    }

    if (kWindow && fits) {
        double (*s_c)[kSide][2][kHalf] = (double (*)[kSide][2][kHalf])s_raw;  // planes mr mg | mb sr | sg sb
        uint32_t (*s_g)[kSide][2][kHalf] =                                     // nx ny | nz px | py pz | count flags
            (uint32_t (*)[kSide][2][kHalf])(s_raw + 3 * kSide * 2 * kHalf);
        // the box clipped to the image: at least one record, since a footprint touches the image
        const int xs = max(bx0, 0), xe = min(bx1, W - 1), ys = max(by0, 0), ye = min(by1, H - 1);
        const uint32_t recs = (uint32_t)(xe - xs + 1), wrows = (uint32_t)(ye - ys + 1);
        for_words(2 * recs, wrows, [&](uint32_t row, uint32_t word) {
            const uint32_t half = word & 1u;
            const int x = xs + (int)(word >> 1), y = ys + (int)row;
            const uint4 a = guide_prev[((size_t)y * P.width + (size_t)x) * 2 + half];
            const int c = x - bx0, rr = y - by0;
            s_g[2 * half][rr][0][c] = a.x; s_g[2 * half][rr][1][c] = a.y;
            s_g[2 * half + 1][rr][0][c] = a.z; s_g[2 * half + 1][rr][1][c] = a.w;
        });
        for_words(3 * recs, wrows, [&](uint32_t row, uint32_t word) {
            const uint32_t rec = word / 3, part = word % 3;
            const int x = xs + (int)rec, y = ys + (int)row;
            const double2 a = colour_prev[((size_t)y * P.width + (size_t)x) * 3 + part];
            s_c[part][y - by0][0][x - bx0] = a.x; s_c[part][y - by0][1][x - bx0] = a.y;
        });
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int qx = x0 + i, qy = y0 + j;
                const bool inside = cand && qx >= 0 && qx < W && qy >= 0 && qy < H;
                const int c = inside ? qx - bx0 : 0, rr = inside ? qy - by0 : 0;
                // a tap outside the image reads a record of the window that may never have been staged:
                // whatever it holds is picked by no select
                const uint4 g0 = make_uint4(s_g[0][rr][0][c], s_g[0][rr][1][c], s_g[1][rr][0][c], s_g[1][rr][1][c]);
                const uint4 g1 = make_uint4(s_g[2][rr][0][c], s_g[2][rr][1][c], s_g[3][rr][0][c], s_g[3][rr][1][c]);
                const bool valid = inside && tap_valid(C, g0, g1);
                const double b = (i ? ax : 1.0 - ax) * (j ? ay : 1.0 - ay);
                tap_add(S, valid, b, make_double2(s_c[0][rr][0][c], s_c[0][rr][1][c]),
                        make_double2(s_c[1][rr][0][c], s_c[1][rr][1][c]), make_double2(s_c[2][rr][0][c], s_c[2][rr][1][c]),
                        g1.z);
            }
        }
    } else if (cand) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int qx = x0 + i, qy = y0 + j;
                if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                const size_t q = (size_t)qy * P.width + (size_t)qx;
                const uint4 g0 = guide_prev[2 * q], g1 = guide_prev[2 * q + 1];
                if (!tap_valid(C, g0, g1)) continue;
                const double b = (i ? ax : 1.0 - ax) * (j ? ay : 1.0 - ay);
                tap_add(S, true, b, colour_prev[3 * q], colour_prev[3 * q + 1], colour_prev[3 * q + 2], g1.z);
            }
        }
    }

    // ---- merge ----
    const uint32_t n_c = min(cnt, kMaxCount);
    const bool cur_ok = n_c >= 1u && finite(cur[0]) && finite(cur[1]) && finite(cur[2]) && finite(cur[3]) &&
                        finite(cur[4]) && finite(cur[5]);
    const bool hist_ok = S.sw > 0.0;
    const uint32_t n_h = min(S.n_min, P.max_history);
    double o[6];
    uint32_t oc = cur_ok ? n_c : 0u;
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = cur[k];
    if (hist_ok) {
        const uint32_t N = n_h + n_c;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double hk = (k < 3 ? S.sm[k] : S.ss[k - 3]) / S.sw;
            o[k] = cur_ok ? ((double)n_h * hk + (double)n_c * cur[k]) / (double)N : hk;
        }
        oc = cur_ok ? N : n_h;
    }
    const bool fin = finite(o[0]) && finite(o[1]) && finite(o[2]) && finite(o[3]) && finite(o[4]) && finite(o[5]);

    // ---- 3. outputs ----
    if (active) {
        uint4 a, b;
        a.x = __float_as_uint(nf[0]); a.y = __float_as_uint(nf[1]); a.z = __float_as_uint(nf[2]);
        a.w = __float_as_uint(xf[0]);
        b.x = __float_as_uint(xf[1]); b.y = __float_as_uint(xf[2]);
        b.z = fin ? oc : 0u;
        b.w = hit ? kHit : 0u;
        guide_next[2 * pix] = a;
        guide_next[2 * pix + 1] = b;
        colour_next[3 * pix] = make_double2(o[0], o[1]);
        colour_next[3 * pix + 1] = make_double2(o[2], o[3]);
        colour_next[3 * pix + 2] = make_double2(o[4], o[5]);
        out_count[pix] = oc;
    }
    __syncthreads();  // every lane is done with the window
    double* s_om = s_raw;
    double* s_os = s_raw + kThreads * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        s_om[3 * l + c] = o[c];
        s_os[3 * l + c] = o[3 + c];
    }
    __syncthreads();
    unstage_rows(s_om, out_mean, first, P.width, cols, rows);
    unstage_rows(s_os, out_sq, first, P.width, cols, rows);
}

}  // namespace

uint64_t temporal_guide_bytes(uint64_t n_pixels) { return (n_pixels * 32 + 255) / 256 * 256; }
uint64_t temporal_colour_bytes(uint64_t n_pixels) { return (n_pixels * 48 + 255) / 256 * 256; }

hipError_t launch_temporal(const TemporalSettings& S, const double* mean, const double* sq, const uint32_t* count,
                           const double* rays, const rt_hit* hits, const void* hist_prev, void* hist_next,
                           double* out_mean, double* out_sq, uint32_t* out_count, hipStream_t st) {
    const uint64_t n = (uint64_t)S.width * S.height, gb = temporal_guide_bytes(n);
    const uint4* gp = (const uint4*)hist_prev;
    const double2* cp = hist_prev ? (const double2*)((const char*)hist_prev + gb) : nullptr;
    uint4* gn = (uint4*)hist_next;
    double2* cn = (double2*)((char*)hist_next + gb);
    const dim3 grid((S.width + kTile - 1) / kTile, (S.height + kTile - 1) / kTile);
    const auto kernel = (S.flags & RT_TEMPORAL_NO_WINDOW) || !hist_prev ? tp_accumulate<false> : tp_accumulate<true>;
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, st, S, mean, sq, count, rays, (const double*)hits, gp, cp, gn, cn,
                       out_mean, out_sq, out_count);
    return hipGetLastError();
}

}  // namespace rt

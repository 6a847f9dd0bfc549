// bvh_build.hip — scene_build.cpp's Builder on the device, level by level.
//
// The host builder sorts each axis once and then, per node, runs a prefix and a
// suffix box sweep per axis, takes the first minimum of the SAH score and stably
// partitions the other two axis lists.  Here every open node of one tree level is
// a SEGMENT [lo, hi) of positions, the same range in all three axis lists, and a
// level is a handful of launches over all positions:
//   sweeps   ordered segmented scans of box_extend, forward and backward, per axis
//   choose   first minimum of (score, axis, position) per segment: an atomic min of
//            the score's integer key, then an atomic min of (axis, position) among
//            the positions that hold that score
//   split    flags by primitive id from the best axis, a prefix count of the flags
//            per axis list, a stable scatter into the ping-pong lists
// The scan operator is box_extend itself (rt_math.h rmin/rmax, earlier element on
// the left).  Without NaN it is associative — it returns the LAST of the smallest
// (largest) elements, zero signs included — so an ordered scan gives the host's
// sequential fold bit for bit (DESIGN.md §2 "device builder").  Nodes are created
// in level order and renumbered into the host's pre-order at the end.
#include <hip/hip_runtime.h>

#include <cstring>
#include <utility>
#include <vector>

#include "bvh_device.h"
#include "scene_build.h"

namespace rt {
namespace {

constexpr uint32_t kThreads = 256;                   // every kernel's block: four wave64s
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kSortTile = kThreads * 16;        // keys per block of a radix pass
constexpr uint32_t kTile = kThreads * 4;             // positions per block of a scan
constexpr uint32_t kNone = 0xffffffffu;              // seg_of: position in a finished leaf; nleft: a leaf
constexpr unsigned long long kNoKey = ~0ull;
constexpr uint64_t kMaxPrims = 1ull << 30;           // positions and 3n-sized grids stay in 32 bits

struct B6 { double v[6]; };  // Box3 as min xyz, max xyz
struct Lists { const double* p[3]; };

// box_extend(l, r): l is the fold so far, r the next element
__device__ __forceinline__ B6 ext(const B6& l, const B6& r) {
    B6 o;
    for (int k = 0; k < 3; ++k) o.v[k] = rmin(l.v[k], r.v[k]);
    for (int k = 3; k < 6; ++k) o.v[k] = rmax(l.v[k], r.v[k]);
    return o;
}
__device__ __forceinline__ double score6(const B6& b) {  // scene_build.cpp score()
    const double x = b.v[3] - b.v[0], y = b.v[4] - b.v[1], z = b.v[5] - b.v[2];
    return x * y + x * z + y * z;
}
// f64::total_cmp as an unsigned key (scene_build.cpp total_key with the sign bit flipped)
__device__ __forceinline__ unsigned long long ukey(double x) {
    long long b = __double_as_longlong(x);
    b ^= (long long)(((unsigned long long)(b >> 63)) >> 1);
    return (unsigned long long)b ^ 0x8000000000000000ull;
}
// a score's key: x + 0.0 turns -0 into +0, so key order is exactly the order of `<`
__device__ __forceinline__ unsigned long long score_key(double x) { return ukey(x + 0.0); }

// ------------------------------------------------------------ presort ----
// Midpoint keys of the three axes, the identity permutation, and the eligibility
// test: every coordinate finite and |v| <= 2^480 (build_bvh_device).
__global__ void bb_keys(const double* boxes, uint32_t n, unsigned long long* keys, uint32_t* ids, uint32_t* bad) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const double* b = boxes + (size_t)i * 6;
    bool ok = true;
    for (int k = 0; k < 6; ++k) ok = ok && fabs(b[k]) <= 0x1p480;  // false for NaN and inf
    if (!ok) atomicOr(bad, 1u);
    for (int a = 0; a < 3; ++a) {
        keys[(size_t)a * n + i] = ukey((b[a] + b[a + 3]) / 2.0);
        ids[(size_t)a * n + i] = i;
    }
}

// One 8-bit pass of the stable LSD radix sort, axis in blockIdx.y.
// table[axis][digit][block]: the block's count of each digit, then (bb_sort_scan)
// the global position of the block's first key with that digit.
__global__ void bb_sort_hist(const unsigned long long* keys, uint32_t n, uint32_t shift, uint32_t* table) {
    __shared__ uint32_t h[256];
    const uint32_t a = blockIdx.y, tid = threadIdx.x;
    h[tid] = 0;
    __syncthreads();
    for (uint32_t r = 0; r < kSortTile / kThreads; ++r) {
        const uint32_t i = blockIdx.x * kSortTile + r * kThreads + tid;
        if (i < n) atomicAdd(&h[(keys[(size_t)a * n + i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    table[((size_t)a * 256 + tid) * gridDim.x + blockIdx.x] = h[tid];
}

// Exclusive scan of one axis' table in (digit, block) order: 16 waves, a wave per digit row.
__global__ void bb_sort_scan(uint32_t* table, uint32_t nblk) {
    __shared__ uint32_t tot[256];
    uint32_t* t = table + (size_t)blockIdx.x * 256 * nblk;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (uint32_t d = w; d < 256; d += nw) {
        uint32_t sum = 0;
        for (uint32_t j = lane; j < nblk; j += 64) sum += t[(size_t)d * nblk + j];
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if (lane == 0) tot[d] = sum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int d = 0; d < 256; ++d) { const uint32_t x = tot[d]; tot[d] = run; run += x; }
    }
    __syncthreads();
    for (uint32_t d = w; d < 256; d += nw) {
        uint32_t carry = tot[d];
        for (uint32_t j0 = 0; j0 < nblk; j0 += 64) {
            const uint32_t j = j0 + lane;
            const uint32_t v = j < nblk ? t[(size_t)d * nblk + j] : 0u;
            uint32_t x = v;
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t y = __shfl_up(x, o);
                if (lane >= (uint32_t)o) x += y;
            }
            if (j < nblk) t[(size_t)d * nblk + j] = carry + x - v;
            carry += __shfl(x, 63);
        }
    }
}

// Stable scatter: keys of one digit keep their order — earlier rounds first, then
// waves in order (their counts scanned through LDS), then lanes (rank by ballot).
__global__ void bb_sort_scatter(const unsigned long long* kin, const uint32_t* iin, unsigned long long* kout,
                                uint32_t* iout, uint32_t n, uint32_t shift, const uint32_t* table) {
    __shared__ uint32_t base[256];
    __shared__ uint32_t cnt[kWaves][256];
    const uint32_t a = blockIdx.y, tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    base[tid] = table[((size_t)a * 256 + tid) * gridDim.x + blockIdx.x];  // read and written by thread tid only
    for (uint32_t r = 0; r < kSortTile / kThreads; ++r) {
        for (uint32_t k = 0; k < kWaves; ++k) cnt[k][tid] = 0;
        __syncthreads();
        const uint32_t i = blockIdx.x * kSortTile + r * kThreads + tid;
        const bool valid = i < n;
        const unsigned long long key = valid ? kin[(size_t)a * n + i] : 0ull;
        const uint32_t d = (uint32_t)(key >> shift) & 255u;
        unsigned long long same = __ballot(valid);  // the lanes that hold this lane's digit
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bal = __ballot(bit);
            same &= bit ? bal : ~bal;
        }
        const uint32_t rank = __popcll(same & ((1ull << lane) - 1ull));
        if (valid && rank == 0) cnt[w][d] = __popcll(same);
        __syncthreads();
        uint32_t run = base[tid];  // thread tid owns digit tid: where each wave's keys of it start
        for (uint32_t k = 0; k < kWaves; ++k) { const uint32_t c = cnt[k][tid]; cnt[k][tid] = run; run += c; }
        base[tid] = run;
        __syncthreads();
        if (valid) {
            const uint32_t pos = cnt[w][d] + rank;
            kout[(size_t)a * n + pos] = key;
            iout[(size_t)a * n + pos] = iin[(size_t)a * n + i];
        }
        __syncthreads();
    }
}

// SB[a][p] = boxes[S[a][p]]; the root segment, and every position in it.
__global__ void bb_gather(const double* boxes, const uint32_t* ids, double* sb, uint32_t n, uint32_t* seg_of) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x, a = blockIdx.y;
    if (p >= n) return;
    const double* s = boxes + (size_t)ids[(size_t)a * n + p] * 6;
    double* d = sb + ((size_t)a * n + p) * 6;
    for (int k = 0; k < 6; ++k) d[k] = s[k];
    if (a == 0) seg_of[p] = 0;
}

// ------------------------------------------------------------- levels ----
struct Segs {  // the open segments of one level
    uint32_t *lo, *hi, *node;          // positions [lo, hi); the node (creation id) they become
    int32_t* paxis;                    // the parent's split axis (-1: the root)
    unsigned long long *best, *pick;   // min score key; min (axis << 32 | position) holding it
};
struct Split {  // what bb_decide found, per segment of the level
    int32_t *axis, *leaf_axis;         // split axis or -1; a leaf's order (axis list, -1: list order)
    uint32_t *mid, *child;             // first right position; the left child's segment (right: + 1)
};
struct Nodes {  // by creation id: level order, a level's nodes contiguous
    double* box;
    uint32_t *left, *lo, *hi, *size, *pre;  // left child id (right: + 1) or kNone
};

__global__ void bb_root(Segs s, uint32_t n, uint32_t* ctr) {
    s.lo[0] = 0; s.hi[0] = n; s.node[0] = 0; s.paxis[0] = -1;
    s.best[0] = kNoKey; s.pick[0] = kNoKey;
    ctr[0] = 0; ctr[1] = 1;  // segments of the next level, nodes
}
__global__ void bb_next_level(uint32_t* ctr) { ctr[0] = 0; }

// One round of the ordered segmented scan over 256 consecutive scan positions.
// v, head: this thread's element and whether a segment starts at it.  *s_carry: the
// fold of the open segment before the round (then: before the next round).  Returns
// the fold from the segment's start to this thread's element.
__device__ __forceinline__ B6 scan_round(B6 v, bool head, B6* s_agg, uint32_t* s_flag, B6* s_carry) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    bool f = head;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        B6 o;
        for (int k = 0; k < 6; ++k) o.v[k] = __shfl_up(v.v[k], d);
        const int of = __shfl_up((int)f, d);
        if (lane >= d) {
            if (!f) v = ext(o, v);
            f = f || of;
        }
    }
    if (lane == 63) { s_agg[w] = v; s_flag[w] = f; }
    __syncthreads();
    B6 c = *s_carry;
    for (uint32_t j = 0; j < w; ++j) c = s_flag[j] ? s_agg[j] : ext(c, s_agg[j]);
    const B6 r = f ? v : ext(c, v);
    __syncthreads();
    if (threadIdx.x == kThreads - 1) *s_carry = r;
    return r;  // the next round reads *s_carry after its own first barrier
}

// Scan position q of direction dir (0 forward, 1 backward) is list position p.
__device__ __forceinline__ void scan_load(const double* src, uint32_t n, uint32_t q, int dir, const uint32_t* seg_of,
                                          const Segs& sg, uint32_t& p, uint32_t& s, B6& v, bool& head) {
    for (int k = 0; k < 6; ++k) v.v[k] = 0.0;
    head = true;
    s = kNone;
    p = 0;
    if (q >= n) return;
    p = dir ? n - 1 - q : q;
    s = seg_of[p];
    if (s == kNone) return;  // a finished leaf: a segment of its own, never read
    head = dir ? p + 1 == sg.hi[s] : p == sg.lo[s];
    const double* b = src + (size_t)p * 6;
    for (int k = 0; k < 6; ++k) v.v[k] = b[k];
}

// Pass 1 of a scan: each block's aggregate (the fold of its last open segment, and
// whether a segment starts in the block).  grid (blocks, lists, directions).
__global__ void bb_scan_reduce(Lists src, uint32_t n, const uint32_t* seg_of, Segs sg, B6* agg, uint32_t* aggf) {
    __shared__ B6 s_agg[kWaves], s_carry;
    __shared__ uint32_t s_flag[kWaves], s_any;
    const uint32_t a = blockIdx.y, dir = blockIdx.z;
    if (threadIdx.x == 0) { s_any = 0; for (int k = 0; k < 6; ++k) s_carry.v[k] = 0.0; }
    __syncthreads();
    for (uint32_t r = 0; r < kTile / kThreads; ++r) {
        uint32_t p, s; B6 v; bool head;
        scan_load(src.p[a], n, blockIdx.x * kTile + r * kThreads + threadIdx.x, dir, seg_of, sg, p, s, v, head);
        if (head) s_any = 1;
        // nothing is carried in here, so the block's first element starts the fold
        scan_round(v, head || (r == 0 && threadIdx.x == 0), s_agg, s_flag, &s_carry);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const size_t o = ((size_t)dir * gridDim.y + a) * gridDim.x + blockIdx.x;
        agg[o] = s_carry;
        aggf[o] = s_any;
    }
}

// Pass 2: the same scan over the block aggregates, in place, one block per (list,
// direction): agg[b] becomes the fold that block b + 1 starts from.
__global__ void bb_scan_blocks(B6* agg, const uint32_t* aggf, uint32_t nblk) {
    __shared__ B6 s_agg[kWaves], s_carry;
    __shared__ uint32_t s_flag[kWaves];
    const size_t base = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * nblk;
    if (threadIdx.x == 0) for (int k = 0; k < 6; ++k) s_carry.v[k] = 0.0;
    __syncthreads();
    for (uint32_t j0 = 0; j0 < nblk; j0 += kThreads) {
        const uint32_t j = j0 + threadIdx.x;
        B6 v;
        for (int k = 0; k < 6; ++k) v.v[k] = 0.0;
        bool head = true;
        if (j < nblk) { v = agg[base + j]; head = aggf[base + j] != 0; }
        const B6 r = scan_round(v, head, s_agg, s_flag, &s_carry);
        if (j < nblk) agg[base + j] = r;
    }
}

enum { kModeSuffix = 0, kModeSweep = 1, kModeRootBox = 2 };

// Pass 3: the scan itself, from the carried aggregates.  grid (blocks, lists).
//   kModeSuffix   backward: bscore[a][p] = score of the fold of positions hi-1 .. p
//   kModeSweep    forward: the split score at every position (scene_build.cpp:170), its
//                 key kept in keybuf and min-reduced into the segment; the node's box from
//                 the segment's last position on the parent's axis
//   kModeRootBox  forward over the list-order boxes: the root's box
__global__ void bb_scan_final(Lists src, uint32_t n, const uint32_t* seg_of, Segs sg, const B6* agg, int mode,
                              double* bscore, unsigned long long* keybuf, double* nbox) {
    __shared__ B6 s_agg[kWaves], s_carry;
    __shared__ uint32_t s_flag[kWaves];
    const uint32_t a = blockIdx.y, dir = mode == kModeSuffix ? 1u : 0u;
    if (threadIdx.x == 0) {
        for (int k = 0; k < 6; ++k) s_carry.v[k] = 0.0;
        if (blockIdx.x > 0) s_carry = agg[((size_t)dir * gridDim.y + a) * gridDim.x + blockIdx.x - 1];
    }
    __syncthreads();
    for (uint32_t r = 0; r < kTile / kThreads; ++r) {
        const uint32_t q = blockIdx.x * kTile + r * kThreads + threadIdx.x;
        uint32_t p, s; B6 v; bool head;
        scan_load(src.p[a], n, q, dir, seg_of, sg, p, s, v, head);
        const B6 f = scan_round(v, head, s_agg, s_flag, &s_carry);
        if (mode == kModeSuffix) {
            if (s != kNone) bscore[(size_t)a * n + p] = score6(f);
            continue;
        }
        uint32_t lo = 0, hi = 0;
        if (s != kNone) { lo = sg.lo[s]; hi = sg.hi[s]; }
        if (s != kNone && p + 1 == hi && (mode == kModeRootBox || sg.paxis[s] == (int32_t)a)) {
            double* b = nbox + (size_t)sg.node[s] * 6;
            for (int k = 0; k < 6; ++k) b[k] = f.v[k];
        }
        if (mode == kModeRootBox) continue;
        const uint32_t cnt = hi - lo;
        const bool cand = s != kNone && cnt > 4 && p + 1 < hi;
        unsigned long long key = kNoKey;
        if (cand) {
            const uint32_t lc = p - lo + 1, rc = cnt - lc;
            key = score_key(score6(f) * (double)lc + bscore[(size_t)a * n + p + 1] * (double)rc);
        }
        if (q < n) keybuf[(size_t)a * n + p] = key;
        // min into the segment: one atomic per wave where the wave is inside one segment,
        // and none where the segment already holds a smaller key (it only ever decreases)
        const uint32_t s0 = __shfl(s, 0);
        if (__all(cand && s == s0)) {
            unsigned long long m = key;
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long y = __shfl_xor(m, o);
                m = y < m ? y : m;
            }
            if ((threadIdx.x & 63u) == 0 && m < *(volatile unsigned long long*)&sg.best[s]) atomicMin(&sg.best[s], m);
        } else if (cand && key < *(volatile unsigned long long*)&sg.best[s]) {
            atomicMin(&sg.best[s], key);
        }
    }
}

// The first position of the first axis that holds the segment's minimum score.
__global__ void bb_pick(uint32_t n, const uint32_t* seg_of, Segs sg, const unsigned long long* keybuf) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x, a = blockIdx.y;
    if (p >= n) return;
    const uint32_t s = seg_of[p];
    if (s == kNone) return;
    const uint32_t lo = sg.lo[s], hi = sg.hi[s];
    if (hi - lo <= 4 || p + 1 >= hi || keybuf[(size_t)a * n + p] != sg.best[s]) return;
    atomicMin(&sg.pick[s], ((unsigned long long)a << 32) | p);
}

// Per segment: leaf or split (scene_build.cpp:154, :174); a split opens two segments
// of the next level and creates their nodes.
__global__ void bb_decide(uint32_t nseg, Segs sg, Segs nx, Split sp, Nodes nd, uint32_t* ctr) {
    const uint32_t s = blockIdx.x * kThreads + threadIdx.x;
    if (s >= nseg) return;
    const uint32_t lo = sg.lo[s], hi = sg.hi[s], cnt = hi - lo, me = sg.node[s];
    nd.lo[me] = lo;
    nd.hi[me] = hi;
    int32_t axis = -1, leaf_axis = 2;  // SameNode: the last sort was axis 2
    uint32_t mid = 0;
    if (cnt <= 4) {
        leaf_axis = sg.paxis[s];
    } else {
        B6 b;
        for (int k = 0; k < 6; ++k) b.v[k] = nd.box[(size_t)me * 6 + k];
        if (sg.best[s] < score_key(score6(b) * (double)cnt)) {  // strict: a tie stays one node
            axis = (int32_t)(sg.pick[s] >> 32);
            mid = (uint32_t)sg.pick[s] + 1;
        }
    }
    sp.axis[s] = axis;
    sp.leaf_axis[s] = leaf_axis;
    nd.left[me] = kNone;
    if (axis < 0) return;
    const uint32_t c = atomicAdd(&ctr[0], 2u), kid = atomicAdd(&ctr[1], 2u);
    sp.mid[s] = mid;
    sp.child[s] = c;
    nd.left[me] = kid;
    for (uint32_t k = 0; k < 2; ++k) {
        nx.lo[c + k] = k ? mid : lo;
        nx.hi[c + k] = k ? hi : mid;
        nx.node[c + k] = kid + k;
        nx.paxis[c + k] = axis;
        nx.best[c + k] = kNoKey;
        nx.pick[c + k] = kNoKey;
    }
}

// left_flag by primitive id, from the best axis' list: every primitive of a split
// segment is written once, so nothing needs clearing.
__global__ void bb_mark(uint32_t n, const uint32_t* seg_of, Split sp, const uint32_t* ids, uint8_t* flag) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const uint32_t s = seg_of[p];
    if (s == kNone || sp.axis[s] < 0) return;
    flag[ids[(size_t)sp.axis[s] * n + p]] = p < sp.mid[s];
}

__device__ __forceinline__ bool goes_left(uint32_t n, uint32_t p, uint32_t a, const uint32_t* seg_of, const Split& sp,
                                          const uint32_t* ids, const uint8_t* flag) {
    if (p >= n) return false;
    const uint32_t s = seg_of[p];
    if (s == kNone || sp.axis[s] < 0) return false;
    return flag[ids[(size_t)a * n + p]] != 0;
}

// excl[a][p] = number of left-going positions before p in axis list a (a plain prefix
// count over the whole list; a segment's own count is a difference of two of them).
// Pass 1 (blkcnt == out): per-block counts.  Pass 3: the counts from the scanned blocks.
__global__ void bb_flag_scan(uint32_t n, const uint32_t* seg_of, Split sp, const uint32_t* ids, const uint8_t* flag,
                             uint32_t* blkcnt, uint32_t* excl) {
    __shared__ uint32_t s_w[kWaves];
    const uint32_t a = blockIdx.y, lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t run = excl ? blkcnt[(size_t)a * gridDim.x + blockIdx.x] : 0u;
    for (uint32_t r = 0; r < kTile / kThreads; ++r) {
        const uint32_t p = blockIdx.x * kTile + r * kThreads + threadIdx.x;
        const unsigned long long bal = __ballot(goes_left(n, p, a, seg_of, sp, ids, flag));
        if (lane == 0) s_w[w] = __popcll(bal);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t k = 0; k < kWaves; ++k) { if (k < w) before += s_w[k]; total += s_w[k]; }
        if (excl && p < n) excl[(size_t)a * n + p] = run + before + __popcll(bal & ((1ull << lane) - 1ull));
        run += total;
        __syncthreads();
    }
    if (!excl && threadIdx.x == 0) blkcnt[(size_t)a * gridDim.x + blockIdx.x] = run;
}
// Pass 2: exclusive scan of the per-block counts, one block per axis list.
__global__ void bb_count_scan(uint32_t* blkcnt, uint32_t nblk) {
    __shared__ uint32_t s_w[kWaves];
    uint32_t* t = blkcnt + (size_t)blockIdx.x * nblk;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t run = 0;
    for (uint32_t j0 = 0; j0 < nblk; j0 += kThreads) {
        const uint32_t j = j0 + threadIdx.x;
        const uint32_t v = j < nblk ? t[j] : 0u;
        uint32_t x = v;
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) s_w[w] = x;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t k = 0; k < kWaves; ++k) { if (k < w) before += s_w[k]; total += s_w[k]; }
        if (j < nblk) t[j] = run + before + x - v;
        run += total;
        __syncthreads();
    }
}

// The stable partition (scene_build.cpp:178-190) of every split segment into the
// ping-pong lists, the leaves' primitive order, and the next level's seg_of.
__global__ void bb_scatter(uint32_t n, const uint32_t* seg_of, Segs sg, Split sp, const uint8_t* flag,
                           const uint32_t* excl, const uint32_t* ids, const double* sb, uint32_t* ids2, double* sb2,
                           uint32_t* seg_of2, uint32_t* order) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x, a = blockIdx.y;
    if (p >= n) return;
    const uint32_t s = seg_of[p];
    const int32_t axis = s == kNone ? -1 : sp.axis[s];
    if (axis < 0) {
        if (a != 0) return;
        seg_of2[p] = kNone;
        if (s == kNone) return;
        const int32_t la = sp.leaf_axis[s];  // list order: only the root, which holds ids 0..n-1 at 0..n-1
        order[p] = la < 0 ? p : ids[(size_t)la * n + p];
        return;
    }
    const uint32_t lo = sg.lo[s], mid = sp.mid[s], id = ids[(size_t)a * n + p];
    uint32_t dst = p;
    if ((int32_t)a == axis) {
        seg_of2[p] = sp.child[s] + (p < mid ? 0u : 1u);
    } else {
        const uint32_t e = excl[(size_t)a * n + p] - excl[(size_t)a * n + lo];
        dst = flag[id] ? lo + e : mid + (p - lo) - e;
    }
    ids2[(size_t)a * n + dst] = id;
    const double* b = sb + ((size_t)a * n + p) * 6;
    double* d = sb2 + ((size_t)a * n + dst) * 6;
    for (int k = 0; k < 6; ++k) d[k] = b[k];
}

// ---------------------------------------------------------- numbering ----
// Subtree sizes, one level at a time from the deepest up.
__global__ void bb_sizes(uint32_t first, uint32_t end, Nodes nd) {
    const uint32_t i = first + blockIdx.x * kThreads + threadIdx.x;
    if (i >= end) return;
    const uint32_t l = nd.left[i];
    nd.size[i] = l == kNone ? 1u : 1u + nd.size[l] + nd.size[l + 1];
}
// Pre-order indices from the root down: left = parent + 1, right = parent + 1 + size(left).
__global__ void bb_preorder(uint32_t first, uint32_t end, Nodes nd) {
    const uint32_t i = first + blockIdx.x * kThreads + threadIdx.x;
    if (i >= end) return;
    if (i == 0) nd.pre[0] = 0;
    const uint32_t l = nd.left[i];
    if (l == kNone) return;
    nd.pre[l] = nd.pre[i] + 1;
    nd.pre[l + 1] = nd.pre[i] + 1 + nd.size[l];
}
__global__ void bb_emit(uint32_t n_nodes, Nodes nd, OutNode* out) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_nodes) return;
    OutNode o;
    for (int k = 0; k < 6; ++k) o.box[k] = nd.box[(size_t)i * 6 + k];
    const uint32_t l = nd.left[i];
    const bool leaf = l == kNone;
    o.left = leaf ? -1 : (int64_t)nd.pre[l];
    o.right = leaf ? -1 : (int64_t)nd.pre[l + 1];
    o.start = leaf ? nd.lo[i] : 0;  // the host's inner nodes carry no range
    o.end = leaf ? nd.hi[i] : 0;
    out[nd.pre[i]] = o;
}
__global__ void bb_order64(uint32_t n, const uint32_t* order, uint64_t* out) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) out[i] = order[i];
}

// ---------------------------------------------------------------- host ----
inline uint32_t blocks(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

Segs alloc_segs(Arena& m, size_t n) {
    Segs s;
    s.lo = m.get<uint32_t>(n); s.hi = m.get<uint32_t>(n); s.node = m.get<uint32_t>(n);
    s.paxis = m.get<int32_t>(n);
    s.best = m.get<unsigned long long>(n); s.pick = m.get<unsigned long long>(n);
    return s;
}

}  // namespace

#define BB_TRY(call)                                                         \
    do {                                                                     \
        const hipError_t e_ = (call);                                        \
        if (e_ != hipSuccess) { err = hipGetErrorString(e_); return kDeviceBuildError; } \
    } while (0)

int build_bvh_device_tree(Arena& m, const double* d_boxes, uint32_t n, uint32_t max_levels, DevTree& out,
                          std::string& err) {
    if (max_levels == 0) max_levels = kDeviceBuildMaxLevels;
    const size_t n3 = (size_t)n * 3;
    const size_t mark = m.ptrs.size();
    const hipStream_t st = 0;

    // keys, the presort
    uint32_t* d_ctr = m.get<uint32_t>(4);  // next-level segments, nodes, ineligible flag
    uint32_t* ids[2] = {m.get<uint32_t>(n3), m.get<uint32_t>(n3)};
    unsigned long long* keys[2] = {m.get<unsigned long long>(n3), m.get<unsigned long long>(n3)};
    const uint32_t sblk = blocks(n, kSortTile);
    uint32_t* d_table = m.get<uint32_t>((size_t)3 * 256 * sblk);
    if (!m.ok()) { if (m.oom) return kDeviceBuildFallback; BB_TRY(m.err); }
    BB_TRY(hipMemsetAsync(d_ctr, 0, 4 * sizeof(uint32_t), st));
    bb_keys<<<blocks(n, kThreads), kThreads, 0, st>>>(d_boxes, n, keys[0], ids[0], d_ctr + 2);
    uint32_t bad = 0;
    BB_TRY(hipMemcpyAsync(&bad, d_ctr + 2, sizeof(bad), hipMemcpyDeviceToHost, st));
    BB_TRY(hipStreamSynchronize(st));
    if (bad) return kDeviceBuildFallback;  // NaN, inf or a huge coordinate: the host builder's case
    for (uint32_t pass = 0; pass < 8; ++pass) {
        const uint32_t shift = pass * 8;
        bb_sort_hist<<<dim3(sblk, 3), kThreads, 0, st>>>(keys[0], n, shift, d_table);
        bb_sort_scan<<<3, 1024, 0, st>>>(d_table, sblk);
        bb_sort_scatter<<<dim3(sblk, 3), kThreads, 0, st>>>(keys[0], ids[0], keys[1], ids[1], n, shift, d_table);
        std::swap(keys[0], keys[1]);
        std::swap(ids[0], ids[1]);
    }
    BB_TRY(hipGetLastError());
    BB_TRY(hipStreamSynchronize(st));
    m.release(keys[0]); m.release(keys[1]); m.release(d_table);

    // the level loop's state
    double* sb[2] = {m.get<double>(n3 * 6), m.get<double>(n3 * 6)};
    uint32_t* seg_of[2] = {m.get<uint32_t>(n), m.get<uint32_t>(n)};
    Segs segs[2] = {alloc_segs(m, n), alloc_segs(m, n)};
    Split sp;
    sp.axis = m.get<int32_t>(n); sp.leaf_axis = m.get<int32_t>(n);
    sp.mid = m.get<uint32_t>(n); sp.child = m.get<uint32_t>(n);
    const size_t max_nodes = (size_t)2 * n;  // every split makes two non-empty children: <= 2n - 1 nodes
    Nodes nd;
    nd.box = m.get<double>(max_nodes * 6);
    nd.left = m.get<uint32_t>(max_nodes); nd.lo = m.get<uint32_t>(max_nodes); nd.hi = m.get<uint32_t>(max_nodes);
    nd.size = m.get<uint32_t>(max_nodes); nd.pre = m.get<uint32_t>(max_nodes);
    double* d_bscore = m.get<double>(n3);
    unsigned long long* d_keybuf = m.get<unsigned long long>(n3);
    uint32_t* d_excl = m.get<uint32_t>(n3);
    uint8_t* d_flag = m.get<uint8_t>(n);
    uint32_t* d_order = m.get<uint32_t>(n);
    const uint32_t nblk = blocks(n, kTile);
    B6* d_agg = m.get<B6>((size_t)6 * nblk);
    uint32_t* d_aggf = m.get<uint32_t>((size_t)6 * nblk);
    uint32_t* d_blkcnt = m.get<uint32_t>((size_t)3 * nblk);
    if (!m.ok()) { if (m.oom) return kDeviceBuildFallback; BB_TRY(m.err); }

    const dim3 per_pos(blocks(n, kThreads), 3);
    bb_gather<<<per_pos, kThreads, 0, st>>>(d_boxes, ids[0], sb[0], n, seg_of[0]);
    bb_root<<<1, 1, 0, st>>>(segs[0], n, d_ctr);
    std::vector<uint32_t> level_start{0, 1};  // creation ids of level L: [level_start[L-1], level_start[L])
    uint32_t nseg = 1, depth = 0;
    for (uint32_t level = 1; nseg > 0; ++level) {
        if (level > max_levels) return kDeviceBuildFallback;
        depth = level;
        const Lists ls{{sb[0], sb[0] + (size_t)n * 6, sb[0] + (size_t)n * 12}};
        bb_next_level<<<1, 1, 0, st>>>(d_ctr);
        if (level == 1) {  // the root's box folds the boxes in list order
            const Lists lb{{d_boxes, d_boxes, d_boxes}};
            bb_scan_reduce<<<dim3(nblk, 1, 1), kThreads, 0, st>>>(lb, n, seg_of[0], segs[0], d_agg, d_aggf);
            bb_scan_blocks<<<dim3(1, 1, 1), kThreads, 0, st>>>(d_agg, d_aggf, nblk);
            bb_scan_final<<<dim3(nblk, 1), kThreads, 0, st>>>(lb, n, seg_of[0], segs[0], d_agg, kModeRootBox,
                                                               d_bscore, d_keybuf, nd.box);
        }
        bb_scan_reduce<<<dim3(nblk, 3, 2), kThreads, 0, st>>>(ls, n, seg_of[0], segs[0], d_agg, d_aggf);
        bb_scan_blocks<<<dim3(1, 3, 2), kThreads, 0, st>>>(d_agg, d_aggf, nblk);
        bb_scan_final<<<dim3(nblk, 3), kThreads, 0, st>>>(ls, n, seg_of[0], segs[0], d_agg, kModeSuffix, d_bscore,
                                                           d_keybuf, nd.box);
        bb_scan_final<<<dim3(nblk, 3), kThreads, 0, st>>>(ls, n, seg_of[0], segs[0], d_agg, kModeSweep, d_bscore,
                                                           d_keybuf, nd.box);
        bb_pick<<<per_pos, kThreads, 0, st>>>(n, seg_of[0], segs[0], d_keybuf);
        bb_decide<<<blocks(nseg, kThreads), kThreads, 0, st>>>(nseg, segs[0], segs[1], sp, nd, d_ctr);
        bb_mark<<<blocks(n, kThreads), kThreads, 0, st>>>(n, seg_of[0], sp, ids[0], d_flag);
        bb_flag_scan<<<dim3(nblk, 3), kThreads, 0, st>>>(n, seg_of[0], sp, ids[0], d_flag, d_blkcnt, nullptr);
        bb_count_scan<<<3, kThreads, 0, st>>>(d_blkcnt, nblk);
        bb_flag_scan<<<dim3(nblk, 3), kThreads, 0, st>>>(n, seg_of[0], sp, ids[0], d_flag, d_blkcnt, d_excl);
        bb_scatter<<<per_pos, kThreads, 0, st>>>(n, seg_of[0], segs[0], sp, d_flag, d_excl, ids[0], sb[0], ids[1],
                                                 sb[1], seg_of[1], d_order);
        BB_TRY(hipGetLastError());
        uint32_t ctr[2];
        BB_TRY(hipMemcpyAsync(ctr, d_ctr, sizeof(ctr), hipMemcpyDeviceToHost, st));
        BB_TRY(hipStreamSynchronize(st));
        nseg = ctr[0];
        if (nseg) level_start.push_back(ctr[1]);
        std::swap(ids[0], ids[1]);
        std::swap(sb[0], sb[1]);
        std::swap(seg_of[0], seg_of[1]);
        std::swap(segs[0], segs[1]);
    }
    const uint32_t n_nodes = level_start.back();

    // numbering: sizes bottom-up, pre-order top-down, then the host's records
    m.release(sb[0]); m.release(sb[1]);
    OutNode* d_out = m.get<OutNode>(n_nodes);
    if (!m.ok()) { if (m.oom) return kDeviceBuildFallback; BB_TRY(m.err); }
    for (size_t l = level_start.size() - 1; l-- > 0;)
        bb_sizes<<<blocks(level_start[l + 1] - level_start[l], kThreads), kThreads, 0, st>>>(level_start[l],
                                                                                             level_start[l + 1], nd);
    for (size_t l = 0; l + 1 < level_start.size(); ++l)
        bb_preorder<<<blocks(level_start[l + 1] - level_start[l], kThreads), kThreads, 0, st>>>(level_start[l],
                                                                                                level_start[l + 1], nd);
    bb_emit<<<blocks(n_nodes, kThreads), kThreads, 0, st>>>(n_nodes, nd, d_out);
    BB_TRY(hipGetLastError());
    BB_TRY(hipStreamSynchronize(st));
    m.release_since(mark, d_out, d_order);
    out.nodes = d_out;
    out.order = d_order;
    out.n_nodes = n_nodes;
    out.depth = depth;
    return kDeviceBuildDone;
}

int build_bvh_device(const std::vector<Box3>& boxes, uint32_t max_levels, HostBvh& out, std::string& err) {
    const uint64_t n64 = boxes.size();
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        err = "no HIP device visible (the device builder needs one)";
        return kDeviceBuildError;
    }
    if (n64 == 0 || n64 > kMaxPrims) return kDeviceBuildFallback;
    const uint32_t n = (uint32_t)n64;
    Arena m;
    const hipStream_t st = 0;
    double* d_boxes = m.get<double>((size_t)n * 6);
    if (!m.ok()) { if (m.oom) return kDeviceBuildFallback; BB_TRY(m.err); }
    static_assert(sizeof(Box3) == 48, "Box3 is six doubles");
    BB_TRY(hipMemcpyAsync(d_boxes, boxes.data(), (size_t)n * 48, hipMemcpyHostToDevice, st));
    DevTree t;
    const int made = build_bvh_device_tree(m, d_boxes, n, max_levels, t, err);
    if (made != kDeviceBuildDone) return made;
    uint64_t* d_order64 = m.get<uint64_t>(n);
    if (!m.ok()) { if (m.oom) return kDeviceBuildFallback; BB_TRY(m.err); }
    bb_order64<<<blocks(n, kThreads), kThreads, 0, st>>>(n, t.order, d_order64);
    BB_TRY(hipGetLastError());
    out.nodes.resize(t.n_nodes);
    out.order.resize(n);
    out.depth = t.depth;
    BB_TRY(hipMemcpyAsync(out.nodes.data(), t.nodes, (size_t)t.n_nodes * sizeof(OutNode), hipMemcpyDeviceToHost, st));
    BB_TRY(hipMemcpyAsync(out.order.data(), d_order64, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    BB_TRY(hipStreamSynchronize(st));
    return kDeviceBuildDone;
}

}  // namespace rt

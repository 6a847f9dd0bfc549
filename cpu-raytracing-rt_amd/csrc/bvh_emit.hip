// bvh_emit.hip — a triangle BVH's device records written on the device.
//
// bvh_build.hip leaves the tree in device memory (pre-order OutNodes, the u32 leaf order).
// The kernels here turn it, and the scene's triangles uploaded once in list order, into
// the nine arrays of a triangle DevBvh, byte for byte what scene_build.cpp's flatten,
// build_compact, build_pairs and build_tri_bvh's gather loop make on the host, written
// straight into the allocations the scene will own (DESIGN.md §2 "Device record emission"):
//   be_boxes        the builder's input boxes out of the uploaded items
//   be_node_flags   fast, f32-exactness and the pair layout's union check over the nodes
//   be_item_flags   f32-exactness and tri_q over the items
//   be_scan_*       leaf-block index and compact slot of every node: three exclusive scans
//                   in pre-order (block lines, inner nodes; then unpackable leaves, which
//                   need the block index), each as reduce / scan of the block sums / final
//   be_nodes        DevNode, 8 lanes per 128-B record
//   be_cnodes       DevNodeC, 4 lanes per 64-B record
//   be_pairs        pair lines, 8 lanes per 128-B line
//   be_leaves       leaf blocks, 8 lanes per 128-B line; a leaf above kGroupLeaf triangles
//                   is queued and written by whole blocks in be_big_leaves
//   be_gather       tris, tri_cold, tri_inv_area, mat, gid: 64 items per block through LDS
// Every record leaves as 16-byte lane stores that cover whole lines.  Nothing here waits on
// another block.  The only arithmetic is f64 -> f32 of values proven exact, and fmin / fmax.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstring>

#include "bvh_device.h"
#include "scene_build.h"

namespace rt {
namespace {

constexpr uint32_t kThreads = 256;                 // every kernel's block: four wave64s
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kTile = kThreads * 4;           // nodes per block of a scan
constexpr uint32_t kNone = 0xffffffffu;            // slot: a packed leaf has none
constexpr uint64_t kMaxPrims = 1ull << 30;         // as the builder's
constexpr uint32_t kGroupLeaf = 16;                // triangles: a larger leaf is written by whole blocks
constexpr uint32_t kBigGrid = 256;                 // blocks of be_big_leaves
constexpr uint32_t kGatherTris = 64;               // items per block of be_gather
typedef unsigned long long u64;

// TriItem as 36 eight-byte words
constexpr uint32_t kItemWords = sizeof(TriItem) / 8;
constexpr uint32_t kWA = offsetof(TriItem, t.a) / 8, kWNg = offsetof(TriItem, t.ng) / 8,
                   kWInvArea = offsetof(TriItem, t.inv_area) / 8, kWNa = offsetof(TriItem, t.na) / 8,
                   kWB = offsetof(TriItem, b) / 8, kWC = offsetof(TriItem, c) / 8,
                   kWMatGid = offsetof(TriItem, mat) / 8, kWBox = offsetof(TriItem, box) / 8;
static_assert(kWA == 0 && offsetof(TriItem, t.ba) == 24 && offsetof(TriItem, t.ca) == 48 && kWNg == 9 &&
              kWInvArea == 12 && kWNa == 13 && offsetof(TriItem, t.nc) == 152 && kWB == 22 && kWC == 25 &&
              offsetof(TriItem, mat) == 224 && offsetof(TriItem, gid) == 228 && kWBox == 29 && kItemWords == 36,
              "TriItem's words as the kernels index them");
static_assert(sizeof(DevTri) == 80 && sizeof(DevTriCold) == 96 && sizeof(DevNode) == 128 && sizeof(DevNodeC) == 64 &&
              kPairFloats == 32 && kLeafBlock == 32, "record sizes in 16-byte parts");

// flags: a bit stays set while every element passes
constexpr uint32_t kFlagFast = 1u, kFlagExact = 2u, kFlagTriQ = 4u, kFlagUnion = 8u, kFlagsAll = 15u;
struct Header {
    u64 n_lines;        // leaf-block lines (n_floats / kLeafBlock)
    uint32_t n_int;     // inner nodes
    uint32_t n_big;     // leaves a child word cannot pack
    uint32_t flags;
    uint32_t n_queued;  // leaves waiting for be_big_leaves
};
struct ScanV { u64 a; uint32_t b; uint32_t pad; };  // two sums scanned together

__device__ __forceinline__ bool is_leaf(const OutNode& n) { return n.left < 0; }
__device__ __forceinline__ uint32_t prims(const OutNode& n) { return (uint32_t)(n.end - n.start); }
__device__ __forceinline__ u64 leaf_lines(uint32_t count) {  // build_compact: 1 header word + kTriC per triangle
    return (1ull + (u64)kTriC * count + kLeafBlock - 1) / kLeafBlock;
}
__device__ __forceinline__ bool packs(uint32_t count, uint32_t block) { return count < 128u && block < (1u << 24); }
__device__ __forceinline__ uint32_t f32_bits(double v) { return __float_as_uint((float)v); }
__device__ __forceinline__ void store16(void* dst, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    *(uint4*)dst = make_uint4(a, b, c, d);
}

// AND of `ok` over the grid into *flags: ballots per wave, LDS per block, one atomic per block.
__device__ __forceinline__ void and_reduce(uint32_t ok, uint32_t* flags) {
    __shared__ uint32_t s_and;
    if (threadIdx.x == 0) s_and = kFlagsAll;
    __syncthreads();
    uint32_t wave = 0;
    for (uint32_t b = 1; b <= kFlagUnion; b <<= 1)
        if (__ballot((ok & b) != 0) == ~0ull) wave |= b;
    if ((threadIdx.x & 63u) == 0 && wave != kFlagsAll) atomicAnd(&s_and, wave);
    __syncthreads();
    if (threadIdx.x == 0 && s_and != kFlagsAll) atomicAnd(flags, s_and);
}

__global__ void be_init(Header* h) {
    h->n_lines = 0; h->n_int = 0; h->n_big = 0; h->flags = kFlagsAll; h->n_queued = 0;
}

// boxes[i] = items[i].box, a lane per double
__global__ void be_boxes(const u64* items, uint32_t n, u64* boxes) {
    const u64 g = (u64)blockIdx.x * kThreads + threadIdx.x;
    if (g >= (u64)n * 6) return;
    boxes[g] = items[(g / 6) * kItemWords + kWBox + g % 6];
}

__global__ void be_node_flags(const OutNode* nodes, uint32_t n_nodes, uint32_t* flags) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    uint32_t ok = kFlagsAll;
    if (i < n_nodes) {
        const OutNode n = nodes[i];
        bool fast = true, exact = true;
        for (int k = 0; k < 6; ++k) {
            fast = fast && coord_fast(n.box[k]);
            exact = exact && f32_exact(n.box[k]) && n.box[k] == n.box[k];
        }
        for (int k = 0; k < 3; ++k) fast = fast && n.box[k] <= n.box[k + 3];  // flatten: min <= max
        // build_pairs: an inner child's box is the union of its children's (as f32; the root is no child)
        bool uni = true;
        if (i > 0 && !is_leaf(n)) {
            const OutNode l = nodes[n.left], r = nodes[n.right];
            for (int k = 0; k < 3; ++k)
                uni = uni && !(fminf((float)l.box[k], (float)r.box[k]) != (float)n.box[k] ||
                               fmaxf((float)l.box[k + 3], (float)r.box[k + 3]) != (float)n.box[k + 3]);
        }
        ok = (fast ? kFlagFast : 0u) | (exact ? kFlagExact : 0u) | kFlagTriQ | (uni ? kFlagUnion : 0u);
    }
    and_reduce(ok, flags);
}

__global__ void be_item_flags(const double* items, uint32_t n, uint32_t* flags) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    uint32_t ok = kFlagsAll;
    if (i < n) {
        const double* it = items + (size_t)i * kItemWords;
        bool exact = true, q = true;
        for (uint32_t k = 0; k < 3; ++k) {
            const double a = it[kWA + k], b = it[kWB + k], c = it[kWC + k];
            exact = exact && f32_exact(a) && a == a && f32_exact(b) && b == b && f32_exact(c) && c == c;
        }
        for (uint32_t k = 3; k < 9; ++k) q = q && edge_ok(it[k]);  // ba, ca
        ok = kFlagFast | (exact ? kFlagExact : 0u) | (q ? kFlagTriQ : 0u) | kFlagUnion;
    }
    and_reduce(ok, flags);
}

// ---------------------------------------------------------------- scans ----
// Round 0: a = the leaf's block lines, b = 1 for an inner node.  Round 1: b = 1 for a leaf
// that does not pack (it needs round 0's block index).
__device__ __forceinline__ ScanV scan_value(const OutNode* nodes, uint32_t n_nodes, uint32_t i, int round,
                                            const uint32_t* blk) {
    ScanV v{0, 0, 0};
    if (i >= n_nodes) return v;
    const OutNode& n = nodes[i];
    const bool leaf = n.left < 0;
    const uint32_t cnt = (uint32_t)(n.end - n.start);
    if (round == 0) {
        v.a = leaf ? leaf_lines(cnt) : 0;
        v.b = leaf ? 0u : 1u;
    } else {
        v.b = leaf && !packs(cnt, blk[i]) ? 1u : 0u;
    }
    return v;
}
// Exclusive scan of one value per thread over the block; `run` carries the block's
// running sum from round to round (every thread holds the same copy).
__device__ __forceinline__ ScanV block_scan(ScanV v, ScanV& run, ScanV* s_w) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    ScanV x = v;
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const u64 ya = __shfl_up(x.a, o);
        const uint32_t yb = __shfl_up(x.b, o);
        if (lane >= o) { x.a += ya; x.b += yb; }
    }
    if (lane == 63) s_w[w] = x;
    __syncthreads();
    ScanV before = run, total{0, 0, 0};
    for (uint32_t k = 0; k < kWaves; ++k) {
        if (k < w) { before.a += s_w[k].a; before.b += s_w[k].b; }
        total.a += s_w[k].a; total.b += s_w[k].b;
    }
    __syncthreads();
    run.a += total.a; run.b += total.b;
    return ScanV{before.a + x.a - v.a, before.b + x.b - v.b, 0};
}
__global__ void be_scan_reduce(const OutNode* nodes, uint32_t n_nodes, int round, const uint32_t* blk, ScanV* agg) {
    __shared__ ScanV s_w[kWaves];
    ScanV run{0, 0, 0};
    for (uint32_t r = 0; r < kTile / kThreads; ++r)
        block_scan(scan_value(nodes, n_nodes, blockIdx.x * kTile + r * kThreads + threadIdx.x, round, blk), run, s_w);
    if (threadIdx.x == 0) agg[blockIdx.x] = run;
}
// One block: agg[b] becomes the sum of the blocks before b; the totals go to the header.
__global__ void be_scan_blocks(ScanV* agg, uint32_t nblk, int round, Header* h) {
    __shared__ ScanV s_w[kWaves];
    ScanV run{0, 0, 0};
    for (uint32_t j0 = 0; j0 < nblk; j0 += kThreads) {
        const uint32_t j = j0 + threadIdx.x;
        ScanV v{0, 0, 0};
        if (j < nblk) v = agg[j];
        const ScanV e = block_scan(v, run, s_w);
        if (j < nblk) agg[j] = e;
    }
    if (threadIdx.x == 0) {
        if (round == 0) { h->n_lines = run.a; h->n_int = run.b; }
        else h->n_big = run.b;
    }
}
// Round 0 writes blk (saturated: a block index past 2^32 never packs, and the layout is
// dropped for it anyway) and the inner nodes' slots; round 1 the unpackable leaves' slots.
__global__ void be_scan_final(const OutNode* nodes, uint32_t n_nodes, int round, const ScanV* agg, uint32_t* blk,
                              uint32_t* slot, const Header* h) {
    __shared__ ScanV s_w[kWaves];
    ScanV run = agg[blockIdx.x];
    const uint32_t n_int = h->n_int;  // round 1 only: written by round 0's be_scan_blocks
    for (uint32_t r = 0; r < kTile / kThreads; ++r) {
        const uint32_t i = blockIdx.x * kTile + r * kThreads + threadIdx.x;
        const ScanV v = scan_value(nodes, n_nodes, i, round, blk);
        const ScanV e = block_scan(v, run, s_w);
        if (i >= n_nodes) continue;
        if (round == 0) {
            blk[i] = e.a > 0xffffffffull ? 0xffffffffu : (uint32_t)e.a;
            slot[i] = v.b ? e.b : kNone;
        } else if (v.b) {
            slot[i] = n_int + e.b;
        }
    }
}

// ------------------------------------------------------------- records ----
// DevNode i from OutNode i and its children: 8 lanes per record, lane p the words 2p, 2p + 1.
__global__ void be_nodes(const OutNode* nodes, uint32_t n_nodes, DevNode* out) {
    const u64 g = (u64)blockIdx.x * kThreads + threadIdx.x;
    const uint32_t i = (uint32_t)(g >> 3), p = (uint32_t)g & 7u;
    if (i >= n_nodes) return;
    const OutNode& n = nodes[i];
    const bool leaf = n.left < 0;
    u64 w0 = 0, w1 = 0;
    if (p < 6) {
        if (!leaf) {  // lmin lmax | rmin rmax: the children's boxes
            const u64* b = (const u64*)nodes[p < 3 ? n.left : n.right].box;
            w0 = b[(p % 3) * 2];
            w1 = b[(p % 3) * 2 + 1];
        }
    } else if (p == 6) {
        w0 = (u64)(uint32_t)(int32_t)n.left | (u64)(uint32_t)(int32_t)n.right << 32;
        w1 = (u64)(uint32_t)n.start | (u64)prims(n) << 32;
    } else if (!leaf) {  // the children's ranges
        const OutNode &l = nodes[n.left], &r = nodes[n.right];
        w0 = (u64)(uint32_t)l.start | (u64)prims(l) << 32;
        w1 = (u64)(uint32_t)r.start | (u64)prims(r) << 32;
    }
    *(ulonglong2*)((char*)(out + i) + p * 16) = make_ulonglong2(w0, w1);
}

// build_compact's word(): how a parent names child idx
__device__ __forceinline__ uint32_t child_word_c(const OutNode* nodes, int64_t idx, const uint32_t* blk,
                                                 const uint32_t* slot) {
    const OutNode& c = nodes[idx];
    if (c.left >= 0) return slot[idx];
    const uint32_t cnt = prims(c);
    if (packs(cnt, blk[idx])) return kPackedLeaf | (cnt << 24) | blk[idx];
    return slot[idx] | kLeafRef;
}
// floats 4q .. 4q + 3 of the twelve box floats (A min, A max, B min, B max) of two boxes
__device__ __forceinline__ void box_floats(const double* A, const double* B, uint32_t q, uint32_t f[4]) {
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t k = q * 4 + j;
        f[j] = f32_bits(k < 6 ? A[k] : B[k - 6]);
    }
}

// DevNodeC at slot[i]: 4 lanes per record, lane p the floats / words 4p .. 4p + 3.
__global__ void be_cnodes(const OutNode* nodes, uint32_t n_nodes, const uint32_t* blk, const uint32_t* slot,
                          DevNodeC* out) {
    const u64 g = (u64)blockIdx.x * kThreads + threadIdx.x;
    const uint32_t i = (uint32_t)(g >> 2), p = (uint32_t)g & 3u;
    if (i >= n_nodes) return;
    const uint32_t s = slot[i];
    if (s == kNone) return;
    const OutNode& n = nodes[i];
    uint32_t f[4] = {0, 0, 0, 0};
    if (n.left >= 0) {
        if (p < 3) {
            box_floats(nodes[n.left].box, nodes[n.right].box, p, f);
        } else {
            f[0] = child_word_c(nodes, n.left, blk, slot);
            f[1] = child_word_c(nodes, n.right, blk, slot);
        }
    } else if (p == 3) {  // a big leaf: its block and count
        f[2] = blk[i];
        f[3] = prims(n);
    }
    store16((char*)(out + s) + p * 16, f[0], f[1], f[2], f[3]);
}

// Pair line of inner slot slot[i]: 8 lanes, lanes 0-3 the left child's half, 4-7 the right's.
__global__ void be_pairs(const OutNode* nodes, uint32_t n_nodes, const uint32_t* blk, const uint32_t* slot,
                         float* out) {
    const u64 g = (u64)blockIdx.x * kThreads + threadIdx.x;
    const uint32_t i = (uint32_t)(g >> 3), p = (uint32_t)g & 7u, q = p & 3u;
    if (i >= n_nodes) return;
    const OutNode& n = nodes[i];
    if (n.left < 0) return;
    const int64_t kid = p < 4 ? n.left : n.right;
    const OutNode& K = nodes[kid];
    const bool leaf = K.left < 0;
    uint32_t f[4];
    if (q < 3) {  // a leaf child: its own box as A and as B
        box_floats(leaf ? K.box : nodes[K.left].box, leaf ? K.box : nodes[K.right].box, q, f);
    } else {
        f[0] = leaf ? 0u : child_word_c(nodes, K.left, blk, slot);
        f[1] = leaf ? 0u : child_word_c(nodes, K.right, blk, slot);
        f[2] = child_word_c(nodes, kid, blk, slot);
        f[3] = leaf ? kPairLeaf : 0u;
    }
    store16((char*)(out + (size_t)slot[i] * kPairFloats) + p * 16, f[0], f[1], f[2], f[3]);
}

// Floats 4c .. 4c + 3 of a leaf's block: the header word (the first primitive index), then
// a, b, c of each triangle as f32, then zeros up to the line's end.
__device__ __forceinline__ void leaf_part(const double* items, const uint32_t* order, uint32_t start, uint32_t count,
                                          u64 c, uint32_t f[4]) {
    for (uint32_t j = 0; j < 4; ++j) {
        const u64 k = c * 4 + j;
        f[j] = 0;
        if (k == 0) { f[j] = start; continue; }
        const u64 t = (k - 1) / kTriC;
        if (t >= count) continue;
        const uint32_t comp = (uint32_t)((k - 1) % kTriC);
        const uint32_t word = comp < 3 ? kWA + comp : (comp < 6 ? kWB + comp - 3 : kWC + comp - 6);
        f[j] = f32_bits(items[(size_t)order[start + t] * kItemWords + word]);
    }
}
// 8 lanes per node: a leaf of up to kGroupLeaf triangles is written line by line, lane p
// the line's 16-byte part p; a larger one is queued for be_big_leaves.
__global__ void be_leaves(const OutNode* nodes, uint32_t n_nodes, const uint32_t* blk, const double* items,
                          const uint32_t* order, float* ctris, uint32_t* queue, Header* h) {
    const u64 g = (u64)blockIdx.x * kThreads + threadIdx.x;
    const uint32_t i = (uint32_t)(g >> 3), p = (uint32_t)g & 7u;
    if (i >= n_nodes) return;
    const OutNode& n = nodes[i];
    if (n.left >= 0) return;
    const uint32_t cnt = prims(n), start = (uint32_t)n.start;
    if (cnt > kGroupLeaf) {
        if (p == 0) queue[atomicAdd(&h->n_queued, 1u)] = i;
        return;
    }
    char* dst = (char*)(ctris + (size_t)blk[i] * kLeafBlock);
    const uint32_t parts = (uint32_t)leaf_lines(cnt) * 8;
    for (uint32_t c = p; c < parts; c += 8) {
        uint32_t f[4];
        leaf_part(items, order, start, cnt, c, f);
        store16(dst + (size_t)c * 16, f[0], f[1], f[2], f[3]);
    }
}
// The queued leaves, a block per leaf at a time (a SameNode leaf can hold thousands).
__global__ void be_big_leaves(const OutNode* nodes, const uint32_t* blk, const double* items, const uint32_t* order,
                              float* ctris, const uint32_t* queue, const Header* h) {
    const uint32_t nq = h->n_queued;
    for (uint32_t e = blockIdx.x; e < nq; e += gridDim.x) {
        const uint32_t i = queue[e];
        const OutNode& n = nodes[i];
        const uint32_t cnt = prims(n), start = (uint32_t)n.start;
        char* dst = (char*)(ctris + (size_t)blk[i] * kLeafBlock);
        const u64 parts = leaf_lines(cnt) * 8;
        for (u64 c = threadIdx.x; c < parts; c += kThreads) {
            uint32_t f[4];
            leaf_part(items, order, start, cnt, c, f);
            store16(dst + c * 16, f[0], f[1], f[2], f[3]);
        }
    }
}

// The per-triangle arrays in BVH order: record k comes from item order[k].  A block
// fetches 64 items (random 288-B reads) as 16-byte loads, 18 per item, into LDS, and
// writes the five arrays' 64-record stretches as 16-byte stores.  Words are copied as
// integers: NaN payloads and zero signs pass through.
__global__ void be_gather(const ulonglong2* items, const uint32_t* order, uint32_t n, DevTri* tris,
                          DevTriCold* cold, u64* inv_area, uint32_t* mat, uint32_t* gid) {
    __shared__ u64 s[kGatherTris * kItemWords];
    const uint32_t k0 = blockIdx.x * kGatherTris, tid = threadIdx.x;
    const uint32_t cnt = n - k0 < kGatherTris ? n - k0 : kGatherTris;
    constexpr uint32_t kParts = kItemWords / 2;  // 16-byte parts per item
    for (uint32_t c = tid; c < cnt * kParts; c += kThreads) {
        const uint32_t t = c / kParts, part = c % kParts;
        const ulonglong2 v = items[(size_t)order[k0 + t] * kParts + part];
        s[t * kItemWords + part * 2] = v.x;
        s[t * kItemWords + part * 2 + 1] = v.y;
    }
    __syncthreads();
    // DevTri: a, ba, ca = the item's first nine words, pad = 0.0
    for (uint32_t c = tid; c < cnt * 5; c += kThreads) {
        const uint32_t t = c / 5, part = c % 5;
        const u64* it = s + t * kItemWords;
        ((ulonglong2*)(tris + k0))[c] = make_ulonglong2(it[part * 2], part < 4 ? it[part * 2 + 1] : 0ull);
    }
    // DevTriCold: ng (words 9-11), then na, nb, nc (13-21)
    for (uint32_t c = tid; c < cnt * 6; c += kThreads) {
        const uint32_t t = c / 6, w = (c % 6) * 2;
        const u64* it = s + t * kItemWords;
        ((ulonglong2*)(cold + k0))[c] =
            make_ulonglong2(it[w < 3 ? kWNg + w : kWNa + w - 3], it[w + 1 < 3 ? kWNg + w + 1 : kWNa + w - 2]);
    }
    // tri_inv_area: two per store
    for (uint32_t c = tid; c < (cnt + 1) / 2; c += kThreads) {
        const u64 x = s[(2 * c) * kItemWords + kWInvArea];
        if (2 * c + 1 < cnt) ((ulonglong2*)(inv_area + k0))[c] = make_ulonglong2(x, s[(2 * c + 1) * kItemWords + kWInvArea]);
        else inv_area[k0 + 2 * c] = x;
    }
    // mat and gid share a word of the item: four of each per store
    for (uint32_t c = tid; c < (cnt + 3) / 4 * 2; c += kThreads) {
        const uint32_t hi = c & 1u, t0 = (c >> 1) * 4;
        uint32_t* dst = (hi ? gid : mat) + k0 + t0;
        uint32_t v[4] = {0, 0, 0, 0};
        for (uint32_t j = 0; j < 4 && t0 + j < cnt; ++j) v[j] = (uint32_t)(s[(t0 + j) * kItemWords + kWMatGid] >> (hi * 32));
        if (t0 + 4 <= cnt) store16(dst, v[0], v[1], v[2], v[3]);
        else for (uint32_t j = 0; t0 + j < cnt; ++j) dst[j] = v[j];
    }
}

inline uint32_t blocks(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

}  // namespace

#define BE_MARK(name) RT_EMIT_MARK(name)
#define BE_TRY(call)                                                         \
    do {                                                                     \
        const hipError_t e_ = (call);                                        \
        if (e_ != hipSuccess) { err = hipGetErrorString(e_); out.dev.reset(); return kDeviceBuildError; } \
    } while (0)
#define BE_SCRATCH_OK()                                                      \
    do {                                                                     \
        if (!m.ok()) { if (m.oom) return kDeviceBuildFallback; BE_TRY(m.err); } \
    } while (0)

namespace {

int emit_core(Arena& m, const TriItem* d_items, double* d_boxes, uint32_t n, bool compact, uint32_t max_levels,
              HostBvhArrays& out, std::string& err) {
    const hipStream_t st = 0;
    RT_EMIT_MARK_START();
    DevTree t;
    const int made = build_bvh_device_tree(m, d_boxes, n, max_levels, t, err);
    if (made != kDeviceBuildDone) return made;
    m.release(d_boxes);
    BE_MARK("builder");
    const uint32_t nn = t.n_nodes;

    // flags, block indices and slots
    const uint32_t nblk = blocks(nn, kTile);
    uint32_t* d_blk = m.get<uint32_t>(nn);
    uint32_t* d_slot = m.get<uint32_t>(nn);
    ScanV* d_agg = m.get<ScanV>(nblk);
    uint32_t* d_queue = m.get<uint32_t>(n / (kGroupLeaf + 1) + 1);  // leaves of more than kGroupLeaf triangles
    Header* d_hdr = m.get<Header>(1);
    BE_SCRATCH_OK();
    be_init<<<1, 1, 0, st>>>(d_hdr);
    be_node_flags<<<blocks(nn, kThreads), kThreads, 0, st>>>(t.nodes, nn, &d_hdr->flags);
    be_item_flags<<<blocks(n, kThreads), kThreads, 0, st>>>((const double*)d_items, n, &d_hdr->flags);
    for (int round = 0; round < 2; ++round) {
        be_scan_reduce<<<nblk, kThreads, 0, st>>>(t.nodes, nn, round, d_blk, d_agg);
        be_scan_blocks<<<1, kThreads, 0, st>>>(d_agg, nblk, round, d_hdr);
        be_scan_final<<<nblk, kThreads, 0, st>>>(t.nodes, nn, round, d_agg, d_blk, d_slot, d_hdr);
    }
    BE_TRY(hipGetLastError());
    Header h;
    double root[6];
    BE_TRY(hipMemcpyAsync(&h, d_hdr, sizeof(h), hipMemcpyDeviceToHost, st));
    BE_TRY(hipMemcpyAsync(root, t.nodes, sizeof(root), hipMemcpyDeviceToHost, st));
    BE_TRY(hipStreamSynchronize(st));

    BE_MARK("flags, scans");

    // build_compact's rules, then build_pairs'
    const uint64_t n_slots = (uint64_t)h.n_int + h.n_big;
    const bool want_c = compact && (h.flags & kFlagExact) && h.n_int > 0 && n_slots < kLeafRef &&
                        h.n_lines < (1ull << 32);
    const bool want_p = want_c && (h.flags & kFlagUnion);

    // the final arrays, in upload_bvh's order and with its sizes
    DevResident& D = out.dev;
    D.reset();
    D.release = [](void* p) { (void)hipFree(p); };
    const uint64_t counts[kResArrays] = {nn, n, n, n, n, n, want_c ? n_slots : 0, want_c ? h.n_lines * kLeafBlock : 0,
                                         want_p ? (uint64_t)h.n_int * kPairFloats : 0};
    const size_t elem[kResArrays] = {sizeof(DevNode), sizeof(DevTri), sizeof(DevTriCold), sizeof(double),
                                     sizeof(uint32_t), sizeof(int32_t), sizeof(DevNodeC), sizeof(float), sizeof(float)};
    for (int k = 0; k < kResArrays; ++k) {
        if (!counts[k]) continue;
        const hipError_t e = hipMalloc(&D.ptr[k], counts[k] * elem[k]);
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); D.reset(); return kDeviceBuildFallback; }
        BE_TRY(e);
        D.count[k] = counts[k];
    }
    BE_MARK("final allocs");
    be_nodes<<<blocks((uint64_t)nn * 8, kThreads), kThreads, 0, st>>>(t.nodes, nn, (DevNode*)D.ptr[kResNodes]);
    be_gather<<<blocks(n, kGatherTris), kThreads, 0, st>>>((const ulonglong2*)d_items, t.order, n,
                                                           (DevTri*)D.ptr[kResTris], (DevTriCold*)D.ptr[kResCold],
                                                           (u64*)D.ptr[kResInvArea], (uint32_t*)D.ptr[kResMat],
                                                           (uint32_t*)D.ptr[kResGid]);
    if (want_c) {
        be_cnodes<<<blocks((uint64_t)nn * 4, kThreads), kThreads, 0, st>>>(t.nodes, nn, d_blk, d_slot,
                                                                           (DevNodeC*)D.ptr[kResCnodes]);
        be_leaves<<<blocks((uint64_t)nn * 8, kThreads), kThreads, 0, st>>>(t.nodes, nn, d_blk, (const double*)d_items,
                                                                           t.order, (float*)D.ptr[kResCtris], d_queue,
                                                                           d_hdr);
        be_big_leaves<<<kBigGrid, kThreads, 0, st>>>(t.nodes, d_blk, (const double*)d_items, t.order,
                                                     (float*)D.ptr[kResCtris], d_queue, d_hdr);
    }
    if (want_p)
        be_pairs<<<blocks((uint64_t)nn * 8, kThreads), kThreads, 0, st>>>(t.nodes, nn, d_blk, d_slot,
                                                                          (float*)D.ptr[kResPnodes]);
    BE_TRY(hipGetLastError());
    BE_TRY(hipStreamSynchronize(st));
    BE_MARK("record kernels");
    D.on = true;
    out.root = Box3{v3(root[0], root[1], root[2]), v3(root[3], root[4], root[5])};
    out.n_prims = n;
    out.depth = t.depth;
    out.fast = (h.flags & kFlagFast) != 0;
    out.tri_q = (h.flags & kFlagTriQ) != 0;
    return kDeviceBuildDone;
}

}  // namespace

int emit_tri_bvh_device_core(Arena& m, const TriItem* d_items, double* d_boxes, uint32_t n, bool compact,
                             uint32_t max_levels, HostBvhArrays& out, std::string& err) {
    if (n == 0 || n > kMaxPrims) return kDeviceBuildFallback;
    const size_t mark = m.ptrs.size();
    const int made = emit_core(m, d_items, d_boxes, n, compact, max_levels, out, err);
    m.release_since(mark, nullptr, nullptr);  // the tree and the tables: the caller's next BVH gets the room
    return made;
}

int emit_tri_bvh_device(const std::vector<TriItem>& items, bool compact, uint32_t max_levels, HostBvhArrays& out,
                        std::string& err) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        err = "no HIP device visible (the device builder needs one)";
        return kDeviceBuildError;
    }
    const uint64_t n64 = items.size();
    if (n64 == 0 || n64 > kMaxPrims) return kDeviceBuildFallback;
    const uint32_t n = (uint32_t)n64;
    const hipStream_t st = 0;
    Arena m;
    RT_EMIT_MARK_START();

    // the triangles as they are, once; the builder's boxes out of them
    TriItem* d_items = m.get<TriItem>(n);
    double* d_boxes = m.get<double>((size_t)n * 6);
    BE_SCRATCH_OK();
    BE_TRY(hipMemcpyAsync(d_items, items.data(), (size_t)n * sizeof(TriItem), hipMemcpyHostToDevice, st));
    be_boxes<<<blocks((uint64_t)n * 6, kThreads), kThreads, 0, st>>>((const u64*)d_items, n, (u64*)d_boxes);
    BE_TRY(hipGetLastError());
    BE_MARK("item upload");
    return emit_tri_bvh_device_core(m, d_items, d_boxes, n, compact, max_levels, out, err);
}

}  // namespace rt

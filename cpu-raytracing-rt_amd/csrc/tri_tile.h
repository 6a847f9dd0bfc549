// tri_tile.h — the tile of TriItems in LDS that ti_items (tri_items.hip) and gf_items
// (gltf_items.hip) both work in: a block takes kTile = 64 triangles, all 256 lanes bring
// the tile's inputs into the LDS slots of the items they belong to, wave 0 computes a
// triangle per lane in its item's slot, and all lanes store the items and the boxes as
// 16-byte words.  An item takes kStride = 37 eight-byte words of LDS, not 36: with an odd
// stride the 8-byte accesses of 32 consecutive lanes fall into 32 different bank pairs.
#pragma once
#include <hip/hip_runtime.h>

#include "bvh_device.h"
#include "scene_build.h"

namespace rt {
namespace tile {

constexpr uint32_t kThreads = 256;            // four wave64s
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kTile = 64;                // triangles per block: a triangle per lane of wave 0
constexpr uint32_t kFixCap = 65536;           // fix-up queue: more NaN triangles than this and the host computes all
constexpr uint64_t kMaxPrims = 1ull << 30;    // as the builder's
typedef unsigned long long u64;

// TriItem as 36 eight-byte words (bvh_emit.hip asserts the same offsets)
constexpr uint32_t kItemWords = sizeof(TriItem) / 8, kItemParts = kItemWords / 2;
constexpr uint32_t kStride = kItemWords + 1;  // LDS words per item: odd
constexpr uint32_t kWBa = offsetof(TriItem, t.ba) / 8, kWNa = offsetof(TriItem, t.na) / 8,
                   kWB = offsetof(TriItem, b) / 8, kWMatGid = offsetof(TriItem, mat) / 8,
                   kWBox = offsetof(TriItem, box) / 8;
static_assert(offsetof(TriItem, t.a) == 0 && kWBa == 3 && offsetof(TriItem, t.ng) == 72 && kWNa == 13 && kWB == 22 &&
              offsetof(TriItem, c) == 200 && offsetof(TriItem, mat) == 224 && offsetof(TriItem, gid) == 228 &&
              kWBox == 29 && kItemWords == 36, "TriItem's words as the kernels index them");

__device__ __forceinline__ bool nan_bits(u64 w) { return (w & 0x7fffffffffffffffull) > 0x7ff0000000000000ull; }
__device__ __forceinline__ double as_f64(u64 w) { return __longlong_as_double((long long)w); }
__device__ __forceinline__ u64 as_u64(double v) { return (u64)__double_as_longlong(v); }
__device__ __forceinline__ V3 lds3(const u64* p) { return v3(as_f64(p[0]), as_f64(p[1]), as_f64(p[2])); }
__device__ __forceinline__ void put3(u64* p, V3 v) { p[0] = as_u64(v.x); p[1] = as_u64(v.y); p[2] = as_u64(v.z); }

// A glTF item in its slot: a | b, c and the normals stand there as its inputs and stay;
// the normals take no part in the arithmetic.  Fills ba, ca, ng, inv_area and the box.
__device__ __forceinline__ void gltf_item_in_slot(u64* it) {
    const V3 a = lds3(it), b = lds3(it + kWB), c = lds3(it + kWB + 3);
    TriItem r;
    tri_item_gltf(a, b, c, v3(0, 0, 0), v3(0, 0, 0), v3(0, 0, 0), r);
    put3(it + kWBa, r.t.ba); put3(it + kWBa + 3, r.t.ca); put3(it + kWBa + 6, r.t.ng);
    it[kWBa + 9] = as_u64(r.t.inv_area);
    put3(it + kWBox, r.box.min); put3(it + kWBox + 3, r.box.max);
}
// Whether any double of the finished item is a NaN (mat | gid is no double)
__device__ __forceinline__ bool item_has_nan(const u64* it) {
    bool bad = false;
    for (uint32_t k = 0; k < kItemWords - 1; ++k)
        if (k != kWMatGid) bad = bad || nan_bits(it[k]);
    return bad;
}
// Wave 0, every lane: triangle j joins the fix-up queue where bad.  One atomic per wave
// that has any; n_nan counts all of them, also those past kFixCap, which are not stored.
__device__ __forceinline__ void queue_bad(bool bad, uint32_t j, uint32_t* queue, ItemsHeader* h) {
    const u64 vote = __ballot(bad);
    if (!vote) return;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&h->n_nan, (uint32_t)__popcll(vote));
    base = __shfl(base, 0);
    const uint32_t at = base + (uint32_t)__popcll(vote & ((1ull << lane) - 1ull));
    if (bad && at < kFixCap) queue[at] = j;
}
// All lanes: the tile's cnt items (18 sixteen-byte words each) and boxes (3 each) to
// items[j0..] and boxes[j0..]
__device__ __forceinline__ void store_tile(const u64* s, uint32_t j0, uint32_t cnt, ulonglong2* items, ulonglong2* boxes) {
    for (uint32_t c = threadIdx.x; c < cnt * kItemParts; c += kThreads) {
        const u64* w = s + c / kItemParts * kStride + c % kItemParts * 2;
        items[(size_t)j0 * kItemParts + c] = make_ulonglong2(w[0], w[1]);
    }
    for (uint32_t c = threadIdx.x; c < cnt * 3; c += kThreads) {
        const u64* w = s + c / 3 * kStride + kWBox + c % 3 * 2;
        boxes[(size_t)j0 * 3 + c] = make_ulonglong2(w[0], w[1]);
    }
}

}  // namespace tile
}  // namespace rt

// The front ends' and the tail's error returns (tris, ltris and err are the caller's):
// a failed HIP call is kDeviceBuildError, scratch that does not fit kDeviceBuildFallback.
#define TI_TRY(call)                                                                         \
    do {                                                                                     \
        const hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) { err = hipGetErrorString(e_); tris.dev.reset(); ltris.dev.reset(); return kDeviceBuildError; } \
    } while (0)
#define TI_SCRATCH_OK()                                                                      \
    do {                                                                                     \
        if (!m.ok()) { if (m.oom) return kDeviceBuildFallback; TI_TRY(m.err); }              \
    } while (0)

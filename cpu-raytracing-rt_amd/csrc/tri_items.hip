// tri_items.hip — the triangle items of scene creation computed on the device.
//
// build_scene's item loop (tri_items.h: triangle_props / triangle_smooth / triangle_geometric,
// the quaternion rotations of a custom-format triangle, the box) is per-triangle f64
// arithmetic from the description's arrays.  The kernels here run it where bvh_emit.hip
// wants its result (DESIGN.md §2 "Device items"):
//   ti_items          description arrays -> TriItem array and the builder's box array
//   ti_patch          the items the host recomputed (the NaN fix-up list) scattered into place
//   ti_light_reduce   light triangles per block of kScanTile
//   ti_light_blocks   one block: exclusive scan of the block sums, the total
//   ti_compact        the light triangles' items and boxes, stably, into arrays of their own
// ti_items: a block takes a tile of 64 triangles (tri_tile.h, shared with gltf_items.hip's
// gf_items).  All 256 lanes stage the tile's inputs with 16-byte loads straight into the
// LDS slots of the items they belong to (vertices, glTF normals and the material are words
// of the item as they are), wave 0 computes a triangle per lane in its item's slot, and
// all lanes store the items and the boxes as 16-byte words.
// Words that are only copied never pass through a floating-point register.
// finish_device_items is the tail after the item kernel, shared with gltf_items.hip.
#include <hip/hip_runtime.h>

#include <cstring>

#include "bvh_device.h"
#include "scene_build.h"
#include "tri_tile.h"

namespace rt {
namespace {

using namespace tile;
constexpr uint32_t kScanTile = 1024;          // triangles per block of the light scan
constexpr uint32_t kNone = 0xffffffffu;
typedef ItemsHeader Header;
// custom mode: where a tile's positions and rotations wait in the item's slot (the normals' words)
constexpr uint32_t kWPos = kWNa, kWRot = kWNa + 3;

__global__ void ti_init(Header* h) { h->n_nan = 0; h->n_light = 0; h->scan = 0; }

// word k of a triangle's nine vertex doubles -> its word in the item (a | b, c)
__device__ __forceinline__ uint32_t vertex_word(uint32_t k) { return k < 3 ? k : kWB + k - 3; }

// The tile's part of an array of `per` words per triangle, src already at the tile's first
// word (16-byte aligned: a tile starts at an even triangle), into the items' slots: word k
// of triangle t goes to s[t * kStride + (vertex ? vertex_word(k) : first + k)].
template <uint32_t per, bool vertex>
__device__ __forceinline__ void stage(const u64* src, uint32_t cnt, uint32_t first, u64* s) {
    const uint32_t words = cnt * per;
    for (uint32_t c = threadIdx.x; c < words / 2; c += kThreads) {
        const ulonglong2 v = ((const ulonglong2*)src)[c];
        const uint32_t w0 = 2 * c, w1 = 2 * c + 1;
        s[w0 / per * kStride + (vertex ? vertex_word(w0 % per) : first + w0 % per)] = v.x;
        s[w1 / per * kStride + (vertex ? vertex_word(w1 % per) : first + w1 % per)] = v.y;
    }
    if ((words & 1u) && threadIdx.x == 0) {  // an odd tail tile: the last word on its own, nothing past the array's end
        const uint32_t w = words - 1;
        s[w / per * kStride + (vertex ? vertex_word(w % per) : first + w % per)] = src[w];
    }
}

// items[j] and boxes[j] of triangles j < n.  nrm: glTF mode (normals); else custom mode
// with pos / rot, either of which may be null (0 / identity).  queue: the triangles with a
// NaN among their input doubles or their item's words, in no order, n_nan counting all of
// them (also those past kFixCap, which are not stored).
__global__ __launch_bounds__(kThreads) void ti_items(const u64* vtx, const u64* nrm, const u64* pos, const u64* rot,
                                                     const uint32_t* mat, uint32_t n, uint32_t n_shapes,
                                                     ulonglong2* items, ulonglong2* boxes, uint32_t* queue,
                                                     Header* h) {
    __shared__ u64 s[kTile * kStride];
    const uint32_t j0 = blockIdx.x * kTile, tid = threadIdx.x;
    const uint32_t cnt = n - j0 < kTile ? n - j0 : kTile;
    const bool gltf = nrm != nullptr;

    stage<9, true>(vtx + (size_t)j0 * 9, cnt, 0, s);
    if (gltf) stage<9, false>(nrm + (size_t)j0 * 9, cnt, kWNa, s);
    if (!gltf && pos) stage<3, false>(pos + (size_t)j0 * 3, cnt, kWPos, s);
    if (!gltf && rot) stage<4, false>(rot + (size_t)j0 * 4, cnt, kWRot, s);
    // the material: four per load into the low halves of the items' mat | gid words
    uint32_t* s32 = (uint32_t*)s;
    for (uint32_t c = tid; c < cnt / 4; c += kThreads) {
        const uint4 m4 = ((const uint4*)(mat + j0))[c];
        s32[((4 * c + 0) * kStride + kWMatGid) * 2] = m4.x;
        s32[((4 * c + 1) * kStride + kWMatGid) * 2] = m4.y;
        s32[((4 * c + 2) * kStride + kWMatGid) * 2] = m4.z;
        s32[((4 * c + 3) * kStride + kWMatGid) * 2] = m4.w;
    }
    if (tid >= (cnt & ~3u) && tid < cnt) s32[(tid * kStride + kWMatGid) * 2] = mat[j0 + tid];
    __syncthreads();

    if (tid < 64) {  // wave 0: lane t computes triangle j0 + t in its slot
        bool bad = false;
        if (tid < cnt) {
            u64* it = s + tid * kStride;
            if (gltf) {
                gltf_item_in_slot(it);
            } else {
                const V3 a = lds3(it), b = lds3(it + kWB), c = lds3(it + kWB + 3);
                TriItem r;
                const V3 p = pos ? lds3(it + kWPos) : v3(0, 0, 0);
                const Quat q = rot ? Quat{as_f64(it[kWRot]), lds3(it + kWRot + 1)} : Quat{1.0, v3(0, 0, 0)};
                for (uint32_t k = 0; k < 9; ++k) bad = bad || nan_bits(it[vertex_word(k)]);
                if (pos) for (uint32_t k = 0; k < 3; ++k) bad = bad || nan_bits(it[kWPos + k]);
                if (rot) for (uint32_t k = 0; k < 4; ++k) bad = bad || nan_bits(it[kWRot + k]);
                tri_item_custom(a, b, c, p, q, r);
                put3(it, r.t.a); put3(it + kWBa, r.t.ba); put3(it + kWBa + 3, r.t.ca); put3(it + kWBa + 6, r.t.ng);
                it[kWBa + 9] = as_u64(r.t.inv_area);
                put3(it + kWNa, r.t.na); put3(it + kWNa + 3, r.t.nb); put3(it + kWNa + 6, r.t.nc);
                put3(it + kWB, r.b); put3(it + kWB + 3, r.c);
                put3(it + kWBox, r.box.min); put3(it + kWBox + 3, r.box.max);
            }
            it[kItemWords - 1] = 0;  // TriItem's tail padding
            s32[(tid * kStride + kWMatGid) * 2 + 1] = n_shapes + j0 + tid;  // gid
            // every double of the item as it stands (in glTF mode these hold all the inputs)
            bad = bad || item_has_nan(it);
        }
        queue_bad(bad, j0 + tid, queue, h);
    }
    __syncthreads();
    store_tile(s, j0, cnt, items, boxes);
}

// fix[e] (contiguous, computed by the host) -> items[queue[e]] and its box
__global__ void ti_patch(const ulonglong2* fix, const uint32_t* queue, uint32_t n_fix, ulonglong2* items, u64* boxes) {
    const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
    if (g < n_fix * kItemParts) items[(size_t)queue[g / kItemParts] * kItemParts + g % kItemParts] = fix[g];
    if (g < n_fix * 6)
        boxes[(size_t)queue[g / 6] * 6 + g % 6] = ((const u64*)fix)[(size_t)(g / 6) * kItemWords + kWBox + g % 6];
}

// ------------------------------------------------------- light triangles ----
__device__ __forceinline__ bool light_flag(const uint32_t* mat, const uint8_t* light, uint32_t n, uint32_t j) {
    return j < n && light[mat[j]] != 0;  // mat[j] < n_materials: checked on the host before any launch
}
__global__ void ti_light_reduce(const uint32_t* mat, const uint8_t* light, uint32_t n, uint32_t* agg) {
    __shared__ uint32_t s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t r = 0; r < kScanTile / kThreads; ++r)
        mine += (uint32_t)__popcll(__ballot(light_flag(mat, light, n, blockIdx.x * kScanTile + r * kThreads + threadIdx.x)));
    if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(&s_sum, mine);
    __syncthreads();
    if (threadIdx.x == 0) agg[blockIdx.x] = s_sum;
}
// One block: agg[b] becomes the number of light triangles before block b; the total goes to the header.
__global__ void ti_light_blocks(uint32_t* agg, uint32_t nblk, Header* h) {
    __shared__ uint32_t s_w[kWaves];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t run = 0;
    for (uint32_t j0 = 0; j0 < nblk; j0 += kThreads) {
        const uint32_t j = j0 + threadIdx.x;
        const uint32_t v = j < nblk ? agg[j] : 0u;
        uint32_t x = v;
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) s_w[w] = x;
        __syncthreads();
        uint32_t before = run;
        for (uint32_t k = 0; k < kWaves; ++k) {
            if (k < w) before += s_w[k];
            run += s_w[k];
        }
        __syncthreads();
        if (j < nblk) agg[j] = before + x - v;
    }
    if (threadIdx.x == 0) h->n_light = run;
}
// The light triangles of the block's kScanTile, 256 at a time: the slot of each from a
// ballot scan, then its item as 18 and its box as 3 sixteen-byte words, a lane per word.
__global__ void ti_compact(const ulonglong2* items, const ulonglong2* boxes, const uint32_t* mat, const uint8_t* light,
                           uint32_t n, const uint32_t* agg, ulonglong2* litems, ulonglong2* lboxes) {
    __shared__ uint32_t s_w[kWaves], s_dst[kThreads];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t run = agg[blockIdx.x];
    for (uint32_t r = 0; r < kScanTile / kThreads; ++r) {
        const uint32_t j0 = blockIdx.x * kScanTile + r * kThreads;
        if (j0 >= n) break;  // the same for every lane
        const bool f = light_flag(mat, light, n, j0 + threadIdx.x);
        const u64 vote = __ballot(f);
        if (lane == 0) s_w[w] = (uint32_t)__popcll(vote);
        __syncthreads();
        uint32_t before = run;
        for (uint32_t k = 0; k < kWaves; ++k) {
            if (k < w) before += s_w[k];
            run += s_w[k];
        }
        s_dst[threadIdx.x] = f ? before + (uint32_t)__popcll(vote & ((1ull << lane) - 1ull)) : kNone;
        __syncthreads();
        const uint32_t cnt = n - j0 < kThreads ? n - j0 : kThreads;
        for (uint32_t c = threadIdx.x; c < cnt * kItemParts; c += kThreads) {
            const uint32_t d = s_dst[c / kItemParts];
            if (d != kNone) litems[(size_t)d * kItemParts + c % kItemParts] = items[(size_t)j0 * kItemParts + c];
        }
        for (uint32_t c = threadIdx.x; c < cnt * 3; c += kThreads) {
            const uint32_t d = s_dst[c / 3];
            if (d != kNone) lboxes[(size_t)d * 3 + c % 3] = boxes[(size_t)j0 * 3 + c];
        }
        __syncthreads();
    }
}

inline uint32_t blocks(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

}  // namespace

void items_header_clear(ItemsHeader* d_hdr, hipStream_t st) { ti_init<<<1, 1, 0, st>>>(d_hdr); }

int finish_device_items(Arena& m, uint32_t n, TriItem* d_items, double* d_boxes, uint32_t* d_mat, uint8_t* d_light,
                        uint32_t* d_queue, ItemsHeader* d_hdr, void* const* inputs, uint32_t n_inputs,
                        void (*item_of)(const void* ctx, uint32_t j, TriItem& it), const void* ctx, uint32_t max_levels,
                        HostBvhArrays& tris, HostBvhArrays& ltris, TriItemsOutcome& res, std::string& err) {
    const hipStream_t st = 0;
    RT_EMIT_MARK_START();
    const uint32_t nblk = blocks(n, kScanTile);
    uint32_t* d_agg = m.get<uint32_t>(nblk);
    TI_SCRATCH_OK();
    ti_light_reduce<<<nblk, kThreads, 0, st>>>(d_mat, d_light, n, d_agg);
    ti_light_blocks<<<1, kThreads, 0, st>>>(d_agg, nblk, d_hdr);
    TI_TRY(hipGetLastError());
    Header h;
    TI_TRY(hipMemcpyAsync(&h, d_hdr, sizeof(h), hipMemcpyDeviceToHost, st));
    TI_TRY(hipStreamSynchronize(st));
    for (uint32_t k = 0; k < n_inputs; ++k) m.release(inputs[k]);
    RT_EMIT_MARK("light scan");
    // the host computes every item, as without this path (and reports what the scan found)
    if (h.scan || h.n_nan > kFixCap) return kDeviceBuildFallback;
    res.n_light = h.n_light;

    // NaN bit patterns are not promised to be the host's: those items come from the host
    if (h.n_nan) {
        std::vector<uint32_t> idx(h.n_nan);
        TI_TRY(hipMemcpy(idx.data(), d_queue, (size_t)h.n_nan * 4, hipMemcpyDeviceToHost));
        std::vector<TriItem> fix(h.n_nan);
        for (uint32_t e = 0; e < h.n_nan; ++e) item_of(ctx, idx[e], fix[e]);
        TriItem* d_fix = m.get<TriItem>(h.n_nan);
        TI_SCRATCH_OK();
        TI_TRY(hipMemcpyAsync(d_fix, fix.data(), (size_t)h.n_nan * sizeof(TriItem), hipMemcpyHostToDevice, st));
        ti_patch<<<blocks((uint64_t)h.n_nan * kItemParts, kThreads), kThreads, 0, st>>>(
            (const ulonglong2*)d_fix, d_queue, h.n_nan, (ulonglong2*)d_items, (u64*)d_boxes);
        TI_TRY(hipGetLastError());
        TI_TRY(hipStreamSynchronize(st));  // fix is the copy's source until here
        m.release(d_fix);
        RT_EMIT_MARK("fix-up");
    }

    // bvh[5]'s items: the light triangles, in list order
    TriItem* d_litems = nullptr;
    double* d_lboxes = nullptr;
    if (h.n_light) {
        d_litems = m.get<TriItem>(h.n_light);
        d_lboxes = m.get<double>((size_t)h.n_light * 6);
        if (m.oom) {  // bvh[5] alone takes the host path
            m.oom = false;
            m.release(d_litems);
            d_litems = nullptr;
        } else {
            TI_SCRATCH_OK();
            ti_compact<<<nblk, kThreads, 0, st>>>((const ulonglong2*)d_items, (const ulonglong2*)d_boxes, d_mat, d_light, n,
                                                  d_agg, (ulonglong2*)d_litems, (ulonglong2*)d_lboxes);
            TI_TRY(hipGetLastError());
            TI_TRY(hipStreamSynchronize(st));
        }
        RT_EMIT_MARK("light compact");
    }
    m.release(d_mat);
    m.release(d_light);
    m.release(d_queue);
    m.release(d_agg);

    // both BVHs from the one item array; the arena frees the items when this returns
    res.made[0] = emit_tri_bvh_device_core(m, d_items, d_boxes, n, true, max_levels, tris, err);
    if (res.made[0] == kDeviceBuildError) { ltris.dev.reset(); return kDeviceBuildError; }
    m.oom = false;  // an allocation the first BVH missed says nothing about the second
    if (d_litems) res.made[1] = emit_tri_bvh_device_core(m, d_litems, d_lboxes, h.n_light, false, max_levels, ltris, err);
    if (res.made[1] == kDeviceBuildError) { tris.dev.reset(); return kDeviceBuildError; }
    return kDeviceBuildDone;
}

static void desc_item_of(const void* ctx, uint32_t j, TriItem& it) { tri_item_of(*(const rt_scene_desc*)ctx, j, it); }

int emit_tri_bvhs_device_items(const rt_scene_desc& d, uint32_t max_levels, HostBvhArrays& tris, HostBvhArrays& ltris,
                               TriItemsOutcome& res, std::string& err) {
    res = TriItemsOutcome{};
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        err = "no HIP device visible (the device builder needs one)";
        return kDeviceBuildError;
    }
    if (d.n_triangles == 0 || d.n_triangles > kMaxPrims) return kDeviceBuildFallback;
    const uint32_t n = (uint32_t)d.n_triangles;
    const bool gltf = d.tri_mode == RT_TRI_GLTF;
    const hipStream_t st = 0;
    Arena m;
    RT_EMIT_MARK_START();

    // the description's triangle arrays as they are, and a byte per material: is_light
    std::vector<uint8_t> light(d.n_materials);
    for (uint32_t i = 0; i < d.n_materials; ++i) {
        const double* e = d.materials[i].emission;
        light[i] = e[0] != 0.0 || e[1] != 0.0 || e[2] != 0.0;  // scene_build.cpp is_light
    }
    struct Src { const void* host; size_t bytes; void* dev; };
    Src src[6] = {{d.tri_vertices, (size_t)n * 72, nullptr},
                  {gltf ? d.tri_normals : nullptr, (size_t)n * 72, nullptr},
                  {gltf ? nullptr : d.tri_position, (size_t)n * 24, nullptr},
                  {gltf ? nullptr : d.tri_rotation, (size_t)n * 32, nullptr},
                  {d.tri_material, (size_t)n * 4, nullptr},
                  {light.data(), light.size(), nullptr}};
    for (Src& a : src)
        if (a.host) a.dev = m.get<char>(a.bytes);
    TriItem* d_items = m.get<TriItem>(n);
    double* d_boxes = m.get<double>((size_t)n * 6);
    uint32_t* d_queue = m.get<uint32_t>(kFixCap);
    Header* d_hdr = m.get<Header>(1);
    TI_SCRATCH_OK();
    for (const Src& a : src)
        if (a.host) TI_TRY(hipMemcpyAsync(a.dev, a.host, a.bytes, hipMemcpyHostToDevice, st));
    RT_EMIT_MARK("desc upload");

    items_header_clear(d_hdr, st);
    ti_items<<<blocks(n, kTile), kThreads, 0, st>>>((const u64*)src[0].dev, (const u64*)src[1].dev, (const u64*)src[2].dev,
                                                    (const u64*)src[3].dev, (const uint32_t*)src[4].dev, n, d.n_shapes,
                                                    (ulonglong2*)d_items, (ulonglong2*)d_boxes, d_queue, d_hdr);
    TI_TRY(hipGetLastError());
    RT_EMIT_MARK("items");
    void* const inputs[4] = {src[0].dev, src[1].dev, src[2].dev, src[3].dev};  // vertices, normals, positions, rotations
    return finish_device_items(m, n, d_items, d_boxes, (uint32_t*)src[4].dev, (uint8_t*)src[5].dev, d_queue, d_hdr, inputs, 4,
                               desc_item_of, &d, max_levels, tris, ltris, res, err);
}

}  // namespace rt

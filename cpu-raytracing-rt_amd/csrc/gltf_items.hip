// gltf_items.hip — the meshes of a deferred glTF parse flattened on the device: from
// accessor bytes straight to the TriItem and box arrays that bvh_emit.hip consumes
// (DESIGN.md §2 "Device meshes").  The host uploads the referenced buffers as one blob, the
// draw plan (gltf_math.h GltfDraw, offsets rebased to the blob) and a byte per material;
// no description array is made or uploaded.
//   gf_scan    one sweep over what the host flatten visits whether a triangle references it
//              or not: a non-finite POSITION element (the host's non-affine error) or an
//              index >= the vertex count sets a flag in the header, and the scene then
//              takes the host flatten, which reports the error in the host's order
//   gf_items   a block per tile of 64 triangles of one draw (tri_tile.h): 192 (triangle,
//              corner) lanes each load their index, gather one vertex (3 f32 position +
//              3 f32 normal at any 4-byte-aligned stride), run gltf_math.h's transforms
//              and write the six doubles into their item's LDS slot; wave 0 then computes
//              a triangle per lane exactly as ti_items does, and all lanes store
// then tri_items.hip's tail (light scan, NaN fix-up, both emissions).  A vertex that k
// corners share is transformed k times: deterministic, so the bits are the host's, and
// there is no 48-byte-per-vertex intermediate to write and read back.
#include <hip/hip_runtime.h>

#include <cstring>

#include "api_internal.h"
#include "bvh_device.h"
#include "gltf_math.h"
#include "scene_build.h"
#include "tri_tile.h"

namespace rt {
namespace {

using namespace tile;

// gf_scan's work: a chunk per block.  Packed (stride 0: elements back to back, which a
// POSITION accessor of stride 12 is as plain f32 words): `count` bytes from `off`, swept
// 16 bytes per lane between the first and last 16-byte boundary, element-wise outside.
// Strided: `count` elements `stride` bytes apart, a lane per element.
constexpr uint32_t kScanBytes = 64 * 1024;  // 16 rounds of 256 lanes x 16 B
constexpr uint32_t kScanElems = 4096;
enum : uint32_t { kF32 = 0, kU16 = 1, kU32 = 2 };
struct ScanChunk { uint64_t off; uint32_t count, stride, kind, limit; };  // limit: the draw's vertex count

__device__ __forceinline__ bool bad_word(uint32_t w, uint32_t kind, uint32_t limit) {
    if (kind == kF32) return (w & 0x7f800000u) == 0x7f800000u;  // inf or NaN
    if (kind == kU32) return w >= limit;
    return (w & 0xffffu) >= limit || (w >> 16) >= limit;
}
// one element (a u16, or a 4-byte word) at p
__device__ __forceinline__ bool bad_elem(const char* p, uint32_t kind, uint32_t limit) {
    if (kind == kU16) return *(const uint16_t*)p >= limit;
    return bad_word(*(const uint32_t*)p, kind, limit);
}

__global__ __launch_bounds__(kThreads) void gf_scan(const char* blob, const ScanChunk* chunks, ItemsHeader* h) {
    const ScanChunk c = chunks[blockIdx.x];
    const uint32_t tid = threadIdx.x, es = c.kind == kU16 ? 2u : 4u;
    const char* p = blob + c.off;  // the blob is 256-byte aligned: p's alignment is off's
    bool bad = false;
    if (c.stride == 0) {
        uint32_t head = (16u - (uint32_t)(c.off & 15u)) & 15u;
        if (head > c.count) head = c.count;
        const uint32_t body = (c.count - head) / 16u, tail = c.count - head - body * 16u;
        for (uint32_t i = tid; i < body; i += kThreads) {
            const uint4 v = *(const uint4*)(p + head + (size_t)i * 16u);
            bad = bad || bad_word(v.x, c.kind, c.limit) || bad_word(v.y, c.kind, c.limit) ||
                  bad_word(v.z, c.kind, c.limit) || bad_word(v.w, c.kind, c.limit);
        }
        if (tid < head / es) bad = bad || bad_elem(p + tid * es, c.kind, c.limit);
        if (tid >= 64u && tid - 64u < tail / es) bad = bad || bad_elem(p + head + (size_t)body * 16u + (tid - 64u) * es, c.kind, c.limit);
    } else {
        for (uint32_t i = tid; i < c.count; i += kThreads) {
            const char* e = p + (size_t)i * c.stride;
            bad = bad || bad_elem(e, c.kind, c.limit);
            if (c.kind == kF32) bad = bad || bad_elem(e + 4, kF32, 0) || bad_elem(e + 8, kF32, 0);
        }
    }
    if (__ballot(bad) && (tid & 63u) == 0) atomicOr(&h->scan, c.kind == kF32 ? kScanNonFinite : kScanIndexRange);
}

// items[j], boxes[j] and mat[j] of the triangles of tile blockIdx.x: tiles[] = (draw, first
// triangle within the draw).  queue / h->n_nan: as ti_items'.  An index out of range reads
// no vertex (gf_scan reports it and the scene's items are discarded).
__global__ __launch_bounds__(kThreads) void gf_items(const char* blob, const GltfDraw* draws, const uint2* tiles,
                                                     ulonglong2* items, ulonglong2* boxes, uint32_t* mat,
                                                     uint32_t* queue, ItemsHeader* h) {
    __shared__ u64 s[kTile * kStride];
    const uint2 tl = tiles[blockIdx.x];
    const GltfDraw& d = draws[__builtin_amdgcn_readfirstlane(tl.x)];  // block-uniform: the matrices are read once
    const uint32_t t0 = __builtin_amdgcn_readfirstlane(tl.y), tid = threadIdx.x;
    const uint32_t cnt = d.n_tris - t0 < kTile ? d.n_tris - t0 : kTile;
    const uint32_t j0 = d.first_tri + t0;

    if (tid < cnt * 3) {  // lane (triangle, corner): its index, its vertex, the transforms, into the item's slot
        const uint32_t corner = tid % 3;
        uint32_t v = t0 * 3 + tid;  // < 3 * 2^30
        const char* ip = blob + d.idx_off + (size_t)v * d.idx_stride;  // consecutive lanes, consecutive indices
        if (d.idx_width == 2) v = *(const uint16_t*)ip;
        else if (d.idx_width == 4) v = *(const uint32_t*)ip;
        float px = 0.f, py = 0.f, pz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
        if (v < d.n_verts) {
            const float* pp = (const float*)(blob + d.pos_off + (size_t)v * d.pos_stride);
            const float* np = (const float*)(blob + d.nrm_off + (size_t)v * d.nrm_stride);
            px = pp[0]; py = pp[1]; pz = pp[2];
            nx = np[0]; ny = np[1]; nz = np[2];
        }
        u64* it = s + tid / 3 * kStride;
        put3(it + (corner ? kWB + 3 * (corner - 1) : 0), gltf_point(d.m, px, py, pz));  // a | b, c
        put3(it + kWNa + 3 * corner, gltf_normal(d.cof, nx, ny, nz));                   // na, nb, nc
    }
    __syncthreads();

    if (tid < 64) {  // wave 0: lane t computes triangle j0 + t in its slot
        bool bad = false;
        if (tid < cnt) {
            u64* it = s + tid * kStride;
            gltf_item_in_slot(it);
            it[kItemWords - 1] = 0;                             // TriItem's tail padding
            it[kWMatGid] = (u64)d.mid | (u64)(j0 + tid) << 32;  // mat | gid: glTF has no shapes, so gid = j
            bad = item_has_nan(it);
            mat[j0 + tid] = d.mid;  // the light scan's input
        }
        queue_bad(bad, j0 + tid, queue, h);
    }
    __syncthreads();
    store_tile(s, j0, cnt, items, boxes);
}

inline uint32_t blocks(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

// One accessor of a draw as gf_scan's chunks
void scan_chunks(std::vector<ScanChunk>& out, uint64_t off, uint32_t stride, uint32_t count, uint32_t width,
                 uint32_t kind, uint32_t limit) {
    if (stride == width) {
        const uint64_t bytes = (uint64_t)count * width;
        for (uint64_t at = 0; at < bytes; at += kScanBytes)
            out.push_back({off + at, (uint32_t)(bytes - at < kScanBytes ? bytes - at : kScanBytes), 0u, kind, limit});
    } else {
        for (uint32_t at = 0; at < count; at += kScanElems)
            out.push_back({off + (uint64_t)at * stride, count - at < kScanElems ? count - at : kScanElems, stride, kind, limit});
    }
}

void parsed_item_of(const void* ctx, uint32_t j, TriItem& it) { gltf_item_of(*(const rt_parsed_scene*)ctx, j, it); }

}  // namespace

int emit_tri_bvhs_device_meshes(const rt_parsed_scene& ps, uint32_t max_levels, HostBvhArrays& tris, HostBvhArrays& ltris,
                                TriItemsOutcome& res, std::string& err) {
    res = TriItemsOutcome{};
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        err = "no HIP device visible (the device builder needs one)";
        return kDeviceBuildError;
    }
    if (ps.n_plan_tris == 0 || ps.n_plan_tris > kMaxPrims) return kDeviceBuildFallback;
    const uint32_t n = (uint32_t)ps.n_plan_tris;
    const hipStream_t st = 0;
    Arena m;
    RT_EMIT_MARK_START();

    // the blob: each referenced buffer once, at a 256-byte boundary; the draws rebased to it
    std::vector<uint64_t> base(ps.bufs.size());
    uint64_t blob_bytes = 0;
    for (size_t b = 0; b < ps.bufs.size(); ++b) {
        base[b] = blob_bytes;
        blob_bytes += (ps.bufs[b].size() + 255u) & ~(uint64_t)255u;
    }
    std::vector<GltfDraw> draws = ps.draws;
    std::vector<uint2> tile_of;
    std::vector<ScanChunk> chunks;
    tile_of.reserve(n / kTile + draws.size());
    for (uint32_t k = 0; k < draws.size(); ++k) {
        GltfDraw& d = draws[k];
        d.pos_off += base[d.pos_buf];
        d.nrm_off += base[d.nrm_buf];
        if (d.idx_width) d.idx_off += base[d.idx_buf];
        for (uint32_t t0 = 0; t0 < d.n_tris; t0 += kTile) tile_of.push_back(make_uint2(k, t0));
        scan_chunks(chunks, d.pos_off, d.pos_stride, d.n_verts, 12, kF32, 0);
        if (d.idx_width) scan_chunks(chunks, d.idx_off, d.idx_stride, d.n_idx, d.idx_width, d.idx_width == 2 ? kU16 : kU32, d.n_verts);
    }
    std::vector<uint8_t> light(ps.mats.size());
    for (size_t i = 0; i < ps.mats.size(); ++i) {
        const double* e = ps.mats[i].emission;
        light[i] = e[0] != 0.0 || e[1] != 0.0 || e[2] != 0.0;  // scene_build.cpp is_light
    }

    char* d_blob = m.get<char>(blob_bytes);
    GltfDraw* d_draws = m.get<GltfDraw>(draws.size());
    uint2* d_tiles = m.get<uint2>(tile_of.size());
    ScanChunk* d_chunks = m.get<ScanChunk>(chunks.size());
    uint8_t* d_light = m.get<uint8_t>(light.size());
    uint32_t* d_mat = m.get<uint32_t>(n);
    TriItem* d_items = m.get<TriItem>(n);
    double* d_boxes = m.get<double>((size_t)n * 6);
    uint32_t* d_queue = m.get<uint32_t>(kFixCap);
    ItemsHeader* d_hdr = m.get<ItemsHeader>(1);
    TI_SCRATCH_OK();
    for (size_t b = 0; b < ps.bufs.size(); ++b)
        if (!ps.bufs[b].empty())
            TI_TRY(hipMemcpyAsync(d_blob + base[b], ps.bufs[b].data(), ps.bufs[b].size(), hipMemcpyHostToDevice, st));
    TI_TRY(hipMemcpyAsync(d_draws, draws.data(), draws.size() * sizeof(GltfDraw), hipMemcpyHostToDevice, st));
    TI_TRY(hipMemcpyAsync(d_tiles, tile_of.data(), tile_of.size() * sizeof(uint2), hipMemcpyHostToDevice, st));
    if (!chunks.empty())
        TI_TRY(hipMemcpyAsync(d_chunks, chunks.data(), chunks.size() * sizeof(ScanChunk), hipMemcpyHostToDevice, st));
    TI_TRY(hipMemcpyAsync(d_light, light.data(), light.size(), hipMemcpyHostToDevice, st));
    RT_EMIT_MARK("blob upload");

    items_header_clear(d_hdr, st);
    if (!chunks.empty()) gf_scan<<<(uint32_t)chunks.size(), kThreads, 0, st>>>(d_blob, d_chunks, d_hdr);
    TI_TRY(hipGetLastError());
    RT_EMIT_MARK("gf_scan");
    gf_items<<<(uint32_t)tile_of.size(), kThreads, 0, st>>>(d_blob, d_draws, d_tiles, (ulonglong2*)d_items,
                                                            (ulonglong2*)d_boxes, d_mat, d_queue, d_hdr);
    TI_TRY(hipGetLastError());
    RT_EMIT_MARK("gf_items");
    void* const inputs[4] = {d_blob, d_draws, d_tiles, d_chunks};
    return finish_device_items(m, n, d_items, d_boxes, d_mat, d_light, d_queue, d_hdr, inputs, 4, parsed_item_of, &ps,
                               max_levels, tris, ltris, res, err);
}

}  // namespace rt

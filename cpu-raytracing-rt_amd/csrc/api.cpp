// api.cpp — the C ABI (include/rt_api.h): scene upload, frame render, tile
// partition, ray queries.  Replaces generate_image (main.rs:85-114) and the
// scene construction behind it (scene.rs:180-223).  Errors become return codes
// (the reference panics).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rt_api.h"
#include "api_internal.h"
#include "render.h"
#include "rt_device.h"
#include "scene_build.h"

namespace rt {

static thread_local std::string g_last_error;

int set_error(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

}  // namespace rt

using namespace rt;

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return set_error(e_ == hipErrorOutOfMemory ? RT_ERR_NOMEM : RT_ERR_DEVICE,        \
                             std::string(#expr) + ": " + hipGetErrorString(e_));              \
    } while (0)

struct rt_scene {
    int device = 0;
    DevScene dev{};
    std::vector<void*> allocs;
    std::vector<size_t> alloc_bytes;  // bytes of each scene array in allocs (scene_allocs: replicas)
    rt_scene_info info{};
    // spill workspace for the traversal stack (grown on demand)
    uint32_t* spill_n = nullptr;
    double* spill_t = nullptr;
    size_t spill_entries = 0;
    // chunk partial sums (KParams::chunks > 1), grown on demand
    double* part = nullptr;
    size_t part_entries = 0;
    // the second partials of a moments frame (rt_render_moments), the same shape, only once one needs them
    double* part_sq = nullptr;
    size_t part_sq_entries = 0;
    // persistent path kernel: wave-tile queue and per-wave sample ring
    uint32_t* queue = nullptr;
    double* ring = nullptr;
    size_t ring_entries = 0;
    // rows of the queue's split tail wave-tiles (KParams::rows), grown on demand
    double* rows = nullptr;
    size_t rows_entries = 0;
    // rt_render_adaptive's state (rt_adaptive_workspace_bytes), grown on demand
    void* adaptive = nullptr;
    size_t adaptive_bytes = 0;
    unsigned long long* d_stats = nullptr;
    // the path kernel reads the scene record and the frame constants by pointer
    DevScene* d_scene = nullptr;
    KParams* d_params = nullptr;
    // Completion of the last launch that used the workspace above (queue, ring,
    // partials, spill, d_params).  Each workspace-using launch first makes its
    // stream wait on it, then re-records it, so calls issued on different
    // streams never overlap on the shared workspace.
    hipEvent_t ws_done = nullptr;
    // bytes of the triangle BVH's compact layout (nodes + leaf blocks), 0 without one
    uint64_t compact_bytes = 0;
    uint64_t pair_bytes = 0;  // the pair layout's lines + the compact leaf blocks, 0 without one
    // requested kernel form (rt_scene_set_tuning); auto fields resolve per scene
    rt_tuning tune{0, -1, 0, 0, 0, 0, -1, 0};
    uint32_t last_tail_split = 0;  // the split the last prepared frame resolved to (0: none since set_tuning)
};

namespace {

// Set while scene_upload builds a replica (multi.cpp): the arrays are allocated
// but not copied from the host; the caller fills them device to device from the
// source scene's arrays (the same build, so the same allocation sequence).
thread_local bool g_replica = false;

template <class T>
int upload(rt_scene* s, const std::vector<T>& v, const T** out) {
    *out = nullptr;
    if (v.empty()) return RT_OK;
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, v.size() * sizeof(T)));
    s->allocs.push_back(p);
    s->alloc_bytes.push_back(v.size() * sizeof(T));
    if (!g_replica) HIP_TRY(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    s->info.device_bytes += v.size() * sizeof(T);
    *out = (const T*)p;
    return RT_OK;
}

// Array k of a BVH: uploaded from its host vector, or, where bvh_emit.hip already wrote it
// on the device (h.dev.on), adopted as it is — the same entry in allocs / alloc_bytes /
// device_bytes as the upload would make, so the checksum and replicas see one sequence.
template <class T>
int upload(rt_scene* s, const HostBvhArrays& h, int k, const std::vector<T>& v, const T** out) {
    if (!h.dev.on) return upload(s, v, out);
    *out = nullptr;
    if (!h.dev.ptr[k]) return RT_OK;
    if (g_replica) return set_error(RT_ERR_INVALID, "a replica cannot adopt device-emitted arrays");
    s->allocs.push_back(h.dev.ptr[k]);  // from here on the scene frees it
    s->alloc_bytes.push_back(h.dev.count[k] * sizeof(T));
    s->info.device_bytes += h.dev.count[k] * sizeof(T);
    *out = (const T*)h.dev.ptr[k];
    h.dev.ptr[k] = nullptr;
    return RT_OK;
}

int upload_bvh(rt_scene* s, const HostBvhArrays& h, DevBvh& d) {
    int rc;
    std::memset(&d, 0, sizeof(d));
    if ((rc = upload(s, h, kResNodes, h.nodes, &d.nodes))) return rc;
    store3(d.root_min, h.root.min);
    store3(d.root_max, h.root.max);
    d.n_prims = h.n_prims;
    d.depth = h.depth;
    d.fast = h.fast ? 1u : 0u;
    d.tri_q = h.tri_q ? 1u : 0u;
    if ((rc = upload(s, h.shapes, &d.shapes))) return rc;
    if ((rc = upload(s, h, kResTris, h.tris, &d.tris))) return rc;
    if ((rc = upload(s, h, kResCold, h.tri_cold, &d.tri_cold))) return rc;
    if ((rc = upload(s, h, kResInvArea, h.tri_inv_area, &d.tri_inv_area))) return rc;
    if ((rc = upload(s, h, kResMat, h.mat, &d.mat))) return rc;
    if ((rc = upload(s, h, kResGid, h.gid, &d.gid))) return rc;
    if ((rc = upload(s, h, kResCnodes, h.cnodes, &d.cnodes))) return rc;
    if ((rc = upload(s, h, kResCtris, h.ctris, &d.ctris))) return rc;
    if ((rc = upload(s, h, kResPnodes, h.pnodes, &d.pnodes))) return rc;
    return RT_OK;
}

void free_scene(rt_scene* s) {
    if (!s) return;
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(s->device);
    for (void* p : s->allocs) (void)hipFree(p);
    if (s->spill_n) (void)hipFree(s->spill_n);
    if (s->spill_t) (void)hipFree(s->spill_t);
    if (s->part) (void)hipFree(s->part);
    if (s->part_sq) (void)hipFree(s->part_sq);
    if (s->queue) (void)hipFree(s->queue);
    if (s->ring) (void)hipFree(s->ring);
    if (s->rows) (void)hipFree(s->rows);
    if (s->adaptive) (void)hipFree(s->adaptive);
    if (s->d_stats) (void)hipFree(s->d_stats);
    if (s->d_scene) (void)hipFree(s->d_scene);
    if (s->d_params) (void)hipFree(s->d_params);
    if (s->ws_done) (void)hipEventDestroy(s->ws_done);
    (void)hipSetDevice(cur);
    delete s;
}

struct SceneDeleter {
    void operator()(rt_scene* s) const { free_scene(s); }
};

// Makes the scene's device current for one entry point and restores the
// caller's current device on every return path.
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) err = hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};
#define DEVICE_GUARD(s)                                                                       \
    DeviceGuard guard_((s)->device);                                                          \
    if (guard_.err != hipSuccess)                                                             \
        return set_error(RT_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(guard_.err))

struct EventPair {  // hipEvent_t pair destroyed on every return path
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};

// Stream ordering of the shared workspace: wait for the previous user, launch,
// then record (ws_begin / ws_end bracket every workspace-using launch).
hipError_t ws_begin(rt_scene* s, hipStream_t st) { return hipStreamWaitEvent(st, s->ws_done, 0); }
hipError_t ws_end(rt_scene* s, hipStream_t st) { return hipEventRecord(s->ws_done, st); }

int check_params(const rt_render_params* p) {
    if (!p) return set_error(RT_ERR_INVALID, "params is NULL");
    if (p->width == 0 || p->height == 0) return set_error(RT_ERR_INVALID, "width/height must be > 0");
    // the path kernel packs a wave-tile's pixel origin into 16 + 16 bits (render.hip store_unit)
    if (p->width > 65535 || p->height > 65535) return set_error(RT_ERR_INVALID, "width/height must be <= 65535");
    if (p->spp == 0) return set_error(RT_ERR_INVALID, "spp must be > 0");
    if (p->ray_depth > 255) return set_error(RT_ERR_INVALID, "ray_depth is a u8 in the reference (scene.rs:85)");
    if (p->fov_axis != RT_FOV_X && p->fov_axis != RT_FOV_Y) return set_error(RT_ERR_INVALID, "bad fov_axis");
    return RT_OK;
}

// Sample chunking of a frame (render.h sample_chunks); a scene's tuning may
// force the run length (rt_tuning.chunk_spp, tests and tuning experiments;
// rt_scene_sample_chunks reports it, so checkers stay consistent).  A forced run
// length is raised, if need be, to keep the frame's rule's limits: at most
// kMaxChunks runs, and the chunk partial sums within kPartBytes.
void frame_chunks(const rt_render_params* p, uint32_t force_spp, uint32_t& chunks, uint32_t& chunk_spp) {
    sample_chunks(p->width, p->height, p->spp, chunks, chunk_spp);
    if (force_spp > 0) {
        const uint64_t chunk_bytes =
            (uint64_t)((p->width + 15) / 16) * ((p->height + 15) / 16) * 256 * 3 * sizeof(double);
        const uint64_t max_chunks = std::max<uint64_t>(1, std::min<uint64_t>(kMaxChunks, kPartBytes / chunk_bytes));
        const uint32_t floor_spp = (uint32_t)((p->spp + max_chunks - 1) / max_chunks);
        chunk_spp = std::min(std::max(force_spp, floor_spp), p->spp);
        chunks = (p->spp + chunk_spp - 1) / chunk_spp;
    }
}

// Camera::new (camera.rs:17-46) on the host + the tile map of one rank.
KParams make_kparams(const rt_render_params* p, uint32_t rank, uint32_t world, uint32_t force_spp = 0) {
    KParams k;
    std::memset(&k, 0, sizeof(k));
    k.width = p->width; k.height = p->height; k.spp = p->spp; k.ray_depth = p->ray_depth;
    k.fw = (double)p->width; k.fh = (double)p->height;
    k.inv_fw = 1.0 / k.fw; k.inv_fh = 1.0 / k.fh;
    if (p->fov_axis == RT_FOV_Y) {
        k.tan_y = std::tan(p->fov / 2.0);
        double aspect = k.fh / k.fw;
        k.tan_x = k.tan_y / aspect;
    } else {
        k.tan_x = std::tan(p->fov / 2.0);
        double aspect = k.fw / k.fh;
        k.tan_y = k.tan_x / aspect;
    }
    for (int i = 0; i < 3; ++i) {
        k.cam_pos[i] = p->cam_position[i]; k.cam_right[i] = p->cam_right[i];
        k.cam_up[i] = p->cam_up[i]; k.cam_fwd[i] = p->cam_forward[i]; k.bg[i] = p->bg_color[i];
    }
    k.scale01 = inclusive_scale(0.0, 1.0);
    k.scale11 = inclusive_scale(-1.0, 1.0);
    k.seed = p->seed;
    k.rank = rank; k.world = world;
    k.tiles_x = (p->width + RT_TILE - 1) / RT_TILE;
    k.tiles_y = (p->height + RT_TILE - 1) / RT_TILE;
    k.n_tiles = (uint64_t)k.tiles_x * k.tiles_y;
    k.n_slots = (uint32_t)((k.n_tiles + world - 1) / world);
    frame_chunks(p, force_spp, k.chunks, k.chunk_spp);
    return k;
}

uint32_t slots_per_rank(const KParams& k) { return k.n_slots; }

// Before a workspace buffer is regrown: the last launch that used it is done.
int ws_idle(rt_scene* s) {
    HIP_TRY(hipEventSynchronize(s->ws_done));
    return RT_OK;
}

// part / part_entries: the scene's chunk partials, or its second ones (a moments frame);
// always: an adaptive pass, whose single run goes to the partials too
int ensure_part(rt_scene* s, const KParams& k, double*& part, size_t& part_entries, bool always = false) {
    if (k.chunks == 1 && !always) return RT_OK;
    const size_t need = (size_t)k.n_slots * k.chunks * 256 * 3;
    if (need <= part_entries) return RT_OK;
    if (int rc = ws_idle(s)) return rc;
    if (part) (void)hipFree(part);
    part = nullptr; part_entries = 0;
    HIP_TRY(hipMalloc(&part, need * sizeof(double)));
    part_entries = need;
    return RT_OK;
}

// Spill area for stack entries beyond the LDS short stack: depth bound of the
// deepest BVH, one slot per launched lane (`no_lds`: a kernel without an LDS
// stack, the 4/5-wave shape-only fused kernel, spills every entry).
int ensure_spill(rt_scene* s, uint64_t lanes, bool no_lds = false) {
    uint32_t depth = s->dev.max_depth;
    const uint32_t lds = no_lds ? 0u : (uint32_t)kMinShort;
    if (depth <= lds) return RT_OK;
    size_t need = (size_t)(depth - lds) * lanes;
    if (need <= s->spill_entries) return RT_OK;
    if (int rc = ws_idle(s)) return rc;
    if (s->spill_n) (void)hipFree(s->spill_n);
    if (s->spill_t) (void)hipFree(s->spill_t);
    s->spill_n = nullptr; s->spill_t = nullptr; s->spill_entries = 0;
    HIP_TRY(hipMalloc(&s->spill_n, need * sizeof(uint32_t)));
    HIP_TRY(hipMalloc(&s->spill_t, need * sizeof(double)));
    s->spill_entries = need;
    return RT_OK;
}

// Register budget of the path kernel for this scene.  Large BVHs make the loop
// latency-bound on dependent node loads, where a 4th wave per SIMD hides more
// than its register spill costs (C3: -9%).  Shape-only scenes with small shape
// BVHs run the fused kernel's shape-only instance at kShapeWaves (round 4: the
// path's T and L in LDS and no LDS stack take it to 128 VGPRs without spill, and
// a 5th wave hides more than its 42 VGPRs of spill cost).  That
// instance has no LDS stack: every push of a BVH walk goes to the global spill
// stack, which a single-leaf BVH (the Cornell box's) never touches; so a
// shape-only scene whose BVHs hold more than kShapeWavesNodes nodes runs the
// 3-wave instance, whose 12-entry LDS stack takes the pushes (round 5, advisor
// finding; measured in DESIGN.md §4).  Other small scenes run the general fused
// instance at 3.  rt_tuning.waves forces one (tests, tuning); 5 exists for the
// shape-only fused form only (other forms take 4).
bool path_resume(const rt_scene* s);
int path_kinds(const rt_scene* s);
uint32_t path_waves(const rt_scene* s) {
    const bool shape_fused = path_kinds(s) == 1 && !path_resume(s);
    if (s->tune.waves) return s->tune.waves == 5 && !shape_fused ? 4u : s->tune.waves;
    uint64_t nodes = 0;
    for (int k = 0; k < 6; ++k) nodes += s->info.bvh_nodes[k];
    if (shape_fused) return nodes <= kShapeWavesNodes ? kShapeWaves : 3u;
    return nodes > kDeepSceneNodes ? 4u : 3u;
}

// Resumable triangle traversal (path_kernel RES) for scenes with a
// deep triangle BVH, where a wave's traversal loop otherwise runs most trips
// with few live lanes (C3: 43%); scenes without one keep the fused segment,
// which carries less state across the loop (C2: 113 vs 130 ms at 64 spp).
// rt_tuning.resume forces one (tests, tuning).
bool path_resume(const rt_scene* s) {
    if (s->tune.resume >= 0) return s->tune.resume == 1;
    return s->info.bvh_nodes[2] > kDeepSceneNodes;
}

// The scene's primitive kinds: 1 = shapes (planes, boxes, ellipsoids), 2 =
// triangles, 3 = both (or neither).  One-kind scenes run kernel instances with no
// code or state for the other kind: triangle-only ones (every glTF scene) the
// 4-wave resumable kernel without a shape candidate carried across its loop
// (C3 -6%), shape-only ones (the Cornell box) the fused kernel without triangle
// traversal.  rt_tuning.kinds = 3 forces the general instances (tests, tuning).
int scene_kinds(const DevScene& d) {
    const bool shapes = d.n_planes || d.boxes.n_prims || d.ells.n_prims || d.lboxes.n_prims || d.lells.n_prims;
    const bool tris = d.tris.n_prims || d.ltris.n_prims;
    return shapes == tris ? 3 : (shapes ? 1 : 2);
}
int path_kinds(const rt_scene* s) { return s->tune.kinds == 3 ? 3 : scene_kinds(s->dev); }

// The triangle BVH's compact layout (rt_layout.h DevNodeC, half the bytes per
// node visit and triangle test, the same numbers): used by the triangle-only
// 4-wave resumable instance — the kernel of every deep glTF scene — whenever the
// host could build it (every coordinate an exact f32).  rt_tuning.compact = 0
// keeps the f64 layout (tests run both).
bool path_compact(const rt_scene* s) {
    return s->tune.compact != 0 && s->dev.tris.cnodes && path_waves(s) == 4 && path_resume(s) && path_kinds(s) == 2;
}
// The pair layout over the compact nodes (rt_layout.h kPairFloats, render.hip trav_step
// PAIR: two BVH levels per dependent line), whenever the scene has it (auto, or
// rt_tuning.compact = 2; 1 forces the 64-B compact nodes): C3 -3.5%, C5 -2.0% in
// alternating runs, the same images and counters (profiles/r06/variants_pair2_C*.log,
// DESIGN.md §4).
bool path_pairs(const rt_scene* s) {
    return (s->tune.compact == -1 || s->tune.compact == 2) && s->dev.tris.pnodes && path_compact(s);
}



// Suspend threshold of the resumable traversal (render.h kSuspendCached /
// kSuspendStreamed): by whether the triangle BVH and its hot records fit the
// Infinity Cache.  rt_tuning.suspend_lanes forces one (tuning).
// The triangle BVH and its hot records exceed the Infinity Cache, sized by the
// layout the kernel reads (path_compact: 64-B nodes and 36-B records, else 128 B
// and 80 B).
uint64_t bvh_hot_bytes(const rt_scene* s) {
    if (path_pairs(s)) return s->pair_bytes;
    if (path_compact(s)) return s->compact_bytes;
    return s->info.bvh_nodes[2] * sizeof(DevNode) + s->info.n_triangles * sizeof(DevTri);
}
bool bvh_streamed(const rt_scene* s) { return bvh_hot_bytes(s) > kCacheBytes; }
uint32_t path_suspend(const rt_scene* s) {
    if (s->tune.suspend_lanes) return s->tune.suspend_lanes;
    if (path_compact(s)) return bvh_streamed(s) ? kSuspendCoopStreamed : kSuspendCoopCached;  // leaf_coop
    return bvh_streamed(s) ? kSuspendStreamed : kSuspendCached;
}

// Leaf batch of the resumable traversal (render.hip trav_step: lanes waiting at
// leaves before the wave tests them), by the same cache criterion as the suspend
// threshold (render.h kLeafCached / kLeafStreamed; the compact layout's kernel, whose
// small leaves are tested cooperatively, kLeafCoop*).  rt_tuning.leaf_lanes forces one.
uint32_t path_leaf_batch(const rt_scene* s) {
    if (s->tune.leaf_lanes) return s->tune.leaf_lanes;
    if (path_compact(s)) return bvh_streamed(s) ? kLeafCoopStreamed : kLeafCoopCached;
    return bvh_streamed(s) ? kLeafStreamed : kLeafCached;
}

// Workspace of one path-kernel launch: persistent grid size, then the spill,
// ring and chunk-partial buffers sized for it (all grow-only, scene-owned).
// moments: the frame of rt_render_moments (path_kernel MOM: no stats, no hit ids), whose
// second partials are sized like the first.  An adaptive pass (sums) is sized by its list:
// k.n_slots is the list's length, and the queue, the grid and the tail split follow from it.
int prepare_path(rt_scene* s, KParams& k, bool stats, bool hits, PathWork& W, bool moments = false, bool sums = false) {
    k.suspend = path_suspend(s);
    k.leaf_batch = path_leaf_batch(s);
    const uint64_t n_units = (uint64_t)k.n_slots * k.chunks * 4;
    if (n_units >= (1ull << 31)) return set_error(RT_ERR_INVALID, "frame too large for one launch");
    std::memset(&W, 0, sizeof(W));
    W.waves = path_waves(s);
    W.resume = path_resume(s);
    W.kinds = path_pairs(s) ? kKindsPair : (path_compact(s) ? kKindsCompact : path_kinds(s));
    HIP_TRY(path_grid(stats, hits, W.waves, W.resume, W.kinds, (uint32_t)n_units, &W.grid, moments));
    const uint64_t lanes = (uint64_t)W.grid * 64u;
    int rc;
    // the 4/5-wave shape-only fused kernel has no LDS stack
    const bool no_lds = W.waves >= 4 && !W.resume && W.kinds == 1;
    if ((rc = ensure_spill(s, lanes, no_lds)) || (rc = ensure_part(s, k, s->part, s->part_entries, sums))) return rc;
    if (moments && (rc = ensure_part(s, k, s->part_sq, s->part_sq_entries, sums))) return rc;
    if (!s->queue) HIP_TRY(hipMalloc(&s->queue, kQueueWords * sizeof(uint32_t)));
    const size_t ring_need = (size_t)W.grid * kRingRows * 64 * 3;
    if (ring_need > s->ring_entries) {
        if (int rc2 = ws_idle(s)) return rc2;
        if (s->ring) (void)hipFree(s->ring);
        s->ring = nullptr; s->ring_entries = 0;
        HIP_TRY(hipMalloc(&s->ring, ring_need * sizeof(double)));
        s->ring_entries = ring_need;
    }
    // The queue's tail (render.hip queue_entry): the last wave-tiles —
    // kTailPerWave per resident wave, so a wave that took the last whole one finishes it
    // while the others still take parts — handed out in kTailSplit parts, so the launch
    // does not wait a whole wave-tile's time for the waves that took the last ones.
    // Capped at 256 MB of row buffer; rt_tuning.tail_split forces the split (1: whole
    // wave-tiles).
    const uint32_t split = s->tune.tail_split ? s->tune.tail_split : kTailSplit;
    uint64_t tail = 0;
    if (split > 1 && k.chunk_spp < (1u << 16)) {
        const uint64_t per_unit = (uint64_t)k.chunk_spp * 64 * 3;  // doubles
        tail = std::min<uint64_t>({n_units, (uint64_t)W.grid * kTailPerWave, (kTailRowBytes / 8) / per_unit});
        if (tail * per_unit > s->rows_entries) {
            if (int rc2 = ws_idle(s)) return rc2;
            if (s->rows) (void)hipFree(s->rows);
            s->rows = nullptr; s->rows_entries = 0;
            HIP_TRY(hipMalloc(&s->rows, tail * per_unit * sizeof(double)));
            s->rows_entries = tail * per_unit;
        }
    }
    k.n_tail = (uint32_t)tail;
    k.tail_split = tail ? split : 1u;
    s->last_tail_split = k.tail_split;  // rt_scene_get_tuning reports what the frame resolved to
    k.rows = s->rows;
    W.queue = s->queue; W.ring = s->ring; W.part = s->part; W.part_sq = s->part_sq;
    W.d_scene = s->d_scene; W.d_params = s->d_params;
    W.spill_n = s->spill_n; W.spill_t = s->spill_t;
    return RT_OK;
}

// Scratch of rt_error_estimate_async: se_kernel's per-block partials (render.h kSeMaxBlocks
// x 8 doubles, 64 KiB).  A fixed pool of kSeSlots per device, handed out round-robin under
// g_se_mutex; a slot carries the event of its last user, which the next user's stream
// waits for, so calls on any number of streams never work in one slot at a time.  Made on
// first use, kept for the life of the process.
constexpr unsigned kSeSlots = 8;
struct SeSlot {
    double* part = nullptr;
    hipEvent_t done = nullptr;
};
struct SePool {
    SeSlot slots[kSeSlots];
    unsigned next = 0;
};
std::mutex g_se_mutex;
std::map<int, SePool> g_se_pools;  // by device
int se_slot_take(hipStream_t st, SeSlot** out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    SePool& pool = g_se_pools[dev];
    SeSlot& sl = pool.slots[pool.next++ % kSeSlots];
    if (!sl.part) HIP_TRY(hipMalloc(&sl.part, (size_t)kSeMaxBlocks * 8 * sizeof(double)));
    if (!sl.done) HIP_TRY(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    else HIP_TRY(hipStreamWaitEvent(st, sl.done, 0));
    *out = &sl;
    return RT_OK;
}

// device counters (render.hip wave_flush order) -> rt_stats (timings untouched)
int copy_stats(rt_scene* s, rt_stats* out) {
    unsigned long long c[kStatStall + 1];
    HIP_TRY(hipMemcpy(c, s->d_stats, sizeof(c), hipMemcpyDeviceToHost));
    // the stats instance's progress guard (render.h kStatStall): a wave that looped
    // without progress exited early, so the frame is incomplete — fail loudly
    if (c[kStatStall])
        return set_error(RT_ERR_DEVICE, "path kernel: " + std::to_string(c[kStatStall]) + " wave(s) made no progress "
                                        "for " + std::to_string(kStallTrips) + " loop trips (livelock guard)");
    out->paths = c[0]; out->segments = c[1]; out->aabb_tests = c[2]; out->tri_tests = c[3];
    out->shape_tests = c[4]; out->shaded_hits = c[5]; out->light_queries = c[6]; out->light_hits = c[7];
    out->lane_steps = c[8]; out->wave_steps = c[9];
    return RT_OK;
}

// DevScene::slt_mask: the scene boxes (BVH order) that are the light boxes, in
// order, when the light pdf can come from the closest-hit box tests (render.hip
// boxes_slt): only box lights, both box BVHs single leaves (bvh.rs:77), and the
// light copies (scene.rs:209-213) byte-identical to the selected scene records.
uint32_t slt_mask(const HostScene& hs) {
    const auto &B = hs.bvh[0], &L = hs.bvh[3];
    if (L.shapes.empty() || !hs.bvh[4].shapes.empty() || hs.bvh[5].n_prims) return 0;
    if (B.depth != 1 || L.depth != 1 || B.shapes.size() > 32) return 0;
    uint32_t mask = 0;
    size_t j = 0;
    for (size_t i = 0; i < B.shapes.size() && j < L.shapes.size(); ++i)
        if (std::memcmp(&B.shapes[i], &L.shapes[j], sizeof(DevShape)) == 0) { mask |= 1u << i; ++j; }
    return j == L.shapes.size() ? mask : 0;
}

// DevScene::lq_boxes / lq_box: the light boxes' world-space bounds, grown by a
// margin of 1e-6 of the coordinates' magnitude (+1e-100) that dwarfs the rounding
// of the model-space map and of the query's slab arithmetic.  model_ray maps a
// world point p to M (p - pos) with M = x -> rotate(conj(rot), x), cgmath's
// rotate_vector: for a quaternion of norm n = |rot|^2 that is n R^T + (1 - n) I,
// a rotation only when n == 1 (the parser, like the reference, does not
// normalise ROTATION).  The box surface is therefore pos + M^-1 (+-half sizes):
// the eight corners come through the inverse of M, built from rotate() on the
// basis vectors and inverted here.  Zero (no skipping) unless every light is a
// box, there are at most kLqBoxes, every box and density is finite and positive,
// and M is well conditioned (n within 10% of 1, the inverse checked).
uint32_t lq_boxes(const HostScene& hs, double (*out)[6]) {
    const auto& L = hs.bvh[3].shapes;
    if (L.empty() || L.size() > kLqBoxes || !hs.bvh[4].shapes.empty() || hs.bvh[5].n_prims) return 0;
    for (size_t i = 0; i < L.size(); ++i) {
        const DevShape& b = L[i];
        const double pb = b.aux[0];
        if (!(pb > 0.0) || !std::isfinite(pb)) return 0;
        const Quat q = load_quat(b.rot);
        const double n = q.s * q.s + dot(q.v, q.v);
        if (!(std::fabs(n - 1.0) <= 0.1)) return 0;
        const Quat c = conjugate(q);
        double M[3][3], Mi[3][3];
        for (int k = 0; k < 3; ++k) {  // column k = M e_k
            const V3 col = rotate(c, v3(k == 0, k == 1, k == 2));
            M[0][k] = col.x; M[1][k] = col.y; M[2][k] = col.z;
        }
        const double det = M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) -
                           M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
                           M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
        if (!(std::fabs(det) > 0.5)) return 0;
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) {  // adjugate / det
                const int r1 = (k + 1) % 3, r2 = (k + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
                Mi[r][k] = (M[r1][c1] * M[r2][c2] - M[r1][c2] * M[r2][c1]) / det;
            }
        for (int r = 0; r < 3; ++r)  // M Mi == I to 1e-12
            for (int k = 0; k < 3; ++k) {
                const double e = M[r][0] * Mi[0][k] + M[r][1] * Mi[1][k] + M[r][2] * Mi[2][k];
                if (!(std::fabs(e - (r == k ? 1.0 : 0.0)) <= 1e-12)) return 0;
            }
        V3 lo = v3(INFINITY, INFINITY, INFINITY), hi = v3(-INFINITY, -INFINITY, -INFINITY);
        for (int k = 0; k < 8; ++k) {
            const double h[3] = {(k & 1) ? b.shape[0] : -b.shape[0], (k & 2) ? b.shape[1] : -b.shape[1],
                                 (k & 4) ? b.shape[2] : -b.shape[2]};
            const V3 p = load3(b.pos) + v3(Mi[0][0] * h[0] + Mi[0][1] * h[1] + Mi[0][2] * h[2],
                                           Mi[1][0] * h[0] + Mi[1][1] * h[1] + Mi[1][2] * h[2],
                                           Mi[2][0] * h[0] + Mi[2][1] * h[1] + Mi[2][2] * h[2]);
            lo = v3(std::min(lo.x, p.x), std::min(lo.y, p.y), std::min(lo.z, p.z));
            hi = v3(std::max(hi.x, p.x), std::max(hi.y, p.y), std::max(hi.z, p.z));
        }
        const double mag = std::max({std::fabs(lo.x), std::fabs(lo.y), std::fabs(lo.z), std::fabs(hi.x),
                                     std::fabs(hi.y), std::fabs(hi.z)});
        if (!std::isfinite(mag) || mag > 0x1p400) return 0;
        const double m = 1e-6 * (1.0 + mag) + 1e-100;
        const double v[6] = {lo.x - m, lo.y - m, lo.z - m, hi.x + m, hi.y + m, hi.z + m};
        for (int k = 0; k < 6; ++k) out[i][k] = v[k];
    }
    return (uint32_t)L.size();
}

template <class T>
struct DevBuf {  // RAII device buffer for per-call scratch
    T* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc((void**)&p, (n ? n : 1) * sizeof(T)); }
};

}  // namespace

static int check_build_flags(uint32_t build_flags);

extern "C" {

const char* rt_last_error(void) { return g_last_error.c_str(); }
int rt_api_version(void) { return RT_API_VERSION; }
int rt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int rt_scene_create_ex(const rt_scene_desc* desc, uint32_t build_flags, rt_scene** out) {
    if (!desc || !out) return set_error(RT_ERR_INVALID, "desc/out is NULL");
    *out = nullptr;
    if (build_flags & RT_BUILD_DEVICE_MESHES)
        return set_error(RT_ERR_INVALID, "RT_BUILD_DEVICE_MESHES needs a deferred glTF parse (rt_scene_create_parsed): a description has no meshes");
    if (const int rc = check_build_flags(build_flags)) return rc;
    HostScene hs;
    const int rc = rt::scene_build_host(*desc, hs, build_flags);
    return rc ? rc : rt::scene_upload(hs, out, false);
}
int rt_scene_create(const rt_scene_desc* desc, rt_scene** out) { return rt_scene_create_ex(desc, 0, out); }

int rt_scene_create_parsed(rt_parsed_scene* ps, uint32_t build_flags, rt_scene** out) {
    if (!ps || !out) return set_error(RT_ERR_INVALID, "parsed scene/out is NULL");
    *out = nullptr;
    const uint32_t three = RT_BUILD_DEVICE | RT_BUILD_DEVICE_RECORDS | RT_BUILD_DEVICE_ITEMS;
    if ((build_flags & RT_BUILD_DEVICE_MESHES) && (build_flags & three) != three)
        return set_error(RT_ERR_INVALID, std::string("RT_BUILD_DEVICE_MESHES needs ") +
                                             (!(build_flags & RT_BUILD_DEVICE_ITEMS) ? "RT_BUILD_DEVICE_ITEMS"
                                              : !(build_flags & RT_BUILD_DEVICE_RECORDS) ? "RT_BUILD_DEVICE_RECORDS"
                                                                                         : "RT_BUILD_DEVICE") +
                                             " (the flattened meshes feed the device's items)");
    if (const int rc = check_build_flags(build_flags & ~RT_BUILD_DEVICE_MESHES)) return rc;
    HostScene hs;
    int rc;
    if ((build_flags & RT_BUILD_DEVICE_MESHES) && ps->deferred) {
        rc = rt::scene_build_parsed(*ps, hs, build_flags);
    } else {
        rt_scene_desc desc;
        if ((rc = rt_parsed_scene_get(ps, &desc, nullptr))) return rc;
        rc = rt::scene_build_host(desc, hs, build_flags & ~RT_BUILD_DEVICE_MESHES);
    }
    return rc ? rc : rt::scene_upload(hs, out, false);
}

}  // extern "C"

static int check_build_flags(uint32_t build_flags) {
    if (build_flags & ~(RT_BUILD_DEVICE | RT_BUILD_DEVICE_RECORDS | RT_BUILD_DEVICE_ITEMS))
        return set_error(RT_ERR_INVALID, "unknown build flag");
    if ((build_flags & RT_BUILD_DEVICE_ITEMS) && !(build_flags & RT_BUILD_DEVICE_RECORDS))
        return set_error(RT_ERR_INVALID, "RT_BUILD_DEVICE_ITEMS needs RT_BUILD_DEVICE_RECORDS (the items feed the device's record emission)");
    if ((build_flags & RT_BUILD_DEVICE_RECORDS) && !(build_flags & RT_BUILD_DEVICE))
        return set_error(RT_ERR_INVALID, "RT_BUILD_DEVICE_RECORDS needs RT_BUILD_DEVICE (the records come from the device's tree)");
    return RT_OK;
}

namespace rt {

static int tri_build_device(const std::vector<Box3>& boxes, HostBvh& out, std::string& err) {
    return build_bvh_device(boxes, 0, out, err);
}
static int tri_emit_device(const std::vector<TriItem>& items, bool compact, HostBvhArrays& out, std::string& err) {
    return emit_tri_bvh_device(items, compact, 0, out, err);
}

static int tri_items_device(const rt_scene_desc& desc, HostBvhArrays& tris, HostBvhArrays& ltris, TriItemsOutcome& res,
                            std::string& err) {
    return emit_tri_bvhs_device_items(desc, 0, tris, ltris, res, err);
}

// The mesh stage of a deferred glTF parse (gltf_items.hip) and the host flatten behind it
struct ParsedCtx { const rt_parsed_scene* ps; int rc; };
static int tri_meshes_device(void* ctx, HostBvhArrays& tris, HostBvhArrays& ltris, TriItemsOutcome& res, std::string& err) {
    return emit_tri_bvhs_device_meshes(*((ParsedCtx*)ctx)->ps, 0, tris, ltris, res, err);
}
static bool parsed_arrays(void* ctx, rt_scene_desc& desc, std::string& err) {
    ParsedCtx& c = *(ParsedCtx*)ctx;
    if ((c.rc = rt_parsed_scene_get(c.ps, &desc, nullptr))) err = rt_last_error();  // the eager load's code and message
    return c.rc == RT_OK;
}

static int scene_build_any(const rt_scene_desc& desc, HostScene& hs, uint32_t build_flags, ParsedCtx* parsed) {
    int ndev = 0;
    if ((build_flags & RT_BUILD_DEVICE) && (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0))
        return set_error(RT_ERR_DEVICE, "no HIP device visible (RT_BUILD_DEVICE builds on one)");
    const TriMeshStage stage = {parsed, tri_meshes_device, parsed_arrays};
    std::string err = build_scene(desc, hs, (build_flags & RT_BUILD_DEVICE) ? tri_build_device : nullptr,
                                  (build_flags & RT_BUILD_DEVICE_RECORDS) ? tri_emit_device : nullptr,
                                  (build_flags & RT_BUILD_DEVICE_ITEMS) ? tri_items_device : nullptr,
                                  parsed ? &stage : nullptr);
    if (!err.empty()) return parsed && parsed->rc ? set_error(parsed->rc, err) : set_error(RT_ERR_INVALID, err);
    for (int k = 0; k < 6; ++k)  // traversal stack words carry node indices in 30 bits (render.hip child_word)
        if (hs.bvh[k].n_nodes() >= (1u << 30)) return set_error(RT_ERR_INVALID, "BVH exceeds 2^30 nodes");
    return RT_OK;
}
int scene_build_host(const rt_scene_desc& desc, HostScene& hs, uint32_t build_flags) {
    return scene_build_any(desc, hs, build_flags, nullptr);
}
int scene_build_parsed(const rt_parsed_scene& ps, HostScene& hs, uint32_t build_flags) {
    rt_scene_desc head;  // the description without its triangle arrays
    std::memset(&head, 0, sizeof(head));
    head.n_materials = (uint32_t)ps.mats.size();
    head.materials = ps.mats.data();
    head.n_triangles = ps.n_plan_tris;
    head.tri_mode = ps.tri_mode;
    ParsedCtx ctx = {&ps, RT_OK};
    return scene_build_any(head, hs, build_flags, &ctx);
}

// Scene::new's device side: the flattened scene on the CURRENT HIP device.
// replica: allocate every scene array but copy none from the host (multi.cpp
// fills them from devices[0]'s copy over xGMI, scene_allocs); the small records
// (DevScene, stats) are still written here.
int scene_upload(const HostScene& hs, rt_scene** out, bool replica) {
    *out = nullptr;
    struct ReplicaFlag {
        explicit ReplicaFlag(bool r) { g_replica = r; }
        ~ReplicaFlag() { g_replica = false; }
    } flag(replica);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return set_error(RT_ERR_DEVICE, "no HIP device visible (the hot path has no CPU fallback)");
    std::unique_ptr<rt_scene, SceneDeleter> owner(new rt_scene());  // frees everything on an error return
    rt_scene* s = owner.get();
    HIP_TRY(hipGetDevice(&s->device));
    HIP_TRY(hipEventCreateWithFlags(&s->ws_done, hipEventDisableTiming));
    auto t0 = std::chrono::steady_clock::now();
    int rc = RT_OK;
    DevScene& d = s->dev;
    d.n_planes = (uint32_t)hs.planes.size();
    if ((rc = upload(s, hs.planes, &d.planes)) || (rc = upload(s, hs.plane_mat, &d.plane_mat)) ||
        (rc = upload(s, hs.plane_gid, &d.plane_gid)) || (rc = upload(s, hs.mats, &d.mats)) ||
        (rc = upload_bvh(s, hs.bvh[0], d.boxes)) || (rc = upload_bvh(s, hs.bvh[1], d.ells)) ||
        (rc = upload_bvh(s, hs.bvh[2], d.tris)) || (rc = upload_bvh(s, hs.bvh[3], d.lboxes)) ||
        (rc = upload_bvh(s, hs.bvh[4], d.lells)) || (rc = upload_bvh(s, hs.bvh[5], d.ltris)))
        return rc;
    // ellipsoid reciprocals for dev_quot: computed by the device's own rcp + Newton steps
    // (a replica receives the source's records with them already written)
    if (!replica) {
        HIP_TRY(launch_ell_rcp(const_cast<DevShape*>(d.ells.shapes), d.ells.n_prims, 0));
        HIP_TRY(launch_ell_rcp(const_cast<DevShape*>(d.lells.shapes), d.lells.n_prims, 0));
        HIP_TRY(hipStreamSynchronize(0));
    }
    {  // world normals of plane sides and box faces: rotated(Hit, rot) of render.hip materialise
        std::vector<double> pn(hs.planes.size() * 6), bn(hs.bvh[0].shapes.size() * 24, 0.0);
        for (size_t i = 0; i < hs.planes.size(); ++i) {
            const DevShape& p = hs.planes[i];
            const Quat q = load_quat(p.rot);
            for (int side = 0; side < 2; ++side)
                store3(&pn[i * 6 + side * 3], normalize(rotate(q, load3(p.shape) * (side ? 1.0 : -1.0))));
        }
        for (size_t i = 0; i < hs.bvh[0].shapes.size(); ++i) {
            const Quat q = load_quat(hs.bvh[0].shapes[i].rot);
            for (uint32_t a = 0; a < 8; ++a) {
                if ((a & 3u) == 3u) continue;
                const double sg = (a & 4u) ? 1.0 : -1.0;
                const uint32_t dim = a & 3u;
                const V3 n = dim == 0 ? v3(sg, 0.0, 0.0) : dim == 1 ? v3(0.0, sg, 0.0) : v3(0.0, 0.0, sg);
                store3(&bn[i * 24 + a * 3], normalize(rotate(q, n)));
            }
        }
        if ((rc = upload(s, pn, &d.plane_nrm)) || (rc = upload(s, bn, &d.box_nrm))) return rc;
    }
    d.n_lights = d.lboxes.n_prims + d.lells.n_prims + d.ltris.n_prims;
    // UINT64_MAX - (2^64 - n) % n (oracle.c usize_zone); unused without lights
    d.light_zone = d.n_lights ? UINT64_MAX - (0ull - (uint64_t)d.n_lights) % (uint64_t)d.n_lights : 0;
    d.slt_mask = slt_mask(hs);
    std::memset(d.lq_box, 0, sizeof(d.lq_box));
    d.lq_boxes = lq_boxes(hs, d.lq_box);
    d.max_depth = 0;
    const DevBvh* all[6] = {&d.boxes, &d.ells, &d.tris, &d.lboxes, &d.lells, &d.ltris};
    for (int k = 0; k < 6; ++k) {
        d.max_depth = std::max(d.max_depth, all[k]->depth);
        s->info.bvh_nodes[k] = hs.bvh[k].n_nodes();
        s->info.bvh_depth[k] = hs.bvh[k].depth;
    }
    HIP_TRY(hipMalloc(&s->d_scene, sizeof(DevScene)));
    HIP_TRY(hipMemcpy(s->d_scene, &s->dev, sizeof(DevScene), hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc(&s->d_params, sizeof(KParamsSlot)));  // + an adaptive pass's fields
    HIP_TRY(hipMalloc(&s->d_stats, kStatsWords * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(s->d_stats, 0, kStatsWords * sizeof(unsigned long long)));
    s->info.n_planes = d.n_planes;
    s->info.n_boxes = d.boxes.n_prims;
    s->info.n_ellipsoids = d.ells.n_prims;
    s->info.n_triangles = d.tris.n_prims;
    s->info.n_light_boxes = d.lboxes.n_prims;
    s->info.n_light_ellipsoids = d.lells.n_prims;
    s->info.n_light_triangles = d.ltris.n_prims;
    s->info.shared_light_mask = d.slt_mask;
    const HostBvhArrays& T = hs.bvh[2];
    const uint64_t n_ctris = T.count(kResCtris, T.ctris.size());
    s->compact_bytes = T.count(kResCnodes, T.cnodes.size()) * sizeof(DevNodeC) + n_ctris * sizeof(float);
    s->pair_bytes = (T.count(kResPnodes, T.pnodes.size()) + n_ctris) * sizeof(float);
    s->info.layout_flags = (d.tris.cnodes ? RT_LAYOUT_COMPACT_TRIS : 0u) | (d.lq_boxes ? RT_LAYOUT_LQ_SKIP : 0u) |
                           (d.tris.pnodes ? RT_LAYOUT_PAIR_NODES : 0u) | (hs.device_built ? RT_LAYOUT_DEVICE_BUILT : 0u) |
                           (hs.device_records ? RT_LAYOUT_DEVICE_RECORDS : 0u) |
                           (hs.device_items ? RT_LAYOUT_DEVICE_ITEMS : 0u) |
                           (hs.device_meshes ? RT_LAYOUT_DEVICE_MESHES : 0u);
    s->info.build_ms = hs.build_ms;
    s->info.upload_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out = owner.release();
    return RT_OK;
}

const std::vector<void*>& scene_allocs(const rt_scene* s, const std::vector<size_t>** bytes) {
    *bytes = &s->alloc_bytes;
    return s->allocs;
}
void scene_add_upload_ms(rt_scene* s, double ms) { s->info.upload_ms += ms; }

}  // namespace rt

extern "C" {

void rt_scene_destroy(rt_scene* s) { free_scene(s); }

int rt_scene_get_info(const rt_scene* s, rt_scene_info* out) {
    if (!s || !out) return set_error(RT_ERR_INVALID, "scene/out is NULL");
    *out = s->info;
    return RT_OK;
}

int rt_tiles_per_rank(const rt_render_params* p, uint32_t world, uint32_t* n) {
    int rc = check_params(p);
    if (rc) return rc;
    if (world == 0 || !n) return set_error(RT_ERR_INVALID, "world must be > 0");
    *n = slots_per_rank(make_kparams(p, 0, world));
    return RT_OK;
}

int rt_sample_chunks(const rt_render_params* p, uint32_t* chunks, uint32_t* chunk_spp) {
    int rc = check_params(p);
    if (rc) return rc;
    if (!chunks || !chunk_spp) return set_error(RT_ERR_INVALID, "output is NULL");
    frame_chunks(p, 0, *chunks, *chunk_spp);
    return RT_OK;
}

int rt_scene_sample_chunks(const rt_scene* s, const rt_render_params* p, uint32_t* chunks, uint32_t* chunk_spp) {
    int rc = check_params(p);
    if (rc) return rc;
    if (!s || !chunks || !chunk_spp) return set_error(RT_ERR_INVALID, "scene/output is NULL");
    frame_chunks(p, s->tune.chunk_spp, *chunks, *chunk_spp);
    return RT_OK;
}

int rt_scene_set_tuning(rt_scene* s, const rt_tuning* t) {
    if (!s) return set_error(RT_ERR_INVALID, "scene is NULL");
    if (!t) { s->tune = rt_tuning{0, -1, 0, 0, 0, 0, -1, 0}; s->last_tail_split = 0; return RT_OK; }
    if (t->waves != 0 && (t->waves < 3 || t->waves > 5)) return set_error(RT_ERR_INVALID, "waves must be 0, 3, 4 or 5");
    if (t->resume < -1 || t->resume > 1) return set_error(RT_ERR_INVALID, "resume must be -1, 0 or 1");
    if (t->kinds > 3) return set_error(RT_ERR_INVALID, "kinds must be 0..3");
    // 1 / 2 (what rt_scene_get_tuning reports for a one-kind scene): only the scene's own kinds
    if ((t->kinds == 1 || t->kinds == 2) && (int)t->kinds != scene_kinds(s->dev))
        return set_error(RT_ERR_INVALID, "kinds 1/2 must be the scene's own primitive kinds (0 or 3 otherwise)");
    if (t->suspend_lanes > 64 || t->leaf_lanes > 64) return set_error(RT_ERR_INVALID, "lane counts must be <= 64");
    if (t->compact < -1 || t->compact > 2) return set_error(RT_ERR_INVALID, "compact must be -1, 0, 1 or 2");
    if (t->compact >= 1 && !s->dev.tris.cnodes)
        return set_error(RT_ERR_UNSUPPORTED, "compact >= 1: the scene has no compact triangle layout");
    if (t->compact == 2 && !s->dev.tris.pnodes)
        return set_error(RT_ERR_UNSUPPORTED, "compact = 2: the scene has no pair layout");
    if (t->tail_split > 8) return set_error(RT_ERR_INVALID, "tail_split must be 0..8");
    s->tune = *t;
    s->last_tail_split = 0;
    return RT_OK;
}

int rt_scene_checksum(rt_scene* s, uint64_t* out) {
    if (!s || !out) return set_error(RT_ERR_INVALID, "scene/out is NULL");
    DEVICE_GUARD(s);
    const size_t n = s->allocs.size();
    DevBuf<unsigned long long> sums;
    HIP_TRY(sums.alloc(std::max<size_t>(n, 1)));
    for (size_t k = 0; k < n; ++k) HIP_TRY(launch_checksum(s->allocs[k], s->alloc_bytes[k], sums.p + k, 0));
    std::vector<unsigned long long> h(n);
    HIP_TRY(hipDeviceSynchronize());
    if (n) HIP_TRY(hipMemcpy(h.data(), sums.p, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    uint64_t acc = 0xcbf29ce484222325ull;  // arrays in allocation order, each with its size
    for (size_t k = 0; k < n; ++k) acc = (acc ^ (h[k] + 0x9e3779b97f4a7c15ull * s->alloc_bytes[k])) * 0x100000001b3ull;
    *out = acc;
    return RT_OK;
}

int rt_scene_get_tuning(const rt_scene* s, rt_tuning* out) {
    if (!s || !out) return set_error(RT_ERR_INVALID, "scene/out is NULL");
    out->waves = path_waves(s);
    out->resume = path_resume(s) ? 1 : 0;
    out->kinds = (uint32_t)path_kinds(s);
    out->suspend_lanes = path_suspend(s);
    out->leaf_lanes = path_leaf_batch(s);
    out->chunk_spp = s->tune.chunk_spp;
    out->compact = path_pairs(s) ? 2 : (path_compact(s) ? 1 : 0);
    out->tail_split = s->last_tail_split ? s->last_tail_split : (s->tune.tail_split ? s->tune.tail_split : kTailSplit);
    return RT_OK;
}

// A moments frame has no stats and no hit-id instance (render.hip path_kernel MOM).
static int check_moments_flags(const rt_render_params* p) {
    if (p->flags & (RT_FLAG_STATS | RT_FLAG_HIT_IDS))
        return set_error(RT_ERR_INVALID, "a moments render takes neither RT_FLAG_STATS nor RT_FLAG_HIT_IDS");
    return RT_OK;
}

// rt_render_tiles_async (d_tile_sq NULL) and rt_render_tiles_moments_async
static int render_tiles(rt_scene* s, const rt_render_params* p, uint32_t rank, uint32_t world, double* d_tile_rgb,
                        double* d_tile_sq, void* stream) {
    if (world == 0 || rank >= world) return set_error(RT_ERR_INVALID, "rank must be < world");
    DEVICE_GUARD(s);
    KParams k = make_kparams(p, rank, world, s->tune.chunk_spp);
    const bool want_stats = (p->flags & RT_FLAG_STATS) != 0;
    PathWork W;
    if (int rc = prepare_path(s, k, want_stats, false, W, d_tile_sq != nullptr)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    HIP_TRY(ws_begin(s, st));
    HIP_TRY(launch_path(s->dev, k, W, d_tile_rgb, nullptr, want_stats ? s->d_stats : nullptr, st, d_tile_sq));
    HIP_TRY(ws_end(s, st));
    return RT_OK;
}

int rt_render_tiles_async(rt_scene* s, const rt_render_params* p, uint32_t rank, uint32_t world,
                          double* d_tile_rgb, void* stream) {
    int rc = check_params(p);
    if (rc) return rc;
    if (!s || !d_tile_rgb) return set_error(RT_ERR_INVALID, "scene/output is NULL");
    return render_tiles(s, p, rank, world, d_tile_rgb, nullptr, stream);
}

int rt_render_tiles_moments_async(rt_scene* s, const rt_render_params* p, uint32_t rank, uint32_t world,
                                  double* d_tile_rgb, double* d_tile_sq, void* stream) {
    int rc = check_params(p);
    if (rc || (rc = check_moments_flags(p))) return rc;
    if (!s || !d_tile_rgb || !d_tile_sq) return set_error(RT_ERR_INVALID, "scene/output is NULL");
    return render_tiles(s, p, rank, world, d_tile_rgb, d_tile_sq, stream);
}

// d_count: nullptr (spp holds), or every pixel's own count (spp unused)
static int error_estimate(const double* d_mean, const double* d_sq, const uint32_t* d_count, uint64_t n_pixels,
                          uint32_t spp, double* d_se, double* d_summary, void* stream) {
    if (!d_summary || ((!d_mean || !d_sq) && n_pixels)) return set_error(RT_ERR_INVALID, "mean/sq/summary is NULL");
    if (n_pixels > UINT64_MAX / 24) return set_error(RT_ERR_INVALID, "n_pixels too large");
    if (((uintptr_t)d_mean | (uintptr_t)d_sq | (uintptr_t)d_se) & 15u)
        return set_error(RT_ERR_INVALID, "mean/sq/se must be 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(g_se_mutex);
    SeSlot* slot = nullptr;
    if (int rc = se_slot_take(st, &slot)) return rc;
    HIP_TRY(launch_error_estimate(d_mean, d_sq, n_pixels, spp, d_se, d_summary, slot->part, st, d_count));
    HIP_TRY(hipEventRecord(slot->done, st));
    return RT_OK;
}

int rt_error_estimate_async(const double* d_mean, const double* d_sq, uint64_t n_pixels, uint32_t spp, double* d_se,
                            double* d_summary, void* stream) {
    if (spp == 0) return set_error(RT_ERR_INVALID, "spp must be > 0");
    return error_estimate(d_mean, d_sq, nullptr, n_pixels, spp, d_se, d_summary, stream);
}

int rt_error_estimate_counts_async(const double* d_mean, const double* d_sq, const uint32_t* d_count, uint64_t n_pixels,
                                   double* d_se, double* d_summary, void* stream) {
    if (!d_count || ((uintptr_t)d_count & 3u)) return set_error(RT_ERR_INVALID, "count is NULL or not 4-byte aligned");
    return error_estimate(d_mean, d_sq, d_count, n_pixels, 0, d_se, d_summary, stream);
}

int rt_camera_rays_async(const rt_render_params* p, double* d_rays, void* stream) {
    int rc = check_params(p);
    if (rc) return rc;
    if (!d_rays || ((uintptr_t)d_rays & 15u)) return set_error(RT_ERR_INVALID, "rays is NULL or not 16-byte aligned");
    HIP_TRY(launch_camera_rays(make_kparams(p, 0, 1), d_rays, (hipStream_t)stream));
    return RT_OK;
}

int rt_denoise_workspace_bytes(uint32_t width, uint32_t height, uint64_t* bytes) {
    if (!bytes) return set_error(RT_ERR_INVALID, "bytes is NULL");
    if (width == 0 || height == 0) return set_error(RT_ERR_INVALID, "width/height must be > 0");
    *bytes = 3 * denoise_buffer_bytes((uint64_t)width * height);
    return RT_OK;
}

// counts: d_count [H][W] u32 is required and p->spp is not looked at; else d_count is nullptr
static int denoise(const rt_denoise_params* p, const double* d_mean, const double* d_sq, const uint32_t* d_count,
                   bool counts, const double* d_rays, const rt_hit* d_hits, double* d_out, double* d_out_var,
                   void* d_workspace, uint64_t workspace_bytes, void* stream) {
    if (!p) return set_error(RT_ERR_INVALID, "params is NULL");
    if (p->width == 0 || p->height == 0) return set_error(RT_ERR_INVALID, "width/height must be > 0");
    if (p->width > 65535 || p->height > 65535) return set_error(RT_ERR_INVALID, "width/height must be <= 65535");
    if (!counts && p->spp < 2) return set_error(RT_ERR_INVALID, "the variance needs spp >= 2");
    if (counts && (!d_count || ((uintptr_t)d_count & 3u)))
        return set_error(RT_ERR_INVALID, "count is NULL or not 4-byte aligned");
    DenoiseSettings S;
    S.width = p->width; S.height = p->height; S.spp = p->spp;
    S.iterations = p->iterations ? p->iterations : RT_DENOISE_ITERATIONS;
    S.squarings = p->normal_squarings == RT_DENOISE_SQUARINGS_NONE ? 0u
                  : p->normal_squarings ? p->normal_squarings : RT_DENOISE_NORMAL_SQUARINGS;
    if (S.iterations > kMaxIterations) return set_error(RT_ERR_INVALID, "iterations must be 1..8 (0: the default)");
    if (S.squarings > kMaxSquarings)
        return set_error(RT_ERR_INVALID, "normal_squarings must be 1..10, 0 (default) or RT_DENOISE_SQUARINGS_NONE");
    const double in[3] = {p->sigma_l, p->sigma_z, p->eps};
    const double def[3] = {RT_DENOISE_SIGMA_L, RT_DENOISE_SIGMA_Z, RT_DENOISE_EPS};
    double v[3];
    for (int i = 0; i < 3; ++i) {
        if (!(in[i] >= 0.0) || !std::isfinite(in[i]))
            return set_error(RT_ERR_INVALID, "sigma_l, sigma_z and eps must be finite and > 0 (0: the default)");
        v[i] = in[i] == 0.0 ? def[i] : in[i];
    }
    S.sigma_l = v[0]; S.sigma_z = v[1]; S.eps = v[2];
    if (!d_mean || !d_sq || !d_rays || !d_hits || !d_out || !d_workspace)
        return set_error(RT_ERR_INVALID, "mean/sq/rays/hits/out/workspace is NULL");
    if (((uintptr_t)d_mean | (uintptr_t)d_sq | (uintptr_t)d_rays | (uintptr_t)d_hits | (uintptr_t)d_out |
         (uintptr_t)d_out_var | (uintptr_t)d_workspace) & 15u)
        return set_error(RT_ERR_INVALID, "the denoiser's buffers must be 16-byte aligned");
    const uint64_t n = (uint64_t)p->width * p->height, need = 3 * denoise_buffer_bytes(n);
    if (workspace_bytes < need)
        return set_error(RT_ERR_INVALID, "workspace too small: " + std::to_string(need) + " bytes needed");
    // an output may overlap neither what the kernels still read nor the other output
    struct Range { const void* p; uint64_t bytes; };
    const Range outs[2] = {{d_out, n * 24}, {d_out_var, d_out_var ? n * 8 : 0}};
    const Range ins[7] = {{d_count, counts ? n * 4 : 0}, {d_mean, n * 24}, {d_sq, n * 24}, {d_rays, n * 48},
                          {d_hits, n * 64}, {d_workspace, need}, outs[1]};
    for (int o = 0; o < 2; ++o)
        for (int i = 0; i < 7 - o; ++i) {
            const uintptr_t a = (uintptr_t)outs[o].p, b = (uintptr_t)ins[i].p;
            if (outs[o].bytes && ins[i].bytes && a < b + ins[i].bytes && b < a + outs[o].bytes)
                return set_error(RT_ERR_INVALID, "out/out_var overlaps an input, the workspace or the other output");
        }
    if (counts && (uintptr_t)d_count < (uintptr_t)d_workspace + need && (uintptr_t)d_workspace < (uintptr_t)d_count + n * 4)
        return set_error(RT_ERR_INVALID, "count overlaps the workspace");
    HIP_TRY(launch_denoise(S, d_mean, d_sq, d_rays, d_hits, d_out, d_out_var, d_workspace, (hipStream_t)stream, d_count));
    return RT_OK;
}

int rt_denoise_async(const rt_denoise_params* p, const double* d_mean, const double* d_sq, const double* d_rays,
                     const rt_hit* d_hits, double* d_out, double* d_out_var, void* d_workspace,
                     uint64_t workspace_bytes, void* stream) {
    return denoise(p, d_mean, d_sq, nullptr, false, d_rays, d_hits, d_out, d_out_var, d_workspace, workspace_bytes, stream);
}

int rt_denoise_counts_async(const rt_denoise_params* p, const double* d_mean, const double* d_sq,
                            const uint32_t* d_count, const double* d_rays, const rt_hit* d_hits, double* d_out,
                            double* d_out_var, void* d_workspace, uint64_t workspace_bytes, void* stream) {
    return denoise(p, d_mean, d_sq, d_count, true, d_rays, d_hits, d_out, d_out_var, d_workspace, workspace_bytes, stream);
}

int rt_ssim_window(double sigma, double* out11) {
    if (!out11) return set_error(RT_ERR_INVALID, "out is NULL");
    if (!(sigma > 0.0) || !std::isfinite(sigma)) return set_error(RT_ERR_INVALID, "sigma must be finite and > 0");
    double sum = 0.0;
    for (int i = 0; i < 11; ++i) {
        const double d = (double)(i - 5);
        out11[i] = std::exp(-(d * d) / (2.0 * (sigma * sigma)));
        sum = sum + out11[i];
    }
    for (int i = 0; i < 11; ++i) out11[i] = out11[i] / sum;
    return RT_OK;
}

static int metrics_size(uint32_t width, uint32_t height) {
    if (width == 0 || height == 0) return set_error(RT_ERR_INVALID, "width/height must be > 0");
    if (width > 65535 || height > 65535) return set_error(RT_ERR_INVALID, "width/height must be <= 65535");
    return RT_OK;
}

int rt_image_metrics_workspace_bytes(uint32_t width, uint32_t height, uint64_t* bytes) {
    if (!bytes) return set_error(RT_ERR_INVALID, "bytes is NULL");
    if (int rc = metrics_size(width, height)) return rc;
    *bytes = (metrics_blocks(width, height) * 64 + 255) / 256 * 256;
    return RT_OK;
}

int rt_image_metrics_async(const rt_metrics_params* p, const void* d_a, const void* d_b, double* d_rel, double* d_ssim,
                           double* d_summary, void* d_workspace, uint64_t workspace_bytes, void* stream) {
    if (!p) return set_error(RT_ERR_INVALID, "params is NULL");
    if (int rc = metrics_size(p->width, p->height)) return rc;
    if (p->format != RT_METRICS_F64 && p->format != RT_METRICS_U8)
        return set_error(RT_ERR_INVALID, "format must be RT_METRICS_F64 or RT_METRICS_U8");
    MetricsSettings S;
    S.width = p->width; S.height = p->height; S.format = p->format;
    if (!(p->peak >= 0.0) || !std::isfinite(p->peak) || !(p->eps >= 0.0) || !std::isfinite(p->eps))
        return set_error(RT_ERR_INVALID, "peak and eps must be finite and > 0 (0: the default)");
    S.peak = p->peak == 0.0 ? (p->format == RT_METRICS_F64 ? 1.0 : 255.0) : p->peak;
    S.eps = p->eps == 0.0 ? RT_METRICS_EPS : p->eps;
    int zeros = 0;
    for (int i = 0; i < 11; ++i) {
        if (!(p->window[i] >= 0.0) || !std::isfinite(p->window[i]))
            return set_error(RT_ERR_INVALID, "the window's taps must be finite and > 0 (all zero: the default)");
        zeros += p->window[i] == 0.0;
        S.window[i] = p->window[i];
    }
    if (zeros != 0 && zeros != 11)
        return set_error(RT_ERR_INVALID, "the window mixes zero and non-zero taps (all zero: the default)");
    if (zeros == 11) rt_ssim_window(1.5, S.window);
    if (!d_a || !d_b || !d_summary || !d_workspace) return set_error(RT_ERR_INVALID, "a/b/summary/workspace is NULL");
    const bool f64 = p->format == RT_METRICS_F64;
    if ((((uintptr_t)d_a | (uintptr_t)d_b) & (f64 ? 7u : 0u)) ||
        (((uintptr_t)d_rel | (uintptr_t)d_ssim | (uintptr_t)d_summary | (uintptr_t)d_workspace) & 7u))
        return set_error(RT_ERR_INVALID, "the f64 buffers and the workspace must be 8-byte aligned");
    const uint64_t n = (uint64_t)p->width * p->height, need = (metrics_blocks(p->width, p->height) * 64 + 255) / 256 * 256;
    if (workspace_bytes < need)
        return set_error(RT_ERR_INVALID, "workspace too small: " + std::to_string(need) + " bytes needed");
    const uint64_t windows = p->width >= 11 && p->height >= 11 ? (uint64_t)(p->width - 10) * (p->height - 10) : 0;
    // an output may overlap neither what the kernels read nor another output
    struct Range { const void* p; uint64_t bytes; };
    const Range outs[3] = {{d_rel, d_rel ? n * 8 : 0}, {d_ssim, d_ssim ? windows * 8 : 0}, {d_summary, 64}};
    const Range ins[5] = {{d_a, n * (f64 ? 24 : 3)}, {d_b, n * (f64 ? 24 : 3)}, {d_workspace, need}, outs[1], outs[2]};
    for (int o = 0; o < 3; ++o)
        for (int i = 0; i < 5; ++i) {
            if (i >= 3 && i - 2 <= o) continue;  // an output against the outputs after it
            const uintptr_t a = (uintptr_t)outs[o].p, b = (uintptr_t)ins[i].p;
            if (outs[o].bytes && ins[i].bytes && a < b + ins[i].bytes && b < a + outs[o].bytes)
                return set_error(RT_ERR_INVALID, "rel/ssim/summary overlaps an input, the workspace or another output");
        }
    HIP_TRY(launch_image_metrics(S, d_a, d_b, d_rel, d_ssim, d_summary, (double*)d_workspace, (hipStream_t)stream));
    return RT_OK;
}

static int temporal_size(uint32_t width, uint32_t height) {
    if (width == 0 || height == 0) return set_error(RT_ERR_INVALID, "width/height must be > 0");
    if (width > 65535 || height > 65535) return set_error(RT_ERR_INVALID, "width/height must be <= 65535");
    return RT_OK;
}

int rt_temporal_history_bytes(uint32_t width, uint32_t height, uint64_t* bytes) {
    if (!bytes) return set_error(RT_ERR_INVALID, "bytes is NULL");
    if (int rc = temporal_size(width, height)) return rc;
    const uint64_t n = (uint64_t)width * height;
    *bytes = temporal_guide_bytes(n) + temporal_colour_bytes(n);
    return RT_OK;
}

int rt_temporal_accumulate_async(const rt_temporal_params* p, const rt_render_params* prev, const double* d_mean,
                                 const double* d_sq, const uint32_t* d_count, const double* d_rays, const rt_hit* d_hits,
                                 const void* d_hist_prev, void* d_hist_next, double* d_out_mean, double* d_out_sq,
                                 uint32_t* d_out_count, void* stream) {
    if (!p) return set_error(RT_ERR_INVALID, "params is NULL");
    if (int rc = temporal_size(p->width, p->height)) return rc;
    if ((prev != nullptr) != (d_hist_prev != nullptr))
        return set_error(RT_ERR_INVALID, "prev_camera and hist_prev go together: both or neither");
    TemporalSettings S;
    std::memset(&S, 0, sizeof(S));
    S.width = p->width; S.height = p->height; S.spp = p->spp; S.flags = p->flags;
    if (!d_count && (p->spp < 1 || p->spp > (1u << 30))) return set_error(RT_ERR_INVALID, "spp must be 1..2^30");
    if (p->max_history > (1u << 30)) return set_error(RT_ERR_INVALID, "max_history must be <= 2^30 (0: the default)");
    S.max_history = p->max_history ? p->max_history : RT_TEMPORAL_MAX_HISTORY;
    if (p->flags & ~RT_TEMPORAL_NO_WINDOW) return set_error(RT_ERR_INVALID, "unknown flag");
    if (!(p->normal_min >= 0.0) || !(p->normal_min <= 1.0))
        return set_error(RT_ERR_INVALID, "normal_min must be in (0, 1] (0: the default)");
    if (!(p->plane_tol >= 0.0) || !std::isfinite(p->plane_tol))
        return set_error(RT_ERR_INVALID, "plane_tol must be finite and > 0 (0: the default)");
    S.normal_min = p->normal_min == 0.0 ? RT_TEMPORAL_NORMAL_MIN : p->normal_min;
    S.plane_tol = p->plane_tol == 0.0 ? RT_TEMPORAL_PLANE_TOL : p->plane_tol;
    if (prev) {
        if (prev->width != p->width || prev->height != p->height)
            return set_error(RT_ERR_INVALID, "prev_camera's width/height differ from the frame's");
        if (prev->fov_axis != RT_FOV_X && prev->fov_axis != RT_FOV_Y) return set_error(RT_ERR_INVALID, "bad fov_axis");
        rt_render_params cam = *prev;
        cam.spp = 1;  // not read here; make_kparams' chunking wants one
        const KParams k = make_kparams(&cam, 0, 1);
        S.has_prev = 1;
        S.fw = k.fw; S.fh = k.fh; S.tan_x = k.tan_x; S.tan_y = k.tan_y;
        // the dual basis: the reference normalises right, up and forward each alone (scene.rs:169-175),
        // so they need not be orthogonal and plain dot products with them are not the inverse
        const V3 r = load3(prev->cam_right), u = load3(prev->cam_up), f = load3(prev->cam_forward);
        const V3 uf = cross(u, f);
        const double det = dot(r, uf);
        if (det == 0.0 || !std::isfinite(det))
            return set_error(RT_ERR_INVALID, "prev_camera's basis is singular or not finite");
        const V3 rs = uf / det, us = cross(f, r) / det, fs = cross(r, u) / det;
        const V3 pos = load3(prev->cam_position);
        const V3 rows[4] = {pos, rs, us, fs};
        double* dst[4] = {S.pos, S.rs, S.us, S.fs};
        for (int i = 0; i < 4; ++i) {
            dst[i][0] = rows[i].x; dst[i][1] = rows[i].y; dst[i][2] = rows[i].z;
        }
    }
    if (!d_mean || !d_sq || !d_rays || !d_hits || !d_hist_next || !d_out_mean || !d_out_sq || !d_out_count)
        return set_error(RT_ERR_INVALID, "mean/sq/rays/hits/hist_next/out_mean/out_sq/out_count is NULL");
    if (((uintptr_t)d_mean | (uintptr_t)d_sq | (uintptr_t)d_rays | (uintptr_t)d_hits | (uintptr_t)d_out_mean |
         (uintptr_t)d_out_sq) & 15u)
        return set_error(RT_ERR_INVALID, "the f64 buffers and the hits must be 16-byte aligned");
    if (((uintptr_t)d_hist_prev | (uintptr_t)d_hist_next) & 255u)
        return set_error(RT_ERR_INVALID, "the history blocks must be 256-byte aligned");
    if (((uintptr_t)d_count | (uintptr_t)d_out_count) & 3u)
        return set_error(RT_ERR_INVALID, "the counts must be 4-byte aligned");
    const uint64_t n = (uint64_t)p->width * p->height, hist = temporal_guide_bytes(n) + temporal_colour_bytes(n);
    // an output may overlap neither what the kernel reads nor another output
    struct Range { const void* p; uint64_t bytes; };
    const Range outs[4] = {{d_hist_next, hist}, {d_out_mean, n * 24}, {d_out_sq, n * 24}, {d_out_count, n * 4}};
    const Range ins[6] = {{d_mean, n * 24}, {d_sq, n * 24}, {d_count, d_count ? n * 4 : 0}, {d_rays, n * 48},
                          {d_hits, n * 64}, {d_hist_prev, d_hist_prev ? hist : 0}};
    for (int o = 0; o < 4; ++o)
        for (int i = 0; i < 6 + 3 - o; ++i) {  // the inputs, then the outputs after this one
            const Range& in = i < 6 ? ins[i] : outs[o + 1 + (i - 6)];
            const uintptr_t a = (uintptr_t)outs[o].p, b = (uintptr_t)in.p;
            if (in.bytes && a < b + in.bytes && b < a + outs[o].bytes)
                return set_error(RT_ERR_INVALID, "hist_next/out_mean/out_sq/out_count overlaps an input, hist_prev or another output");
        }
    HIP_TRY(launch_temporal(S, d_mean, d_sq, d_count, d_rays, d_hits, d_hist_prev, d_hist_next, d_out_mean, d_out_sq,
                            d_out_count, (hipStream_t)stream));
    return RT_OK;
}

int rt_read_stats(rt_scene* s, rt_stats* out, int reset) {
    if (!s || !out) return set_error(RT_ERR_INVALID, "scene/out is NULL");
    DEVICE_GUARD(s);
    HIP_TRY(hipDeviceSynchronize());
    std::memset(out, 0, sizeof(*out));
    int rc = copy_stats(s, out);
    if (rc) return rc;
    if (reset) HIP_TRY(hipMemset(s->d_stats, 0, kStatsWords * sizeof(unsigned long long)));
    return RT_OK;
}

int rt_read_raw_stats(rt_scene* s, uint64_t* out, uint32_t n) {
    if (!s || !out || n > (uint32_t)kStatsWords) return set_error(RT_ERR_INVALID, "scene/out NULL or n > 64");
    DEVICE_GUARD(s);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, s->d_stats, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_unpack_tiles_async(const rt_render_params* p, uint32_t world, const double* d_gathered, double* d_image,
                          void* stream) {
    int rc = check_params(p);
    if (rc) return rc;
    if (!d_gathered || !d_image || world == 0) return set_error(RT_ERR_INVALID, "bad unpack arguments");
    KParams k = make_kparams(p, 0, world);
    HIP_TRY(launch_unpack(d_gathered, d_image, p->width, p->height, k.tiles_x, world, slots_per_rank(k),
                          (hipStream_t)stream));
    return RT_OK;
}

int rt_unpack_tiles_bytes_async(const rt_render_params* p, uint32_t world, const double* d_gathered,
                                uint8_t* d_bytes, void* stream) {
    int rc = check_params(p);
    if (rc) return rc;
    if (!d_gathered || !d_bytes || world == 0) return set_error(RT_ERR_INVALID, "bad unpack arguments");
    KParams k = make_kparams(p, 0, world);
    HIP_TRY(launch_unpack_bytes(d_gathered, d_bytes, p->width, p->height, k.tiles_x, world, slots_per_rank(k),
                                (hipStream_t)stream));
    return RT_OK;
}

int rt_tonemap_bytes_async(const double* d_rgb, uint64_t n_pixels, uint8_t* d_bytes, void* stream) {
    if ((!d_rgb || !d_bytes) && n_pixels) return set_error(RT_ERR_INVALID, "rgb/bytes is NULL");
    HIP_TRY(launch_tonemap_bytes(d_rgb, 3 * n_pixels, d_bytes, (hipStream_t)stream));
    return RT_OK;
}

// rt_render (out_sq_rgb NULL) and rt_render_moments (no hit ids, no counters)
static int render_frame(rt_scene* s, const rt_render_params* p, double* out_mean_rgb, double* out_sq_rgb,
                        int32_t* opt_hit_ids, rt_stats* opt_stats) {
    auto t0 = std::chrono::steady_clock::now();
    int rc;
    DEVICE_GUARD(s);
    KParams k = make_kparams(p, 0, 1, s->tune.chunk_spp);
    const uint32_t slots = slots_per_rank(k);
    const uint64_t npx = (uint64_t)p->width * p->height;
    const bool want_hits = opt_hit_ids && (p->flags & RT_FLAG_HIT_IDS);
    const bool want_stats = opt_stats && (p->flags & RT_FLAG_STATS);
    PathWork W;
    if ((rc = prepare_path(s, k, want_stats, want_hits, W, out_sq_rgb != nullptr))) return rc;
    DevBuf<double> tiles, img, tiles_sq, img_sq;
    DevBuf<int32_t> hits;
    HIP_TRY(tiles.alloc((size_t)slots * 256 * 3));
    HIP_TRY(img.alloc(npx * 3));
    if (out_sq_rgb) {
        HIP_TRY(tiles_sq.alloc((size_t)slots * 256 * 3));
        HIP_TRY(img_sq.alloc(npx * 3));
    }
    const uint64_t nhits = npx * p->spp * p->ray_depth;
    if (want_hits) HIP_TRY(hits.alloc(nhits));
    if (want_stats) HIP_TRY(hipMemset(s->d_stats, 0, kStatsWords * sizeof(unsigned long long)));
    EventPair ev;
    HIP_TRY(hipEventCreate(&ev.a));
    HIP_TRY(hipEventCreate(&ev.b));
    HIP_TRY(ws_begin(s, 0));
    HIP_TRY(hipEventRecord(ev.a, 0));
    hipError_t le = launch_path(s->dev, k, W, tiles.p, want_hits ? hits.p : nullptr,
                                want_stats ? s->d_stats : nullptr, 0, tiles_sq.p);
    HIP_TRY(hipEventRecord(ev.b, 0));
    if (le != hipSuccess) return set_error(RT_ERR_DEVICE, std::string("path kernel launch: ") + hipGetErrorString(le));
    HIP_TRY(ws_end(s, 0));
    HIP_TRY(launch_unpack(tiles.p, img.p, p->width, p->height, k.tiles_x, 1, slots, 0));
    if (out_sq_rgb) HIP_TRY(launch_unpack(tiles_sq.p, img_sq.p, p->width, p->height, k.tiles_x, 1, slots, 0));
    HIP_TRY(hipDeviceSynchronize());
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev.a, ev.b);
    HIP_TRY(hipMemcpy(out_mean_rgb, img.p, npx * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_sq_rgb) HIP_TRY(hipMemcpy(out_sq_rgb, img_sq.p, npx * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (want_hits) HIP_TRY(hipMemcpy(opt_hit_ids, hits.p, nhits * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (opt_stats) {
        std::memset(opt_stats, 0, sizeof(*opt_stats));
        if (want_stats && (rc = copy_stats(s, opt_stats))) return rc;
        opt_stats->kernel_ms = ms;
        opt_stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return RT_OK;
}

int rt_render(rt_scene* s, const rt_render_params* p, double* out_mean_rgb, int32_t* opt_hit_ids,
              rt_stats* opt_stats) {
    int rc = check_params(p);
    if (rc) return rc;
    if (!s || !out_mean_rgb) return set_error(RT_ERR_INVALID, "scene/output is NULL");
    return render_frame(s, p, out_mean_rgb, nullptr, opt_hit_ids, opt_stats);
}

int rt_render_moments(rt_scene* s, const rt_render_params* p, double* out_mean_rgb, double* out_sq_rgb,
                      rt_stats* opt_stats) {
    int rc = check_params(p);
    if (rc || (rc = check_moments_flags(p))) return rc;
    if (!s || !out_mean_rgb || !out_sq_rgb) return set_error(RT_ERR_INVALID, "scene/output is NULL");
    return render_frame(s, p, out_mean_rgb, out_sq_rgb, nullptr, opt_stats);
}

/* ---- adaptive sampling (adaptive.hip) ---- */
static uint64_t frame_tiles(uint32_t width, uint32_t height) {
    return (uint64_t)((width + RT_TILE - 1) / RT_TILE) * ((height + RT_TILE - 1) / RT_TILE);
}
// (no upper limit: only a pass, which check_params guards, packs pixel origins into 16 bits)
static int check_frame(uint32_t width, uint32_t height) {
    if (width == 0 || height == 0) return set_error(RT_ERR_INVALID, "width/height must be > 0");
    return RT_OK;
}
static int check_adaptive_workspace(uint32_t width, uint32_t height, const void* ws, uint64_t bytes) {
    if (!ws || ((uintptr_t)ws & 255u)) return set_error(RT_ERR_INVALID, "workspace is NULL or not 256-byte aligned");
    const uint64_t need = adaptive_layout(frame_tiles(width, height)).bytes;
    if (bytes < need) return set_error(RT_ERR_INVALID, "workspace too small: " + std::to_string(need) + " bytes needed");
    return RT_OK;
}

int rt_adaptive_workspace_bytes(uint32_t width, uint32_t height, uint64_t* bytes, rt_adaptive_layout* opt_layout) {
    if (!bytes) return set_error(RT_ERR_INVALID, "bytes is NULL");
    if (int rc = check_frame(width, height)) return rc;
    const AdaptiveLayout L = adaptive_layout(frame_tiles(width, height));
    *bytes = L.bytes;
    if (opt_layout) {
        opt_layout->n_tiles = frame_tiles(width, height);
        opt_layout->acc_sum = L.acc_sum; opt_layout->acc_sq = L.acc_sq; opt_layout->tile_count = L.tile_count;
        opt_layout->tile_err = L.tile_err; opt_layout->tile_flag = L.tile_flag; opt_layout->tile_list = L.tile_list;
        opt_layout->info = L.info;
    }
    return RT_OK;
}

int rt_adaptive_pass_async(rt_scene* s, const rt_render_params* p, void* d_workspace, uint64_t workspace_bytes,
                           int use_list, uint32_t n_list, uint32_t sample_base, void* stream) {
    int rc = check_params(p);
    if (rc || (rc = check_moments_flags(p))) return rc;
    if (!s) return set_error(RT_ERR_INVALID, "scene is NULL");
    if (p->spp < 2) return set_error(RT_ERR_INVALID, "a pass needs spp >= 2");
    if ((uint64_t)sample_base + p->spp > (1ull << 32)) return set_error(RT_ERR_INVALID, "sample_base + spp exceeds 2^32");
    if ((rc = check_adaptive_workspace(p->width, p->height, d_workspace, workspace_bytes))) return rc;
    const uint64_t n_tiles = frame_tiles(p->width, p->height);
    if (use_list && n_list > n_tiles) return set_error(RT_ERR_INVALID, "n_list exceeds the frame's tiles");
    if (use_list && n_list == 0) return RT_OK;
    DEVICE_GUARD(s);
    KParams k = make_kparams(p, 0, 1, s->tune.chunk_spp);
    const uint32_t* list = nullptr;
    if (use_list) {
        list = (const uint32_t*)((char*)d_workspace + adaptive_layout(n_tiles).tile_list);
        k.n_slots = n_list;
    }
    const KList kl{list, k.n_slots, sample_base, 1u, 0u};
    PathWork W;
    if ((rc = prepare_path(s, k, false, false, W, true, true))) return rc;
    const hipStream_t st = (hipStream_t)stream;
    HIP_TRY(ws_begin(s, st));
    // both outputs go to the scene's partials, where a chunked pass's run sums are anyway
    HIP_TRY(launch_path(s->dev, k, W, W.part, nullptr, nullptr, st, W.part_sq, &kl));
    HIP_TRY(launch_adaptive_accumulate(d_workspace, n_tiles, W.part, W.part_sq, list, k.n_slots, k.chunks, p->spp,
                                       sample_base == 0, st));
    HIP_TRY(ws_end(s, st));
    return RT_OK;
}

// rank < 0: the largest pixel error (as_metric); else the ranked one (as_metric_rank)
static int adaptive_select(uint32_t width, uint32_t height, void* d_workspace, uint64_t workspace_bytes, double threshold,
                           double eps, uint32_t pass_spp, uint32_t max_spp, int rank, void* stream) {
    int rc = check_frame(width, height);
    if (rc || (rc = check_adaptive_workspace(width, height, d_workspace, workspace_bytes))) return rc;
    if (!(threshold >= 0.0)) return set_error(RT_ERR_INVALID, "threshold must be >= 0");
    if (!(eps >= 0.0) || !std::isfinite(eps)) return set_error(RT_ERR_INVALID, "eps must be finite and > 0 (0: the default)");
    if (rank > 255) return set_error(RT_ERR_INVALID, "rank must be 0..255");
    eps = eps == 0.0 ? RT_ADAPTIVE_EPS : eps;
    if (rank < 0)
        HIP_TRY(launch_adaptive_select(d_workspace, frame_tiles(width, height), threshold, eps, pass_spp, max_spp,
                                       (hipStream_t)stream));
    else
        HIP_TRY(launch_adaptive_select_rank(d_workspace, width, height, threshold, eps, pass_spp, max_spp, (uint32_t)rank,
                                            (hipStream_t)stream));
    return RT_OK;
}

int rt_adaptive_select_async(uint32_t width, uint32_t height, void* d_workspace, uint64_t workspace_bytes,
                             double threshold, double eps, uint32_t pass_spp, uint32_t max_spp, void* stream) {
    return adaptive_select(width, height, d_workspace, workspace_bytes, threshold, eps, pass_spp, max_spp, -1, stream);
}

int rt_adaptive_select_rank_async(uint32_t width, uint32_t height, void* d_workspace, uint64_t workspace_bytes,
                                  double threshold, double eps, uint32_t pass_spp, uint32_t max_spp, uint32_t rank,
                                  void* stream) {
    return adaptive_select(width, height, d_workspace, workspace_bytes, threshold, eps, pass_spp, max_spp,
                           rank > 255 ? 256 : (int)rank, stream);
}

int rt_adaptive_resolve_async(const rt_render_params* p, const void* d_workspace, uint64_t workspace_bytes,
                              double* d_mean, double* d_sq, uint32_t* d_count, void* stream) {
    int rc = check_params(p);
    if (rc || (rc = check_adaptive_workspace(p->width, p->height, d_workspace, workspace_bytes))) return rc;
    if (!d_mean || !d_sq) return set_error(RT_ERR_INVALID, "mean/sq is NULL");
    HIP_TRY(launch_adaptive_resolve(d_workspace, p->width, p->height, d_mean, d_sq, d_count, (hipStream_t)stream));
    return RT_OK;
}

// the loop of rt_render_adaptive (rank < 0) and rt_render_adaptive_rank
static int render_adaptive(rt_scene* s, const rt_render_params* p, const rt_adaptive_params* a, int rank,
                           double* out_mean_rgb, double* out_sq_rgb, uint32_t* out_count, rt_stats* opt_stats) {
    const auto t0 = std::chrono::steady_clock::now();
    int rc = check_params(p);
    if (rc || (rc = check_moments_flags(p))) return rc;
    if (!s || !a || !out_mean_rgb || !out_sq_rgb) return set_error(RT_ERR_INVALID, "scene/adaptive params/output is NULL");
    if (rank > 255) return set_error(RT_ERR_INVALID, "rank must be 0..255");
    if (a->pass_spp < 2 || a->max_spp < a->pass_spp || a->max_spp % a->pass_spp)
        return set_error(RT_ERR_INVALID, "pass_spp must be >= 2 and max_spp a multiple of it");
    if (!(a->threshold >= 0.0) || !(a->eps >= 0.0) || !std::isfinite(a->eps))
        return set_error(RT_ERR_INVALID, "threshold must be >= 0, eps finite and >= 0");
    DEVICE_GUARD(s);
    const uint64_t npx = (uint64_t)p->width * p->height;
    const AdaptiveLayout L = adaptive_layout(frame_tiles(p->width, p->height));
    if (L.bytes > s->adaptive_bytes) {
        if ((rc = ws_idle(s))) return rc;
        if (s->adaptive) (void)hipFree(s->adaptive);
        s->adaptive = nullptr; s->adaptive_bytes = 0;
        HIP_TRY(hipMalloc(&s->adaptive, L.bytes));
        s->adaptive_bytes = L.bytes;
    }
    DevBuf<double> mean, sq;
    DevBuf<uint32_t> count;
    HIP_TRY(mean.alloc(npx * 3));
    HIP_TRY(sq.alloc(npx * 3));
    HIP_TRY(count.alloc(npx));
    EventPair ev;
    HIP_TRY(hipEventCreate(&ev.a));
    HIP_TRY(hipEventCreate(&ev.b));
    HIP_TRY(hipEventRecord(ev.a, 0));
    rt_render_params pass = *p;
    pass.spp = a->pass_spp;
    uint32_t n_list = 0;
    for (uint32_t base = 0; base < a->max_spp; base += a->pass_spp) {
        if ((rc = rt_adaptive_pass_async(s, &pass, s->adaptive, L.bytes, base != 0, n_list, base, nullptr))) return rc;
        if (base + a->pass_spp >= a->max_spp) break;  // the cap: nothing could be selected
        if ((rc = adaptive_select(p->width, p->height, s->adaptive, L.bytes, a->threshold, a->eps, a->pass_spp, a->max_spp,
                                  rank, nullptr)))
            return rc;
        HIP_TRY(hipMemcpy(&n_list, (char*)s->adaptive + L.info, sizeof(n_list), hipMemcpyDeviceToHost));
        if (n_list == 0) break;
    }
    if ((rc = rt_adaptive_resolve_async(p, s->adaptive, L.bytes, mean.p, sq.p, count.p, nullptr))) return rc;
    HIP_TRY(hipEventRecord(ev.b, 0));
    HIP_TRY(hipDeviceSynchronize());
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev.a, ev.b);
    HIP_TRY(hipMemcpy(out_mean_rgb, mean.p, npx * 3 * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_sq_rgb, sq.p, npx * 3 * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<uint32_t> counts;
    if (!out_count && opt_stats) { counts.resize(npx); out_count = counts.data(); }
    if (out_count) HIP_TRY(hipMemcpy(out_count, count.p, npx * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (opt_stats) {
        std::memset(opt_stats, 0, sizeof(*opt_stats));
        for (uint64_t i = 0; i < npx; ++i) opt_stats->paths += out_count[i];
        opt_stats->kernel_ms = ms;
        opt_stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return RT_OK;
}

int rt_render_adaptive(rt_scene* s, const rt_render_params* p, const rt_adaptive_params* a, double* out_mean_rgb,
                       double* out_sq_rgb, uint32_t* out_count, rt_stats* opt_stats) {
    return render_adaptive(s, p, a, -1, out_mean_rgb, out_sq_rgb, out_count, opt_stats);
}

int rt_render_adaptive_rank(rt_scene* s, const rt_render_params* p, const rt_adaptive_params* a, uint32_t rank,
                            double* out_mean_rgb, double* out_sq_rgb, uint32_t* out_count, rt_stats* opt_stats) {
    return render_adaptive(s, p, a, rank > 255 ? 256 : (int)rank, out_mean_rgb, out_sq_rgb, out_count, opt_stats);
}

int rt_intersect_rays(rt_scene* s, const double* rays, uint32_t n, rt_hit* out) {
    if (!s || (!rays && n) || (!out && n)) return set_error(RT_ERR_INVALID, "bad arguments");
    if (n == 0) return RT_OK;
    DEVICE_GUARD(s);
    int rc = ensure_spill(s, ((uint64_t)n + 255) / 256 * 256);
    if (rc) return rc;
    DevBuf<double> r;
    DevBuf<rt_hit> h;
    HIP_TRY(r.alloc((size_t)n * 6));
    HIP_TRY(h.alloc(n));
    HIP_TRY(hipMemcpy(r.p, rays, (size_t)n * 6 * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(ws_begin(s, 0));
    HIP_TRY(launch_intersect(s->dev, r.p, n, h.p, s->spill_n, s->spill_t, 0));
    HIP_TRY(ws_end(s, 0));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, h.p, (size_t)n * sizeof(rt_hit), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_intersect_rays_async(rt_scene* s, const double* d_rays, uint32_t n, rt_hit* d_out, int method,
                            void* hip_stream) {
    if (!s || (!d_rays && n) || (!d_out && n)) return set_error(RT_ERR_INVALID, "bad arguments");
#ifdef RT_WF_PROBE
    if (method == 2) {  // experiment: the traversal-only kernel (render.hip trace_tri_kernel)
        if (n == 0) return RT_OK;
        DEVICE_GUARD(s);
        if (!s->dev.tris.cnodes || path_kinds(s) != 2) return set_error(RT_ERR_INVALID, "probe: compact triangles only");
        uint32_t grid = 0;
        HIP_TRY(trace_tri_grid(n, &grid));
        int rc = ensure_spill(s, (uint64_t)grid * 64);
        if (rc) return rc;
        if (!s->queue) HIP_TRY(hipMalloc(&s->queue, kQueueWords * sizeof(uint32_t)));
        const hipStream_t st = (hipStream_t)hip_stream;
        HIP_TRY(ws_begin(s, st));
        HIP_TRY(launch_trace_tri(s->dev, d_rays, n, d_out, s->queue, s->spill_n, s->spill_t, grid, st));
        HIP_TRY(ws_end(s, st));
        return RT_OK;
    }
#endif
    if (method != RT_TRACE_PER_RAY && method != RT_TRACE_PERSISTENT) return set_error(RT_ERR_INVALID, "bad method");
    if (n == 0) return RT_OK;
    DEVICE_GUARD(s);
    const hipStream_t st = (hipStream_t)hip_stream;
    if (method == RT_TRACE_PER_RAY) {
        int rc = ensure_spill(s, ((uint64_t)n + 255) / 256 * 256);
        if (rc) return rc;
        HIP_TRY(ws_begin(s, st));
        HIP_TRY(launch_intersect(s->dev, d_rays, n, d_out, s->spill_n, s->spill_t, st));
        HIP_TRY(ws_end(s, st));
        return RT_OK;
    }
    uint32_t grid = 0;
    HIP_TRY(trace_grid(n, &grid));
    // the ray counter may run past n by one refill per wave: keep it in 32 bits
    if ((uint64_t)n + (uint64_t)grid * 64 >= (1ull << 32)) return set_error(RT_ERR_INVALID, "too many rays");
    int rc = ensure_spill(s, (uint64_t)grid * 64);
    if (rc) return rc;
    if (!s->queue) HIP_TRY(hipMalloc(&s->queue, kQueueWords * sizeof(uint32_t)));
    HIP_TRY(ws_begin(s, st));
    // the persistent form reads the compact triangle layout's pair lines, or its 64-B nodes, or the
    // f64 layout, as rt_tuning.compact says (auto: the pair lines when the scene has them)
    HIP_TRY(launch_trace(s->dev, d_rays, n, d_out, s->queue, s->spill_n, s->spill_t, grid,
                         s->tune.compact == 0 ? 0 : (s->tune.compact == 1 ? 1 : 2), st));
    HIP_TRY(ws_end(s, st));
    return RT_OK;
}

static int light_query(rt_scene* s, const double* rays, uint32_t n, int mode, double* out, uint32_t* cnt) {
    if (!s || (!rays && n) || (!out && n)) return set_error(RT_ERR_INVALID, "bad arguments");
    if (n == 0) return RT_OK;
    DEVICE_GUARD(s);
    int rc = ensure_spill(s, ((uint64_t)n + 255) / 256 * 256);
    if (rc) return rc;
    DevBuf<double> r, o;
    DevBuf<uint32_t> c;
    HIP_TRY(r.alloc((size_t)n * 6));
    HIP_TRY(o.alloc(n));
    if (cnt) HIP_TRY(c.alloc(n));
    HIP_TRY(hipMemcpy(r.p, rays, (size_t)n * 6 * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(ws_begin(s, 0));
    HIP_TRY(launch_light(s->dev, r.p, n, mode, o.p, cnt ? c.p : nullptr, s->spill_n, s->spill_t, 0));
    HIP_TRY(ws_end(s, 0));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, o.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    if (cnt) HIP_TRY(hipMemcpy(cnt, c.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_light_pdf_rays(rt_scene* s, const double* pos_dir, uint32_t n, double* out_pdf) {
    return light_query(s, pos_dir, n, 1, out_pdf, nullptr);
}

// Extra query (not in the reference's call graph as a batch): the raw
// intersect_lights accumulation of Light::pdf without the epsilon offset and
// the 1/len normalisation, plus the number of callbacks.  Used by the
// triangle::aaa known-answer test (primitives/triangle.rs:98-128).
int rt_intersect_lights_rays(rt_scene* s, const double* rays, uint32_t n, double* out_impact, uint32_t* out_count) {
    return light_query(s, rays, n, 0, out_impact, out_count);
}

// rt_bvh_build and rt_bvh_build_device: on_device null = the host builder
static int bvh_build_out(const double* boxes, uint64_t n, uint32_t max_levels, uint64_t* n_nodes, int64_t* out_links,
                         double* out_bounds, uint64_t* out_order, uint32_t* out_depth, uint32_t* on_device) {
    if ((!boxes && n) || !n_nodes) return set_error(RT_ERR_INVALID, "boxes/n_nodes is NULL");
    std::vector<Box3> b(n);
    for (uint64_t i = 0; i < n; ++i) b[i] = Box3{load3(boxes + 6 * i), load3(boxes + 6 * i + 3)};
    HostBvh h;
    int made = kDeviceBuildFallback;
    if (on_device) {
        std::string err;
        made = build_bvh_device(b, max_levels, h, err);
        if (made == kDeviceBuildError) return set_error(RT_ERR_DEVICE, err);
        *on_device = made == kDeviceBuildDone;
    }
    if (made != kDeviceBuildDone) h = build_bvh(b);
    if (out_links && *n_nodes < h.nodes.size()) return set_error(RT_ERR_INVALID, "output too small");
    *n_nodes = h.nodes.size();
    if (out_depth) *out_depth = h.depth;
    if (!out_links) return RT_OK;
    for (size_t i = 0; i < h.nodes.size(); ++i) {
        const HostNode& nd = h.nodes[i];
        out_links[4 * i] = nd.left; out_links[4 * i + 1] = nd.right;
        out_links[4 * i + 2] = (int64_t)nd.start; out_links[4 * i + 3] = (int64_t)nd.end;
        if (out_bounds) { store3(out_bounds + 6 * i, nd.box.min); store3(out_bounds + 6 * i + 3, nd.box.max); }
    }
    if (out_order) for (uint64_t i = 0; i < n; ++i) out_order[i] = h.order[i];
    return RT_OK;
}

int rt_bvh_build(const double* boxes, uint64_t n, uint64_t* n_nodes, int64_t* out_links, double* out_bounds,
                 uint64_t* out_order, uint32_t* out_depth) {
    return bvh_build_out(boxes, n, 0, n_nodes, out_links, out_bounds, out_order, out_depth, nullptr);
}
int rt_bvh_build_device(const double* boxes, uint64_t n, uint32_t max_levels, uint64_t* n_nodes, int64_t* out_links,
                        double* out_bounds, uint64_t* out_order, uint32_t* out_depth, uint32_t* on_device) {
    if (!on_device) return set_error(RT_ERR_INVALID, "on_device is NULL");
    return bvh_build_out(boxes, n, max_levels, n_nodes, out_links, out_bounds, out_order, out_depth, on_device);
}

// Diagnostic: device f64 sqrt (op 0), division (op 1), the split division
// dev_quot(a, b, dev_rcp(b)) (op 2), dev_sqrt(a) (op 3), dev_inv_len(a)
// (op 4) and dev_quotf(a, b, dev_rcp(b)) (op 5) for bit-exactness checks.
int rt_probe_fp64(int op, const double* a, const double* b, uint32_t n, double* out) {
    const bool two = op == 1 || op == 2 || op == 5;
    if (!a || !out || (two && !b) || op < 0 || op > 5) return set_error(RT_ERR_INVALID, "bad arguments");
    if (n == 0) return RT_OK;
    DevBuf<double> da, db, dout;
    HIP_TRY(da.alloc(n));
    HIP_TRY(db.alloc(n));
    HIP_TRY(dout.alloc(n));
    HIP_TRY(hipMemcpy(da.p, a, n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(db.p, two ? b : a, n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(launch_fp64_probe(da.p, db.p, dout.p, n, op, 0));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dout.p, n * sizeof(double), hipMemcpyDeviceToHost));
    return RT_OK;
}

}  // extern "C"

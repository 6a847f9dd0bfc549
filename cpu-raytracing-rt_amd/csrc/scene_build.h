// scene_build.h — host-side Scene::new / make_scenes / BVH::new
// (scene.rs:92-223, bvh.rs:11-140, 224-256) producing the flattened HBM
// layout of rt_layout.h.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/rt_api.h"
#include "rt_layout.h"
#include "rt_math.h"
#include "tri_items.h"

struct rt_parsed_scene;

namespace rt {

// One BVH in host form: pre-order nodes + primitive permutation.
struct HostNode {
    Box3 box;
    int64_t left = -1, right = -1;
    uint64_t start = 0, end = 0;
};
struct HostBvh {
    std::vector<HostNode> nodes;
    std::vector<uint64_t> order;   // order[i] = list index of the i-th primitive in BVH order
    uint32_t depth = 0;
};
// BVH::new over primitive boxes given in list order (bvh.rs:12-17).
HostBvh build_bvh(const std::vector<Box3>& boxes);

// bvh_build.hip: build_bvh on the current HIP device, the same tree byte for byte.
// kDeviceBuildFallback: nothing was built and the caller runs build_bvh — a coordinate
// is NaN, infinite or above 2^480 in magnitude (up to there every SAH score of up to
// 2^30 boxes is finite, whatever the boxes' signs, so no NaN reaches a comparison and
// box_extend stays associative), the tree has more than max_levels levels, there are
// no or more than 2^30 boxes, or the scratch (about 0.7 kB per box) does not fit.
// kDeviceBuildError: a HIP call failed or no device is visible; err says which.
enum { kDeviceBuildError = -1, kDeviceBuildFallback = 0, kDeviceBuildDone = 1 };
// The default max_levels.  A level is a fixed number of launches over all boxes, so the
// cap bounds what a degenerate one-primitive-per-level tree can cost; a full-sweep SAH
// tree over n boxes in leaves of <= 4 has at least log2(n / 4) levels (22 at 10M) and
// scenes with clustered geometry reach two to three times that, so 128 leaves a wide margin.
constexpr uint32_t kDeviceBuildMaxLevels = 128;
int build_bvh_device(const std::vector<Box3>& boxes, uint32_t max_levels, HostBvh& out, std::string& err);

// Triangle j of the description (arrays and material index already checked) as
// build_scene's item: tri_items.h's arithmetic, mat and gid.  The device's fix-up list
// (tri_items.hip) recomputes its items with this too.
inline void tri_item_of(const rt_scene_desc& d, uint64_t j, TriItem& it) {
    const double* v = d.tri_vertices + 9 * j;
    it.mat = d.tri_material[j];
    it.gid = (int32_t)(d.n_shapes + j);
    if (d.tri_mode == RT_TRI_GLTF) {
        const double* nn = d.tri_normals + 9 * j;
        tri_item_gltf(load3(v), load3(v + 3), load3(v + 6), load3(nn), load3(nn + 3), load3(nn + 6), it);
    } else {
        const V3 pos = d.tri_position ? load3(d.tri_position + 3 * j) : v3(0, 0, 0);
        const Quat rot = d.tri_rotation ? load_quat(d.tri_rotation + 4 * j) : Quat{1.0, v3(0, 0, 0)};
        tri_item_custom(load3(v), load3(v + 3), load3(v + 6), pos, rot, it);
    }
}

// The arrays of a triangle BVH that bvh_emit.hip wrote on the device, in upload_bvh's
// order: nodes, tris, tri_cold, tri_inv_area, mat, gid, cnodes, ctris, pnodes (null and 0
// where the host vector would be empty).  Owns them until api.cpp adopts them into the scene.
enum { kResNodes, kResTris, kResCold, kResInvArea, kResMat, kResGid, kResCnodes, kResCtris, kResPnodes, kResArrays };
struct DevResident {
    bool on = false;
    mutable void* ptr[kResArrays] = {};  // adoption (api.cpp upload_bvh) takes the pointer and nulls it
    uint64_t count[kResArrays] = {};     // elements
    DevResident() = default;
    DevResident(const DevResident&) = delete;
    DevResident& operator=(const DevResident&) = delete;
    ~DevResident() { reset(); }
    void (*release)(void*) = nullptr;    // set by the emitter (hipFree); the host sources link without HIP
    void reset() {                       // frees what was not adopted
        for (void*& p : ptr) {
            if (p && release) release(p);
            p = nullptr;
        }
        for (uint64_t& c : count) c = 0;
        on = false;
    }
};

// Flattened scene ready for upload: every array is a host vector that maps
// 1:1 onto a device allocation (see api.cpp), or, for a triangle BVH emitted on the
// device, an allocation that already exists (dev.on; the vectors are then empty).
struct HostBvhArrays {
    DevResident dev;
    uint64_t count(int k, size_t host_size) const { return dev.on ? dev.count[k] : host_size; }
    uint64_t n_nodes() const { return count(kResNodes, nodes.size()); }
    std::vector<DevNode> nodes;
    Box3 root;
    uint32_t n_prims = 0, depth = 0;
    bool fast = false;  // all box coordinates pass coord_fast (DevBvh::fast)
    bool tri_q = false;  // every triangle edge component 0 or in [2^-149, 2^129) (DevBvh::tri_q)
    std::vector<DevShape> shapes;
    std::vector<DevTri> tris;
    std::vector<DevTriCold> tri_cold;
    std::vector<double> tri_inv_area;
    std::vector<uint32_t> mat;
    std::vector<int32_t> gid;
    // compact layout of a triangle BVH (rt_layout.h DevNodeC, kTriC floats per
    // triangle): filled only when every box coordinate and vertex is an exact f32
    std::vector<DevNodeC> cnodes;
    std::vector<float> ctris;
    // pair layout over the compact nodes (rt_layout.h kPairFloats per internal slot),
    // filled when every internal child's box is the union of its children's
    std::vector<float> pnodes;
};
struct HostScene {
    std::vector<DevMaterial> mats;
    std::vector<DevShape> planes;
    std::vector<uint32_t> plane_mat;
    std::vector<int32_t> plane_gid;
    HostBvhArrays bvh[6];   // boxes, ellipsoids, triangles, light boxes, light ellipsoids, light triangles
    double build_ms = 0.0;
    bool device_built = false;  // a triangle BVH came from build_bvh_device
    bool device_records = false;  // a triangle BVH's arrays came from emit_tri_bvh_device
    bool device_items = false;  // ... emitted from items computed on the device (tri_items.hip)
    bool device_meshes = false;  // ... from items flattened there from glTF accessor bytes (gltf_items.hip)
};
// tri_build: makes the two triangle BVHs and returns as build_bvh_device does (the host
// builder runs on kDeviceBuildFallback); null: the host builder.  The small shape BVHs
// are always the host's.
using TriBvhBuild = int (*)(const std::vector<Box3>& boxes, HostBvh& out, std::string& err);
// tri_emit: builds one non-empty triangle BVH and writes its final arrays on the device
// (out.dev), returning as build_bvh_device does; on kDeviceBuildFallback that BVH takes the
// host path.  compact: also the compact and pair layouts where build_compact would make them.
using TriBvhEmit = int (*)(const std::vector<TriItem>& items, bool compact, HostBvhArrays& out, std::string& err);
// bvh_emit.hip: the TriBvhEmit of the current HIP device (max_levels as build_bvh_device).
int emit_tri_bvh_device(const std::vector<TriItem>& items, bool compact, uint32_t max_levels, HostBvhArrays& out,
                        std::string& err);
// tri_items: computes the items of all the description's triangles (n_triangles > 0, arrays
// and material indices checked) on the device and emits both triangle BVHs from them.
// made[0] is bvh[2]'s outcome (tris, with the compact layouts), made[1] bvh[5]'s (ltris),
// each as build_bvh_device returns; a BVH left at kDeviceBuildFallback takes the tri_emit /
// tri_build / host chain with items computed on the host.  n_light: the number of light
// triangles, or UINT64_MAX where the device did not get to count them.
struct TriItemsOutcome { int made[2] = {kDeviceBuildFallback, kDeviceBuildFallback}; uint64_t n_light = UINT64_MAX; };
using TriBvhItems = int (*)(const rt_scene_desc& desc, HostBvhArrays& tris, HostBvhArrays& ltris, TriItemsOutcome& res,
                            std::string& err);
// tri_items.hip: the TriBvhItems of the current HIP device.
int emit_tri_bvhs_device_items(const rt_scene_desc& desc, uint32_t max_levels, HostBvhArrays& tris,
                               HostBvhArrays& ltris, TriItemsOutcome& res, std::string& err);
// gltf_items.hip: the mesh stage of the current HIP device, for a deferred glTF parse: gf_scan
// and gf_items go from the buffers' bytes and the draw plan to the items, then tri_items.hip's tail.
int emit_tri_bvhs_device_meshes(const rt_parsed_scene& ps, uint32_t max_levels, HostBvhArrays& tris,
                                HostBvhArrays& ltris, TriItemsOutcome& res, std::string& err);
// tri_meshes: the stage before the items, for a deferred glTF parse.  build_scene is then
// given the description without its triangle arrays (materials, n_triangles, tri_mode).
// run flattens the meshes on the device and emits both triangle BVHs from the items, as a
// TriBvhItems returns.  arrays fills in desc's triangle arrays (the host flatten, made on
// first use) for whatever the device left to the host; false: err is the flatten's error.
struct TriMeshStage {
    void* ctx;
    int (*run)(void* ctx, HostBvhArrays& tris, HostBvhArrays& ltris, TriItemsOutcome& res, std::string& err);
    bool (*arrays)(void* ctx, rt_scene_desc& desc, std::string& err);
};
// Returns empty string on success, else an error message.
std::string build_scene(const rt_scene_desc& desc, HostScene& out, TriBvhBuild tri_build = nullptr,
                        TriBvhEmit tri_emit = nullptr, TriBvhItems tri_items = nullptr,
                        const TriMeshStage* tri_meshes = nullptr);

}  // namespace rt

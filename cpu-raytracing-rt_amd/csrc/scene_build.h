// scene_build.h — host-side Scene::new / make_scenes / BVH::new
// (scene.rs:92-223, bvh.rs:11-140, 224-256) producing the flattened HBM
// layout of rt_layout.h.
#pragma once
#include <stdint.h>

#include <string>
#include <type_traits>
#include <vector>

#include "../../include/rt_api.h"
#include "rt_layout.h"
#include "rt_math.h"

namespace rt {

struct Triangle {            // triangle.rs:5-17
    V3 a, ba, ca, ng;
    double inv_area;
    V3 na, nb, nc;
};
Triangle triangle_props(V3 a, V3 b, V3 c);                          // triangle.rs:41-47
Triangle triangle_smooth(V3 a, V3 b, V3 c, V3 na, V3 nb, V3 nc);    // triangle.rs:20-23
Triangle triangle_geometric(V3 a, V3 b, V3 c);                      // triangle.rs:25-28

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

// One triangle of the scene in list order, as build_scene computes it.  bvh_emit.hip
// uploads the vector as it is and reads the records by 16-byte loads, hence the alignment.
struct alignas(16) TriItem { Triangle t; V3 b, c; uint32_t mat; int32_t gid; Box3 box; };  // b, c: the vertices t was built from
static_assert(sizeof(TriItem) == 288 && std::is_trivially_copyable<TriItem>::value && std::is_standard_layout<TriItem>::value,
              "TriItem is a POD of 36 eight-byte words (bvh_emit.hip indexes them)");

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
// Returns empty string on success, else an error message.
std::string build_scene(const rt_scene_desc& desc, HostScene& out, TriBvhBuild tri_build = nullptr,
                        TriBvhEmit tri_emit = nullptr);

}  // namespace rt

// api_internal.h — shared internals of the C ABI implementation.
#pragma once
#include <string>
#include <vector>

#include "../../include/rt_api.h"
#include "gltf_math.h"

namespace rt {

int set_error(int code, const std::string& msg);  // records rt_last_error, returns code

// post.cpp: the 255 byte thresholds of the gamma + PPM quantisation on a
// tonemapped value, derived from the host pow and proven exact; false if the
// proof fails (the device epilogue then uses its own pow).
bool byte_thresholds(double thr[255]);

struct HostScene;
// rt_scene_create in two halves (api.cpp): the host build (six BVHs, flattened
// records) and the upload of that build to the current HIP device, so a
// multi-GPU frame (multi.cpp) builds once and uploads one replica per device.
int scene_build_host(const rt_scene_desc& desc, HostScene& hs, uint32_t build_flags = 0);  // RT_BUILD_*
// scene_build_host for a deferred glTF parse with RT_BUILD_DEVICE_MESHES: the meshes are
// flattened on the device, the description is made only for what falls back to the host.
int scene_build_parsed(const rt_parsed_scene& ps, HostScene& hs, uint32_t build_flags);
int scene_upload(const HostScene& hs, rt_scene** out, bool replica);
// A scene's device arrays in allocation order (with their sizes): a replica built
// from the same HostScene allocates the same sequence, so array k of the replica
// is filled from array k of the source (multi.cpp: ncclBroadcast or peer copies).
const std::vector<void*>& scene_allocs(const rt_scene* s, const std::vector<size_t>** bytes);
void scene_add_upload_ms(rt_scene* s, double ms);  // the replica's device-to-device fill time

// gltf.cpp.  The description of a deferred parse, made on first use by the host flatten over
// the draw plan and cached, error included: RT_OK, or the code and message the eager load
// would have reported (index out of range, non-affine transform).
int parsed_materialise(const rt_parsed_scene* ps);
struct TriItem;
// Triangle j of a deferred parse as build_scene's item (the three vertices through
// gltf_math.h, then tri_item_gltf; mat and gid): the device's fix-up list recomputes with it.
void gltf_item_of(const rt_parsed_scene& ps, uint32_t j, TriItem& it);

}  // namespace rt

// Host-side parse result of the input surfaces (custom text / glTF).
struct rt_parsed_scene {
    std::vector<rt_material> mats;
    std::vector<rt_shape> shapes;
    std::vector<double> tri_v, tri_n, tri_pos, tri_rot;
    std::vector<uint32_t> tri_mat;
    uint32_t tri_mode = RT_TRI_CUSTOM;
    rt_render_params params{};
    // rt_load_gltf_ex with RT_GLTF_DEFER: the draw plan and the buffers' bytes in place of
    // the triangle arrays, which parsed_materialise fills on first use (flat: 0 not yet,
    // 1 done, -1 failed with flat_rc / flat_msg)
    bool deferred = false;
    std::vector<rt::GltfDraw> draws;
    std::vector<std::string> bufs;
    uint64_t n_plan_tris = 0;
    mutable int flat = 0, flat_rc = 0;
    mutable std::string flat_msg;
};

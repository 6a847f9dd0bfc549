/*
 * rt_api.h — C ABI of the MI355X-native path-tracing hot path.
 *
 * Drop-in boundary for uncerso/cpu-raytracing-rt (Rust, CPU).  The reference
 * has no FFI: its only seam is `generate_image(&Scene) -> Image`
 * (src/main.rs:85-114), called once per frame by `main` (src/main.rs:73).
 * Every entry point below names the reference item it replaces.  All
 * signatures are plain C (PODs, pointers, sizes) so a Rust host can bind them
 * with `extern "C"` + `#[repr(C)]`, or Python via ctypes.
 *
 * Conventions
 *  - Return value: 0 (RT_OK) on success, a negative rt_error otherwise.  Nothing
 *    unwinds or aborts across the ABI (the reference panics instead:
 *    src/gltf/scene_builder.rs:58,210,212, src/scene.rs:188).  The message of the
 *    last failure on the calling thread is available from rt_last_error().
 *  - Ownership: the caller owns every host buffer; arrays in descriptors are
 *    BORROWED for the duration of the call.  The library owns device memory
 *    behind opaque handles.
 *  - Numerics: f64 everywhere, like the reference (src/types.rs:5).
 *  - Threading: one host thread per handle (a handle is not re-entrant), as
 *    the reference calls its pixel loop once from the main thread.
 *  - Devices: a scene lives on the device that was current at rt_scene_create.
 *    Every call taking a scene switches to that device for its duration and
 *    restores the caller's current device before returning.
 *  - Streams: launches that use a scene's shared workspace (queue, sample ring,
 *    chunk partials, stack spill) are ordered by the library: each waits for
 *    the previous one on that scene through an event, whatever stream either
 *    was issued on.  Calls on different streams therefore never overlap on one
 *    scene (they serialise); use one scene per stream for concurrency.
 */
#ifndef RT_API_H
#define RT_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_API_VERSION 6

typedef enum rt_error {
    RT_OK = 0,
    RT_ERR_INVALID = -1,     /* bad argument / inconsistent descriptor            */
    RT_ERR_DEVICE = -2,      /* HIP runtime error (no device, launch failure ...) */
    RT_ERR_NOMEM = -3,       /* host or device allocation failed                  */
    RT_ERR_PARSE = -4,       /* scene text / glTF JSON could not be parsed        */
    RT_ERR_IO = -5,          /* file could not be read or written                 */
    RT_ERR_UNSUPPORTED = -6  /* input the reference also rejects (e.g. glTF mode!=4) */
} rt_error;

/* ---- materials: src/scene.rs:6-18 (Material, Metadata) ------------------- */
enum { RT_MAT_DIFFUSE = 0, RT_MAT_METALLIC = 1, RT_MAT_DIELECTRIC = 2 };

typedef struct rt_material {
    uint32_t kind;        /* RT_MAT_*                                         */
    uint32_t _pad;
    double ior;           /* Material::Dielectric(ior); ignored otherwise      */
    double color[3];      /* Metadata::color    (default 0, scene.rs:102)      */
    double emission[3];   /* Metadata::emission (!= 0 => light, scene.rs:225)  */
} rt_material;

/* ---- analytic shapes: src/primitives/{plane,box,ellipsoid}.rs ------------ */
enum { RT_SHAPE_PLANE = 0, RT_SHAPE_BOX = 1, RT_SHAPE_ELLIPSOID = 2 };

typedef struct rt_shape {
    uint32_t type;        /* RT_SHAPE_*                                        */
    uint32_t material;    /* index into rt_scene_desc.materials                */
    double shape[3];      /* plane normal | box half-sizes | ellipsoid radii   */
    double position[3];   /* Primitive::position (default 0, scene.rs:110)     */
    double rotation[4];   /* Primitive::rotation as (s, x, y, z); NOT normalised,
                             exactly as parsed (scene_parser.rs:51-57)         */
} rt_shape;

/* ---- triangles ------------------------------------------------------------ */
enum {
    /* custom-format TRIANGLE: Triangle::new_with_geometry_normals then
       TrianglePrimitive::new (rotate+translate, props recomputed)
       (scene_parser.rs:71-73, scene.rs:139-165)                                */
    RT_TRI_CUSTOM = 0,
    /* glTF: world-space vertices+normals, Triangle::new_with_smooth_normal then
       `instantiate` (AABB of a, a+ba, a+ca) (gltf/scene_builder.rs:42-55,329-356) */
    RT_TRI_GLTF = 1
};

/*
 * Scene description = the reference's parsed scene (parsed_scene.rs:4-75 for
 * the custom format; the flattened triangle list of gltf/scene_builder.rs for
 * glTF).  Shapes and triangles are each in INPUT order; the library splits them
 * per kind preserving relative order and builds the six BVHs exactly as
 * make_scenes does (scene.rs:194-223).  Global primitive id (used by hit-id
 * dumps): shape i -> i, triangle j -> n_shapes + j.
 */
typedef struct rt_scene_desc {
    uint32_t n_materials;
    uint32_t n_shapes;
    uint64_t n_triangles;
    const rt_material* materials;
    const rt_shape* shapes;
    uint32_t tri_mode;              /* RT_TRI_CUSTOM | RT_TRI_GLTF            */
    uint32_t _pad;
    const double* tri_vertices;     /* [n][3][3]: a, b, c                     */
    const double* tri_normals;      /* [n][3][3]: na, nb, nc (GLTF only)      */
    const double* tri_position;     /* [n][3] (CUSTOM only; NULL => 0)        */
    const double* tri_rotation;     /* [n][4] (s,x,y,z) (CUSTOM; NULL => id)  */
    const uint32_t* tri_material;   /* [n]                                    */
} rt_scene_desc;

/* ---- camera: src/scene.rs:36-49 (Fov, CameraParams), src/camera.rs ------- */
enum { RT_FOV_X = 0, RT_FOV_Y = 1 };

/* flags */
#define RT_FLAG_STATS        0x1u  /* fill rt_stats work counters (separate untimed pass) */
#define RT_FLAG_HIT_IDS      0x2u  /* dump (pixel, sample, bounce) -> global primitive id */

typedef struct rt_render_params {
    uint32_t width, height;        /* Scene::dimensions                        */
    uint32_t spp;                  /* Scene::samples                           */
    uint32_t ray_depth;            /* Scene::ray_depth (u8 in the reference)   */
    double bg_color[3];            /* Scene::bg_color                          */
    double cam_position[3];        /* CameraParams (already normalised for the
                                      custom format, scene.rs:169-175)         */
    double cam_right[3], cam_up[3], cam_forward[3];
    uint32_t fov_axis;             /* RT_FOV_X | RT_FOV_Y                      */
    uint32_t flags;                /* RT_FLAG_*                                */
    double fov;                    /* radians                                  */
    uint64_t seed;                 /* counter-based RNG key (replaces the
                                      OS-seeded thread_rng, main.rs:95)        */
} rt_render_params;

/* Work counters of one render (canonical byte model: DESIGN.md §4). */
typedef struct rt_stats {
    uint64_t paths;            /* camera paths = W*H*spp                         */
    uint64_t segments;         /* closest-hit queries (raytrace.rs:14) = samples */
    uint64_t aabb_tests;       /* AABB::intersects calls (aabb.rs:51)            */
    uint64_t tri_tests;        /* Triangle::intersection calls                   */
    uint64_t shape_tests;      /* plane/box/ellipsoid intersection calls         */
    uint64_t shaded_hits;      /* closest hits returned to the integrator        */
    uint64_t light_queries;    /* Light::pdf all-hits queries                    */
    uint64_t light_hits;       /* callbacks of intersect_lights                  */
    double   kernel_ms;        /* device time of the path kernel(s)              */
    double   total_ms;         /* wall time of rt_render incl. copies            */
    uint64_t lane_steps;       /* regeneration-loop steps summed over lanes      */
    uint64_t wave_steps;       /* 64 x (steps of the wave's longest lane): lane  */
                               /* utilisation of the path loop = lane/wave steps */
} rt_stats;

/* Hit-id sentinels in the (pixel, sample, bounce) dump */
#define RT_HIT_MISS      (-1)   /* closest-hit query returned None -> bg_color   */
#define RT_HIT_NONE      (-2)   /* bounce not reached (path ended earlier)       */

/* Ray-query result (intersections.rs:10-16 Intersection + winner id). */
typedef struct rt_hit {
    double t;
    double geometry_normal[3];  /* world space, rotated+normalised (intersections.rs:32-39) */
    double shading_normal[3];
    int32_t inside;
    int32_t prim;               /* global primitive id or RT_HIT_MISS            */
} rt_hit;

typedef struct rt_scene rt_scene;            /* opaque, device-resident       */
typedef struct rt_parsed_scene rt_parsed_scene; /* opaque, host-side parse result */

/* ======================= scene lifetime =================================== */
/* Replaces Scene::new + make_scenes (src/scene.rs:180-223) and BVH::new
   (src/bvh.rs:12-17); uploads the flattened scene to the CURRENT HIP device. */
int  rt_scene_create(const rt_scene_desc* desc, rt_scene** out);
/* rt_scene_create with build flags (0: exactly rt_scene_create).  RT_BUILD_DEVICE: the
   triangle and light-triangle BVHs are built on the current HIP device, the same trees
   byte for byte (rt_bvh_build_device; a BVH it cannot take is built on the host); the
   small shape BVHs stay on the host.  build_ms then covers the device build and the
   copy back.
   RT_BUILD_DEVICE_RECORDS (valid only with RT_BUILD_DEVICE, alone RT_ERR_INVALID): the
   tree stays on the device and the triangle BVHs' arrays (nodes, triangle records, the
   compact and pair layouts) are written there too, into the allocations the scene owns:
   the same bytes as the host's (rt_scene_checksum agrees).  A BVH the device builder
   cannot take, or whose arrays do not fit beside the build's scratch, takes the host
   path, so a scene may mix.  build_ms then covers the device build and the emission;
   upload_ms covers what is still copied from the host (shapes, materials, any host-built
   BVH).
   RT_BUILD_DEVICE_ITEMS (valid only with RT_BUILD_DEVICE | RT_BUILD_DEVICE_RECORDS, else
   RT_ERR_INVALID): the per-triangle items those records are made from (the triangle's
   edges, geometric normal and inverse area, a custom-format triangle's rotation and
   translation, its box) are computed on the device from the description's arrays, which
   are uploaded in place of the finished items; the light-triangle BVH's items are picked
   out of them there.  The same bytes again: a triangle with a NaN among its inputs or
   results is recomputed on the host (up to 65,536 of them; a scene with more computes all
   its items on the host), and a BVH the device path cannot take gets host items and the
   path above.  The argument checks and their messages are the host's. */
#define RT_BUILD_DEVICE 0x1u
#define RT_BUILD_DEVICE_RECORDS 0x2u
#define RT_BUILD_DEVICE_ITEMS 0x4u
int  rt_scene_create_ex(const rt_scene_desc* desc, uint32_t build_flags, rt_scene** out);
/* Scene creation from a parse result.  Without RT_BUILD_DEVICE_MESHES, or on a parse that
   is not deferred (rt_load_gltf_ex, RT_GLTF_DEFER), this is rt_parsed_scene_get +
   rt_scene_create_ex.
   RT_BUILD_DEVICE_MESHES (valid only with the three flags above, else RT_ERR_INVALID; to
   rt_scene_create_ex always RT_ERR_INVALID, a description has no meshes): the glTF meshes
   are flattened on the device.  The referenced buffers are uploaded as they are, with the
   draw plan and a byte per material, and gltf_items.hip goes from accessor bytes to the
   items and boxes of RT_BUILD_DEVICE_ITEMS: no description array is made or uploaded.
   The same bytes again (rt_scene_checksum agrees).  A non-finite POSITION element or an
   index out of range, anywhere in a drawn accessor, sends the scene to the host flatten,
   which reports its error as the eager load does; triangles with a NaN are recomputed on
   the host as above; a BVH the device cannot take gets host items from the description,
   made then.  build_ms covers the buffers' upload, the flatten, the build and the emission. */
#define RT_BUILD_DEVICE_MESHES 0x8u
int  rt_scene_create_parsed(rt_parsed_scene* ps, uint32_t build_flags, rt_scene** out);
void rt_scene_destroy(rt_scene* scene);

typedef struct rt_scene_info {
    uint32_t n_planes, n_boxes, n_ellipsoids;
    uint64_t n_triangles;
    uint32_t n_light_boxes, n_light_ellipsoids;
    uint64_t n_light_triangles;
    uint64_t bvh_nodes[6];       /* boxes, ellipsoids, triangles, light boxes, light ellipsoids, light triangles */
    uint32_t bvh_depth[6];
    double   build_ms;           /* BVH build (host, or device with RT_BUILD_DEVICE; with
                                    RT_BUILD_DEVICE_RECORDS also the record emission, with
                                    RT_BUILD_DEVICE_ITEMS the description's upload too, with
                                    RT_BUILD_DEVICE_MESHES the buffers' upload and the flatten) */
    double   upload_ms;          /* H2D copy of what the host made                 */
    uint64_t device_bytes;       /* the scene's arrays; the per-launch workspace (commit
                                    ring, split-tail row buffer <= 256 MB, chunk partials
                                    <= 4 GiB, stack spill) is grow-only, sized by the
                                    largest frame rendered, and not counted here      */
    /* bit i: scene box i (BVH order) doubles as the next light box, so the light
       pdf of a diffuse bounce comes from the next segment's box tests (DESIGN.md
       §4 "shared light tests"); 0 = separate light queries */
    uint32_t shared_light_mask;
    /* RT_LAYOUT_COMPACT_TRIS: the triangle BVH also has its compact layout (f32
       child boxes and vertices, every one an exact copy of the f64 value; DESIGN.md
       §2), which the resumable triangle-only kernel reads */
    /* RT_LAYOUT_LQ_SKIP: every light is a box whose world bounds the host could
       bound exactly (api.cpp lq_boxes), so the timed kernel may skip
       last-bounce light queries proven NaN-free */
    uint32_t layout_flags;
} rt_scene_info;
#define RT_LAYOUT_COMPACT_TRIS 0x1u
#define RT_LAYOUT_LQ_SKIP      0x2u
/* RT_LAYOUT_PAIR_NODES: the compact triangle BVH also has its pair layout (one 128-B
   line per inner node holding what a visit of either child tests, so a descent reads
   one line per two levels), which the resumable kernel reads when it is
   there (rt_tuning.compact auto or 2) */
#define RT_LAYOUT_PAIR_NODES   0x4u
/* RT_LAYOUT_DEVICE_BUILT: a triangle BVH of the scene was built on the device
   (rt_scene_create_ex with RT_BUILD_DEVICE); the arrays are the host build's */
#define RT_LAYOUT_DEVICE_BUILT 0x8u
/* RT_LAYOUT_DEVICE_RECORDS: at least one triangle BVH's arrays were written on the device
   (RT_BUILD_DEVICE_RECORDS) rather than uploaded; RT_LAYOUT_DEVICE_BUILT is then set too */
#define RT_LAYOUT_DEVICE_RECORDS 0x10u
/* RT_LAYOUT_DEVICE_ITEMS: at least one triangle BVH's arrays were written from items
   computed on the device (RT_BUILD_DEVICE_ITEMS); RT_LAYOUT_DEVICE_RECORDS and
   RT_LAYOUT_DEVICE_BUILT are then set too */
#define RT_LAYOUT_DEVICE_ITEMS 0x20u
/* RT_LAYOUT_DEVICE_MESHES: at least one triangle BVH's arrays were written from items
   flattened on the device from glTF accessor bytes (RT_BUILD_DEVICE_MESHES); the three
   flags above are then set too */
#define RT_LAYOUT_DEVICE_MESHES 0x40u
int rt_scene_get_info(const rt_scene* scene, rt_scene_info* out);
/* Content hash of the scene's device arrays (BVHs, records, materials; not the
   per-launch workspace), computed on the scene's device.  Two handles built from the
   same description — or an rt_multi replica and devices[0]'s scene — hash equal;
   rt_multi_create checks every replica this way after the fill. */
int rt_scene_checksum(rt_scene* scene, uint64_t* out);

/* Kernel form of a scene's renders.  The library picks every
   field from the scene itself ("auto"); a caller may force one for tests and
   tuning.  The library reads no environment variables: the resolved form is a
   property of the scene handle, reported by rt_scene_get_tuning, so every rank
   and process rendering one frame runs the same kernel instance. */
typedef struct rt_tuning {
    uint32_t waves;          /* 0 auto (shape-only scenes 5; else 4 when the BVHs hold > 4096 nodes,
                                else 3); 3, 4 or 5 waves/SIMD (5: the shape-only fused kernel only,
                                other forms run 4 and report it) */
    int32_t  resume;         /* -1 auto (1 for a triangle BVH of > 4096 nodes); 0 fused segment,
                                1 resumable triangle traversal                                          */
    uint32_t kinds;          /* 0 auto (the scene's primitive kinds); 3 the all-kinds instance; 1 or 2
                                only as the scene's own kinds (the value rt_scene_get_tuning reports)   */
    uint32_t suspend_lanes;  /* 0 auto (compact layouts: 24 cache-resident BVH, 48 HBM-streamed; the f64
                                layout: 32 / 48); 1..64                                                 */
    uint32_t leaf_lanes;     /* 0 auto (compact layouts: 16 cache-resident BVH, 12 HBM-streamed; the f64
                                layout: 32 / 28); 1..64                                                 */
    uint32_t chunk_spp;      /* 0 the frame's rule (rt_sample_chunks); else the sample run length,
                                raised if need be to <= 64 runs and <= 4 GiB of partial sums
                                (rt_scene_sample_chunks reports the run length used)                    */
    int32_t  compact;        /* -1 auto (2 when the scene has RT_LAYOUT_PAIR_NODES, else 1 when it
                                has RT_LAYOUT_COMPACT_TRIS); 0 the f64 triangle-BVH layout; 1 the
                                compact one with 64-B nodes (triangle-only resumable kernel;
                                RT_ERR_UNSUPPORTED on a scene without RT_LAYOUT_COMPACT_TRIS); 2 the
                                compact one with its pair layout (RT_LAYOUT_PAIR_NODES)               */
    uint32_t tail_split;     /* 0 auto (8); 1 every wave-tile whole; 2..8: the queue's last wave-tiles
                                (three per resident wave) are handed out in this many parts of
                                consecutive sample rows and summed in sample order after the launch
                                (the same image: DESIGN.md section 5 "per-launch tail")            */
    /* Version 5 replaced version 4's last field (`sorted`, the regrouped-shading kernel) with
       tail_split; version 6 added compact = 2 (the same struct).  Auto is 0 for the unsigned fields and -1 for the signed ones (resume,
       compact): a zero-initialised struct is not all-auto.  NULL restores every field to auto. */
} rt_tuning;
/* NULL restores every field to auto.  Fields out of range -> RT_ERR_INVALID. */
int rt_scene_set_tuning(rt_scene* scene, const rt_tuning* tuning);
/* The form the next render of this scene runs: auto fields resolved (chunk_spp
   stays 0 when the frame's rule applies).  tail_split: after a render, the split that
   frame resolved to (1 when the split cannot apply: sample runs >= 65536 rows or no
   room for a row buffer); before any render since rt_scene_set_tuning, the setting. */
int rt_scene_get_tuning(const rt_scene* scene, rt_tuning* resolved);

/* ======================= the frame (hot path) ============================= */
/* Replaces generate_image's pixel loop (src/main.rs:85-103): for every pixel,
   the mean over spp of raytrace(Camera::fuzzy_ray(px)) (camera.rs:48-55,
   raytrace.rs:8-60).  out_mean_rgb: caller-owned [H][W][3] f64, row-major
   idx = y*W + x (main.rs:96-97), BEFORE aces_tonemap/correct_gamma
   (main.rs:104).  opt_hit_ids: NULL or caller-owned [W*H][spp][ray_depth]
   int32 (requires RT_FLAG_HIT_IDS).  opt_stats: NULL or filled. */
int rt_render(rt_scene* scene, const rt_render_params* params,
              double* out_mean_rgb, int32_t* opt_hit_ids, rt_stats* opt_stats);
/* rt_render + the per-pixel second moment: out_sq_rgb [H][W][3] f64 = (sum over the
   pixel's samples, in the order of the mean's sum, of L * L per channel) / spp (chunked frames,
   rt_scene_sample_chunks: run by run like the mean).  out_mean_rgb is rt_render's, bit
   for bit, and a pixel with a NaN sample is NaN in both.  Both outputs are required.
   RT_FLAG_HIT_IDS / RT_FLAG_STATS: RT_ERR_INVALID (the moments kernel has no such
   form).  opt_stats: NULL, or kernel_ms and total_ms filled, the counters 0. */
int rt_render_moments(rt_scene* scene, const rt_render_params* params, double* out_mean_rgb,
                      double* out_sq_rgb, rt_stats* opt_stats);

/* Multi-GPU tile partition: 16x16 tiles, tile t belongs to
   rank t % world.  Each rank renders its tiles into a packed DEVICE buffer
   [n_tiles_padded][256][3] f64 (n_tiles_padded = ceil(total_tiles/world)),
   asynchronously on `hip_stream` (NULL = default stream). */
#define RT_TILE 16
int rt_tiles_per_rank(const rt_render_params* params, uint32_t world, uint32_t* n_tiles_padded);
/* The scene's per-call workspace (stack spill, chunk partials) is shared;
   successive calls are ordered on it across streams (Conventions: Streams). */
int rt_render_tiles_async(rt_scene* scene, const rt_render_params* params,
                          uint32_t rank, uint32_t world,
                          double* d_tile_rgb, void* hip_stream);
/* rt_render_tiles_async with a second packed buffer of the same shape for the second
   moment (rt_render_moments); both gather and unpack with the existing calls
   (rt_unpack_tiles_async on each).  Flags as rt_render_moments. */
int rt_render_tiles_moments_async(rt_scene* scene, const rt_render_params* params,
                                  uint32_t rank, uint32_t world,
                                  double* d_tile_rgb, double* d_tile_sq, void* hip_stream);
/* Standard error of the mean from a frame's mean and second moment, on the current
   device, stream-ordered.  d_mean, d_sq: [n_pixels][3] f64; d_se: NULL or
   [n_pixels][3]; all 16-byte aligned.  Per value
     se = sqrt(max(sq - mean * mean, 0) / (spp - 1)),
   IEEE sqrt and division, NaN where an input is NaN; spp == 1: +inf (NaN where an
   input is NaN).  d_summary, 8 doubles, over the frame: [0] the pixels with a
   non-finite se or mean in any channel; over the other pixels [1..3] the sum of se
   per channel, [4..6] the sum of the mean per channel, [7] the largest se (0 without
   such a pixel).  The sums have a fixed order that depends on n_pixels alone: the
   same bits on every call and stream.  n_pixels == 0: RT_OK, the summary zeroed.
   Scratch comes from a small per-device pool that orders its users across streams. */
int rt_error_estimate_async(const double* d_mean, const double* d_sq, uint64_t n_pixels, uint32_t spp,
                            double* d_se, double* d_summary, void* hip_stream);
/* rt_error_estimate_async for a frame whose pixels have counts of their own
   (rt_adaptive_resolve_async's d_count): d_count [n_pixels] u32, required, 4-byte aligned.
   Per value se = sqrt(max(sq - mean * mean, 0) / (count_pixel - 1)); count_pixel < 2 is the
   spp == 1 rule, +inf (NaN where an input is NaN), so such a pixel counts in summary [0].
   The summary, its fixed order (the same function of n_pixels), the scratch pool and the
   stream ordering are rt_error_estimate_async's: a uniform count c gives the bytes of spp = c. */
int rt_error_estimate_counts_async(const double* d_mean, const double* d_sq, const uint32_t* d_count,
                                   uint64_t n_pixels, double* d_se, double* d_summary, void* hip_stream);

/* ---- denoiser: a variance-guided a-trous filter (no counterpart in the reference) ----
   The first consumer of the second moment: it smooths where the estimate is uncertain,
   stops at geometric edges, and fills non-finite pixels from their valid neighbours.
   All weights are rational (+ - * / sqrt in a fixed order, IEEE, nothing fused), so the
   output is a pure function of the inputs and parameters: the same bits on every call,
   stream and launch geometry, and the bits of a float64 restatement on the host
   (tests/test_gpu_denoise.py).
   Preparation, per pixel: per channel v_c = max(sq_c - mean_c * mean_c, 0) / (spp - 1)
   (max(d, 0) = d < 0 ? 0 : d, a NaN stays); var = (Lr*Lr*v_r + Lg*Lg*v_g) + Lb*Lb*v_b with
   L = (0.2126, 0.7152, 0.0722); ok = the three mean_c and var all finite.  Guide: hit =
   (prim != RT_HIT_MISS), n = shading_normal, t, x = origin + t * dir (unfused), each
   rounded to f32 and widened back to f64 at every use.
   Iteration i = 0 .. iterations - 1, step s = 2^i: for pixel p the taps q = p + s * (dx, dy),
   dy = -2..2 outer, dx = -2..2 inner, taps outside the image skipped; h = (1/16, 1/4, 3/8,
   1/4, 1/16); lum(c) = (Lr*c_r + Lg*c_g) + Lb*c_b.
     w_g = w_n * w_z when p and q are hits, 1 when both are misses, 0 otherwise;
       w_n = (d < 0 ? 0 : d), d = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z, squared
       normal_squarings times; w_z = 1 / (1 + xz*xz), xz = |(n_p.x*e.x + n_p.y*e.y) +
       n_p.z*e.z| / (sigma_z * t_p), e = x_q - x_p;
     w_l = 1 / (1 + xl*xl), xl = (lum_q - lum_p) / (sigma_l * sqrt(var_p) + eps), when p is ok,
       else 1;
     w = (h[dy] * h[dx]) * (w_g * w_l) when q is ok, else q contributes nothing;
     in tap order sw = sw + w, sc = sc + w * c_q, sv = sv + (w * w) * var_q.
   sw > 0: c'_p = sc / sw, var'_p = sv / (sw * sw), p becomes ok (a missing pixel is filled);
   otherwise c, var and ok of p pass through.  The next iteration reads c', var', ok'. */
#define RT_DENOISE_ITERATIONS       5u
#define RT_DENOISE_NORMAL_SQUARINGS 7u    /* w_n = max(0, n_p . n_q)^128 */
#define RT_DENOISE_SIGMA_L          4.0
#define RT_DENOISE_SIGMA_Z          0.01
#define RT_DENOISE_EPS              1e-8
/* normal_squarings: no squaring at all, w_n = max(0, n_p . n_q) (0 is taken by "default") */
#define RT_DENOISE_SQUARINGS_NONE   0xffffffffu
typedef struct rt_denoise_params {
    uint32_t width, height;
    uint32_t spp;               /* of the frame that made mean and sq; >= 2                  */
    uint32_t iterations;        /* 0 = RT_DENOISE_ITERATIONS; 1..8                           */
    uint32_t normal_squarings;  /* 0 = RT_DENOISE_NORMAL_SQUARINGS; 1..10;
                                   RT_DENOISE_SQUARINGS_NONE = 0 squarings                   */
    uint32_t _pad;
    double sigma_l, sigma_z, eps; /* 0 = RT_DENOISE_SIGMA_L / _SIGMA_Z / _EPS; else finite, > 0 */
} rt_denoise_params;
/* Pixel-centre primary rays of the frame, d_rays [H*W][6] f64 = (cam_position, direction),
   row-major: Camera::fuzzy_ray's arithmetic (camera.rs:48-55) with px + 0.5, py + 0.5 in
   place of the two random draws, normalised as raytrace does (raytrace.rs:9).  The first
   hits of these rays (rt_intersect_rays_async) are the denoiser's guide.  Current device,
   stream-ordered; d_rays 16-byte aligned. */
int rt_camera_rays_async(const rt_render_params* params, double* d_rays, void* hip_stream);
/* Bytes of rt_denoise_async's workspace: 96 B per pixel (two colour buffers {r, g, b, var}
   f64 and the f32 guide), each of the three rounded up to 256 B.  Zero width or height:
   RT_ERR_INVALID. */
int rt_denoise_workspace_bytes(uint32_t width, uint32_t height, uint64_t* bytes);
/* The filter above on the current device, stream-ordered, in caller-owned memory: no hidden
   allocation and no scene handle, so calls on different streams share no state.  d_mean,
   d_sq [H][W][3] f64 (rt_render_moments, or unpacked tiles); d_rays [H*W][6] f64 and d_hits
   [H*W] the first hit of each (rt_camera_rays_async, rt_intersect_rays_async); d_out
   [H][W][3] f64, ready for rt_tonemap_bytes_async; d_out_var NULL or [H][W] f64, the
   filtered var.  All 16-byte aligned.  RT_ERR_INVALID: spp < 2, zero width or height (there
   is no frame), a parameter out of range, a sigma or eps that is negative or not finite, a
   NULL required pointer, a workspace too small or misaligned, d_out or d_out_var
   overlapping an input, the workspace or each other. */
int rt_denoise_async(const rt_denoise_params* p, const double* d_mean, const double* d_sq,
                     const double* d_rays, const rt_hit* d_hits,
                     double* d_out, double* d_out_var /* NULL ok */,
                     void* d_workspace, uint64_t workspace_bytes, void* hip_stream);
/* rt_denoise_async for a frame whose pixels have counts of their own: d_count [H][W] u32,
   required, 4-byte aligned (rt_adaptive_resolve_async's d_count).  p->spp is ignored, any
   value is accepted.  Preparation: v_c = max(sq_c - mean_c * mean_c, 0) / (count - 1) with the
   pixel's count, and ok = count >= 2 && the three mean_c and var all finite, so a pixel with
   too few samples is filled from its neighbours like any other missing pixel.  The filter is
   unchanged: the per-pixel var already carries the count.  RT_ERR_INVALID as
   rt_denoise_async (but for spp), and a d_count that is NULL or overlaps an output. */
int rt_denoise_counts_async(const rt_denoise_params* p, const double* d_mean, const double* d_sq,
                            const uint32_t* d_count, const double* d_rays, const rt_hit* d_hits,
                            double* d_out, double* d_out_var /* NULL ok */,
                            void* d_workspace, uint64_t workspace_bytes, void* hip_stream);

/* ---- adaptive sampling: error-driven passes over a device-built tile list ----
   A frame is rendered in passes of pass_spp samples.  The first pass covers every 16x16 tile;
   after each pass the device measures every tile's error and lists the tiles still above a
   threshold, and the next pass renders only those, continuing each pixel's sample sequence
   where it stopped: a pass at sample base b draws samples [b, b + spp) of its pixels, the
   samples a plain frame of more spp draws (the RNG is keyed by seed, pixel and sample index).
   A tile that received j passes of a samples, each cut into runs of c (rt_scene_sample_chunks
   of a frame of `a` spp; c divides a), holds the sums of a plain frame of j * a spp with runs
   of c, bit for bit: a pass's run sums are added onto the accumulators one by one, in order.
   State, in one caller-owned block (rt_adaptive_workspace_bytes; offsets in rt_adaptive_layout,
   each a multiple of 256), n = tiles_x * tiles_y tiles, tile t = ty * tiles_x + tx:
     acc_sum, acc_sq  [n][256][3] f64  per-pixel sum of L and of L * L, the packed tile layout of
                                       rt_render_tiles_async (pixels outside the image: zeros)
     tile_count       [n] u32          samples every pixel of the tile has received
     tile_err         [n] f64          the tile's error (below); +inf: not measured (count < 2)
     tile_flag        [n] u32          1: the tile has a pixel whose error is not finite
     tile_list        [n] u32          the tiles selected for the next pass, ascending
     info             16 B             {u32 n_list, u32 n_flagged, f64 max_err}
   The error of a pixel with n = tile_count samples, per channel c, IEEE and nothing fused:
     mean_c = sum_c / n, m2_c = sq_c / n, v_c = max(m2_c - mean_c * mean_c, 0) / (n - 1)
     (max(d, 0) = d < 0 ? 0 : d, the denoiser's), var = (Lr*Lr*v_r + Lg*Lg*v_g) + Lb*Lb*v_b,
     lum = (Lr*mean_r + Lg*mean_g) + Lb*mean_b, L the denoiser's, e = sqrt(var) / (lum + eps):
   the standard error of the pixel's luminance relative to the luminance.  A tile's error is
   the largest finite e of its pixels (0 without one).  A pixel whose e is NaN or infinite
   (a NaN sample: more samples cannot repair it) sets tile_flag and holds no tile open.
   eps keeps black pixels finite: with the default a pixel below 1e-3 of display white is
   measured against 1e-3, an absolute floor (a definition, not a tuned number). */
#define RT_ADAPTIVE_EPS 1e-3
typedef struct rt_adaptive_layout {
    uint64_t n_tiles;
    uint64_t acc_sum, acc_sq, tile_count, tile_err, tile_flag, tile_list, info; /* byte offsets */
} rt_adaptive_layout;
typedef struct rt_adaptive_params {
    uint32_t pass_spp;  /* samples a pass adds; >= 2                                   */
    uint32_t max_spp;   /* cap per pixel; a multiple of pass_spp                       */
    double threshold;   /* a tile whose error is <= threshold is done; >= 0, +inf ok   */
    double eps;         /* 0 = RT_ADAPTIVE_EPS; else finite, > 0                       */
} rt_adaptive_params;
/* Bytes of the state above; opt_layout NULL or filled.  Zero width or height: RT_ERR_INVALID. */
int rt_adaptive_workspace_bytes(uint32_t width, uint32_t height, uint64_t* bytes, rt_adaptive_layout* opt_layout);
/* One pass: params->spp (>= 2) samples from sample_base for every tile (use_list == 0) or
   for the first n_list entries of the workspace's tile_list, rendered by the moments kernel
   and added onto the accumulators; tile_count += spp.  A pass at sample_base 0 starts its
   tiles: their accumulators are set, not added to, their count becomes spp and their error
   "not measured", so an all-tiles pass at base 0 initialises a fresh workspace.  A list
   entry >= n_tiles is skipped; an entry that occurs twice is undefined.  Ordered on the
   scene's workspace like every render (Conventions: Streams).  RT_ERR_INVALID: hit-id or
   stats flags, spp < 2, n_list > n_tiles, sample_base + spp > 2^32, a workspace that is NULL,
   too small or not 256-byte aligned.  use_list with n_list == 0: RT_OK, nothing launched. */
int rt_adaptive_pass_async(rt_scene* scene, const rt_render_params* params, void* d_workspace,
                           uint64_t workspace_bytes, int use_list, uint32_t n_list, uint32_t sample_base,
                           void* hip_stream);
/* Measure and select, on the current device, stream-ordered, no scene: tile_err and
   tile_flag of every tile whose count is below max_spp (a tile at the cap keeps what it
   had), then tile_list = the tiles with err > threshold && count + pass_spp <= max_spp in
   ascending order, and info = {their number, the flagged tiles, the largest finite
   tile_err}.  The same bytes on every call and stream.  RT_ERR_INVALID: threshold negative
   or NaN, eps negative or not finite, the workspace as above. */
int rt_adaptive_select_async(uint32_t width, uint32_t height, void* d_workspace, uint64_t workspace_bytes,
                             double threshold, double eps, uint32_t pass_spp, uint32_t max_spp, void* hip_stream);
/* rt_adaptive_select_async in every respect (workspace checks, tiles at the cap, count < 2,
   tile_flag, the list, info, the error codes) except the value written to tile_err, which is
   ranked: one pixel that a rare path lit (e ~ 1 at any count) no longer holds its tile open.
   For each of the tile's 256 packed pixels, e as above and g = e when e is finite and > 0,
   else 0 (pixels outside the image have zero accumulators: g = 0; a non-finite e flags the
   tile as before).  With m the tile's pixels inside the image (from its index, width and
   height) and r = rank * m / 256 in integer arithmetic, so that a ragged tile is not measured
   by a pixel it does not have, tile_err is the (r + 1)-th largest of the 256 values g, counted
   with multiplicity: one of the inputs, unchanged (finite doubles >= 0 order as their bit
   patterns).  rank 0 is rt_adaptive_select_async's maximum, bit for bit; rank 12 is about the
   95th percentile of a full tile.  RT_ERR_INVALID also for rank > 255. */
int rt_adaptive_select_rank_async(uint32_t width, uint32_t height, void* d_workspace, uint64_t workspace_bytes,
                                  double threshold, double eps, uint32_t pass_spp, uint32_t max_spp,
                                  uint32_t rank /* 0..255 */, void* hip_stream);
/* The frame from the state: d_mean, d_sq [H][W][3] f64 = acc / tile_count, d_count NULL or
   [H][W] u32.  d_mean is ready for rt_tonemap_bytes_async; (d_mean, d_sq) are what
   rt_error_estimate_async and rt_denoise_async take only when the count is uniform;
   with d_count they are what rt_error_estimate_counts_async and rt_denoise_counts_async take. */
int rt_adaptive_resolve_async(const rt_render_params* params, const void* d_workspace, uint64_t workspace_bytes,
                              double* d_mean, double* d_sq, uint32_t* d_count /* NULL ok */, void* hip_stream);
/* The loop on the host: a pass over all tiles at base 0; select; read info (16 bytes); a pass
   over the list at base k * pass_spp; ... until the list is empty or max_spp is reached; resolve.
   params->spp is ignored.  out_mean_rgb, out_sq_rgb [H][W][3] f64 required, out_count NULL or
   [H][W] u32.  The state lives in the scene's grow-only workspace.  opt_stats: paths = the
   samples spent, kernel_ms = device time from the first pass to the resolve (the info
   read-backs included), total_ms; the other counters 0. */
int rt_render_adaptive(rt_scene* scene, const rt_render_params* params, const rt_adaptive_params* adaptive,
                       double* out_mean_rgb, double* out_sq_rgb, uint32_t* out_count, rt_stats* opt_stats);
/* The same loop with rt_adaptive_select_rank_async as its select; rank > 255: RT_ERR_INVALID. */
int rt_render_adaptive_rank(rt_scene* scene, const rt_render_params* params, const rt_adaptive_params* adaptive,
                            uint32_t rank, double* out_mean_rgb, double* out_sq_rgb, uint32_t* out_count,
                            rt_stats* opt_stats);

/* ---- image metrics: the distance of a frame to a reference frame (no counterpart in the reference) ----
   What judges the quality pipeline above: A is the frame under test, B a converged frame of the
   same scene, both [H][W][3] in one format.  RT_METRICS_F64: f64 radiance, 8-byte aligned (rows
   need not be 16-byte aligned).  RT_METRICS_U8: display bytes as rt_tonemap_bytes_async writes
   them, each widened exactly to f64.  Like the denoiser it is rational arithmetic (+ - * /) in a
   fixed order, IEEE, nothing fused: the maps are the bits of a float64 restatement on the host
   (tests/test_gpu_metrics.py).
   Per pixel, with L = (0.2126, 0.7152, 0.0722), the denoiser's:
     d_c = a_c - b_c;  se = (d_r*d_r + d_g*d_g) + d_b*d_b;
     rel = (d_r*d_r / (b_r*b_r + eps) + d_g*d_g / (b_g*b_g + eps)) + d_b*d_b / (b_b*b_b + eps);
     ya = (L_r*a_r + L_g*a_g) + L_b*a_b, yb likewise;  the pixel is good when its six inputs are finite.
   SSIM over valid windows only: for 0 <= x <= W - 11 and 0 <= y <= H - 11 there is a window whose
   top-left pixel is (x, y); a frame with W < 11 or H < 11 has none.  The filter is separable over
   the five planes q = (ya, yb, ya*ya, yb*yb, ya*yb), with the taps w[0..10]:
     horizontal  h = w[0]*q(x, r), then h = h + w[i]*q(x + i, r) for i = 1..10;
     vertical    v = w[0]*h(x, y), then v = v + w[j]*h(x, y + j) for j = 1..10.
   With ma = v0, mb = v1: sa = v2 - ma*ma, sb = v3 - mb*mb, sab = v4 - ma*mb, none of them clamped;
   C1 = (0.01*peak)*(0.01*peak), C2 = (0.03*peak)*(0.03*peak);
     ssim = (((2*ma)*mb + C1) * (2*sab + C2)) / (((ma*ma + mb*mb) + C1) * ((sa + sb) + C2)).
   A window that touches a non-finite pixel comes out non-finite by this arithmetic alone (the taps
   are positive: no 0*inf hides one); no flag is carried, a window counts exactly when its ssim is
   finite.
   Summary, 8 doubles: [0] the pixels that are not good; over the good pixels [1] the sum of se,
   [2] the sum of rel, [3] the largest |d_c| (0 without a good pixel); [4] the windows that count,
   [5] the sum of ssim over them, [6] their smallest ssim (+inf without one), [7] the windows that
   do not count.  The sums have a fixed order that depends on (W, H) alone and use no
   floating-point atomics: the same bits on every call and stream.  From it the host derives, with
   good = W*H - [0]: MSE = [1] / (3*good), relMSE = [2] / (3*good), PSNR = 10*log10(peak*peak / MSE),
   mean SSIM = [5] / [4]. */
enum { RT_METRICS_F64 = 0, RT_METRICS_U8 = 1 };
#define RT_METRICS_EPS 1e-2   /* the customary relMSE floor: a definition, not a tuned number */
typedef struct rt_metrics_params {
    uint32_t width, height;
    uint32_t format;      /* RT_METRICS_F64 | RT_METRICS_U8                                    */
    uint32_t _pad;
    double peak;          /* 0 = 1.0 for f64, 255.0 for u8; else finite, > 0                    */
    double eps;           /* 0 = RT_METRICS_EPS; else finite, > 0                               */
    double window[11];    /* the 1-D SSIM taps, all finite and > 0; all zero = rt_ssim_window(1.5, .) */
} rt_metrics_params;
/* Host only: out[i] = exp(-(i - 5)^2 / (2 * sigma^2)), i = 0..10, divided by their sum taken in
   index order.  exp runs here and nowhere else: the device receives the eleven numbers.  sigma
   not finite or <= 0, or out NULL: RT_ERR_INVALID. */
int rt_ssim_window(double sigma, double* out11);
/* Bytes of rt_image_metrics_async's workspace: 8 doubles for every 32x16 block of pixels, rounded
   up to 256 B.  Zero width or height, or one above 65535: RT_ERR_INVALID. */
int rt_image_metrics_workspace_bytes(uint32_t width, uint32_t height, uint64_t* bytes);
/* The metrics above on the current device, stream-ordered, in caller-owned memory: no scene
   handle and no hidden allocation, as rt_denoise_async.  d_a, d_b [H][W][3] in p->format (they
   may be the same frame); d_rel NULL or [H][W] f64, the per-pixel rel; d_ssim NULL or
   [H - 10][W - 10] f64, the per-window ssim (not touched, and NULL is fine, when there is no
   window); d_summary 8 doubles; f64 buffers and the workspace 8-byte aligned.  RT_ERR_INVALID:
   zero width or height (or above 65535), an unknown format, a peak, eps or tap that is negative or
   not finite, a window that mixes zero and non-zero taps, a NULL required pointer, a workspace too
   small or misaligned, an output overlapping an input, the workspace or another output. */
int rt_image_metrics_async(const rt_metrics_params* p, const void* d_a, const void* d_b,
                           double* d_rel /* NULL ok */, double* d_ssim /* NULL ok */, double* d_summary,
                           void* d_workspace, uint64_t workspace_bytes, void* hip_stream);

/* ---- temporal accumulation: frame history reprojected through a camera change (no counterpart in the reference) ----
   The temporal half of SVGF; the denoiser above is the spatial half.  The scene is static and only the
   camera moves: what pixel p of the current frame sees is looked up where the previous camera saw it, and
   the previous frame's (mean, second moment, count) there are merged with p's own, so a surface both
   frames see keeps its samples.  Rational arithmetic (+ - * /, floor, comparisons) in a fixed order, IEEE,
   nothing fused: the outputs are the bits of a float64 restatement on the host
   (tests/test_gpu_temporal.py).  dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z throughout.
   Current frame, per pixel p: n_c = min(d_count ? d_count[p] : spp, 2^30); cur_ok = n_c >= 1 and the
   six values mean_c, sq_c all finite.  Guide, the denoiser's: hit_p = (prim != RT_HIT_MISS), n_p =
   shading_normal, t_p, x_p = origin + t * dir (unfused); n_p, t_p and x_p are rounded to f32 and widened
   back where they are compared with history (the tap tests) and where they are stored.
   Previous camera, on the host: tan_x, tan_y, fw = W, fh = H as the renderer makes them (tan(fov / 2) on
   the fov axis, the other divided by the aspect), and the dual basis of (right, up, forward), which need
   not be orthogonal (the reference normalises each vector alone): with cross(a, b) = (a.y*b.z - a.z*b.y,
   a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x), det = dot(right, cross(up, forward)), r* = cross(up, forward) /
   det, u* = cross(forward, right) / det, f* = cross(right, up) / det, each component divided.  det zero
   or not finite: RT_ERR_INVALID.
   Reprojection, f64, from the unrounded x_p: v = x_p - prev_position; zc = dot(v, f*), xc = dot(v, r*),
   yc = dot(v, u*); gx = ((xc / zc) / tan_x + 1) * 0.5 * fw - 0.5; gy = ((-(yc / zc)) / tan_y + 1) * 0.5 *
   fh - 0.5, evaluated left to right.  p has a candidate when hit_p, zc > 0, -1 <= gx < W and -1 <= gy < H
   (each comparison false for a NaN).  x0 = floor(gx), y0 = floor(gy), ax = gx - x0, ay = gy - y0.
   Taps q = (x0 + i, y0 + j), j = 0, 1 outer, i = 0, 1 inner, weight b = (i ? ax : 1 - ax) * (j ? ay :
   1 - ay).  A tap is valid when it lies inside the image, its history record has count >= 1 and the hit
   flag, dot(n_p, n_q) >= normal_min, and |dot(n_p, x_q - x_p)| <= plane_tol * t_p.  Over the valid taps,
   in tap order: sw = sw + b, sm_c = sm_c + b * mean_q,c, ss_c = ss_c + b * sq_q,c, n_min = min(count_q).
   hist_ok = sw > 0; then h_c = sm_c / sw, hs_c = ss_c / sw, n_h = min(n_min, max_history).
   Merge:  cur_ok and hist_ok: N = n_h + n_c, out_c = ((double)n_h * h_c + (double)n_c * mean_c) /
             (double)N, sq likewise with hs_c, out_count = N;
           only cur_ok: the current values, out_count = n_c;
           only hist_ok: h_c and hs_c (a hole is filled), out_count = n_h;
           neither: the current values as they are (a NaN passes through), out_count = 0.
   New history record of p: the colour is the six outputs; count = out_count, but 0 when any of the six
   is not finite; the guide of p, the hit flag clear for a miss.  Without d_hist_prev every pixel is the
   "no history" case: that is how a sequence starts.
   History: a caller-owned block of rt_temporal_history_bytes bytes, 80 B a pixel in two arrays, each
   rounded up to 256 B: [H][W] guide records of 32 B, {nx, ny, nz, px, py, pz} f32, count u32, flags u32
   (bit 0: hit), then [H][W] colour records of 48 B, mean r, g, b and sq r, g, b as f64.  A call reads
   d_hist_prev and writes d_hist_next; the caller ping-pongs two blocks (taps read arbitrary pixels, so
   the accumulation cannot run in place). */
#define RT_TEMPORAL_MAX_HISTORY (1u << 20)
#define RT_TEMPORAL_NORMAL_MIN  0.9
#define RT_TEMPORAL_PLANE_TOL   0.02
/* every tap straight from global memory: the same bits, without the kernel's LDS window of the history
   (for tests and measurements) */
#define RT_TEMPORAL_NO_WINDOW   0x1u
typedef struct rt_temporal_params {
    uint32_t width, height;
    uint32_t spp;          /* the current frame's samples when d_count is NULL; 1..2^30   */
    uint32_t max_history;  /* cap, in samples, on what history contributes; 0 = default; <= 2^30 */
    uint32_t flags, _pad;
    double normal_min;     /* 0 = default; else finite, in (0, 1]                         */
    double plane_tol;      /* 0 = default; else finite, > 0                                */
} rt_temporal_params;
/* Bytes of one history block.  Zero width or height, or one above 65535: RT_ERR_INVALID. */
int rt_temporal_history_bytes(uint32_t width, uint32_t height, uint64_t* bytes);
/* The accumulation above on the current device, stream-ordered, in caller-owned memory: no scene handle
   and no hidden allocation, so two calls on different streams share nothing.  d_mean, d_sq [H][W][3] f64
   (rt_render_moments, rt_adaptive_resolve_async, or unpacked tiles); d_count NULL or [H][W] u32; d_rays
   [H*W][6] f64 and d_hits [H*W], the current frame's pixel-centre rays and their first hits, as the
   denoiser takes them; prev_camera the camera of the frame that wrote d_hist_prev (its cam_*, fov and
   fov_axis are read; its width and height must be p's).  d_out_mean, d_out_sq [H][W][3] f64 and
   d_out_count [H][W] u32 are what rt_denoise_counts_async and rt_error_estimate_counts_async take.
   RT_ERR_INVALID, all checked before any device call: zero width or height (or above 65535), prev_camera
   without d_hist_prev or the reverse, a prev_camera of another size or with a bad fov_axis, a previous
   basis that is singular or not finite, spp (when d_count is NULL), max_history, flags, normal_min or
   plane_tol out of range, a NULL required pointer, misalignment (f64 buffers and hits 16 bytes, the
   history blocks 256, counts 4), an output or d_hist_next overlapping an input, d_hist_prev or another
   output. */
int rt_temporal_accumulate_async(const rt_temporal_params* p,
        const rt_render_params* prev_camera,        /* NULL iff d_hist_prev is NULL */
        const double* d_mean, const double* d_sq, const uint32_t* d_count /* NULL ok */,
        const double* d_rays, const rt_hit* d_hits,
        const void* d_hist_prev /* NULL: first frame */, void* d_hist_next,
        double* d_out_mean, double* d_out_sq, uint32_t* d_out_count, void* hip_stream);

/* Diagnostics: the scene's raw device counter words (n <= 64), accumulated by
   RT_FLAG_STATS renders: words 0..9 are rt_stats' counters; word 10 counts the
   last-bounce light queries the timed (no-stats) kernel skips because they cannot
   be NaN (the stats render still runs them); words 11..13
   count the inner-node visits of closest-hit BVH traversals whose two child boxes
   were hit by none / one / both slab tests; builds compiled
   with -DRT_PHASES add wave cycles and loop counts per path-kernel region at
   words 16..51 (16 + kPhN - 1, phases.h; tools/phases.py).  Word 14 counts waves
   the stats kernel's progress guard stopped (kStallTrips trips without progress; a
   nonzero word makes rt_render / rt_read_stats return RT_ERR_DEVICE).  Words 52..59
   are the last stats launch's wave timeline (s_memrealtime, 100 MHz; cleared at
   each stats launch, not accumulated; tools/timeline.py): ~earliest start, last
   exit, ~earliest and last time a wave found the wave-tile queue drained, sum and
   max of drain-to-exit, sum of start-to-exit, waves.  Not needed to render. */
int rt_read_raw_stats(rt_scene* scene, uint64_t* out, uint32_t n);

/* Sample chunking of the work units: a pixel's spp samples are
   rendered in `chunks` runs of `chunk_spp` consecutive samples by different
   lanes; each run is summed in sample order from 0, the run sums are added in
   run order and divided by spp.  A function of (width, height, spp) only, so the
   image is identical for any rank count.  chunks == 1 is exactly main.rs:94-104's
   sequential sum; otherwise the result differs from it by f64 reassociation only
   (no replacement for main.rs; exposed so checkers can reproduce the order). */
int rt_sample_chunks(const rt_render_params* params, uint32_t* chunks, uint32_t* chunk_spp);
/* The chunking this scene's renders use: rt_sample_chunks unless its tuning
   forces a run length (rt_tuning.chunk_spp). */
int rt_scene_sample_chunks(const rt_scene* scene, const rt_render_params* params, uint32_t* chunks,
                           uint32_t* chunk_spp);
/* Work counters accumulated on the device by every rt_render_tiles_async call
   made with RT_FLAG_STATS since the last reset (synchronises the device). */
int rt_read_stats(rt_scene* scene, rt_stats* out, int reset);
/* Root side after the gather: d_gathered = [world][n_tiles_padded][256][3]
   (rank-major, as ncclGather lays it out) -> d_image [H][W][3]. */
int rt_unpack_tiles_async(const rt_render_params* params, uint32_t world,
                          const double* d_gathered, double* d_image, void* hip_stream);
/* The same unpack fused with correct_gamma(aces_tonemap(.)) and the PPM byte
   quantisation (main.rs:104, postprocessing.rs:5-37, ppm.rs:13-19): d_bytes is
   the P6 payload [H][W][3] u8, so the f64 image never leaves the device.  The
   bytes are the host path's (rt_tonemap_gamma + rt_save_ppm) bit for bit: the
   device computes aces_tonemap with the same IEEE operations, and the gamma +
   quantisation step is a search over 255 thresholds on the tonemapped value
   that the host derives from its own `pow` (post.cpp byte_thresholds). */
int rt_unpack_tiles_bytes_async(const rt_render_params* params, uint32_t world,
                                const double* d_gathered, uint8_t* d_bytes, void* hip_stream);
/* Device tonemap + gamma + PPM bytes of a mean-radiance image already in HBM
   ([n_pixels][3] f64 -> [n_pixels][3] u8). */
int rt_tonemap_bytes_async(const double* d_rgb, uint64_t n_pixels, uint8_t* d_bytes, void* hip_stream);

/* ======================= one process, several GPUs ======================== */
/* generate_image (src/main.rs:85-114) over several GPUs of one node, driven
   from ONE host thread exactly like rt_render (the Rust `main`, main.rs:73,
   keeps its single call per frame):
    - rt_multi_create builds the six BVHs once on the host (scene.rs:180-223,
      bvh.rs:12-17) and uploads one scene replica per listed device;
    - rt_multi_render deals the frame's 16x16 tiles round-robin (tile t ->
      device index t % n, the rt_render_tiles_async partition), renders every
      share on its own device and stream, makes ONE gather of the packed tiles
      to devices[0] (an RCCL ncclGather over xGMI; peer copies with
      RT_MULTI_PEER), then unpacks on devices[0] and copies the image to the
      host once.
   The image is bit-identical to rt_render's for any device count (the RNG is
   keyed by the global pixel and sample, the chunking by the frame alone).
   out_mean_rgb: NULL or caller-owned [H][W][3] f64 (main.rs:104 before the
   tonemap); out_ppm_bytes: NULL or caller-owned [H][W][3] u8, the P6 payload
   of correct_gamma(aces_tonemap(.)) made on the device (as
   rt_unpack_tiles_bytes_async); at least one is required.  opt_stats: work
   counters summed over the devices (RT_FLAG_STATS), kernel_ms = the slowest
   device's render, total_ms = the call's wall time.
   RCCL is loaded at rt_multi_create (dlopen of librccl.so.1); without it, or
   with a device listed twice, RT_MULTI_PEER is required. */
#define RT_MULTI_PEER 0x1u  /* gather with hipMemcpyPeerAsync instead of RCCL;
                               allows a device listed more than once (several
                               replicas on one GPU: a rehearsal of the N-way
                               partition on a one-GPU machine) */
typedef struct rt_multi rt_multi;
int  rt_multi_create(const rt_scene_desc* desc, const int* devices, uint32_t n_devices, uint32_t flags,
                     rt_multi** out);
int  rt_multi_render(rt_multi* m, const rt_render_params* params, double* out_mean_rgb,
                     uint8_t* out_ppm_bytes, rt_stats* opt_stats);
/* The replica on device index i (0 <= i < n) for per-device queries; owned by m. */
rt_scene* rt_multi_scene(rt_multi* m, uint32_t index);
void rt_multi_destroy(rt_multi* m);

/* ======================= ray queries ====================================== */
/* Closest hit for a batch of world rays [n][6] = (origin, dir) — replaces
   intersections.rs:42-62 `intersect(ray, &scene.primitives, +inf)`. */
int rt_intersect_rays(rt_scene* scene, const double* rays, uint32_t n, rt_hit* out);
/* The same query on device-resident buffers, stream-ordered (no host copies):
   d_rays [n][6] f64 and d_out [n] rt_hit in HBM.  method 0 runs one thread per
   ray; method 1 the persistent traversal (waves refill finished lanes from a
   queue), on the triangle BVH's compact layout when the scene has it and its
   tuning allows (rt_tuning.compact).  Both give identical hits.  Uses the scene's workspace, ordered
   after the scene's previous launch (Conventions: Streams). */
#define RT_TRACE_PER_RAY    0
#define RT_TRACE_PERSISTENT 1
int rt_intersect_rays_async(rt_scene* scene, const double* d_rays, uint32_t n, rt_hit* d_out, int method,
                            void* hip_stream);
/* Light-area pdf for a batch [n][6] = (surface pos, unit dir) — replaces
   ray_sampler.rs:132-139 Light::pdf (all-hits query intersections.rs:87-91). */
int rt_light_pdf_rays(rt_scene* scene, const double* pos_dir, uint32_t n, double* out_pdf);
/* The raw intersect_lights accumulation of Light::pdf for rays [n][6] used as
   given (no EPSILON offset, no 1/len): out_impact = sum over every light
   crossing of p_area * t^2/|d.n_g|; out_count = number of callbacks
   (intersections.rs:87-91; known-answer test primitives/triangle.rs:98-128). */
int rt_intersect_lights_rays(rt_scene* scene, const double* rays, uint32_t n,
                             double* out_impact, uint32_t* out_count);

/* ======================= host BVH builder ================================= */
/* BVH::new (bvh.rs:12-17, build_nodes :75-113) over primitive boxes
   [n][6] = (min xyz, max xyz) given in list order; host only, no device.
   Ties of equal midpoints are broken by list index (deterministic tree).
   Call with out_links == NULL to get *n_nodes; then with buffers of that size:
   out_links [n_nodes][4] = (left, right, start, end) (-1: none), out_bounds
   [n_nodes][6], out_order [n] = list index of the i-th primitive in BVH order. */
int rt_bvh_build(const double* boxes, uint64_t n, uint64_t* n_nodes, int64_t* out_links,
                 double* out_bounds, uint64_t* out_order, uint32_t* out_depth);
/* rt_bvh_build on the current HIP device: the same outputs, byte for byte (a tree has
   at most 2n - 1 nodes, so buffers of that size need no sizing call).  max_levels 0 =
   the library's cap.  *on_device = 1 when the device builder made the tree, 0 when the
   host builder did: a coordinate that is NaN, infinite or above 2^480 in magnitude, a
   tree deeper than max_levels, no or more than 2^30 boxes, or no memory for the scratch. */
int rt_bvh_build_device(const double* boxes, uint64_t n, uint32_t max_levels,
                        uint64_t* n_nodes, int64_t* out_links, double* out_bounds,
                        uint64_t* out_order, uint32_t* out_depth, uint32_t* on_device);

/* ======================= host input surface =============================== */
/* Custom text format (src/scene_parser.rs:5-85, defaults scene.rs:167-191). */
int rt_parse_custom_scene(const char* text, rt_parsed_scene** out);
/* glTF subset (src/gltf/parser.rs, src/gltf/scene_builder.rs:9-22); external
   .bin buffers resolved relative to the .gltf path (main.rs:54-59,77-83). */
int rt_load_gltf(const char* gltf_path, uint32_t width, uint32_t height,
                 uint32_t spp, rt_parsed_scene** out);
/* rt_load_gltf with flags (0: exactly rt_load_gltf).  RT_GLTF_DEFER: the parse does all
   that does not depend on the buffers' elements (the JSON and its checks, materials, node
   transforms, the camera, the buffer files) and, in place of the triangle arrays, records a
   draw plan: per converted primitive the node matrix and its cofactor matrix, where its
   POSITION, NORMAL and index elements lie, its material and its triangles' place in the
   scene.  Where planning meets anything the eager load would report, or an input the
   device flatten does not take (an accessor without a bufferView, a last element past its
   buffer's end, a node matrix whose row 3 is not (0, 0, 0, 1), an offset or stride that is
   no multiple of the component size, more than 2^30 triangles), the call runs the eager
   load instead and returns what that returns.  rt_parsed_scene_get on a deferred parse
   makes the description on first use (the host flatten over the plan, cached); the errors
   that depend on elements (index out of range, non-affine node transform) are reported
   there, with the eager load's code and message. */
#define RT_GLTF_DEFER 0x1u
int rt_load_gltf_ex(const char* gltf_path, uint32_t width, uint32_t height, uint32_t spp,
                    uint32_t flags, rt_parsed_scene** out);
/* Views into the parse result (valid until rt_parsed_scene_free). */
int rt_parsed_scene_get(const rt_parsed_scene* ps, rt_scene_desc* desc,
                        rt_render_params* params);
void rt_parsed_scene_free(rt_parsed_scene* ps);

/* ======================= host output surface ============================== */
/* correct_gamma(aces_tonemap(x)) per pixel (postprocessing.rs:5-37). */
void rt_tonemap_gamma(const double* mean_rgb, uint64_t n_pixels, double* out_rgb);
/* Binary P6 PPM of an already tonemapped image (ppm.rs:4-19). */
int rt_save_ppm(const char* path, uint32_t width, uint32_t height, const double* rgb);
/* The device epilogue's table (host only): out[k-1] = the least tonemapped
   value a >= 0 whose PPM byte round(clamp(pow(a, 1/2.2))*255) is >= k, k =
   1..255, derived from this library's host pow and proven exact
   (RT_ERR_UNSUPPORTED if the proof fails). */
int rt_byte_thresholds(double* out255);

/* ======================= misc ============================================= */
const char* rt_last_error(void);
int rt_api_version(void);
/* Number of visible HIP devices (0 when none); never fails. */
int rt_device_count(void);
/* Diagnostic: device f64 sqrt (op 0), a/b (op 1), or the kernels' forms
   (rt_device.h): the split division dev_quot(a, b, dev_rcp(b)) (op 2), dev_sqrt(a)
   (op 3), dev_inv_len(a) = 1/sqrt(a) (op 4) and dev_quotf(a, b, dev_rcp(b)) (op 5,
   the split division with the signed-zero fixup), for n values, to check that the
   device rounds like the host (the bit-exact parity premise).
   b is read for ops 1, 2 and 5 only. */
int rt_probe_fp64(int op, const double* a, const double* b, uint32_t n, double* out);

#ifdef __cplusplus
}
#endif
#endif /* RT_API_H */

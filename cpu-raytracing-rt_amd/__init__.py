"""MI355X-native path-tracing hot path of uncerso/cpu-raytracing-rt — host side.

Python mirror of the reference's frame-level interface over the C ABI in
``include/rt_api.h`` (``build/librt_amd.so``, HIP kernels for gfx950):

=====================================  ==========================================
reference (Rust, /root/reference/src)  here
=====================================  ==========================================
scene_parser::parse_scene (:5-43)      :func:`parse_scene` (text -> ParsedScene)
gltf::parse + gltf::build_scene        :func:`load_gltf`
Scene::new / make_scenes (scene.rs)    :class:`Scene` (device-resident, BVHs built)
generate_image (main.rs:85-114)        :meth:`Scene.generate_image` (mean radiance),
                                       :func:`generate_image` (tonemapped like main.rs:104)
intersect (intersections.rs:42-62)     :meth:`Scene.intersect`
Light::pdf (ray_sampler.rs:132-139)    :meth:`Scene.light_pdf`
aces_tonemap/correct_gamma             :func:`tonemap_gamma`
ppm::save_to_ppm (ppm.rs:4-11)         :func:`save_to_ppm`
=====================================  ==========================================

There is no CPU fallback: loading fails loudly if the shared library is
missing, and every render call fails with ``RtError`` when no HIP device is
visible.  The package directory name contains dashes, so import it with
``importlib`` (see ``tests/conftest.py``) or ``__graft_entry__``.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# RT_AMD_LIB: alternate build of the same library (tuning experiments only)
LIB_PATH = os.environ.get("RT_AMD_LIB") or os.path.join(_HERE, "build", "librt_amd.so")

# ----------------------------------------------------------------- ABI ----
RT_MAT_DIFFUSE, RT_MAT_METALLIC, RT_MAT_DIELECTRIC = 0, 1, 2
RT_SHAPE_PLANE, RT_SHAPE_BOX, RT_SHAPE_ELLIPSOID = 0, 1, 2
RT_TRI_CUSTOM, RT_TRI_GLTF = 0, 1
RT_FOV_X, RT_FOV_Y = 0, 1
RT_FLAG_STATS, RT_FLAG_HIT_IDS = 0x1, 0x2
RT_HIT_MISS, RT_HIT_NONE = -1, -2
# rt_denoise_params: what a zeroed field means, and the value of normal_squarings for no squaring at all
RT_DENOISE_ITERATIONS, RT_DENOISE_NORMAL_SQUARINGS = 5, 7
RT_DENOISE_SIGMA_L, RT_DENOISE_SIGMA_Z, RT_DENOISE_EPS = 4.0, 0.01, 1e-8
RT_DENOISE_SQUARINGS_NONE = 0xFFFFFFFF
RT_METRICS_F64, RT_METRICS_U8 = 0, 1
RT_METRICS_EPS = 1e-2
RT_TEMPORAL_MAX_HISTORY, RT_TEMPORAL_NORMAL_MIN, RT_TEMPORAL_PLANE_TOL = 1 << 20, 0.9, 0.02
RT_TEMPORAL_NO_WINDOW = 0x1
RT_TILE = 16
ERRORS = {0: "OK", -1: "INVALID", -2: "DEVICE", -3: "NOMEM", -4: "PARSE", -5: "IO", -6: "UNSUPPORTED"}
(RT_OK, RT_ERR_INVALID, RT_ERR_DEVICE, RT_ERR_NOMEM, RT_ERR_PARSE, RT_ERR_IO,
 RT_ERR_UNSUPPORTED) = 0, -1, -2, -3, -4, -5, -6


class rt_material(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("_pad", C.c_uint32), ("ior", C.c_double),
                ("color", C.c_double * 3), ("emission", C.c_double * 3)]


class rt_shape(C.Structure):
    _fields_ = [("type", C.c_uint32), ("material", C.c_uint32), ("shape", C.c_double * 3),
                ("position", C.c_double * 3), ("rotation", C.c_double * 4)]


class rt_scene_desc(C.Structure):
    _fields_ = [("n_materials", C.c_uint32), ("n_shapes", C.c_uint32), ("n_triangles", C.c_uint64),
                ("materials", C.POINTER(rt_material)), ("shapes", C.POINTER(rt_shape)),
                ("tri_mode", C.c_uint32), ("_pad", C.c_uint32),
                ("tri_vertices", C.POINTER(C.c_double)), ("tri_normals", C.POINTER(C.c_double)),
                ("tri_position", C.POINTER(C.c_double)), ("tri_rotation", C.POINTER(C.c_double)),
                ("tri_material", C.POINTER(C.c_uint32))]


class rt_render_params(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("spp", C.c_uint32), ("ray_depth", C.c_uint32),
                ("bg_color", C.c_double * 3), ("cam_position", C.c_double * 3), ("cam_right", C.c_double * 3),
                ("cam_up", C.c_double * 3), ("cam_forward", C.c_double * 3), ("fov_axis", C.c_uint32),
                ("flags", C.c_uint32), ("fov", C.c_double), ("seed", C.c_uint64)]


class rt_stats(C.Structure):
    _fields_ = [("paths", C.c_uint64), ("segments", C.c_uint64), ("aabb_tests", C.c_uint64),
                ("tri_tests", C.c_uint64), ("shape_tests", C.c_uint64), ("shaded_hits", C.c_uint64),
                ("light_queries", C.c_uint64), ("light_hits", C.c_uint64), ("kernel_ms", C.c_double),
                ("total_ms", C.c_double), ("lane_steps", C.c_uint64), ("wave_steps", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class rt_hit(C.Structure):
    _fields_ = [("t", C.c_double), ("geometry_normal", C.c_double * 3), ("shading_normal", C.c_double * 3),
                ("inside", C.c_int32), ("prim", C.c_int32)]


HIT_DTYPE = np.dtype([("t", "<f8"), ("geometry_normal", "<f8", 3), ("shading_normal", "<f8", 3),
                      ("inside", "<i4"), ("prim", "<i4")])
assert HIT_DTYPE.itemsize == C.sizeof(rt_hit)


class rt_scene_info(C.Structure):
    _fields_ = [("n_planes", C.c_uint32), ("n_boxes", C.c_uint32), ("n_ellipsoids", C.c_uint32),
                ("n_triangles", C.c_uint64), ("n_light_boxes", C.c_uint32), ("n_light_ellipsoids", C.c_uint32),
                ("n_light_triangles", C.c_uint64), ("bvh_nodes", C.c_uint64 * 6), ("bvh_depth", C.c_uint32 * 6),
                ("build_ms", C.c_double), ("upload_ms", C.c_double), ("device_bytes", C.c_uint64),
                ("shared_light_mask", C.c_uint32), ("layout_flags", C.c_uint32)]


class rt_tuning(C.Structure):
    _fields_ = [("waves", C.c_uint32), ("resume", C.c_int32), ("kinds", C.c_uint32),
                ("suspend_lanes", C.c_uint32), ("leaf_lanes", C.c_uint32), ("chunk_spp", C.c_uint32),
                ("compact", C.c_int32), ("tail_split", C.c_uint32)]


class rt_denoise_params(C.Structure):
    """Zeroed fields take the header's defaults (RT_DENOISE_*)."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("spp", C.c_uint32), ("iterations", C.c_uint32),
                ("normal_squarings", C.c_uint32), ("_pad", C.c_uint32), ("sigma_l", C.c_double),
                ("sigma_z", C.c_double), ("eps", C.c_double)]


class rt_metrics_params(C.Structure):
    """Zeroed peak, eps and window take the header's defaults (rt_image_metrics_async)."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("format", C.c_uint32), ("_pad", C.c_uint32),
                ("peak", C.c_double), ("eps", C.c_double), ("window", C.c_double * 11)]


class rt_temporal_params(C.Structure):
    """Zeroed max_history, normal_min and plane_tol take the header's defaults (RT_TEMPORAL_*)."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("spp", C.c_uint32), ("max_history", C.c_uint32),
                ("flags", C.c_uint32), ("_pad", C.c_uint32), ("normal_min", C.c_double), ("plane_tol", C.c_double)]


class rt_adaptive_layout(C.Structure):
    """Byte offsets of the adaptive workspace's sub-buffers (rt_adaptive_workspace_bytes)."""
    _fields_ = [(k, C.c_uint64) for k in ("n_tiles", "acc_sum", "acc_sq", "tile_count", "tile_err", "tile_flag",
                                          "tile_list", "info")]


class rt_adaptive_params(C.Structure):
    _fields_ = [("pass_spp", C.c_uint32), ("max_spp", C.c_uint32), ("threshold", C.c_double), ("eps", C.c_double)]


TUNING_AUTO = dict(waves=0, resume=-1, kinds=0, suspend_lanes=0, leaf_lanes=0, chunk_spp=0, compact=-1, tail_split=0)
RT_LAYOUT_COMPACT_TRIS = 0x1
RT_LAYOUT_PAIR_NODES = 0x4
RT_LAYOUT_DEVICE_BUILT = 0x8
RT_LAYOUT_DEVICE_RECORDS = 0x10
RT_LAYOUT_DEVICE_ITEMS = 0x20
RT_LAYOUT_DEVICE_MESHES = 0x40
RT_BUILD_DEVICE = 0x1
RT_BUILD_DEVICE_RECORDS = 0x2
RT_BUILD_DEVICE_ITEMS = 0x4
RT_BUILD_DEVICE_MESHES = 0x8
RT_GLTF_DEFER = 0x1


# every symbol include/rt_api.h declares (checked by tests/test_abi.py)
EXPORTS = {
    "rt_scene_create": (C.c_int, [C.POINTER(rt_scene_desc), C.POINTER(C.c_void_p)]),
    "rt_scene_create_ex": (C.c_int, [C.POINTER(rt_scene_desc), C.c_uint32, C.POINTER(C.c_void_p)]),
    "rt_scene_create_parsed": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    "rt_scene_destroy": (None, [C.c_void_p]),
    "rt_scene_get_info": (C.c_int, [C.c_void_p, C.POINTER(rt_scene_info)]),
    "rt_scene_checksum": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "rt_scene_set_tuning": (C.c_int, [C.c_void_p, C.POINTER(rt_tuning)]),
    "rt_scene_get_tuning": (C.c_int, [C.c_void_p, C.POINTER(rt_tuning)]),
    "rt_scene_sample_chunks": (C.c_int, [C.c_void_p, C.POINTER(rt_render_params), C.POINTER(C.c_uint32),
                                         C.POINTER(C.c_uint32)]),
    "rt_render": (C.c_int, [C.c_void_p, C.POINTER(rt_render_params), C.c_void_p, C.c_void_p, C.POINTER(rt_stats)]),
    "rt_render_moments": (C.c_int, [C.c_void_p, C.POINTER(rt_render_params), C.c_void_p, C.c_void_p,
                                    C.POINTER(rt_stats)]),
    "rt_render_tiles_moments_async": (C.c_int, [C.c_void_p, C.POINTER(rt_render_params), C.c_uint32, C.c_uint32,
                                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_error_estimate_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "rt_camera_rays_async": (C.c_int, [C.POINTER(rt_render_params), C.c_void_p, C.c_void_p]),
    "rt_denoise_workspace_bytes": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
    "rt_denoise_async": (C.c_int, [C.POINTER(rt_denoise_params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "rt_adaptive_workspace_bytes": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64),
                                              C.POINTER(rt_adaptive_layout)]),
    "rt_adaptive_pass_async": (C.c_int, [C.c_void_p, C.POINTER(rt_render_params), C.c_void_p, C.c_uint64, C.c_int,
                                         C.c_uint32, C.c_uint32, C.c_void_p]),
    "rt_adaptive_select_async": (C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_double, C.c_double,
                                           C.c_uint32, C.c_uint32, C.c_void_p]),
    "rt_adaptive_resolve_async": (C.c_int, [C.POINTER(rt_render_params), C.c_void_p, C.c_uint64, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_render_adaptive": (C.c_int, [C.c_void_p, C.POINTER(rt_render_params), C.POINTER(rt_adaptive_params),
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(rt_stats)]),
    "rt_adaptive_select_rank_async": (C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_double, C.c_double,
                                                C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "rt_render_adaptive_rank": (C.c_int, [C.c_void_p, C.POINTER(rt_render_params), C.POINTER(rt_adaptive_params),
                                          C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(rt_stats)]),
    "rt_error_estimate_counts_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]),
    "rt_denoise_counts_async": (C.c_int, [C.POINTER(rt_denoise_params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "rt_ssim_window": (C.c_int, [C.c_double, C.c_void_p]),
    "rt_image_metrics_workspace_bytes": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
    "rt_image_metrics_async": (C.c_int, [C.POINTER(rt_metrics_params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "rt_temporal_history_bytes": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
    "rt_temporal_accumulate_async": (C.c_int, [C.POINTER(rt_temporal_params), C.POINTER(rt_render_params)] +
                                     [C.c_void_p] * 11),
    "rt_tiles_per_rank": (C.c_int, [C.POINTER(rt_render_params), C.c_uint32, C.POINTER(C.c_uint32)]),
    "rt_sample_chunks": (C.c_int, [C.POINTER(rt_render_params), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "rt_render_tiles_async": (C.c_int, [C.c_void_p, C.POINTER(rt_render_params), C.c_uint32, C.c_uint32,
                                        C.c_void_p, C.c_void_p]),
    "rt_read_stats": (C.c_int, [C.c_void_p, C.POINTER(rt_stats), C.c_int]),
    "rt_read_raw_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "rt_unpack_tiles_async": (C.c_int, [C.POINTER(rt_render_params), C.c_uint32, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "rt_unpack_tiles_bytes_async": (C.c_int, [C.POINTER(rt_render_params), C.c_uint32, C.c_void_p, C.c_void_p,
                                              C.c_void_p]),
    "rt_tonemap_bytes_async": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "rt_intersect_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rt_intersect_rays_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p]),
    "rt_light_pdf_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rt_intersect_lights_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "rt_parse_custom_scene": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "rt_load_gltf": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "rt_load_gltf_ex": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "rt_parsed_scene_get": (C.c_int, [C.c_void_p, C.POINTER(rt_scene_desc), C.POINTER(rt_render_params)]),
    "rt_parsed_scene_free": (None, [C.c_void_p]),
    "rt_tonemap_gamma": (None, [C.c_void_p, C.c_uint64, C.c_void_p]),
    "rt_save_ppm": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "rt_byte_thresholds": (C.c_int, [C.c_void_p]),
    "rt_last_error": (C.c_char_p, []),
    "rt_api_version": (C.c_int, []),
    "rt_device_count": (C.c_int, []),
    "rt_probe_fp64": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rt_bvh_build": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_void_p,
                               C.POINTER(C.c_uint32)]),
    "rt_bvh_build_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "rt_multi_create": (C.c_int, [C.POINTER(rt_scene_desc), C.POINTER(C.c_int), C.c_uint32, C.c_uint32,
                                  C.POINTER(C.c_void_p)]),
    "rt_multi_render": (C.c_int, [C.c_void_p, C.POINTER(rt_render_params), C.c_void_p, C.c_void_p,
                                  C.POINTER(rt_stats)]),
    "rt_multi_scene": (C.c_void_p, [C.c_void_p, C.c_uint32]),
    "rt_multi_destroy": (None, [C.c_void_p]),
}
RT_MULTI_PEER = 0x1

_lib = None


def lib() -> C.CDLL:
    """Load ``build/librt_amd.so`` (raises if it was not built — no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} missing: run __graft_entry__.build() (no CPU fallback exists)")
        # One HIP runtime per process: torch ships its own libamdhip64.so with
        # the same SONAME (libamdhip64.so.7) as /opt/rocm's.  Importing torch
        # first makes our DT_NEEDED bind to torch's copy, so device pointers
        # and streams from torch (tile buffers, RCCL gather) are valid here;
        # loading ours first would leave torch unable to initialise HIP.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in EXPORTS.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


class RtError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"rt error {code} ({ERRORS.get(code, '?')}): {msg}")
        self.code = code


def _check(rc: int):
    if rc != 0:
        raise RtError(rc, lib().rt_last_error().decode(errors="replace"))


def _ptr(a: Optional[np.ndarray], ctype=C.c_double):
    if a is None:
        return None
    return a.ctypes.data_as(C.POINTER(ctype))


def device_count() -> int:
    return lib().rt_device_count()


# --------------------------------------------------------- scene model ----
@dataclass
class RenderParams:
    """Scene-level settings of the reference's Scene (scene.rs:81-90) + RNG seed."""
    width: int
    height: int
    spp: int = 64
    ray_depth: int = 16
    bg_color: tuple = (0.0, 0.0, 0.0)
    cam_position: tuple = (0.0, 0.0, 0.0)
    cam_right: tuple = (1.0, 0.0, 0.0)
    cam_up: tuple = (0.0, 1.0, 0.0)
    cam_forward: tuple = (0.0, 0.0, 1.0)
    fov_axis: int = RT_FOV_X
    fov: float = np.pi / 2
    seed: int = 0x5EED
    flags: int = 0

    def to_c(self) -> rt_render_params:
        p = rt_render_params()
        p.width, p.height, p.spp, p.ray_depth = self.width, self.height, self.spp, self.ray_depth
        p.bg_color[:] = self.bg_color
        p.cam_position[:] = self.cam_position
        p.cam_right[:] = self.cam_right
        p.cam_up[:] = self.cam_up
        p.cam_forward[:] = self.cam_forward
        p.fov_axis, p.fov, p.seed, p.flags = self.fov_axis, self.fov, self.seed, self.flags
        return p

    @staticmethod
    def from_c(p: rt_render_params) -> "RenderParams":
        return RenderParams(p.width, p.height, p.spp, p.ray_depth, tuple(p.bg_color), tuple(p.cam_position),
                            tuple(p.cam_right), tuple(p.cam_up), tuple(p.cam_forward), p.fov_axis, p.fov,
                            p.seed, p.flags)

    def replace(self, **kw) -> "RenderParams":
        d = dict(self.__dict__)
        d.update(kw)
        return RenderParams(**d)


@dataclass
class SceneDesc:
    """The parsed scene (parsed_scene.rs) as numpy arrays; see rt_scene_desc."""
    materials: np.ndarray                  # structured, rt_material layout
    shapes: np.ndarray                     # structured, rt_shape layout
    tri_vertices: np.ndarray = field(default_factory=lambda: np.zeros((0, 9)))
    tri_normals: Optional[np.ndarray] = None
    tri_position: Optional[np.ndarray] = None
    tri_rotation: Optional[np.ndarray] = None
    tri_material: np.ndarray = field(default_factory=lambda: np.zeros(0, np.uint32))
    tri_mode: int = RT_TRI_CUSTOM

    def to_c(self):
        """Returns (rt_scene_desc, keepalive) — the arrays must outlive the call."""
        keep = []

        def arr(a, dt):
            if a is None or len(a) == 0:
                return None
            a = np.ascontiguousarray(a, dtype=dt)
            keep.append(a)
            return a

        mats = arr(self.materials, MATERIAL_DTYPE)
        shapes = arr(self.shapes, SHAPE_DTYPE)
        tv = arr(self.tri_vertices, np.float64)
        tn = arr(self.tri_normals, np.float64)
        tp = arr(self.tri_position, np.float64)
        tr = arr(self.tri_rotation, np.float64)
        tm = arr(self.tri_material, np.uint32)
        d = rt_scene_desc()
        d.n_materials = 0 if mats is None else len(mats)
        d.n_shapes = 0 if shapes is None else len(shapes)
        d.n_triangles = 0 if tm is None else len(tm)
        d.materials = None if mats is None else mats.ctypes.data_as(C.POINTER(rt_material))
        d.shapes = None if shapes is None else shapes.ctypes.data_as(C.POINTER(rt_shape))
        d.tri_mode = self.tri_mode
        d.tri_vertices = _ptr(tv)
        d.tri_normals = _ptr(tn)
        d.tri_position = _ptr(tp)
        d.tri_rotation = _ptr(tr)
        d.tri_material = _ptr(tm, C.c_uint32)
        return d, keep


MATERIAL_DTYPE = np.dtype([("kind", "<u4"), ("_pad", "<u4"), ("ior", "<f8"), ("color", "<f8", 3),
                           ("emission", "<f8", 3)])
SHAPE_DTYPE = np.dtype([("type", "<u4"), ("material", "<u4"), ("shape", "<f8", 3), ("position", "<f8", 3),
                        ("rotation", "<f8", 4)])
assert MATERIAL_DTYPE.itemsize == C.sizeof(rt_material) and SHAPE_DTYPE.itemsize == C.sizeof(rt_shape)


def _desc_from_c(d: rt_scene_desc) -> SceneDesc:
    def np_from(ptr, n, dt, shape):
        if not ptr or n == 0:
            return None
        buf = C.cast(ptr, C.POINTER(C.c_char * (n * np.dtype(dt).itemsize))).contents
        return np.frombuffer(bytes(buf), dtype=dt).reshape(shape).copy()

    nt = d.n_triangles
    mats = np_from(d.materials, d.n_materials, MATERIAL_DTYPE, (d.n_materials,))
    shapes = np_from(d.shapes, d.n_shapes, SHAPE_DTYPE, (d.n_shapes,))
    return SceneDesc(
        materials=mats if mats is not None else np.zeros(0, MATERIAL_DTYPE),
        shapes=shapes if shapes is not None else np.zeros(0, SHAPE_DTYPE),
        tri_vertices=np_from(d.tri_vertices, nt * 9, np.float64, (nt, 9)) if nt else np.zeros((0, 9)),
        tri_normals=np_from(d.tri_normals, nt * 9, np.float64, (nt, 9)),
        tri_position=np_from(d.tri_position, nt * 3, np.float64, (nt, 3)),
        tri_rotation=np_from(d.tri_rotation, nt * 4, np.float64, (nt, 4)),
        tri_material=np_from(d.tri_material, nt, np.uint32, (nt,)) if nt else np.zeros(0, np.uint32),
        tri_mode=d.tri_mode)


def _take_parsed(handle: C.c_void_p):
    d, p = rt_scene_desc(), rt_render_params()
    try:
        _check(lib().rt_parsed_scene_get(handle, C.byref(d), C.byref(p)))
        return _desc_from_c(d), RenderParams.from_c(p)
    finally:
        lib().rt_parsed_scene_free(handle)


def parse_scene(text: str):
    """scene_parser::parse_scene + Scene::new defaults -> (SceneDesc, RenderParams)."""
    h = C.c_void_p()
    _check(lib().rt_parse_custom_scene(text.encode(), C.byref(h)))
    return _take_parsed(h)


class ParsedScene:
    """A deferred glTF parse (rt_load_gltf_ex, RT_GLTF_DEFER): the draw plan and the buffers'
    bytes.  ``params`` is there at once; ``desc()`` makes the SceneDesc on first use (the
    host flatten) and raises what the eager load would have raised.  Owns the handle until
    ``close()``."""

    def __init__(self, handle: C.c_void_p):
        self._h = handle
        self._desc = None
        p = rt_render_params()
        _check(lib().rt_parsed_scene_get(handle, None, C.byref(p)))
        self.params = RenderParams.from_c(p)

    @property
    def handle(self):
        return self._h

    def desc(self) -> "SceneDesc":
        if self._desc is None:
            d = rt_scene_desc()
            _check(lib().rt_parsed_scene_get(self._h, C.byref(d), None))
            self._desc = _desc_from_c(d)
        return self._desc

    def close(self):
        if getattr(self, "_h", None):
            lib().rt_parsed_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def load_gltf(path: str, width: int, height: int, spp: int, defer: bool = False):
    """gltf::parse + gltf::build_scene (main.rs:47-66) -> (SceneDesc, RenderParams); with
    defer=True a ParsedScene, whose meshes Scene.from_parsed can flatten on the device."""
    h = C.c_void_p()
    if defer:
        _check(lib().rt_load_gltf_ex(path.encode(), width, height, spp, RT_GLTF_DEFER, C.byref(h)))
        return ParsedScene(h)
    _check(lib().rt_load_gltf(path.encode(), width, height, spp, C.byref(h)))
    return _take_parsed(h)


class Scene:
    """Scene::new: BVHs built on the host (build="device": the triangle BVHs on the current
    HIP device, the same trees; records="device": their arrays written there too, not
    uploaded; items="device": the per-triangle items behind those arrays computed there from
    the description's arrays), flattened arrays resident on the current HIP device."""

    @staticmethod
    def _build_flags(build: str, records: str, items: str, meshes: str = "host") -> int:
        if build not in ("host", "device"):
            raise ValueError(f"build must be 'host' or 'device', not {build!r}")
        if records not in ("host", "device"):
            raise ValueError(f"records must be 'host' or 'device', not {records!r}")
        if records == "device" and build != "device":
            raise ValueError("records='device' needs build='device'")
        if items not in ("host", "device"):
            raise ValueError(f"items must be 'host' or 'device', not {items!r}")
        if items == "device" and records != "device":
            raise ValueError("items='device' needs build='device' and records='device'")
        if meshes not in ("host", "device"):
            raise ValueError(f"meshes must be 'host' or 'device', not {meshes!r}")
        if meshes == "device" and items != "device":
            raise ValueError("meshes='device' needs build='device', records='device' and items='device'")
        return ((RT_BUILD_DEVICE if build == "device" else 0) | (RT_BUILD_DEVICE_RECORDS if records == "device" else 0) |
                (RT_BUILD_DEVICE_ITEMS if items == "device" else 0) | (RT_BUILD_DEVICE_MESHES if meshes == "device" else 0))

    def __init__(self, desc: SceneDesc, build: str = "host", records: str = "host", items: str = "host"):
        flags = self._build_flags(build, records, items)
        self.desc = desc
        d, keep = desc.to_c()
        h = C.c_void_p()
        _check(lib().rt_scene_create_ex(C.byref(d), flags, C.byref(h)))
        self._h = h
        del keep

    @classmethod
    def from_parsed(cls, parsed: "ParsedScene", build: str = "host", records: str = "host", items: str = "host",
                    meshes: str = "host") -> "Scene":
        """rt_scene_create_parsed: the scene of a deferred glTF parse.  meshes="device" (with
        the other three) flattens the meshes on the device from the buffers' bytes; the
        description is then made only for what falls back to the host."""
        flags = cls._build_flags(build, records, items, meshes)
        h = C.c_void_p()
        _check(lib().rt_scene_create_parsed(parsed.handle, flags, C.byref(h)))
        self = cls.__new__(cls)
        self.desc = None
        self._h = h
        return self

    def close(self):
        if getattr(self, "_h", None):
            lib().rt_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def checksum(self) -> int:
        """rt_scene_checksum: content hash of the scene's device arrays."""
        h = C.c_uint64()
        _check(lib().rt_scene_checksum(self._h, C.byref(h)))
        return h.value

    def info(self) -> dict:
        i = rt_scene_info()
        _check(lib().rt_scene_get_info(self._h, C.byref(i)))
        out = {k: getattr(i, k) for k, _ in i._fields_}
        out["bvh_nodes"] = list(i.bvh_nodes)
        out["bvh_depth"] = list(i.bvh_depth)
        return out

    def set_tuning(self, **kw):
        """Force the kernel form of this scene's renders (rt_scene_set_tuning): waves (3|4|5; 5 = shape-only fused only),
        resume (0|1), kinds (3 = all-kinds instance), suspend_lanes, leaf_lanes (1..64),
        chunk_spp, compact (0 = f64 triangle-BVH layout, 1 = compact when the scene has it),
        tail_split (1 = every wave-tile whole, 2..8 = the queue's last wave-tiles in that many parts).
        Fields not given are auto (the library's per-scene pick)."""
        bad = set(kw) - set(TUNING_AUTO)
        if bad:
            raise ValueError(f"unknown tuning fields {sorted(bad)}")
        t = rt_tuning(**{**TUNING_AUTO, **{k: int(v) for k, v in kw.items()}})
        _check(lib().rt_scene_set_tuning(self._h, C.byref(t)))

    def tuning(self) -> dict:
        """The resolved kernel form the next render runs (rt_scene_get_tuning)."""
        t = rt_tuning()
        _check(lib().rt_scene_get_tuning(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in t._fields_ if not k.startswith("_")}

    def sample_chunks(self, params: RenderParams):
        """(chunks, chunk_spp) this scene's renders use (rt_scene_sample_chunks)."""
        k, cs = C.c_uint32(), C.c_uint32()
        _check(lib().rt_scene_sample_chunks(self._h, C.byref(params.to_c()), C.byref(k), C.byref(cs)))
        return k.value, cs.value

    def generate_image(self, params: RenderParams, hit_ids: bool = False, stats: bool = False):
        """Mean radiance per pixel [H, W, 3] f64 (main.rs:100-104 before tonemapping).

        Returns (image, hit_ids or None, stats dict)."""
        flags = params.flags | (RT_FLAG_HIT_IDS if hit_ids else 0) | (RT_FLAG_STATS if stats else 0)
        p = params.replace(flags=flags).to_c()
        img = np.zeros((params.height, params.width, 3), np.float64)
        hits = None
        if hit_ids:
            hits = np.zeros((params.height * params.width, params.spp, params.ray_depth), np.int32)
        st = rt_stats()
        _check(lib().rt_render(self._h, C.byref(p), img.ctypes.data_as(C.c_void_p),
                               None if hits is None else hits.ctypes.data_as(C.c_void_p), C.byref(st)))
        return img, hits, st.as_dict()

    def render_moments(self, params: RenderParams):
        """(mean, sq), both [H, W, 3] f64 (rt_render_moments): generate_image's mean, bit for
        bit, and the per-pixel second moment, sum of L * L over the samples / spp."""
        p = params.to_c()
        mean = np.zeros((params.height, params.width, 3), np.float64)
        sq = np.zeros_like(mean)
        _check(lib().rt_render_moments(self._h, C.byref(p), mean.ctypes.data_as(C.c_void_p),
                                       sq.ctypes.data_as(C.c_void_p), None))
        return mean, sq

    def render_adaptive(self, params: RenderParams, pass_spp: int, max_spp: int, rel_error: float, eps: float = 0.0,
                        rank: int = 0):
        """Adaptive sampling (rt_render_adaptive): passes of pass_spp samples, every tile until its
        error is <= rel_error or it has max_spp.  rank != 0: the tile's error is its (rank + 1)-th largest
        pixel error, not the largest (rt_render_adaptive_rank).  Returns (mean, sq [H, W, 3] f64, count
        [H, W] u32, info: paths = samples spent, kernel_ms, total_ms).  params.spp is ignored."""
        mean = np.zeros((params.height, params.width, 3), np.float64)
        sq = np.zeros_like(mean)
        count = np.zeros((params.height, params.width), np.uint32)
        a, st = rt_adaptive_params(pass_spp, max_spp, rel_error, eps), rt_stats()
        out = (mean.ctypes.data_as(C.c_void_p), sq.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p), C.byref(st))
        if rank:
            _check(lib().rt_render_adaptive_rank(self._h, C.byref(params.to_c()), C.byref(a), rank, *out))
        else:
            _check(lib().rt_render_adaptive(self._h, C.byref(params.to_c()), C.byref(a), *out))
        info = st.as_dict()
        return mean, sq, count, {k: info[k] for k in ("paths", "kernel_ms", "total_ms")}

    def adaptive_pass_async(self, params: RenderParams, d_workspace_ptr: int, workspace_bytes: int, use_list: bool,
                            n_list: int, sample_base: int, stream_ptr: int = 0):
        """One pass of params.spp samples from sample_base onto the workspace's accumulators
        (rt_adaptive_pass_async): every tile, or the first n_list entries of its tile_list."""
        _check(lib().rt_adaptive_pass_async(self._h, C.byref(params.to_c()), C.c_void_p(d_workspace_ptr),
                                            workspace_bytes, 1 if use_list else 0, n_list, sample_base,
                                            C.c_void_p(stream_ptr)))

    def intersect(self, rays: np.ndarray) -> np.ndarray:
        """intersect(ray, &scene.primitives, +inf) for rays [n, 6] -> structured hits."""
        rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
        out = np.zeros(len(rays), HIT_DTYPE)
        _check(lib().rt_intersect_rays(self._h, rays.ctypes.data_as(C.c_void_p), len(rays),
                                       out.ctypes.data_as(C.c_void_p)))
        return out

    def intersect_async(self, d_rays_ptr: int, n: int, d_hits_ptr: int, method: int = 1, stream_ptr: int = 0):
        """Device-buffer batch intersect (rt_intersect_rays_async): d_rays [n][6] f64 and
        d_hits [n] rt_hit (64 B) in HBM; method 0 = one thread per ray, 1 = persistent."""
        _check(lib().rt_intersect_rays_async(self._h, C.c_void_p(d_rays_ptr), n, C.c_void_p(d_hits_ptr), method,
                                             C.c_void_p(stream_ptr)))

    def light_pdf(self, pos_dir: np.ndarray) -> np.ndarray:
        """Light::pdf for [n, 6] (surface position, unit direction)."""
        pos_dir = np.ascontiguousarray(pos_dir, np.float64).reshape(-1, 6)
        out = np.zeros(len(pos_dir), np.float64)
        _check(lib().rt_light_pdf_rays(self._h, pos_dir.ctypes.data_as(C.c_void_p), len(pos_dir),
                                       out.ctypes.data_as(C.c_void_p)))
        return out

    def intersect_lights(self, rays: np.ndarray):
        """Raw intersect_lights accumulation -> (impact sum, callback count)."""
        rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
        imp = np.zeros(len(rays), np.float64)
        cnt = np.zeros(len(rays), np.uint32)
        _check(lib().rt_intersect_lights_rays(self._h, rays.ctypes.data_as(C.c_void_p), len(rays),
                                              imp.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p)))
        return imp, cnt

    def denoise(self, params: RenderParams, mean: np.ndarray, sq: np.ndarray, count: Optional[np.ndarray] = None, **kw):
        """The à-trous filter (rt_denoise_async) of a frame's (mean, sq) [H, W, 3], as render_moments
        returns them: pixel-centre rays, their first hits in this scene, the filter; everything
        between the upload and the download stays on the device.  count: None, or [H, W] u32 as
        render_adaptive returns it, every pixel's own sample count in place of params.spp
        (rt_denoise_counts_async).  kw: rt_denoise_params fields
        (iterations, normal_squarings, sigma_l, sigma_z, eps).  Returns (out [H, W, 3], out_var [H, W]).
        The buffers are made on torch's current device, where the rays and the filter also run: the
        scene must live there (it does unless the current device changed since it was created)."""
        import torch
        h, w = params.height, params.width
        dev = dict(dtype=torch.float64, device="cuda")
        # one allocation each: rt_denoise_async wants every buffer 16-byte aligned, and the second half of a
        # stacked upload is not when W * H is odd
        d_mean, d_sq = (torch.from_numpy(np.ascontiguousarray(a, np.float64).reshape(h, w, 3)).cuda() for a in (mean, sq))
        d_rays, d_hits = torch.empty((h * w, 6), **dev), torch.empty((h * w, 8), **dev)
        d_out, d_var = torch.empty((h, w, 3), **dev), torch.empty((h, w), **dev)
        d_ws = torch.empty(denoise_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        camera_rays_async(params, d_rays.data_ptr(), stream)
        self.intersect_async(d_rays.data_ptr(), h * w, d_hits.data_ptr(), stream_ptr=stream)
        tail = (d_rays.data_ptr(), d_hits.data_ptr(), d_out.data_ptr(), d_var.data_ptr(), d_ws.data_ptr(), d_ws.numel(), stream)
        p = rt_denoise_params(width=w, height=h, spp=params.spp, **kw)
        if count is None:
            denoise_async(p, d_mean.data_ptr(), d_sq.data_ptr(), *tail)
        else:
            d_count = torch.from_numpy(np.ascontiguousarray(count, np.uint32).reshape(h, w).view(np.int32)).cuda()
            denoise_counts_async(p, d_mean.data_ptr(), d_sq.data_ptr(), d_count.data_ptr(), *tail)
        return d_out.cpu().numpy(), d_var.cpu().numpy()

    def accumulate(self, params: RenderParams, mean: np.ndarray, sq: np.ndarray, count: Optional[np.ndarray] = None,
                   history=None, prev_params: Optional[RenderParams] = None, **kw):
        """Temporal accumulation (rt_temporal_accumulate_async) of a frame's (mean, sq) [H, W, 3] with the
        history of the frames before it: pixel-centre rays and their first hits in this scene as
        denoise makes them, then the kernel.  count: None (every pixel has params.spp samples) or
        [H, W] u32.  history, prev_params: None for the first frame of a sequence, else the history
        the previous call returned and the RenderParams it was called with.  kw: rt_temporal_params
        fields (max_history, flags, normal_min, plane_tol).  Returns (mean [H, W, 3], sq [H, W, 3],
        count [H, W] u32, history); the arrays go straight into denoise(..., count=count), and
        history, a device torch.uint8 tensor, into the next call.  Runs on torch's current device,
        where the scene must live (see denoise)."""
        import torch
        h, w = params.height, params.width
        dev = dict(dtype=torch.float64, device="cuda")
        d_mean, d_sq = (torch.from_numpy(np.ascontiguousarray(a, np.float64).reshape(h, w, 3)).cuda() for a in (mean, sq))
        d_count = None
        if count is not None:
            d_count = torch.from_numpy(np.ascontiguousarray(count, np.uint32).reshape(h, w).view(np.int32)).cuda()
        d_rays, d_hits = torch.empty((h * w, 6), **dev), torch.empty((h * w, 8), **dev)
        d_om, d_os = torch.empty((h, w, 3), **dev), torch.empty((h, w, 3), **dev)
        d_oc = torch.empty((h, w), dtype=torch.int32, device="cuda")
        d_next = torch.empty(temporal_history_bytes(w, h), dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        camera_rays_async(params, d_rays.data_ptr(), stream)
        self.intersect_async(d_rays.data_ptr(), h * w, d_hits.data_ptr(), stream_ptr=stream)
        temporal_accumulate_async(rt_temporal_params(width=w, height=h, spp=params.spp, **kw), prev_params,
                                  d_mean.data_ptr(), d_sq.data_ptr(), 0 if d_count is None else d_count.data_ptr(),
                                  d_rays.data_ptr(), d_hits.data_ptr(), 0 if history is None else history.data_ptr(),
                                  d_next.data_ptr(), d_om.data_ptr(), d_os.data_ptr(), d_oc.data_ptr(), stream)
        return d_om.cpu().numpy(), d_os.cpu().numpy(), d_oc.cpu().numpy().view(np.uint32), d_next

    # ---- multi-GPU tile partition ----
    def tiles_per_rank(self, params: RenderParams, world: int) -> int:
        n = C.c_uint32()
        _check(lib().rt_tiles_per_rank(C.byref(params.to_c()), world, C.byref(n)))
        return n.value

    def render_tiles_async(self, params: RenderParams, rank: int, world: int, d_out_ptr: int, stream_ptr: int = 0,
                           stats: bool = False):
        p = params.replace(flags=params.flags | (RT_FLAG_STATS if stats else 0)).to_c()
        _check(lib().rt_render_tiles_async(self._h, C.byref(p), rank, world, C.c_void_p(d_out_ptr),
                                           C.c_void_p(stream_ptr)))

    def render_tiles_moments_async(self, params: RenderParams, rank: int, world: int, d_out_ptr: int, d_sq_ptr: int,
                                   stream_ptr: int = 0):
        """render_tiles_async with a second packed buffer for the second moment."""
        _check(lib().rt_render_tiles_moments_async(self._h, C.byref(params.to_c()), rank, world, C.c_void_p(d_out_ptr),
                                                   C.c_void_p(d_sq_ptr), C.c_void_p(stream_ptr)))

    def read_stats(self, reset: bool = True) -> dict:
        st = rt_stats()
        _check(lib().rt_read_stats(self._h, C.byref(st), 1 if reset else 0))
        return st.as_dict()

    def read_raw_stats(self, n: int = 64) -> np.ndarray:
        """Raw device counter words (diagnostics; rt_read_raw_stats)."""
        out = np.zeros(n, np.uint64)
        _check(lib().rt_read_raw_stats(self._h, out.ctypes.data_as(C.c_void_p), n))
        return out


class MultiScene:
    """generate_image over several GPUs of one process (rt_multi_*): one scene
    replica per listed device (BVHs built once, uploaded to devices[0] and
    broadcast from there: ncclBroadcast, or peer copies), the frame's tiles dealt
    round-robin, one gather to devices[0] (RCCL ncclGather, or peer copies with
    peer=True, which also allows a device listed twice)."""

    def __init__(self, desc: SceneDesc, devices, peer: bool = False):
        self.desc = desc
        self.devices = [int(d) for d in devices]
        d, keep = desc.to_c()
        devs = (C.c_int * len(self.devices))(*self.devices)
        h = C.c_void_p()
        _check(lib().rt_multi_create(C.byref(d), devs, len(self.devices), RT_MULTI_PEER if peer else 0,
                                     C.byref(h)))
        self._h = h
        del keep

    def close(self):
        if getattr(self, "_h", None):
            lib().rt_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def scene_checksum(self, index: int) -> int:
        """rt_scene_checksum of the replica on devices[index] (rt_multi_create already
        checked every replica against devices[0]'s)."""
        h = lib().rt_multi_scene(self._h, index)
        if not h:
            raise IndexError(index)
        v = C.c_uint64()
        _check(lib().rt_scene_checksum(C.c_void_p(h), C.byref(v)))
        return v.value

    def scene_info(self, index: int) -> dict:
        """rt_scene_get_info of the replica on devices[index] (rt_multi_scene): devices[0]'s came
        from the host, the others from devices[0] (ncclBroadcast / peer copies), whose fill time
        is part of their upload_ms."""
        h = lib().rt_multi_scene(self._h, index)
        if not h:
            raise IndexError(index)
        i = rt_scene_info()
        _check(lib().rt_scene_get_info(C.c_void_p(h), C.byref(i)))
        out = {k: getattr(i, k) for k, _ in i._fields_}
        out["bvh_nodes"] = list(i.bvh_nodes)
        out["bvh_depth"] = list(i.bvh_depth)
        return out

    def generate_image(self, params: RenderParams, ppm_bytes: bool = False, stats: bool = False):
        """(mean radiance [H, W, 3] f64, PPM payload [H, W, 3] u8 or None, stats dict)."""
        p = params.replace(flags=params.flags | (RT_FLAG_STATS if stats else 0)).to_c()
        img = np.zeros((params.height, params.width, 3), np.float64)
        byts = np.zeros((params.height, params.width, 3), np.uint8) if ppm_bytes else None
        st = rt_stats()
        _check(lib().rt_multi_render(self._h, C.byref(p), img.ctypes.data_as(C.c_void_p),
                                     None if byts is None else byts.ctypes.data_as(C.c_void_p), C.byref(st)))
        return img, byts, st.as_dict()


def tile_layout(width: int, height: int, world: int):
    """16x16 tiles, tile t owned by rank t % world at slot t // world.
    Returns (tiles_x, tiles_y, n_tiles, slots_per_rank)."""
    tx = (width + RT_TILE - 1) // RT_TILE
    ty = (height + RT_TILE - 1) // RT_TILE
    n = tx * ty
    return tx, ty, n, (n + world - 1) // world


def gather_tiles(tiles, gathered, rank: int, world: int, group=None):
    """The single framebuffer exchange: every rank's packed tiles [slots, 256, 3]
    to rank 0's [world, slots, 256, 3] (rank-major, ncclGather layout) with one
    torch.distributed gather (RCCL under the "nccl" backend, gloo on CPU)."""
    if world == 1:
        return tiles
    import torch.distributed as dist
    dist.gather(tiles, list(gathered.unbind(0)) if rank == 0 else None, dst=0, group=group)
    return gathered


def unpack_tiles_async(params: RenderParams, world: int, d_gathered_ptr: int, d_image_ptr: int, stream_ptr: int = 0):
    _check(lib().rt_unpack_tiles_async(C.byref(params.to_c()), world, C.c_void_p(d_gathered_ptr),
                                       C.c_void_p(d_image_ptr), C.c_void_p(stream_ptr)))


def error_estimate_async(d_mean_ptr: int, d_sq_ptr: int, n_pixels: int, spp: int, d_se_ptr: int, d_summary_ptr: int,
                         stream_ptr: int = 0):
    """Device (mean, second moment) [n_pixels][3] f64 -> standard error of the mean (d_se_ptr 0: none)
    and the 8-double frame summary (rt_error_estimate_async)."""
    _check(lib().rt_error_estimate_async(C.c_void_p(d_mean_ptr), C.c_void_p(d_sq_ptr), n_pixels, spp,
                                         C.c_void_p(d_se_ptr), C.c_void_p(d_summary_ptr), C.c_void_p(stream_ptr)))


def error_estimate_counts_async(d_mean_ptr: int, d_sq_ptr: int, d_count_ptr: int, n_pixels: int, d_se_ptr: int,
                                d_summary_ptr: int, stream_ptr: int = 0):
    """error_estimate_async with every pixel's own count, [n_pixels] u32 (rt_error_estimate_counts_async)."""
    _check(lib().rt_error_estimate_counts_async(C.c_void_p(d_mean_ptr), C.c_void_p(d_sq_ptr), C.c_void_p(d_count_ptr),
                                                n_pixels, C.c_void_p(d_se_ptr), C.c_void_p(d_summary_ptr),
                                                C.c_void_p(stream_ptr)))


def camera_rays_async(params: RenderParams, d_rays_ptr: int, stream_ptr: int = 0):
    """Pixel-centre primary rays [H * W][6] f64 of the frame into device memory (rt_camera_rays_async)."""
    _check(lib().rt_camera_rays_async(C.byref(params.to_c()), C.c_void_p(d_rays_ptr), C.c_void_p(stream_ptr)))


def denoise_workspace_bytes(width: int, height: int) -> int:
    n = C.c_uint64()
    _check(lib().rt_denoise_workspace_bytes(width, height, C.byref(n)))
    return n.value


def denoise_async(p: rt_denoise_params, d_mean_ptr: int, d_sq_ptr: int, d_rays_ptr: int, d_hits_ptr: int,
                  d_out_ptr: int, d_out_var_ptr: int, d_workspace_ptr: int, workspace_bytes: int, stream_ptr: int = 0):
    """Device (mean, second moment, pixel-centre rays, their first hits) -> the filtered frame [H][W][3] f64 and
    (d_out_var_ptr 0: none) its variance [H][W], in the caller's workspace (rt_denoise_async)."""
    _check(lib().rt_denoise_async(C.byref(p), C.c_void_p(d_mean_ptr), C.c_void_p(d_sq_ptr), C.c_void_p(d_rays_ptr),
                                  C.c_void_p(d_hits_ptr), C.c_void_p(d_out_ptr), C.c_void_p(d_out_var_ptr),
                                  C.c_void_p(d_workspace_ptr), workspace_bytes, C.c_void_p(stream_ptr)))


def denoise_counts_async(p: rt_denoise_params, d_mean_ptr: int, d_sq_ptr: int, d_count_ptr: int, d_rays_ptr: int,
                         d_hits_ptr: int, d_out_ptr: int, d_out_var_ptr: int, d_workspace_ptr: int, workspace_bytes: int,
                         stream_ptr: int = 0):
    """denoise_async with every pixel's own count, [H][W] u32, in place of p.spp (rt_denoise_counts_async)."""
    _check(lib().rt_denoise_counts_async(C.byref(p), C.c_void_p(d_mean_ptr), C.c_void_p(d_sq_ptr),
                                         C.c_void_p(d_count_ptr), C.c_void_p(d_rays_ptr), C.c_void_p(d_hits_ptr),
                                         C.c_void_p(d_out_ptr), C.c_void_p(d_out_var_ptr), C.c_void_p(d_workspace_ptr),
                                         workspace_bytes, C.c_void_p(stream_ptr)))


def temporal_history_bytes(width: int, height: int) -> int:
    n = C.c_uint64()
    _check(lib().rt_temporal_history_bytes(width, height, C.byref(n)))
    return n.value


def temporal_accumulate_async(p: rt_temporal_params, prev_params: Optional[RenderParams], d_mean_ptr: int, d_sq_ptr: int,
                              d_count_ptr: int, d_rays_ptr: int, d_hits_ptr: int, d_hist_prev_ptr: int,
                              d_hist_next_ptr: int, d_out_mean_ptr: int, d_out_sq_ptr: int, d_out_count_ptr: int,
                              stream_ptr: int = 0):
    """Device buffers in, device buffers out: the frame's (mean, sq [, count]) merged with the history
    reprojected from prev_params' camera (rt_temporal_accumulate_async).  d_count_ptr 0: p.spp for
    every pixel; prev_params None and d_hist_prev_ptr 0: the first frame of a sequence."""
    prev = None if prev_params is None else C.byref(prev_params.to_c())
    _check(lib().rt_temporal_accumulate_async(C.byref(p), prev, *(C.c_void_p(v) for v in (
        d_mean_ptr, d_sq_ptr, d_count_ptr, d_rays_ptr, d_hits_ptr, d_hist_prev_ptr, d_hist_next_ptr, d_out_mean_ptr,
        d_out_sq_ptr, d_out_count_ptr, stream_ptr))))


def ssim_window(sigma: float = 1.5) -> np.ndarray:
    """The eleven normalised Gaussian SSIM taps (rt_ssim_window; host only)."""
    out = np.zeros(11)
    _check(lib().rt_ssim_window(sigma, out.ctypes.data_as(C.c_void_p)))
    return out


def image_metrics_workspace_bytes(width: int, height: int) -> int:
    n = C.c_uint64()
    _check(lib().rt_image_metrics_workspace_bytes(width, height, C.byref(n)))
    return n.value


def image_metrics_async(p: rt_metrics_params, d_a_ptr: int, d_b_ptr: int, d_rel_ptr: int, d_ssim_ptr: int,
                        d_summary_ptr: int, d_workspace_ptr: int, workspace_bytes: int, stream_ptr: int = 0):
    """Device frames a (under test) and b (reference), [H][W][3] in p.format -> the 8 doubles of the summary and
    (pointers 0: none) the per-pixel rel [H][W] and per-window ssim [H - 10][W - 10] (rt_image_metrics_async)."""
    _check(lib().rt_image_metrics_async(C.byref(p), C.c_void_p(d_a_ptr), C.c_void_p(d_b_ptr), C.c_void_p(d_rel_ptr),
                                        C.c_void_p(d_ssim_ptr), C.c_void_p(d_summary_ptr), C.c_void_p(d_workspace_ptr),
                                        workspace_bytes, C.c_void_p(stream_ptr)))


def image_metrics(a: np.ndarray, b: np.ndarray, peak: Optional[float] = None, eps: Optional[float] = None,
                  window: Optional[np.ndarray] = None, maps: bool = False) -> dict:
    """The distance of frame a to the reference frame b, both [H, W, 3] float64 radiance or both uint8
    display bytes, computed on torch's current device (rt_image_metrics_async).  peak, eps, window: None
    for the header's defaults.  Returns mse, rel_mse, psnr and max_abs over the good pixels, ssim (the mean
    over the windows that count), bad_pixels, bad_windows, the raw summary, and with maps=True also rel
    [H, W] and ssim_map [H - 10, W - 10] (empty when the frame has no window)."""
    import torch
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.dtype not in (np.float64, np.uint8) or a.shape != b.shape or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("a and b must both be [H, W, 3] float64 or both [H, W, 3] uint8")
    h, w, _ = a.shape
    u8 = a.dtype == np.uint8
    p = rt_metrics_params(width=w, height=h, format=RT_METRICS_U8 if u8 else RT_METRICS_F64, peak=peak or 0.0, eps=eps or 0.0)
    if window is not None:
        p.window[:] = [float(t) for t in window]
    ws_bytes = image_metrics_workspace_bytes(w, h)
    d_a, d_b = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (a, b))
    dev = dict(dtype=torch.float64, device="cuda")
    d_summary, d_ws = torch.empty(8, **dev), torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    wh, ww = (h - 10, w - 10) if w >= 11 and h >= 11 else (0, 0)
    d_rel = torch.empty((h, w), **dev) if maps else None
    d_ssim = torch.empty((wh, ww), **dev) if maps and wh else None
    image_metrics_async(p, d_a.data_ptr(), d_b.data_ptr(), d_rel.data_ptr() if maps else 0,
                        d_ssim.data_ptr() if d_ssim is not None else 0, d_summary.data_ptr(), d_ws.data_ptr(), ws_bytes,
                        torch.cuda.current_stream().cuda_stream)
    s = d_summary.cpu().numpy()
    good = w * h - s[0]
    pk = peak or (255.0 if u8 else 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mse = s[1] / (3.0 * good)
        out = dict(mse=float(mse), rel_mse=float(s[2] / (3.0 * good)), psnr=float(10.0 * np.log10(pk * pk / mse)),
                   ssim=float(s[5] / s[4]), max_abs=float(s[3]), bad_pixels=int(s[0]), bad_windows=int(s[7]), summary=s)
    if maps:
        out["rel"] = d_rel.cpu().numpy()
        out["ssim_map"] = d_ssim.cpu().numpy() if d_ssim is not None else np.zeros((wh, ww))
    return out


def adaptive_workspace(width: int, height: int):
    """(bytes, layout dict of byte offsets and n_tiles) of the adaptive state (rt_adaptive_workspace_bytes)."""
    n, lay = C.c_uint64(), rt_adaptive_layout()
    _check(lib().rt_adaptive_workspace_bytes(width, height, C.byref(n), C.byref(lay)))
    return n.value, {k: getattr(lay, k) for k, _ in lay._fields_}


def adaptive_select_async(width: int, height: int, d_workspace_ptr: int, workspace_bytes: int, threshold: float,
                          eps: float, pass_spp: int, max_spp: int, stream_ptr: int = 0):
    """Every tile's error, then the list of the tiles above threshold and info (rt_adaptive_select_async)."""
    _check(lib().rt_adaptive_select_async(width, height, C.c_void_p(d_workspace_ptr), workspace_bytes, threshold, eps,
                                          pass_spp, max_spp, C.c_void_p(stream_ptr)))


def adaptive_select_rank_async(width: int, height: int, d_workspace_ptr: int, workspace_bytes: int, threshold: float,
                               eps: float, pass_spp: int, max_spp: int, rank: int, stream_ptr: int = 0):
    """adaptive_select_async with a tile's (rank + 1)-th largest pixel error as its error (rt_adaptive_select_rank_async)."""
    _check(lib().rt_adaptive_select_rank_async(width, height, C.c_void_p(d_workspace_ptr), workspace_bytes, threshold,
                                               eps, pass_spp, max_spp, rank, C.c_void_p(stream_ptr)))


def adaptive_resolve_async(params: RenderParams, d_workspace_ptr: int, workspace_bytes: int, d_mean_ptr: int,
                           d_sq_ptr: int, d_count_ptr: int = 0, stream_ptr: int = 0):
    """Accumulators / count -> mean, sq [H][W][3] f64 and (d_count_ptr 0: none) count [H][W] u32."""
    _check(lib().rt_adaptive_resolve_async(C.byref(params.to_c()), C.c_void_p(d_workspace_ptr), workspace_bytes,
                                           C.c_void_p(d_mean_ptr), C.c_void_p(d_sq_ptr), C.c_void_p(d_count_ptr),
                                           C.c_void_p(stream_ptr)))


def unpack_tiles_bytes_async(params: RenderParams, world: int, d_gathered_ptr: int, d_bytes_ptr: int,
                             stream_ptr: int = 0):
    """Gathered tiles -> PPM payload [H][W][3] u8 on the device (unpack + tonemap + gamma + bytes)."""
    _check(lib().rt_unpack_tiles_bytes_async(C.byref(params.to_c()), world, C.c_void_p(d_gathered_ptr),
                                             C.c_void_p(d_bytes_ptr), C.c_void_p(stream_ptr)))


def tonemap_bytes_async(d_rgb_ptr: int, n_pixels: int, d_bytes_ptr: int, stream_ptr: int = 0):
    """Device correct_gamma(aces_tonemap(.)) + PPM bytes of an HBM-resident mean image."""
    _check(lib().rt_tonemap_bytes_async(C.c_void_p(d_rgb_ptr), n_pixels, C.c_void_p(d_bytes_ptr),
                                        C.c_void_p(stream_ptr)))


# ------------------------------------------------------- output surface ----
def tonemap_gamma(mean_rgb: np.ndarray) -> np.ndarray:
    """correct_gamma(aces_tonemap(x)) per channel (postprocessing.rs:5-37)."""
    a = np.ascontiguousarray(mean_rgb, np.float64)
    out = np.empty_like(a)
    lib().rt_tonemap_gamma(a.ctypes.data_as(C.c_void_p), a.size // 3, out.ctypes.data_as(C.c_void_p))
    return out


def save_to_ppm(path: str, rgb: np.ndarray):
    """ppm::save_to_ppm of an already tonemapped [H, W, 3] image (ppm.rs:4-19)."""
    rgb = np.ascontiguousarray(rgb, np.float64)
    _check(lib().rt_save_ppm(path.encode(), rgb.shape[1], rgb.shape[0], rgb.ctypes.data_as(C.c_void_p)))


def generate_image(scene: Scene, params: RenderParams) -> np.ndarray:
    """generate_image (main.rs:85-114): tonemapped + gamma-corrected pixels."""
    img, _, _ = scene.generate_image(params)
    return tonemap_gamma(img)


def build_bvh(boxes: np.ndarray):
    """BVH::new over [n, 6] (min, max) boxes on the host -> (links [m,4], bounds [m,6], order [n], depth)."""
    boxes = np.ascontiguousarray(boxes, np.float64).reshape(-1, 6)
    n = C.c_uint64(0)
    depth = C.c_uint32(0)
    _check(lib().rt_bvh_build(boxes.ctypes.data_as(C.c_void_p), len(boxes), C.byref(n), None, None, None,
                              C.byref(depth)))
    links = np.zeros((n.value, 4), np.int64)
    bounds = np.zeros((n.value, 6), np.float64)
    order = np.zeros(len(boxes), np.uint64)
    _check(lib().rt_bvh_build(boxes.ctypes.data_as(C.c_void_p), len(boxes), C.byref(n),
                              links.ctypes.data_as(C.c_void_p), bounds.ctypes.data_as(C.c_void_p),
                              order.ctypes.data_as(C.c_void_p), C.byref(depth)))
    return links, bounds, order, depth.value


def build_bvh_device(boxes: np.ndarray, max_levels: int = 0):
    """build_bvh on the current HIP device -> (links, bounds, order, depth, on_device); on_device is 0
    when the host builder made the tree (rt_bvh_build_device).  max_levels 0: the library's cap."""
    boxes = np.ascontiguousarray(boxes, np.float64).reshape(-1, 6)
    n = C.c_uint64(max(1, 2 * len(boxes)))  # a tree over n boxes has at most 2n - 1 nodes
    depth, on_device = C.c_uint32(0), C.c_uint32(0)
    links = np.zeros((n.value, 4), np.int64)
    bounds = np.zeros((n.value, 6), np.float64)
    order = np.zeros(len(boxes), np.uint64)
    _check(lib().rt_bvh_build_device(boxes.ctypes.data_as(C.c_void_p), len(boxes), max_levels, C.byref(n),
                                     links.ctypes.data_as(C.c_void_p), bounds.ctypes.data_as(C.c_void_p),
                                     order.ctypes.data_as(C.c_void_p), C.byref(depth), C.byref(on_device)))
    return links[:n.value].copy(), bounds[:n.value].copy(), order, depth.value, on_device.value


def byte_thresholds() -> np.ndarray:
    """The device epilogue's 255 byte thresholds on the tonemapped value (host only)."""
    out = np.zeros(255, np.float64)
    _check(lib().rt_byte_thresholds(out.ctypes.data_as(C.c_void_p)))
    return out


def sample_chunks(params: RenderParams):
    """(chunks, chunk_spp) of the device's work units for this frame (rt_sample_chunks)."""
    k, cs = C.c_uint32(), C.c_uint32()
    _check(lib().rt_sample_chunks(C.byref(params.to_c()), C.byref(k), C.byref(cs)))
    return k.value, cs.value


def probe_fp64(op: int, a: np.ndarray, b: Optional[np.ndarray] = None) -> np.ndarray:
    a = np.ascontiguousarray(a, np.float64)
    bb = None if b is None else np.ascontiguousarray(b, np.float64)
    out = np.zeros_like(a)
    _check(lib().rt_probe_fp64(op, a.ctypes.data_as(C.c_void_p),
                               None if bb is None else bb.ctypes.data_as(C.c_void_p), len(a),
                               out.ctypes.data_as(C.c_void_p)))
    return out

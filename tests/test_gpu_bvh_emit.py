"""Device record emission (bvh_emit.hip, rt.Scene(desc, build="device", records="device")):
the triangle BVHs' arrays written on the device against the host-built scene — the same
bytes (rt_scene_checksum hashes every array with its size, in allocation order), the same
counts, the same image.  RT_LAYOUT_DEVICE_RECORDS must be set, so a path that silently fell
back to the host would fail; then the fallbacks and the argument checks."""
import ctypes as C

import numpy as np
import pytest

from fuzz_scenes import random_scene

pytestmark = pytest.mark.gpu


def _mesh(rt, n, seed=0, same=(), zeros=False, nan=False):
    """n random small triangles with f32-valued world-space vertices (then same[i] copies of
    the i-th one), unit normals, one diffuse material, as an RT_TRI_GLTF description."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, (n, 1, 3))
    v = (a + np.concatenate([np.zeros((n, 1, 3)), rng.uniform(-0.2, 0.2, (n, 2, 3))], 1)).astype(np.float32)
    v = np.concatenate([v] + [np.repeat(v[i:i + 1], c, 0) for i, c in enumerate(same)]).astype(np.float64).reshape(-1, 9)
    if zeros:
        v[3::5, 0:9:4] = -0.0      # a coordinate of each vertex of every fifth triangle
        v[7, 3:6] = v[7, 6:9] = v[7, 0:3]  # zero area: ng is NaN and 1/area inf in the records
        assert np.signbit(v[v == 0.0]).any()
    if nan:
        v[len(v) // 2, 7] = np.nan  # in c, the last vertex box_extend takes: the NaN stays in the box
    nrm = rng.normal(size=(len(v), 3, 3))
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    mats = np.zeros(1, rt.MATERIAL_DTYPE)
    mats["kind"], mats["ior"], mats["color"] = rt.RT_MAT_DIFFUSE, 1.0, (0.8, 0.7, 0.6)
    desc = rt.SceneDesc(materials=mats, shapes=np.zeros(0, rt.SHAPE_DTYPE), tri_vertices=v,
                        tri_normals=nrm.reshape(-1, 9), tri_material=np.zeros(len(v), np.uint32),
                        tri_mode=rt.RT_TRI_GLTF)
    return desc, rt.RenderParams(24, 16, spp=4, ray_depth=4, bg_color=(0.3, 0.4, 0.5), cam_position=(0.0, 0.0, -3.0))


def _fuzz(seed, tri_only):
    def make(rt):
        return rt.parse_scene(random_scene(seed, spp=4, tri_only=tri_only))
    return make


CASES = {
    "fuzz-compact": _fuzz(5008, True),          # compact and pair layouts, no lights
    "fuzz-lights": _fuzz(5004, True),           # light triangles: bvh[5], emitted without the compact layout
    "fuzz-rotated": _fuzz(5041, False),         # shapes too, a rotated mesh: inexact f32, no compact layout
    "tri-1": lambda rt: _mesh(rt, 1),           # a leaf root: no compact layout
    "tri-4": lambda rt: _mesh(rt, 4),
    "tri-5": lambda rt: _mesh(rt, 5),           # the first split
    "tri-300": lambda rt: _mesh(rt, 300),
    # SameNode leaves of 201 (a kLeafRef slot, a block-written multi-line leaf), 41 (block-written,
    # packed) and 11 triangles (the lane groups' loop over lines)
    "same-leaf": lambda rt: _mesh(rt, 60, same=(200, 40, 10)),
    "tri-70000": lambda rt: _mesh(rt, 70000),   # crosses the block boundaries of the three-launch scans
    "zeros": lambda rt: _mesh(rt, 40, zeros=True),    # -0.0 coordinates, NaN and inf record bytes
}


@pytest.mark.parametrize("case", list(CASES))
def test_device_records_match_host(rt, case):
    desc, params = CASES[case](rt)
    host = rt.Scene(desc)
    hi = host.info()
    if case == "fuzz-rotated":
        assert hi["n_triangles"] > 4 and not hi["layout_flags"] & rt.RT_LAYOUT_COMPACT_TRIS
    if case == "fuzz-lights":
        assert hi["n_light_triangles"] > 0
    if case in ("fuzz-compact", "same-leaf", "tri-300", "tri-70000"):
        assert hi["layout_flags"] & rt.RT_LAYOUT_COMPACT_TRIS
    dev = rt.Scene(desc, build="device", records="device")
    di = dev.info()
    both = rt.RT_LAYOUT_DEVICE_BUILT | rt.RT_LAYOUT_DEVICE_RECORDS
    assert di["layout_flags"] & both == both and not hi["layout_flags"] & both
    assert di["layout_flags"] & ~both == hi["layout_flags"]
    assert dev.checksum() == host.checksum()
    for k in ("bvh_nodes", "bvh_depth", "device_bytes", "n_triangles", "n_light_triangles"):
        assert di[k] == hi[k], k
    params = params.replace(width=24, height=16, spp=4)
    assert np.array_equal(dev.generate_image(params)[0], host.generate_image(params)[0])


def test_device_records_fall_back(rt):
    desc, _ = _mesh(rt, 300, nan=True)
    dev = rt.Scene(desc, build="device", records="device")
    assert dev.checksum() == rt.Scene(desc).checksum()
    assert not dev.info()["layout_flags"] & rt.RT_LAYOUT_DEVICE_RECORDS


def test_device_records_arguments(rt):
    desc, _ = _mesh(rt, 5)
    with pytest.raises(ValueError):
        rt.Scene(desc, build="host", records="device")
    d, keep = desc.to_c()
    h = C.c_void_p()
    assert rt.lib().rt_scene_create_ex(C.byref(d), rt.RT_BUILD_DEVICE_RECORDS, C.byref(h)) == rt.RT_ERR_INVALID
    assert not h.value and b"RT_BUILD_DEVICE" in rt.lib().rt_last_error()
    del keep

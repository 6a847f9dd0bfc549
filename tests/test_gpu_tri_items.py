"""Device items (tri_items.hip, rt.Scene(desc, build="device", records="device", items="device")):
the per-triangle items computed on the device from the description's arrays against the
host-built scene — the same bytes (rt_scene_checksum), the same counts, the same image.
RT_LAYOUT_DEVICE_ITEMS must be set, so a path that silently fell back to the host's items
would fail; then the fallback and the argument checks."""
import ctypes as C

import numpy as np
import pytest

from fuzz_scenes import random_scene

pytestmark = pytest.mark.gpu


def _params(rt):
    return rt.RenderParams(24, 16, spp=4, ray_depth=4, bg_color=(0.3, 0.4, 0.5), cam_position=(0.0, 0.0, -3.0))


def _mesh(rt, n, mode="gltf", lights=False, zeros=False, nan_at=None):
    """n random small triangles with f32-valued vertices.  gltf: unit normals given; custom:
    no positions and no rotations.  lights: a second, emissive material on every third
    triangle.  zeros: -0.0 coordinates and a zero-area triangle.  nan_at: the vertex double
    (0-8) of the middle triangle that is NaN."""
    rng = np.random.default_rng(n)
    a = rng.uniform(-1.0, 1.0, (n, 1, 3))
    v = (a + np.concatenate([np.zeros((n, 1, 3)), rng.uniform(-0.2, 0.2, (n, 2, 3))], 1)).astype(np.float32)
    v = v.astype(np.float64).reshape(-1, 9)
    if zeros:
        v[3::5, 0:9:4] = -0.0      # a coordinate of each vertex of every fifth triangle
        v[7, 3:6] = v[7, 6:9] = v[7, 0:3]  # zero area: ng is NaN and 1/area inf
    if nan_at is not None:
        v[n // 2, nan_at] = np.nan
    nrm = rng.normal(size=(n, 3, 3))
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    mats = np.zeros(2 if lights else 1, rt.MATERIAL_DTYPE)
    mats["kind"], mats["ior"], mats["color"] = rt.RT_MAT_DIFFUSE, 1.0, (0.8, 0.7, 0.6)
    mat = np.zeros(n, np.uint32)
    if lights:
        mats["emission"][1] = (4.0, 3.0, 2.0)
        mat[::3] = 1
    gltf = mode == "gltf"
    desc = rt.SceneDesc(materials=mats, shapes=np.zeros(0, rt.SHAPE_DTYPE), tri_vertices=v,
                        tri_normals=nrm.reshape(-1, 9) if gltf else None, tri_position=None, tri_rotation=None,
                        tri_material=mat, tri_mode=rt.RT_TRI_GLTF if gltf else rt.RT_TRI_CUSTOM)
    return desc, _params(rt)


def _fuzz(seed, tri_only):
    return lambda rt: rt.parse_scene(random_scene(seed, spp=4, tri_only=tri_only))


CASES = {f"tri-{n}": (lambda n: lambda rt: _mesh(rt, n))(n) for n in (1, 5, 63, 64, 65, 300)}  # around the 64-triangle tile
CASES.update({
    "lights-70000": lambda rt: _mesh(rt, 70000, lights=True),   # the light scan crosses its block sums
    "fuzz-lights": _fuzz(5004, True),                           # RT_TRI_CUSTOM, light triangles
    "fuzz-rotated": _fuzz(5041, False),                         # RT_TRI_CUSTOM rotated, with shapes (gid offset)
    "custom-identity": lambda rt: _mesh(rt, 70, mode="custom", zeros=True),  # NULL position / rotation, -0.0
    "nan-fixup": lambda rt: _mesh(rt, 40, zeros=True, nan_at=4),  # NaN in b: the box stays finite, the records hold NaNs
})


@pytest.mark.parametrize("case", list(CASES))
def test_device_items_match_host(rt, case):
    desc, params = CASES[case](rt)
    host = rt.Scene(desc)
    hi = host.info()
    dev = rt.Scene(desc, build="device", records="device", items="device")
    di = dev.info()
    three = rt.RT_LAYOUT_DEVICE_BUILT | rt.RT_LAYOUT_DEVICE_RECORDS | rt.RT_LAYOUT_DEVICE_ITEMS
    assert di["layout_flags"] & three == three and not hi["layout_flags"] & three
    assert di["layout_flags"] & ~three == hi["layout_flags"]
    assert dev.checksum() == host.checksum()
    for k in ("bvh_nodes", "bvh_depth", "device_bytes", "n_triangles", "n_light_triangles"):
        assert di[k] == hi[k], k
    if case == "lights-70000":
        assert di["n_light_triangles"] > 1024
    if case == "fuzz-lights":
        assert di["n_light_triangles"] > 0
    params = params.replace(width=24, height=16, spp=4)
    assert np.array_equal(dev.generate_image(params)[0], host.generate_image(params)[0], equal_nan=case == "nan-fixup")


def test_device_items_fall_back(rt):
    desc, _ = _mesh(rt, 300, nan_at=7)  # in c, the last vertex box_extend takes: the NaN stays in the box
    dev = rt.Scene(desc, build="device", records="device", items="device")
    assert dev.checksum() == rt.Scene(desc).checksum()
    assert not dev.info()["layout_flags"] & rt.RT_LAYOUT_DEVICE_ITEMS


def test_device_items_arguments(rt):
    desc, _ = _mesh(rt, 5)
    for kw in ({}, {"build": "device"}, {"records": "device"}):
        with pytest.raises(ValueError):
            rt.Scene(desc, items="device", **kw)
    d, keep = desc.to_c()
    for flags in (rt.RT_BUILD_DEVICE_ITEMS, rt.RT_BUILD_DEVICE_ITEMS | rt.RT_BUILD_DEVICE):
        h = C.c_void_p()
        assert rt.lib().rt_scene_create_ex(C.byref(d), flags, C.byref(h)) == rt.RT_ERR_INVALID
        assert not h.value and b"RT_BUILD_DEVICE_RECORDS" in rt.lib().rt_last_error()
    del keep
    desc.tri_material[3] = 1  # one material: out of range
    errors = []
    for kw in ({}, {"build": "device", "records": "device", "items": "device"}):
        with pytest.raises(Exception) as e:
            rt.Scene(desc, **kw)
        errors.append(str(e.value))
    assert errors[0] == errors[1] and "triangle material out of range" in errors[0]

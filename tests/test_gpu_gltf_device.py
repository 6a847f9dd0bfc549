"""Device meshes (gltf_items.hip, rt.Scene.from_parsed(parsed, ..., meshes="device")): a scene
whose glTF meshes were flattened on the device from the buffers' bytes against the
host-built one: the same bytes (rt_scene_checksum), the same counts, the same image.
RT_LAYOUT_DEVICE_MESHES must be set, so a path that silently fell back to the host flatten
would fail; then the fallback and the argument checks."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
import gltf_scenes

pytestmark = pytest.mark.gpu
DEVICE = dict(build="device", records="device", items="device", meshes="device")


def _generated(script, name, *args):
    def make(d):
        subprocess.run([sys.executable, os.path.join(REPO, "scenes", script), str(d), "--name", name, *args],
                       check=True, capture_output=True)
        return os.path.join(str(d), name + ".gltf")
    return make


def _room(d):
    return gltf_scenes.write_room(str(d))[0]


def _patch(path, g, accessor, element, data):
    """Overwrites one element of an accessor in the room's .bin."""
    a = g["accessors"][accessor]
    v = g["bufferViews"][a["bufferView"]]
    with open(path[:-5] + ".bin", "r+b") as f:
        f.seek(v["byteOffset"] + a.get("byteOffset", 0) + element * v.get("byteStride", data.nbytes))
        f.write(data.tobytes())


def _room_zero_normal(d):
    path, g = gltf_scenes.write_room(str(d))
    _patch(path, g, 4, 20, np.zeros(3, np.float32))  # a sphere normal: 0 * inf in normalize
    return path


CASES = {"room": _room, "room-zero-normal": _room_zero_normal,
         "atrium": _generated("gen_sponza_like.py", "atrium", "--scale", "0.1")}
CASES.update({f"hairball-{n}": _generated("gen_hairball.py", "hb", "--tris", str(n)) for n in (1, 63, 64, 65, 300)})


@pytest.mark.parametrize("case", list(CASES))
def test_device_meshes_match_host(rt, tmp_path, case):
    path = CASES[case](tmp_path)
    desc, params = rt.load_gltf(path, 24, 16, 4)
    host = rt.Scene(desc)
    hi = host.info()
    parsed = rt.load_gltf(path, 24, 16, 4, defer=True)
    dev = rt.Scene.from_parsed(parsed, **DEVICE)
    di = dev.info()
    four = (rt.RT_LAYOUT_DEVICE_BUILT | rt.RT_LAYOUT_DEVICE_RECORDS | rt.RT_LAYOUT_DEVICE_ITEMS |
            rt.RT_LAYOUT_DEVICE_MESHES)
    assert di["layout_flags"] & four == four and not hi["layout_flags"] & four
    assert di["layout_flags"] & ~four == hi["layout_flags"]
    assert dev.checksum() == host.checksum()
    for k in ("bvh_nodes", "bvh_depth", "device_bytes", "n_triangles", "n_light_triangles"):
        assert di[k] == hi[k], k
    assert di["n_triangles"] > 0 and di["n_light_triangles"] > 0
    assert parsed.params == params
    assert np.array_equal(dev.generate_image(params)[0], host.generate_image(params)[0],
                          equal_nan=case == "room-zero-normal")
    parsed.close()


def test_device_meshes_fall_back(rt, tmp_path):
    """A non-finite position in a vertex no triangle references: the host's error, from gf_scan's flag."""
    path, g = gltf_scenes.write_room(str(tmp_path))
    _patch(path, g, 5, 92, np.array([14], np.uint32))               # the one corner that referenced sphere vertex 16
    _patch(path, g, 3, 16, np.array([np.inf, 1.0, 0.0], np.float32))
    with pytest.raises(rt.RtError) as eager:
        rt.load_gltf(path, 8, 8, 1)
    with pytest.raises(rt.RtError) as device:
        rt.Scene.from_parsed(rt.load_gltf(path, 8, 8, 1, defer=True), **DEVICE)
    assert "non-affine" in str(eager.value) and str(device.value) == str(eager.value)


def test_device_meshes_arguments(rt, tmp_path):
    parsed = rt.load_gltf(_room(tmp_path), 8, 8, 1, defer=True)
    with pytest.raises(ValueError):
        rt.Scene.from_parsed(parsed, build="device", records="device", meshes="device")
    h = C.c_void_p()
    for flags in (rt.RT_BUILD_DEVICE_MESHES, rt.RT_BUILD_DEVICE_MESHES | rt.RT_BUILD_DEVICE | rt.RT_BUILD_DEVICE_RECORDS):
        assert rt.lib().rt_scene_create_parsed(parsed.handle, flags, C.byref(h)) == rt.RT_ERR_INVALID
        assert not h.value and b"RT_BUILD_DEVICE_ITEMS" in rt.lib().rt_last_error()
    d, keep = parsed.desc().to_c()
    assert rt.lib().rt_scene_create_ex(C.byref(d), 0xf, C.byref(h)) == rt.RT_ERR_INVALID and not h.value
    del keep
    parsed.close()

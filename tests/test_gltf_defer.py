"""The deferred glTF parse (rt_load_gltf_ex with RT_GLTF_DEFER, rt.load_gltf(..., defer=True)):
the description it makes on first use is rt_load_gltf's byte for byte, and every error is
the eager load's, whether it surfaces at the load or at .desc()."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
import gltf_scenes


def _hairball(d):
    subprocess.run([sys.executable, os.path.join(REPO, "scenes", "gen_hairball.py"), str(d), "--tris", "300",
                    "--name", "hb"], check=True, capture_output=True)
    return os.path.join(str(d), "hb.gltf")


@pytest.mark.parametrize("scene", ["room", "hairball"])
def test_deferred_description_is_the_eager_one(rt, tmp_path, scene):
    path = gltf_scenes.write_room(str(tmp_path))[0] if scene == "room" else _hairball(tmp_path)
    desc, params = rt.load_gltf(path, 40, 30, 4)
    parsed = rt.load_gltf(path, 40, 30, 4, defer=True)
    assert parsed.params == params
    lazy = parsed.desc()
    assert lazy.tri_mode == desc.tri_mode and len(desc.tri_material) > 0
    for name in ("materials", "shapes", "tri_vertices", "tri_normals", "tri_material"):
        a, b = getattr(lazy, name), getattr(desc, name)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    assert lazy.tri_position is None and lazy.tri_rotation is None
    parsed.close()


def _odd_index_count(g):
    g["accessors"][2]["count"] -= 1  # the room's u16 indices


def _fourth_row(g):
    g["nodes"][4]["matrix"][3] = 0.25  # the matrix node: pos.w = 1 + 0.25 x


def _index_out_of_range(path, g):
    v = g["bufferViews"][g["accessors"][2]["bufferView"]]
    with open(path[:-5] + ".bin", "r+b") as f:
        f.seek(v["byteOffset"] + 2 * 7)
        f.write(np.uint16(60000).tobytes())


@pytest.mark.parametrize("case", ["odd-index-count", "fourth-row", "index-out-of-range"])
def test_deferred_errors_are_the_eager_ones(rt, tmp_path, case):
    if case == "index-out-of-range":
        path, g = gltf_scenes.write_room(str(tmp_path))
        _index_out_of_range(path, g)
    else:
        path = gltf_scenes.write_variant(str(tmp_path), _odd_index_count if case == "odd-index-count" else _fourth_row)
    with pytest.raises(rt.RtError) as eager:
        rt.load_gltf(path, 8, 8, 1)
    with pytest.raises(rt.RtError) as deferred:
        rt.load_gltf(path, 8, 8, 1, defer=True).desc()
    assert deferred.value.code == eager.value.code and str(deferred.value) == str(eager.value)

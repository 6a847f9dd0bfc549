"""The device BVH builder (bvh_build.hip, rt_bvh_build_device) against the oracle's
sequential builder: the same tree node for node — links, leaf order, depth, and the
bounds bit for bit (zero signs count).  Every device case also checks on_device, so a
builder that always fell back to the host would fail.  Then the fallbacks, and scenes
built with build="device" against the host-built ones."""
import numpy as np
import pytest

from fuzz_scenes import random_scene
from test_abi import _boxes

pytestmark = pytest.mark.gpu


def _identical(rng, n):
    return np.tile([0, 0, 0, 1, 1, 1.0], (n, 1))


def _clustered(rng, n):  # a dense cluster plus far outliers: a deep, unbalanced tree
    b = _boxes(rng, n)
    b[: n // 2] *= 1e-3
    return b


def _grid(rng, n):  # integer centres: heavy equal-midpoint ties on every axis
    return _boxes(rng, n, grid=True)


def _neg_zero(rng, n):  # grid boxes snapped to integers, a third of the zero coordinates as -0.0
    b = np.round(_boxes(rng, n, grid=True))
    zero = b == 0.0
    b[zero & (rng.integers(0, 3, b.shape) == 0)] = -0.0
    assert np.signbit(b).any() and (zero & ~np.signbit(b)).any()
    return b


CASES = [(_boxes, n) for n in (1, 4, 5, 37, 64, 65, 257)] + [
    (_grid, 2000), (_grid, 70000), (_boxes, 70000), (_clustered, 70000),
    (_identical, 9), (_identical, 5000), (_neg_zero, 300)]


def _same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
            and np.array_equal(a[2], b[2]) and a[3] == b[3])


@pytest.mark.parametrize("make,n", CASES, ids=[f"{m.__name__.strip('_')}-{n}" for m, n in CASES])
def test_device_builder_matches_oracle(rt, orc, make, n):
    boxes = make(np.random.default_rng(n), n)
    want = orc.build_bvh(boxes)
    if make is _neg_zero:  # the host builder and the oracle agree on this input byte for byte
        assert _same(rt.build_bvh(boxes), want)
    got = rt.build_bvh_device(boxes)
    assert got[4] == 1
    assert _same(got, want)
    if make is _identical:
        assert len(got[0]) == 1 and got[3] == 1  # SameNode at the root: one leaf


@pytest.mark.parametrize("case", ["nan", "inf", "max_levels"])
def test_device_builder_falls_back(rt, case):
    boxes = _boxes(np.random.default_rng(3), 500)
    if case == "nan":
        boxes[123, 4] = np.nan
    elif case == "inf":
        boxes[77, 5] = np.inf
    got = rt.build_bvh_device(boxes, max_levels=2 if case == "max_levels" else 0)
    assert got[4] == 0
    assert _same(got, rt.build_bvh(boxes))


@pytest.mark.parametrize("seed,lights", [(5008, False), (5004, True)])
def test_scene_built_on_device(rt, seed, lights):
    desc, params = rt.parse_scene(random_scene(seed, spp=4, tri_only=True))
    host, dev = rt.Scene(desc), rt.Scene(desc, build="device")
    assert (dev.info()["n_light_triangles"] > 0) == lights and dev.info()["n_triangles"] > 4
    assert dev.checksum() == host.checksum()
    assert dev.info()["layout_flags"] & rt.RT_LAYOUT_DEVICE_BUILT
    assert not host.info()["layout_flags"] & rt.RT_LAYOUT_DEVICE_BUILT
    params = params.replace(width=24, height=16, spp=4)
    assert np.array_equal(dev.generate_image(params)[0], host.generate_image(params)[0])

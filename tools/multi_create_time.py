"""rt_multi_create of a bench workload's scene with N replicas (one GPU: a device listed N
times, RT_MULTI_PEER): the host build once, devices[0] from the host, the replicas filled
device to device from devices[0]; prints each replica's upload_ms beside a plain
rt_scene_create (what one replica's own host upload costs).  --build device builds that
plain scene's triangle BVHs on the device (rt_scene_create_ex, RT_BUILD_DEVICE) and prints a
second device-built scene's times too (the first one loads the builder's code object);
--records device (with --build device) also writes the triangle BVHs' arrays on the device
(RT_BUILD_DEVICE_RECORDS); --items device (with both) computes the per-triangle items there
too (RT_BUILD_DEVICE_ITEMS); --runs K times K scenes after that warm-up one; --no-multi stops
before rt_multi_create, which always builds on the host.  --from-gltf host|device (a glTF
workload, with the three device options) times load + creation from the .gltf path instead,
a warm-up scene and then --runs timed ones: host is rt_load_gltf + rt_scene_create_ex, device
is rt_load_gltf_ex (RT_GLTF_DEFER) + rt_scene_create_parsed with RT_BUILD_DEVICE_MESHES.
    python tools/multi_create_time.py [WORKLOAD] [N] [--build host|device] [--records host|device]
                                      [--items host|device] [--runs K] [--no-multi] [--from-gltf host|device]"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import torch  # noqa: E402,F401  (one HIP runtime per process)
import bench  # noqa: E402
from conftest import load_package  # noqa: E402

rt = load_package()


def option(name, default):
    if name not in sys.argv:
        return default
    k = sys.argv.index(name)
    value = sys.argv[k + 1]
    del sys.argv[k:k + 2]
    return value


build, records, runs = option("--build", "host"), option("--records", "host"), int(option("--runs", "1"))
items = option("--items", "host")
from_gltf = option("--from-gltf", None)
no_multi = "--no-multi" in sys.argv
if no_multi:
    sys.argv.remove("--no-multi")
wl = sys.argv[1] if len(sys.argv) > 1 else "C5"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 4
scene_file, W, H, spp, _ = bench.WORKLOADS[wl]
path = os.path.join(HERE, "..", "scenes", "gen", scene_file[5:] + ".gltf")
if not (from_gltf and os.path.exists(path)):  # (load_workload also generates a glTF workload's files)
    desc, params = bench.load_workload(rt, scene_file, W, H, spp)
if from_gltf:
    for k in range(runs + 1):
        t = time.perf_counter()
        if from_gltf == "device":
            parsed = rt.load_gltf(path, W, H, spp, defer=True)
            load = time.perf_counter() - t
            s = rt.Scene.from_parsed(parsed, build=build, records=records, items=items, meshes="device")
        else:
            d, _ = rt.load_gltf(path, W, H, spp)
            load = time.perf_counter() - t
            s = rt.Scene(d, build=build, records=records, items=items)
        total = time.perf_counter() - t
        i0 = s.info()
        assert bool(i0["layout_flags"] & rt.RT_LAYOUT_DEVICE_MESHES) == (from_gltf == "device")
        print(f"{wl} from .gltf ({from_gltf} meshes){' warm-up' if k == 0 else ''}: load {load * 1e3:.0f} ms, "
              f"creation {(total - load) * 1e3:.0f} ms (build {i0['build_ms']:.0f} ms, host upload "
              f"{i0['upload_ms']:.1f} ms), sum {total * 1e3:.0f} ms", flush=True)
        del s
    sys.exit(0)
for _ in range(runs + 1 if build == "device" else runs):
    t = time.perf_counter()
    s = rt.Scene(desc, build=build, records=records, items=items)
    one = time.perf_counter() - t
    i0 = s.info()
    if build == "device":
        assert i0["layout_flags"] & rt.RT_LAYOUT_DEVICE_BUILT
    assert bool(i0["layout_flags"] & rt.RT_LAYOUT_DEVICE_RECORDS) == (records == "device")
    assert bool(i0["layout_flags"] & rt.RT_LAYOUT_DEVICE_ITEMS) == (items == "device")
    print(f"{wl}: rt_scene_create ({build} build, {records} records, {items} items) {one * 1e3:.0f} ms (build {i0['build_ms']:.0f} ms, host upload {i0['upload_ms']:.1f} ms, "
          f"{i0['device_bytes'] / 1e9:.3f} GB)", flush=True)
    del s
if no_multi:
    sys.exit(0)
t = time.perf_counter()
m = rt.MultiScene(desc, [0] * n, peer=True)
tot = time.perf_counter() - t
for i in range(n):
    inf = m.scene_info(i)
    print(f"  replica {i}: upload_ms {inf['upload_ms']:.1f} ({'host' if i == 0 else 'device-to-device fill'}), "
          f"{inf['device_bytes'] / 1e9:.3f} GB", flush=True)
print(f"rt_multi_create x{n}: {tot * 1e3:.0f} ms", flush=True)

"""rt_bvh_build (host) against rt_bvh_build_device on the same boxes, alternating, one
GPU: median and spread of the wall time of each call (both return synchronised), and a
byte comparison of the two trees at the timed size.
    python tools/bvh_build_time.py [--sizes 1000000 10000000] [--c5] [--runs 5] [--device-only]
--c5: the triangle boxes of the C5 hairball (bench.py's workload), as build_scene makes them."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import torch  # noqa: E402,F401  (one HIP runtime per process)
import bench  # noqa: E402
from conftest import load_package  # noqa: E402

rt = load_package()
L = rt.lib()


def random_boxes(n):  # tests/test_abi.py _boxes
    rng = np.random.default_rng(n)
    c, h = rng.uniform(-10, 10, (n, 3)), rng.uniform(0.01, 1.0, (n, 3))
    return np.concatenate([c - h, c + h], axis=1)


def c5_boxes():  # scene_build.cpp: box of a, a + (b - a), a + (c - a)
    scene_file, W, H, spp, _ = bench.WORKLOADS["C5"]
    desc, _ = bench.load_workload(rt, scene_file, W, H, spp)
    v = np.asarray(desc.tri_vertices, np.float64).reshape(-1, 3, 3)
    a = v[:, 0]
    p = np.stack([a, a + (v[:, 1] - a), a + (v[:, 2] - a)], axis=1)
    return np.concatenate([p.min(axis=1), p.max(axis=1)], axis=1)


class Out:
    def __init__(self, n):
        self.links = np.zeros((2 * n, 4), np.int64)
        self.bounds = np.zeros((2 * n, 6), np.float64)
        self.order = np.zeros(n, np.uint64)
        self.n, self.depth, self.on_device = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)

    def args(self):
        return (self.links.ctypes.data_as(C.c_void_p), self.bounds.ctypes.data_as(C.c_void_p),
                self.order.ctypes.data_as(C.c_void_p), C.byref(self.depth))


def build(boxes, out, device):
    out.n.value = len(out.links)
    p = boxes.ctypes.data_as(C.c_void_p)
    t = time.perf_counter()
    if device:
        rc = L.rt_bvh_build_device(p, len(boxes), 0, C.byref(out.n), *out.args(), C.byref(out.on_device))
    else:
        rc = L.rt_bvh_build(p, len(boxes), C.byref(out.n), *out.args())
    dt = time.perf_counter() - t
    assert rc == 0, L.rt_last_error()
    assert not device or out.on_device.value == 1, "the device builder fell back to the host"
    return dt * 1e3


def stats(ms):
    return f"median {statistics.median(ms):.1f} ms (min {min(ms):.1f}, max {max(ms):.1f}, {len(ms)} runs)"


ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="*", default=[1_000_000, 10_000_000])
ap.add_argument("--c5", action="store_true")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--device-only", action="store_true", help="no host builds (a profiler run of the device builder)")
args = ap.parse_args()
build(random_boxes(1000), Out(1000), True)  # loads the code object
sets = [(f"{n} random boxes", random_boxes(n)) for n in args.sizes]
if args.c5:
    sets.append(("C5 triangle boxes", c5_boxes()))
for name, boxes in sets:
    boxes = np.ascontiguousarray(boxes)
    h, d = Out(len(boxes)), Out(len(boxes))
    host_ms, dev_ms = [], []
    for run in range(args.runs + 1):  # run 0 warms up
        th = None if args.device_only else build(boxes, h, False)
        td = build(boxes, d, True)
        if run:
            host_ms.append(th)
            dev_ms.append(td)
    print(f"{name}: {d.n.value} nodes, depth {d.depth.value}", flush=True)
    print(f"  device {stats(dev_ms)}", flush=True)
    if not args.device_only:
        m = d.n.value
        same = (h.n.value == m and h.depth.value == d.depth.value and np.array_equal(h.links[:m], d.links[:m])
                and np.array_equal(h.bounds[:m].view(np.uint64), d.bounds[:m].view(np.uint64))
                and np.array_equal(h.order, d.order))
        print(f"  host   {stats(host_ms)}", flush=True)
        print(f"  host/device {statistics.median(host_ms) / statistics.median(dev_ms):.2f}x, trees identical: {same}",
              flush=True)
        assert same

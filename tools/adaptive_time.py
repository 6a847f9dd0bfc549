"""Device-event times of the adaptive-sampling calls (DESIGN.md §4 "Adaptive sampling").

    python tools/adaptive_time.py pipeline [--sizes 1920x1080,3840x2160] [--rank 12]
    python tools/adaptive_time.py form [--workloads C2,C3] [--spp 32]
    python tools/adaptive_time.py frame [--workload C2] [--pass-spp 32] [--max-spp 256] [--threshold 0.05] [--rank 12]

pipeline: rt_adaptive_select_async and rt_adaptive_resolve_async on synthetic state, the median of
  --calls calls after two warm-up calls, with the bytes they have to move.  as_accumulate has no
  call of its own; its time comes from a kernel trace of `frame` (rocprofv3 --kernel-trace --stats).
form: an all-tiles pass (the list form of the moments kernel + as_accumulate) against
  rt_render_moments at the same spp, alternating, --calls each.
frame: the driver against the fixed frame of max_spp samples: samples spent, time, and the largest
  tile error of both (the fixed frame's from a single pass of max_spp samples).
"""
import argparse
import ctypes as C
import importlib.util
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
spec = importlib.util.spec_from_file_location("rt_amd", os.path.join(REPO, "cpu-raytracing-rt_amd", "__init__.py"))
rt = importlib.util.module_from_spec(spec)
sys.modules["rt_amd"] = rt
spec.loader.exec_module(rt)


def timed(fn, calls, warm=2):
    out = []
    for call in range(calls + warm):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if call >= warm:
            out.append(e0.elapsed_time(e1))
    return out


def spread(ms):
    return f"{statistics.median(ms):.3f} ms (min {min(ms):.3f}, max {max(ms):.3f})"


def workspace(w, h):
    nbytes, lay = rt.adaptive_workspace(w, h)
    return torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), lay


def view(ws, lay, key, dtype, n):
    return ws[lay[key]:lay[key] + n * dtype.itemsize].view(dtype)


def load(workload, spp):
    import bench
    scene_file, w, h, _, _ = bench.WORKLOADS[workload]
    desc, params = bench.load_workload(rt, scene_file, w, h, spp)
    return rt.Scene(desc), params


def pipeline(a):
    for size in a.sizes.split(","):
        w, h = map(int, size.split("x"))
        ws, lay = workspace(w, h)
        n = lay["n_tiles"]
        g = torch.Generator(device="cuda").manual_seed(w)
        s = torch.rand(n * 768, generator=g, dtype=torch.float64, device="cuda") * 16.0 + 1.0
        view(ws, lay, "acc_sum", torch.float64, n * 768).copy_(s)
        view(ws, lay, "acc_sq", torch.float64, n * 768).copy_(s * s / 16.0 * (1.0 + torch.rand_like(s)))
        view(ws, lay, "tile_count", torch.int32, n).fill_(16)
        p = rt.RenderParams(w, h)
        mean = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
        sq, count = torch.empty_like(mean), torch.empty((h, w), dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        sel = timed(lambda: rt.adaptive_select_async(w, h, ws.data_ptr(), ws.numel(), 0.05, 0.0, 16, 256, stream), a.calls)
        if a.rank is not None:  # plain and ranked select alternating, call by call
            plain, ranked = [], []
            for call in range(a.calls + 2):
                t = (timed(lambda: rt.adaptive_select_async(w, h, ws.data_ptr(), ws.numel(), 0.05, 0.0, 16, 256, stream), 1, 0)[0],
                     timed(lambda: rt.adaptive_select_rank_async(w, h, ws.data_ptr(), ws.numel(), 0.05, 0.0, 16, 256, a.rank,
                                                                 stream), 1, 0)[0])
                if call >= 2:
                    plain.append(t[0])
                    ranked.append(t[1])
            print(f"{size}, {n} tiles, alternating: select {spread(plain)}; select at rank {a.rank} {spread(ranked)}; "
                  f"ratio of medians {statistics.median(ranked) / statistics.median(plain):.2f}")
        res = timed(lambda: rt.adaptive_resolve_async(p, ws.data_ptr(), ws.numel(), mean.data_ptr(), sq.data_ptr(),
                                                      count.data_ptr(), stream), a.calls)
        b_sel, b_res = n * (12288 + 4 + 12) + n * 16, n * (12288 + 4) + w * h * 52
        print(f"{size}, {n} tiles: select {spread(sel)}, {b_sel / 1e6:.1f} MB, {b_sel / statistics.median(sel) / 1e9:.2f} TB/s; "
              f"resolve {spread(res)}, {b_res / 1e6:.1f} MB, {b_res / statistics.median(res) / 1e9:.2f} TB/s")


def form(a):
    for workload in a.workloads.split(","):
        scene, params = load(workload, a.spp)
        ws, _ = workspace(params.width, params.height)
        mom, lst = [], []
        for call in range(a.calls + 1):  # alternating; the first pair is the warm-up
            lib_st = rt.rt_stats()
            mean = np.zeros((params.height, params.width, 3))
            sq = np.zeros_like(mean)
            rt._check(rt.lib().rt_render_moments(scene.handle, C.byref(params.to_c()), C.c_void_p(mean.ctypes.data),
                                                 C.c_void_p(sq.ctypes.data), C.byref(lib_st)))
            t = timed(lambda: scene.adaptive_pass_async(params, ws.data_ptr(), ws.numel(), False, 0, 0), 1, warm=0)
            if call:
                mom.append(lib_st.kernel_ms)
                lst.append(t[0])
        print(f"{workload} at {a.spp} spp: rt_render_moments kernel {spread(mom)}; all-tiles pass {spread(lst)}; "
              f"ratio of medians {statistics.median(lst) / statistics.median(mom):.4f}")


def frame(a):
    scene, params = load(a.workload, a.max_spp)
    w, h = params.width, params.height
    ws, lay = workspace(w, h)
    big, rank = 2 ** 32 - 1, a.rank or 0  # rank 0 is the plain select, bit for bit

    def max_err():
        rt.adaptive_select_rank_async(w, h, ws.data_ptr(), ws.numel(), a.threshold, 0.0, a.pass_spp, big, rank)
        torch.cuda.synchronize()
        raw = ws[lay["info"]:lay["info"] + 16].cpu().numpy()
        return float(raw[8:].view(np.float64)[0]), int(raw[4:8].view(np.uint32)[0])

    for rep in range(a.calls):
        mean, sq, count, info = scene.render_adaptive(params, a.pass_spp, a.max_spp, a.threshold, rank=rank)
        fixed = timed(lambda: scene.adaptive_pass_async(params, ws.data_ptr(), ws.numel(), False, 0, 0), 1, warm=0)
        e_fixed = max_err()
        base, n_list = 0, 0
        while base < a.max_spp:  # the driver's loop once more, to measure its final state
            scene.adaptive_pass_async(params.replace(spp=a.pass_spp), ws.data_ptr(), ws.numel(), base != 0, n_list, base)
            rt.adaptive_select_rank_async(w, h, ws.data_ptr(), ws.numel(), a.threshold, 0.0, a.pass_spp, a.max_spp, rank)
            torch.cuda.synchronize()
            n_list, base = int(ws[lay["info"]:lay["info"] + 4].cpu().numpy().view(np.uint32)[0]), base + a.pass_spp
            if n_list == 0:
                break
        e_adaptive = max_err()
        hist = {int(k): int(v) for k, v in zip(*np.unique(count, return_counts=True))}
        print(f"{a.workload} {w}x{h}, passes of {a.pass_spp} to {a.max_spp}, threshold {a.threshold}, rank {rank}: adaptive "
              f"{info['paths']} samples ({info['paths'] / (w * h * a.max_spp):.3f} of the fixed frame's), kernel "
              f"{info['kernel_ms']:.2f} ms, largest tile error {e_adaptive[0]:.4f} ({e_adaptive[1]} flagged); fixed "
              f"{a.max_spp} spp pass {fixed[0]:.2f} ms, largest tile error {e_fixed[0]:.4f}; pixels by count {hist}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["pipeline", "form", "frame"])
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--workloads", default="C2,C3")
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--pass-spp", type=int, default=32)
    ap.add_argument("--max-spp", type=int, default=256)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rank", type=int, help="pipeline: also time the ranked select; frame: the tile error's rank (0..255)")
    a = ap.parse_args()
    dict(pipeline=pipeline, form=form, frame=frame)[a.mode](a)


if __name__ == "__main__":
    main()

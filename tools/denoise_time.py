"""Device-event times of rt_denoise_async on synthetic full-size frames.

    python tools/denoise_time.py [--sizes 1920x1080,3840x2160] [--calls 9]
    python tools/denoise_time.py --counts      rt_error_estimate_counts_async and rt_denoise_counts_async
                                               against the plain entries, alternating

Per size: the whole call at the default 5 iterations, and the call at 1..5 iterations, whose
differences are the times of the iterations with s = 2, 4, 8, 16 (the call at 1 iteration is
dn_prepare plus the s = 1 launch).  Each figure is the median of --calls calls after two
warm-up calls.  Bytes an iteration has to move: 64 B read (colour record and guide) and 32 B
written per pixel (the last one writes 24 + 8); dn_prepare reads 160 B and writes 72 B.

Per launch, from the device's own timestamps: run the tool under a kernel trace, in a run of its
own, then give the trace to --trace:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/denoise_time.py --only 5
    python tools/denoise_time.py --trace DIR

--only 5 makes every call a 5-iteration one, so the launches after each dn_prepare are s = 1, 2, 4,
8, 16 in order; --trace prints the median time of each over the traced calls, warm-up calls left out.
"""
import argparse
import csv
import importlib.util
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("rt_amd", os.path.join(REPO, "cpu-raytracing-rt_amd", "__init__.py"))
rt = importlib.util.module_from_spec(spec)
sys.modules["rt_amd"] = rt
spec.loader.exec_module(rt)


def frame(w, h):
    """A noisy two-plane frame with a miss band, made on the device."""
    g = torch.Generator(device="cuda").manual_seed(w)
    mean = torch.rand((h, w, 3), generator=g, dtype=torch.float64, device="cuda") + 0.1
    sq = mean * mean * (1.0 + torch.rand((h, w, 3), generator=g, dtype=torch.float64, device="cuda"))
    hits = np.zeros(h * w, rt.HIT_DTYPE)
    xs = np.tile(np.arange(w), h)
    hits["shading_normal"] = np.where((xs < w // 2)[:, None], [0.6, 0.0, 0.8], [0.0, 0.8, -0.6])
    hits["t"] = 5.0
    hits["prim"] = np.where(np.arange(h * w) >= w * (h - h // 4), -1, 7)
    rays = np.zeros((h * w, 6))
    rays[:, 3], rays[:, 4], rays[:, 5] = (xs - w / 2) * 1e-3, (np.arange(h * w) // w - h / 2) * 1e-3, 1.0
    return mean, sq, torch.from_numpy(rays).cuda(), torch.from_numpy(hits.view(np.float64)).cuda()


def trace_summary(root):
    """Median device time of each launch of a call, per frame size (dn_prepare's grid), from rocprofv3's
    kernel-trace CSVs under root: calls are the runs of launches that a dn_prepare starts."""
    rows = []
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith("kernel_trace.csv"):
                rows += [r for r in csv.DictReader(open(os.path.join(d, f))) if "rt::" in r["Kernel_Name"] and "dn_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls = {}
    for r in rows:
        if "dn_prepare" in r["Kernel_Name"]:
            call = calls.setdefault(int(r["Grid_Size_X"]), [])
            call.append([])
        call[-1].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for pixels, runs in sorted(calls.items()):
        runs = [c for c in runs[2:] if len(c) == len(runs[-1])]  # two warm-up calls
        names = ["dn_prepare"] + [f"dn_atrous s={1 << i}" for i in range(len(runs[-1]) - 1)]
        print(f"~{pixels} pixels, {len(runs)} calls: " +
              ", ".join(f"{n} {statistics.median(c[i] for c in runs):.1f} us" for i, n in enumerate(names)))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def counts_leg(a):
    """The counts entries against the plain ones, alternating call by call: the standard error (with
    its se output), and the denoiser at one iteration, whose difference is dn_prepare_counts against
    dn_prepare (the s = 1 launch is the same kernel on the same records)."""
    for size in a.sizes.split(","):
        w, h = map(int, size.split("x"))
        n = w * h
        mean, sq, rays, hits = frame(w, h)
        count = torch.full((h, w), 16, dtype=torch.int32, device="cuda")
        out, var = torch.empty((h, w, 3), dtype=torch.float64, device="cuda"), torch.empty((h, w), dtype=torch.float64, device="cuda")
        se, summary = torch.empty_like(mean), torch.empty(8, dtype=torch.float64, device="cuda")
        ws = torch.empty(rt.denoise_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        p = rt.rt_denoise_params(width=w, height=h, spp=16, iterations=1)
        tail = (rays.data_ptr(), hits.data_ptr(), out.data_ptr(), var.data_ptr(), ws.data_ptr(), ws.numel(), stream)
        legs = {
            "se plain": lambda: rt.error_estimate_async(mean.data_ptr(), sq.data_ptr(), n, 16, se.data_ptr(), summary.data_ptr(), stream),
            "se counts": lambda: rt.error_estimate_counts_async(mean.data_ptr(), sq.data_ptr(), count.data_ptr(), n, se.data_ptr(),
                                                                summary.data_ptr(), stream),
            "denoise(1) plain": lambda: rt.denoise_async(p, mean.data_ptr(), sq.data_ptr(), *tail),
            "denoise(1) counts": lambda: rt.denoise_counts_async(p, mean.data_ptr(), sq.data_ptr(), count.data_ptr(), *tail),
        }
        ms = {k: [] for k in legs}
        for call in range(a.calls + 2):  # plain, counts, plain, counts, ...; two warm-up rounds
            for k, fn in legs.items():
                t = timed(fn)
                if call >= 2:
                    ms[k].append(t)
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k, b in (("se plain", 72), ("se counts", 76)):
            print(f"{size} {k}: {med[k]:.3f} ms (min {min(ms[k]):.3f}, max {max(ms[k]):.3f}), {n * b / 1e6:.1f} MB, "
                  f"{n * b / med[k] / 1e9:.2f} TB/s")
        d = med["denoise(1) counts"] - med["denoise(1) plain"]
        print(f"{size} denoise at 1 iteration: plain {med['denoise(1) plain']:.3f} ms, counts {med['denoise(1) counts']:.3f} ms: "
              f"dn_prepare_counts - dn_prepare = {d * 1e3:+.1f} us for {n * 4 / 1e6:.1f} MB more on {n * 232 / 1e6:.1f} MB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--only", type=int, default=0, help="time calls of this many iterations only")
    ap.add_argument("--squarings", type=int, default=0, help="normal_squarings (0: the default, 7)")
    ap.add_argument("--trace", help="summarise a kernel trace directory and exit")
    ap.add_argument("--counts", action="store_true", help="the per-pixel-count entries against the plain ones")
    a = ap.parse_args()
    if a.trace:
        return trace_summary(a.trace)
    if a.counts:
        return counts_leg(a)
    for size in a.sizes.split(","):
        w, h = map(int, size.split("x"))
        mean, sq, rays, hits = frame(w, h)
        out = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
        var = torch.empty((h, w), dtype=torch.float64, device="cuda")
        ws = torch.empty(rt.denoise_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        ms = {}
        for it in ([a.only] if a.only else (5, 1, 2, 3, 4)):
            p = rt.rt_denoise_params(width=w, height=h, spp=16, iterations=it, normal_squarings=a.squarings)
            times = []
            for call in range(a.calls + 2):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rt.denoise_async(p, mean.data_ptr(), sq.data_ptr(), rays.data_ptr(), hits.data_ptr(), out.data_ptr(),
                                 var.data_ptr(), ws.data_ptr(), ws.numel(), stream)
                e1.record()
                e1.synchronize()
                if call >= 2:
                    times.append(e0.elapsed_time(e1))
            ms[it] = statistics.median(times)
        if a.only:
            print(f"{size}: whole call ({a.only} iterations, normal_squarings {a.squarings or 7}) {ms[a.only]:.3f} ms")
            continue
        n = w * h
        print(f"{size}: whole call (5 iterations) {ms[5]:.3f} ms; prepare + s=1 {ms[1]:.3f} ms "
              f"({n * (232 + 96) / ms[1] / 1e9:.2f} TB/s of the bytes they have to move)")
        for it in (2, 3, 4, 5):
            d = ms[it] - ms[it - 1]
            print(f"  + iteration s={1 << (it - 1)}: {d:.3f} ms ({n * 96 / d / 1e9:.2f} TB/s of 96 B a pixel)")
        assert torch.isfinite(out).all()


if __name__ == "__main__":
    main()

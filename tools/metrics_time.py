"""Device-event times of rt_image_metrics_async on synthetic full-size frames.

    python tools/metrics_time.py [--sizes 1920x1080,3840x2160] [--calls 9]
    python tools/metrics_time.py --frames C2 [--pass-spp 32] [--max-spp 256]

Per size and format (f64 radiance, u8 display bytes), the whole call (im_tile + im_fold) with and
without the two maps: the median of --calls calls after two warm-up calls, the bytes the call has
to move, and that over the time.  Bytes a pixel: both frames read once (2 x 24 B of f64, 2 x 3 B of
u8; the halo a block re-reads is not counted), and with the maps 8 B of rel written a pixel and 8 B
of ssim a window; the block partials are 64 B a 32x16 block.

--frames: the adaptive frames of a bench.py workload at thresholds 0.3 and 0.6, rank 0 and 12, against the
fixed frame of max_spp samples: relMSE, mean SSIM and PSNR of the radiance (indicative, one run each).
"""
import argparse
import importlib.util
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("rt_amd", os.path.join(REPO, "cpu-raytracing-rt_amd", "__init__.py"))
rt = importlib.util.module_from_spec(spec)
sys.modules["rt_amd"] = rt
spec.loader.exec_module(rt)


def frames(w, h, u8):
    """A noisy frame and a reference, made on the device."""
    g = torch.Generator(device="cuda").manual_seed(w)
    b = torch.rand((h, w, 3), generator=g, dtype=torch.float64, device="cuda") + 0.1
    a = b * (0.9 + 0.2 * torch.rand((h, w, 3), generator=g, dtype=torch.float64, device="cuda"))
    if u8:
        a, b = ((x * 200.0).round().clamp(0, 255).to(torch.uint8) for x in (a, b))
    return a.contiguous(), b.contiguous()


def worked_frames(args):
    sys.path.insert(0, REPO)
    import bench
    scene_file, w, h, _, _ = bench.WORKLOADS[args.frames]
    desc, params = bench.load_workload(rt, scene_file, w, h, args.max_spp)
    scene = rt.Scene(desc)
    fixed, _ = scene.render_moments(params)
    for threshold in (0.3, 0.6):
        for rank in (0, 12):
            mean, _, _, info = scene.render_adaptive(params, args.pass_spp, args.max_spp, threshold, rank=rank)
            m = rt.image_metrics(mean, fixed)
            print(f"{args.frames} {w}x{h}, passes of {args.pass_spp} to {args.max_spp}, threshold {threshold}, rank {rank}: "
                  f"{info['paths']} samples ({info['paths'] / (w * h * args.max_spp):.3f} of the fixed frame's); against the fixed "
                  f"{args.max_spp} spp frame relMSE {m['rel_mse']:.6f}, mean SSIM {m['ssim']:.6f}, PSNR {m['psnr']:.2f} dB, "
                  f"largest |d| {m['max_abs']:.4f}, {m['bad_pixels']} bad pixels, {m['bad_windows']} bad windows")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--frames", help="a bench.py workload: its adaptive frames against its fixed frame, and exit")
    ap.add_argument("--pass-spp", type=int, default=32)
    ap.add_argument("--max-spp", type=int, default=256)
    args = ap.parse_args()
    if args.frames:
        return worked_frames(args)
    stream = torch.cuda.current_stream().cuda_stream
    for size in args.sizes.split(","):
        w, h = map(int, size.split("x"))
        n, windows = w * h, (w - 10) * (h - 10)
        dev = dict(dtype=torch.float64, device="cuda")
        rel, ssim, summary = torch.empty((h, w), **dev), torch.empty((h - 10, w - 10), **dev), torch.empty(8, **dev)
        ws = torch.empty(rt.image_metrics_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
        for u8 in (False, True):
            a, b = frames(w, h, u8)
            p = rt.rt_metrics_params(width=w, height=h, format=rt.RT_METRICS_U8 if u8 else rt.RT_METRICS_F64)
            for maps in (True, False):
                times = []
                for call in range(args.calls + 2):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    rt.image_metrics_async(p, a.data_ptr(), b.data_ptr(), rel.data_ptr() if maps else 0,
                                           ssim.data_ptr() if maps else 0, summary.data_ptr(), ws.data_ptr(), ws.numel(), stream)
                    e1.record()
                    e1.synchronize()
                    if call >= 2:
                        times.append(e0.elapsed_time(e1))
                ms = statistics.median(times)
                moved = n * (6 if u8 else 48) + (n * 8 + windows * 8 if maps else 0) + ws.numel()
                s = summary.cpu()
                print(f"{size} {'u8 ' if u8 else 'f64'} {'maps   ' if maps else 'no maps'}: {ms:.3f} ms (min {min(times):.3f}, "
                      f"max {max(times):.3f}), {moved / 1e6:.1f} MB, {moved / ms / 1e9:.2f} TB/s, {n / ms / 1e6:.2f} Gpixel/s; "
                      f"relMSE {s[2].item() / (3 * (n - s[0].item())):.6f}, mean SSIM {s[5].item() / s[4].item():.6f}")
                assert s[0].item() == 0 and s[4].item() == windows and s[7].item() == 0


if __name__ == "__main__":
    main()

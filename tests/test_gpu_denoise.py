"""The à-trous denoiser (rt_denoise_async, rt_camera_rays_async, Scene.denoise) against a numpy
float64 restatement of the definition in include/rt_api.h, bit for bit: the filter uses only
+ - * / sqrt in a fixed order, which the device rounds as the host does."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LUM = (0.2126, 0.7152, 0.0722)
H5 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)


def same_bits(a, b):
    """Every number equal as bits, NaNs in the same places."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def restated(mean, sq, spp, rays, hits, iterations=5, squarings=7, sigma_l=4.0, sigma_z=0.01, eps=1e-8):
    """(out [H, W, 3], out_var [H, W]) of the definition, every pixel at once, taps in dy, dx order."""
    h, w, _ = mean.shape
    f32 = lambda a: a.astype(np.float32).astype(np.float64).reshape(h, w, -1)  # noqa: E731
    with np.errstate(all="ignore"):
        d = sq - mean * mean
        v = np.where(d < 0.0, 0.0, d) / (spp - 1.0)
        var = ((LUM[0] * LUM[0]) * v[..., 0] + (LUM[1] * LUM[1]) * v[..., 1]) + (LUM[2] * LUM[2]) * v[..., 2]
        ok = np.isfinite(mean).all(-1) & np.isfinite(var)
        hit = (hits["prim"] != -1).reshape(h, w)
        n, t = f32(hits["shading_normal"]), f32(hits["t"])[..., 0]
        x = f32(rays[:, :3] + hits["t"][:, None] * rays[:, 3:])
        col, (ys, xs) = mean, np.mgrid[0:h, 0:w]
        for i in range(iterations):
            lum = dot3(np.array(LUM), col)
            den = sigma_l * np.sqrt(var) + eps
            sw, sc, sv = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = ys + (dy << i), xs + (dx << i)
                    inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                    qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                    ok_q = ok[qy, qx] & inside
                    nn = dot3(n, n[qy, qx])
                    wn = np.where(nn < 0.0, 0.0, nn)
                    for _ in range(squarings):
                        wn = wn * wn
                    xz = np.abs(dot3(n, x[qy, qx] - x)) / (sigma_z * t)
                    wg = np.where(hit & hit[qy, qx], wn * (1.0 / (1.0 + xz * xz)), np.where(hit | hit[qy, qx], 0.0, 1.0))
                    xl = (lum[qy, qx] - lum) / den
                    wl = np.where(ok, 1.0 / (1.0 + xl * xl), 1.0)
                    wt = np.where(ok_q, (H5[dy + 2] * H5[dx + 2]) * (wg * wl), 0.0)
                    sw = sw + wt
                    sc = sc + wt[..., None] * np.where(ok_q[..., None], col[qy, qx], 0.0)
                    sv = sv + (wt * wt) * np.where(ok_q, var[qy, qx], 0.0)
            good = sw > 0.0
            col = np.where(good[..., None], sc / sw[..., None], col)
            var = np.where(good, sv / (sw * sw), var)
            ok = ok | good
    return col, var


def synthetic(rt, w, h, spp=16):
    """Two planes whose normals have a negative dot product (left | right), the bottom quarter a miss
    region, and where the frame has room a NaN in mean, an inf in sq and a pixel with var == 0."""
    rng = np.random.default_rng(1000 * w + h)
    ys, xs = np.mgrid[0:h, 0:w]
    left = xs < max(w // 2, 1)
    mean = np.where(left[..., None], [0.8, 0.3, 0.2], [0.2, 0.3, 0.9]) * rng.gamma(4.0, 0.25, (h, w, 3))
    sq = mean * mean * (1.0 + rng.random((h, w, 3)))
    if w >= 5 and h >= 3:
        mean[1, 1, 1] = np.nan
        sq[0, w - 2, 2] = np.inf
        sq[2, 0] = mean[2, 0] * mean[2, 0]
    hits = np.zeros(h * w, rt.HIT_DTYPE)
    nrm = np.where(left[..., None], [0.6, 0.0, 0.8], [0.0, 0.8, -0.6]) + rng.uniform(-0.03, 0.03, (h, w, 3))
    hits["shading_normal"] = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).reshape(-1, 3)
    hits["t"] = rng.uniform(4.0, 6.0, h * w)
    hits["prim"] = np.where(ys >= h - h // 4, -1, 7).ravel()
    rays = np.concatenate([np.tile([0.5, -1.0, 2.0], (h * w, 1)),
                           np.stack([(xs - w / 2) * 0.02, (ys - h / 2) * 0.02, np.ones((h, w))], -1).reshape(-1, 3)], 1)
    return mean, sq, spp, np.ascontiguousarray(rays), hits


def on_device(rt, mean, sq, spp, rays, hits, want_var=True, **kw):
    import torch
    h, w, _ = mean.shape
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.float64).reshape(-1)).cuda()  # noqa: E731
    d = [up(a) for a in (mean, sq, rays, hits)]
    out = torch.full((h, w, 3), -1.0, dtype=torch.float64, device="cuda")
    var = torch.full((h, w), -1.0, dtype=torch.float64, device="cuda")
    ws = torch.empty(rt.denoise_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
    rt.denoise_async(rt.rt_denoise_params(width=w, height=h, spp=spp, **kw), *[a.data_ptr() for a in d],
                     out.data_ptr(), var.data_ptr() if want_var else 0, ws.data_ptr(), ws.numel(),
                     torch.cuda.current_stream().cuda_stream)
    return out.cpu().numpy(), var.cpu().numpy()


# 1x1: smaller than the halo; 5x3: every tap out of bounds from s = 4 on; 37x29: partial tiles in both
# axes, lattices smaller than a tile from s = 4; 70x45: several blocks per lattice at s = 1
CASES = [(size, dict(iterations=i)) for size in [(1, 1), (5, 3), (37, 29), (70, 45)] for i in (1, 3, 5)]
CASES.append(((37, 29), dict(iterations=2, squarings=0, sigma_l=1.5, sigma_z=0.1, eps=1e-4)))  # no default left
CASES.append(((5, 3), dict(iterations=2, squarings=3)))  # the kernel's instance for a count that is not the default


@pytest.mark.parametrize("size,kw", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else
                         "-".join(f"{k}{x}" for k, x in v.items()))
def test_filter_matches_numpy(rt, size, kw):
    frame = synthetic(rt, *size)
    ref = restated(*frame, **kw)
    if "squarings" in kw:  # 0 squarings has a name of its own, 0 being "the default"
        kw = dict(kw, normal_squarings=kw["squarings"] or rt.RT_DENOISE_SQUARINGS_NONE)
        del kw["squarings"]
    assert not np.isnan(ref[0]).any() and not np.isnan(ref[1]).any()  # every missing pixel was filled
    got = on_device(rt, *frame, **kw)
    assert same_bits(got[0], ref[0]), np.argwhere(got[0] != ref[0])[:4]
    assert same_bits(got[1], ref[1]), np.argwhere(got[1] != ref[1])[:4]


def test_out_var_is_optional(rt):
    frame = synthetic(rt, 5, 3)
    with_var, without = on_device(rt, *frame), on_device(rt, *frame, want_var=False)
    assert same_bits(with_var[0], without[0]) and (without[1] == -1.0).all()


def test_no_leak_across_normal_edge(rt):
    """The right plane's colours scaled: the left plane's output keeps its bits, because the weight
    across normals with a negative dot product is exactly 0."""
    w, h = 37, 29
    mean, sq, spp, rays, hits = synthetic(rt, w, h)
    right_hits = np.s_[:h - h // 4, w // 2:]
    mean2, sq2 = mean.copy(), sq.copy()
    mean2[right_hits] *= 3.0
    sq2[right_hits] *= 9.0
    a, b = on_device(rt, mean, sq, spp, rays, hits), on_device(rt, mean2, sq2, spp, rays, hits)
    for k in range(2):
        assert same_bits(a[k][:h - h // 4, :w // 2], b[k][:h - h // 4, :w // 2])
        assert not same_bits(a[k][right_hits], b[k][right_hits])


def restated_rays(p):
    """camera_dir (render.hip, camera.rs:48-55) at the pixel centres; normalize = v * (1 / |v|)."""
    tan = math.tan(p.fov / 2.0)
    tan_x, tan_y = (tan, tan / (p.width / p.height)) if p.fov_axis == 0 else (tan / (p.height / p.width), tan)
    ys, xs = np.mgrid[0:p.height, 0:p.width]
    x = (2.0 * (xs + 0.5) / float(p.width) - 1.0) * tan_x
    y = -(2.0 * (ys + 0.5) / float(p.height) - 1.0) * tan_y
    r, u, f = (np.array(v) for v in (p.cam_right, p.cam_up, p.cam_forward))
    d = (r * x[..., None] + u * y[..., None]) + f * 1.0
    d = d * (1.0 / np.sqrt(dot3(d, d)))[..., None]
    return np.concatenate([np.broadcast_to(np.array(p.cam_position), d.shape), d], -1).reshape(-1, 6)


@pytest.mark.parametrize("axis", ["RT_FOV_X", "RT_FOV_Y"])
def test_camera_rays(rt, scene_text, axis):
    torch = pytest.importorskip("torch")
    p = rt.parse_scene(scene_text("cornell.txt"))[1].replace(width=7, height=5, fov_axis=getattr(rt, axis))
    d_rays = torch.full((35, 6), -1.0, dtype=torch.float64, device="cuda")
    rt.camera_rays_async(p, d_rays.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert same_bits(d_rays.cpu().numpy(), restated_rays(p))


@pytest.mark.parametrize("size", [(24, 20), (7, 5)], ids=lambda v: "x".join(map(str, v)))
def test_scene_denoise_end_to_end(rt, scene_text, size):
    """Cornell at 16 spp (7x5: an odd pixel count, where a pixel array's size is no multiple of 16 B): Scene.denoise (rays, first hits and filter on the device) equals the
    restatement on the same moments and Scene.intersect's hits of the restated rays."""
    desc, params = rt.parse_scene(scene_text("cornell.txt"))
    p, g = params.replace(width=size[0], height=size[1], spp=16), rt.Scene(desc)
    mean, sq = g.render_moments(p)
    rays = np.ascontiguousarray(restated_rays(p))
    ref = restated(mean, sq, p.spp, rays, g.intersect(rays))
    got = g.denoise(p, mean, sq)
    assert same_bits(got[0], ref[0]) and same_bits(got[1], ref[1])


@pytest.mark.parametrize("case", ["spp1", "short_workspace", "iterations9", "no_frame", "null_rays", "out_is_sq",
                                  "var_in_workspace", "mean_off_by_8"])
def test_argument_errors(rt, case):
    torch = pytest.importorskip("torch")
    w, h = 8, 4
    buf = torch.ones((8, w * h * 8), dtype=torch.float64, device="cuda")  # mean sq rays hits out var workspace(2 rows)
    ptr = [C.c_void_p(buf[i].data_ptr()) for i in range(7)]
    need, L = rt.denoise_workspace_bytes(w, h), rt.lib()
    assert need == 3 * 1024 and need <= 2 * buf[0].numel() * 8
    p = rt.rt_denoise_params(width=w, height=h, spp=1 if case == "spp1" else 4, iterations=9 if case == "iterations9" else 0)
    if case == "no_frame":
        rc = L.rt_denoise_workspace_bytes(0, h, C.byref(C.c_uint64()))
    elif case == "null_rays":
        rc = L.rt_camera_rays_async(C.byref(rt.RenderParams(w, h).to_c()), None, None)
    else:
        if case == "out_is_sq":
            ptr[4] = ptr[1]
        elif case == "var_in_workspace":
            ptr[5] = C.c_void_p(ptr[6].value + need - 16)
        elif case == "mean_off_by_8":
            ptr[0] = C.c_void_p(ptr[0].value + 8)
        rc = L.rt_denoise_async(C.byref(p), *ptr, need - 1 if case == "short_workspace" else need, None)
    torch.cuda.synchronize()
    assert rc == rt.RT_ERR_INVALID and (buf.cpu().numpy() == 1.0).all()

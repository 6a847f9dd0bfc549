"""Temporal accumulation (rt_temporal_accumulate_async, Scene.accumulate) against a numpy float64
restatement of the definition in include/rt_api.h, bit for bit, over chains of three frames: the
device's history goes back to the device and the restatement's to the restatement, so a wrong history
record shows in the next frame."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_HISTORY = 6  # uniform frames have 4 samples: 4, then 8 in history, so the cap binds in frame 2


def same_bits(a, b):
    """Every number equal as bits, NaNs in the same places."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def restated(mean, sq, n_c, rays, hits, prev, hist, max_history, normal_min=0.9, plane_tol=0.02):
    """(out_mean, out_sq, out_count, new history) of the definition, every pixel at once, taps in j, i order.
    hist: None, or the dict a call returned; prev: the RenderParams of the frame that made it."""
    h, w, _ = mean.shape
    f32 = lambda a: a.astype(np.float32).astype(np.float64).reshape(h, w, -1)  # noqa: E731
    with np.errstate(all="ignore"):
        cur = np.concatenate([mean, sq], -1)
        n_c = np.minimum(np.broadcast_to(n_c, (h, w)).astype(np.int64), 1 << 30)
        cur_ok = (n_c >= 1) & np.isfinite(cur).all(-1)
        hit = (hits["prim"] != -1).reshape(h, w)
        xp = (rays[:, :3] + hits["t"][:, None] * rays[:, 3:]).reshape(h, w, 3)
        n, t, x = f32(hits["shading_normal"]), f32(hits["t"])[..., 0], f32(xp)
        sw, sc, n_min = np.zeros((h, w)), np.zeros((h, w, 6)), np.full((h, w), 1 << 40)
        if hist is not None:
            tan = math.tan(prev.fov / 2.0)
            tan_x, tan_y = (tan, tan / (float(w) / float(h))) if prev.fov_axis == 0 else (tan / (float(h) / float(w)), tan)
            r, u, f = (np.array(v, np.float64) for v in (prev.cam_right, prev.cam_up, prev.cam_forward))
            det = dot3(r, cross(u, f))
            v = xp - np.array(prev.cam_position, np.float64)
            zc, xc, yc = dot3(v, cross(r, u) / det), dot3(v, cross(u, f) / det), dot3(v, cross(f, r) / det)
            gx = ((xc / zc) / tan_x + 1.0) * 0.5 * float(w) - 0.5
            gy = ((-(yc / zc)) / tan_y + 1.0) * 0.5 * float(h) - 0.5
            cand = hit & (zc > 0.0) & (gx >= -1.0) & (gx < w) & (gy >= -1.0) & (gy < h)
            gx, gy = np.where(cand, gx, 0.0), np.where(cand, gy, 0.0)
            fx, fy = np.floor(gx), np.floor(gy)
            ax, ay = gx - fx, gy - fy
            for j in (0, 1):
                for i in (0, 1):
                    qx, qy = fx.astype(np.int64) + i, fy.astype(np.int64) + j
                    inside = cand & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                    valid = (inside & (hist["count"][qy, qx] >= 1) & hist["hit"][qy, qx]
                             & (dot3(n, hist["n"][qy, qx]) >= normal_min)
                             & (np.abs(dot3(n, hist["x"][qy, qx] - x)) <= plane_tol * t))
                    b = (ax if i else 1.0 - ax) * (ay if j else 1.0 - ay)
                    sw = np.where(valid, sw + b, sw)
                    sc = np.where(valid[..., None], sc + b[..., None] * hist["col"][qy, qx], sc)
                    n_min = np.where(valid, np.minimum(n_min, hist["count"][qy, qx]), n_min)
        hist_ok = sw > 0.0
        hc, n_h = sc / sw[..., None], np.minimum(n_min, max_history)
        total = n_h + n_c
        both = (n_h.astype(np.float64)[..., None] * hc + n_c.astype(np.float64)[..., None] * cur) / total.astype(np.float64)[..., None]
        out = np.where((hist_ok & cur_ok)[..., None], both, np.where(hist_ok[..., None], hc, cur))
        oc = np.where(hist_ok & cur_ok, total, np.where(hist_ok, n_h, np.where(cur_ok, n_c, 0)))
    new = dict(n=n, x=x, hit=hit, col=out, count=np.where(np.isfinite(out).all(-1), oc, 0))
    return out[..., :3].copy(), out[..., 3:].copy(), oc.astype(np.uint32), new


def device_rays(rt, p):
    import torch
    d_rays = torch.empty((p.width * p.height, 6), dtype=torch.float64, device="cuda")
    rt.camera_rays_async(p, d_rays.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return d_rays.cpu().numpy()


def synthetic(rt, p, k, counts):
    """Frame k of camera p: a ridge at x = 0.3 pointing at the cameras, its two faces planes whose normals
    have a negative dot product, everything below y = -1 a miss; random moments with, where the frame has
    room, a NaN in one mean, an inf in one sq and (with counts) a pixel without samples, each moving with k."""
    w, h = p.width, p.height
    rng = np.random.default_rng(1000 * w + 10 * h + k)
    rays = device_rays(rt, p)
    o, d = rays[:, :3], rays[:, 3:]
    hits = np.zeros(h * w, rt.HIT_DTYPE)
    hits["prim"] = -1
    with np.errstate(all="ignore"):
        for side, nrm in ((1.0, (0.8, 0.0, -0.6)), (-1.0, (-0.8, 0.0, -0.6))):
            nrm = np.array(nrm)
            t = dot3(nrm, np.array([0.3, 0.0, 5.0]) - o) / dot3(nrm, d)
            at = o + t[:, None] * d
            on = (t > 0.0) & np.isfinite(t) & (side * (at[:, 0] - 0.3) >= 0.0) & (at[:, 1] >= -1.0)
            hits["t"][on], hits["shading_normal"][on], hits["prim"][on] = t[on], nrm, 7
    mean = rng.gamma(4.0, 0.25, (h, w, 3))
    sq = mean * mean * (1.0 + rng.random((h, w, 3)))
    count = rng.integers(1, 9, (h, w)).astype(np.uint32) if counts else 4
    if w >= 5 and h >= 3:
        mean[1, 1 + k, 1] = np.nan
        sq[0, w - 2 - k, 2] = np.inf
        if counts:
            count[2, k] = 0
    return mean, sq, count, rays, hits


def on_device(rt, p, frame, prev, d_hist, flags):
    import torch
    mean, sq, count, rays, hits = frame
    h, w, _ = mean.shape
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.float64).reshape(-1)).cuda()  # noqa: E731
    d = [up(a) for a in (mean, sq, rays, hits)]
    d_count = torch.from_numpy(count.view(np.int32)).cuda() if isinstance(count, np.ndarray) else None
    om, os_ = (torch.full((h, w, 3), -1.0, dtype=torch.float64, device="cuda") for _ in range(2))
    oc = torch.full((h, w), -1, dtype=torch.int32, device="cuda")
    nxt = torch.empty(rt.temporal_history_bytes(w, h), dtype=torch.uint8, device="cuda")
    rt.temporal_accumulate_async(
        rt.rt_temporal_params(width=w, height=h, spp=0 if d_count is not None else count, max_history=MAX_HISTORY, flags=flags),
        prev, d[0].data_ptr(), d[1].data_ptr(), 0 if d_count is None else d_count.data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
        0 if d_hist is None else d_hist.data_ptr(), nxt.data_ptr(), om.data_ptr(), os_.data_ptr(), oc.data_ptr(),
        torch.cuda.current_stream().cuda_stream)
    return om.cpu().numpy(), os_.cpu().numpy(), oc.cpu().numpy().view(np.uint32), nxt


def cameras(rt, motion, w, h):
    """The three cameras of a chain; the ridge is at z = 5, where a pixel of the 60-degree frame is 5.8 / w wide."""
    cam = lambda pos, **kw: rt.RenderParams(w, h, cam_position=pos, fov=math.pi / 3, **kw)  # noqa: E731
    if motion == "static":
        return [cam((0.0, 0.0, 0.0))] * 3
    if motion == "pan":  # about w / 115 and then w / 16 pixels
        return [cam((0.0, 0.0, 0.0)), cam((0.05, 0.0, 0.0)), cam((0.4, 0.05, 0.0))]
    if motion == "zoom":  # frame 1 sees the ridge from 4.3 times as far as frame 0: 16 pixels span 69 of frame 0's
        return [cam((0.3, 0.0, 3.85)), cam((0.3, 0.0, 0.0)), cam((0.3, 0.1, 1.0))]
    if motion == "behind":
        away = dict(cam_right=(-1.0, 0.0, 0.0), cam_forward=(0.0, 0.0, -1.0))
        return [cam((0.0, 0.0, 0.0), **away), cam((0.0, 0.0, 0.0)), cam((0.1, 0.0, 0.0), **away)]
    unit = lambda v: tuple(np.array(v) / np.linalg.norm(v))  # noqa: E731
    skew = dict(cam_right=unit((1.0, 0.0, 0.2)), cam_up=unit((0.1, 1.0, 0.0)))  # each normalised alone: not orthogonal
    return [cam((0.0, 0.0, 0.0), **skew), cam((0.1, 0.0, 0.0), **skew), cam((0.5, 0.05, 0.1), **skew)]


# 1x1: one ragged tile of one pixel; 5x3: odd rows that start on an odd double; 37x29: ragged tiles in both
# axes; 70x45: several tiles.  pan and zoom run with the window and without it.
MOTIONS = [("static", 0), ("pan", 0), ("pan", 1), ("zoom", 0), ("zoom", 1), ("behind", 0), ("skew", 0)]


@pytest.mark.parametrize("counts", [False, True], ids=["spp", "counts"])
@pytest.mark.parametrize("motion,flags", MOTIONS, ids=[m + "-gather" * f for m, f in MOTIONS])
@pytest.mark.parametrize("size", [(1, 1), (5, 3), (37, 29), (70, 45)], ids=lambda v: "x".join(map(str, v)))
def test_chain_matches_numpy(rt, size, motion, flags, counts):
    ref_hist = d_hist = prev = None
    for k, p in enumerate(cameras(rt, motion, *size)):
        frame = synthetic(rt, p, k, counts)
        ref = restated(*frame, prev, ref_hist, MAX_HISTORY)
        if k == 1:  # the case is not vacuous: enough hit pixels of frame 1 took history (none in behind)
            hit = (frame[4]["prim"] != -1).reshape(ref[2].shape)
            took = (ref[2] > np.broadcast_to(frame[2], hit.shape))[hit].mean()
            assert hit.any() and (took == 0.0 if motion == "behind" else took >= (0.1 if motion == "zoom" else 0.5)), took
            if motion == "static" and size[0] >= 5:
                assert np.isnan(frame[0][1, 2]).any() and np.isfinite(ref[0][1, 2]).all()  # the NaN pixel was filled
        got = on_device(rt, p, frame, prev, d_hist, flags)
        for a, b, what in zip(got, ref, ("mean", "sq", "count")):
            ok = same_bits(a, b) if what != "count" else np.array_equal(a, b)
            assert ok, (k, what, np.argwhere(~((a == b) | (a != a)))[:4])
        ref_hist, d_hist, prev = ref[3], got[3], p


def test_scene_accumulate_end_to_end(rt, scene_text):
    """Cornell at 48x32, two seeds from one camera: Scene.accumulate (rays, first hits and accumulation on
    the device) equals the restatement on the same moments, rays and hits, and feeds Scene.denoise."""
    desc, params = rt.parse_scene(scene_text("cornell.txt"))
    p, g = params.replace(width=48, height=32, spp=4), rt.Scene(desc)
    rays = device_rays(rt, p)
    hits = g.intersect(rays)
    ref_hist = hist = prev = None
    for seed in (1, 2):
        q = p.replace(seed=seed)
        mean, sq = g.render_moments(q)
        ref = restated(mean, sq, q.spp, rays, hits, prev, ref_hist, rt.RT_TEMPORAL_MAX_HISTORY)
        got = g.accumulate(q, mean, sq, history=hist, prev_params=prev)
        assert same_bits(got[0], ref[0]) and same_bits(got[1], ref[1]) and np.array_equal(got[2], ref[2])
        ref_hist, hist, prev = ref[3], got[3], q
    assert (got[2][(hits["prim"] != -1).reshape(32, 48)] == 8).mean() > 0.9  # both frames' samples
    out, var = g.denoise(p, got[0], got[1], count=got[2])
    assert out.shape == (32, 48, 3) and np.isfinite(out).all()

"""Adaptive frames downstream: the ranked tile error (rt_adaptive_select_rank_async), and the standard
error and the denoiser with every pixel's own sample count (rt_error_estimate_counts_async,
rt_denoise_counts_async), each against the float64 numpy restatement of its definition, bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

from test_gpu_adaptive import numpy_metric, read_info, resolve, workspace
from test_gpu_denoise import restated, same_bits, synthetic

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rank", [0, 1, 12, 64, 255])
@pytest.mark.parametrize("n_tiles", [1, 65, 1025])
def test_select_rank_matches_numpy(rt, n_tiles, rank):
    """One row of tiles, every one ragged (m = 176, the last 121).  test_select_matches_numpy's accumulators,
    and by tile index mod 5: 1 one pixel's accumulators over the whole tile, 2 over pixels 32..71 (runs of
    equal e around position r), 3 all zeros, 4 three positive pixels (fewer than r + 1 from rank 6 on)."""
    import torch
    a, cap, eps, w, h = 4, 16, 1e-3, 16 * n_tiles - 5, 11
    rng = np.random.default_rng(n_tiles)
    count = rng.choice([0, a, 2 * a, 3 * a, cap], n_tiles).astype(np.int32)
    mean = rng.random((n_tiles, 256, 3)) * 10.0 ** rng.integers(-3, 4, (n_tiles, 256, 3))
    sq = mean * mean * (1.0 + rng.random(mean.shape) * 10.0 ** rng.integers(-4, 1, (n_tiles, 256, 1)))
    i = np.arange(n_tiles * 256).reshape(n_tiles, 256)
    sq[i % 5 == 1] = np.nextafter((mean * mean)[i % 5 == 1], 0.0)
    mean[i % 1031 == 3, 1] = np.nan
    sq[i % 1733 == 5, 2] = np.inf
    mean[i % 2311 == 7, 0] = -np.inf
    sq[i % 3001 == 9, 0] = np.nan
    t = np.arange(n_tiles)
    for x in (mean, sq):
        x[t % 5 == 1] = x[t % 5 == 1, 40:41]
        x[t % 5 == 2, 32:72] = x[t % 5 == 2, 32:33]
        x[t % 5 == 3] = 0.0
        x[t % 5 == 4, 3:] = 0.0
    inside = ((i % 256 >> 4) < h) & (16 * (i // 256) + i % 16 < w)
    mean[~inside], sq[~inside] = 0.0, 0.0  # as the path kernel leaves them
    with np.errstate(invalid="ignore"):
        acc_sum, acc_sq = mean * count[:, None, None], sq * count[:, None, None]
    acc_sum[count == 0], acc_sq[count == 0] = 0.0, 0.0
    g, bad = numpy_metric(acc_sum.reshape(-1, 1, 3), acc_sq.reshape(-1, 1, 3), np.repeat(count, 256), eps)
    m = inside.sum(axis=1)
    assert (m[:-1] == 176).all() and m[-1] == 121
    err = np.sort(g.reshape(n_tiles, 256), axis=1)[:, ::-1][t, rank * m // 256]
    flag = bad.reshape(n_tiles, 256).any(axis=1)
    err[count < 2], flag[count < 2] = np.inf, False
    err[count >= cap], flag[count >= cap] = 0.25, True  # what the workspace held before
    fin = np.isfinite(err)
    threshold = float(np.median(err[fin])) if fin.any() else 1.0
    want = np.flatnonzero((err > threshold) & (count + a <= cap))
    results = []
    for ranked in (True, False):
        ws, v = workspace(rt, w, h)
        v["acc_sum"].copy_(torch.from_numpy(acc_sum.ravel()))
        v["acc_sq"].copy_(torch.from_numpy(acc_sq.ravel()))
        v["tile_count"].copy_(torch.from_numpy(count))
        v["tile_err"].fill_(0.25)
        v["tile_flag"].fill_(1)
        if ranked:
            rt.adaptive_select_rank_async(w, h, ws.data_ptr(), ws.numel(), threshold, eps, a, cap, rank)
            torch.cuda.synchronize()
            assert v["tile_err"].cpu().numpy().tobytes() == err.tobytes()
            assert np.array_equal(v["tile_flag"].cpu().numpy() != 0, flag)
            assert np.array_equal(v["tile_list"].cpu().numpy()[:len(want)], want)
            assert read_info(v) == (len(want), int(flag.sum()), err[fin].max() if fin.any() else 0.0)
        else:
            rt.adaptive_select_async(w, h, ws.data_ptr(), ws.numel(), threshold, eps, a, cap)
        results.append(ws.cpu().numpy().tobytes())
    assert rank != 0 or results[0] == results[1]  # rank 0 is the plain select's maximum, the whole workspace


def estimate(rt, mean, sq, count, spp=None, want_se=True, stream=0):
    """(se, summary) of the counts entry, or with spp of the plain one"""
    import torch
    n = len(mean)
    d_mean, d_sq, d_count = (torch.from_numpy(x).cuda() for x in (mean, sq, count.astype(np.int32)))
    d_se = torch.full((n, 3), -1.0, dtype=torch.float64, device="cuda")
    d_sum = torch.full((8,), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    if spp is None:
        rt.error_estimate_counts_async(d_mean.data_ptr(), d_sq.data_ptr(), d_count.data_ptr(), n,
                                       d_se.data_ptr() if want_se else 0, d_sum.data_ptr(), stream)
    else:
        rt.error_estimate_async(d_mean.data_ptr(), d_sq.data_ptr(), n, spp, d_se.data_ptr(), d_sum.data_ptr(), stream)
    torch.cuda.synchronize()
    return d_se.cpu().numpy(), d_sum.cpu().numpy()


@pytest.mark.parametrize("n", [1, 127, 128, 129, 4099, 256 * 1024 + 7])
def test_error_estimate_counts(rt, n):
    """test_error_estimate's frame with a count per pixel; 127..129: around one wave's trip of 128 pixels,
    whose counts are staged together.  Sums within n * 2^-52 relative of math.fsum, as there."""
    import torch
    rng = np.random.default_rng(n)
    mean = rng.random((n, 3)) * 10.0 ** rng.integers(-3, 4, (n, 3))
    sq = mean * mean * (1.0 + rng.random((n, 3)))
    i = np.arange(n)
    sq[i % 5 == 1] = np.nextafter((mean * mean)[i % 5 == 1], 0.0)
    mean[i % 17 == 3, 1] = np.nan
    sq[i % 29 == 5, 2] = np.inf
    mean[i % 31 == 7, 0] = np.inf
    sq[i % 37 == 9, 0] = np.nan
    count = rng.choice([0, 1, 2, 5, 64], n)
    with np.errstate(all="ignore"):
        d = sq - mean * mean
        se = np.sqrt(np.where(d < 0.0, 0.0, d) / (count[:, None] - 1.0))
        se = np.where(count[:, None] < 2, np.where(np.isnan(mean) | np.isnan(sq), np.nan, np.inf), se)
    good = (np.isfinite(se) & np.isfinite(mean)).all(axis=1)
    got, s = estimate(rt, mean, sq, count)
    assert same_bits(got, se)
    second = torch.cuda.Stream()
    other = estimate(rt, mean, sq, count, want_se=False, stream=second.cuda_stream)
    assert (other[0] == -1.0).all() and other[1].tobytes() == s.tobytes()
    assert s[0] == n - good.sum() and s[7] == (se[good].max() if good.any() else 0.0)
    for c in range(3):
        for x, want in ((s[1 + c], math.fsum(se[good, c])), (s[4 + c], math.fsum(mean[good, c]))):
            assert abs(x - want) <= n * 2.0 ** -52 * want
    uniform, plain = estimate(rt, mean, sq, np.full(n, 16)), estimate(rt, mean, sq, count, spp=16)
    assert same_bits(uniform[0], plain[0]) and uniform[1].tobytes() == plain[1].tobytes()


def denoised(rt, mean, sq, count, rays, hits, spp=0, **kw):
    """(out, out_var) of rt_denoise_counts_async, or with count None of rt_denoise_async at spp"""
    import torch
    h, w, _ = mean.shape
    d = [torch.from_numpy(np.ascontiguousarray(x).view(np.float64).reshape(-1)).cuda() for x in (mean, sq, rays, hits)]
    out = torch.full((h, w, 3), -1.0, dtype=torch.float64, device="cuda")
    var = torch.full((h, w), -1.0, dtype=torch.float64, device="cuda")
    ws = torch.empty(rt.denoise_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
    p, tail = rt.rt_denoise_params(width=w, height=h, spp=spp, **kw), [x.data_ptr() for x in d[2:] + [out, var, ws]]
    if count is None:
        rt.denoise_async(p, d[0].data_ptr(), d[1].data_ptr(), *tail, ws.numel())
    else:
        d_count = torch.from_numpy(count.astype(np.int32)).cuda()
        rt.denoise_counts_async(p, d[0].data_ptr(), d[1].data_ptr(), d_count.data_ptr(), *tail, ws.numel())
    return out.cpu().numpy(), var.cpu().numpy()


@pytest.mark.parametrize("iterations", [1, 5])
@pytest.mark.parametrize("size", [(5, 3), (37, 29)], ids=lambda v: "x".join(map(str, v)))
def test_denoise_counts_matches_numpy(rt, size, iterations):
    """synthetic's frame with counts in {1, 2, 7, 16}, and three pixels the resolve would make of count 0."""
    mean, sq, _, rays, hits = synthetic(rt, *size)
    w, h = size
    count = np.random.default_rng(w).choice([1, 2, 7, 16], (h, w))
    for y, x in ((0, 0), (h - 1, w - 1), (h // 2, w // 2)):
        count[y, x], mean[y, x], sq[y, x] = 0, np.nan, np.nan
    ref = restated(mean, sq, count[..., None].astype(np.float64), rays, hits, iterations=iterations)
    assert not np.isnan(ref[0]).any() and not np.isnan(ref[1]).any()  # every pixel with count < 2 was filled
    got = denoised(rt, mean, sq, count, rays, hits, iterations=iterations)
    assert same_bits(got[0], ref[0]), np.argwhere(got[0] != ref[0])[:4]
    assert same_bits(got[1], ref[1]), np.argwhere(got[1] != ref[1])[:4]
    uniform = denoised(rt, mean, sq, np.full((h, w), 16), rays, hits, iterations=iterations)
    plain = denoised(rt, mean, sq, None, rays, hits, spp=16, iterations=iterations)
    assert same_bits(uniform[0], plain[0]) and same_bits(uniform[1], plain[1])


def test_pipeline(rt, scene_text):
    """Cornell 48x32, passes of 8 to a cap of 32 at rank 12, the threshold the median tile_err after one
    pass: the driver against the loop through the async calls, then Scene.denoise with the counts against
    rt_denoise_counts_async by hand on the same buffers."""
    import torch
    desc, params = rt.parse_scene(scene_text("cornell.txt"))
    p, g, rank = params.replace(width=48, height=32, spp=8), rt.Scene(desc), 12
    g.set_tuning(chunk_spp=8, tail_split=8)
    ws, v = workspace(rt, p.width, p.height)

    def loop(threshold):
        n_list, base = 0, 0
        while base < 32:
            g.adaptive_pass_async(p, ws.data_ptr(), ws.numel(), base != 0, n_list, base)
            rt.adaptive_select_rank_async(p.width, p.height, ws.data_ptr(), ws.numel(), threshold, 0.0, 8, 32, rank)
            torch.cuda.synchronize()
            n_list, base = read_info(v)[0], base + 8
            if n_list == 0:
                break
        return resolve(rt, p, ws)

    loop(np.inf)
    threshold = float(np.median(v["tile_err"].cpu().numpy()))
    want = loop(threshold)
    mean, sq, count, _ = g.render_adaptive(p, 8, 32, threshold, rank=rank)
    for x, y in zip((mean, sq, count), want):
        assert same_bits(x.astype(np.float64), y.astype(np.float64))
    assert count.min() == 8 and 8 < count.max() <= 32
    out, var = g.denoise(p, mean, sq, count=count)
    assert np.isfinite(out).all() and np.isfinite(var).all()
    d_rays = torch.empty((48 * 32, 6), dtype=torch.float64, device="cuda")
    rt.camera_rays_async(p, d_rays.data_ptr())
    rays = d_rays.cpu().numpy()
    by_hand = denoised(rt, mean, sq, count, rays, g.intersect(rays))
    assert same_bits(out, by_hand[0]) and same_bits(var, by_hand[1])


@pytest.mark.parametrize("case", ["rank256", "estimate_null_count", "denoise_null_count", "count_is_out"])
def test_argument_errors(rt, case):
    import torch
    w, h, L = 8, 4, rt.lib()
    ws, _ = workspace(rt, w, h, fill=0x5A)
    buf = torch.ones((9, w * h * 8), dtype=torch.float64, device="cuda")  # mean sq count rays hits out var workspace(2 rows)
    ptr = [C.c_void_p(buf[k].data_ptr()) for k in range(7)]
    if case == "rank256":
        rc = L.rt_adaptive_select_rank_async(w, h, C.c_void_p(ws.data_ptr()), ws.numel(), 0.5, 0.0, 4, 16, 256, None)
    elif case == "estimate_null_count":
        rc = L.rt_error_estimate_counts_async(ptr[0], ptr[1], None, w * h, ptr[5], ptr[6], None)
    else:
        ptr[2] = None if case == "denoise_null_count" else ptr[5]
        rc = L.rt_denoise_counts_async(C.byref(rt.rt_denoise_params(width=w, height=h)), *ptr,
                                       C.c_void_p(buf[7].data_ptr()), rt.denoise_workspace_bytes(w, h), None)
    torch.cuda.synchronize()
    assert rc == rt.RT_ERR_INVALID
    assert (ws.cpu().numpy() == 0x5A).all() and (buf.cpu().numpy() == 1.0).all()

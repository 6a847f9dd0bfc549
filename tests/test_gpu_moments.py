"""Per-pixel second moments (rt_render_moments, rt_render_tiles_moments_async) against the
oracle's oracle_render_moments, and the standard-error map and frame summary
(rt_error_estimate_async) against the numpy float64 formula."""
import ctypes as C
import math

import numpy as np
import pytest

from fuzz_scenes import random_scene

pytestmark = pytest.mark.gpu

TRI = dict(resume=1, waves=4)  # the 4-wave resumable kernel, whose triangle layouts rt_tuning.compact picks
FORMS = {"cornell": {}, "tri_f64": dict(TRI, compact=0), "tri_c64": dict(TRI, compact=1), "tri_pair": dict(TRI, compact=2)}
# 24x20x5: partial 16x16 tiles and 8x8 quadrants, fewer rows than the 64-row ring; x70: the ring
# wraps, several open wave-tiles; 16x16x1: a single row
FRAMES = [(24, 20, 5), (24, 20, 70), (16, 16, 1)]


@pytest.fixture(scope="module")
def scenes(rt, orc, scene_text):
    """name -> (params, device scene, oracle scene, cache of oracle frames)"""
    out = {}
    for name, text in (("cornell", scene_text("cornell.txt")), ("sink", scene_text("kitchen_sink.txt")),
                       ("tri", random_scene(5000, tri_only=True))):
        desc, params = rt.parse_scene(text)
        out[name] = (params, rt.Scene(desc), orc.OracleScene(desc), {})
    assert out["tri"][1].info()["layout_flags"] & 0x5 == 0x5  # the compact layout and its pair lines
    return out


def oracle_frame(entry, p):
    """oracle_render_moments, iterative form, once per frame: (mean, sq) in single-run sample order"""
    key = (p.width, p.height, p.spp, p.ray_depth)
    if key not in entry[3]:
        entry[3][key] = entry[2].render_moments(p, mode=1)[:2]
    return entry[3][key]


def same_bits(a, b):
    """Every number equal as bits, NaNs in the same places (a NaN's payload is the host's or the device's own)."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


def check_single_run(entry, p, **tuning):
    g = entry[1]
    g.set_tuning(chunk_spp=p.spp, **tuning)  # one run per pixel: the oracle's order
    assert g.sample_chunks(p) == (1, p.spp)
    mean, sq = g.render_moments(p)
    o_mean, o_sq = oracle_frame(entry, p)
    assert same_bits(sq, o_sq), f"max |d| {np.nanmax(np.abs(sq - o_sq))}"
    assert same_bits(mean, g.generate_image(p)[0]) and same_bits(mean, o_mean)
    return mean, sq


@pytest.mark.parametrize("tail_split", [1, 8])
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "x".join(map(str, f)))
@pytest.mark.parametrize("form", FORMS)
def test_second_moment_matches_oracle(scenes, form, frame, tail_split):
    entry = scenes["cornell" if form == "cornell" else "tri"]
    w, h, spp = frame
    check_single_run(entry, entry[0].replace(width=w, height=h, spp=spp), tail_split=tail_split, **FORMS[form])
    assert form == "cornell" or entry[1].tuning()["compact"] == FORMS[form]["compact"]


@pytest.mark.parametrize("tail_split", [1, 8])
def test_nan_sample_is_nan_in_both(scenes, tail_split):
    """test_last_bounce_nan's frame: pixel 33, sample 213 of the kitchen sink has a NaN radiance."""
    entry = scenes["sink"]
    mean, sq = check_single_run(entry, entry[0].replace(width=32, height=24, spp=214, ray_depth=3), tail_split=tail_split)
    for a in (mean, sq):
        assert np.isnan(a[1, 1]).all() and np.isnan(a).sum() == 3


@pytest.mark.parametrize("form", ["cornell", "tri_pair"])
def test_forced_chunks(scenes, form):
    """chunk_spp 3 at spp 8: three runs, the last one short, through the chunk partials, and with
    tail_split 8 through the row buffer too.  The device adds run sums, the oracle one run: two
    orders of one sum of non-negative terms, each within (spp - 1) * 2^-53 relative of the exact
    sum, so within spp * 2^-52 of each other."""
    entry = scenes["cornell" if form == "cornell" else "tri"]
    p, g = entry[0].replace(width=24, height=20, spp=8), entry[1]
    g.set_tuning(chunk_spp=3, tail_split=8, **FORMS[form])
    assert g.sample_chunks(p) == (3, 3)
    mean, sq = g.render_moments(p)
    assert same_bits(mean, g.generate_image(p)[0])
    o_sq = oracle_frame(entry, p)[1]
    fin = np.isfinite(o_sq)
    assert np.array_equal(fin, np.isfinite(sq)) and same_bits(sq[~fin], o_sq[~fin])
    print("max rel", (np.abs(sq[fin] - o_sq[fin]) / np.maximum(o_sq[fin], 1e-300)).max())
    assert (np.abs(sq[fin] - o_sq[fin]) <= p.spp * 2.0 ** -52 * o_sq[fin]).all()


def test_tiles_match_single(scenes, rt):
    """World 3, rank-major, each buffer through rt_unpack_tiles_async: rt_render_moments' outputs."""
    torch = pytest.importorskip("torch")
    params, g = scenes["cornell"][:2]
    p, world = params.replace(width=24, height=20, spp=5), 3
    g.set_tuning()
    ref = g.render_moments(p)
    per = g.tiles_per_rank(p, world)
    packed = torch.zeros((2, world, per, 256, 3), dtype=torch.float64, device="cuda")
    for r in range(world):
        g.render_tiles_moments_async(p, r, world, packed[0, r].data_ptr(), packed[1, r].data_ptr())
    img = torch.zeros((2, p.height, p.width, 3), dtype=torch.float64, device="cuda")
    for k in range(2):
        rt.unpack_tiles_async(p, world, packed[k].data_ptr(), img[k].data_ptr())
    torch.cuda.synchronize()
    assert same_bits(img[0].cpu().numpy(), ref[0]) and same_bits(img[1].cpu().numpy(), ref[1])


@pytest.mark.parametrize("n,spp", [(1, 16), (63, 16), (64, 16), (65, 16), (4099, 16), (4099, 1), (256 * 1024 + 7, 16)])
def test_error_estimate(rt, n, spp):
    """se against numpy's sqrt(max(sq - mean * mean, 0) / (spp - 1)): the kernel uses the compiler's
    IEEE sqrt and /, the correctly rounded forms test_fp64_rounding_matches_host pins, and no fused
    multiply-add, so every number is equal as bits.  The summary's count and max are exact; its sums
    are fixed-order sums of non-negative terms, within n * 2^-52 relative of math.fsum.  Sizes: the
    lane map's tails (n odd and even, below and above one wave's 64 words), one block, many blocks."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(n + spp)
    mean = rng.random((n, 3)) * 10.0 ** rng.integers(-3, 4, (n, 3))
    sq = mean * mean * (1.0 + rng.random((n, 3)))
    i = np.arange(n)
    sq[i % 5 == 1] = np.nextafter((mean * mean)[i % 5 == 1], 0.0)  # below mean^2 by rounding: clamps to 0
    mean[i % 17 == 3, 1] = np.nan
    sq[i % 29 == 5, 2] = np.inf
    mean[i % 31 == 7, 0] = np.inf
    sq[i % 37 == 9, 0] = np.nan
    with np.errstate(all="ignore"):
        d = sq - mean * mean
        se = np.sqrt(np.where(d < 0.0, 0.0, d) / (spp - 1.0))
        if spp == 1:
            se = np.where(np.isnan(mean) | np.isnan(sq), np.nan, np.inf)
    good = (np.isfinite(se) & np.isfinite(mean)).all(axis=1)
    d_mean, d_sq = torch.from_numpy(mean).cuda(), torch.from_numpy(sq).cuda()
    d_se = torch.full((n, 3), -1.0, dtype=torch.float64, device="cuda")
    d_sum = torch.full((2, 8), -1.0, dtype=torch.float64, device="cuda")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    rt.error_estimate_async(d_mean.data_ptr(), d_sq.data_ptr(), n, spp, d_se.data_ptr(), d_sum[0].data_ptr(),
                            streams[0].cuda_stream)
    rt.error_estimate_async(d_mean.data_ptr(), d_sq.data_ptr(), n, spp, 0, d_sum[1].data_ptr(), streams[1].cuda_stream)
    torch.cuda.synchronize()
    assert same_bits(d_se.cpu().numpy(), se)
    s = d_sum.cpu().numpy()
    assert s[0].tobytes() == s[1].tobytes()  # another stream, no se output: the same bits
    assert s[0, 0] == n - good.sum() and s[0, 7] == (se[good].max() if good.any() else 0.0)
    for c in range(3):
        for got, want in ((s[0, 1 + c], math.fsum(se[good, c])), (s[0, 4 + c], math.fsum(mean[good, c]))):
            assert abs(got - want) <= n * 2.0 ** -52 * want


@pytest.mark.parametrize("case", ["null_sq", "null_mean", "hit_ids", "stats", "tiles_null_sq", "tiles_stats",
                                  "estimate_spp0", "estimate_empty"])
def test_argument_errors(scenes, rt, case):
    torch = pytest.importorskip("torch")
    params, g = scenes["cornell"][:2]
    buf = np.zeros((16, 16, 3))
    ptr = buf.ctypes.data_as(C.c_void_p)
    dev = torch.ones(8, dtype=torch.float64, device="cuda")
    d, L = C.c_void_p(dev.data_ptr()), rt.lib()
    flag = dict(hit_ids=rt.RT_FLAG_HIT_IDS, stats=rt.RT_FLAG_STATS, tiles_stats=rt.RT_FLAG_STATS).get(case, 0)
    pc = C.byref(params.replace(width=16, height=16, spp=1, flags=flag).to_c())
    if case.startswith("tiles"):
        rc = L.rt_render_tiles_moments_async(g.handle, pc, 0, 1, d, None if case == "tiles_null_sq" else d, None)
    elif case.startswith("estimate"):
        rc = L.rt_error_estimate_async(d, d, 0, 0 if case == "estimate_spp0" else 4, None, d, None)
    else:
        rc = L.rt_render_moments(g.handle, pc, None if case == "null_mean" else ptr, None if case == "null_sq" else ptr, None)
    torch.cuda.synchronize()
    if case == "estimate_empty":  # no pixels: RT_OK and the summary zeroed
        assert rc == rt.RT_OK and (dev.cpu().numpy() == 0.0).all()
    else:
        assert rc == rt.RT_ERR_INVALID and (dev.cpu().numpy() == 1.0).all()

"""Adaptive sampling (rt_adaptive_*_async, rt_render_adaptive): passes over tile lists at sample bases
against the oracle's chunked frames, the tile error and the compacted list against a float64 numpy
restatement, the host driver against the same loop driven from here."""
import ctypes as C

import numpy as np
import pytest

from fuzz_scenes import random_scene
from test_gpu_moments import FORMS, same_bits

pytestmark = pytest.mark.gpu
LR, LG, LB = 0.2126, 0.7152, 0.0722


@pytest.fixture(scope="module")
def scenes(rt, orc, scene_text):
    """name -> (params, device scene, oracle scene, cache of oracle frames)"""
    out = {}
    for name, text in (("cornell", scene_text("cornell.txt")), ("tri", random_scene(5000, tri_only=True))):
        desc, params = rt.parse_scene(text)
        out[name] = (params, rt.Scene(desc), orc.OracleScene(desc), {})
    return out


def oracle_frame(entry, p, chunk_spp):
    """(mean in runs of chunk_spp, second moment in single-run order), once per frame"""
    key = (p.width, p.height, p.spp, chunk_spp)
    if key not in entry[3]:
        entry[3][key] = (entry[2].render(p, mode=1, chunk_spp=chunk_spp)[0], entry[2].render_moments(p, mode=1)[1])
    return entry[3][key]


def workspace(rt, w, h, fill=0):
    """(device bytes, typed views of its sub-buffers); u32 buffers are viewed as i32"""
    import torch
    nbytes, lay = rt.adaptive_workspace(w, h)
    ws = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
    n = lay["n_tiles"]
    shape = dict(acc_sum=(torch.float64, n * 768), acc_sq=(torch.float64, n * 768), tile_count=(torch.int32, n),
                 tile_err=(torch.float64, n), tile_flag=(torch.int32, n), tile_list=(torch.int32, n),
                 info=(torch.uint8, 16))
    assert all(lay[k] % 256 == 0 for k in shape)
    return ws, {k: ws[lay[k]:lay[k] + cnt * dt.itemsize].view(dt) for k, (dt, cnt) in shape.items()}


def resolve(rt, p, ws):
    import torch
    mean = torch.zeros((p.height, p.width, 3), dtype=torch.float64, device="cuda")
    sq, count = torch.zeros_like(mean), torch.zeros((p.height, p.width), dtype=torch.int32, device="cuda")
    rt.adaptive_resolve_async(p, ws.data_ptr(), ws.numel(), mean.data_ptr(), sq.data_ptr(), count.data_ptr())
    torch.cuda.synchronize()
    return mean.cpu().numpy(), sq.cpu().numpy(), count.cpu().numpy()


def read_info(v):
    raw = v["info"].cpu().numpy()
    return int(raw[:4].view(np.uint32)[0]), int(raw[4:8].view(np.uint32)[0]), float(raw[8:].view(np.float64)[0])


def tile_slice(t, tiles_x):
    return slice(t // tiles_x * 16, t // tiles_x * 16 + 16), slice(t % tiles_x * 16, t % tiles_x * 16 + 16)


@pytest.mark.parametrize("a,c", [(5, 5), (6, 3)])
@pytest.mark.parametrize("form", FORMS)
def test_passes_match_oracle(scenes, rt, form, a, c):
    """40x24: 3x2 tiles, ragged both ways.  Three passes of `a` samples in runs of c (6, 3: two runs a
    pass, which pins the flat run order): all tiles at base 0, [4, 1, 3] at a, [3] at 2a.  A tile with j
    passes holds the oracle's frame of j * a spp in runs of c: the mean bit for bit; sq is the oracle's
    single-run sum re-associated, non-negative terms, within j * a * 2^-52 (test_forced_chunks' bound)."""
    import torch
    entry = scenes["cornell" if form == "cornell" else "tri"]
    p, g = entry[0].replace(width=40, height=24, spp=a), entry[1]
    g.set_tuning(chunk_spp=c, tail_split=8, **FORMS[form])
    assert g.sample_chunks(p) == (a // c, c)
    ws, v = workspace(rt, p.width, p.height)
    for tiles, base in ((None, 0), ([4, 1, 3], a), ([3], 2 * a)):
        if tiles:
            v["tile_list"][:len(tiles)] = torch.tensor(tiles, dtype=torch.int32, device="cuda")
        g.adaptive_pass_async(p, ws.data_ptr(), ws.numel(), tiles is not None, len(tiles or ()), base)
    mean, sq, count = resolve(rt, p, ws)
    for t, j in enumerate([1, 2, 1, 3, 2, 1]):
        sl = tile_slice(t, 3)
        o_mean, o_sq = (x[sl] for x in oracle_frame(entry, p.replace(spp=j * a), c))
        assert (count[sl] == j * a).all()
        assert same_bits(mean[sl], o_mean), (t, np.nanmax(np.abs(mean[sl] - o_mean)))
        fin = np.isfinite(o_sq)
        assert np.array_equal(fin, np.isfinite(sq[sl])) and same_bits(sq[sl][~fin], o_sq[~fin])
        print(t, "max rel", (np.abs(sq[sl][fin] - o_sq[fin]) / np.maximum(o_sq[fin], 1e-300)).max())
        assert (np.abs(sq[sl][fin] - o_sq[fin]) <= j * a * 2.0 ** -52 * o_sq[fin]).all()


def numpy_metric(acc_sum, acc_sq, count, eps):
    """The header's definition on [n][256][3] accumulators: (tile error, flagged)."""
    with np.errstate(all="ignore"):
        n = count.astype(np.float64)[:, None, None]
        mean, m2 = acc_sum / n, acc_sq / n
        d = m2 - mean * mean
        v = np.where(d < 0.0, 0.0, d) / (n - 1.0)
        var = ((LR * LR) * v[..., 0] + (LG * LG) * v[..., 1]) + (LB * LB) * v[..., 2]
        lum = (LR * mean[..., 0] + LG * mean[..., 1]) + LB * mean[..., 2]
        e = np.sqrt(var) / (lum + eps)
        bad = ~np.isfinite(e)
        return np.where(bad | ~(e > 0.0), 0.0, e).max(axis=1), bad.any(axis=1)


@pytest.mark.parametrize("n_tiles", [1, 63, 64, 65, 1025, 4099])  # 1025: one more than as_compact's trip
def test_select_matches_numpy(rt, n_tiles):
    """tile_err and the flags bit for bit (IEEE / and sqrt, nothing fused), the list, info; tiles at the
    cap keep the error and flag they had; a second workspace on another stream gets the same bytes."""
    import torch
    a, cap, eps = 4, 16, 1e-3
    rng = np.random.default_rng(n_tiles)
    count = rng.choice([0, a, 2 * a, 3 * a, cap], n_tiles).astype(np.int32)
    mean = rng.random((n_tiles, 256, 3)) * 10.0 ** rng.integers(-3, 4, (n_tiles, 256, 3))
    sq = mean * mean * (1.0 + rng.random(mean.shape) * 10.0 ** rng.integers(-4, 1, (n_tiles, 256, 1)))
    i = np.arange(n_tiles * 256).reshape(n_tiles, 256)
    sq[i % 5 == 1] = np.nextafter((mean * mean)[i % 5 == 1], 0.0)  # a hair below mean^2
    mean[i % 1031 == 3, 1] = np.nan
    sq[i % 1733 == 5, 2] = np.inf
    mean[i % 2311 == 7, 0] = -np.inf
    sq[i % 3001 == 9, 0] = np.nan
    mean[i % 16 >= 11], sq[i % 16 >= 11] = 0.0, 0.0  # "outside the image"
    with np.errstate(invalid="ignore"):
        acc_sum, acc_sq = mean * count[:, None, None], sq * count[:, None, None]
    acc_sum[count == 0], acc_sq[count == 0] = 0.0, 0.0
    err, flag = numpy_metric(acc_sum, acc_sq, count, eps)
    err[count < 2], flag[count < 2] = np.inf, False
    err[count >= cap], flag[count >= cap] = 0.25, True  # what the workspace held before
    fin = np.isfinite(err)
    threshold = float(np.median(err[fin])) if fin.any() else 1.0
    want = np.flatnonzero((err > threshold) & (count + a <= cap))
    results = []
    for stream in (torch.cuda.Stream(), torch.cuda.Stream()):
        ws, v = workspace(rt, 16 * n_tiles, 16)
        v["acc_sum"].copy_(torch.from_numpy(acc_sum.ravel()))
        v["acc_sq"].copy_(torch.from_numpy(acc_sq.ravel()))
        v["tile_count"].copy_(torch.from_numpy(count))
        v["tile_err"].fill_(0.25)
        v["tile_flag"].fill_(1)
        torch.cuda.synchronize()
        rt.adaptive_select_async(16 * n_tiles, 16, ws.data_ptr(), ws.numel(), threshold, eps, a, cap, stream.cuda_stream)
        torch.cuda.synchronize()
        results.append(ws.cpu().numpy().tobytes())
    assert v["tile_err"].cpu().numpy().tobytes() == err.tobytes()
    assert np.array_equal(v["tile_flag"].cpu().numpy() != 0, flag)
    assert np.array_equal(v["tile_list"].cpu().numpy()[:len(want)], want)
    assert read_info(v) == (len(want), int(flag.sum()), err[fin].max() if fin.any() else 0.0)
    assert results[0] == results[1]


def test_driver(scenes, rt):
    """Cornell 48x32 (3x2 tiles), passes of 8 to a cap of 32 in runs of 8.  threshold inf: one pass;
    0: every tile to the cap; both the oracle's frames bit for bit.  Between: the median of tile_err after
    one pass (6 tiles: 3 stop at once, 3 go on), the driver against the same loop through the async calls."""
    import torch
    entry = scenes["cornell"]
    p, g = entry[0].replace(width=48, height=32, spp=8), entry[1]
    g.set_tuning(chunk_spp=8, tail_split=8)
    for threshold, spp in ((np.inf, 8), (0.0, 32)):
        mean, sq, count, info = g.render_adaptive(p, 8, 32, threshold)
        assert (count == spp).all() and info["paths"] == spp * 48 * 32
        assert same_bits(mean, oracle_frame(entry, p.replace(spp=spp), 8)[0])
    ws, v = workspace(rt, p.width, p.height)
    big = 2 ** 32 - 1

    def loop(threshold):
        n_list, base = 0, 0
        while base < 32:
            g.adaptive_pass_async(p, ws.data_ptr(), ws.numel(), base != 0, n_list, base)
            rt.adaptive_select_async(p.width, p.height, ws.data_ptr(), ws.numel(), threshold, 0.0, 8, 32)
            torch.cuda.synchronize()
            n_list, base = read_info(v)[0], base + 8
            if n_list == 0:
                break
        return resolve(rt, p, ws)

    loop(np.inf)
    threshold = float(np.median(v["tile_err"].cpu().numpy()))
    want = loop(threshold)
    got = g.render_adaptive(p, 8, 32, threshold)
    for x, y in zip(got[:3], want):
        assert same_bits(x.astype(np.float64), y.astype(np.float64))
    count = want[2]
    assert (count % 8 == 0).all() and count.min() == 8 and 8 < count.max() <= 32
    rt.adaptive_select_async(p.width, p.height, ws.data_ptr(), ws.numel(), threshold, 0.0, 8, big)  # measures every tile
    torch.cuda.synchronize()
    tile_count, tile_err = v["tile_count"].cpu().numpy(), v["tile_err"].cpu().numpy()
    print("threshold", threshold, "counts", tile_count, "errors", tile_err)
    assert (tile_err[tile_count < 32] <= threshold).all()


@pytest.mark.parametrize("case", ["hit_ids", "stats", "spp1", "n_list", "base", "short", "misaligned", "threshold_neg",
                                  "threshold_nan", "eps_neg", "empty_list"])
def test_argument_errors(scenes, rt, case):
    import torch
    params, g = scenes["cornell"][:2]
    ws, v = workspace(rt, 40, 24, fill=0x5A)
    flag = dict(hit_ids=rt.RT_FLAG_HIT_IDS, stats=rt.RT_FLAG_STATS).get(case, 0)
    pc = C.byref(params.replace(width=40, height=24, spp=1 if case == "spp1" else 4, flags=flag).to_c())
    ptr = C.c_void_p(ws.data_ptr() + (16 if case == "misaligned" else 0))
    nbytes, L = ws.numel() - (1 if case == "short" else 0), rt.lib()
    if case in ("threshold_neg", "threshold_nan", "eps_neg"):
        threshold, eps = dict(threshold_neg=(-1.0, 0.0), threshold_nan=(np.nan, 0.0), eps_neg=(1.0, -1e-3))[case]
        rc = L.rt_adaptive_select_async(40, 24, ptr, nbytes, threshold, eps, 4, 16, None)
    else:
        rc = L.rt_adaptive_pass_async(g.handle, pc, ptr, nbytes, 1, dict(n_list=7, empty_list=0).get(case, 2),
                                      2 ** 32 - 3 if case == "base" else 0, None)
    torch.cuda.synchronize()
    assert rc == (rt.RT_OK if case == "empty_list" else rt.RT_ERR_INVALID)
    assert (ws.cpu().numpy() == 0x5A).all()

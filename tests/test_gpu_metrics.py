"""Image metrics (rt_image_metrics_async, image_metrics) against a numpy float64 restatement of the
definition in include/rt_api.h: the maps bit for bit (only + - * / in a fixed order, which the device
rounds as the host does), the counts, max and min exactly, the three sums within the bound that holds
for any summation order of n terms, n * 2^-53 * sum |term|, against math.fsum."""
import ctypes as C
import math

import numpy as np
import pytest

gpu = pytest.mark.gpu
LUM = (0.2126, 0.7152, 0.0722)


def same_bits(a, b):
    """Every number equal as bits, NaNs in the same places."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


def restated(a, b, w, peak, eps):
    """(rel [H, W], ssim [H - 10, W - 10], se, good, |d|) of the definition, every pixel and window at once."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    H, W, _ = a.shape
    with np.errstate(all="ignore"):
        d = a - b
        se = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        q = d * d / (b * b + eps)
        rel = (q[..., 0] + q[..., 1]) + q[..., 2]
        good = np.isfinite(a).all(-1) & np.isfinite(b).all(-1)
        ya, yb = [(LUM[0] * c[..., 0] + LUM[1] * c[..., 1]) + LUM[2] * c[..., 2] for c in (a, b)]
        if W < 11 or H < 11:
            return rel, np.zeros((0, 0)), se, good, np.abs(d)
        v = []
        for p in (ya, yb, ya * ya, yb * yb, ya * yb):
            h = w[0] * p[:, 0:W - 10]
            for i in range(1, 11):
                h = h + w[i] * p[:, i:W - 10 + i]
            t = w[0] * h[0:H - 10]
            for j in range(1, 11):
                t = t + w[j] * h[j:H - 10 + j]
            v.append(t)
        ma, mb = v[0], v[1]
        sa, sb, sab = v[2] - ma * ma, v[3] - mb * mb, v[4] - ma * mb
        c1, c2 = (0.01 * peak) * (0.01 * peak), (0.03 * peak) * (0.03 * peak)
        ssim = (((2.0 * ma) * mb + c1) * (2.0 * sab + c2)) / (((ma * ma + mb * mb) + c1) * ((sa + sb) + c2))
    return rel, ssim, se, good, np.abs(d)


def frames(w, h, fmt):
    """B a smooth ramp times gamma noise, A = B * (1 + noise), one pixel of A equal to B; f64 frames with
    room also get a NaN in A and a +inf in B, more than 11 pixels apart."""
    rng = np.random.default_rng(1000 * w + h)
    ys, xs = np.mgrid[0:h, 0:w]
    b = (0.1 + (xs + 2.0 * ys)[..., None] / (w + 2.0 * h) * [0.9, 0.6, 0.3]) * rng.gamma(4.0, 0.25, (h, w, 3))
    a = b * (1.0 + rng.normal(0.0, 0.1, (h, w, 3)))
    a[h // 2, w // 2] = b[h // 2, w // 2]
    if fmt == "u8":
        return [np.clip(np.rint(c * 200.0), 0, 255).astype(np.uint8) for c in (a, b)]
    if w >= 40 and h >= 25:
        a[2, 3, 1] = np.nan
        b[20, 30, 2] = np.inf
    return a, b


def check(rt, a, b, **kw):
    """image_metrics(a, b, maps=True, **kw) against the restatement; returns the restatement's ssim."""
    peak = kw.get("peak") or (255.0 if a.dtype == np.uint8 else 1.0)
    w = kw["window"] if "window" in kw else rt.ssim_window(1.5)
    rel, ssim, se, good, absd = restated(a, b, w, peak, kw.get("eps") or rt.RT_METRICS_EPS)
    got = rt.image_metrics(a, b, maps=True, **kw)
    assert same_bits(got["rel"], rel), np.argwhere(got["rel"] != rel)[:4]
    assert got["ssim_map"].shape == ssim.shape and same_bits(got["ssim_map"], ssim), np.argwhere(got["ssim_map"] != ssim)[:4]
    s, counts = got["summary"], np.isfinite(ssim)
    assert s[0] == (~good).sum() and s[3] == absd[good].max(initial=0.0)
    assert s[4] == counts.sum() and s[7] == ssim.size - counts.sum() and s[6] == ssim[counts].min(initial=np.inf)
    for i, terms in ((1, se[good]), (2, rel[good]), (5, ssim[counts])):
        print(i, s[i], math.fsum(terms), terms.size * 2.0 ** -53 * math.fsum(np.abs(terms)))
        assert abs(s[i] - math.fsum(terms)) <= terms.size * 2.0 ** -53 * math.fsum(np.abs(terms))
    return ssim


# 1x1, 40x10: no window; 11x11: exactly one; 12x11; 43x27: 2x2 blocks with partial cores, the last column and
# row of windows read a halo that crosses both block edges; 75x40: 3x3 blocks, W odd (f64 rows not 16-byte aligned)
@gpu
@pytest.mark.parametrize("fmt", ["f64", "u8"])
@pytest.mark.parametrize("size", [(1, 1), (40, 10), (11, 11), (12, 11), (43, 27), (75, 40)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_metrics_match_numpy(rt, size, fmt):
    a, b = frames(*size, fmt)
    ssim = check(rt, a, b)
    assert ssim.size == max(size[0] - 10, 0) * max(size[1] - 10, 0)
    assert ssim.size == 0 or np.isfinite(ssim).any()  # the non-finite windows are a strict subset
    if fmt == "f64" and size[0] >= 40 and size[1] >= 25:
        assert not np.isfinite(ssim).all()


@gpu
def test_frame_against_itself(rt):
    """2*m*m and m*m + m*m are the same bits, and so are 2*s and s + s: every ssim is exactly 1, every rel +0."""
    b = frames(43, 27, "u8")[1].astype(np.float64) / 255.0
    got = rt.image_metrics(b, b, maps=True)
    assert (got["rel"].view(np.uint64) == 0).all() and (got["ssim_map"] == 1.0).all()
    assert got["mse"] == 0.0 and got["ssim"] == 1.0 and got["bad_pixels"] == 0


@gpu
def test_no_default_left(rt):
    check(rt, *frames(43, 27, "f64"), window=rt.ssim_window(0.8), peak=2.5, eps=1e-3)


@gpu
def test_maps_are_optional(rt):
    a, b = frames(43, 27, "f64")
    assert same_bits(rt.image_metrics(a, b)["summary"], rt.image_metrics(a, b, maps=True)["summary"])


def test_argument_errors(rt):
    """The argument checks run before any device call."""
    L = rt.lib()
    n = C.c_uint64()
    assert L.rt_image_metrics_workspace_bytes(0, 8, C.byref(n)) == -1 and L.rt_image_metrics_workspace_bytes(8, 0, C.byref(n)) == -1
    mixed = (C.c_double * 11)(*([0.1] * 10 + [0.0]))
    for text, kw in (("width/height", dict(width=0, height=8)), ("width/height", dict(width=8, height=0)),
                     ("format", dict(width=8, height=8, format=2)), ("peak", dict(width=8, height=8, peak=-1.0)),
                     ("mixes", dict(width=8, height=8, window=mixed))):
        p = rt.rt_metrics_params(**kw)
        assert L.rt_image_metrics_async(C.byref(p), None, None, None, None, None, None, 0, None) == -1
        assert text in L.rt_last_error().decode()

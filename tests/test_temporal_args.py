"""rt_temporal_accumulate_async and rt_temporal_history_bytes refuse bad arguments before any device
call (CPU, no device: the pointers are never followed)."""
import ctypes as C

import pytest

W, H = 8, 4
HIST = 32 * W * H + 48 * W * H  # 1024 + 1536, both multiples of 256
BASE = 0x10000000
ORDER = ("mean", "sq", "count", "rays", "hits", "hist_prev", "hist_next", "out_mean", "out_sq", "out_count")
PTR = {k: BASE + i * 0x10000 for i, k in enumerate(ORDER)}
NAN, INF = float("nan"), float("inf")

# case -> (rt_temporal_params fields, previous camera fields or None for no camera, pointers)
CASES = {
    "zero_width": (dict(width=0), {}, {}),
    "zero_height": (dict(height=0), {}, {}),
    "camera_without_history": ({}, {}, dict(hist_prev=0)),
    "history_without_camera": ({}, None, {}),
    "camera_of_another_size": ({}, dict(width=W + 1), {}),
    "singular_basis": ({}, dict(cam_up=(1.0, 0.0, 0.0)), {}),
    "nan_basis": ({}, dict(cam_forward=(0.0, NAN, 1.0)), {}),
    "spp_0": (dict(spp=0), {}, dict(count=0)),
    "spp_above_2^30": (dict(spp=(1 << 30) + 1), {}, dict(count=0)),
    "max_history_above_2^30": (dict(max_history=(1 << 30) + 1), {}, {}),
    "unknown_flag": (dict(flags=2), {}, {}),
    "normal_min_above_1": (dict(normal_min=1.5), {}, {}),
    "normal_min_negative": (dict(normal_min=-0.5), {}, {}),
    "normal_min_nan": (dict(normal_min=NAN), {}, {}),
    "plane_tol_negative": (dict(plane_tol=-1.0), {}, {}),
    "plane_tol_inf": (dict(plane_tol=INF), {}, {}),
    "null_mean": ({}, {}, dict(mean=0)),
    "null_hits": ({}, {}, dict(hits=0)),
    "null_hist_next": ({}, {}, dict(hist_next=0)),
    "null_out_count": ({}, {}, dict(out_count=0)),
    "mean_off_by_8": ({}, {}, dict(mean=PTR["mean"] + 8)),
    "hist_next_off_by_128": ({}, {}, dict(hist_next=PTR["hist_next"] + 128)),
    "count_off_by_2": ({}, {}, dict(count=PTR["count"] + 2)),
    "out_mean_is_sq": ({}, {}, dict(out_mean=PTR["sq"])),
    "hist_next_in_hist_prev": ({}, {}, dict(hist_next=PTR["hist_prev"] + HIST - 256)),
    "out_sq_in_out_mean": ({}, {}, dict(out_sq=PTR["out_mean"] + 24 * W * H - 16)),
    "out_count_in_hist_next": ({}, {}, dict(out_count=PTR["hist_next"] + 4)),
}


@pytest.mark.parametrize("case", CASES)
def test_argument_errors(rt, case):
    fields, camera, pointers = CASES[case]
    p = rt.rt_temporal_params(**dict(dict(width=W, height=H, spp=4), **fields))
    prev = None if camera is None else C.byref(rt.RenderParams(W, H).replace(**camera).to_c())
    ptr = dict(PTR, **pointers)
    rc = rt.lib().rt_temporal_accumulate_async(C.byref(p), prev, *(C.c_void_p(ptr[k]) for k in ORDER), None)
    assert rc == rt.RT_ERR_INVALID


@pytest.mark.parametrize("size,want", [((8, 4), HIST), ((37, 29), 34560 + 51712), ((0, 4), None), ((4, 70000), None)])
def test_history_bytes(rt, size, want):
    n = C.c_uint64()
    rc = rt.lib().rt_temporal_history_bytes(*size, C.byref(n))
    assert (rc, n.value) == (0, want) if want else rc == rt.RT_ERR_INVALID

"""The reach records and the tile selection on the host (rt.h rt_tile_reach_host / rt_refine_select;
rt_refine_host.cpp over rt_refine_math.h) against the NumPy restatement of refine_ref.py bit for bit, over
rt_reproject_host's output on test_reproject_host.py's synthetic cases, the selection rule on those counts
and on a tie, and the argument errors.  No device.
"""
import ctypes
import functools

import numpy as np
import pytest

import rtamd
from rtamd import _lib
import refine_ref as RR
from test_reproject_host import SHAPES, case

F = np.float32
MIN_COUNTS = (1.5, 4.0, 1e9)
# rt_reproject_host at its defaults on the clean 32x18 case, min_count 4: the short pixels of its 4x3 tiles
CLEAN_32x18_SHORT = [3, 0, 5, 20, 6, 1, 28, 44, 16, 3, 0, 3]


@functools.lru_cache(maxsize=None)
def reprojected(W, H, clean):
    c = case(W, H, clean=clean)
    out = rtamd.reproject_host(c["hist"], c["hnd"], c["hai"], c["hcam"], c["image"], c["tf"], c["nd"], c["ai"], c["cam"])
    out.setflags(write=False)
    return out


def planted(W, H):
    """The dirty case's result with every pixel of the last tile a count that is not good: NaN, +inf, negative, 0."""
    r = reprojected(W, H, False).copy()
    x0, y0 = (W - 1) // 8 * 8, (H - 1) // 8 * 8
    bad = [np.nan, np.inf, -3.0, 0.0]
    k = 0
    for y in range(y0, H):
        for x in range(x0, W):
            r[y, x, 3] = bad[k % 4]
            k += 1
    assert k >= 4
    return r


def same_records(a, b):
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1. the host function against the restatement -----------------------------------------------------------

@pytest.mark.parametrize("clean", [False, True], ids=["dirty", "clean"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_matches_numpy_bit_for_bit(shape, clean):
    W, H = shape
    r = reprojected(W, H, clean)
    nt = ((W + 7) // 8) * ((H + 7) // 8)
    for mc in MIN_COUNTS:
        got = rtamd.tile_reach_host(r, mc)
        ref = RR.tile_reach(r, mc)
        assert got.dtype == rtamd.TILE_REACH_DTYPE == RR.REACH_DTYPE and got.shape == (nt,)
        assert same_records(got, ref), (mc, got, ref)
        assert (got["pixels"] <= 64).all() and got["pixels"].sum() == W * H
        assert (got["short_px"] <= got["pixels"]).all()
    # nothing reaches 1e9: every pixel is short, a whole tile's 64
    far = rtamd.tile_reach_host(r, 1e9)
    assert np.array_equal(far["short_px"], far["pixels"]) and far["short_px"][0] == 64
    if shape == (13, 9):   # partial tiles both ways
        assert far["pixels"].tolist() == [64, 40, 8, 5]
    # the counts differ between pixels, so the thresholds separate them
    some = rtamd.tile_reach_host(r, 4.0)
    assert 0 < some["short_px"].sum() < W * H
    good = np.isfinite(some["n_min"])
    assert (some["n_min"][good] > 0).all() and (some["n_sum"][good] >= some["n_min"][good]).all()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_planted_counts_that_are_not_good(shape):
    W, H = shape
    r = planted(W, H)
    for mc in MIN_COUNTS:
        got, ref = rtamd.tile_reach_host(r, mc), RR.tile_reach(r, mc)
        assert same_records(got, ref), (mc, got, ref)
    got = rtamd.tile_reach_host(r, 4.0)
    last = got[-1]
    assert last["n_min"] == np.inf and last["n_sum"] == 0.0            # no good pixel in the tile
    assert np.isinf(got["n_min"]).any() and np.isfinite(got["n_min"][0])
    assert last["pixels"] in (40, 8, 5, 16) and last["pixels"] < 64     # a partial tile
    if shape == (13, 9):
        assert last["pixels"] == 5
    # NaN, negative and 0 are short; +inf is a count that no threshold is above
    vals = r[(H - 1) // 8 * 8:, (W - 1) // 8 * 8:, 3].ravel()
    assert last["short_px"] == int((~(vals >= F(4.0))).sum()) == int(last["pixels"]) - int(np.isposinf(vals).sum())
    assert np.isposinf(vals).any() and np.isnan(vals).any() and (vals < 0).any() and (vals == 0).any()


# ---- 2. the selection ---------------------------------------------------------------------------------------

def select(reach, min_pixels=1, max_tiles=0):
    got = rtamd.refine_select(reach, min_pixels, max_tiles)
    ref, t = RR.refine_select(reach["short_px"], min_pixels, max_tiles)
    assert np.array_equal(got, ref), (min_pixels, max_tiles, got, ref)
    return got, t


def test_select_on_real_counts():
    reach = rtamd.tile_reach_host(reprojected(32, 18, True), 4.0)
    sp = reach["short_px"].tolist()
    assert len(sp) == 12
    assert sp == CLEAN_32x18_SHORT
    a, t = select(reach)                                   # every tile with a short pixel
    assert t == 1 and a.tolist() == [int(v >= 1) for v in sp] and a.sum() == 10
    a, t = select(reach, min_pixels=4)
    assert t == 4 and a.tolist() == [int(v >= 4) for v in sp] and a.sum() == 6
    # a cap of 3: the threshold rises past 16 (t = 17, the smallest that fits), so the least count chosen is 20
    a, t = select(reach, max_tiles=3)
    assert t == 17 and a.sum() == 3 and sorted(np.array(sp)[a == 1].tolist()) == [20, 28, 44]
    a, t = select(reach, max_tiles=12)                     # a cap nothing reaches changes nothing
    assert t == 1 and a.sum() == 10
    a, t = select(reach, min_pixels=64)
    assert a.sum() == 0
    # the structure, whatever the counts: a cap never admits a tile below one it leaves out
    for cap in range(1, 12):
        a, t = select(reach, max_tiles=cap)
        assert a.sum() <= cap and (np.array(sp)[a == 1] >= t).all() and (np.array(sp)[a == 0] < t).all()


def records(short_px):
    r = np.zeros(len(short_px), rtamd.TILE_REACH_DTYPE)
    r["short_px"] = short_px
    r["pixels"] = 64
    return r


def test_select_never_breaks_a_tie_by_index():
    a, t = select(records([8] * 6), max_tiles=2)
    assert a.sum() == 0 and t == 9                          # six equal tiles do not fit a cap of 2: none
    a, t = select(records([8, 9, 8, 9, 8, 9]), max_tiles=4)
    assert a.tolist() == [0, 1, 0, 1, 0, 1]
    a, t = select(records([64] * 5), max_tiles=4)           # every tile entirely fresh: nothing to favour
    assert a.sum() == 0 and t == 65
    a, t = select(records([64] * 5), max_tiles=5)
    assert a.sum() == 5
    a, t = select(records([64] * 5))
    assert a.sum() == 5
    n = ctypes.c_int(-1)
    L = rtamd.amd()
    assert L.rt_refine_select(None, 0, 1, 0, None, ctypes.byref(n)) == 0 and n.value == 0    # no tiles
    r = records([3, 0, 7])
    out = np.zeros(3, np.uint8)
    u8 = ctypes.POINTER(ctypes.c_uint8)
    assert L.rt_refine_select(r.ctypes.data_as(ctypes.POINTER(_lib.RtTileReach)), 3, 1, 0, out.ctypes.data_as(u8), None) == 0
    assert out.tolist() == [1, 0, 1]                        # n_active may be NULL


# ---- 3. arguments -------------------------------------------------------------------------------------------

def rt_err(code, fn):
    with pytest.raises(rtamd.RTError) as e:
        fn()
    assert e.value.code == code, e.value


def test_bad_arguments_are_invalid():
    r = reprojected(13, 9, True)
    for mc in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        rt_err(-1, lambda: rtamd.tile_reach_host(r, mc))
    L = rtamd.amd()
    tr_p = ctypes.POINTER(_lib.RtTileReach)
    out = np.zeros(8, rtamd.TILE_REACH_DTYPE)
    rp, op = r.ctypes.data_as(_lib.c_float_p), out.ctypes.data_as(tr_p)
    assert L.rt_tile_reach_host(rp, 13, 9, 4.0, op, 4) == 0
    for n_tiles in (3, 5, 0):
        assert L.rt_tile_reach_host(rp, 13, 9, 4.0, op, n_tiles) == -1
    assert L.rt_tile_reach_host(None, 13, 9, 4.0, op, 4) == -1
    assert L.rt_tile_reach_host(rp, 13, 9, 4.0, None, 4) == -1
    assert L.rt_tile_reach_host(rp, 0, 9, 4.0, op, 0) == -1
    assert L.rt_tile_reach_host(rp, 13, -1, 4.0, op, 4) == -1
    reach = records([1, 2, 3])
    for bad in (dict(min_pixels=0), dict(min_pixels=65), dict(min_pixels=-1), dict(max_tiles=-1)):
        rt_err(-1, lambda: rtamd.refine_select(reach, **bad))
    rt_err(-1, lambda: rtamd.refine_select(records([1, 65, 3])))         # a tile has 64 pixels
    u8 = ctypes.POINTER(ctypes.c_uint8)
    act = np.zeros(3, np.uint8)
    assert L.rt_refine_select(None, 3, 1, 0, act.ctypes.data_as(u8), None) == -1
    assert L.rt_refine_select(reach.ctypes.data_as(tr_p), 3, 1, 0, None, None) == -1
    assert L.rt_refine_select(reach.ctypes.data_as(tr_p), -1, 1, 0, act.ctypes.data_as(u8), None) == -1


def test_structs_have_the_header_layout_and_null_contexts_are_rejected():
    assert ctypes.sizeof(_lib.RtTileReach) == 16 == rtamd.TILE_REACH_DTYPE.itemsize
    assert ctypes.sizeof(_lib.RtRefineParams) == 32
    assert _lib.RtRefineParams.reserved.offset == 16
    L = rtamd.amd()
    n = ctypes.c_int()
    assert L.rt_reach_tiles(None, 4.0) == -1
    assert L.rt_read_tile_reach(None, None, 0, ctypes.byref(n)) == -1
    assert L.rt_render_moved_refined(None, None, 1, None, None, None, None, None, None, None) == -1
    assert L.rt_abi_version() == 1

"""The noise records' host half (rt.h rt_tile_noise_host / rt_refine_noise_select; csrc/rt_refine_host.cpp) on the
CPU: the records against the NumPy float32 restatement bit for bit on synthetic arrays with every kind of odd
value, and hand-made records through the selection against the float64 restatement."""
import ctypes
import math

import numpy as np
import pytest

import rtamd
from rtamd import _lib
import noise_refine_ref as NR

F = np.float32
FLT_MAX = float(np.finfo(F).max)
SIZES = [(1, 1), (8, 8), (9, 9), (13, 9), (70, 11)]
ODD_N = [np.nan, np.inf, -np.inf, -3.0, 0.0, -0.0]
ODD_S2 = [np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, 1e-42, 3e38]


def same_records(a, b):
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


def synthetic(w, h, seed):
    """A result [h, w, 4] and its s2 [h, w]: mostly plain values, every few pixels an odd count, colour or variance."""
    g = np.random.default_rng(seed)
    rgbn = g.random((h, w, 4), dtype=F)
    rgbn[..., 3] = g.integers(1, 70, (h, w)).astype(F)
    s2 = (g.random((h, w), dtype=F) * F(4)).astype(F)
    pick = g.integers(0, 9, (h, w))
    which = g.integers(0, 64, (h, w))
    for k, odd in enumerate(ODD_N):
        rgbn[..., 3][(pick == 0) & (which % len(ODD_N) == k)] = F(odd)
    for k, odd in enumerate(ODD_S2):
        s2[(pick == 1) & (which % len(ODD_S2) == k)] = F(odd)
    for k, odd in enumerate((np.nan, np.inf, -np.inf, 3e38)):             # a colour that is not finite, or sums past FLT_MAX
        rgbn[..., k % 3][(pick == 2) & (which % 4 == k)] = F(odd)
    return rgbn, s2


# ---- the records ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_records_match_the_restatement(size):
    w, h = size
    nt = ((w + 7) // 8) * ((h + 7) // 8)
    for seed in (1, 2):
        rgbn, s2 = synthetic(w, h, 10 * seed + w)
        for mc in (2.0, 4.0, 35.5, 1e9):
            got = rtamd.tile_noise_host(rgbn, s2, mc)
            ref = NR.tile_noise(rgbn, s2, mc)
            assert got.shape == (nt,) and got.dtype == rtamd.TILE_NOISE_DTYPE == NR.NOISE_DTYPE
            assert same_records(got, ref), (mc, got, ref)
            assert got["pixels"].sum() == w * h
            assert (got["known_px"].astype(int) + got["bad_px"] <= got["pixels"]).all()
            assert (got["thin_px"].astype(int) + got["bad_px"] <= got["pixels"]).all()
        assert np.array_equal(got["thin_px"], got["pixels"] - got["bad_px"])   # nothing reaches 1e9: every good pixel is thin


def test_the_odd_values_are_all_met():
    rgbn, s2 = synthetic(70, 11, 80)
    n = rgbn[..., 3]
    assert np.isnan(n).any() and np.isposinf(n).any() and np.isneginf(n).any() and (n < 0).any() and (n == 0).any()
    assert np.isnan(s2).any() and np.isinf(s2).any() and (s2 < 0).any()
    rec = rtamd.tile_noise_host(rgbn, s2, 4.0)
    assert rec["bad_px"].sum() > 0 and 0 < rec["known_px"].sum() < 70 * 11 - rec["bad_px"].sum()


def test_a_record_by_hand():
    rgbn = np.zeros((1, 3, 4), F)
    rgbn[0, 0] = (0.25, 0.5, 0.25, 4.0)      # known, v = 2 / 4
    rgbn[0, 1] = (1.0, 1.0, 1.0, 1.0)        # good, s2 unknown: thin
    rgbn[0, 2] = (np.nan, 0.0, 0.0, 7.0)     # bad
    s2 = np.array([[2.0, -1.0, 1.0]], F)
    rec = rtamd.tile_noise_host(rgbn, s2, 2.0)[0]
    assert rec.tolist() == (0.5, 4.0, 1, 1, 1, 3)
    rec = rtamd.tile_noise_host(rgbn, s2, 5.0)[0]                            # ... and below min_count: thin as well
    assert rec.tolist() == (0.5, 4.0, 1, 2, 1, 3)


def test_host_refuses_bad_arguments():
    rgbn, s2 = synthetic(13, 9, 3)
    for mc in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(rtamd.RTError):
            rtamd.tile_noise_host(rgbn, s2, mc)
    with pytest.raises(ValueError):
        rtamd.tile_noise_host(rgbn, s2[:, :-1], 2.0)
    L = rtamd.amd()
    out = np.zeros(4, rtamd.TILE_NOISE_DTYPE)
    fp = lambda a: a.ctypes.data_as(_lib.c_float_p)  # noqa: E731
    op = out.ctypes.data_as(ctypes.POINTER(_lib.RtTileNoise))
    assert L.rt_tile_noise_host(fp(rgbn), fp(s2), 13, 9, 2.0, op, 4) == 0
    assert L.rt_tile_noise_host(fp(rgbn), fp(s2), 13, 9, 2.0, op, 3) == -1
    assert L.rt_tile_noise_host(None, fp(s2), 13, 9, 2.0, op, 4) == -1
    assert L.rt_tile_noise_host(fp(rgbn), None, 13, 9, 2.0, op, 4) == -1
    assert L.rt_tile_noise_host(fp(rgbn), fp(s2), 13, 9, 2.0, None, 4) == -1
    assert L.rt_tile_noise_host(fp(rgbn), fp(s2), 0, 9, 2.0, op, 4) == -1


# ---- the selection -------------------------------------------------------------------------------------------

def records(rows):
    """(v_sum, y_sum, known_px, thin_px, bad_px, pixels) per tile."""
    out = np.zeros(len(rows), rtamd.TILE_NOISE_DTYPE)
    for i, row in enumerate(rows):
        out[i] = row
    return out


def check(tiles, target, active=None):
    got, stats = rtamd.refine_noise_select(tiles, target, active)
    ref, ref_stats = NR.noise_select(tiles, target, active)
    assert np.array_equal(got, ref), (got, ref)
    assert stats.keys() == ref_stats.keys()
    for k in stats:
        a, b = stats[k], ref_stats[k]
        assert a == b or (isinstance(a, float) and math.isnan(a) and math.isnan(b)), (k, a, b)
    return got, stats


# ybar = (64 + 64 + 32 + 6.4) / (64 + 64 + 32 + 64) with the tiles below
HAND = [(0.64, 64.0, 64, 0, 0, 64),     # 0: v_t = 0.01
        (64.0, 64.0, 64, 0, 0, 64),     # 1: v_t = 1
        (0.0, 32.0, 32, 0, 32, 64),     # 2: exact
        (6.4e-5, 6.4, 64, 0, 0, 64),    # 3: dark and quiet, v_t = 1e-6
        (0.0, 0.0, 0, 0, 40, 40)]       # 4: only bad pixels


def test_selection_by_the_variance():
    tiles = records(HAND)
    _, stats = check(tiles, 0.0)
    ybar = stats["sum_y"] / (stats["pixels"] - stats["bad"])
    assert stats["pixels"] == 296 and stats["bad"] == 72 and stats["known"] == 224 and stats["thin"] == 0
    assert stats["rounds"] == 0 and stats["converged"] == 0
    assert stats["noise"] == math.sqrt(stats["sum_v"] / 224) / ybar
    assert check(tiles, 0.0)[0].tolist() == [1, 1, 0, 1, 0]                  # target 0: every tile with variance
    assert check(tiles, 0.5 / ybar)[0].tolist() == [0, 1, 0, 0, 0]           # lim = 0.5: v_t > 0.25
    assert check(tiles, 0.05 / ybar)[0].tolist() == [1, 1, 0, 0, 0]          # lim = 0.05: v_t > 0.0025
    assert check(tiles, 2.0 / ybar)[0].tolist() == [0, 0, 0, 0, 0]
    assert check(tiles, FLT_MAX)[0].tolist() == [0, 0, 0, 0, 0]


def test_a_thin_pixel_forces_activity_at_any_target():
    rows = list(HAND)
    rows[2] = (0.0, 32.0, 31, 1, 32, 64)                                      # one thin pixel in the exact tile
    rows.append((0.0, 3.0, 0, 3, 0, 3))                                       # three fresh pixels, no estimate at all
    tiles = records(rows)
    for target in (0.0, 0.1, 10.0, FLT_MAX):
        got, _ = check(tiles, target)
        assert got[2] == 1 and got[5] == 1 and got[4] == 0, target
    assert check(tiles, FLT_MAX)[0].tolist() == [0, 0, 1, 0, 0, 1]            # FLT_MAX keeps only the thin tiles


def test_active_in_is_respected():
    tiles = records(HAND)
    mask = np.array([0, 1, 1, 1, 1], np.uint8)
    assert check(tiles, 0.0, mask)[0].tolist() == [0, 1, 0, 1, 0]
    assert check(tiles, 0.0, np.zeros(5, np.uint8))[0].tolist() == [0] * 5
    assert check(tiles, 0.0, np.ones(5, np.uint8))[0].tolist() == check(tiles, 0.0)[0].tolist()
    # the stats are over ALL tiles, whatever the mask
    assert check(tiles, 0.0, mask)[1] == check(tiles, 0.0)[1]


def test_stats_zero_and_infinite_cases():
    _, s = check(records([(0.0, 64.0, 64, 0, 0, 64)]), 0.1)
    assert s["noise"] == 0.0                                                   # sum_v 0 with known pixels
    _, s = check(records([(0.0, 0.0, 64, 0, 0, 64)]), 0.1)
    assert s["noise"] == 0.0                                                   # ... also when ybar is 0 too
    _, s = check(records([(1.0, 0.0, 64, 0, 0, 64)]), 0.1)
    assert s["noise"] == math.inf                                              # ybar alone is 0
    _, s = check(records([(0.0, 5.0, 0, 5, 0, 5)]), 0.1)
    assert s["noise"] == math.inf                                              # nothing known
    _, s = check(records([(0.0, 0.0, 0, 0, 7, 7)]), 0.1)
    assert s["noise"] == math.inf and s["sum_y"] == 0.0                        # no good pixel: ybar is 0
    got, s = check(records([]), 0.1)
    assert got.size == 0 and s["noise"] == math.inf and s["pixels"] == 0
    _, s = check(records([(np.inf, 64.0, 64, 0, 0, 64)]), 0.1)
    assert s["noise"] == math.inf


def raw_select(tiles, n, target, out=True, active=None):
    L = rtamd.amd()
    u8_p = ctypes.POINTER(ctypes.c_uint8)
    act = np.zeros(max(n, 1), np.uint8)
    return L.rt_refine_noise_select(None if tiles is None else tiles.ctypes.data_as(ctypes.POINTER(_lib.RtTileNoise)),
                                    None if active is None else active.ctypes.data_as(u8_p), n, target,
                                    act.ctypes.data_as(u8_p) if out else None, None, None)


def test_selection_refuses_bad_arguments():
    good = records(HAND)
    assert raw_select(good, 5, 0.1) == 0                                      # n_active and stats may be NULL
    assert raw_select(None, 0, 0.1, out=False) == 0                           # no tiles is fine
    assert raw_select(None, 5, 0.1) == -1
    assert raw_select(good, 5, 0.1, out=False) == -1
    assert raw_select(good, -1, 0.1) == -1
    for target in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert raw_select(good, 5, target) == -1, target
    for row in ((0.0, 1.0, 65, 0, 0, 65), (0.0, 1.0, 0, 65, 0, 64), (0.0, 1.0, 0, 0, 65, 65), (0.0, 1.0, 1, 0, 0, 65),
                (0.0, 1.0, 33, 0, 32, 64), (0.0, 1.0, 1, 0, 0, 0)):
        assert raw_select(records([HAND[0], row]), 2, 0.1) == -1, row
        with pytest.raises(rtamd.RTError):
            rtamd.refine_noise_select(records([row]), 0.1)
    with pytest.raises(ValueError):
        rtamd.refine_noise_select(good, 0.1, np.ones(4, np.uint8))

"""CPU tests of the adaptive-sampling layer's host-only entries (rt.h rt_adaptive_select,
rt_noise_from_tile_sums_frames) against a Python float (double) restatement, equal exactly; argument
checks without a device; the recorded kernel resources, which the tile indirection in the render
kernel must not change; and the command line's --adaptive rule.
"""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import rtamd
from rtamd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "raytracing-book_amd", "bin", "rtrender")
PROFILES = os.path.join(REPO, "profiles")


def random_tiles(seed, n=97):
    """Seeded tile records: plain ones, bad pixels, pixels == bad, all-zero y, partial tiles."""
    rng = np.random.default_rng(seed)
    t = np.zeros(n, dtype=rtamd.TILE_SUM_DTYPE)
    t["pixels"] = rng.choice([64, 64, 64, 32, 16, 4], n)
    t["bad"] = np.where(rng.random(n) < 0.2, rng.integers(0, 5, n), 0)
    t["bad"] = np.minimum(t["bad"], t["pixels"])
    t["y"] = (rng.random(n) * 40.0).astype(np.float32)
    t["m2y"] = (rng.random(n) * np.exp(rng.normal(0.0, 3.0, n))).astype(np.float32)
    dead = rng.random(n) < 0.1          # every pixel bad: both sums are +0
    t["bad"][dead] = t["pixels"][dead]
    t["y"][dead] = 0.0
    t["m2y"][dead] = 0.0
    dark = rng.random(n) < 0.1          # no light found yet: y and M2 all zero
    t["y"][dark] = 0.0
    t["m2y"][dark] = 0.0
    t["m2y"][rng.random(n) < 0.05] = np.float32(-1e-4)   # a negative sum is taken as it is
    assert n < 50 or (dead.any() and dark.any() and (t["bad"] > 0).any())
    return t


def good(t):
    return float(int(t["pixels"]) - int(t["bad"]))


def select_ref(tiles, active, F, min_frames, target):
    sy = sp = 0.0
    for t in tiles:
        sy += float(t["y"])
        sp += good(t)
    ybar = sy / sp if sp > 0.0 else 0.0
    lim = float(np.float32(target)) * ybar
    out = []
    for k, t in enumerate(tiles):
        keep = True if active is None else bool(active[k])
        if keep and F >= min_frames:
            pt = good(t)
            if pt == 0.0:
                keep = False
            else:
                v = float(t["m2y"]) / (float(F) * (float(F) - 1.0)) / pt
                keep = not (v <= lim * lim)
        out.append(1 if keep else 0)
    return out


def noise_frames_ref(tiles, frames):
    var = sm = sy = 0.0
    px = bad = 0
    for t, n in zip(tiles, frames):
        n = float(n)
        var += float(t["m2y"]) / (n * (n - 1.0))
        sm += float(t["m2y"])
        sy += float(t["y"])
        px += int(t["pixels"])
        bad += int(t["bad"])
    num = math.sqrt(max(0.0, var) * float(px - bad))
    noise = (0.0 if num == 0.0 else math.inf) if sy == 0.0 else num / sy
    return dict(sum_m2y=sm, sum_y=sy, pixels=px, bad=bad, frames=max(frames) if len(frames) else 0, converged=0,
                noise=noise)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("F,min_frames", [(16, 16), (17, 16), (8, 16), (2, 2), (400, 16)])
@pytest.mark.parametrize("target", [0.0, 0.02, 0.3, 5.0])
def test_adaptive_select_matches_the_restatement(seed, F, min_frames, target):
    tiles = random_tiles(seed)
    rng = np.random.default_rng(100 + seed)
    active = (rng.random(tiles.size) < 0.7).astype(np.uint8)   # some tiles already inactive
    for act in (active, None):
        got = rtamd.adaptive_select(tiles, act, F, min_frames, target)
        ref = select_ref(tiles, act, F, min_frames, target)
        assert list(got) == ref
        if act is not None:
            assert not (got.astype(bool) & ~act.astype(bool)).any()   # an inactive tile stays inactive
        if F < min_frames:
            assert list(got) == ([1] * tiles.size if act is None else list(act))
    if F >= min_frames and target in (0.02, 0.3):
        ref = select_ref(tiles, None, F, min_frames, target)
        dead = tiles["pixels"] == tiles["bad"]
        assert not any(ref[k] for k in np.nonzero(dead)[0])       # no good pixel: the tile stops


def test_adaptive_select_meets_the_global_target():
    """If every tile passes the rule at F, the image-level figure is at most the target."""
    tiles = random_tiles(5)
    tiles["m2y"] = np.abs(tiles["m2y"])
    F = 24
    for target in (0.5, 2.0, 50.0):
        keep = rtamd.adaptive_select(tiles, None, F, 16, target)
        if not keep.any():
            assert rtamd.noise_from_tile_sums(tiles, F)["noise"] <= target * (1 + 1e-12)
    assert not rtamd.adaptive_select(tiles, None, F, 16, 1e6).any()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_noise_from_tile_sums_frames_matches_the_restatement(seed):
    tiles = random_tiles(seed)
    rng = np.random.default_rng(seed)
    frames = rng.choice([2, 8, 16, 24, 400], tiles.size).astype(np.int32)
    got = rtamd.noise_from_tile_sums_frames(tiles, frames)
    ref = noise_frames_ref(tiles, [int(v) for v in frames])
    for k in ("sum_m2y", "sum_y", "noise"):
        assert np.float64(got[k]).view(np.uint64) == np.float64(ref[k]).view(np.uint64), (k, got[k], ref[k])
    for k in ("pixels", "bad", "frames", "converged"):
        assert got[k] == ref[k], k
    zero = np.zeros(3, rtamd.TILE_SUM_DTYPE)
    zero["pixels"] = 64
    assert rtamd.noise_from_tile_sums_frames(zero, [2, 3, 4])["noise"] == 0.0
    zero["m2y"] = 1.0
    assert rtamd.noise_from_tile_sums_frames(zero, [2, 3, 4])["noise"] == math.inf
    assert rtamd.noise_from_tile_sums_frames(zero[:0], [])["frames"] == 0


@pytest.mark.parametrize("frames", [2, 16, 4096])
def test_equal_counts_agree_with_the_plain_figure(frames):
    tiles = random_tiles(4)
    tiles["m2y"] = np.abs(tiles["m2y"])   # (no cancellation between tiles: the two sums round alike)
    a = rtamd.noise_from_tile_sums_frames(tiles, np.full(tiles.size, frames, np.int32))
    b = rtamd.noise_from_tile_sums(tiles, frames)
    assert a["noise"] == pytest.approx(b["noise"], rel=1e-12) and a["noise"] > 0
    for k in ("sum_m2y", "sum_y", "pixels", "bad", "frames"):
        assert a[k] == b[k], k


def test_argument_errors():
    L = rtamd.amd()
    tiles = random_tiles(1, 4)
    tp = tiles.ctypes.data_as(ctypes.POINTER(_lib.RtTileSum))
    u8_p, i32_p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int32)
    out = (ctypes.c_uint8 * 4)()
    n = ctypes.c_int()
    st = _lib.RtNoiseStats()
    fr = (ctypes.c_int32 * 4)(2, 2, 2, 2)
    assert L.rt_adaptive_select(tp, None, 4, 16, 16, 0.1, out, ctypes.byref(n)) == 0 and n.value <= 4
    assert L.rt_adaptive_select(tp, None, 4, 16, 16, 0.1, out, None) == 0
    assert L.rt_adaptive_select(tp, None, 4, 16, 1, 0.1, out, ctypes.byref(n)) == -1     # min_frames >= 2
    assert L.rt_adaptive_select(tp, None, 4, 0, 16, 0.1, out, ctypes.byref(n)) == -1     # frames >= 1
    assert L.rt_adaptive_select(tp, None, -1, 16, 16, 0.1, out, ctypes.byref(n)) == -1
    assert L.rt_adaptive_select(None, None, 4, 16, 16, 0.1, out, ctypes.byref(n)) == -1
    assert L.rt_adaptive_select(tp, None, 4, 16, 16, 0.1, None, ctypes.byref(n)) == -1
    assert L.rt_adaptive_select(None, None, 0, 16, 16, 0.1, None, ctypes.byref(n)) == 0 and n.value == 0
    assert L.rt_noise_from_tile_sums_frames(tp, fr, 4, ctypes.byref(st)) == 0
    assert L.rt_noise_from_tile_sums_frames(tp, fr, 4, None) == -1
    assert L.rt_noise_from_tile_sums_frames(None, fr, 4, ctypes.byref(st)) == -1
    assert L.rt_noise_from_tile_sums_frames(tp, None, 4, ctypes.byref(st)) == -1
    assert L.rt_noise_from_tile_sums_frames(tp, fr, -1, ctypes.byref(st)) == -1
    fr[2] = 1
    assert L.rt_noise_from_tile_sums_frames(tp, fr, 4, ctypes.byref(st)) == -1           # every count >= 2
    with pytest.raises(rtamd.RTError):
        rtamd.noise_from_tile_sums_frames(tiles, [2, 2, 1, 2])
    with pytest.raises(rtamd.RTError):
        rtamd.adaptive_select(tiles, None, 16, 1, 0.1)
    # the context entries reject a NULL context
    assert L.rt_set_active_tiles(None, out, 4) == -1
    assert L.rt_read_tile_frames(None, fr, 4, ctypes.byref(n)) == -1
    assert L.rt_write_tile_frames(None, fr, 4) == -1
    assert L.rt_render_adaptive(None, 1, 8, 4, 2, ctypes.c_uint64(1), 0.5, ctypes.byref(n), ctypes.byref(st)) == -1


def test_launch_fields_name_the_active_tiles():
    assert rtamd.render.LAUNCH_FIELDS[-1] == "tiles_active" and len(rtamd.render.LAUNCH_FIELDS) == 21


FIELDS = ("VGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
          "Occupancy [waves/SIMD]")


def render_instances(text):
    """`make resources` output -> {render_persistent instance: {field: value}}."""
    out, cur = {}, None
    for ln in text.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: .*?\s{2,}([A-Za-z][\w \[\]/-]*?): (\S+)", ln)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return {k: v for k, v in out.items() if "render_persistent" in k}


def test_recorded_resources_are_identical():
    """profiles/adaptive_resources_{parent,this}.txt: `make -C raytracing-book_amd resources` on the
    parent commit and on the commit that added the tile indirection as a compile-time option bit
    (RT_OPT_MASK, OPT + 512): every render_persistent instance of the parent is still there with
    its VGPRs, spills, scratch, LDS and occupancy, and each has its masked twin."""
    a = render_instances(open(os.path.join(PROFILES, "adaptive_resources_parent.txt")).read())
    b = render_instances(open(os.path.join(PROFILES, "adaptive_resources_this.txt")).read())
    assert len(a) >= 10 and set(a) <= set(b) and len(b) == 2 * len(a)
    for k in a:   # <MINW, STATS, BLOCK, OPT>: the twin's OPT has bit 512
        m = re.search(r"ELi(\d+)EEEvPK", k)
        assert m and int(m.group(1)) < 512 and k.replace(f"ELi{m.group(1)}EEEvPK", f"ELi{int(m.group(1)) + 512}EEEvPK") in b, k
    for k in a:
        for f in FIELDS:
            assert f in a[k], (k, f)
            assert a[k][f] == b[k][f], (k, f, a[k][f], b[k][f])


def test_cli_adaptive_needs_a_noise_target():
    r = subprocess.run([BIN, "-s", "0", "-r", "16:16", "-spp", "8", "--adaptive"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "--adaptive" in r.stderr and "--noise" in r.stderr
    r = subprocess.run([BIN, "-s", "0", "-r", "16:16", "-spp", "8", "--min-frames", "4"], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 1 and "--min-frames" in r.stderr
    r = subprocess.run([BIN, "-s", "0", "-r", "16:16", "-spp", "8", "--noise", "0.5", "--adaptive", "--min-frames", "1"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--min-frames" in r.stderr

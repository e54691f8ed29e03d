"""CPU tests of the sample-moments layer (rt.h rt_set_moments ... rt_render_until): the host-only
noise figure against a float64 restatement, argument checks without a device, and the render
kernels' resource usage, which the layer must not change (it lives in its own translation unit).
"""
import ctypes
import hashlib
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import rtamd
from rtamd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILES = os.path.join(REPO, "profiles")


def tiles_of(rows):
    t = np.zeros(len(rows), dtype=rtamd.TILE_SUM_DTYPE)
    for k, (m2y, y, bad, pixels) in enumerate(rows):
        t[k] = (np.float32(m2y), np.float32(y), bad, pixels)
    return t


def noise_ref(tiles, frames):
    """rt.h's formula in float64, the tiles summed in order."""
    sm = sy = 0.0
    px = bad = 0
    for t in tiles:
        sm += float(t["m2y"])
        sy += float(t["y"])
        px += int(t["pixels"])
        bad += int(t["bad"])
    num = math.sqrt(max(0.0, sm / (frames * (frames - 1.0))) * (px - bad))
    if sy == 0.0:
        noise = 0.0 if num == 0.0 else math.inf
    else:
        noise = num / sy
    return dict(sum_m2y=sm, sum_y=sy, pixels=px, bad=bad, frames=frames, converged=0, noise=noise)


CASES = {
    "plain": ([(0.5, 12.25, 0, 64), (1.75, 3.0, 0, 64), (0.001, 40.5, 0, 48)], 16),
    "bad_pixels": ([(0.5, 12.25, 3, 64), (0.0, 0.0, 64, 64), (2.5, 7.0, 1, 16)], 7),
    "order_matters": ([(1e8, 1.0, 0, 64), (1.0, 1e-3, 0, 64), (-1e8, 2.0, 0, 64), (1.0, 3.0, 0, 64)], 2),
    "negative_m2_sum": ([(-0.25, 5.0, 0, 64)], 3),
    "zero_over_zero": ([(0.0, 0.0, 0, 64), (0.0, 0.0, 0, 64)], 4),
    "something_over_zero": ([(0.5, 1.0, 0, 64), (0.25, -1.0, 0, 64)], 4),
    "no_tiles": ([], 2),
    "many_frames": ([(3.0e-5, 9.0, 0, 64)] * 50, 4096),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_noise_from_tile_sums_matches_float64(name):
    rows, frames = CASES[name]
    tiles = tiles_of(rows)
    got = rtamd.noise_from_tile_sums(tiles, frames)
    ref = noise_ref(tiles, frames)
    for k in ("sum_m2y", "sum_y", "noise"):
        assert np.float64(got[k]).view(np.uint64) == np.float64(ref[k]).view(np.uint64), (k, got[k], ref[k])
    for k in ("pixels", "bad", "frames", "converged"):
        assert got[k] == ref[k], k
    if name == "zero_over_zero":
        assert got["noise"] == 0.0
    if name == "something_over_zero":
        assert got["sum_y"] == 0.0 and got["noise"] == math.inf
    if name == "negative_m2_sum":
        assert got["noise"] == 0.0   # max(0, .) before the root


def test_noise_from_tile_sums_rejects_bad_arguments():
    L = rtamd.amd()
    tiles = tiles_of([(1.0, 1.0, 0, 64)])
    tp = tiles.ctypes.data_as(ctypes.POINTER(_lib.RtTileSum))
    st = _lib.RtNoiseStats()
    for frames in (1, 0, -3):
        assert L.rt_noise_from_tile_sums(tp, 1, frames, ctypes.byref(st)) == -1   # RT_ERR_INVALID_ARG
    assert L.rt_noise_from_tile_sums(tp, 1, 2, None) == -1
    assert L.rt_noise_from_tile_sums(None, 1, 2, ctypes.byref(st)) == -1
    assert L.rt_noise_from_tile_sums(tp, -1, 2, ctypes.byref(st)) == -1
    with pytest.raises(rtamd.RTError):
        rtamd.noise_from_tile_sums(tiles, 1)


def test_null_context_calls_are_rejected():
    L = rtamd.amd()
    buf = (ctypes.c_float * 4)()
    n = ctypes.c_int()
    st = _lib.RtNoiseStats()
    ts = _lib.RtTileSum()
    assert L.rt_set_moments(None, 1) == -1
    assert L.rt_read_moments(None, buf) == -1
    assert L.rt_write_moments(None, buf, 1) == -1
    assert L.rt_read_tile_sums(None, ctypes.byref(ts), 1, ctypes.byref(n)) == -1
    assert L.rt_noise(None, ctypes.byref(st)) == -1
    assert L.rt_render_until(None, 1, 4, 2, ctypes.c_uint64(1), 0.5, ctypes.byref(n), ctypes.byref(st)) == -1
    assert L.rt_debug_read_samples(None, buf, 4, ctypes.byref(n)) == -1


def test_structs_have_the_header_layout():
    assert ctypes.sizeof(_lib.RtTileSum) == 16 == rtamd.TILE_SUM_DTYPE.itemsize
    assert ctypes.sizeof(_lib.RtNoiseStats) == 48
    assert _lib.RtNoiseStats.noise.offset == 40 and _lib.RtNoiseStats.frames.offset == 32


# --- the render kernels compile exactly as before ------------------------------------------------

def parse_resources(text):
    """`make resources` output -> {kernel: {field: value}} (the -Rpass-analysis remarks)."""
    out, cur = {}, None
    for ln in text.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: .*?\s{2,}([A-Za-z][\w \[\]/-]*?): (\S+)", ln)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return out


def render_instances(res):
    return {k: v for k, v in res.items() if "render_persistent" in k}


FIELDS = ("VGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]")


def test_recorded_resources_are_identical():
    """profiles/moments_resources_{parent,this}.txt: `make -C raytracing-book_amd resources` on the
    parent commit and on this one."""
    a = render_instances(parse_resources(open(os.path.join(PROFILES, "moments_resources_parent.txt")).read()))
    b = render_instances(parse_resources(open(os.path.join(PROFILES, "moments_resources_this.txt")).read()))
    assert len(a) >= 10 and sorted(a) == sorted(b)
    for k in a:
        for f in FIELDS:
            assert f in a[k], (k, f)
            assert a[k][f] == b[k][f], (k, f, a[k][f], b[k][f])


KERNEL_SOURCES = ("rt_kernel.hip", "rt_kernel_common.h", "rt_device.h")


def kernel_source_hashes():
    csrc = os.path.join(REPO, "raytracing-book_amd", "csrc")
    return {n: hashlib.sha256(open(os.path.join(csrc, n), "rb").read()).hexdigest() for n in KERNEL_SOURCES}


@pytest.mark.slow
def test_render_kernel_resources_match_the_parent():
    """The same report compiled from this tree against the parent's recorded one: VGPRs, spills,
    scratch and LDS of every render_persistent instance.  The record is about the commit that
    added the moments: it is compared only while the kernel sources are the ones it was taken
    from (profiles/moments_resources_sources.json); a later change of the render kernels
    changes their resources on purpose and is not this test's business."""
    recorded = json.load(open(os.path.join(PROFILES, "moments_resources_sources.json")))
    if kernel_source_hashes() != recorded["sha256"]:
        return
    r = subprocess.run(["make", "-C", os.path.join(REPO, "raytracing-book_amd"), "resources"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    now = render_instances(parse_resources(r.stdout))
    parent = render_instances(parse_resources(open(os.path.join(PROFILES, "moments_resources_parent.txt")).read()))
    assert len(parent) >= 10 and sorted(now) == sorted(parent)
    for k in parent:
        for f in FIELDS:
            assert now[k][f] == parent[k][f], (k, f, now[k][f], parent[k][f])

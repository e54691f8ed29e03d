"""Every render_persistent instance rt_render can launch, on the device, against the CPU oracle bit for bit.

tests/kernel_matrix.py names, for each of the 52 reachable instances (26 entries of RT_RENDER_KERNELS and their
tile-mask twins), the scene and options that launch it; one test per instance (id BLOCK-OPT) runs that
instance's configurations: its row as the default staged launch for an RT_OPT_STD kernel, under all four
staging states for the others (sparse staging, dense staging, ordered one-frame chunks, one chunk in place),
and (512, 47) also with every table in LDS.  Per configuration, at 61x45 (ragged right column and bottom row
of tiles), depth 5, spp 6:
  * two launches, frames 1-3 then 4-6; before each the host plans the launch from the scene, the options, the
    mask, the tile counts, the device's resident waves and its free memory, and after each all 21 fields of
    rt_debug_last_launch must equal the plan, whose (block, opt) must be the test's id -- rt_debug_last_launch
    does not carry OPT, so this is what proves which kernel ran;
  * the image (a twin: the pixels of the active tiles) equals pyoracle.render of the same six frames;
  * a twin starts from an image of distinct finite bit patterns: every word outside the active tiles still
    holds its pattern, rt_read_tile_frames is 6 on the active tiles and unchanged on the others; then the
    other 43 tiles are rendered through the same twin (one launch of six frames, planned and checked alike)
    and the whole image equals the oracle's, so a twin's leaf and shading code sees every pixel.
No tolerance anywhere.  The four instances left out are kernel_matrix.DEAD (tests/test_kernel_matrix.py).
"""
import functools

import numpy as np
import pytest
import torch

import kernel_matrix as km
import pyoracle
import rtamd
from helpers import bit_equal, mismatch_report

pytestmark = pytest.mark.gpu

KERNELS = km.kernels()


@functools.lru_cache(maxsize=None)
def oracle_image(name):
    """The six frames of a scene (s8, s0, edges), computed once and never written to."""
    o = pyoracle.OracleScene(km.scene(name), max_depth=km.DEPTH, spp=km.FRAMES)
    img = pyoracle.render(o, rtamd.frame_rand_factors(1, 0, km.FRAMES))
    img.setflags(write=False)
    return img


def pattern(base=0x3F800000):
    """A distinct positive finite float per word: bits base + index (tests/test_gpu_adaptive.py pattern)."""
    bits = np.uint32(base) + np.arange(km.H * km.W * 4, dtype=np.uint32)
    out = bits.view(np.float32).reshape(km.H, km.W, 4).copy()
    assert np.isfinite(out).all() and (out > 0).all()
    return out


def pixels_of(tiles):
    """Tile indices -> per-pixel bool [H, W]."""
    t = np.zeros(km.NT, bool)
    t[tiles] = True
    return np.repeat(np.repeat(t.reshape(km.TY, km.TX), 8, axis=0), 8, axis=1)[:km.H, :km.W]


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def run(kernel, label, name, options, mask):
    scene = km.scene(name)
    waves = torch.cuda.get_device_properties(0).multi_processor_count * 16
    ctx = rtamd.RenderContext(devices=(0,), options=options or None)
    try:
        ctx.upload_scene(scene)
        ctx.set_params(max_depth=km.DEPTH, spp=km.FRAMES)
        ctx.resize(km.W, km.H)
        pat = None
        if mask is not None:
            pat = pattern()
            ctx.write_image(pat)
            active = np.zeros(km.NT, np.uint8)
            active[mask] = 1
            ctx.set_active_tiles(active)
        start = ctx.read_tile_frames()
        assert start.size == km.NT and not start.any()
        for first in (1, km.LAUNCH + 1):
            launch(ctx, kernel, label, scene, options, mask, first, km.LAUNCH, waves)
        img = ctx.read_image()
        counts = ctx.read_tile_frames()
        ref = oracle_image(name)
        if mask is None:
            assert (counts == km.FRAMES).all()
            assert bit_equal(img, ref), f"{kernel} {label}: {mismatch_report(img, ref)}"
            return
        px = pixels_of(mask)
        assert int(px.sum()) == 2 * 64 + 2 * 40 + 25   # tiles 7 and 40: 5 wide, 5 high; tile 47: 5 x 5
        assert bit_equal(img[px], ref[px]), \
            f"{kernel} {label}: {mismatch_report(np.where(px[..., None], img, 0), np.where(px[..., None], ref, 0))}"
        assert same_bits(img[~px], pat[~px]), f"{kernel} {label}: words outside the active tiles changed"
        want = start.copy()
        want[mask] = km.FRAMES
        assert np.array_equal(counts, want), (label, counts)
        # and the other 43 tiles through the same twin, all six frames in one launch: five tiles reach few of
        # the leaf and shading paths (a sphere-pair mutant of 1024-587 passed on them), the whole image does
        active = np.ones(km.NT, np.uint8)
        active[mask] = 0
        ctx.set_active_tiles(active)
        launch(ctx, kernel, label + " rest", scene, options, km.REST, 1, km.FRAMES, waves)
        img = ctx.read_image()
        assert (ctx.read_tile_frames() == km.FRAMES).all()
        assert bit_equal(img, ref), f"{kernel} {label} rest: {mismatch_report(img, ref)}"
    finally:
        ctx.close()


launch = km.launch   # shared with tests/test_gpu_random_scenes.py


@pytest.mark.parametrize("kernel", KERNELS, ids=[f"{b}-{o}" for b, o in KERNELS])
def test_kernel_matches_oracle(gpu, kernel):
    cfgs = km.configurations(kernel)
    assert len(cfgs) == (1 if kernel[1] & km.STD else 5 if kernel[1] & ~km.MASKED == 47 and kernel[0] == 512 else 4)
    for label, name, options, mask in cfgs:
        assert (mask is not None) == bool(kernel[1] & km.MASKED)
        run(kernel, label, name, options, mask)

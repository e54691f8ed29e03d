"""The variance-guided a-trous preview filter on the device (rt.h rt_denoise / rt_read_denoised; kernels
in rt_denoise.hip) against the host reference rt_denoise_host, bit for bit: both run
rt_denoise_math.h's operations, and tests/test_denoise_host.py pins the host reference to a numpy
restatement of rt.h's definition.  Injected inputs use that file's generator and shapes (plus one that
spans several workgroups in x); the renders are 40x24, depth 5, seed 1.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import rtamd
from rtamd import _lib
import test_denoise_host as TH
from helpers import bit_equal, mismatch_report

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1
W, H = 40, 24
GPU_SHAPES = TH.SHAPES + [(150, 37)]   # 3 workgroups across (64 pixels each, the last partial), 10 down


def context(scene, spp, **kw):
    ctx = rtamd.RenderContext(**kw)
    ctx.upload_scene(scene)
    ctx.set_params(max_depth=5, spp=spp)
    ctx.resize(scene.width, scene.height)
    return ctx


def render(ctx, first, n, seed=SEED):
    ctx.render(first, rtamd.frame_rand_factors(seed, first - 1, n))


def rt_err(code, fn):
    with pytest.raises(rtamd.RTError) as e:
        fn()
    assert e.value.code == code, e.value


def inject(ctx, w, h, img, m2, tf):
    ctx.resize(w, h)
    ctx.set_moments(True)
    ctx.write_image(img)
    ctx.write_moments(m2, int(tf.max()))
    if tf.min() != tf.max():
        ctx.write_tile_frames(tf)
    assert list(ctx.read_tile_frames()) == list(tf)


# ---- 1. injected inputs ---------------------------------------------------------------------------

@pytest.mark.parametrize("levels", TH.LEVELS)
@pytest.mark.parametrize("shape", GPU_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_injected_inputs_match_the_host(gpu, shape, levels):
    w, h = shape
    img, m2, tf = TH.make_inputs(w, h, seed=1000 * w + 10 * h + levels)
    ctx = rtamd.RenderContext()
    inject(ctx, w, h, img, m2, tf)
    for k in TH.KS:
        got = ctx.denoise(levels=levels, k=k)
        ref = rtamd.denoise_host(img, m2, tf, levels=levels, k=k)
        assert TH.same_bits(got, ref), (k, TH.where_differs(got, ref))
    # neither input was written
    assert TH.same_bits(ctx.read_image(), img) and TH.same_bits(ctx.read_moments(), m2)
    ctx.close()


def test_uniform_counts_and_defaults(gpu):
    w, h = 37, 23
    img, m2, tf = TH.make_inputs(w, h, seed=77, counts=7)
    ctx = rtamd.RenderContext()
    inject(ctx, w, h, img, m2, tf)
    got = ctx.denoise()
    assert TH.same_bits(got, rtamd.denoise_host(img, m2, 7)), TH.where_differs(got, rtamd.denoise_host(img, m2, 7))
    assert TH.same_bits(got, ctx.denoise(levels=3, k=3.0))
    # other counts, same buffers: the device's copy of the counts follows
    tf2 = TH.make_inputs(w, h, seed=78)[2]
    ctx.write_tile_frames(tf2)
    got2 = ctx.denoise()
    assert TH.same_bits(got2, rtamd.denoise_host(img, m2, tf2)) and not TH.same_bits(got2, got)
    # zero variance: the identity
    clean = TH.make_inputs(w, h, seed=79, bad=False)[0]
    ctx.write_image(clean)
    ctx.write_moments(np.zeros_like(m2), 5)
    assert TH.same_bits(ctx.denoise(levels=5)[..., :3], clean[..., :3])
    ctx.close()


# ---- 2. after real renders ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def scene_of(sid, w=W, h=H):
    return rtamd.Scene(sid, w, h, seed=SEED)


def check_against_host(ctx, **kw):
    img, m2, tf = ctx.read_image(), ctx.read_moments(), ctx.read_tile_frames()
    got = ctx.denoise(**kw)
    ref = rtamd.denoise_host(img, m2, tf, **kw)
    assert TH.same_bits(got, ref), TH.where_differs(got, ref)
    assert TH.same_bits(ctx.read_image(), img) and TH.same_bits(ctx.read_moments(), m2)
    assert list(ctx.read_tile_frames()) == list(tf)
    assert not TH.same_bits(got[..., :3], img[..., :3])   # the filter did something
    return got, tf


def scene6_run(with_denoise):
    ctx = context(scene_of(6), 16)
    ctx.set_moments(True)
    render(ctx, 1, 8)
    den = None
    if with_denoise:
        den, tf = check_against_host(ctx)
        assert list(tf) == [8] * len(tf)
    render(ctx, 9, 8)
    out = dict(image=ctx.read_image(), m2=ctx.read_moments(), den=den, frames=list(ctx.read_tile_frames()))
    ctx.close()
    return out


def test_scene6_and_the_frames_after_it(gpu):
    a = scene6_run(True)
    b = scene6_run(False)
    assert a["frames"] == b["frames"] == [16] * 15
    assert bit_equal(a["image"], b["image"]), mismatch_report(a["image"], b["image"])
    assert bit_equal(a["m2"], b["m2"]), mismatch_report(a["m2"], b["m2"])
    # determinism: a second run gives the same filtered bits
    c = scene6_run(True)
    assert TH.same_bits(a["den"], c["den"])


def test_scene0_after_an_adaptive_render(gpu):
    probe = context(scene_of(0), 24)
    probe.set_moments(True)
    render(probe, 1, 16)
    tiles = probe.tile_sums()
    probe.close()
    # the median tile's relative noise at 16 frames as the target: about half the tiles stop by then
    good = (tiles["pixels"] - tiles["bad"]).astype(np.float64)
    ybar = tiles["y"].astype(np.float64).sum() / good.sum()
    rel = np.sqrt(np.maximum(0.0, tiles["m2y"].astype(np.float64)) / (16.0 * 15.0) / good) / ybar
    target = float(np.float32(np.median(rel)))
    ctx = context(scene_of(0), 24)
    ctx.set_moments(True)
    ctx.render_adaptive(target, 24, 8, min_frames=8, seed=SEED)
    counts = ctx.read_tile_frames()
    assert len(set(counts)) > 1 and counts.min() >= 8, counts
    for kw in (dict(), dict(levels=5, k=4.5), dict(levels=1, k=0.75)):
        got, tf = check_against_host(ctx, **kw)
        assert list(tf) == list(counts)
    ctx.close()


# ---- 3. state rules ---------------------------------------------------------------------------------

def raw_denoise(ctx, levels=3, k=3.0, reserved=None):
    return ctx._L.rt_denoise(ctx._h, ctypes.byref(TH.params(levels, k, reserved)))


def test_state_rules(gpu):
    buf = np.empty((H, W, 4), np.float32)
    read = lambda c: c._L.rt_read_denoised(c._h, buf.ctypes.data_as(_lib.c_float_p))
    two = rtamd.RenderContext(devices=(0, 0))
    two.resize(W, H)
    rt_err(-3, two.denoise)                                   # RT_ERR_STATE: a multi-device context
    two.close()
    part = rtamd.RenderContext(rank=0, world=2, stripe_rows=8)
    part.resize(W, H)
    part.set_moments(True)
    rt_err(-3, part.denoise)                                  # ... a partition
    part.close()
    empty = rtamd.RenderContext()                             # a (0, 0) context: no image
    rt_err(-3, empty.denoise)
    assert read(empty) == -3
    empty.set_moments(True)
    rt_err(-3, empty.denoise)
    empty.close()

    ctx = context(scene_of(6), 16)
    rt_err(-3, ctx.denoise)                                   # the moments are off
    assert read(ctx) == -3                                    # no result held
    ctx.set_moments(True)
    rt_err(-3, ctx.denoise)                                   # ... on, but nothing rendered: invalid
    render(ctx, 1, 1)
    rt_err(-3, ctx.denoise)                                   # one frame: every count is 1
    render(ctx, 2, 3)
    assert read(ctx) == -3
    # bad parameters: RT_ERR_INVALID_ARG, and still no result
    for levels in (0, -1, 6):
        assert raw_denoise(ctx, levels=levels) == -1, levels
    for k in (0.0, -2.0, float("nan"), float("inf")):
        assert raw_denoise(ctx, k=k) == -1, k
    for slot in range(6):
        r = [0] * 6
        r[slot] = 7
        assert raw_denoise(ctx, reserved=r) == -1, slot
    assert read(ctx) == -3
    first = ctx.denoise()
    assert read(ctx) == 0 and TH.same_bits(buf, first)
    assert ctx._L.rt_read_denoised(ctx._h, None) == -1        # NULL rgba
    assert read(ctx) == 0 and TH.same_bits(buf, first)        # the result stays until the next rt_denoise
    # a tile below two frames
    img, m2 = ctx.read_image(), ctx.read_moments()
    tf = np.full(15, 4, np.int32)
    tf[7] = 1
    ctx.write_tile_frames(tf)
    rt_err(-3, ctx.denoise)
    tf[7] = 0
    ctx.write_tile_frames(tf)
    rt_err(-3, ctx.denoise)
    tf[7] = 2
    ctx.write_tile_frames(tf)
    assert TH.same_bits(ctx.denoise(), rtamd.denoise_host(img, m2, tf))
    # the image overwritten: the moments are invalid until rt_write_moments
    ctx.write_image(img)
    rt_err(-3, ctx.denoise)
    ctx.write_moments(m2, 4)
    assert TH.same_bits(ctx.denoise(), first)
    # the buffers go with rt_resize and with rt_set_moments(0)
    ctx.resize(W, H)
    assert read(ctx) == -3
    render(ctx, 1, 4)
    assert TH.same_bits(ctx.denoise(), first)
    ctx.set_moments(False)
    assert read(ctx) == -3
    rt_err(-3, ctx.denoise)
    ctx.close()


# ---- 4. what it is worth ----------------------------------------------------------------------------

# scene, W, H -> the ratio RMSE(filtered) / RMSE(raw) measured on the CPU (tools/denoise_quality.py:
# oracle frames + rt_denoise_host; profiles/denoise_quality.json) and the bound halfway between it and 1
QUALITY = {(8, 96, 54): (0.5875, 0.7937), (6, 64, 64): (0.7788, 0.8894)}


def test_quality_bounds_are_the_recorded_ones():
    rec = json.load(open(os.path.join(REPO, "profiles", "denoise_quality.json")))
    seen = {(c["scene"], c["width"], c["height"]): c for c in rec["cases"]}
    for key, (ratio, bound) in QUALITY.items():
        c = seen[key]
        assert c["asserted"] and c["ratio_defaults"] == ratio and c["bound"] == bound == round((1.0 + ratio) / 2.0, 4)
        assert (c["frames"], c["ref_frames"], c["seed"], c["ref_seed"]) == (16, 1024, 1, 2)


@pytest.mark.parametrize("case", sorted(QUALITY), ids=lambda c: f"scene{c[0]}-{c[1]}x{c[2]}")
def test_quality(gpu, case):
    sid, w, h = case
    measured, bound = QUALITY[case]
    scene = rtamd.Scene(sid, w, h, seed=SEED)
    ref_ctx = context(scene, 1024)
    render(ref_ctx, 1, 1024, seed=2)
    ref = ref_ctx.read_image()
    ref_ctx.close()
    ctx = context(scene, 16)
    ctx.set_moments(True)
    render(ctx, 1, 16)
    raw = ctx.read_image()
    den = ctx.denoise()
    ctx.close()
    ratio = TH.rmse(den, ref) / TH.rmse(raw, ref)
    print(f"scene {sid} {w}x{h}: RMSE filtered / raw = {ratio:.4f} (CPU measurement {measured}, bound {bound})")
    assert ratio <= bound

"""The first-hit pass on the device (rt.h rt_render_features / rt_read_features; rt_features.hip) against
tests/features_ref.py's CPU reference, the state rules of the feature buffers, and the guided preview
filter (rt_denoise_guided) against its host reference bit for bit.  Renders are depth 5, seed 1.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import rtamd
from rtamd import _lib
import features_ref
import test_denoise_host as TH
from helpers import bit_equal, mismatch_report

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1
MISS = features_ref.MISS
GUIDES = (1.0, 2.0, 1.5)   # every term on, none of them the defaults


@functools.lru_cache(maxsize=None)
def scene_of(sid, w, h):
    return rtamd.Scene(sid, w, h, seed=SEED)


def context(scene, spp=16, **kw):
    ctx = rtamd.RenderContext(**kw)
    ctx.upload_scene(scene)
    ctx.set_params(max_depth=5, spp=spp)
    ctx.resize(scene.width, scene.height)
    return ctx


def render(ctx, first, n, seed=SEED):
    ctx.render(first, rtamd.frame_rand_factors(seed, first - 1, n))


def rt_err(code, fn, names=None):
    with pytest.raises(rtamd.RTError) as e:
        fn()
    assert e.value.code == code, e.value
    if names:
        assert names in str(e.value), e.value


def features(sid, w, h, bvh_mode=0):
    ctx = context(scene_of(sid, w, h))
    if bvh_mode:
        ctx.set_bvh_mode(bvh_mode)
    ctx.render_features()
    out = ctx.read_features()
    ctx.close()
    return out


# ---- 1. the buffers against the CPU reference -------------------------------------------------------

@pytest.mark.parametrize("case", features_ref.CASES + [(8, 13, 9), (9, 32, 18)], ids=lambda c: f"scene{c[0]}_{c[1]}x{c[2]}")
def test_buffers_match_the_reference(gpu, case):
    sid, w, h = case   # 13x9: partial tiles in both directions
    ref = features_ref.reference(sid, w, h)
    assert ref.tied.sum() <= features_ref.TIE_CAPS[sid] * w * h
    nd, alb, ids = features(sid, w, h)
    features_ref.check(ref, nd, alb, ids)
    miss = ids == MISS
    assert (nd[miss] == np.array([0, 0, 0, -1], np.float32)).all()
    assert (alb[miss] == ref.background).all()
    assert ref.hit.any()


def test_scene7_fog_is_seen_through(gpu):
    scene = scene_of(7, 32, 32)
    assert len(scene.buffers[3]) > 0   # the scene has constant media
    nd, alb, ids = features(7, 32, 32)
    hit = ids != MISS
    assert ((ids[hit] & 0xF) != features_ref.MEDIUM).all()
    # the media's boundary boxes are in no leaf: only the room's quads are hit, as in the reference
    assert set((ids[hit] & 0xF).tolist()) <= {features_ref.QUAD}
    features_ref.check(features_ref.reference(7, 32, 32), nd, alb, ids)


@pytest.mark.parametrize("sid", [0, 9])
def test_defocus_scenes_give_the_pinhole_result(gpu, sid):
    scene = scene_of(sid, 32, 18)
    assert scene.camera[3] > 0.0   # defocus_angle: the render's rays start on the disk
    nd, alb, ids = features(sid, 32, 18)
    features_ref.check(features_ref.reference(sid, 32, 18), nd, alb, ids)   # rays from camera_pos
    assert bit_equal(nd, features(sid, 32, 18)[0])                          # and nothing random in them


@pytest.mark.parametrize("case", [(6, 32, 32), (0, 32, 18), (8, 32, 24)], ids=lambda c: f"scene{c[0]}")
def test_sah_tree_gives_the_same_hits(gpu, case):
    sid, w, h = case
    ref = features_ref.reference(sid, w, h)
    nd, alb, ids = features(sid, w, h, bvh_mode=1)
    nd0, alb0, ids0 = features(sid, w, h)
    assert bit_equal(nd[..., 3], nd0[..., 3])
    assert np.array_equal(ids[~ref.tied], ids0[~ref.tied])
    features_ref.check(ref, nd, alb, ids)


def test_nothing_else_moves(gpu):
    def run(with_features):
        ctx = context(scene_of(6, 32, 32))
        ctx.set_moments(True)
        for first in (1, 5):
            if with_features:
                ctx.render_features()
            render(ctx, first, 4)
        if with_features:
            ctx.render_features()
        out = dict(image=ctx.read_image(), m2=ctx.read_moments(), frames=list(ctx.read_tile_frames()))
        if with_features:
            features_ref.check(features_ref.reference(6, 32, 32), *ctx.read_features())
        ctx.close()
        return out

    a, b = run(True), run(False)
    assert a["frames"] == b["frames"] == [8] * 16
    assert bit_equal(a["image"], b["image"]), mismatch_report(a["image"], b["image"])
    assert bit_equal(a["m2"], b["m2"]), mismatch_report(a["m2"], b["m2"])


# ---- 2. state ----------------------------------------------------------------------------------------

def test_state_rules(gpu):
    scene = scene_of(6, 32, 32)
    ctx = rtamd.RenderContext()
    ctx.upload_scene(scene)
    rt_err(-3, ctx.render_features)                                   # before rt_resize
    rt_err(-3, ctx.read_features, "rt_render_features")
    ctx.close()
    two = rtamd.RenderContext(devices=(0, 0))
    two.upload_scene(scene)
    two.resize(32, 32)
    rt_err(-3, two.render_features)                                   # a two-slot context
    two.close()
    part = rtamd.RenderContext(rank=0, world=2, stripe_rows=8)
    part.upload_scene(scene)
    part.resize(32, 32)
    rt_err(-3, part.render_features)                                  # a partition
    part.close()
    bare = rtamd.RenderContext()
    bare.resize(32, 32)
    rt_err(-3, bare.render_features)                                  # no scene
    bare.close()

    ctx = context(scene)
    ctx.set_moments(True)
    render(ctx, 1, 4)
    rt_err(-3, ctx.read_features, "rt_render_features")               # none held
    rt_err(-3, lambda: ctx.denoise(guides=True), "rt_render_features")
    ctx.render_features()
    first = ctx.read_features_raw()
    guided = ctx.denoise(guides=GUIDES)
    # either pointer may be NULL
    nd = np.empty((32, 32, 4), np.float32)
    assert ctx._L.rt_read_features(ctx._h, nd.ctypes.data_as(_lib.c_float_p), None) == 0 and bit_equal(nd, first[0])
    assert ctx._L.rt_read_features(ctx._h, None, nd.ctypes.data_as(_lib.c_float_p)) == 0 and bit_equal(nd, first[1])
    assert ctx._L.rt_read_features(ctx._h, None, None) == 0
    # bad guide parameters: RT_ERR_INVALID_ARG
    for bad in ((-1.0, 0.0, 0.0), (0.0, float("nan"), 0.0), (0.0, 0.0, float("inf"))):
        rt_err(-1, lambda: ctx.denoise(guides=bad))
    gp = _lib.RtGuideParams()
    gp.reserved[1] = 1
    assert ctx._L.rt_denoise_guided(ctx._h, None, ctypes.byref(gp)) == -1
    # stale after rt_set_camera, valid again after a second pass
    ctx.set_camera(scene.camera)
    rt_err(-3, ctx.read_features, "rt_render_features")
    rt_err(-3, lambda: ctx.denoise(guides=GUIDES), "rt_render_features")
    assert TH.same_bits(ctx.denoise(), rtamd.denoise_host(ctx.read_image(), ctx.read_moments(), ctx.read_tile_frames()))
    ctx.render_features()
    again = ctx.read_features_raw()
    assert bit_equal(again[0], first[0]) and bit_equal(again[1], first[1])
    assert TH.same_bits(ctx.denoise(guides=GUIDES), guided)
    # ... after rt_upload_texture
    t = scene.textures[0]
    buf = ctypes.create_string_buffer(t.data, len(t.data))
    assert ctx._L.rt_upload_texture(ctx._h, t.slot, t.format, t.width, t.height, buf) == 0
    rt_err(-3, ctx.read_features, "rt_render_features")
    ctx.render_features()
    assert bit_equal(ctx.read_features_raw()[1], first[1])
    # ... after rt_upload_buffer and rt_set_bvh_mode
    data = scene.buffers[0]
    assert ctx._L.rt_upload_buffer(ctx._h, 0, ctypes.create_string_buffer(data, len(data)), len(data)) == 0
    rt_err(-3, ctx.read_features, "rt_render_features")
    ctx.render_features()
    ctx.set_bvh_mode(1)
    rt_err(-3, ctx.read_features, "rt_render_features")
    ctx.set_bvh_mode(0)
    ctx.render_features()
    assert bit_equal(ctx.read_features_raw()[0], first[0])
    # rt_set_params does not: a miss keeps the background of the pass
    ctx.set_params(background=(0.25, 0.5, 0.75))
    assert bit_equal(ctx.read_features_raw()[1], first[1])
    # rt_resize frees them
    ctx.resize(32, 32)
    rt_err(-3, ctx.read_features, "rt_render_features")
    ctx.close()


# ---- 3. the guided filter ------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [(8, 32, 24), (6, 32, 32)], ids=lambda c: f"scene{c[0]}")
def test_guided_filter_matches_the_host(gpu, case):
    sid, w, h = case
    ctx = context(scene_of(sid, w, h))
    ctx.set_moments(True)
    render(ctx, 1, 16)
    ctx.render_features()
    img, m2, tf = ctx.read_image(), ctx.read_moments(), ctx.read_tile_frames()
    nd, ai = ctx.read_features_raw()
    for levels in (1, 3, 5):
        plain = ctx.denoise(levels=levels, k=3.0)
        got = ctx.denoise(levels=levels, k=3.0, guides=GUIDES)
        ref = rtamd.denoise_guided_host(img, m2, tf, nd, ai, levels=levels, k=3.0, guides=GUIDES)
        assert TH.same_bits(got, ref), (levels, TH.where_differs(got, ref))
        assert not TH.same_bits(got, plain)                          # the guides did something
        zero = ctx.denoise(levels=levels, k=3.0, guides=(0.0, 0.0, 0.0))
        assert TH.same_bits(zero, plain)                             # k = 0: rt_denoise's bits
    # the defaults (NULL guides) are the recorded ones
    rec = json.load(open(os.path.join(REPO, "profiles", "denoise_guided_quality.json")))["defaults"]
    dflt = ctx.denoise(guides=True)
    assert TH.same_bits(dflt, ctx.denoise(guides=(rec["kn"], rec["kz"], rec["ka"])))
    assert TH.same_bits(dflt, rtamd.denoise_guided_host(img, m2, tf, nd, ai))
    # neither the image, the moments nor the features were written
    assert TH.same_bits(ctx.read_image(), img) and TH.same_bits(ctx.read_moments(), m2)
    assert bit_equal(ctx.read_features_raw()[0], nd) and bit_equal(ctx.read_features_raw()[1], ai)
    ctx.close()


def test_quality_on_scene0(gpu):
    """Scene 0 (checker ground, small spheres) at tools/denoise_quality.py's size with the default guides:
    the RMSE ratio against a long render stays below the point halfway between the guided and the unguided
    ratio the CPU grid recorded (profiles/denoise_guided_quality.json) -- it fails when the guides stop
    helping, not on a last digit."""
    rec = json.load(open(os.path.join(REPO, "profiles", "denoise_guided_quality.json")))
    assert rec["beats_unguided_on_scene0"]
    guided, unguided = rec["ratios_at_defaults"]["0"], rec["ratios_unguided"]["0"]
    bound = rec["scene0_bound"]
    assert bound == round((guided + unguided) / 2.0, 4) and guided < bound < unguided
    c0 = [c for c in rec["cases"] if c["scene"] == 0][0]
    w, h = c0["width"], c0["height"]
    assert (c0["frames"], c0["ref_frames"], c0["seed"], c0["ref_seed"]) == (16, 1024, 1, 2)
    scene = rtamd.Scene(0, w, h, seed=SEED)
    ref_ctx = context(scene, 1024)
    render(ref_ctx, 1, 1024, seed=2)
    ref = ref_ctx.read_image()
    ref_ctx.close()
    ctx = context(scene, 16)
    ctx.set_moments(True)
    render(ctx, 1, 16)
    ctx.render_features()
    raw = ctx.read_image()
    den = ctx.denoise(guides=True)
    plain = ctx.denoise()
    ctx.close()
    ratio = TH.rmse(den, ref) / TH.rmse(raw, ref)
    print(f"scene 0 {w}x{h}: RMSE guided / raw = {ratio:.4f}, unguided / raw = {TH.rmse(plain, ref) / TH.rmse(raw, ref):.4f} "
          f"(CPU grid: guided {guided}, unguided {unguided}, bound {bound})")
    assert ratio <= bound

"""The per-pass trims of the scene-8 kernels (rt_kernel_common.h RT_PB_NOLIGHT: with no registered
light, shade()'s mixture sets d = vec3(0) without the lights_random call and takes the mixture pdf
and its reciprocal as constants) against the untrimmed twins (box_interior = 0) and the CPU oracle,
bit for bit.

The trim is compiled into the RT_OPT_BOXQ instantiations alone, and rt_debug_last_launch's
box_interior says which kernel ran.  Scene 8 (no light) at depth 5, 2 and 1 and under a tile mask; a
compact-box scene under a sphere-bounded fog without a light and with one registered quad light (the
lit launch takes the untrimmed mixture in the same kernel), with Lambertian, metal and dielectric
spheres (skip_pdf materials never reach the mixture), with zero_dir_end off (the isotropic lane's
zero direction ends one pass later), camera rays with +0, -0 and denormal direction components, and
one 1080p x 64-frame image on against off.
"""
import functools

import numpy as np
import pytest

import pyoracle
import rtamd
from adversarial import grid_camera
from helpers import bit_equal, mismatch_report

pytestmark = pytest.mark.gpu

W, H, FRAMES = 32, 18, 4


def render(scene, frames, options=None, depth=5, uniforms=None, spp=None, tiles=None):
    ctx = rtamd.RenderContext(devices=(0,), options=options)
    ctx.upload_scene(scene)
    if uniforms is not None:
        ctx.set_params(max_depth=depth, uniforms=uniforms)
    else:
        ctx.set_params(max_depth=depth, spp=spp or frames)
    ctx.resize(scene.width, scene.height)
    if tiles is not None:
        ctx.set_active_tiles(tiles)
    ctx.render(1, rtamd.frame_rand_factors(1, 0, frames))
    img, info = ctx.read_image(), ctx.last_launch()
    ctx.close()
    return img, info


def oracle(scene, frames, depth=5, uniforms=None):
    if uniforms is not None:
        o = pyoracle.OracleScene(scene, max_depth=depth, uniforms=uniforms)
    else:
        o = pyoracle.OracleScene(scene, max_depth=depth, spp=frames)
    return pyoracle.render(o, rtamd.frame_rand_factors(1, 0, frames))


def n_lights(scene):
    return scene.info["n_lights"]   # the registered lights (lights_count)


def on_off_oracle(scene, frames, depth=5, uniforms=None, options=None, ref=None):
    """This kernel, the box_interior = 0 twin and the oracle agree bit for bit; returns the image and
    what the default launch reported."""
    on, info_on = render(scene, frames, options, depth=depth, uniforms=uniforms)
    off, info_off = render(scene, frames, dict(options or {}, box_interior=0), depth=depth, uniforms=uniforms)
    print(f"launch on {info_on} off {info_off}")
    assert info_on["box_interior"] == 1 and info_off["box_interior"] == 0, f"{info_on} {info_off}"
    if ref is None:
        ref = oracle(scene, frames, depth, uniforms)
    assert bit_equal(on, off), "on vs off: " + mismatch_report(on, off)
    assert bit_equal(on, ref), "on vs oracle: " + mismatch_report(on, ref)
    return on, info_on


# ---- scene 8 (no registered light, background (0, 0, 0))


@functools.lru_cache(maxsize=None)
def scene8():
    return rtamd.Scene(8, 64, 36, seed=1)


@pytest.mark.parametrize("depth", [5, 2, 1])
def test_scene8_on_off_oracle(gpu, depth):
    scene = scene8()
    assert n_lights(scene) == 0
    on, info = on_off_oracle(scene, 4, depth=depth)
    if depth == 5:
        assert float(np.nanmean(on[..., :3])) > 0.01


def test_scene8_masked_on_off_oracle(gpu):
    """Half the tiles active (the RT_OPT_MASK twins): their pixels are the oracle's."""
    scene = scene8()
    w, h = 64, 36
    tx, ty = (w + 7) // 8, (h + 7) // 8
    tiles = (np.arange(tx * ty) % 2 == 0).astype(np.uint8)
    on, info_on = render(scene, 4, tiles=tiles)
    off, info_off = render(scene, 4, {"box_interior": 0}, tiles=tiles)
    assert info_on["box_interior"] == 1 and info_off["box_interior"] == 0, f"{info_on} {info_off}"
    assert info_on["tiles_active"] == int(tiles.sum()), info_on
    ref = oracle(scene, 4)
    px = np.kron(tiles.reshape(ty, tx), np.ones((8, 8), np.uint8))[:h, :w].astype(bool)
    assert bit_equal(on, off), "on vs off: " + mismatch_report(on, off)
    act, want = np.where(px[..., None], on, 0), np.where(px[..., None], ref, 0)
    assert bit_equal(act, want), "on vs oracle, active tiles: " + mismatch_report(act, want)


def test_scene8_1080p_64_frames_on_off(gpu):
    """The headline launch: a whole 1080p image of 64 frames, this kernel against its twin."""
    scene = rtamd.Scene(8, 1920, 1080, seed=1)
    on, info_on = render(scene, 64, spp=4096)
    off, info_off = render(scene, 64, {"box_interior": 0}, spp=4096)
    assert info_on["box_interior"] == 1 and info_off["box_interior"] == 0, f"{info_on} {info_off}"
    assert info_on["block"] == 1024, info_on
    assert bit_equal(on, off), mismatch_report(on, off)


# ---- a compact-box scene: three axis-aligned boxes under a sphere-bounded fog.  The emitting quad
# lights the scene either way; `light` registers it (lights_count 1), and then a mixture draw below
# 0.5 aims at it (lights_random) and lights_pdf_value is not 0.


def boxes_in_fog(light, spheres=False, camera=None):
    b = rtamd.SceneBuilder(seed=1)
    white = b.lambertian(b.solid(0.73, 0.73, 0.73))
    red = b.lambertian(b.solid(0.65, 0.05, 0.05))
    b.add(b.box((-1.5, -2, -7), (0, -0.25, -5), red))
    b.add(b.box((0.5, -2, -6), (2, 0.5, -4.5), white))
    b.add(b.box((-6, -3, -12), (6, -2, 3), white))   # the floor slab
    if spheres:
        b.add(b.sphere((-0.75, 0.35, -6), 0.6, b.dielectric(1.5)))
        b.add(b.sphere((2.5, -1.4, -3.5), 0.6, b.metal(b.solid(0.8, 0.8, 0.9), 0.25)))
        b.add(b.sphere((-2.5, -1.5, -3), 0.5, red))
    lq = b.add(b.quad((-2, 3.5, -8), (4, 0, 0), (0, 0, 4), b.diffuse_light(7, 7, 7)))
    if light:
        b.add_light(lq)
    b.add(b.constant_medium(b.sphere((0, 0, -3), 60.0, b.dielectric(1.5)), 0.02, b.isotropic(b.solid(0.9, 0.9, 0.9))))
    b.camera(look_from=(0.5, 0.5, 2), look_at=(0, -0.5, -6), vfov=65, background=(0.2, 0.25, 0.3))
    scene = b.finish(W, H)
    if camera is not None:
        scene.override_camera(camera)
    return scene


def test_boxes_in_fog_no_light(gpu):
    scene = boxes_in_fog(False)
    assert n_lights(scene) == 0
    on, info = on_off_oracle(scene, FRAMES)
    assert float(np.nanmean(on[..., :3])) > 0.01


def test_boxes_in_fog_one_registered_light(gpu):
    """lights_count 1: the same BOXQ kernel, the untrimmed mixture."""
    scene = boxes_in_fog(True)
    assert n_lights(scene) == 1
    lit, info = on_off_oracle(scene, FRAMES)
    dark, _ = render(boxes_in_fog(False), FRAMES)
    assert not bit_equal(lit, dark)   # registering the light changes the image: the lit branch ran


@pytest.mark.parametrize("light", [False, True])
def test_boxes_in_fog_with_three_sphere_materials(gpu, light):
    """A Lambertian, a metal and a dielectric sphere: metal and dielectric lanes return before the
    mixture, whichever branch it takes."""
    on_off_oracle(boxes_in_fog(light, spheres=True), FRAMES)


@pytest.mark.parametrize("spheres", [False, True])
def test_boxes_in_fog_zero_dir_end_off(gpu, spheres):
    """zero_dir_end = 0: an isotropic lane whose mixture draw is below 0.5 begins one more walk along
    vec3(0), which hits nothing and draws no rand()."""
    scene = boxes_in_fog(False, spheres=spheres)
    off_end, info = on_off_oracle(scene, FRAMES, options={"zero_dir_end": 0})
    on_end, _ = render(scene, FRAMES)
    assert bit_equal(on_end, off_end), mismatch_report(on_end, off_end)


# Camera rays whose direction has a +0, a -0 or a denormal y component (the walk's 1 / d.y is +inf,
# -inf or overflows): jittered (spp 1 uniforms), so d.y = (zero or denormal step) * (sub-pixel offset).
DENORM = np.float32(2.0 ** -140)
ZERO_Y = {"plus_zero": np.float32(0.0), "minus_zero": np.float32(-0.0), "denormal": DENORM, "minus_denormal": -DENORM}


@pytest.mark.parametrize("name", list(ZERO_Y))
def test_zero_and_denormal_direction_components(gpu, name):
    z = ZERO_Y[name]
    cam = grid_camera((0.5, 0.0, 2.0), (0.5 - 1.0, z, 2.0 - 1.0), (1 / 16, z, 0), (0, z, -1 / 16))
    scene = boxes_in_fog(False, camera=cam)
    on_off_oracle(scene, FRAMES, uniforms=rtamd.spp_uniforms(1))


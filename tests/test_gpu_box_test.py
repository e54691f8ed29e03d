"""The compact box test with one reciprocal per axis and no division per face (option
box_interior, rt_kernel_common.h box_test_compact_q) against the per-face divisions it replaces
(box_interior = 0) and the CPU oracle, bit for bit.

Custom scenes at 48x27 x 4 frames put boxes where the two forms could part: seen from outside
and from inside, rays on a face's plane and along an axis (zero direction components, plane
numerators and alpha / beta at exactly 0 and 1: the lanes that leave the shared-reciprocal
regime and send their wave through the division form), two boxes sharing a face (ties in t), a
box behind a closer sphere (ray_t.max already small) and an image-textured box (alpha / beta
reach the uv).  Then scene 8 small, and one whole 1080p image of it.
"""
import os

import numpy as np
import pytest

import pyoracle
import rtamd
from adversarial import EXACT, grid_camera
from helpers import bit_equal, mismatch_report

pytestmark = pytest.mark.gpu

W, H, FRAMES = 48, 27, 4
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _base():
    b = rtamd.SceneBuilder(seed=1)
    white = b.lambertian(b.solid(0.73, 0.73, 0.73))
    red = b.lambertian(b.solid(0.65, 0.05, 0.05))
    return b, white, red


def _light(b, y=4.0):
    # (a sphere in every scene: the default launch's kernels keep their sphere table in LDS)
    b.add(b.sphere((2.5, 2.5, -9), 0.4, b.metal(b.solid(0.8, 0.8, 0.9), 0.25)))
    lq = b.add(b.quad((-3, y, -12), (6, 0, 0), (0, 0, 8), b.diffuse_light(6, 6, 6)))
    b.add_light(lq)


def outside():
    b, white, red = _base()
    b.add(b.box((-1.5, -1, -7), (1, 0.75, -4.5), red))
    b.add(b.box((-6, -3, -14), (6, -2, 2), white))
    _light(b)
    b.camera(look_from=(2.5, 1.5, 1), look_at=(0, 0, -6), vfov=55, background=(0.2, 0.25, 0.3))
    return b.finish(W, H), None


def inside():
    b, white, red = _base()
    b.add(b.box((-3, -2, -8), (3, 2, 2), white))          # the camera's room: every face hit from inside
    b.add(b.box((-1, -2, -6), (0.5, -0.5, -4), red))
    b.add(b.sphere((-1.5, 0.5, -5), 0.5, b.dielectric(1.5)))
    lq = b.add(b.quad((-1, 1.99, -5), (2, 0, 0), (0, 0, 2), b.diffuse_light(8, 8, 8)))
    b.add_light(lq)
    b.camera(look_from=(0.5, 0.25, 0), look_at=(0, -0.5, -5), vfov=80, background=(0.1, 0.1, 0.1))
    return b.finish(W, H), None


def grazing():
    """An exact ray grid d = (-1.5 + x/16, 0.75 - y/16, -1) from the origin: column 24 has d.x = 0 and
    row 12 d.y = 0 (zero direction components); the camera lies on the plane y = 0 of box 1's top
    face and on the plane x = 0 shared by boxes 1 and 2; box 3's front face z = -4 spans
    x in [-2, 2], y in [-1, 1], so its edges and corners are hit at exact pixel centres."""
    b, white, red = _base()
    b.add(b.box((0, -2, -9), (3, 0, -2), white))
    b.add(b.box((-3, -2, -9), (0, -0.5, -2), red))
    b.add(b.box((-2, -1, -12), (2, 1, -4), white))
    _light(b)
    b.add(b.box((-6, -5, -20), (6, -4, 2), white))
    b.camera(background=(0.2, 0.25, 0.3))
    s = b.finish(W, H)
    s.override_camera(grid_camera((0, 0, 0), (-1.5 + 1 / 32, 0.75 - 1 / 32, -1), (1 / 16, 0, 0), (0, -1 / 16, 0)))
    return s, EXACT


def shared_face():
    b, white, red = _base()
    b.add(b.box((-2, -1, -8), (0, 1, -5), white))
    b.add(b.box((0, -1, -8), (2, 1, -5), red))            # shares x = 0
    b.add(b.box((-2, 1, -8), (2, 1.5, -5), white))        # lies on both: shares y = 1
    b.add(b.box((-6, -2, -14), (6, -1, 2), white))        # the floor touches them at y = -1
    _light(b)
    b.camera(look_from=(0, 0.5, 1), look_at=(0, 0, -6), vfov=60, background=(0.2, 0.25, 0.3))
    return b.finish(W, H), None


def behind_sphere():
    b, white, red = _base()
    b.add(b.sphere((0, 0, -3), 1.0, b.metal(b.solid(0.8, 0.8, 0.9), 0.1)))
    b.add(b.sphere((1.2, -0.4, -3.5), 0.6, b.dielectric(1.5)))
    b.add(b.box((-2.5, -1.5, -9), (2.5, 1.5, -6), red))   # behind them: ray_t.max already the sphere's t
    b.add(b.box((-6, -3, -14), (6, -1.5, 2), white))
    _light(b)
    b.camera(look_from=(0, 0.2, 1), look_at=(0, 0, -4), vfov=60, background=(0.2, 0.25, 0.3))
    return b.finish(W, H), None


def textured():
    b, white, red = _base()
    rgba = b.image(os.path.join(GOLD, "tex_rgba.png"), 5, 3)
    b.add(b.box((-1.5, -1, -6), (1.5, 1, -4), b.lambertian(rgba)))
    b.add(b.box((-6, -2, -14), (6, -1, 2), white))
    _light(b)
    b.camera(look_from=(2, 1.5, 0.5), look_at=(0, 0, -5), vfov=55, background=(0.3, 0.3, 0.35))
    return b.finish(W, H), None


SCENES = {"outside": outside, "inside": inside, "grazing": grazing, "shared_face": shared_face,
          "behind_sphere": behind_sphere, "textured": textured}


def render(scene, frames, options=None, depth=5, uniforms=None, spp=None):
    ctx = rtamd.RenderContext(devices=(0,), options=options)
    ctx.upload_scene(scene)
    if uniforms is not None:
        ctx.set_params(max_depth=depth, uniforms=uniforms)
    else:
        ctx.set_params(max_depth=depth, spp=spp or frames)
    ctx.resize(scene.width, scene.height)
    ctx.render(1, rtamd.frame_rand_factors(1, 0, frames))
    img, info = ctx.read_image(), ctx.last_launch()
    ctx.close()
    return img, info


@pytest.mark.parametrize("name", list(SCENES))
def test_custom_box_scene_on_off_oracle(gpu, name):
    scene, uniforms = SCENES[name]()
    on, info_on = render(scene, FRAMES, uniforms=uniforms)
    off, info_off = render(scene, FRAMES, {"box_interior": 0}, uniforms=uniforms)
    assert info_on["box_interior"] == 1 and info_off["box_interior"] == 0, f"{info_on} {info_off}"
    if uniforms is not None:
        o = pyoracle.OracleScene(scene, max_depth=5, uniforms=uniforms)
    else:
        o = pyoracle.OracleScene(scene, max_depth=5, spp=FRAMES)
    ref = pyoracle.render(o, rtamd.frame_rand_factors(1, 0, FRAMES))
    assert bit_equal(on, off), f"{name} on vs off: " + mismatch_report(on, off)
    assert bit_equal(on, ref), f"{name} on vs oracle: " + mismatch_report(on, ref)
    assert float(np.nanmean(on[..., :3])) > 0.01   # lit, not a black frame


def test_scene8_small_on_off(gpu):
    scene = rtamd.Scene(8, 64, 36, seed=1)
    on, info_on = render(scene, 4)
    off, info_off = render(scene, 4, {"box_interior": 0})
    assert info_on["box_interior"] == 1 and info_off["box_interior"] == 0, f"{info_on} {info_off}"
    assert bit_equal(on, off), mismatch_report(on, off)


def test_box_interior_changes_no_bit_1080p(gpu):
    """Scene 8 (ground boxes seen at grazing angles), a whole 1080p image, every ray of 8 frames."""
    scene = rtamd.Scene(8, 1920, 1080, seed=1)
    on, info_on = render(scene, 8, spp=4096)
    off, info_off = render(scene, 8, {"box_interior": 0}, spp=4096)
    assert info_on["box_interior"] == 1 and info_off["box_interior"] == 0, f"{info_on} {info_off}"
    assert bit_equal(on, off), mismatch_report(on, off)

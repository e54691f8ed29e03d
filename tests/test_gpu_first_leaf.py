"""The first-leaf prologue of the scene-8 kernels (rt_kernel.hip render_stream, option first_leaf: a walk
that starts at the spine's leaf tests that leaf where the walk begins, from a wave-uniform record)
against the form without it (first_leaf = 0) and the CPU oracle, bit for bit.  rt_debug_first_leaf says
whether a launch armed the prologue and which leaf it took.

The prologue runs the walk's own first two tests earlier in the pass, so every case must equal both.
Scene 8 small (plain and under a tile mask), custom compact-box scenes whose first leaf -- the
reference builder's right-most leaf: the two models with the smallest bounds -- holds each slot type,
origins that start at the root although the prologue is armed, rays with a -0 direction component (the
wave takes the exact walk form after the prologue), depths 1 and 2, and one 1080p image on against off.
"""
import functools

import numpy as np
import pytest

import pyoracle
import rtamd
from adversarial import EXACT, grid_camera, spine
from helpers import bit_equal, mismatch_report

pytestmark = pytest.mark.gpu

SPHERE, QUAD, MEDIUM, BOX = 1, 2, 3, 4
W, H, FRAMES = 48, 27, 4


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
    img, info, fl = ctx.read_image(), ctx.last_launch(), ctx.first_leaf()
    ctx.close()
    return img, info, fl


def oracle(scene, frames, depth=5, uniforms=None):
    if uniforms is not None:
        o = pyoracle.OracleScene(scene, max_depth=depth, uniforms=uniforms)
    else:
        o = pyoracle.OracleScene(scene, max_depth=depth, spp=frames)
    return pyoracle.render(o, rtamd.frame_rand_factors(1, 0, frames))


def on_off_oracle(scene, frames, depth=5, uniforms=None, armed=True, types=None, ref=None):
    """Renders with the prologue and without: the two and the oracle agree bit for bit; returns what
    the default launch reported."""
    on, info_on, fl_on = render(scene, frames, depth=depth, uniforms=uniforms)
    off, info_off, fl_off = render(scene, frames, {"first_leaf": 0}, depth=depth, uniforms=uniforms)
    print(f"first_leaf on {fl_on} off {fl_off} launch {info_on}")
    assert fl_off["armed"] == 0, fl_off
    assert fl_on["armed"] == (1 if armed else 0), f"{fl_on} {info_on}"
    if armed:
        assert info_on["box_interior"] == 1 and info_on["spine"] >= 1, info_on
        assert fl_on["link"] & 0x80000000 and fl_on["link"] != 0xFFFFFFFF, fl_on
    if types is not None:
        assert fl_on["types"] & 0x77 == types[0] | types[1] << 4, fl_on
    if ref is None:
        ref = oracle(scene, frames, depth, uniforms)
    assert bit_equal(on, off), "on vs off: " + mismatch_report(on, off)
    assert bit_equal(on, ref), "on vs oracle: " + mismatch_report(on, ref)
    return info_on, fl_on


# ---- scene 8


@functools.lru_cache(maxsize=None)
def scene8(w, h, frames):
    scene = rtamd.Scene(8, w, h, seed=1)
    return scene, oracle(scene, frames)


@pytest.mark.parametrize("w,h,frames", [(64, 36, 4), (200, 112, 8)])
def test_scene8_on_off_oracle(gpu, w, h, frames):
    scene, ref = scene8(w, h, frames)
    # the ground's box and the global fog; the rebuilt tree splits their leaf off at the root (spine 1 or 2)
    info, fl = on_off_oracle(scene, frames, types=(BOX, MEDIUM), ref=ref)
    assert 1 <= info["spine"] <= 2 and info["rebuilt"] == 1, info
    assert float(np.nanmean(ref[..., :3])) > 0.01


@pytest.mark.parametrize("w,h,frames", [(64, 36, 4), (200, 112, 8)])
def test_scene8_masked_on_off_oracle(gpu, w, h, frames):
    """Half the tiles active (the RT_OPT_MASK twin): their pixels are the oracle's."""
    scene, ref = scene8(w, h, frames)
    tx, ty = (w + 7) // 8, (h + 7) // 8
    tiles = (np.arange(tx * ty) % 2 == 0).astype(np.uint8)
    on, info_on, fl_on = render(scene, frames, tiles=tiles)
    off, info_off, fl_off = render(scene, frames, {"first_leaf": 0}, tiles=tiles)
    print(f"first_leaf on {fl_on} off {fl_off} launch {info_on}")
    assert fl_on["armed"] == 1 and fl_off["armed"] == 0, f"{fl_on} {fl_off}"
    assert info_on["tiles_active"] == int(tiles.sum()) and info_on["box_interior"] == 1, info_on
    px = np.kron(tiles.reshape(ty, tx), np.ones((8, 8), np.uint8))[:h, :w].astype(bool)
    assert bit_equal(on, off), "on vs off: " + mismatch_report(on, off)
    act, want = np.where(px[..., None], on, 0), np.where(px[..., None], ref, 0)
    assert bit_equal(act, want), "on vs oracle, active tiles: " + mismatch_report(act, want)


def test_scene8_1080p_on_off(gpu):
    """A whole 1080p image, 2 frames: the size at which packet walks once differed while small images
    passed."""
    scene = rtamd.Scene(8, 1920, 1080, seed=1)
    on, info_on, fl_on = render(scene, 2, spp=4096)
    off, info_off, fl_off = render(scene, 2, {"first_leaf": 0}, spp=4096)
    assert fl_on["armed"] == 1 and fl_off["armed"] == 0, f"{fl_on} {fl_off}"
    assert info_on["block"] == 1024 and info_on["box_interior"] == 1, info_on
    assert bit_equal(on, off), mismatch_report(on, off)


def test_scenes_0_and_6_are_not_armed(gpu):
    """Their kernels hold no prologue: unarmed, their walks begin as before, and the oracle's bits."""
    for sid in (0, 6):
        scene = rtamd.Scene(sid, W, H, seed=1)
        img, info, fl = render(scene, FRAMES)
        assert fl == {"armed": 0, "link": 0, "types": 0, "prims": 0}, (sid, fl)
        assert info["box_interior"] == 0 and info["spine"] == 0, (sid, info)
        ref = oracle(scene, FRAMES)
        assert bit_equal(img, ref), mismatch_report(img, ref)


# ---- custom compact-box scenes.  The builder sorts by descending bound minimum and splits in halves,
# so the right-most leaf -- the first the walk reaches -- holds the two models whose bounds reach
# furthest down the axes: (the smaller, the larger).  Every chain box contains them, so the spine runs
# down to that leaf.


def _world(b, room=True):
    """A lit interior: boxes, spheres, a light quad; at least 8 models, so the chain has 3 nodes."""
    white = b.lambertian(b.solid(0.73, 0.73, 0.73))
    red = b.lambertian(b.solid(0.65, 0.05, 0.05))
    b.add(b.box((-1.5, -2, -7), (0, -0.25, -5), red))
    b.add(b.box((0.5, -2, -6), (2, 0.5, -4.5), white))
    b.add(b.box((-4, -2, -9), (-2.5, 1, -7.5), white))
    b.add(b.sphere((-0.75, 0.35, -6), 0.6, b.dielectric(1.5)))
    b.add(b.sphere((2.5, -1.4, -3.5), 0.6, b.metal(b.solid(0.8, 0.8, 0.9), 0.25)))
    b.add(b.sphere((-2.5, -1.5, -3), 0.5, red))
    if room:
        b.add(b.box((-6, -3, -12), (6, -2, 3), white))   # the floor slab
    lq = b.add(b.quad((-2, 3.5, -8), (4, 0, 0), (0, 0, 4), b.diffuse_light(7, 7, 7)))
    b.add_light(lq)
    return white, red


def _camera(b):
    b.camera(look_from=(0.5, 0.5, 2), look_at=(0, -0.5, -6), vfov=65, background=(0.2, 0.25, 0.3))


def _fog(b, r, density=0.02, colour=(0.9, 0.9, 0.9)):
    return b.constant_medium(b.sphere((0, 0, -3), r, b.dielectric(1.5)), density, b.isotropic(b.solid(*colour)))


def box_medium():
    """(a) as in scene 8: a huge box (the ground, r 40) and the global fog (r 60)."""
    b = rtamd.SceneBuilder(seed=1)
    white, red = _world(b)
    b.add(b.box((-40, -43, -43), (40, -3, 37), white))
    b.add(_fog(b, 60.0))
    _camera(b)
    return b.finish(W, H)


def sphere_sphere():
    """(c) two shells around everything: a glass sphere (r 50) inside an emitting one (r 60)."""
    b = rtamd.SceneBuilder(seed=1)
    white, red = _world(b)
    b.add(b.sphere((0, 0, -3), 50.0, b.dielectric(1.5)))
    b.add(b.sphere((0, 0, -3), 60.0, b.diffuse_light(0.6, 0.7, 0.9)))
    _camera(b)
    return b.finish(W, H)


def quad_medium():
    """(d) a huge ground quad (200 x 200) and the fog (r 150)."""
    b = rtamd.SceneBuilder(seed=1)
    white, red = _world(b, room=False)
    b.add(b.quad((-100, -2, -103), (200, 0, 0), (0, 0, 200), white))
    b.add(_fog(b, 150.0, 0.01))
    _camera(b)
    return b.finish(W, H)


def two_media():
    """(f) the fog in the first leaf and a ball of smoke later in the order: the fog draws each walk's
    first rnd(), the smoke a later one."""
    b = rtamd.SceneBuilder(seed=1)
    white, red = _world(b)
    smoke = b.sphere((0.5, 0.75, -4), 1.0, b.dielectric(1.5))
    b.add(b.constant_medium(smoke, 0.8, b.isotropic(b.solid(0.1, 0.1, 0.1))))
    b.add(b.box((-40, -43, -43), (40, -3, 37), white))
    b.add(_fog(b, 60.0, 0.03))
    _camera(b)
    return b.finish(W, H)


def _singleton(scene, slot):
    """The scene with its right-most leaf made a singleton of its slot `slot` model (both ids the same,
    as the builder writes a span of one): the other model leaves the tree."""
    raw = np.frombuffer(scene.buffers[1], np.uint8).reshape(-1, 32).copy()
    ids = raw[:, 24:].view(np.int32)
    k = 0
    while ids[k, 0] & 0xFFFF == 0:   # an inner node: to its right child
        k = (ids[k, 1] >> 16) & 0xFFFF
    ids[k, 1 - slot] = ids[k, slot]
    scene.buffers[1] = raw.tobytes()
    return scene


def singleton_sphere():
    """(b) the first leaf a singleton solid: the outer shell alone."""
    return _singleton(sphere_sphere(), 1)


def singleton_medium():
    """(b) the first leaf a singleton medium, tested twice (two rnd() draws): the fog alone."""
    return _singleton(box_medium(), 1)


CUSTOM = {"box_medium": (box_medium, (BOX, MEDIUM)), "sphere_sphere": (sphere_sphere, (SPHERE, SPHERE)),
          "quad_medium": (quad_medium, (QUAD, MEDIUM)), "two_media": (two_media, (BOX, MEDIUM)),
          "singleton_sphere": (singleton_sphere, (SPHERE, 0)), "singleton_medium": (singleton_medium, (MEDIUM, MEDIUM))}


@pytest.mark.parametrize("name", list(CUSTOM))
def test_custom_first_leaf_on_off_oracle(gpu, name):
    make, types = CUSTOM[name]
    scene = make()
    info, fl = on_off_oracle(scene, FRAMES, types=types)


def test_origins_outside_the_spine_margin(gpu):
    """(e) adversarial.spine: the camera 0.0005 inside the spine box's face, so the host arms the
    prologue but the camera rays, closer to the face than their margin, start at the root; the walks
    after a scatter start on either side of it."""
    scene = spine(0.0005)
    info, fl = on_off_oracle(scene, 3, depth=4, uniforms=EXACT, types=None)
    assert fl["types"] & 0x70 == MEDIUM << 4, fl


def test_leaf_alone_ends_the_walk(gpu):
    """(g) a scene of one leaf (box, medium): its skip link ends the walk, so the prologue's lanes are
    done before the first round.  The chain is the root alone (spine 1); the scene plans the 512-thread
    compact-box kernel (box_interior 1), which holds the prologue."""
    b = rtamd.SceneBuilder(seed=1)
    white = b.lambertian(b.solid(0.73, 0.73, 0.73))
    b.add(b.box((-2, -2, -8), (2, -1, -3), white))
    b.add(_fog(b, 30.0, 0.05))
    _camera(b)
    scene = b.finish(W, H)
    info, fl = on_off_oracle(scene, FRAMES, types=(BOX, MEDIUM))
    assert info["spine"] == 1 and info["lds_nodes"] == 1 and info["block"] == 512, info


def test_negative_zero_direction(gpu):
    """Camera rays in the plane y = 0 with jitter (spp 1 uniforms): d.y = -0 (pixel_delta_u/v.y = -0)
    * (a positive sub-pixel offset) summed with -0 terms, so about a quarter of the lanes have
    1 / d.y = -inf and their waves take the exact walk form after the prologue."""
    scene = box_medium()
    nz = np.float32(-0.0)
    scene.override_camera(grid_camera((0.5, 0.0, 2.0), (0.5 - 1.5, nz, 2.0 - 1.0), (1 / 16, nz, 0), (0, nz, -1 / 16)))
    info, fl = on_off_oracle(scene, FRAMES, uniforms=rtamd.spp_uniforms(1), types=(BOX, MEDIUM))


@pytest.mark.parametrize("depth", [1, 2])
def test_shallow_depth(gpu, depth):
    """A path that ends in the pass that began its walk."""
    scene, ref = scene8(64, 36, 4)
    info, fl = on_off_oracle(scene, 4, depth=depth, types=(BOX, MEDIUM))

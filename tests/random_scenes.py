"""Seeded random scenes over rtamd.SceneBuilder (test infrastructure; a plain module, no device).

tests/kernel_matrix.py reaches most render_persistent instances by switching options off on scene 8 or
scene 0, tests/adversarial.py aims a dozen hand-built scenes at one shortcut each.  The scenes here reach
their instance because of what they contain: 1 to 2500 prims (one-, two- and three-prim trees, the 64- and
1024-node walk_frac steps, tables that outgrow LDS), at a spread of 4 and of 300000 units (the extent on
both sides of 2^20, where the planner drops the shared-reciprocal division itself), with or without a
scene-8-style enclosing fog (a spine and an armed first leaf on trees that are not scene 8's).

scene(family, n, seed, scale, fog) is deterministic from its arguments.  The n prims sit in the cube
[-scale, scale]^3 around (0, 0, -3 scale), each about scale / n^(1/3) across, the camera at the origin looks at
the cube's centre; 29x21 is 4x3 tiles whose right column is 5 pixels wide and whose bottom row is 5 high.
The first prims of a scene are its registered lights (quads and spheres, never a medium): none, one or three,
drawn with the scene; the first is a quad over the cube, or, where the background is black, a larger one
behind the cube that faces the camera.  A scene without a light has a bright background, so every image
carries radiance (tests/test_random_scenes.py asserts it).  The light quads are tilted: an axis-aligned quad's
bounding box, padded by 0.0005, has no thickness left in float32 at a spread of 300000, and the reference's
slab test never enters such a box.  Defocus is on in about half the scenes.

SCENES is the fixed list the tests run (tests/test_random_scenes.py on the host, tests/test_gpu_random_scenes.py
on the device), grouped by family and ordered from the smallest n up.
"""
import functools

import numpy as np

from rtamd.scene import SceneBuilder

F32 = np.float32
W, H = 29, 21
TX, TY = 4, 3
NT = TX * TY
LAUNCH, FRAMES, DEPTH = 3, 6, 5            # two launches of LAUNCH frames, spp FRAMES
MASK = [0, 3, 8, 11]                       # both corners' tiles, a right-edge tile (3), a bottom-edge tile (8)
REST = [t for t in range(NT) if t not in MASK]
FOG_RADIUS = 5000.0                        # scene 8's enclosing medium: the camera sits inside

FAMILIES = ("spheres", "textured", "quads", "boxes", "boxes_spheres", "rotated", "media", "mixed")
MIXED = ("media", "mixed")                 # the families whose leaves hold spheres, quads, boxes and media
SIZES = (1, 2, 3, 9, 40, 200, 1000, 2500)
SCALES = (4.0, 300000.0)
FEATURES_MAX_N = 200                       # the first-hit comparison's brute force stays cheap up to here

# what a family draws its prims from
KINDS = {
    "spheres": ("sphere",),
    "textured": ("sphere", "moving"),
    "quads": ("quad",),
    "boxes": ("box",),
    "boxes_spheres": ("box", "sphere"),
    "rotated": ("rotated", "box"),
    "media": ("fog_sphere", "fog_box", "sphere", "quad", "box", "fog_rotated"),
    "mixed": ("sphere", "moving", "quad", "box", "rotated", "fog_sphere", "fog_box"),
}
TEXTURED = ("textured", "media", "mixed")  # checker, Perlin and image textures beside the solid ones


def _v(a):
    return tuple(float(x) for x in np.asarray(a, F32))


class _Palette:
    """The scene's shared materials: all five kinds; in the textured families every texture type on
    lambertian, metal and isotropic."""

    def __init__(self, b, rng, textured):
        col = lambda: _v(rng.uniform(0.15, 0.95, 3))  # noqa: E731
        tex = [b.solid(*col()) for _ in range(3)]
        if textured:
            tex += [b.checker(col(), col(), float(rng.uniform(0.2, 3.0))), b.perlin(float(rng.uniform(0.5, 6.0))),
                    b.image("earthmap.jpg", int(rng.integers(0, 64)), int(rng.integers(0, 64)))]
        self.surface = []
        for t in tex:
            self.surface.append(b.lambertian(t))
            self.surface.append(b.metal(t, float(rng.uniform(0.0, 0.9))))
        self.surface.append(b.dielectric(1.5))
        self.surface.append(b.dielectric(float(rng.uniform(1.0, 2.5))))
        self.surface.append(b.diffuse_light(*_v(rng.uniform(0.5, 3.0, 3))))   # emits, is not registered
        self.phase = [b.isotropic(t) for t in tex]
        self.light = b.diffuse_light(*_v(rng.uniform(3.0, 7.0, 3)))

    def any(self, rng):
        return self.surface[int(rng.integers(len(self.surface)))]

    def any_phase(self, rng):
        return self.phase[int(rng.integers(len(self.phase)))]


def _prim(b, kind, rng, pal, c, r, prev_fog, have_fog):
    """One prim of `kind` about r across around c; a medium every other time overlaps the one before."""
    if kind == "sphere":
        return b.sphere(_v(c), float(r), pal.any(rng))
    if kind == "moving":
        return b.sphere(_v(c), float(r), pal.any(rng), center2=_v(c + rng.uniform(-1, 1, 3) * r))
    if kind == "quad":
        u, v = rng.uniform(-1, 1, 3) * 2 * r, rng.uniform(-1, 1, 3) * 2 * r
        return b.quad(_v(c - (u + v) / 2), _v(u), _v(v), pal.any(rng))
    h = rng.uniform(0.4, 1.0, 3) * r
    if kind == "box":
        return b.box(_v(c - h), _v(c + h), pal.any(rng))
    if kind == "rotated":
        return b.box((0, 0, 0), _v(2 * h), pal.any(rng), translation=_v(c - h),
                     rotation=(0, float(F32(rng.uniform(-1.5, 1.5))), 0))
    # media: a boundary twice the size, a density that scatters within it about every other time
    if have_fog and rng.integers(2):
        c = prev_fog + rng.uniform(-1, 1, 3) * r
    glass = pal.surface[-3]
    if kind == "fog_sphere":
        bound = b.sphere(_v(c), float(2 * r), glass)
    elif kind == "fog_box":
        bound = b.box(_v(c - 2 * h), _v(c + 2 * h), glass)
    else:
        bound = b.box((0, 0, 0), _v(4 * h), glass, translation=_v(c - 2 * h),
                      rotation=(0, float(F32(rng.uniform(-1.5, 1.5))), 0))
    prev_fog[:] = c
    return b.constant_medium(bound, float(rng.uniform(0.1, 1.0) / r), pal.any_phase(rng))


def scene(family, n, seed, scale=4.0, fog=False, W=W, H=H):
    """The rtamd.Scene of n prims of a family (plus the enclosing fog, added last, when fog is set)."""
    rng = np.random.default_rng(seed)
    s = float(scale)
    centre = np.array([0.0, 0.0, -3.0 * s])
    b = SceneBuilder(seed=1)
    pal = _Palette(b, rng, family in TEXTURED)
    kinds = KINDS[family]
    n_lights = (0, 1, 3)[int(rng.integers(3))]
    n_lights = min(n_lights, n - 1)                        # at least one prim is the family's own
    dark = n_lights > 0 and bool(rng.integers(2))          # a black background: the light is all there is
    defocus = bool(rng.integers(2))
    size = 0.45 * s / n ** (1.0 / 3.0)
    prev_fog = np.zeros(3)
    fogs = 0
    for k in range(n):
        c = centre + rng.uniform(-1, 1, 3) * s
        r = size * rng.uniform(0.5, 1.2)
        if k == 0 and n_lights and dark:   # the light behind the cube, facing the camera: most pixels see it or a prim
            m = b.add(b.quad(_v(centre + [-2.5 * s, -2.5 * s, -1.3 * s]), (5 * s, 0, 0), (0, 5 * s, 0.5 * s), pal.light))
            b.add_light(m)
        elif k == 0 and n_lights:        # the light over the cube, facing down
            m = b.add(b.quad(_v(centre + [-s, 1.25 * s, -s]), (2 * s, 0, 0), (0, 0.2 * s, 2 * s), pal.light))
            b.add_light(m)
        elif k < n_lights:
            c[1] = centre[1] + rng.uniform(0.6, 1.1) * s
            if k == 1:
                m = b.add(b.sphere(_v(c), float(r), pal.light))
            else:
                m = b.add(b.quad(_v(c), _v([2 * r, 0, 0]), _v([0, 0.3 * r, 2 * r]), pal.light))
            b.add_light(m)
        else:
            kind = kinds[(k + seed) % len(kinds)] if n < 9 else kinds[int(rng.integers(len(kinds)))]
            b.add(_prim(b, kind, rng, pal, c, r, prev_fog, fogs > 0))
            fogs += kind.startswith("fog")
    if fog:
        bound = b.sphere((0, 0, 0), FOG_RADIUS, pal.surface[-3])
        b.add(b.constant_medium(bound, 0.0001, b.isotropic(b.solid(1, 1, 1))))
    b.camera(look_from=(0, 0, 0), look_at=_v(centre), vfov=50.0, defocus_angle=0.8 if defocus else 0.0,
             focus_dist=3.0 * s, background=(0, 0, 0) if dark else _v(rng.uniform(0.3, 0.9, 3)))
    return b.finish(W, H)


def _scenes():
    out = []
    for fi, family in enumerate(FAMILIES):
        rows = []
        for ni, n in enumerate(SIZES):
            for si, scale in enumerate(SCALES):
                rows.append((family, n, 100 * fi + 10 * ni + si + 1, scale, False))
        for ni, n in enumerate((3, 40, 200)):   # and under the enclosing fog
            rows.append((family, n, 100 * fi + 90 + ni, SCALES[ni % 2], True))
        out += sorted(rows, key=lambda r: (r[1], r[3], r[4]))
    return out


# (a seed whose scene had a tied first hit or too dark an image would be replaced here; none of these has)
SCENES = _scenes()


def by_family():
    """{family: [(index into SCENES, arguments)]}, each from the smallest n up."""
    out = {f: [] for f in FAMILIES}
    for i, a in enumerate(SCENES):
        out[a[0]].append((i, a))
    return out


@functools.lru_cache(maxsize=None)
def built(index):
    """SCENES[index], built once per process."""
    return scene(*SCENES[index])


@functools.lru_cache(maxsize=None)
def oracle(index):
    """(image, counters) of SCENES[index] on the CPU oracle: FRAMES frames at depth DEPTH, spp FRAMES; computed
    once per process and never written to."""
    import pyoracle
    import rtamd
    o = pyoracle.OracleScene(built(index), max_depth=DEPTH, spp=FRAMES)
    img, counters = pyoracle.render(o, rtamd.frame_rand_factors(1, 0, FRAMES), counters=True)
    img.setflags(write=False)
    return img, counters


# the unmasked (block, opt) instances the scenes reach at default options on 4096 resident waves
# (tests/test_random_scenes.py holds the list to this set, exactly)
REACHED = {(512, 11), (512, 15), (512, 43), (512, 47), (512, 75), (512, 79), (512, 143), (512, 207), (512, 431),
           (1024, 11), (1024, 15), (1024, 43), (1024, 47), (1024, 59), (1024, 63), (1024, 75), (1024, 79),
           (1024, 143), (1024, 431)}

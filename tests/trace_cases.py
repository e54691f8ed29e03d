"""The scenes and row sets of the closest-hit walk's tests, in the manner of tests/shade_cases.py:
tests/test_trace_ref64.py (CPU: the oracle's RT_SOP_TRACE against the float64 walk of tests/ref64_trace.py),
tests/test_gpu_trace_op.py (the device's plain walk against the oracle, word for word) and the path replays
(tests/test_path_replay.py, tests/test_gpu_path_replay.py).

Scenes: shade_cases' four (a moving sphere, media, five lights, a defocus disk) and `knot`, a small scene of
stations along x, every coordinate a binary fraction, so that the edge rays below have float64 bound 0 up to
a medium's logarithm: two pairs of overlapping spheres that the ray through their middle meets at one t, two
coplanar quads abutting along an edge, a sphere-bounded fog around a solid sphere with a quad behind it, a
box-bounded fog with a quad in front of it, a box turned about y, a moving sphere, a quad light; both big fogs
and a small one sit alone in their leaves (knot() says how the builder is led to that).
Rows are rt_debug_eval_shade_op rows (pyoracle.shade_rows): o, d, time, px, py, rf and the uv source before
the walk.  hit_sphere accepts tmin < t < tmax and hit_quad tmin <= t <= tmax (interval.glsl), so of two spheres
at one t the first visited stays and of two quads at one t the second replaces it.
"""
import os

import numpy as np

import adversarial
import pyoracle
import shade_cases
from pyoracle import SOP_PX, SOP_PY, SOP_RF, shade_rows
from rtamd.scene import SceneBuilder
from shade_cases import Batch, _seeds, _with_seeds, found, records

F32 = np.float32
N_DRAWS = 64      # draws handed to the float64 walk per row: one per medium test, two media tests per leaf at most
SPHERE, QUAD, MEDIUM, BOX = 1, 2, 3, 4
NODE_DT = np.dtype([("box", "<f4", 6), ("left", "<i4"), ("right", "<i4")])


# ------------------------------------------------------------------------------------------------ scenes
def knot():
    """19 prims whose x-mins descend in the order of the comments' ranks: the builder halves the sorted list, so the
    leaves are (0, 1) (2, 3) (4, 5) (6) (7, 8) (9, 10) (11) (12, 13) (14, 15) (16) (17, 18), reached from the last to the
    first, the left (lower-rank) slot of a leaf tested first; edge_sets() asserts what it relies on."""
    b = SceneBuilder(seed=1)
    white = b.lambertian(b.solid(0.75, 0.75, 0.75))
    red = b.lambertian(b.solid(0.75, 0.25, 0.25))
    iso = b.isotropic(b.solid(0.5, 0.75, 0.5))
    glow = b.diffuse_light(4, 4, 4)
    # the sphere fog's colour is an image's, read at hit_record.uv: a medium writes none, so it is whatever the last
    # sphere or quad hit left, in this walk or in an earlier bounce's (the render depends on the hand-over)
    iso_img = b.isotropic(b.image(os.path.join(adversarial.GOLD, "tex_rgba.png"), 0, 0))
    b.add(b.sphere((7, 0, 0), 1.25, white))                                    # sphere 0, 1: the pair at x = 8 (ranks 8, 7)
    b.add(b.sphere((9, 0, 0), 1.25, red))
    b.add(b.sphere((25, 0, 0), 1.25, white))                                   # sphere 2, 3: the pair at x = 24 (ranks 4, 5)
    b.add(b.sphere((23, 0, 0), 1.25, red))
    b.add(b.quad((30, -1, 0), (2, 0, 0), (0, 2, 0), white))                    # quad 0, 1: abutting along x = 32 (ranks 3, 2)
    b.add(b.quad((32, -1, 0), (2, 0, 0), (0, 2, 0), red))
    b.add(b.constant_medium(b.sphere((-16, 0, 0), 2.0, white), 2.0, iso_img))  # medium 0, boundary sphere 4 (rank 11, alone)
    b.add(b.sphere((-17.5, 0, -1), 1.0, b.metal(b.solid(0.75, 0.75, 0.75), 0.25)))   # sphere 5, inside the fog (rank 12)
    b.add(b.quad((-19, -2, -3), (6, 0, 0), (0, 4, 0), red))                    # quad 2: behind the sphere fog (rank 13)
    b.add(b.constant_medium(b.box((-34, -1, -1), (-30, 1, 1), white), 1.0, iso))   # medium 1, boundary box 0 (rank 16, alone)
    b.add(b.quad((-36, -0.5, 2), (4, 0, 0), (0, 1, 0), white))                 # quad 3: in front of the box fog (rank 17)
    b.add(b.sphere((-40, 0, 0), 1.0, white))                                   # sphere 6 (rank 18)
    b.add(b.box((0, 0, 0), (2, 2, 2), white, translation=(40, -1, -1), rotation=(0, 0.5, 0)))   # box 1, turned (rank 0)
    b.add(b.sphere((37, 0, 0), 0.5, b.dielectric(1.5), center2=(37, 1, 0)))    # sphere 7, moving (rank 1)
    b.add(b.constant_medium(b.sphere((16, 0, 0), 1.0, white), 4.0, iso))       # medium 2, boundary sphere 8 (rank 6, alone)
    b.add_light(b.add(b.quad((-2, 6, -2), (4, 0, 0), (0, 0, 4), glow)))        # quad 4, the light (rank 9)
    b.add(b.sphere((-4, 0, 0), 0.5, red))                                      # sphere 9 (rank 10)
    b.add(b.sphere((-26, 0, 0), 1.0, red))                                     # sphere 10 (rank 15)
    b.add(b.quad((-24, -1, -1), (2, 0, 0), (0, 2, 0), white))                  # quad 5 (rank 14)
    b.camera(look_from=(-16, 1, 12), look_at=(-16, 0, 0), vfov=60, background=(0.5, 0.625, 0.75))   # at the sphere fog
    return b.finish(16, 12)


SCENES = dict(shade_cases.SCENES, knot=(knot, (2.0, 0.5)))
_scenes = {}


def scene(name):
    """(the rtamd Scene, (sqrt_spp, recip_sqrt_spp)), built once; shade_cases' scenes are its own objects."""
    if name in shade_cases.SCENES:
        return shade_cases.scene(name)
    if name not in _scenes:
        _scenes[name] = (SCENES[name][0](), SCENES[name][1])
    return _scenes[name]


def nodes(sc):
    return np.frombuffer(bytes(sc.buffers[1]), NODE_DT)


def leaf_order(sc):
    """The leaves in the order every walk reaches them (compute.glsl:236-261: the right child is popped
    first): [(node, (type, index) of the left slot, of the right slot)]."""
    nd = nodes(sc)
    out, stack = [], [0]
    while stack:
        i = stack.pop()
        l, r = int(nd["left"][i]), int(nd["right"][i])
        if l & 0xFFFF:
            out.append((i, (l & 0xFFFF, (l >> 16) & 0xFFFF), (r & 0xFFFF, (r >> 16) & 0xFFFF)))
        else:
            stack += [(l >> 16) & 0xFFFF, (r >> 16) & 0xFFFF]
    return out


def slot_rank(sc):
    """(type, index) -> position of the prim's first test in a walk that reaches every leaf."""
    rank = {}
    for k, (_, a, b) in enumerate(leaf_order(sc)):
        rank.setdefault(a, 2 * k)
        rank.setdefault(b, 2 * k + 1)
    return rank


def leaf_of(sc, prim):
    return [n for n, a, b in leaf_order(sc) if prim in (a, b)][0]


# -------------------------------------------------------------------------------------------------- rows
def _uv_sources(sc, rng, n):
    """A uv source before the walk per row: none, a sphere's point, a quad's (alpha, beta) with a stale c."""
    n_sph = len(records(sc)[0])
    kind = rng.integers(0, 3, n)
    uvk = np.where(kind == 1, 1 << 16 | rng.integers(0, max(n_sph, 1), n), np.where(kind == 2, 2 << 16, 0)).astype(np.int32)
    uv = rng.uniform(-2, 2, (n, 3)).astype(F32)
    uv[kind == 0] = 0
    return uvk, uv


def random_rows(name, n, seed):
    """Seeded rays from inside the scene's bounds, at times in [0, 1): a third aimed at a prim's bounds."""
    sc = scene(name)[0]
    rng = np.random.default_rng(seed)
    nd = nodes(sc)
    root = nd["box"][0].astype(np.float64)
    lo, hi = np.clip(root[0::2], -64, 64), np.clip(root[1::2], -64, 64)
    pad = 0.25 * (hi - lo) + 1.0
    o = rng.uniform(lo - pad, hi + pad, (n, 3))
    d = rng.normal(size=(n, 3)) * np.exp2(rng.integers(-2, 3, (n, 1)))
    leaves = [i for i, _, _ in leaf_order(sc)]
    aim = rng.random(n) < 0.34
    lb = nd["box"][rng.choice(leaves, n)].astype(np.float64)
    tgt = rng.uniform(np.clip(lb[:, 0::2], -64, 64), np.clip(lb[:, 1::2], -64, 64))
    d = np.where(aim[:, None], (tgt - o) * rng.uniform(0.25, 2, (n, 1)), d)
    px, py, rf = _seeds(rng, n)
    uvk, uv = _uv_sources(sc, rng, n)
    return shade_rows(n, o=o, d=d, time=rng.random(n).astype(F32), px=px, py=py, rf=rf, uvk=uvk, uv=uv)


def _ray(o, d, time=0.0, px=3, py=5, rf=0.25, uvk=0, uv=(0, 0, 0)):
    return shade_rows(1, o=[o], d=[d], time=time, px=px, py=py, rf=rf, uvk=uvk, uv=[uv])


def _first_draw_hits(sc, row):
    """Seeds (px, py, rf) under which the oracle's walk of `row` ends in a medium."""
    osc = pyoracle.OracleScene(sc)
    rng = np.random.default_rng(7)
    px, py, rf = _seeds(rng, 64)
    rows = np.repeat(row, 64, axis=0)
    rows[:, SOP_PX], rows[:, SOP_PY], rows[:, SOP_RF] = px, py, rf
    w = pyoracle.eval_shade_op(osc, "trace", rows)
    k = np.nonzero((w[:, 0] != 0) & ((w[:, 2] & 0xF) == MEDIUM))[0]
    assert k.size, "no seed of 64 scatters in the medium"
    return rows[k[:4]]


def edge_sets():
    """name -> rows on `knot`; tests/test_trace_ref64.py's EXPECT says what each set must give whoever computes it."""
    sc = scene("knot")[0]
    rank = slot_rank(sc)
    nd = nodes(sc)
    down = (0, 0, -1)
    sets = {}
    # an exact tie at t = 3.25: of two spheres the first visited stays; one pair is visited lower index first, one higher
    assert rank[SPHERE, 1] + 1 == rank[SPHERE, 0] and rank[SPHERE, 2] + 1 == rank[SPHERE, 3]
    sets["tie_spheres"] = np.concatenate([_ray((8, 0, 4), down), _ray((24, 0, 4), down)])
    # ... of two quads (t <= ray_t.max) the second replaces it: the shared edge x = 32, alpha 0 of one and 1 of the other
    assert rank[QUAD, 1] + 1 == rank[QUAD, 0]
    sets["tie_quads"] = np.concatenate([_ray((32, 0, 4), down), _ray((32, 0.5, 2), (0, 0, -0.5))])
    # a quad's plane exactly at tmin = 0.001 (accepted: tmin <= t), one ulp nearer (passed through) and farther
    z = F32(0.001)
    sets["tmin"] = np.concatenate([_ray((31, 0, zz), down) for zz in (z, np.nextafter(z, F32(0)), np.nextafter(z, F32(1)))]
                                  + [_ray((31, 0, -zz), (0, 0, 1)) for zz in (z, np.nextafter(z, F32(0)))])
    # an origin on a slab plane of the first pair's leaf (y = 1.25, x = 5.75) and of the root (its zmax), with that
    # direction component +0 and -0: 0 * inf
    pair = leaf_of(sc, (SPHERE, 0))
    assert pair == leaf_of(sc, (SPHERE, 1)) and nd["box"][pair][3] == 1.25 and nd["box"][pair][0] == 5.75
    zmax = float(nd["box"][0][5])
    sets["slab_plane"] = np.concatenate([_ray((8.25, 1.25, 4), (0.0625, s, -1)) for s in (0.0, -0.0)]
                                        + [_ray((8.25, 0.5, zmax), (0.0625, -0.125, s)) for s in (0.0, -0.0)]
                                        + [_ray((5.75, 0.5, 4), (s, 0.125, -1)) for s in (0.0, -0.0)])
    # ... where the sign of the zero decides the walk: y = 2 is the top of quad 2 and of its leaf's box, a ray in that
    # plane meets the quad's edge (beta 1).  With +0 the far slab value is NaN and the near one -inf, so hit_aabb's
    # else branch lowers ray_t.max to -inf and the leaf is missed; with -0 the near one is +inf, nothing moves, and
    # the quad is hit
    behind = leaf_of(sc, (QUAD, 2))
    assert nd["box"][behind][3] == 2.0 and nd["box"][behind][2] == -2.0
    sets["slab_sign"] = np.concatenate([_ray((-14, 2, 4), (0.0625, s, -1)) for s in (0.0, -0.0)])
    # a reciprocal of -inf on each axis, on rays that go on to hit something
    sets["recip_minus_inf"] = np.concatenate([_ray((7.5, 0.25, 4), (-0.0, 0, -1)), _ray((24.5, 0.25, 4), (0.125, -0.0, -1)),
                                              _ray((4, 0.25, -0.0), (1, 0, -0.0)), _ray((31, 0.5, 3), (-0.0, -0.0, -2)),
                                              _ray((-16, 0.5, 4), (-0.0, 0, -1), px=9)])
    # d = 0: outside everything, inside the sphere fog, inside the box fog, inside a solid sphere, on a quad
    sets["zero_dir"] = np.concatenate([_ray(o, (0, s, 0), rf=0.5) for o in ((50, 9, 9), (-16.5, 0.5, 1), (-32, 0.25, 0.5),
                                                                            (7, 0, 0), (31, 0, 0)) for s in (0.0, -0.0)])
    # the stale uv: quad 2 (behind the sphere fog) is accepted, then the fog, visited later, scatters nearer; and a
    # sphere's uv point kept the same way (the solid sphere 5 inside the fog).  The fog is alone in its leaf, so a
    # first test that does not scatter is followed by a second one that draws again
    assert rank[QUAD, 2] < rank[MEDIUM, 0] and rank[SPHERE, 5] < rank[MEDIUM, 0], "the fog is visited before what is behind it"
    sets["stale_uv"] = np.concatenate([_first_draw_hits(sc, _ray((-15, 0.5, 4), down, uvk=1 << 16 | 6, uv=(1, 2, 3))),
                                       _first_draw_hits(sc, _ray((-17.5, 0.25, 4), down, uvk=2 << 16, uv=(0.5, 0.25, 7)))])
    # a shrunken ray_t.max prunes a medium's box: quad 3 at t = 2 in front of the box fog, whose leaf comes later
    fog_leaf = leaf_of(sc, (MEDIUM, 1))
    assert rank[QUAD, 3] < rank[MEDIUM, 1] and fog_leaf != leaf_of(sc, (QUAD, 3)) and nd["box"][fog_leaf][5] <= 1.0
    sets["pruned_medium"] = np.concatenate([_ray((-33, 0, 4), down, rf=r) for r in (0.25, 1.5, 3.0)])
    # a medium draw that is exactly 0: log(0) = -inf, the distance +inf, no scatter
    through = np.concatenate([_ray((-15, 0.5, 4), down), _ray((-31, 0.25, 4), down), _ray((16, 0.25, 4), down)])
    sets["zero_draw"] = _with_seeds(through, found("zero_draw"))
    return sets


def singleton_media(sc):
    """The media that sit alone in a leaf (both slots name them)."""
    return [a[1] for _, a, b in leaf_order(sc) if a == b and a[0] == MEDIUM]


def device_only_rows():
    """NaN and inf in o and d (outside float64's scope): the device against the oracle only."""
    nan, inf = F32(np.nan), F32(np.inf)
    rows = []
    for v in (nan, inf, -inf):
        for k in range(3):
            o, d = [8.0, 0.25, 4.0], [0.0, 0.0, -1.0]
            o[k] = v
            rows.append(_ray(o, d))
            o, d = [-15.0, 0.5, 4.0], [0.0, 0.0, -1.0]
            d[k] = v
            rows.append(_ray(o, d, px=7 + k))
    rows.append(_ray((nan, nan, nan), (nan, nan, nan)))
    rows.append(_ray((8, 0, 4), (0, 0, -3.0e38)))
    rows.append(_ray((8, 0, 3.0e38), (0, 0, -1)))
    rows.append(_ray((8, 0, 4), (0, 0, -1e-30)))
    return np.concatenate(rows)


RANDOM_N = {"zoo0": 2048, "zoo1": 2048, "five": 2048, "inside": 2048, "knot": 4096}
_batches = None


def batches():
    """Every batch, built once, each within the hook's input guard and padded to whole waves by the hook."""
    global _batches
    if _batches is None:
        out = [Batch("trace", f"random_{name}", "random", name, random_rows(name, n, 100 + k))
               for k, (name, n) in enumerate(RANDOM_N.items())]
        # (an origin on a slab plane with a zero direction component: 0 * inf, outside float64's scope like NaN itself)
        out += [Batch("trace", name, "device" if name.startswith("slab_") else "edge", "knot", rows)
                for name, rows in edge_sets().items()]
        out.append(Batch("trace", "nan_inf", "device", "knot", device_only_rows()))
        for b in out:
            r = b.rows
            assert ((r[:, SOP_PX] >= 0) & (r[:, SOP_PX] < 16384) & (r[:, SOP_PY] >= 0) & (r[:, SOP_PY] < 16384)
                    & (r[:, SOP_RF] >= 0) & (r[:, SOP_RF] < 4096)).all(), b
        _batches = out
    return _batches

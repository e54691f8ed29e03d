"""The row sets of tests/test_shade_ref64.py (CPU: oracle against float64) and tests/test_gpu_shade_ops.py
(device against oracle, word for word), in the manner of tests/ops_cases.py: per operation of
rt_debug_eval_shade_op a seeded random set and edge sets, each on one of the scenes below.

Edges in the geometry are built from binary fractions, so the float64 bound is 0 up to the first
built-in.  Edges in a draw were found by a seeded search over (px, py, rf) candidates of _seeds()'
distribution (seed SEARCH_SEED; rand() restated in numpy, 2^20 candidates, each hit confirmed with the
oracle's rand_sequence on the CPU).  The found rows are fixed in FOUND below; found() only checks that
they still meet their targets, so a change of the oracle's rand or sine fails loudly.  rand()'s values
are coarse (multiples of about 2^-8 over most of its range), so a draw "below 2^-16" is exactly 0 and
about one draw in 400 is exactly 0.5.

Every set satisfies the hook's input guard (px, py in [0, 16384), rf in [0, 4096), all finite): batches()
asserts it.  The oracle loops on the same draws as the device, so a set the CPU tests have run is a set
whose rejection loops end.
"""
import os

import numpy as np

import adversarial
import pyoracle
from pyoracle import SOP_PX, SOP_PY, SOP_RF, shade_rows
from rtamd.scene import SceneBuilder

F32 = np.float32
N_DRAWS = 96      # draws handed to the float64 reference per row (a row that needs more is out of its scope)
SEARCH_SEED = 20


class Batch:
    def __init__(self, op, name, kind, scene, rows):
        self.op, self.name, self.kind, self.scene, self.rows = op, name, kind, scene, np.ascontiguousarray(rows, F32)
        assert kind in ("random", "edge", "device") and len(self.rows) <= 2 ** 14

    def __repr__(self):
        return f"<{self.op}/{self.name} on {self.scene}: {len(self.rows)} rows>"


# ------------------------------------------------------------------------------------------------ scenes
def zoo(lights):
    """Every material on a sphere, a quad and a medium, and all but the fuzz-0 metal on a box (metal and
    dielectric with several parameter words on spheres and quads), solid textures on the rows that are
    compared by value; a checker, a Perlin and an image texture on three more quads.  lights 0:
    no registered light (the diffuse-light prims emit but are not sampled); 1: one quad light and a
    defocus disk."""
    b = SceneBuilder(seed=1)
    sol = b.solid(0.5, 0.25, 0.75)
    lam, iso = b.lambertian(sol), b.isotropic(b.solid(0.75, 0.75, 0.5))
    m0, m1, m3 = b.metal(sol, 0.0), b.metal(sol, 0.99999), b.metal(sol, 0.3)
    d0, d1, d15 = b.dielectric(1.0), b.dielectric(2.5), b.dielectric(1.5)
    glow = b.diffuse_light(4, 2, 1)
    for i, m in enumerate((lam, m0, m1, m3, d0, d1, d15, glow, iso)):
        b.add(b.sphere((3 * i - 10, 0, -10), 1.0, m))
    b.add(b.sphere((-10, 4, -10), 0.5, lam, center2=(-10, 5, -10)))      # moving
    for i, m in enumerate((lam, m0, m1, d15, glow, iso)):
        b.add(b.quad((3 * i - 6, -3, -14), (2, 0, 0), (0, 2, 0), m))
    for i, m in enumerate((lam, m3, d15, glow, iso)):
        b.add(b.box((4 * i - 8, -8, -12), (4 * i - 6, -6, -10), m))
    for i, m in enumerate((iso, lam, m3, d15, glow)):   # set_material_properties takes any material for a medium
        b.add(b.constant_medium(b.sphere((4 * i - 8, 5, -10), 1.5, d15), 0.5, m))
    gold = os.path.join(adversarial.GOLD, "tex_rgba.png")
    for i, t in enumerate((b.checker((0.1, 0.2, 0.1), (0.9, 0.9, 0.9), 0.5), b.perlin(4.0), b.image(gold, 0, 0))):
        b.add(b.quad((3 * i - 4, 8, -14), (2, 0, 0), (0, 2, 0), b.lambertian(t)))
    if lights:
        b.add_light(b.add(b.quad((-2, 12, -12), (4, 0, 0), (0, 0, 4), glow)))
    b.camera(look_from=(0, 1, 4), look_at=(0, 0, -10), vfov=50, defocus_angle=2.0 if lights else 0.0, focus_dist=14.0,
             background=(0.25, 0.5, 0.75))
    sc = b.finish(64, 48)
    # fuzz 1: the builder takes fuzz below 1 only, so the word 65535 is written into the records of the
    # sphere and the quad it gave the largest fuzz
    for bind, width, col in ((0, 12, 11), (2, 20, 7)):
        rec = np.frombuffer(sc.buffers[bind], np.int32).reshape(-1, width).copy()
        metal = [i for i in range(len(rec)) if (rec[i, col] >> 16) & 0xFFFF == 1]
        top = max(metal, key=lambda i: rec[i, col] & 0xFFFF)
        rec[top, col] = 1 << 16 | 65535
        sc.buffers[bind] = rec.tobytes()
    return sc


# name -> (builder, (sqrt_spp, recip_sqrt_spp))
SCENES = {"zoo0": (lambda: zoo(0), (1.0, 1.0)), "zoo1": (lambda: zoo(1), (4.0, 0.25)),
          "five": (adversarial.lights_many, (2.0, 0.5)), "inside": (adversarial.light_inside, (1.0, 1.0))}
_scenes = {}


def scene(name):
    """(the rtamd Scene, (sqrt_spp, recip_sqrt_spp)), built once."""
    if name not in _scenes:
        _scenes[name] = (SCENES[name][0](), SCENES[name][1])
    return _scenes[name]


def records(sc):
    """The scene's records as float32 / int32 views: spheres [n, 12], quads [n, 20], boxes [n, 6, 20], media [n, 5]."""
    f = lambda b, w: np.frombuffer(bytes(sc.buffers[b]), F32).reshape(-1, w)   # noqa: E731
    return f(0, 12), f(2, 20), f(4, 120).reshape(-1, 6, 20), f(3, 5)


# ------------------------------------------------------------------------------------------------- draws
def draws(rows, n=N_DRAWS):
    """The rows' draw sequences [len, n] float32: oracle_rand_sequence of (px, py, rf)."""
    out = np.zeros((len(rows), n), F32)
    for i, r in enumerate(rows):
        out[i] = pyoracle.rand_sequence(float(r[SOP_PX]), float(r[SOP_PY]), float(r[SOP_RF]), n)
    return out


def _seeds(rng, n):
    """Random (px, py, rf): whole pixels below 2048, rf in [0, 8)."""
    return (rng.integers(0, 2048, n).astype(F32), rng.integers(0, 2048, n).astype(F32),
            rng.uniform(0, 8, n).astype(F32))


# The targets of the search: name -> (draws looked at, predicate on them, rows wanted)
def _rejected(s):   # a rejection round on these draws fails, clear of the boundary
    return sum((-1.0 + float(x) * 2.0) ** 2 for x in s) >= 1.02


TARGETS = {
    "unit_vec_3_rounds": (6, lambda s: _rejected(s[0:3]) and _rejected(s[3:6])),
    "disk_3_rounds": (7, lambda s: _rejected(s[3:5]) and _rejected(s[5:7])),   # after time and the two jitters
    **{f"light_{k}": (1, (lambda k: lambda s: int(np.floor(F32(s[0]) * F32(5.0))) == k)(k)) for k in range(5)},
    "zero_draw": (1, lambda s: s[0] < 2.0 ** -16),                       # medium_tail takes log of it
    "mix_below_half": (3, lambda s: 0.5 - 2.0 ** -12 < s[2] < 0.5),       # a lambertian's third draw
    "mix_at_half": (3, lambda s: s[2] == 0.5),
    "mix_above_half": (3, lambda s: 0.5 < s[2] < 0.5 + 2.0 ** -12),
    "r2_near_one": (2, lambda s: s[1] > 1.0 - 2.0 ** -12),               # sqrt(1 - r2) cancels
    # rand_unit_vec's first candidate is (0, 0, z), z < 0: -z-hat, which cancels a reflection along +z
    "metal_cancel": (3, lambda s: s[0] == 0.5 and s[1] == 0.5 and s[2] < 0.5),
}

# (px, py, rf) per target, as the search found them
FOUND = {
    "unit_vec_3_rounds": [(1904.0, 1421.0, 3.589507579803467), (957.0, 1428.0, 0.7629523873329163), (87.0, 142.0, 7.446344375610352), (1038.0, 1866.0, 7.113885879516602)],
    "disk_3_rounds": [(1286.0, 491.0, 2.9704782962799072), (1805.0, 1446.0, 4.987193584442139), (1281.0, 1549.0, 4.89763069152832), (121.0, 1046.0, 2.0023720264434814)],
    "light_0": [(1827.0, 573.0, 3.689173698425293)],
    "light_1": [(1127.0, 1311.0, 2.1639108657836914)],
    "light_2": [(70.0, 202.0, 7.8903069496154785)],
    "light_3": [(450.0, 958.0, 4.9415154457092285)],
    "light_4": [(1832.0, 249.0, 4.180866718292236)],
    "zero_draw": [(232.0, 216.0, 6.109776973724365), (406.0, 593.0, 3.4655981063842773)],
    "mix_below_half": [(1801.0, 1946.0, 4.897587776184082), (1693.0, 1059.0, 2.2095274925231934)],
    "mix_at_half": [(185.0, 1588.0, 4.112555980682373), (729.0, 1936.0, 0.8066879510879517)],
    "mix_above_half": [(40.0, 21.0, 5.358074188232422), (574.0, 422.0, 4.537913799285889)],
    "r2_near_one": [(879.0, 357.0, 1.1137633323669434), (320.0, 437.0, 5.354884147644043)],
    "metal_cancel": [(684.0, 483.0, 5.013318061828613), (60.0, 1408.0, 5.545443058013916), (231.0, 1494.0, 1.4589152336120605), (1686.0, 1980.0, 1.733339786529541)],
}


def found(name):
    """The fixed rows of a target, checked against it with the oracle's rand_sequence."""
    nd, pred = TARGETS[name]
    for px, py, rf in FOUND[name]:
        assert pred(pyoracle.rand_sequence(px, py, rf, nd)), (name, px, py, rf)
    return FOUND[name]


def _with_seeds(rows, seeds):
    """A copy of `rows` per seed (px, py, rf)."""
    out = []
    for px, py, rf in seeds:
        r = rows.copy()
        r[:, SOP_PX], r[:, SOP_PY], r[:, SOP_RF] = px, py, rf
        out.append(r)
    return np.concatenate(out)


# ------------------------------------------------------------------------------------------- sampling ops
def rand_batches():
    rng = np.random.default_rng(1)
    px, py, rf = _seeds(rng, 4096)
    edge = shade_rows(6, px=[0, 8191, 0, 8191, 16383, 5], py=[0, 0, 8191, 8191, 16383, 7],
                      rf=[0, 0.5, 1023.5, 4095, 0.999, 2.0 ** -20])
    return [Batch("rand", "random", "random", "zoo0", shade_rows(4096, px=px, py=py, rf=rf)),
            Batch("rand", "corners", "edge", "zoo0", edge)]


def onb_batches():
    rng = np.random.default_rng(2)
    n = 4096
    vec = rng.uniform(-1, 1, (n, 3)).astype(F32)
    nrm = (rng.normal(size=(n, 3)) * np.exp2(rng.integers(-4, 5, (n, 1)))).astype(F32)
    # normals along and between the axes, built from binary fractions: |w.x| is 0, 1, or far from 0.9
    ax = np.array([[1, 0, 0], [-4, 0, 0], [0, 2, 0], [0, 0, -0.5], [0, 3, 4], [0, -3, 4], [0, 0, 16], [0, 0.25, 0]], F32)
    ev = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.25, -0.75], [1, 1, 1], [0, 0, 0], [-1, 2, 0.5], [2, 2, 2]], F32)
    return [Batch("onb", "random", "random", "zoo0", shade_rows(n, o=vec, d=nrm)),
            Batch("onb", "axes", "edge", "zoo0", shade_rows(len(ax), o=ev, d=ax))]


def unit_vec_batches():
    rng = np.random.default_rng(3)
    px, py, rf = _seeds(rng, 4096)
    e = _with_seeds(shade_rows(1), found("unit_vec_3_rounds"))
    return [Batch("unit_vec", "random", "random", "zoo0", shade_rows(4096, px=px, py=py, rf=rf)),
            Batch("unit_vec", "three_rounds", "edge", "zoo0", e)]


def _tail_rows(nid, t1, t2, a, tmin, tmax, px=0, py=0, rf=0):
    n = len(np.atleast_1d(t1))
    r = shade_rows(n, px=px, py=py, rf=rf)
    r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4], r[:, 5] = nid, t1, t2, a, tmin, tmax
    return r


def medium_tail_batches():
    rng = np.random.default_rng(4)
    n = 4096
    px, py, rf = _seeds(rng, n)
    t1 = rng.uniform(-3, 3, n)
    t2 = t1 + rng.uniform(-0.5, 4, n)                    # some t1 >= t2
    tmax = np.where(rng.random(n) < 0.5, 3.402823e38, rng.uniform(0, 6, n))
    rnd = _tail_rows(-1.0 / rng.uniform(0.05, 2, n), t1, t2, rng.uniform(0.25, 9, n), 0.001, tmax, px, py, rf)
    inf = F32(3.402823e38)
    # binary fractions: t1 at / below / above tmin, t2 at / above tmax, t1 == t2, t1 < 0, a = 4 (length 2)
    e = _tail_rows(-0.5, [0.5, 0.25, 0.75, 1, 2, -1, -1, 1], [4, 4, 4, 8, 2, 3, 3, 0.5], 4.0,
                   [0.5, 0.5, 0.5, 0.5, 0.5, -2, 0.5, 0.5], [inf, inf, inf, 4, inf, inf, inf, inf], 3, 5, 0.25)
    zero = _with_seeds(_tail_rows(-0.5, [1.0, -1.0], [1024.0, 2.0], 1.0, 0.001, inf), found("zero_draw"))   # log(0) = -inf
    return [Batch("medium_tail", "random", "random", "zoo0", rnd), Batch("medium_tail", "clamps", "edge", "zoo0", e),
            Batch("medium_tail", "log_of_zero", "edge", "zoo0", zero)]


# ---------------------------------------------------------------------------------------------- light ops
def _toward_lights(sc, rng, n):
    """Origins around the scene and directions aimed at points of its lights (or anywhere)."""
    sph, quads, _, _ = records(sc)
    lw = np.frombuffer(bytes(sc.buffers[5]), np.int32)
    o = (rng.uniform(-1, 1, (n, 3)) * [6, 3, 5] + [0, 1, -9]).astype(F32)
    d = rng.normal(size=(n, 3)).astype(F32)
    for i in range(n):
        if lw[0] and rng.random() < 0.8:
            w = int(lw[1 + rng.integers(0, lw[0])])
            typ, idx = (w >> 16) & 0xFFFF, w & 0xFFFF
            if typ == 1:
                tgt = sph[idx, 0:3] + sph[idx, 7] * 0.7 * rng.uniform(-1, 1, 3)
            else:
                tgt = quads[idx, 4:7] + rng.uniform(-0.2, 1.2) * quads[idx, 8:11] + rng.uniform(-0.2, 1.2) * quads[idx, 12:15]
            d[i] = (tgt - o[i]) * rng.uniform(0.25, 2)
    return o, d


def light_pdf_batches():
    out = []
    for k, name in enumerate(("five", "zoo1", "zoo0")):
        rng = np.random.default_rng(50 + k)
        n = 2048
        o, d = _toward_lights(scene(name)[0], rng, n)
        out.append(Batch("light_pdf", f"random_{name}", "random", name, shade_rows(n, o=o, d=d, time=rng.random(n).astype(F32))))
    # light_inside: the sphere light (0, -1, -6) r 2 seen from inside (NaN), from exactly on it (cos_theta_max 0),
    # from 2^14 away (1 - cos_theta_max cancels); the quad light y = 4 seen edge-on, from behind, from below
    o = np.array([[0, -1, -6.5], [0, -1, -4], [0, -1, -6 + 2.0 ** 14], [0, -1, 2], [-3, 4, -6], [0, 6, -6], [0, 0, -6]], F32)
    d = np.array([[0, 0, 1], [0, 0, -1], [0, 0, -1], [0, 0, -2], [1, 0, 0], [0, -1, 0], [0, 2, 0]], F32)
    out.append(Batch("light_pdf", "geometry", "edge", "inside", shade_rows(len(o), o=o, d=d)))
    return out


def light_dir_batches():
    out = []
    for k, name in enumerate(("five", "zoo1", "zoo0", "inside")):
        rng = np.random.default_rng(60 + k)
        n = 2048
        px, py, rf = _seeds(rng, n)
        o = (rng.uniform(-1, 1, (n, 3)) * [6, 3, 5] + [0, 1, -9]).astype(F32)
        if name == "inside":   # keep clear of the sphere light's inside (NaN: the edge set has it)
            o[:, 2] = rng.uniform(0, 6, n)
        out.append(Batch("light_dir", f"random_{name}", "random", name, shade_rows(n, o=o, px=px, py=py, rf=rf)))
    each = np.concatenate([_with_seeds(shade_rows(1, o=[[0.5, 0.25, -3]]), found(f"light_{k}")) for k in range(5)])
    out.append(Batch("light_dir", "each_of_five", "edge", "five", each))
    o = np.array([[0, -1, -6.5], [0, -1, -4], [0, -1, -6 + 2.0 ** 14], [-3, 4, -6], [0, 6, -6]], F32)
    out.append(Batch("light_dir", "geometry", "edge", "inside", shade_rows(len(o), o=o, px=[3, 4, 5, 6, 7], py=9, rf=0.5)))
    return out


def camera_ray_batches():
    out = []
    for k, name in enumerate(("zoo0", "zoo1", "five")):
        rng = np.random.default_rng(70 + k)
        n = 2048
        px, py, rf = _seeds(rng, n)
        out.append(Batch("camera_ray", f"random_{name}", "random", name,
                         shade_rows(n, px=px, py=py, rf=rf, frame=rng.integers(1, 17, n))))
    # sqrt_spp 1 (zoo0, defocus off) and 4 (zoo1, defocus on): frame_count a multiple of sqrt_spp, spp itself,
    # 2^24 + 1; pixel coordinates 0 and 8191
    fr = np.array([4, 8, 16, 2 ** 24 + 1, 1, 16], np.int32)
    for name in ("zoo0", "zoo1"):
        out.append(Batch("camera_ray", f"frames_{name}", "edge", name,
                         shade_rows(len(fr), px=[0, 8191, 0, 8191, 0, 8191], py=[0, 0, 8191, 8191, 8191, 0], rf=0.25, frame=fr)))
    out.append(Batch("camera_ray", "disk_three_rounds", "edge", "zoo1", _with_seeds(shade_rows(1, frame=3), found("disk_3_rounds"))))
    return out


# -------------------------------------------------------------------------------------------------- shade
def _hits(sc, rng, per):
    """`per` rows on each side of every sphere, quad and box face of the scene and inside every medium."""
    sph, quads, boxes, media = records(sc)
    rows = []

    def add(p, nrm, tif, uvk, uv, time, side):
        d = rng.normal(size=(per, 3))
        d *= np.where((d * nrm).sum(axis=1) * side > 0, -1.0, 1.0)[:, None]   # side +1: against the normal (front)
        d *= np.exp2(rng.integers(-2, 3, (per, 1)))
        t = rng.uniform(0.5, 4, (per, 1))
        px, py, rf = _seeds(rng, per)
        rows.append(shade_rows(per, o=p - d * t, d=d, t=t[:, 0], tif=tif, time=time, px=px, py=py, rf=rf,
                               acc=rng.uniform(0.1, 1, (per, 3)), uvk=uvk, uv=uv))

    for i, s in enumerate(sph):
        for side in (1, -1):
            time = rng.random(per).astype(F32)
            u = rng.normal(size=(per, 3))
            u /= np.linalg.norm(u, axis=1)[:, None]
            p = s[0:3] + s[4:7] * time[:, None] + s[7] * u
            add(p, u, 1 | i << 16, 1 << 16 | i, p, time, side)
    for i, q in enumerate(quads):
        for side in (1, -1):
            ab = rng.uniform(0.05, 0.95, (per, 2))
            p = q[4:7] + ab[:, :1] * q[8:11] + ab[:, 1:] * q[12:15]
            add(p, q[0:3], 2 | i << 16, 2 << 16, np.concatenate([ab, ab[:, :1]], axis=1), 0.0, side)
    for i, bx in enumerate(boxes):
        for face in range(6):
            q = bx[face]
            ab = rng.uniform(0.05, 0.95, (per, 2))
            p = q[4:7] + ab[:, :1] * q[8:11] + ab[:, 1:] * q[12:15]
            add(p, q[0:3], 4 | face << 4 | i << 16, 2 << 16, np.concatenate([ab, ab[:, :1]], axis=1), 0.0, 1 if face % 2 else -1)
    for i, m in enumerate(media):
        c = sph[int(m.view(np.int32)[0])]
        p = c[0:3] + 0.5 * c[7] * rng.uniform(-1, 1, (per, 3))
        add(p, np.array([1.0, 0, 0]), 3 | i << 16, 0, p, 0.0, 1)
    return np.concatenate(rows)


def _find(sc, kind, mid, word=None):
    """Index of the first sphere / quad whose material is (mid, word)."""
    sph, quads, _, _ = records(sc)
    mats = sph.view(np.int32)[:, 11] if kind == "sphere" else quads.view(np.int32)[:, 7]
    for i, m in enumerate(mats):
        if (m >> 16) & 0xFFFF == mid and (word is None or (m & 0xFFFF) == word):
            return i
    raise KeyError((kind, mid, word))


def _shade_edges(sc):
    """Geometry edges from binary fractions on the zoo's unit spheres (centres (3 i - 10, 0, -10)) and its quads
    (the plane z = -14, normal +z): dielectric at normal incidence, grazing, past the critical angle from inside,
    with the nior words 0 and 65535; metal with fuzz 0 and 1 (the word 65535), grazing (the fuzzed direction may land below
    the surface); acc holding 0 and inf."""
    sph, quads, _, _ = records(sc)
    rows = []

    def sphere_normal(i, px):   # from 2 in front of the sphere's +z pole, straight at it
        c = sph[i, 0:3]
        p = c + [0, 0, 1]
        return shade_rows(1, o=[c + [0, 0, 3]], d=[[0, 0, -1]], t=2.0, tif=1 | i << 16, px=px, py=11, rf=0.125,
                          acc=[[0.5, 0.25, 1.0]], uvk=1 << 16 | i, uv=[p])

    def quad_hit(i, d, px, acc=(0.5, 0.25, 1.0), t=2.0):   # the quad's centre, reached along d
        q = quads[i]
        p = q[4:7] + 0.5 * q[8:11] + 0.5 * q[12:15]
        d = np.asarray(d, np.float64)
        return shade_rows(1, o=[p - d * t], d=[d], t=t, tif=2 | i << 16, px=px, py=13, rf=0.375, acc=[acc],
                          uvk=2 << 16, uv=[[0.5, 0.5, 0]])

    glass = [i for i, m in enumerate(sph.view(np.int32)[:, 11]) if (m >> 16) & 0xFFFF == 2]
    assert {0, 65535} < {int(sph.view(np.int32)[i, 11]) & 0xFFFF for i in glass}   # the nior words 0 and 65535
    for k, i in enumerate(glass):
        rows.append(sphere_normal(i, 20 + k))
    qd, ql = _find(sc, "quad", 2), _find(sc, "quad", 0)
    for k, d in enumerate(([0, 0, -1], [1, 0, -2.0 ** -10], [1, 0, 0.25], [0, 0, 1], [1, 0, 0.5])):
        rows.append(quad_hit(qd, d, 30 + k))   # front: normal, grazing; back: past critical, normal, oblique
    for qm in [i for i, m in enumerate(quads.view(np.int32)[:, 7]) if (m >> 16) & 0xFFFF == 1]:   # fuzz 0 and the largest
        for k, d in enumerate(([0, 0, -1], [1, 0, -2.0 ** -6], [1, 0.5, -2.0 ** -6], [0, 0, 1])):
            for px in range(4):
                rows.append(quad_hit(qm, d, 40 + 4 * k + px))
    inf = F32(np.inf)
    for k, acc in enumerate(((0, 0, 0), (inf, inf, inf), (0, 1, inf))):
        rows.append(quad_hit(ql, [0.25, 0.5, -1], 60 + k, acc=acc))
        rows.append(sphere_normal(_find(sc, "sphere", 3), 70 + k))
        rows[-1][:, 12:15] = acc
    return np.concatenate(rows)


def _textured(sc):
    """Rows on the checker, Perlin and image quads: device against oracle only."""
    _, quads, _, _ = records(sc)
    rng = np.random.default_rng(91)
    rows = []
    textured = [i for i, t in enumerate(quads.view(np.int32)[:, 11]) if (t >> 28) & 0xF in (1, 2, 3)]
    assert len(textured) == 3
    for i in textured:
        q = quads[i]
        ab = rng.uniform(0, 1, (8, 2))
        p = q[4:7] + ab[:, :1] * q[8:11] + ab[:, 1:] * q[12:15]
        d = rng.normal(size=(8, 3))
        px, py, rf = _seeds(rng, 8)
        rows.append(shade_rows(8, o=p - d * 2.0, d=d, t=2.0, tif=2 | i << 16, px=px, py=py, rf=rf, uvk=2 << 16,
                               uv=np.concatenate([ab, ab[:, :1]], axis=1)))
    return np.concatenate(rows)


def shade_batches():
    out = []
    for k, (name, per) in enumerate((("zoo0", 48), ("zoo1", 48), ("five", 256), ("inside", 256))):
        rng = np.random.default_rng(80 + k)
        out.append(Batch("shade", f"random_{name}", "random", name, _hits(scene(name)[0], rng, per)))
    for name in ("zoo0", "zoo1"):
        sc = scene(name)[0]
        out.append(Batch("shade", f"geometry_{name}", "edge", name, _shade_edges(sc)))
        out.append(Batch("shade", f"textured_{name}", "edge", name, _textured(sc)))
    for name in ("zoo0", "zoo1"):
        sc = scene(name)[0]
        quads = records(sc)[1]
        ql = _find(sc, "quad", 0)
        q = quads[ql]
        p = q[4:7] + 0.5 * q[8:11] + 0.5 * q[12:15]
        base = shade_rows(1, o=[p + [0.5, 1, 2]], d=[[-0.25, -0.5, -1]], t=2.0, tif=2 | ql << 16, acc=[[0.5, 0.25, 1.0]],
                          uvk=2 << 16, uv=[[0.5, 0.5, 0]])
        seeds = found("mix_below_half") + found("mix_at_half") + found("mix_above_half") + found("r2_near_one")
        out.append(Batch("shade", f"draws_{name}", "edge", name, _with_seeds(base, seeds)))
        # near_zero (scatter.glsl:93-95): no material gives a direction below 1e-8 in every component short of an
        # exact cancellation (unit vectors are 6e-8 apart near 1).  Metal with fuzz 1 hit along -n reflects to
        # n = (0, 0, 1); a rand_unit_vec of exactly (0, 0, -1) cancels it.  float64 cannot decide |0| < 1e-8
        # under a bound of 1e-7, so these rows go to the device comparison only.
        qm = _find(sc, "quad", 1, 65535)
        assert tuple(quads[qm, 0:3]) == (0.0, 0.0, 1.0)
        pm = quads[qm, 4:7] + 0.5 * quads[qm, 8:11] + 0.5 * quads[qm, 12:15]
        hit = shade_rows(1, o=[pm + [0, 0, 2]], d=[[0, 0, -1]], t=2.0, tif=2 | qm << 16, acc=[[0.5, 0.25, 1.0]],
                         uvk=2 << 16, uv=[[0.5, 0.5, 0]])
        cancels = 0
        for px, py, rf in found("metal_cancel"):
            z = F32(-1.0) + pyoracle.rand_sequence(px, py, rf, 3)[2] * F32(2.0)
            inv = pyoracle.eval_builtin("inversesqrt", np.array([z * z, 1.0], F32))
            cancels += int(F32(1.0) * inv[1] + F32(1.0) * (z * inv[0]) == 0.0)
        assert cancels >= 1, "no row's fuzzed direction is exactly vec3(0)"
        out.append(Batch("shade", f"near_zero_{name}", "device", name, _with_seeds(hit, found("metal_cancel"))))
    return out


ALL = {"rand": rand_batches, "onb": onb_batches, "unit_vec": unit_vec_batches, "medium_tail": medium_tail_batches,
       "light_pdf": light_pdf_batches, "light_dir": light_dir_batches, "camera_ray": camera_ray_batches,
       "shade": shade_batches}
_batches = {}


def batches(op):
    """The op's batches, built once, each within the hook's input guard."""
    if op not in _batches:
        _batches[op] = ALL[op]()
        for b in _batches[op]:
            r = b.rows
            assert b.op == op and np.isfinite(r[:, [SOP_PX, SOP_PY, SOP_RF]]).all(), b
            assert ((r[:, SOP_PX] >= 0) & (r[:, SOP_PX] < 16384) & (r[:, SOP_PY] >= 0) & (r[:, SOP_PY] < 16384)
                    & (r[:, SOP_RF] >= 0) & (r[:, SOP_RF] < 4096)).all(), b
    return _batches[op]

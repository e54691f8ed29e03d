"""A float64 reference of the operations that decide where a path goes next and what it carries, on
tests/ref64.py's `Err` / `Path` machinery (its docstring defines the running rounding bound and the
decision margins).  Written from the reference's shader text -- utils/random.glsl, math.glsl, pdf.glsl,
scatter.glsl, hitting.glsl (hit_constant_medium) and raytrace/compute.glsl (set_material_properties,
get_norm_coord, get_ray, ray_color, main); each function cites its lines -- not from the oracle or the
kernel.  tests/test_shade_ref64.py compares the CPU oracle's oracle_eval_shade_op with it.

Draws are inputs.  rand() (random.glsl:2-7) is a hash of float32 rounding and has no float64 meaning, so
every function takes the row's draw sequence as exact float32 numbers (`seq` [n, K]), consumes it in the
shader's order and reports how many draws it used (`count`): a draw taken early, late, or when an
early-out should have prevented it shows as a wrong count or a wrong value.  `rand32` restates the hash
itself in float32 numpy (the built-in sin left to the caller).

Built-ins GLSL leaves to the driver carry the bounds tests/test_oracle.py asserts for the project's
(sin / cos 2 ulp, 1e-7 absolute where |value| < 1e-3; log 2 ulp; inversesqrt 2 ulp), propagated through
their derivatives.

Every function returns dict(cls: the classification a float32 implementation must share on decided rows
(the draw count among it), val: name -> Err, mask: name -> the rows where that value means something,
path: ref64.Path).  Out of scope (path.scope False): NaN, values past float32's range, a sphere light's
solid angle whose rounding bound reaches its own size (1 - cos_theta_max cancelled), textures other than
solid ones (pinned by tests/test_ops_ref64.py).

Quirks kept as the shader has them: sphere_model_pdf's and lights_random's center1 without time
(pdf.glsl:18, :92); normalize() of a scalar in cosine_pdf_value (pdf.glsl:33: 1, -1 or NaN); a light index
outside the list, and no light at all, giving vec3(0) (lights_random has no default return: SURVEY
App. A Q1); a frame_count at or past spp placing the sample outside the pixel (random.glsl:84).
"""
import numpy as np

from ref64 import (INFINITY, PI, U, Err, Path, _cmp, _dot, _hit_quad, _hit_sphere, _ulp, _vec, le, lt, pick,
                   select)

MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC, MAT_DIFFUSE_LIGHT, MAT_ISOTROPIC = range(5)   # compute.glsl:8-12
MODEL_SPHERE, MODEL_QUAD, MODEL_CONSTANT_MEDIUM, MODEL_BOX = 1, 2, 3, 4               # compute.glsl:14-17
TEXTYPE_SOLID = 4                                                                       # texture.glsl:1-4
MAX_ROUNDS = 40   # of a rejection loop the reference follows (a row that needs more is out of scope)


def _k(n, x):
    """The float32 constant x in every row."""
    return Err(np.full(n, float(np.float32(x))))


# ---------------------------------------------------------------------------------- built-ins with a bound
def _sin(x, cos=False):
    with np.errstate(all="ignore"):
        v = np.cos(x.v) if cos else np.sin(x.v)
        dv = np.sin(x.v) if cos else np.cos(x.v)
        own = np.where(np.abs(v) < 1e-3, 1e-7, 2.0 * _ulp(v))
        return Err(v, np.abs(dv) * x.e + own, x.n + 1)


def _log(x):
    with np.errstate(all="ignore"):
        v = np.log(x.v)
        # log(+-0) is -inf on either side (tests/test_oracle.py::test_builtin_special_cases): an exact zero is exact
        zero = (x.v == 0.0) & (x.e == 0.0)
        return Err(v, np.where(zero, 0.0, x.e / np.abs(x.v) + 2.0 * _ulp(v)), x.n + 1)


def _inversesqrt(x):
    with np.errstate(all="ignore"):
        v = 1.0 / np.sqrt(x.v)
        return Err(v, x.e * v / (2.0 * np.abs(x.v)) + 2.0 * _ulp(v), x.n + 1)


def _normalize(a):
    inv = _inversesqrt(_dot(a, a))
    return [c * inv for c in a]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _pickv(mask, a, b):
    return [pick(mask, a[k], b[k]) for k in range(3)]


def _zero3(n):
    return [Err(np.zeros(n)) for _ in range(3)]


class Draws:
    """A row's draws, consumed in order: take(live) gives the next one to the rows `live`."""

    def __init__(self, seq):
        self.seq = np.asarray(seq, np.float32).astype(np.float64)
        self.k = np.zeros(self.seq.shape[0], np.int64)
        self.short = np.zeros(self.seq.shape[0], bool)

    def take(self, live):
        K = self.seq.shape[1]
        self.short |= live & (self.k >= K)
        v = self.seq[np.arange(self.seq.shape[0]), np.minimum(self.k, K - 1)]
        self.k = self.k + live.astype(np.int64)
        return Err(v)


def advance_rf(rf, count):
    """rf after `count` draws: that many float32 additions of 0.001 (random.glsl:3)."""
    rf = np.asarray(rf, np.float32).copy()
    count = np.asarray(count)
    for k in range(int(count.max()) if count.size else 0):
        rf = np.where(count > k, rf + np.float32(0.001), rf).astype(np.float32)
    return rf


# ------------------------------------------------------------------------------------------- random.glsl
def rand32(px, py, rf, n_draws, sin32):
    """random.glsl:2-7 in float32: rand_factor += 0.001; co = pixel_coord + rand_factor;
    fract(sin(dot(co, vec2(12.9898, 78.233))) * 43758.5453123), with dot as include/rt/rt_glsl.h states it
    (x x' rounded, then one fused y y' + that) and sin32 the float32 sine under test.  The fused step is
    evaluated in extended precision (its exact value has at most 59 significant bits here) and rounded
    once.  Returns (draws [n, n_draws] float32, rf after)."""
    px, py, rf = (np.asarray(a, np.float32) for a in (px, py, rf))
    k0, k1 = np.float32(12.9898), np.float32(78.233)
    out = np.zeros((px.shape[0], n_draws), np.float32)
    for j in range(n_draws):
        rf = (rf + np.float32(0.001)).astype(np.float32)
        cx, cy = (px + rf).astype(np.float32), (py + rf).astype(np.float32)
        xk = (cx * k0).astype(np.float32)
        dot = (cy.astype(np.longdouble) * np.longdouble(k1) + xk.astype(np.longdouble)).astype(np.float32)
        s = (sin32(dot) * np.float32(43758.5453123)).astype(np.float32)
        out[:, j] = (s - np.floor(s)).astype(np.float32)
    return out, rf


def _unit_vec(P, live, D):
    """rand_unit_vec (random.glsl:33-49): rounds of three rand(-1, 1) until dot(p, p) < 1, normalized."""
    n = live.shape[0]
    p = _zero3(n)
    todo = live.copy()
    for _ in range(MAX_ROUNDS):
        if not todo.any():
            break
        c = [_k(n, -1.0) + D.take(todo) * _k(n, 2.0) for _ in range(3)]   # :10-12, :34-36
        inside, m = lt(_dot(c, c), _k(n, 1.0))                            # :43
        P.take(m, todo)
        p = _pickv(todo, c, p)
        todo = todo & ~inside
    P.scope &= ~todo
    return _normalize(p)                                                  # :48


def unit_vec(seq):
    n = seq.shape[0]
    P, D = Path(n), Draws(seq)
    v = _unit_vec(P, np.ones(n, bool), D)
    P.scope &= ~D.short
    all_ = np.ones(n, bool)
    return dict(cls=dict(count=D.k), val=dict(x=v[0], y=v[1], z=v[2]), mask=dict(x=all_, y=all_, z=all_), path=P)


# --------------------------------------------------------------------------------------------- math.glsl
def _onb(P, live, vec, normal):
    """transform_onb (math.glsl:3-12)."""
    n = live.shape[0]
    w = _normalize(normal)                                                # :5
    big, m = lt(_k(n, 0.9), w[0].abs())                                   # :6
    P.take(m, live)
    P.need(*w, live=live)
    one, zero = Err(np.ones(n)), Err(np.zeros(n))
    a = [pick(big, zero, one), pick(big, one, zero), zero]
    v = _normalize(_cross(w, a))                                          # :7
    u = _cross(w, v)                                                      # :8
    return [(u[k] * vec[0] + v[k] * vec[1]) + w[k] * vec[2] for k in range(3)]   # :10-11


def onb(vec, normal):
    vec, normal = np.asarray(vec, np.float32), np.asarray(normal, np.float32)
    n = vec.shape[0]
    P = Path(n)
    all_ = np.ones(n, bool)
    r = _onb(P, all_, _vec(vec), _vec(normal))
    P.need(*r)
    return dict(cls={}, val=dict(x=r[0], y=r[1], z=r[2]), mask=dict(x=all_, y=all_, z=all_), path=P)


# ------------------------------------------------------------------------------------------ hitting.glsl
def _medium_tail(P, draw, live, nid, t1, t2, a, tmin, tmax):
    """hit_constant_medium after its two boundary hits (hitting.glsl:172-187) for the rows `live`; draw(rows)
    gives those rows their next rand().  Returns (hit, t)."""
    n = live.shape[0]
    c, m = lt(t1, tmin)                                                   # :172
    P.take(m, live)
    t1 = pick(c, tmin, t1)
    c, m = lt(tmax, t2)                                                   # :173
    P.take(m, live)
    t2 = pick(c, tmax, t2)
    ge, m = le(t2, t1)                                                    # :175
    P.take(m, live)
    live = live & ~ge
    c, m = lt(t1, Err(np.zeros(n)))                                       # :178
    P.take(m, live)
    t1 = pick(c & live, Err(np.zeros(n)), t1)
    length = a.sqrt()                                                     # :181
    inside = (t2 - t1) * length                                           # :182
    hd = nid * _log(draw(live))                                           # :183
    P.need(hd, inside, live=live, inf_ok=True)
    past, m = lt(inside, hd)                                              # :185
    P.take(m, live)
    hit = live & ~past
    t = t1 + hd / length                                                  # :188
    P.need(t, live=hit)
    return hit, t


def medium_tail(nid, t1, t2, a, tmin, tmax, seq):
    """hit_constant_medium after its two boundary hits (hitting.glsl:172-187): a = dot(ray.dir, ray.dir)."""
    nid, t1, t2, a, tmin, tmax = (Err.of(x) for x in (nid, t1, t2, a, tmin, tmax))
    n = t1.v.shape[0]
    P, D = Path(n), Draws(seq)
    hit, t = _medium_tail(P, D.take, np.ones(n, bool), nid, t1, t2, a, tmin, tmax)
    return dict(cls=dict(hit=hit, count=D.k), val=dict(t=t), mask=dict(t=hit), path=P)


# ---------------------------------------------------------------------------------------------- the scene
class RefScene:
    """The records of an rtamd Scene as float64 / int arrays, and the uniforms the operations read."""

    def __init__(self, scene, sqrt_spp=1.0, recip_sqrt_spp=1.0):
        f = lambda b, w: np.frombuffer(bytes(scene.buffers[b]), np.float32).reshape(-1, w)   # noqa: E731
        self.spheres, self.quads, self.media = f(0, 12), f(2, 20), f(3, 5)
        self.boxes = f(4, 120).reshape(-1, 6, 20)
        lw = np.frombuffer(bytes(scene.buffers[5]), np.int32)
        self.lights = [((int(x) >> 16) & 0xFFFF, int(x) & 0xFFFF) for x in lw[1:1 + int(lw[0])]] if lw.size else []
        self.tex = {t.slot: (t.format, t.width, t.height, np.frombuffer(bytes(t.data), np.uint8)) for t in scene.textures}
        self.cam = np.asarray(scene.camera, np.float32)
        self.sqrt_spp, self.recip_sqrt_spp = np.float32(sqrt_spp), np.float32(recip_sqrt_spp)

    def sphere(self, i, n):
        s = self.spheres[i].astype(np.float64)
        return ([Err(np.full(n, s[k])) for k in range(3)], [Err(np.full(n, s[4 + k])) for k in range(3)],
                Err(np.full(n, s[7])))

    @staticmethod
    def quad_of(rec, n):
        q = rec.astype(np.float64)
        g = lambda k: [Err(np.full(n, q[k + i])) for i in range(3)]   # noqa: E731
        return dict(normal=g(0), d=Err(np.full(n, q[3])), q=g(4), u=g(8), v=g(12), area=Err(np.full(n, q[15])))

    def solid_rgb(self, tex_id):
        """texture_color's solid case (texture.glsl:112-132): texel (detail, 0) of the slot, a stored number."""
        fmt, w, h, data = self.tex[(tex_id >> 12) & 7]
        x = tex_id & 0xFFF
        if fmt == 3:
            return [float(data.view(np.float32)[x]), 0.0, 0.0]
        comps = 3 if fmt == 1 else 4
        return [float(np.float32(data[x * comps + c]) / np.float32(255.0)) for c in range(3)]


# ---------------------------------------------------------------------------------------------- pdf.glsl
def _lights_pdf(S, P, live, o, d, time):
    """lights_pdf_value (pdf.glsl:58-81) with sphere_model_pdf (:11-24) and quad_pdf_value (:41-51)."""
    n = live.shape[0]
    total = Err(np.zeros(n))
    if not S.lights:
        return total                                                      # weight = 1 / 0 multiplies nothing
    weight = Err(np.ones(n)) / Err(np.full(n, float(len(S.lights))))      # :59
    lo, hi = _k(n, 0.001), _k(n, INFINITY)
    one = Err(np.ones(n))
    for typ, idx in S.lights:
        pdf = Err(np.zeros(n))
        if typ == MODEL_SPHERE:
            c1, cv, r = S.sphere(idx, n)
            hit, _t = _hit_sphere(P, live, o, d, c1, cv, r, time, lo, hi)  # :15
            pc = [c1[k] - o[k] for k in range(3)]                         # :18: center1, no time
            ctm = (one - r * r / _dot(pc, pc)).sqrt()                     # :20
            solid = _k(n, 2.0) * _k(n, PI) * (one - ctm)                  # :21
            with np.errstate(all="ignore"):
                lost = hit & live & ~(solid.bound() < np.abs(solid.v))
            P.scope &= ~lost
            P.need(ctm, solid, live=hit & live)
            pdf = pick(hit, one / solid, pdf)                             # :23
        elif typ == MODEL_QUAD:
            Q = S.quad_of(S.quads[idx], n)
            hit, t, _a, _b = _hit_quad(P, live, o, d, Q, lo, hi)          # :44
            d2 = t * t * _dot(d, d)                                       # :47
            cosine = (_dot(d, Q["normal"]) / _dot(d, d).sqrt()).abs()     # :48 (abs: either face's normal)
            q = d2 / (cosine * Q["area"])                                 # :50
            P.need(q, live=hit & live, inf_ok=True)
            pdf = pick(hit, q, pdf)
        total = total + weight * pdf                                      # :77
    return total


def light_pdf(S, o, d, time):
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    n = o.shape[0]
    P = Path(n)
    all_ = np.ones(n, bool)
    pdf = _lights_pdf(S, P, all_, _vec(o), _vec(d), Err.of(time))
    P.need(pdf, inf_ok=True)
    return dict(cls={}, val=dict(pdf=pdf), mask=dict(pdf=all_), path=P)


def _floor_decided(x, P, live):
    """floor(x) and the margin of its decision: the distance to the nearer integer."""
    with np.errstate(invalid="ignore"):
        ok = np.abs(x.v) < 2.0 ** 31
    v = np.where(ok, x.v, 0.0)
    P.scope &= ~(live & ~ok)
    fl = np.floor(v)
    P.take(_cmp(np.minimum(v - fl, fl + 1.0 - v), x.bound()), live)
    return fl


def _lights_random(S, P, live, o, D):
    """lights_random (pdf.glsl:83-96), rand_int (random.glsl:15-17), sphere_model_random (pdf.glsl:26-30),
    rand_to_sphere (random.glsl:71-80), quad_random (pdf.glsl:53-56)."""
    n = live.shape[0]
    count = len(S.lights)
    x = Err(np.zeros(n)) + D.take(live) * (Err(np.full(n, float(count))) - Err(np.zeros(n)))   # :11, :16
    li = _floor_decided(x, P, live)
    out = _zero3(n)                                                       # an index outside the list: vec3(0)
    one = Err(np.ones(n))
    for L, (typ, idx) in enumerate(S.lights):
        m = live & (li == L)
        if not m.any():
            continue
        if typ == MODEL_SPHERE:
            c1, _cv, r = S.sphere(idx, n)
            dirn = [c1[k] - o[k] for k in range(3)]                       # :27 (center1: :92)
            d2 = _dot(dirn, dirn)                                         # :28
            r1, r2 = D.take(m), D.take(m)                                 # :72-73
            z = one + r2 * ((one - r * r / d2).sqrt() - one)              # :74
            phi = _k(n, 2.0) * _k(n, PI) * r1                             # :75
            s = (one - z * z).sqrt()
            v = _onb(P, m, [_sin(phi, cos=True) * s, _sin(phi) * s, z], dirn)   # :76-77, :29
            P.need(*v, live=m)
        elif typ == MODEL_QUAD:
            Q = S.quad_of(S.quads[idx], n)
            r1 = D.take(m)
            p = [Q["q"][k] + r1 * Q["u"][k] for k in range(3)]            # :54, left to right
            r2 = D.take(m)
            v = [(p[k] + r2 * Q["v"][k]) - o[k] for k in range(3)]        # :55
        else:
            continue
        out = _pickv(m, v, out)
    return out


def light_dir(S, o, seq):
    o = np.asarray(o, np.float32)
    n = o.shape[0]
    P, D = Path(n), Draws(seq)
    all_ = np.ones(n, bool)
    v = _lights_random(S, P, all_, _vec(o), D)
    P.scope &= ~D.short
    return dict(cls=dict(count=D.k), val=dict(x=v[0], y=v[1], z=v[2]), mask=dict(x=all_, y=all_, z=all_), path=P)


# ------------------------------------------------------------------------------------------ compute.glsl
def camera_ray(S, px, py, frame, seq):
    """main()'s time = rand() (compute.glsl:349), get_ray (:282-294), get_norm_coord (:268-280),
    pixel_sample_square (random.glsl:82-100), defocus_disk_sample (:19-30)."""
    px, py = Err.of(px), Err.of(py)
    n = px.v.shape[0]
    P, D = Path(n), Draws(seq)
    all_ = np.ones(n, bool)
    C = S.cam.astype(np.float64)
    cv = lambda k: [Err(np.full(n, C[k + i])) for i in range(3)]   # noqa: E731
    cpos, ul, du, dv, ddu, ddv = cv(4), cv(8), cv(12), cv(16), cv(20), cv(24)
    time = D.take(all_)
    coord = [ul[k] + px * du[k] for k in range(3)]                        # :274
    coord = [coord[k] + py * dv[k] for k in range(3)]                     # :276
    fc = Err.of(np.asarray(frame, np.int64).astype(np.float32))           # float(frame_count)
    ss, rs = Err(np.full(n, float(S.sqrt_spp))), Err(np.full(n, float(S.recip_sqrt_spp)))
    half = Err(np.full(n, 0.5))
    q = fc / ss
    col = fc - ss * Err(_floor_decided(q, P, all_))                       # :83: mod(x, y) = x - y floor(x / y)
    layer = fc / ss                                                       # :84
    base_x = (col + half) * rs                                            # :87
    base_y = (layer + half) * rs                                          # :88
    jx = (D.take(all_) - half) * rs                                       # :91
    jy = (D.take(all_) - half) * rs                                       # :92
    sx = base_x + jx - half                                               # :95
    sy = base_y + jy - half                                               # :96
    coord = [coord[k] + (sx * du[k] + sy * dv[k]) for k in range(3)]      # :99, :279
    o = cpos
    if not (C[3] <= 0.0):                                                 # :291: a uniform, exact
        p = [Err(np.zeros(n)), Err(np.zeros(n))]
        todo = all_.copy()
        for _ in range(MAX_ROUNDS):                                       # random.glsl:19-24
            if not todo.any():
                break
            c = [_k(n, -1.0) + D.take(todo) * _k(n, 2.0) for _ in range(2)]
            inside, m = lt(c[0] * c[0] + c[1] * c[1], _k(n, 1.0))
            P.take(m, todo)
            p = [pick(todo, c[k], p[k]) for k in range(2)]
            todo = todo & ~inside
        P.scope &= ~todo
        o = [(cpos[k] + p[0] * ddu[k]) + p[1] * ddv[k] for k in range(3)]  # :29
    d = [coord[k] - o[k] for k in range(3)]                               # :292
    P.scope &= ~D.short
    P.need(*d)
    val = dict(ox=o[0], oy=o[1], oz=o[2], dx=d[0], dy=d[1], dz=d[2])
    # time is the first draw itself: part of the classification, compared exactly
    return dict(cls=dict(count=D.k, time=time.v.astype(np.float32)), val=val, mask={k: all_ for k in val}, path=P)


def _near_zero(v, P, live):
    """near_zero (scatter.glsl:3-6): every |component| < 1e-8."""
    n = live.shape[0]
    res, ms = np.ones(n, bool), []
    for c in v:
        b, m = lt(c.abs(), _k(n, 1e-8))
        res &= b
        ms.append((b, m))
    # one component decidedly not small settles it; else all three must be decided
    settled = np.zeros(n, bool)
    allm = np.full(n, np.inf)
    for b, m in ms:
        settled |= ~b & (m > 1.0)
        allm = np.minimum(allm, m)
    P.take(np.where(settled, np.inf, allm), live)
    return res


def _reflect(i, nrm):
    n = i[0].v.shape[0]
    t = _k(n, 2.0) * _dot(nrm, i)                                         # I - 2 dot(N, I) N
    return [i[k] - t * nrm[k] for k in range(3)]


def _shade_group(S, tif, o, d, t, time, acc, seq):
    """One closest hit `tif` shared by the rows: the hit record (hitting.glsl:38-46, :122-131, :188-190),
    set_material_properties (compute.glsl:197-224), then ray_color's loop body (:310-339) with scatter
    (scatter.glsl) and the mixture's pdfs (pdf.glsl:32-39, :98-124)."""
    n = o.shape[0]
    P, D = Path(n), Draws(seq)
    all_ = np.ones(n, bool)
    o, d, t, time = _vec(o), _vec(d), Err.of(t), Err.of(time)
    acc = _vec(acc)
    one, zero = Err(np.ones(n)), Err(np.zeros(n))
    typ, face, idx = tif & 0xF, (tif >> 4) & 7, (tif >> 16) & 0xFFFF
    p = [o[k] + d[k] * t for k in range(3)]
    front = all_
    if typ == MODEL_SPHERE:
        rec = S.spheres[idx]
        c1, cv, r = S.sphere(idx, n)
        center = [c1[k] + cv[k] * time for k in range(3)]
        outward = [(p[k] - center[k]) / r for k in range(3)]
        front, m = lt(_dot(d, outward), zero)
        P.take(m)
        normal = _pickv(front, outward, [-c for c in outward])
        material, tex_id, emis = int(rec.view(np.int32)[11]), int(rec.view(np.int32)[3]), rec[8:11]
    elif typ in (MODEL_QUAD, MODEL_BOX):
        rec = S.quads[idx] if typ == MODEL_QUAD else S.boxes[idx, face]
        first = S.quads[idx] if typ == MODEL_QUAD else S.boxes[idx, 0]    # compute.glsl:219: box.quads[0]
        nq = [Err(np.full(n, float(rec[k]))) for k in range(3)]
        front, m = lt(_dot(d, nq), zero)
        P.take(m)
        normal = _pickv(front, nq, [-c for c in nq])
        material, tex_id, emis = int(first.view(np.int32)[7]), int(first.view(np.int32)[11]), first[16:19]
    else:
        rec = S.media[idx]
        normal = [one, zero, zero]
        material, tex_id, emis = int(rec.view(np.int32)[3]), int(rec.view(np.int32)[4]), np.zeros(3, np.float32)
    emission = [pick(front, Err(np.full(n, float(e))), zero) for e in emis]
    solid = ((tex_id >> 28) & 0xF) == TEXTYPE_SOLID and ((tex_id >> 12) & 7) in S.tex
    att = [Err(np.full(n, c)) for c in (S.solid_rgb(tex_id) if solid else [0.0, 0.0, 0.0])]
    mid, word = (material >> 16) & 0xFFFF, material & 0xFFFF
    with np.errstate(invalid="ignore"):
        acc_ok = np.all([np.isfinite(c.v) for c in acc], axis=0)

    def out(ended, result, d_new, acc_new):
        res = [acc[k] * emission[k] for k in range(3)] if result is None else result
        cont = ~ended
        val = dict(zip(("r", "g", "b", "ox", "oy", "oz", "dx", "dy", "dz", "ar", "ag", "ab"), res + p + d_new + acc_new))
        mask = {k: (ended if k in "rgb" else cont) & (acc_ok | (k[0] in "od")) for k in val}
        if not solid:
            for k in ("ar", "ag", "ab"):
                mask[k] = np.zeros(n, bool)
        P.scope &= ~D.short
        return dict(cls=dict(ended=ended, count=D.k), val=val, mask=mask, path=P)

    if mid == MAT_DIFFUSE_LIGHT:                                          # scatter.glsl:83-84
        return out(all_, None, d, acc)
    skip_pdf, should = False, all_
    if mid == MAT_LAMBERTIAN:                                             # :49-54, random.glsl:59-69
        r1, r2 = D.take(all_), D.take(all_)
        phi = _k(n, 2.0) * _k(n, PI) * r1
        cd = [_sin(phi, cos=True) * r2.sqrt(), _sin(phi) * r2.sqrt(), (one - r2).sqrt()]
        dn = _onb(P, all_, cd, normal)
    elif mid == MAT_METAL:                                                # :55-66, :12-15
        fuzz = Err(np.full(n, float(word))) / _k(n, 65535.0)
        rd = _normalize(_reflect(d, normal))
        uv = _unit_vec(P, all_, D)
        dn = [rd[k] + fuzz * uv[k] for k in range(3)]
        should, m = lt(zero, _dot(dn, normal))                            # :63
        P.take(m)
        skip_pdf = True
    elif mid == MAT_DIELECTRIC:                                           # :67-82, :17-37
        nior = Err(np.full(n, float(word))) / _k(n, 65535.0)
        eta = _k(n, 1.0) * (one - nior) + _k(n, 2.5) * nior               # mix(MIN_IOR, MAX_IOR, a)
        eta = pick(front, one / eta, eta)                                 # :77
        ud = _normalize(d)                                                # :25
        cos_t = _dot([-c for c in ud], normal)
        cos_t = select(cos_t.v < 1.0, cos_t, one)                         # :26
        s2 = one - cos_t * cos_t                                          # :27
        # cos_t <= 1 after the min on either side, so float32's operand is never negative; near zero the
        # root's change is at most sqrt(|change of the operand|), where e / (2 z) diverges
        with np.errstate(all="ignore"):
            zs = np.sqrt(np.maximum(s2.v, 0.0))
            sin_t = Err(zs, np.minimum(s2.e / (2.0 * zs), np.sqrt(s2.e)) + U * zs, s2.n + 1)
        P.need(sin_t)
        cannot, m = lt(one, eta * sin_t)                                  # :30
        P.take(m)
        r0 = (one - eta) / (one + eta)                                    # :19
        r0 = r0 * r0
        x = one - cos_t
        x2 = x * x
        refl = r0 + (one - r0) * ((x2 * x2) * x)                          # :21: pow(x, 5)
        draw = D.take(~cannot)                                            # :32: || short-circuits
        rgt, m = lt(draw, refl)
        P.take(m, ~cannot)
        reflect = cannot | rgt
        dr = _reflect(ud, normal)                                         # :33
        dni = _dot(normal, ud)                                            # refract(I, N, eta)
        k_ = one - (eta * eta) * (one - dni * dni)
        kneg, m = lt(k_, zero)
        P.take(m, ~reflect)
        s = eta * dni + pick(kneg, zero, k_).sqrt()
        dt = [pick(kneg, zero, eta * ud[k] - s * normal[k]) for k in range(3)]   # :35
        dn = _pickv(reflect, dr, dt)
        skip_pdf = True
    elif mid == MAT_ISOTROPIC:                                            # :85-90
        dn = _unit_vec(P, all_, D)
    else:
        raise ValueError(f"material {mid} is not one the shader names")
    P.need(*dn)
    nz = _near_zero(dn, P, all_)                                          # :94-95
    dn = _pickv(nz, normal, dn)
    if skip_pdf:                                                          # compute.glsl:317-324
        return out(~should, None, dn, [acc[k] * att[k] for k in range(3)])
    mix, m = lt(D.take(all_), Err(np.full(n, 0.5)))                       # :328
    P.take(m)
    ld = _lights_random(S, P, mix, p, D)
    dn = _pickv(mix, ld, dn)
    P.need(*dn)
    lpdf = _lights_pdf(S, P, all_, p, dn, time)                           # :329
    if mid == MAT_LAMBERTIAN:                                             # pdf.glsl:32-35: normalize(float)
        cs = _dot(dn, normal)
        pos, m = lt(zero, cs)
        P.take(m)
        P.need(cs)
        mpdf = pick(pos, one / _k(n, PI), zero)
    else:
        mpdf = one / (_k(n, 4.0) * _k(n, PI))                             # :4
    half = Err(np.full(n, 0.5))
    pdf = half * lpdf + half * mpdf                                       # :330
    P.need(pdf, inf_ok=True)
    P.take(_cmp(pdf.v, pdf.bound()))                                      # :333: == 0.0
    ended = pdf.v == 0.0
    if mid == MAT_LAMBERTIAN:                                             # pdf.glsl:115-118
        ct = _dot(normal, _normalize(dn)) / _k(n, PI)
        spdf = select(ct.v > 0.0, ct, zero)
    else:
        spdf = one / (_k(n, 4.0) * _k(n, PI))
    acc_new = [acc[k] * (att[k] * spdf / pdf) for k in range(3)]          # :338
    P.need(*acc_new, live=~ended & acc_ok)
    return out(ended, None, dn, acc_new)


def shade(S, rows, seq):
    """Rows of rt_debug_eval_shade_op's layout (o, d, t, tif, time, .., acc): grouped by their hit."""
    rows = np.asarray(rows, np.float32)
    n = rows.shape[0]
    tifs = rows.view(np.int32)[:, 7]
    P = Path(n)
    cls = dict(ended=np.zeros(n, bool), count=np.zeros(n, np.int64))
    val, mask = {}, {}
    for tif in np.unique(tifs):
        g = np.nonzero(tifs == tif)[0]
        R = _shade_group(S, int(tif), rows[g, 0:3], rows[g, 3:6], rows[g, 6], rows[g, 8], rows[g, 12:15], seq[g])
        P.margin[g], P.scope[g] = R["path"].margin, R["path"].scope
        for k in cls:
            cls[k][g] = R["cls"][k]
        for k, e in R["val"].items():
            if k not in val:
                val[k], mask[k] = Err(np.zeros(n), np.zeros(n)), np.zeros(n, bool)
            with np.errstate(all="ignore"):
                val[k].v[g], val[k].e[g] = e.v, e.bound()
            mask[k][g] = R["mask"][k]
    return dict(cls=cls, val=val, mask=mask, path=P)

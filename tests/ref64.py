"""A float64 reference of the kernel's per-ray operations, written from the reference's shader text
(src/main/resources/shaders/utils/hitting.glsl and texture.glsl; each function cites its lines), not
from the oracle or the kernel.  Plain numpy.  tests/test_ops_ref64.py compares the CPU oracle with it.

How a float32 implementation is compared with it
------------------------------------------------
Every function evaluates the shader's expressions on `Err` values: a float64 value `v` together with
a bound `e` on |float32 result - v| for an implementation that performs the shader's operations in
IEEE float32 with any mix of fused and unfused multiply-adds (a fused one has one rounding fewer).
The bound is the first-order running error of the operation sequence, u = 2^-24:

    z = x + y, x - y:  e_z = e_x + e_y + u |z|
    z = x * y:         e_z = |x| e_y + |y| e_x + u |z|
    z = x / y:         e_z = (e_x + |z| e_y) / |y| + u |z|
    z = sqrt(x):       e_z = e_x / (2 z) + u |z|
    z = min / max / select(x, y):  e_z = e_x + e_y  (the other side may have chosen the other
                       operand, which is then within e_x + e_y of this one)

so a path of n operations on well-conditioned data ends with about n u |z|, and the propagation terms
ARE the condition factors.  For a sphere root, t = (-hb -+ sqrt(disc)) / a with disc = hb^2 - a c:
e_disc / |disc| carries (hb^2 + |a c|) / |disc| times the operands' relative errors, the square root
halves it, and the numerator's cancellation multiplies by (|hb| + sqrt(disc)) / |-hb -+ sqrt(disc)|
-- the two factors of the closed form, here accumulated operation by operation.  For a quad's alpha
and beta the 2-D cross terms ph.x v.y - ph.y v.x cancel: e grows by (|ph.x v.y| + |ph.y v.x|) / |their
difference|.  Higher-order terms are covered by the factor 1 / (1 - n u) with n the operations on
the path (`Err.n`), i.e. the bound is the n u / (1 - n u) form with each operation's own weight.

An operation whose float32 result is exact contributes no u |z|: operands without error, a float64
result that a float32 holds, and a float64 operation that was itself exact (checked by an
error-free transformation: TwoSum for sums, z y == x for quotients, z z == x for roots; a product of
two float32 values is always exact in float64).  So on inputs chosen as binary fractions the bound is
0, every comparison is decided, and a float32 implementation must give float64's value exactly.
Results below 2^-126 in magnitude round absolutely (2^-150), and a value at or above 2^128 has no
float32: such rows are out of this reference's scope (`scope` False), as is anything involving NaN.

Decisions.  Each comparison the shader makes (discriminant against 0, a root against ray_t, |denom|
against 1e-8, alpha / beta against 0 and 1, slab overlap, a checker coordinate against the next
integer) returns its float64 outcome and a decision margin |lhs - rhs| / (e_lhs + e_rhs) (inf when
both errors are 0).  A row is decided when every comparison on its path has a margin above 1; only
then must a float32 implementation agree on hit / miss, face or parity, and only then is the value
bound meaningful (the same branch was taken).

The reference's quirks are kept: the Perlin fade applied twice (texture.glsl:42-44 and :20-22), the
uv of a rejected face left alone (hitting.glsl:83-87), INFINITY = 3.402823E+38 (compute.glsl:7).
"""
import numpy as np

U = 2.0 ** -24
F32_MIN = 2.0 ** -126
F32_LIM = 2.0 ** 128
INFINITY = float(np.float32(3.402823e38))      # compute.glsl:7
PI = float(np.float32(3.14159265359))          # math.glsl:1


def _f32rep(z):
    with np.errstate(over="ignore", invalid="ignore"):
        return z.astype(np.float32).astype(np.float64) == z


class Err:
    """value, error bound, operation count (see the module docstring)."""
    __slots__ = ("v", "e", "n")

    def __init__(self, v, e=None, n=0):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, np.float64)
        self.n = n

    @staticmethod
    def of(x):
        return x if isinstance(x, Err) else Err(np.asarray(x, np.float32).astype(np.float64))

    def _round(self, z, prop, exact, n):
        r = np.where(exact & (prop == 0.0), 0.0, np.maximum(U * np.abs(z), 2.0 ** -150))
        return Err(z, prop + r, n)

    def __neg__(self):
        return Err(-self.v, self.e, self.n)

    def __add__(self, o):
        o = Err.of(o)
        with np.errstate(all="ignore"):
            z = self.v + o.v
            bb = z - self.v
            two_sum = (self.v - (z - bb)) + (o.v - bb)
            return self._round(z, self.e + o.e, _f32rep(z) & (two_sum == 0.0), self.n + o.n + 1)

    def __sub__(self, o):
        return self + (-Err.of(o))

    def __mul__(self, o):
        o = Err.of(o)
        with np.errstate(all="ignore"):
            z = self.v * o.v
            prop = np.where(self.e == 0.0, 0.0, np.abs(o.v) * self.e) + np.where(o.e == 0.0, 0.0, np.abs(self.v) * o.e)
            return self._round(z, prop, _f32rep(z), self.n + o.n + 1)

    def __truediv__(self, o):
        o = Err.of(o)
        with np.errstate(all="ignore"):
            z = self.v / o.v
            prop = np.where((self.e == 0.0) & (o.e == 0.0), 0.0, (self.e + np.abs(z) * o.e) / np.abs(o.v))
            # x / +-0 and x / +-inf are the same +-inf, +-0 (or NaN) in either precision
            return self._round(z, prop, _f32rep(z) & ((z * o.v == self.v) | (o.v == 0.0) | np.isinf(o.v)),
                               self.n + o.n + 1)

    def sqrt(self):
        with np.errstate(all="ignore"):
            z = np.sqrt(self.v)
            prop = np.where(self.e == 0.0, 0.0, self.e / (2.0 * z))
            return self._round(z, prop, _f32rep(z) & (z * z == self.v), self.n + 1)

    def abs(self):
        return Err(np.abs(self.v), self.e, self.n)

    def bound(self):
        """The error bound with the higher-order factor 1 / (1 - n u)."""
        return self.e / (1.0 - self.n * U)


def select(mask, x, y):
    """mask ? x : y where the other side's mask may differ only when x and y are within their errors."""
    x, y = Err.of(x), Err.of(y)
    same = (x.e == 0.0) & (y.e == 0.0)
    return Err(np.where(mask, x.v, y.v), np.where(same, 0.0, x.e + y.e), max(x.n, y.n))


def pick(mask, x, y):
    """mask ? x : y for a mask that is decided (a branch the caller accounts for with its margin)."""
    x, y = Err.of(x), Err.of(y)
    return Err(np.where(mask, x.v, y.v), np.where(mask, x.e, y.e), max(x.n, y.n))


def _cmp(diff, e):
    with np.errstate(all="ignore"):
        m = np.where(e == 0.0, np.inf, np.abs(diff) / e)
    return np.where(np.isnan(m), 0.0, m)


def lt(x, y):
    """(x < y in float64, decision margin)."""
    x, y = Err.of(x), Err.of(y)
    with np.errstate(invalid="ignore"):
        return x.v < y.v, _cmp(x.v - y.v, x.bound() + y.bound())


def le(x, y):
    x, y = Err.of(x), Err.of(y)
    with np.errstate(invalid="ignore"):
        return x.v <= y.v, _cmp(x.v - y.v, x.bound() + y.bound())


class Path:
    """The decision margin and scope of each row along its path: `take(cond, margin, live)` records a
    comparison that rows `live` evaluate."""

    def __init__(self, n):
        self.margin = np.full(n, np.inf)
        self.scope = np.ones(n, bool)

    def take(self, margin, live=True):
        self.margin = np.where(live, np.minimum(self.margin, margin), self.margin)

    def need(self, *vals, live=True, inf_ok=False):
        """Rows whose value leaves float32's finite range (or is NaN) are out of scope; inf_ok: an
        infinity both precisions produce alike (x / 0) stays in."""
        for x in vals:
            v = Err.of(x).v
            with np.errstate(invalid="ignore"):
                bad = ~(np.abs(v) < F32_LIM)
                if inf_ok:
                    bad &= ~np.isinf(v)
            self.scope &= ~(bad & live)

    @property
    def decided(self):
        return self.scope & (self.margin > 1.0)


def _vec(a):
    a = np.asarray(a, np.float32).astype(np.float64).reshape(-1, 3)
    return [Err(a[:, k]) for k in range(3)]


def _dot(a, b):
    """GLSL dot: x x' + y y' + z z' (five roundings; a fused form has fewer and the same bound holds)."""
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _surrounds(lo, hi, x, P, live):   # interval.glsl: min < x && x < max
    a, ma = lt(lo, x)
    b, mb = lt(x, hi)
    # a false and decided settles it; so does b false and decided; else both must be decided
    m = np.where(~a & (ma > 1.0), ma, np.where(~b & (mb > 1.0), mb, np.minimum(ma, mb)))
    P.take(m, live)
    return a & b


def _contains(lo, hi, x, P, live):    # interval.glsl: min <= x && x <= max
    a, ma = le(lo, x)
    b, mb = le(x, hi)
    m = np.where(~a & (ma > 1.0), ma, np.where(~b & (mb > 1.0), mb, np.minimum(ma, mb)))
    P.take(m, live)
    return a & b


# ------------------------------------------------------------------------------------------ hitting.glsl
def _hit_sphere(P, live, o, d, c1, cv, radius, time, tmin, tmax):
    """hitting.glsl:17-47 up to hit_record.t (:38).  Returns (hit, t)."""
    center = [c1[k] + cv[k] * time for k in range(3)]        # :13-15, :18
    oc = [o[k] - center[k] for k in range(3)]                # :19
    a = _dot(d, d)                                           # :20
    half_b = _dot(oc, d)                                     # :21
    c = _dot(oc, oc) - radius * radius                       # :22
    disc = half_b * half_b - a * c                           # :23
    P.need(a, half_b, c, disc, live=live)
    neg, m = lt(disc, 0.0)                                   # :25
    P.take(m, live)
    live = live & ~neg
    sqrtd = disc.sqrt()                                      # :28
    root = (-half_b - sqrtd) / a                             # :31
    P.need(root, live=live)
    in1 = _surrounds(tmin, tmax, root, P, live)              # :32
    root2 = (-half_b + sqrtd) / a                            # :33
    P.need(root2, live=live & ~in1)
    in2 = _surrounds(tmin, tmax, root2, P, live & ~in1)      # :34
    hit = live & (in1 | in2)
    return hit, pick(in1, root, root2)


def _sphere_fields(spheres):
    s = np.ascontiguousarray(spheres).view(np.float32).reshape(-1, 12).astype(np.float64)
    return [Err(s[:, k]) for k in range(3)], [Err(s[:, 4 + k]) for k in range(3)], Err(s[:, 7])


def hit_sphere(spheres, rows):
    """hit_sphere (hitting.glsl:17-47) per row.  Returns dict(hit, t (Err), path)."""
    rows = np.asarray(rows, np.float32)
    n = rows.shape[0]
    P = Path(n)
    c1, cv, r = _sphere_fields(spheres)
    hit, t = _hit_sphere(P, np.ones(n, bool), _vec(rows[:, 0:3]), _vec(rows[:, 3:6]), c1, cv, r, Err.of(rows[:, 8]),
                         Err.of(rows[:, 6]), Err.of(rows[:, 7]))
    return dict(hit=hit, t=t, path=P)


def medium_boundary_hits(spheres, rows):
    """hit_constant_medium's two hit_boundary calls (hitting.glsl:163-169) on a sphere boundary:
    rec1 over (-INFINITY, INFINITY), rec2 over (rec1.t + 0.0001, INFINITY).  dict(ok, t1, t2, path)."""
    rows = np.asarray(rows, np.float32)
    n = rows.shape[0]
    P = Path(n)
    c1, cv, r = _sphere_fields(spheres)
    o, d, time = _vec(rows[:, 0:3]), _vec(rows[:, 3:6]), Err.of(rows[:, 8])
    all_ = np.ones(n, bool)
    h1, t1 = _hit_sphere(P, all_, o, d, c1, cv, r, time, Err.of(np.float32(-INFINITY)), Err.of(np.float32(INFINITY)))
    lo2 = t1 + Err.of(np.float32(0.0001))                     # :168
    h2, t2 = _hit_sphere(P, h1, o, d, c1, cv, r, time, lo2, Err.of(np.float32(INFINITY)))
    return dict(ok=h1 & h2, t1=t1, t2=t2, path=P)


def _quad_fields(quads):
    q = np.ascontiguousarray(quads).view(np.float32).reshape(-1, 20).astype(np.float64)
    f = lambda k: [Err(q[:, k + i]) for i in range(3)]   # noqa: E731
    return dict(normal=f(0), d=Err(q[:, 3]), q=f(4), u=f(8), v=f(12))


def _hit_quad(P, live, o, d, Q, tmin, tmax):
    """hitting.glsl:90-133 up to :123.  Returns (hit, t, alpha, beta)."""
    denom = _dot(Q["normal"], d)                              # :92
    small, m = lt(denom.abs(), Err.of(np.float32(1e-8)))      # :95
    P.need(denom, live=live)
    P.take(m, live)
    live = live & ~small
    t = (Q["d"] - _dot(Q["normal"], o)) / denom               # :99
    P.need(t, live=live)
    live = live & _contains(tmin, tmax, t, P, live)           # :100
    inter = [o[k] + d[k] * t for k in range(3)]               # :104
    ph = [inter[k] - Q["q"][k] for k in range(3)]             # :105
    u, v = Q["u"], Q["v"]
    x, y, z = 0, 1, 2
    alpha = beta = None
    chosen = np.zeros(live.shape, bool)
    for a_, b_ in ((x, y), (x, z), (y, z)):                   # :111, :114, :117
        delta = u[a_] * v[b_] - u[b_] * v[a_]
        al = (ph[a_] * v[b_] - ph[b_] * v[a_]) / delta        # :112 / :115 / :119
        be = (ph[b_] * u[a_] - ph[a_] * u[b_]) / delta        # :113 / :116 / :120
        if (a_, b_) == (y, z):
            use = ~chosen                                      # the else branch: no test of delta
        else:
            zero, m = le(delta.abs(), 0.0)                     # delta != 0
            P.take(m, live & ~chosen)
            use = ~chosen & ~zero
        alpha = al if alpha is None else pick(use, al, alpha)
        beta = be if beta is None else pick(use, be, beta)
        chosen = chosen | use
    P.need(alpha, beta, live=live)
    ia = _contains(0.0, 1.0, alpha, P, live)                  # :83
    ib = _contains(0.0, 1.0, beta, P, live & ia)
    return live & ia & ib, t, alpha, beta


def hit_quad(quads, rows):
    """hit_quad (hitting.glsl:90-133) per row: dict(hit, t, alpha, beta, path); alpha / beta are
    hit_record.uv, defined on a hit only (a rejected face leaves the record's uv alone, :83-87)."""
    rows = np.asarray(rows, np.float32)
    n = rows.shape[0]
    P = Path(n)
    hit, t, al, be = _hit_quad(P, np.ones(n, bool), _vec(rows[:, 0:3]), _vec(rows[:, 3:6]), _quad_fields(quads),
                               Err.of(rows[:, 6]), Err.of(rows[:, 7]))
    return dict(hit=hit, t=t, alpha=al, beta=be, path=P)


def hit_box(boxes, rows):
    """hit_box (hitting.glsl:135-146): the six sides in order, ray_t.max shrinking to each accepted
    side's t; the record ends with the last accepted side's t and uv.  dict(hit, t, face, alpha, beta,
    path)."""
    rows = np.asarray(rows, np.float32)
    n = rows.shape[0]
    P = Path(n)
    b = np.ascontiguousarray(boxes).view(np.float32).reshape(n, 6, 20)
    o, d = _vec(rows[:, 0:3]), _vec(rows[:, 3:6])
    tmin, tmax = Err.of(rows[:, 6]), Err.of(rows[:, 7])
    has = np.zeros(n, bool)
    face = np.zeros(n, np.int32)
    t = al = be = Err(np.zeros(n))
    for i in range(6):                                        # :138
        h, ti, ai, bi = _hit_quad(P, np.ones(n, bool), o, d, _quad_fields(b[:, i]), tmin, tmax)   # :139
        tmax = pick(h, ti, tmax)                              # :140
        t, al, be = pick(h, ti, t), pick(h, ai, al), pick(h, bi, be)
        face = np.where(h, i, face)
        has |= h                                              # :141
    return dict(hit=has, t=t, face=face, alpha=al, beta=be, path=P)


def _hit_aabb(P, live, o, d, bx, mn, mx):
    """hit_aabb (hitting.glsl:55-76) on the box bx = [xmin, xmax, ymin, ymax, zmin, zmax] (Err each) over
    ray_t = (mn, mx).  Returns the rows of `live` that hit."""
    n = live.shape[0]
    for axis in range(3):                                     # :56
        with np.errstate(all="ignore"):
            adinv = Err(np.ones(n)) / d[axis]                 # :58
            t0 = (bx[2 * axis] - o[axis]) * adinv             # :60
            t1 = (bx[2 * axis + 1] - o[axis]) * adinv         # :61
            # 1 / +-0 is the same infinity in either precision, and a difference times it the same infinity
            # too wherever the difference's sign is beyond its error: no bound to carry (inf * e is not one)
            flat = np.isinf(adinv.v) & (adinv.e == 0.0)
            for tt, plane in ((t0, bx[2 * axis]), (t1, bx[2 * axis + 1])):
                diff = plane - o[axis]
                tt.e = np.where(flat & (np.abs(diff.v) > diff.bound()), 0.0, tt.e)
        P.need(adinv, t0, t1, live=live, inf_ok=True)
        with np.errstate(invalid="ignore"):
            P.scope &= ~(live & (np.isnan(t0.e) | np.isnan(t1.e)))
            order = t0.v < t1.v                               # :63
            near, far = select(order, t0, t1), select(order, t1, t0)
            mn = select(near.v > mn.v, near, mn)              # :64 / :67
            mx = select(far.v < mx.v, far, mx)                # :65 / :68
        miss, m = le(mx, mn)                                  # :71
        P.take(m, live)
        live = live & ~miss
    return live


def hit_aabb(box6, rows):
    """hit_aabb (hitting.glsl:55-76).  dict(hit, path).  In scope: finite slab values (a zero direction
    component with the origin on its slab plane gives NaN: device against oracle only)."""
    rows = np.asarray(rows, np.float32)
    n = rows.shape[0]
    P = Path(n)
    bx = np.asarray(box6, np.float32).astype(np.float64).reshape(n, 6)
    hit = _hit_aabb(P, np.ones(n, bool), _vec(rows[:, 0:3]), _vec(rows[:, 3:6]), [Err(bx[:, k]) for k in range(6)],
                    Err.of(rows[:, 6]), Err.of(rows[:, 7]))
    return dict(hit=hit, path=P)


# ------------------------------------------------------------------------------------------ texture.glsl
def checker_parity(scale, p):
    """checkerboard's parity (texture.glsl:8-11): ivec3(p * (1 / scale)) truncates toward zero, the sum
    wraps as a 32-bit int, even when (sum % 2) == 0.  dict(odd, path).  In scope: |p / scale| < 2^31
    (the conversion of a larger float to int is undefined in GLSL).  A coordinate's decision is its
    distance to the nearest non-zero integer, where the truncation changes."""
    p = np.asarray(p, np.float32).reshape(-1, 3)
    n = p.shape[0]
    P = Path(n)
    inv = Err(np.ones(n)) / Err.of(np.broadcast_to(np.asarray(scale, np.float32), (n,)))   # :8
    s = np.zeros(n, np.int64)
    for k in range(3):
        q = Err.of(p[:, k]) * inv                                                         # :10
        with np.errstate(invalid="ignore"):
            P.scope &= np.abs(q.v) < 2.0 ** 31
            qv = np.where(np.abs(q.v) < 2.0 ** 31, q.v, 0.0)
        lo, hi = np.floor(qv), np.floor(qv) + 1.0
        lo_d = np.where(lo == 0.0, np.inf, np.abs(qv - lo))      # crossing 0 does not change trunc
        hi_d = np.where(hi == 0.0, np.inf, np.abs(hi - qv))
        P.take(_cmp(np.minimum(lo_d, hi_d), q.bound()))
        s += np.trunc(qv).astype(np.int64)
    s = ((s + 2 ** 31) % 2 ** 32) - 2 ** 31                      # 32-bit wrap
    return dict(odd=(s % 2) != 0, path=P)


def _fade(x):
    return x * x * (Err(np.full(x.v.shape, 3.0)) - Err(np.full(x.v.shape, 2.0)) * x)


def perlin_turb(table, p, depth=7):
    """noise_turb (texture.glsl:79-90) of noise (:38-77) and perlin_interp (:19-36) on the 6 x 256
    table (row r: ranvec x y z, perm_x, perm_y, perm_z).  The fade is applied in noise (:42-44) and
    again in perlin_interp (:20-22).  dict(turb (Err), path).  In scope: |p| 2^(depth-1) < 2^31."""
    tab = np.asarray(table, np.float32).astype(np.float64).reshape(256, 6)
    p = np.asarray(p, np.float32).reshape(-1, 3)
    n = p.shape[0]
    P = Path(n)
    with np.errstate(invalid="ignore"):
        P.scope &= (np.abs(p.astype(np.float64)) * 2.0 ** (depth - 1) < 2.0 ** 31).all(axis=1)
    q = [Err(np.where(P.scope, p[:, k].astype(np.float64), 0.0)) for k in range(3)]
    one = Err(np.ones(n))
    accum, weight = Err(np.zeros(n)), 1.0
    perm = tab[:, 3:6].astype(np.int64)
    for _ in range(depth):                                        # :83
        fl = [np.floor(x.v) for x in q]
        u, v, w = [_fade(q[k] - Err(fl[k])) for k in range(3)]    # :39-44
        ijk = [f.astype(np.int64) for f in fl]                    # :46-48
        uu, vv, ww = _fade(u), _fade(v), _fade(w)                 # :20-22
        acc = Err(np.zeros(n))
        for i in range(2):
            for j in range(2):
                for k in range(2):
                    idx = perm[(ijk[0] + i) & 255, 0] ^ perm[(ijk[1] + j) & 255, 1] ^ perm[(ijk[2] + k) & 255, 2]
                    inside = (idx >= 0) & (idx < 256)             # texelFetch outside the texture reads 0
                    c = [Err(np.where(inside, tab[np.clip(idx, 0, 255), a], 0.0)) for a in range(3)]
                    wv = [u - Err(np.full(n, float(i))), v - Err(np.full(n, float(j))), w - Err(np.full(n, float(k)))]
                    fi, fj, fk = (Err(np.full(n, float(x))) for x in (i, j, k))
                    acc = acc + (fi * uu + (one - fi) * (one - uu)) * (fj * vv + (one - fj) * (one - vv)) * \
                        (fk * ww + (one - fk) * (one - ww)) * _dot(c, wv)   # :29-32
        accum = accum + Err(np.full(n, weight)) * acc             # :84
        weight *= 0.5                                             # :85
        q = [x * Err(np.full(n, 2.0)) for x in q]                 # :86
    return dict(turb=accum.abs(), path=P)                         # :89


# The accuracy tests/test_oracle.py holds the project's GLSL built-ins to (GLSL leaves them to the driver):
INVERSESQRT_ULP, ACOS_ULP, ATAN2_ABS = 2.0, 3.0, 4e-7


def _ulp(v):
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def sphere_uv(p):
    """get_sphere_uv (texture.glsl:96-110): p = normalize(p), theta = acos(-p.y), phi = atan(-p.z, p.x)
    + PI, uv = (phi / (2 PI), theta / PI) with PI = 3.14159265359 as a float.  dict(u, v (Err), path).
    The built-ins' own errors are the bounds tests/test_oracle.py asserts for them (inversesqrt 2 ulp,
    acos 3 ulp, atan 4e-7 absolute), propagated through their derivatives: acos' by
    1 / sqrt(1 - y^2), atan's by 1 / (x^2 + z^2).  At the -x seam with z = +-0 the sign of zero decides
    phi = 0 or 2 PI: float64 keeps it."""
    p = np.asarray(p, np.float32).reshape(-1, 3)
    n = p.shape[0]
    P = Path(n)
    v = _vec(p)
    d2 = _dot(v, v)
    with np.errstate(all="ignore"):
        P.scope &= (d2.v >= F32_MIN) & (d2.v < F32_LIM)
        inv = 1.0 / np.sqrt(d2.v)
        inv = Err(inv, d2.e * inv / (2.0 * d2.v) + INVERSESQRT_ULP * _ulp(inv), d2.n + 1)
        q = [x * inv for x in v]                                   # :105
        ny = -q[1]
        th = np.arccos(np.clip(ny.v, -1.0, 1.0))
        # acos' derivative at the nearer end of [y - e, y + e]; within 16 e of a pole its Hoelder bound
        # |acos a - acos b| <= (pi / sqrt 2) sqrt |a - b| instead
        ay = np.minimum(np.abs(ny.v) + ny.e, 1.0)
        e_th = np.where(1.0 - np.abs(ny.v) > 16.0 * ny.e, ny.e / np.sqrt(1.0 - ay * ay), 2.2215 * np.sqrt(ny.e))
        theta = Err(th, e_th + ACOS_ULP * _ulp(th), ny.n + 1)      # :106
        nz = -q[2]
        at = np.arctan2(nz.v, q[0].v)
        r2 = nz.v * nz.v + q[0].v * q[0].v
        at = Err(at, (np.abs(q[0].v) * nz.e + np.abs(nz.v) * q[0].e) / r2 + ATAN2_ABS, max(nz.n, q[0].n) + 1)
        phi = at + Err(np.full(n, PI))                             # :107
        two_pi = Err(np.full(n, 2.0)) * Err(np.full(n, PI))
        P.scope &= np.isfinite(theta.e)
        # at a pole (x = z = 0) phi, so u, is not determined by p: u_scope False there
        return dict(u=phi / two_pi, v=theta / Err(np.full(n, PI)), u_scope=P.scope & np.isfinite(phi.e), path=P)   # :109


def texture_bilinear(fmt, w, h, texels, uv):
    """texture2D(sampler, uv).rgb under GL_LINEAR and GL_CLAMP_TO_EDGE (Texture.java:74-77; the
    OpenGL 4.6 specification, 8.14.2-3): u' = u W, i0 = floor(u' - 1/2), i1 = i0 + 1, both clamped to
    [0, W - 1], alpha = frac(u' - 1/2), likewise j and beta, and the result (1 - alpha)(1 - beta) t00 +
    alpha (1 - beta) t10 + (1 - alpha) beta t01 + alpha beta t11, evaluated as a lerp of two lerps.  An
    RGBA8 / RGB8 component is c / 255 (correctly rounded), an R32F texel (r, 0, 0).  dict(rgb: 3 Err, path).
    The filter is continuous across a texel boundary, so a float32 floor() that falls on the other
    side of one changes the result by no more than the propagated error of u' - 1/2.
    In scope: |u W|, |v H| < 2^31."""
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    n = uv.shape[0]
    P = Path(n)
    t = np.asarray(texels)
    if fmt == 3:
        tex = np.zeros((h, w, 3))
        tex[..., 0] = t.view(np.float32).reshape(h, w).astype(np.float64)
        tex = [Err(tex[..., c]) for c in range(3)]
    else:
        comps = 3 if fmt == 1 else 4
        b = t.view(np.uint8).reshape(h, w, comps)[..., :3].astype(np.float64)
        tex = [Err(b[..., c]) / Err(np.full((h, w), 255.0)) for c in range(3)]
    half, one = Err(np.full(n, 0.5)), Err(np.ones(n))
    x = Err.of(uv[:, 0]) * Err(np.full(n, float(w))) - half
    y = Err.of(uv[:, 1]) * Err(np.full(n, float(h))) - half
    with np.errstate(invalid="ignore"):
        P.scope &= (np.abs(x.v) < 2.0 ** 31) & (np.abs(y.v) < 2.0 ** 31)
    xv, yv = np.where(P.scope, x.v, 0.0), np.where(P.scope, y.v, 0.0)
    fx, fy = np.floor(xv), np.floor(yv)
    a, b_ = Err(xv, x.e, x.n) - Err(fx), Err(yv, y.e, y.n) - Err(fy)
    i0 = np.clip(fx, 0, w - 1).astype(np.int64)
    i1 = np.clip(fx + 1, 0, w - 1).astype(np.int64)
    j0 = np.clip(fy, 0, h - 1).astype(np.int64)
    j1 = np.clip(fy + 1, 0, h - 1).astype(np.int64)
    rgb = []
    for c in range(3):
        T = tex[c]
        g = lambda j, i: Err(T.v[j, i], T.e[j, i], T.n)   # noqa: E731
        top = g(j0, i0) * (one - a) + g(j0, i1) * a
        bot = g(j1, i0) * (one - a) + g(j1, i1) * a
        rgb.append(top * (one - b_) + bot * b_)
    return dict(rgb=rgb, path=P)

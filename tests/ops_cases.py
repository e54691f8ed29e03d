"""Input batches for the per-operation tests (test infrastructure): tests/test_ops_ref64.py puts them
through the CPU oracle and the float64 reference, tests/test_gpu_ops.py through rt_debug_eval_op and
the oracle.  A batch is the rows of one launch (rt_debug.h: 12 floats per row) with their records.

kind "random": a seeded random set (at most 2^17 rows) whose distributions keep most rows away from
               the deciding comparisons (at most 10 % may be undecided in float64);
kind "edge":   the smallest inputs at which the op can still go wrong, on binary fractions, so that
               float64 decides every row that is in its scope;
kind "near":   neighbours of those edges (the float on either side, rotated boxes, ...): float64
               cannot decide them all, the device and the oracle still have to agree bit for bit.
fd: what the host prep must report for the records (flags[0]); out_rows: the rows the host must report
outside the fd sphere regime (flags[3]); compact: every box record compact (forms 2..4 valid).
The quad and box "one_lane_out" batches: in every wave lane 17's alpha numerator is non-zero and below
2^-100 (face_interior's and box_test_compact_q's wave-wide fallback to '/'), the other 63 lanes' numerators
are far above it; the hook cannot see numerators, so the tests compute them from the rows
(lanes_out_of_regime).
"""
import numpy as np

import pyoracle

F32 = np.float32
INF = F32(3.402823e38)   # compute.glsl:7
TMIN = F32(0.001)


def up(x):
    return np.nextafter(F32(x), F32(np.inf))


def dn(x):
    return np.nextafter(F32(x), F32(-np.inf))


class Batch:
    def __init__(self, name, op, kind, rows, recs=None, tex=None, fd=None, out_rows=None, compact=None, delta=None):
        self.name, self.op, self.kind = name, op, kind
        self.delta = delta   # quad / box one_lane_out: the hit face's delta per row (numerator = alpha, beta x delta)
        self.rows = np.ascontiguousarray(rows, F32)
        self.recs = None if recs is None else np.ascontiguousarray(recs)
        self.tex, self.fd, self.out_rows, self.compact = tex, fd, out_rows, compact
        assert self.rows.shape[0] <= 2 ** 17

    def __repr__(self):
        return f"{self.op}:{self.name}"


# ------------------------------------------------------------------------------------------ records
def sphere_recs(c1, cv, r):
    c1 = np.asarray(c1, F32).reshape(-1, 3)
    n = c1.shape[0]
    s = np.zeros((n, 12), F32)
    s[:, 0:3] = c1
    s[:, 4:7] = np.broadcast_to(np.asarray(cv, F32), (n, 3))
    s[:, 7] = r
    return s


def quad_recs(q, u, v):
    """rt_quad records as Quad.java:23-41 builds them, in float32: normal = unit(u x v), d = normal . q."""
    q, u, v = (np.asarray(a, F32).reshape(-1, 3) for a in (q, u, v))
    n = np.cross(u, v).astype(F32)
    ln = np.sqrt((n * n).sum(axis=1, dtype=F32)).astype(F32)
    with np.errstate(all="ignore"):
        normal = (n / ln[:, None]).astype(F32)
    rec = np.zeros((q.shape[0], 20), F32)
    rec[:, 0:3] = normal
    rec[:, 3] = (normal * q).sum(axis=1, dtype=F32)
    rec[:, 4:7], rec[:, 8:11], rec[:, 12:15], rec[:, 15] = q, u, v, ln
    return rec


def box_recs(mn, mx, rot_y=None, translate=None):
    """6 rt_quad per box in Box.java:19-37's order; rot_y = (cos, sin) turns every side about y first."""
    mn, mx = np.asarray(mn, F32).reshape(-1, 3), np.asarray(mx, F32).reshape(-1, 3)
    n = mn.shape[0]
    z = np.zeros(n, F32)
    dx = np.stack([mx[:, 0] - mn[:, 0], z, z], 1)
    dy = np.stack([z, mx[:, 1] - mn[:, 1], z], 1)
    dz = np.stack([z, z, mx[:, 2] - mn[:, 2]], 1)
    P = lambda a, b, c: np.stack([a, b, c], 1)   # noqa: E731
    sides = [(P(mn[:, 0], mn[:, 1], mx[:, 2]), dx, dy), (P(mx[:, 0], mn[:, 1], mx[:, 2]), -dz, dy),
             (P(mx[:, 0], mn[:, 1], mn[:, 2]), -dx, dy), (P(mn[:, 0], mn[:, 1], mn[:, 2]), dz, dy),
             (P(mn[:, 0], mx[:, 1], mx[:, 2]), dx, -dz), (P(mn[:, 0], mn[:, 1], mn[:, 2]), dx, dz)]
    out = np.zeros((n, 6, 20), F32)
    for i, (q, u, v) in enumerate(sides):
        if rot_y is not None:
            c, s = F32(rot_y[0]), F32(rot_y[1])
            R = lambda a: np.stack([c * a[:, 0] + s * a[:, 2], a[:, 1], -s * a[:, 0] + c * a[:, 2]], 1).astype(F32)  # noqa: E731
            q, u, v = R(q) + np.asarray(translate if translate is not None else 0, F32), R(u), R(v)
        out[:, i] = quad_recs(q, u, v)
    return out.reshape(n, 120)


def rows_of(o, d, tmin=TMIN, tmax=INF, time=0.0):
    return pyoracle.op_rows(o, d, tmin, tmax, time)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _perp(rng, a):
    w = np.cross(a, _unit(rng, a.shape[0]))
    return w / np.linalg.norm(w, axis=1, keepdims=True)


# ------------------------------------------------------------------------------------------ spheres
def _sphere_random(rng, n, inside_share, r_max=10.0, far=20.0, d_exp=(-4, 4)):
    c = rng.uniform(-50, 50, (n, 3))
    r = np.exp(rng.uniform(np.log(0.1), np.log(r_max), n))
    moving = rng.random(n) < 0.25
    cv = np.where(moving[:, None], rng.uniform(-1, 1, (n, 3)), 0.0)
    time = np.where(moving, rng.random(n), 0.0).astype(F32)
    centre = c + cv * time[:, None]
    away = _unit(rng, n)
    inside = rng.random(n) < inside_share
    dist = np.where(inside, rng.uniform(0, 0.95, n), np.exp(rng.uniform(np.log(1.5), np.log(far), n))) * r
    o = centre + away * dist[:, None]
    # aimed at the disc seen from o: inside 0.9 r for most rows, a band around the limb for the rest
    k = np.where(rng.random(n) < 0.8, rng.uniform(0, 0.9, n), rng.uniform(0.9, 1.2, n))
    target = centre + _perp(rng, away) * (k * r)[:, None]
    d = target - o
    d *= (np.exp2(rng.uniform(*d_exp, n)) / np.linalg.norm(d, axis=1))[:, None]
    return sphere_recs(c, cv, r), o, d, time, np.linalg.norm(target - o, axis=1) / np.linalg.norm(d, axis=1)


def sphere_batches():
    rng = np.random.default_rng(101)
    n = 2 ** 17
    recs, o, d, time, reach = _sphere_random(rng, n, 0.1)
    tmax = np.where(rng.random(n) < 0.3, reach * rng.uniform(0.5, 1.5, n), INF).astype(F32)
    rows = rows_of(o, d, TMIN, tmax, time)
    out = [Batch("random", "sphere", "random", rows, recs, fd=1, out_rows=0)]
    # one lane per wave with a = dot(d, d) < 2^-60: the other 63 take '/' in the fd forms
    m = 64 * 64
    r2 = rows[:m].copy()
    r2[17::64, 3:6] *= F32(2.0 ** -31) / np.abs(r2[17::64, 3:6]).max(axis=1, keepdims=True)
    out.append(Batch("one_lane_out", "sphere", "random", r2, recs[:m], fd=1, out_rows=64))

    # the ray o = 0, d = (0, 0, -1) against centre (0, 0, -4), r = 1: hb = -4, c = 15, disc = 1, roots 3 and 5
    C, Z = (0, 0, -4), (0, 0, 0)
    E = []   # (c1, cv, r, o, d, tmin, tmax, time)
    E += [(C, Z, 1, (1, 0, 0), (0, 0, -1), TMIN, INF, 0)]            # tangent: disc = 16 - 16 = 0, root 4
    E += [(C, Z, 1.5, C, (0, 0, -2), TMIN, INF, 0)]                  # origin at the centre: roots -+ 3/4
    E += [(C, Z, 1.5, (0, 0, -2.5), (0, 0, -1), TMIN, INF, 0)]       # on the surface: roots 0 and 3
    E += [(C, Z, 1.25, (0, 0.75, -4), (1, 0, 0), TMIN, INF, 0)]      # inside: roots -+ 1
    for tm in (3.0, dn(3.0), up(3.0)):                               # the near root at tmin: strict
        E += [(C, Z, 1, Z, (0, 0, -1), tm, INF, 0)]
    for tx in (5.0, dn(5.0), up(5.0), 3.0, up(3.0)):                 # roots at tmax: strict
        E += [(C, Z, 1, Z, (0, 0, -1), 3.0, tx, 0)]
    E += [(C, Z, 1, Z, (0, 0, -2.0 ** 20), TMIN, INF, 0)]            # a = 2^40: roots 3, 5 x 2^-20
    E += [(C, (0, 0, -2), 1, Z, (0, 0, -1), TMIN, INF, 0), (C, (0, 0, -2), 1, Z, (0, 0, -1), TMIN, INF, 1)]   # time 0, 1
    E += [(C, Z, 0, Z, (0, 0, -1), TMIN, INF, 0)]                    # radius 0: the double root 4
    E += [(C, Z, -1, Z, (0, 0, -1), TMIN, INF, 0), (C, Z, -1.5, C, (0, 0, -2), TMIN, INF, 0)]   # hollow-glass radius
    E += [(C, Z, 1, (3, 0, 0), (0, 0, -1), TMIN, INF, 0)]            # a clear miss: disc = 16 - 24

    def pack(E):
        a = [np.array([e[k] for e in E], F32) for k in range(8)]
        return sphere_recs(a[0], a[1], a[2]), rows_of(a[3], a[4], a[5], a[6], a[7])
    recs, rows = pack(E)
    out.append(Batch("edges", "sphere", "edge", rows, recs, fd=1, out_rows=0))
    recs, rows = pack([(C, Z, 1, Z, (0, 0, -2.0 ** -31), TMIN, INF, 0),      # a = 2^-62: '/' (roots 3, 5 x 2^31)
                       (C, Z, 1, Z, (0, 0, -1), TMIN, INF, 0)])
    out.append(Batch("edges_tiny_a", "sphere", "edge", rows, recs, fd=1, out_rows=1))
    N = [(C, Z, 1, (up(1.0), 0, 0), (0, 0, -1), TMIN, INF, 0), (C, Z, 1, (dn(1.0), 0, 0), (0, 0, -1), TMIN, INF, 0),
         (C, (0, 0, -2), 1, Z, (0, 0, -1), TMIN, INF, dn(1.0)),                  # time: the float below 1
         (C, Z, 1, Z, (0, 0, 0), TMIN, INF, 0),                                  # d = 0: a = 0
         (C, Z, 2.0 ** 20, Z, (0, 0, -1), TMIN, INF, 0)]                         # a radius outside the fd regime
    recs, rows = pack(N)
    out.append(Batch("near", "sphere", "near", rows, recs, fd=0, out_rows=1))
    return out


def medium_sphere_batches():
    rng = np.random.default_rng(202)
    n = 2 ** 17
    # the second boundary hit starts 0.0001 past the first: decidable only while a root's rounding error stays
    # well below that, so the roots are kept small (radius <= 2, origin within 3 r, |d| >= 1)
    recs, o, d, time, _ = _sphere_random(rng, n, 0.35, r_max=2.0, far=3.0, d_exp=(0, 4))
    rows = rows_of(o, d, TMIN, INF, time)
    out = [Batch("random", "medium_sphere", "random", rows, recs, fd=1, out_rows=0)]
    m = 64 * 64
    r2 = rows[:m].copy()
    r2[5::64, 3:6] *= F32(2.0 ** -31) / np.abs(r2[5::64, 3:6]).max(axis=1, keepdims=True)
    out.append(Batch("one_lane_out", "medium_sphere", "random", r2, recs[:m], fd=1, out_rows=64))
    C, Z = (0, 0, -4), (0, 0, 0)
    E = [(C, 1, (1, 0, 0), (0, 0, -1)),            # tangent: r_lo == r_hi = 4, the second hit fails
         (C, 1, Z, (0, 0, -1)),                    # the chord 3 .. 5
         (C, 1, Z, (0, 0, -2.0 ** 20)),            # a chord of 2^-19 < 0.0001: the second hit fails
         (C, 1, Z, (0, 0, -2.0 ** 14)),            # a chord of 2^-13 > 0.0001
         (C, 1.5, C, (0, 0, -2)),                  # origin at the centre: -3/4 .. 3/4
         (C, 1.25, (0, 0.75, -4), (1, 0, 0)),      # origin inside
         (C, 1, (3, 0, 0), (0, 0, -1))]            # a miss
    a = [np.array([e[k] for e in E], F32) for k in range(4)]
    out.append(Batch("edges", "medium_sphere", "edge", rows_of(a[2], a[3]), sphere_recs(a[0], Z, a[1]), fd=1, out_rows=0))
    N = [(C, 1, Z, (0, 0, 0)), (C, 1, (up(1.0), 0, 0), (0, 0, -1)), (C, 1, (dn(1.0), 0, 0), (0, 0, -1)),
         (C, 1, Z, (0, 0, -2.0 ** -31))]
    a = [np.array([e[k] for e in N], F32) for k in range(4)]
    out.append(Batch("near", "medium_sphere", "near", rows_of(a[2], a[3]), sphere_recs(a[0], Z, a[1]), fd=1, out_rows=2))
    return out


# ------------------------------------------------------------------------------------------ quads, boxes
def quad_batches():
    rng = np.random.default_rng(303)
    n = 2 ** 17
    q = rng.uniform(-20, 20, (n, 3))
    u = _unit(rng, n) * rng.uniform(1, 10, (n, 1))
    v = _unit(rng, n) * rng.uniform(1, 10, (n, 1))
    case = rng.integers(0, 6, n)          # 0..3 general (xy), 4 u.y = v.y = 0 (xz), 5 u.x = v.x = 0 (yz)
    u[case == 4, 1] = 0
    v[case == 4, 1] = 0
    u[case == 5, 0] = 0
    v[case == 5, 0] = 0
    ab = np.where(rng.random((n, 2)) < 0.8, rng.uniform(0.05, 0.95, (n, 2)), rng.uniform(-0.2, 1.2, (n, 2)))
    target = q + u * ab[:, :1] + v * ab[:, 1:]
    o = target + _unit(rng, n) * rng.uniform(1, 40, (n, 1))
    d = (target - o) * np.exp2(rng.uniform(-3, 3, (n, 1)))
    reach = np.linalg.norm(target - o, axis=1) / np.linalg.norm(d, axis=1)
    tmax = np.where(rng.random(n) < 0.2, rng.uniform(0.5, 1.5, n) * reach, INF).astype(F32)
    out = [Batch("random", "quad", "random", rows_of(o, d, TMIN, tmax), quad_recs(q, u, v), fd=1)]

    # a sheared parallelogram in each projection case, hit from the origin at alpha, beta in {0, 1/2, 1}: the
    # plane is 4 away, d = the target, so t = 1 and every product is a binary fraction
    E = []
    perm = {"xy": (0, 1, 2), "xz": (0, 2, 1), "yz": (2, 0, 1)}
    for name, p in perm.items():
        P = lambda a: tuple(np.array(a, F32)[list(p)])   # noqa: E731
        Q, Uv, Vv = P((1, 2, -4)), P((2, 0.5, 0)), P((0.5, 2, 0))
        for a in (0.0, 0.5, 1.0, -0.25, 1.25):
            for b in (0.0, 0.5, 1.0, 1.25):
                tgt = np.array(Q, F32) + F32(a) * np.array(Uv, F32) + F32(b) * np.array(Vv, F32)
                E.append((Q, Uv, Vv, (0, 0, 0), tuple(tgt), TMIN, INF))
        for tm in (1.0, dn(1.0), up(1.0)):         # t = 1 at tmin: inclusive
            E.append((Q, Uv, Vv, (0, 0, 0), tuple(np.array(Q, F32) + np.array(Uv, F32) * F32(0.5)), tm, INF))
        for tx in (1.0, dn(1.0)):                  # and at tmax: inclusive
            E.append((Q, Uv, Vv, (0, 0, 0), tuple(np.array(Q, F32) + np.array(Uv, F32) * F32(0.5)), TMIN, tx))
    # |denom| = |d.z| at the 1e-8 cut, one float under and over (normal (0, 0, 1); the plane z = 0 is 2^-30 ahead)
    c = F32(1e-8)
    for dz in (c, dn(c), up(c), -c, -dn(c), -up(c), 0.0, -0.0):
        E.append(((-8, -8, 0), (16, 0, 0), (0, 16, 0), (0, 0, -(2.0 ** -30) * np.sign(dz if dz else 1)), (0.25, 0.5, dz),
                  TMIN, INF))
    a = [np.array([e[k] for e in E], F32) for k in range(7)]
    out.append(Batch("edges", "quad", "edge", rows_of(a[3], a[4], a[5], a[6]), quad_recs(a[0], a[1], a[2]), fd=1))
    # an extent past 2^20 (the hook reports fd 0) and a degenerate quad (delta = 0 in every projection)
    N = [((-8, -8, -1.1 * 2 ** 20), (16, 0, 0), (0, 16, 0), (0, 0, 0), (0, 0, -1), TMIN, INF),
         ((0, 0, -4), (1, 0, 0), (2, 0, 0), (0, 0, 0), (0.5, 0, -4), TMIN, INF),
         ((1, 2, -4), (2, 0.5, 0), (0.5, 2, 0), (0, 0, 0), (up(1.0), 2, -4), TMIN, INF),
         ((1, 2, -4), (2, 0.5, 0), (0.5, 2, 0), (0, 0, 0), (dn(1.0), 2, -4), TMIN, INF)]
    a = [np.array([e[k] for e in N], F32) for k in range(7)]
    out.append(Batch("near", "quad", "near", rows_of(a[3], a[4], a[5], a[6]), quad_recs(a[0], a[1], a[2]), fd=0))
    DX, d = tiny_numerator_rows()
    k = len(DX)
    z = np.zeros(k, F32)
    out.append(Batch("one_lane_out", "quad", "near", rows_of(np.zeros((k, 3)), d),
                     quad_recs(np.tile(F32([0, -1, -4]), (k, 1)), np.stack([DX, z, z], 1), np.tile(F32([0, 2, 0]), (k, 1))),
                     fd=1, delta=DX * F32(2)))
    return out


def tiny_numerator_rows(n_waves=512):
    """Rays from the origin onto the face q = (0, -1, -4), u = (DX, 0, 0), v = (0, 2, 0) (a canonical box's
    front face with mn.x = 0): t = 4, pa = 4 d.x, so alpha's numerator is 2 pa and alpha = pa / DX.  Lane 17
    of every wave has d.x = m 2^-k (k = 105 .. 140, m in [1, 2)): numerators from 2^-101 down into the
    subnormals, where the shared-reciprocal quotient's residual underflows and it is no longer the rounded
    quotient; DX is random in [3, 1000], in odd waves x 2^-20 (no power of two: an inexact reciprocal).  The
    other lanes hit at x = 0.1 .. 0.73 DX.  Returns (DX [n], d [n, 3])."""
    rng = np.random.default_rng(1717)
    n = 64 * n_waves
    lane = np.arange(n) % 64
    wave = np.arange(n) // 64
    # odd waves: faces 2^-20 as wide, delta = 2 DX around 2^-14 -- a tiny numerator over a small delta is a normal
    # quotient whose residual num - delta q underflows
    DX = (rng.uniform(3, 1000, n) * np.where(wave % 2 == 1, 2.0 ** -20, 1.0)).astype(F32)
    d = np.stack([(0.1 + 0.01 * lane) * DX / 4, -0.2 + 0.006 * lane, -np.ones(n)], 1).astype(F32)
    k = 105 + wave[lane == 17] % 36
    d[lane == 17, 0] = (rng.uniform(1, 2, n_waves) * np.exp2(-k.astype(np.float64))).astype(F32)
    return DX, d


def lanes_out_of_regime(batch):
    """For a quad / box one_lane_out batch, from its rows: the rows whose alpha or beta numerator -- 2 pa and
    DX pb with pa = 4 d.x, pb = 4 d.y + 1 at t = 4 -- is below 2^-100; every numerator is non-zero."""
    d = batch.rows[:, 3:6].astype(np.float64)
    assert (batch.rows[:, 0:3] == 0).all() and (d[:, 2] == -1).all()
    na, nb = np.abs(4 * d[:, 0] * 2), np.abs((4 * d[:, 1] + 1) * batch.delta / 2)
    assert (na > 0).all() and (nb > 0).all()
    return (na < 2.0 ** -100) | (nb < 2.0 ** -100)


def _box_rays(rng, mn, mx, n):
    ctr, half = (mn + mx) / 2, (mx - mn) / 2
    inside = rng.random(n) < 0.15
    o = ctr + np.where(inside[:, None], rng.uniform(-0.9, 0.9, (n, 3)) * half,
                       _unit(rng, n) * (np.linalg.norm(half, axis=1, keepdims=True) * rng.uniform(1.5, 8, (n, 1))))
    target = ctr + rng.uniform(-1.3, 1.3, (n, 3)) * half
    return o, (target - o) * np.exp2(rng.uniform(-3, 3, (n, 1)))


def box_batches():
    rng = np.random.default_rng(404)
    n = 2 ** 16
    mn = rng.uniform(-20, 20, (n, 3))
    mx = mn + rng.uniform(0.5, 10, (n, 3))
    o, d = _box_rays(rng, mn, mx, n)
    out = [Batch("random", "box", "random", rows_of(o, d), box_recs(mn, mx), fd=1, compact=True)]
    m = 2 ** 14
    ang = 0.5
    R = lambda a: np.stack([np.cos(ang) * a[:, 0] + np.sin(ang) * a[:, 2], a[:, 1],   # noqa: E731
                            -np.sin(ang) * a[:, 0] + np.cos(ang) * a[:, 2]], 1)
    out.append(Batch("random_rotated", "box", "random", rows_of(R(o[:m]), R(d[:m])),
                     box_recs(mn[:m], mx[:m], rot_y=(np.cos(ang), np.sin(ang))), fd=1, compact=False))

    # adversarial.edges()'s box 1: (-2, -1, -8) .. (2, 1, -4) from the origin; d = (x, y, -1) meets its front
    # face z = -4 at (4 x, 4 y): the edges at x = +-1/2, y = +-1/4
    MN, MX = (-2, -1, -8), (2, 1, -4)
    E = []
    for x in (-0.5, 0.0, 0.25, 0.5, 0.75):
        for y in (-0.25, 0.0, 0.25, 0.5):
            E.append((MN, MX, (0, 0, 0), (x, y, -1)))
    E += [(MN, MX, (0, 0, -6), dd) for dd in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, -0.5, 0.25), (0.5, 0.25, 1))]  # inside
    E += [(MN, MX, (0, 1, 0), (0, 0, -1)), (MN, MX, (2, 0, 0), (0, 0, -1)), (MN, MX, (2, 1, 0), (0, 0, -1))]   # in a face plane
    E += [(MN, MX, (0, 0, 0), (0.0, -0.0, -1)), (MN, MX, (0, 0, 0), (-0.0, 0.0, -1)),
          (MN, MX, (0, 0, 0), (1e-40, -1e-40, -1)), (MN, MX, (0, 0, -6), (1e-40, 1, -1e-45))]             # +-0, subnormal
    a = [np.array([e[k] for e in E], F32) for k in range(4)]
    out.append(Batch("edges", "box", "edge", rows_of(a[2], a[3]), box_recs(a[0], a[1]), fd=1, compact=True))
    # the same box scaled by 16 and moved 0.95 / 1.1 x 2^20 down -z (adversarial.extent): fd on / off
    for name, dist, fd in (("extent_inside", 0.95 * 2 ** 20, 1), ("extent_past", 1.1 * 2 ** 20, 0)):
        c = np.array([0, 0, -dist], F32)
        mn_, mx_ = c + F32(16) * np.array(MN, F32), c + F32(16) * np.array(MX, F32)
        dirs = np.array([(x, y, -1) for x in (-0.5, 0.0, 0.25, 0.5, 0.75) for y in (-0.25, 0.0, 0.25, 0.5)], F32) * F32(16)
        k = dirs.shape[0]
        out.append(Batch(name, "box", "near", rows_of(np.tile(c, (k, 1)), dirs),
                         box_recs(np.tile(mn_, (k, 1)), np.tile(mx_, (k, 1))), fd=fd, compact=True))
    # y-rotated by (cos, sin) = (0.6, 0.8): the edges and corners of its front face, hit from the origin
    cs = (F32(0.6), F32(0.8))
    Rf = lambda p: np.array([cs[0] * p[0] + cs[1] * p[2], p[1], -cs[1] * p[0] + cs[0] * p[2]], F32)   # noqa: E731
    pts = [Rf(np.array((x, y, -4), F32)) for x in (-2, 0, 1, 2, 3) for y in (-1, 0, 1, 2)]
    k = len(pts)
    out.append(Batch("rotated_edges", "box", "near", rows_of(np.zeros((k, 3)), np.array(pts)),
                     box_recs(np.tile(np.array(MN, F32), (k, 1)), np.tile(np.array(MX, F32), (k, 1)), rot_y=cs),
                     fd=1, compact=False))
    # canonical boxes (0, -1, -8) .. (DX, 1, -4): the front face is quad_batches' one_lane_out face
    DX, d = tiny_numerator_rows()
    k = len(DX)
    out.append(Batch("one_lane_out", "box", "near", rows_of(np.zeros((k, 3)), d),
                     box_recs(np.tile(F32([0, -1, -8]), (k, 1)), np.stack([DX, np.ones(k, F32), np.full(k, -4, F32)], 1)),
                     fd=1, compact=True, delta=DX * F32(2)))
    return out


# ------------------------------------------------------------------------------------------ BVH nodes
def node_batches():
    rng = np.random.default_rng(505)
    n = 2 ** 17
    mn = rng.uniform(-20, 20, (n, 3))
    mx = mn + rng.uniform(0.1, 10, (n, 3))
    o, d = _box_rays(rng, mn, mx, n)
    reach = np.linalg.norm((mn + mx) / 2 - o, axis=1) / np.linalg.norm(d, axis=1)
    tmax = np.where(rng.random(n) < 0.3, reach * rng.uniform(0.3, 1.5, n), INF).astype(F32)
    b6 = np.stack([mn[:, 0], mx[:, 0], mn[:, 1], mx[:, 1], mn[:, 2], mx[:, 2]], 1).astype(F32)
    out = [Batch("random", "node", "random", rows_of(o, d, TMIN, tmax), b6)]
    B = (-2, 2, -1, 1, -8, -4)
    E = []
    for dd in ((0, 0, -1), (0.0, -0.0, -1), (-0.0, 0.0, -1), (0.5, 0, -1), (0.5, 0.25, -1), (0.75, 0, -1), (0, 0, 1),
               (1, 0, 0), (0, -0.0, 1e-40)):
        for oo in ((0, 0, 0), (2, 0, 0), (-2, 1, 0), (0, 0, -4), (0, 0, -6), (3, 0, 0), (2, 1, -4)):   # on slab planes too
            E.append((B, oo, dd, TMIN, INF))
    for tx in (4.0, dn(4.0), up(4.0)):           # the slab entered at t = 4: hi <= lo
        E.append((B, (0, 0, 0), (0, 0, -1), TMIN, tx))
    for tm in (8.0, dn(8.0), up(8.0)):           # and left at t = 8
        E.append((B, (0, 0, 0), (0, 0, -1), tm, INF))
    Zt = (-2, 2, 1, 1, -8, -4)                   # zero thickness in y
    E += [(Zt, (0, 1, 0), (0, 0, -1), TMIN, INF), (Zt, (0, 0, 0), (0, 0.25, -1), TMIN, INF), (Zt, (0, 0, 0), (0, 0.5, -1), TMIN, INF),
          ((1, 1, 1, 1, -4, -4), (0, 0, 0), (0.25, 0.25, -1), TMIN, INF)]
    # +-inf direction components: 1 / d = +-0, both slab values (mn - o) x 0 are zeros of either sign -- origin
    # inside the slab, outside it and on its planes, with tmin above and below 0
    inf = np.inf
    for dd in ((inf, 0, -1), (-inf, 0, -1), (0.5, inf, -1), (0.5, -inf, -1), (0.5, 0.25, -inf), (0.5, 0.25, inf),
               (inf, -inf, inf), (-inf, -0.0, -1)):
        for oo in ((0, 0, 0), (3, 0, 0), (2, 0, 0), (-2, 1, -6), (0, -1, -4), (0, 0, -8)):
            for tm in (TMIN, -1.0, 0.0, -0.0):
                E.append((B, oo, dd, tm, INF))
    a = [np.array([e[k] for e in E], F32) for k in range(5)]
    out.append(Batch("edges", "node", "edge", rows_of(a[1], a[2], a[3], a[4]), a[0]))
    return out


# ------------------------------------------------------------------------------------------ textures
def perlin_table(seed=7, bad_perm=False):
    """A 6 x 256 table as the builder's (Perlin.java): unit vectors, three permutations of 0..255."""
    rng = np.random.default_rng(seed)
    t = np.zeros((256, 6), F32)
    t[:, 0:3] = _unit(rng, 256)
    for k in range(3):
        t[:, 3 + k] = rng.permutation(256)
    if bad_perm:
        t[9, 4] = 256.0      # the table does not pack; ranvec row 256 ^ ... reads 0 outside the texture
    return t


def perlin_batches():
    rng = np.random.default_rng(606)
    tab = perlin_table()
    tex = (3, 6, 256, tab)
    p = rng.uniform(-100, 100, (2 ** 15, 3))
    out = [Batch("random", "perlin", "random", pyoracle.op_rows(p), tex=tex, compact=True)]
    E = [(0, 0, 0), (1, 2, 3), (-1, -2, -3), (255, 256, 257), (-256, -255, 0.5), (0.5, 0.25, 0.75), (-0.5, -0.25, -0.75),
         (2.0 ** 24, 2.0 ** 24 + 2, -(2.0 ** 24) - 4), (2.0 ** 24 + 6, -(2.0 ** 24) - 2, 2.0 ** 23 + 0.5), (3.999999, -3.999999, 1e-30)]
    out.append(Batch("edges", "perlin", "edge", pyoracle.op_rows(E), tex=tex, compact=True))
    N = [(2.0 ** 31, 0, 0), (-2.0 ** 33, 1.5, 2.5), (1e30, -1e30, 0.5), (np.nan, 0, 0), (0.5, np.nan, np.inf), (2.0 ** 26, 2.0 ** 25, -2.0 ** 30)]
    out.append(Batch("beyond_int", "perlin", "near", pyoracle.op_rows(N), tex=tex, compact=True))
    out.append(Batch("unpackable", "perlin", "random", pyoracle.op_rows(p[:4096]), tex=(3, 6, 256, perlin_table(bad_perm=True)),
                     compact=False))
    return out


def sphere_uv_batches():
    rng = np.random.default_rng(707)
    n = 2 ** 16
    p = _unit(rng, n) * np.exp2(rng.uniform(-8, 8, (n, 1)))
    out = [Batch("random", "sphere_uv", "random", pyoracle.op_rows(p))]
    E = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),          # texture.glsl:100-102
         (-1, 0, 0.0), (-1, 0, -0.0), (1, 0, 0.0), (1, 0, -0.0), (-1, 0.5, -0.0), (-2, 0, 2.0 ** -40), (-2, 0, -2.0 ** -40),
         (0.0, 1, -0.0), (-0.0, -1, 0.0), (2.0 ** -20, 1, 0), (0, -1, 2.0 ** -20),     # the poles and just off them
         (3, 4, 12), (-300, 400, 1200), (2.0 ** -30, 2.0 ** -31, 2.0 ** -30), (2.0 ** 40, 2.0 ** 40, -2.0 ** 41)]
    out.append(Batch("edges", "sphere_uv", "edge", pyoracle.op_rows(E)))
    N = [(1e-30, 1e-30, 1e-30), (0, 0, 0), (1e30, 0, 0), (np.nan, 1, 0), (np.inf, 1, 0), (1e-40, 0, 0)]
    out.append(Batch("tiny_huge", "sphere_uv", "near", pyoracle.op_rows(N)))
    return out


def _uv_rows(uv):
    uv = np.asarray(uv, F32).reshape(-1, 2)
    d = np.zeros((uv.shape[0], 3), F32)
    d[:, :2] = uv
    return pyoracle.op_rows(np.zeros((uv.shape[0], 3), F32), d, word=pyoracle.TEXTYPE_IMAGE << 28)


def texel_batches():
    rng = np.random.default_rng(808)
    out = []
    texs = {"rgba_1x1": (2, 1, 1, rng.integers(0, 256, (1, 1, 4), dtype=np.uint8)),
            "rgba_1x5": (2, 1, 5, rng.integers(0, 256, (5, 1, 4), dtype=np.uint8)),
            "rgba_3x2": (2, 3, 2, rng.integers(0, 256, (2, 3, 4), dtype=np.uint8)),
            "rgb_3x2": (1, 3, 2, rng.integers(0, 256, (2, 3, 3), dtype=np.uint8)),
            "r32f_3x2": (3, 3, 2, rng.uniform(-4, 4, (2, 3)).astype(F32)),
            # every byte value: red = the texel's index, green its complement, blue a shuffle
            "rgba_16x16": (2, 16, 16, np.stack([np.arange(256), 255 - np.arange(256), rng.permutation(256), np.full(256, 255)],
                                               1).astype(np.uint8).reshape(16, 16, 4))}
    for name, tex in texs.items():
        w, h = tex[1], tex[2]
        uv = rng.uniform(-0.1, 1.1, (2 ** 13, 2))
        out.append(Batch(name + "_random", "texture", "random", _uv_rows(uv), tex=tex))
        us = [0.0, 1.0, -0.0, dn(0.0), up(1.0), -0.25, 1.25] + [k / w for k in range(w + 1)] + [(k + 0.5) / w for k in range(w)]
        vs = [0.0, 1.0, dn(0.0), up(1.0), 1.5] + [k / h for k in range(h + 1)] + [(k + 0.5) / h for k in range(h)]
        E = [(F32(u), F32(v)) for u in us for v in vs]
        out.append(Batch(name + "_edges", "texture", "edge", _uv_rows(E), tex=tex))
    N = [(np.nan, 0.5), (0.5, np.nan), (np.inf, 0.5), (-np.inf, -np.inf), (1e30, 0.5), (-1e30, 3e9), (2.0 ** 31, 0.5)]
    out.append(Batch("rgba_3x2_nan", "texture", "near", _uv_rows(N), tex=texs["rgba_3x2"]))
    return out


CHECKER_SCALES = np.array([1.0, 0.5, 0.32, 3.0, 2.0 ** -20, 0.01], F32)


def checker_batches():
    rng = np.random.default_rng(909)
    n = 2 ** 16
    tex = pyoracle.checker_table(CHECKER_SCALES)
    which = rng.integers(0, 4, n)
    p = rng.uniform(-50, 50, (n, 3))
    out = [Batch("random", "texture", "random", pyoracle.checker_rows(p, which), tex=tex)]
    E, W, N, NW = [], [], [], []
    for k in (-3, -2, -1, 0, 1, 2, 3, 7):        # exactly on multiples of the scale: 1 and 1/2 (1 / scale exact), 3 (not)
        for w_, s in ((0, 1.0), (1, 0.5), (3, 3.0)):
            pts = [(k * s, 0.25 * s, 0.25 * s), (0.25 * s, k * s, -0.25 * s), (k * s, k * s, k * s), (-0.75 * s, -0.5 * s, k * s)]
            if w_ == 3:
                N += pts
                NW += [w_] * 4
            else:
                E += pts
                W += [w_] * 4
    for pp in ((-0.25, -0.5, -0.75), (-0.999, 0.999, 0), (-1.5, 1.5, 0), (-1.5, -1.5, -1.5), (-0.0, 0.0, -0.0)):   # toward zero
        E.append(pp)
        W.append(0)
    for pp in ((1500, 1500, 1500), (2047, 2047, 1), (-2047, -2047, -1), (2047.5, 2047.5, 2047.5), (1024, 1024, 0)):   # int sums wrap
        E.append(pp)
        W.append(4)
    out.append(Batch("edges", "texture", "edge", pyoracle.checker_rows(E, np.array(W)), tex=tex))
    out.append(Batch("scale_3", "texture", "near", pyoracle.checker_rows(N, np.array(NW)), tex=tex))
    N = [(2048, 0, 0), (-4096, 1, 1), (1e30, -1e30, 0), (np.nan, 1, 1), (np.inf, 0, 0)]       # beyond int: the conversion saturates
    out.append(Batch("beyond_int", "texture", "near", pyoracle.checker_rows(N, 4), tex=tex))
    return out


def checker_scale_of(batch):
    """The scale of each row of a checker batch (from its texture id's detail bits)."""
    return CHECKER_SCALES[batch.rows.view(np.int32)[:, 9] & 0xFFF]


ALL = {"sphere": sphere_batches, "medium_sphere": medium_sphere_batches, "quad": quad_batches, "box": box_batches,
       "node": node_batches, "perlin": perlin_batches, "sphere_uv": sphere_uv_batches, "texel": texel_batches,
       "checker": checker_batches}

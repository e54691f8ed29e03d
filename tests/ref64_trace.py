"""A float64 reference of ray_color's closest-hit walk, on tests/ref64.py's `Err` / `Path` machinery (its
docstring defines the running rounding bound and the decision margins) and tests/ref64_shade.py's draws.
Written from the reference's shader text -- raytrace/compute.glsl:225-266 (trace_through_bvh) and
utils/hitting.glsl:135-206 (hit_box, hit_boundary, hit_constant_medium, hit_model) over ref64's hit_sphere,
hit_quad and hit_aabb -- not from the oracle or the kernel.  tests/test_trace_ref64.py compares the CPU
oracle's RT_SOP_TRACE with it.

All rows are walked together, level-synchronously: each row has its own int stack[64] and pops one node per
step (compute.glsl:236-238); the rows that popped a node test its box, those that reached a leaf test its
two slots in turn, grouped by prim type.  Each step works on the rows still walking only.

What the walk keeps of the shader:
  * the root is pushed first, the left child before the right one, so the right one is popped first (:259-260);
  * a leaf is a node whose left id has a non-zero type (:241-242); both slots are tested, left then right, the
    second under the ray_t.max the first one left (:247-256), and a leaf the builder gave one prim names it in
    both slots and tests it twice: a medium then draws a second time, a solid prim's second test changes nothing
    (walk() says why it is counted and not evaluated);
  * hit_sphere accepts ray_t.min < t < ray_t.max, hit_quad ray_t.min <= t <= ray_t.max (interval.glsl): of two
    spheres at one t the first visited stays, of two quads the later one replaces it;
  * hit_model (:195-206): hit_boundary first -- a sphere, a quad, a box's six sides in order, each under the
    ray_t.max its predecessor left (:135-146), nothing for any other type -- then, for a constant medium,
    hit_constant_medium: its boundary over (-INFINITY, INFINITY), again from rec1.t + 0.0001 (:165-168), the
    clamps and the one rand() of ref64_shade._medium_tail; rec1 and rec2 are locals, so a medium writes no uv;
  * hit_record is the caller's (an inout): the uv a sphere or a quad (a box side) wrote stays until the next
    such hit writes it, within a walk and from one walk to the next.  Here it is carried as its source --
    (1 << 16 | sphere index, that hit's point p) or (2 << 16, alpha, beta, the third word untouched) -- as
    include/rt/rt_debug.h's UvSrc states it, so that a texture is not evaluated.

Draws are inputs (`seq`, the row's rand() sequence), consumed in visit order; `count` is how many were used.

The result: dict(cls: hit, tif (type | box side << 4 | index << 16, 0 on a miss), uvk (the uv source's kind and
index), count, visits (nodes popped), slots (hit_model calls), hash (the visited indices' FNV-1a, as
oracle/rt_oracle.h fixes it: h = 2166136261, then h = (h ^ index) * 16777619 mod 2^32 per node);
val: t, uva, uvb, uvc (Err); mask; path; relaxed: the rows decided by the relaxed rule (walk() states it); doubted: the
rows that rule had to follow a node test's both outcomes for).  A row is decided when every comparison on its way had margin --
node tests, root selection, t against ray_t, the quad's interior tests, the medium's clamps and its
hit_distance > distance_inside_boundary.  Out of scope: NaN (a zero direction component with the origin on a
slab plane, 0 * inf), values past float32's range, more than 64 stack entries or more draws than `seq` holds.
"""
import numpy as np

from ref64 import INFINITY, Err, Path, _dot, _hit_aabb, _hit_quad, _hit_sphere, _surrounds, lt, pick
from ref64_shade import MODEL_BOX, MODEL_CONSTANT_MEDIUM, MODEL_QUAD, MODEL_SPHERE, _medium_tail

NODE_DT = np.dtype([("box", "<f4", 6), ("left", "<i4"), ("right", "<i4")])   # compute.glsl:117-125
HASH_INIT, HASH_MUL = 2166136261, 16777619
STACK = 64                                                                  # compute.glsl:229
DOUBT_BIT = 20                                                              # of a stack entry here (indices are below 2^16)


def _sub(e, i):
    return Err(e.v[i], e.e[i], e.n)


def _put(dst, i, src, mask):
    """Rows i[mask] of dst take src[mask]."""
    j = i[mask]
    dst.v[j], dst.e[j] = src.v[mask], src.e[mask]
    dst.n = max(dst.n, src.n)


def _const(n, x):
    return Err(np.full(n, float(np.float32(x))))


def _cols(a, ks):
    return [Err(a[:, k].astype(np.float64)) for k in ks]


def _quad_fields(q):
    """rt_quad rows [m, 20] as ref64._hit_quad takes them."""
    return dict(normal=_cols(q, (0, 1, 2)), d=_cols(q, (3,))[0], q=_cols(q, (4, 5, 6)), u=_cols(q, (8, 9, 10)),
                v=_cols(q, (12, 13, 14)))


def _quad(P, live, o, d, Q, tmin, tmax):
    """ref64._hit_quad with the conjunction's margin: hit_quad returns at the first of its tests that fails (denom,
    t in ray_t, alpha, beta) and has no side effect before it hits, so a row that fails one of them decidedly is a
    decided miss whatever the others' margins.  The tests that do not read ray_t are therefore evaluated once more
    over (-INFINITY, INFINITY): where they fail decidedly, they settle it.  (Coplanar faces of neighbouring prims meet a
    ray at one t, bit for bit, and all but one of them fail the interior test by far.)"""
    m = live.shape[0]
    A, B = Path(m), Path(m)
    hit, t, al, be = _hit_quad(A, live, o, d, Q, tmin, tmax)
    inside = _hit_quad(B, live, o, d, Q, _const(m, -INFINITY), _const(m, INFINITY))[0]
    off = live & ~inside & B.decided
    P.take(np.where(off, B.margin, A.margin), live)
    P.scope &= ~live | np.where(off, B.scope, A.scope)
    return hit & ~off, t, al, be


def _hit_box(P, live, o, d, box, tmin, tmax):
    """hit_box (hitting.glsl:135-146) on rt_box rows [m, 6, 20]: (hit, t, side, alpha, beta)."""
    m = live.shape[0]
    has, side = np.zeros(m, bool), np.zeros(m, np.int64)
    t = al = be = Err(np.zeros(m))
    for i in range(6):                                                      # :138
        h, ti, ai, bi = _quad(P, live, o, d, _quad_fields(box[:, i]), tmin, tmax)        # :139
        tmax = pick(h, ti, tmax)                                            # :140
        t, al, be = pick(h, ti, t), pick(h, ai, al), pick(h, bi, be)
        side = np.where(h, i, side)
        has = has | h                                                       # :141
    return has, t, side, al, be


def _hit_boundary(S, P, live, o, d, time, typ, idx, tmin, tmax):
    """hit_boundary (hitting.glsl:148-160) for rows that all hold a prim of type `typ`: (hit, t, side, uv source or
    None).  The uv source is (kind, a, b, c or None): what the hit wrote into hit_record.uv, as its source."""
    m = live.shape[0]
    zero = np.zeros(m, np.int64)
    if typ == MODEL_SPHERE:
        s = S.spheres[idx]
        hit, t = _hit_sphere(P, live, o, d, _cols(s, (0, 1, 2)), _cols(s, (4, 5, 6)), _cols(s, (7,))[0], time, tmin, tmax)
        p = [o[k] + d[k] * t for k in range(3)]                             # hitting.glsl:39
        P.need(*p, live=hit)
        return hit, t, zero, ((1 << 16) | idx, p[0], p[1], p[2])
    if typ == MODEL_QUAD:
        hit, t, al, be = _quad(P, live, o, d, _quad_fields(S.quads[idx]), tmin, tmax)
        return hit, t, zero, (np.full(m, 2 << 16), al, be, None)
    if typ == MODEL_BOX:
        hit, t, side, al, be = _hit_box(P, live, o, d, S.boxes[idx], tmin, tmax)
        return hit, t, side, (np.full(m, 2 << 16), al, be, None)
    return np.zeros(m, bool), Err(np.zeros(m)), zero, None                  # :157-158


def _sphere_bounds(S, P, live, o, d, time, idx):
    """hit_constant_medium's two hit_sphere calls (hitting.glsl:165-168, :17-47) on one pair of roots: (ok, t1, t2).
    The second call computes the roots again from the same ray and sphere -- the same floats -- and asks
    rec1.t + 0.0001 < root.  For the root that gave rec1.t that fails by identity (a rounded x + 0.0001 is not below
    x), which a rounding bound cannot express: at a fog of radius 5000 the bound on a root is far above 0.0001.  So
    that comparison is not evaluated.  When rec1.t is the nearer root the farther one is tried; when it is the farther
    one (the nearer was not finite, and is not again) nothing is left and the medium is missed."""
    m = live.shape[0]
    s = S.spheres[idx]
    c1, cv, radius = _cols(s, (0, 1, 2)), _cols(s, (4, 5, 6)), _cols(s, (7,))[0]
    center = [c1[k] + cv[k] * time for k in range(3)]         # :13-15, :18
    oc = [o[k] - center[k] for k in range(3)]                 # :19
    a = _dot(d, d)                                            # :20
    half_b = _dot(oc, d)                                      # :21
    c = _dot(oc, oc) - radius * radius                        # :22
    disc = half_b * half_b - a * c                            # :23
    P.need(a, half_b, c, disc, live=live)
    neg, mg = lt(disc, 0.0)                                   # :25
    P.take(mg, live)
    live = live & ~neg
    sqrtd = disc.sqrt()                                       # :28
    near, far = (-half_b - sqrtd) / a, (-half_b + sqrtd) / a  # :31, :33
    lo, hi = _const(m, -INFINITY), _const(m, INFINITY)
    P.need(near, live=live)
    in1 = _surrounds(lo, hi, near, P, live)                   # the first call, :32
    P.need(far, live=live & ~in1)
    in2 = _surrounds(lo, hi, far, P, live & ~in1)             # :34
    t1 = pick(in1, near, far)
    again = live & in1                                        # the second call: only the farther root is left
    P.need(far, live=again)
    ok = _surrounds(t1 + _const(m, 0.0001), hi, far, P, again)   # hitting.glsl:168, :34
    del in2
    return again & ok, t1, far


def _hit_medium(S, P, live, o, d, time, idx, tmin, tmax, draw):
    """hit_constant_medium (hitting.glsl:162-193) for rows that all hold a medium: (hit, t)."""
    m = live.shape[0]
    med = S.media[idx]
    b_idx, b_typ = med.view(np.int32)[:, 0].astype(np.int64), med.view(np.int32)[:, 1]
    lo, hi = _const(m, -INFINITY), _const(m, INFINITY)
    ok = np.zeros(m, bool)
    t1, t2 = Err(np.zeros(m)), Err(np.zeros(m))
    for typ in np.unique(b_typ[live]):
        rows = live & (b_typ == typ)
        bi = np.where(rows, b_idx, 0)
        if typ == MODEL_SPHERE:
            both, a1, a2 = _sphere_bounds(S, P, rows, o, d, time, bi)
            t1, t2, ok = pick(rows, a1, t1), pick(rows, a2, t2), ok | both
            continue
        h1, a1, _, _ = _hit_boundary(S, P, rows, o, d, time, int(typ), bi, lo, hi)           # :165
        lo2 = a1 + _const(m, 0.0001)                                                           # :168
        h2, a2, _, _ = _hit_boundary(S, P, h1, o, d, time, int(typ), bi, lo2, hi)
        t1, t2 = pick(rows, a1, t1), pick(rows, a2, t2)
        ok = ok | (h1 & h2)
    a = _dot(d, d)                                                          # length(ray.dir) = sqrt of it, :180
    return _medium_tail(P, draw, ok, Err(med[:, 2].astype(np.float64)), t1, t2, a, tmin, tmax)


def walk(S, nodes, rows, seq):
    """trace_through_bvh (compute.glsl:225-266) over ray_t = [0.001, INFINITY] for rt_debug_eval_shade_op rows
    (o, d, time, the uv source before the walk) on the RefScene S and its BVH `nodes` (the upload's bytes)."""
    rows = np.asarray(rows, np.float32)
    nd = np.frombuffer(bytes(nodes), NODE_DT)
    n = rows.shape[0]
    seq = np.asarray(seq, np.float32).astype(np.float64)
    P = Path(n)
    f64 = rows.astype(np.float64)
    o_all, d_all = [Err(f64[:, k].copy()) for k in range(3)], [Err(f64[:, 3 + k].copy()) for k in range(3)]
    time_all = Err(f64[:, 8].copy())
    tmax = _const(n, INFINITY)
    t = Err(np.zeros(n))
    has, tif = np.zeros(n, bool), np.zeros(n, np.int64)
    uvk = rows.view(np.int32)[:, 15].astype(np.int64)
    uv = [Err(f64[:, 16 + k].copy()) for k in range(3)]
    count = np.zeros(n, np.int64)
    visits, slots = np.zeros(n, np.int64), np.zeros(n, np.int64)
    hsh = np.full(n, HASH_INIT, np.uint64)
    stack = np.zeros((n, STACK), np.int64)                                  # :229-231: stack[0] = 0
    sp = np.ones(n, np.int64) if len(nd) else np.zeros(n, np.int64)
    short, wrote = np.zeros(n, bool), np.zeros(n, bool)
    # The relaxed rule for a node test without margin: both outcomes are followed.  The node is visited, and it and
    # everything pushed from it is marked doubtful (a bit of the stack entry); a row in which a doubtful node's leaf
    # accepted a hit or drew stays undecided (`effect`).  Otherwise skipping any of the doubtful nodes leaves every
    # other test of the walk with the ray_t.max it had, so every outcome of those node tests gives this hit, tif, t,
    # uv and draw sequence; only the visit counts and hash depend on them.  R collects the margins of everything else.
    R = Path(n)
    effect, doubted = np.zeros(n, bool), np.zeros(n, bool)

    while True:
        i = np.nonzero(sp > 0)[0]                                           # :236
        if i.size == 0:
            break
        m = i.size
        sp[i] -= 1
        node = stack[i, sp[i]]                                              # :237
        doubt, node = (node >> DOUBT_BIT) != 0, node & ((1 << DOUBT_BIT) - 1)
        visits[i] += 1
        hsh[i] = ((hsh[i] ^ node.astype(np.uint64)) * np.uint64(HASH_MUL)) & np.uint64(0xFFFFFFFF)
        Q, N = Path(m), Path(m)
        o, d, time = [_sub(x, i) for x in o_all], [_sub(x, i) for x in d_all], _sub(time_all, i)
        tmin, mx = _const(m, 0.001), _sub(tmax, i)
        box = nd["box"][node].astype(np.float64)
        inside = _hit_aabb(N, np.ones(m, bool), o, d, [Err(box[:, k]) for k in range(6)], tmin, mx)   # :240
        unsure = N.scope & ~(N.margin > 1.0)
        inside, doubt = inside | unsure, doubt | unsure
        doubted[i] |= doubt
        left, right = nd["left"][node].astype(np.int64), nd["right"][node].astype(np.int64)
        leaf = inside & ((left & 0xFFFF) != 0)                              # :241-242
        inner = inside & ~leaf
        over = inner & (sp[i] + 2 > STACK)
        Q.scope &= ~over
        push = inner & ~over
        j = i[push]
        mark = doubt[push].astype(np.int64) << DOUBT_BIT
        stack[j, sp[j]] = ((left[push] >> 16) & 0xFFFF) | mark              # :259
        stack[j, sp[j] + 1] = ((right[push] >> 16) & 0xFFFF) | mark         # :260
        sp[j] += 2
        for word in (left, right):                                          # :247, :254-255
            if not leaf.any():
                break
            typ, idx = word & 0xFFFF, (word >> 16) & 0xFFFF
            slots[i[leaf]] += 1
            drawn = count[i].copy()
            if word is right:
                # A sphere, quad or box alone in its leaf is tested a second time (both ids name it).  hit_boundary
                # draws nothing, so that test repeats the first on the same ray and prim under a ray_t.max that is
                # either unchanged (the first missed: so does the second) or the first's own t -- the same float, not
                # a value within a bound of it.  Then t < ray_t.max fails for both of a sphere's roots (the other one
                # is past it or was below ray_t.min), and t <= ray_t.max accepts a quad, or a box's last accepted
                # side, again with the values it already wrote.  Either way nothing changes, and the comparison is
                # decided by identity, which a rounding bound cannot express: the test is counted and not evaluated.
                leaf = leaf & ~((left == right) & (typ != MODEL_CONSTANT_MEDIUM))
            hit, th = np.zeros(m, bool), Err(np.zeros(m))
            side = np.zeros(m, np.int64)
            for ty in np.unique(typ[leaf]):                                 # hit_model, hitting.glsl:195-206
                rws = leaf & (typ == ty)
                size = {MODEL_SPHERE: len(S.spheres), MODEL_QUAD: len(S.quads), MODEL_BOX: len(S.boxes),
                        MODEL_CONSTANT_MEDIUM: len(S.media)}.get(int(ty), 0)
                if size == 0:
                    continue
                ix = np.where(rws, idx, 0)
                Q.scope &= ~(rws & (ix >= size))
                ix = np.minimum(ix, size - 1)
                if ty == MODEL_CONSTANT_MEDIUM:
                    def draw(lv):
                        r = i[lv]
                        short[r] |= count[r] >= seq.shape[1]
                        v = np.zeros(m)
                        v[lv] = seq[r, np.minimum(count[r], seq.shape[1] - 1)]
                        count[r] += 1
                        return Err(v)
                    h, tt = _hit_medium(S, Q, rws, o, d, time, ix, tmin, mx, draw)   # :201-203
                    src, sd = None, np.zeros(m, np.int64)
                else:
                    h, tt, sd, src = _hit_boundary(S, Q, rws, o, d, time, int(ty), ix, tmin, mx)   # :197
                h = h & rws
                hit, th, side = hit | h, pick(h, tt, th), np.where(h, sd, side)
                if src is not None and h.any():                             # hit_record.uv written (hitting.glsl:45, :85-86)
                    uvk[i[h]] = np.broadcast_to(src[0], (m,))[h]
                    wrote[i[h]] = True
                    for k in range(3):
                        if src[1 + k] is not None:
                            _put(uv[k], i, src[1 + k], h)
            effect[i] |= doubt & (hit | (count[i] != drawn))
            mx = pick(hit, th, mx)                                          # :250
            _put(t, i, th, hit)
            has[i[hit]] = True                                              # :249
            tif[i[hit]] = (typ | (side << 4) | (idx << 16))[hit]
        _put(tmax, i, mx, np.ones(m, bool))
        P.margin[i] = np.minimum(P.margin[i], np.minimum(Q.margin, N.margin))
        R.margin[i] = np.minimum(R.margin[i], np.minimum(Q.margin, np.where(unsure, np.inf, N.margin)))
        P.scope[i] &= Q.scope & N.scope
    P.scope &= ~short
    P.need(t, live=has)
    R.scope = P.scope
    cls = dict(hit=has, tif=np.where(has, tif, 0), uvk=uvk, count=count, visits=visits, slots=slots,
               hash=hsh.astype(np.int64))
    sph = (uvk >> 16) == 1
    val = dict(t=t, uva=uv[0], uvb=uv[1], uvc=uv[2])
    return dict(cls=cls, val=val, mask=dict(t=has, uva=uvk != 0, uvb=uvk != 0, uvc=sph), path=P, written=wrote,
                relaxed=R.decided & ~effect, doubted=doubted)

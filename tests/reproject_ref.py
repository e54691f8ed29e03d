"""NumPy float32 restatement of temporal reprojection (rt.h rt_reproject), written from rt.h alone: the
history view's matrix in float64, every other operation in float32 in the header's order, so that
rt_reproject_host (and through it the kernel) can be compared bit for bit.  `reproject` also returns
which branch every pixel and every tap took, for the tests that ask for every branch.

Also the synthetic inputs of tests/test_reproject_host.py: a wall of two coplanar quads and a sphere in
front of it, ray-cast here for any camera block.
"""
import numpy as np

F = np.float32
MISS = 0xFFFFFFFF
DEFAULTS = (0.9, 0.1, 64.0)   # rt.h RT_REPROJECT_DEFAULT_*

# pixel status
NOT_REPROJECTED, BEHIND, OUTSIDE, NO_TAP, HISTORY_ONLY, BLENDED = range(6)


def cam_parts(cam):
    c = np.asarray(cam, F).ravel()
    assert c.size == 28
    return c[4:7], c[8:11], c[12:15], c[16:19]   # camera_pos, up_left, pixel_delta_u, pixel_delta_v


def matrix(cam):
    """M of rt.h: float64, each entry rounded to float32 once.  ValueError when det is 0 or not finite."""
    o, ul, du, dv = (v.astype(np.float64) for v in cam_parts(cam))
    c0, c1, c2 = du, dv, ul - o

    def cross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])

    r0, r1, r2 = cross(c1, c2), cross(c2, c0), cross(c0, c1)
    with np.errstate(all="ignore"):
        det = (c0[0] * r0[0] + c0[1] * r0[1]) + c0[2] * r0[2]
        if det == 0.0 or not np.isfinite(det):
            raise ValueError("singular camera")
        return np.array([r0 / det, r1 / det, r2 / det]).astype(F)


def tile_counts(tile_frames, W, H):
    tx, ty = (W + 7) // 8, (H + 7) // 8
    tf = np.asarray(tile_frames, np.int32).ravel()
    if tf.size == 1:
        tf = np.full(tx * ty, tf[0], np.int32)
    assert tf.size == tx * ty
    return np.repeat(np.repeat(tf.reshape(ty, tx), 8, axis=0), 8, axis=1)[:H, :W]


def guide_good(nd, ai):
    return np.isfinite(nd).all(axis=-1) & np.isfinite(ai[..., :3]).all(axis=-1)


def id_word(ai):
    return np.ascontiguousarray(ai, F).view(np.uint32)[..., 3]


def pixel_base(cam, fx, fy):
    _, ul, du, dv = cam_parts(cam)
    return [(ul[c] + du[c] * fx) + dv[c] * fy for c in range(3)]


def history_from_image(image, tile_frames):
    img = np.ascontiguousarray(image, F)
    H, W = img.shape[:2]
    out = img.copy()
    out[..., 3] = np.where(np.isfinite(img[..., :3]).all(axis=-1), tile_counts(tile_frames, W, H).astype(F), F(0))
    return out


def reproject(hist, hnd, hai, hcam, image, tile_frames, nd, ai, cam, cos_min=DEFAULTS[0], kz=DEFAULTS[1],
              max_history=DEFAULTS[2]):
    """-> (out [H, W, 4] float32, info dict)."""
    hist, hnd, hai, image, nd, ai = (np.ascontiguousarray(a, F) for a in (hist, hnd, hai, image, nd, ai))
    cos_min, kz, max_history = F(cos_min), F(kz), F(max_history)
    H, W = image.shape[:2]
    M = matrix(hcam)
    o, o_h = cam_parts(cam)[0], cam_parts(hcam)[0]
    ys, xs = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        C = image[..., :3]
        n_c = np.where(np.isfinite(C).all(axis=-1), tile_counts(tile_frames, W, H).astype(F), F(0))
        ids = id_word(ai)
        live = guide_good(nd, ai) & (ids != MISS)                                    # 1
        base = pixel_base(cam, xs.astype(F), ys.astype(F))                           # 2
        d = [base[c] - o[c] for c in range(3)]
        t = nd[..., 3]
        P = [o[c] + d[c] * t for c in range(3)]
        w = [P[c] - o_h[c] for c in range(3)]                                        # 3
        a, b, c_ = [(M[r, 0] * w[0] + M[r, 1] * w[1]) + M[r, 2] * w[2] for r in range(3)]
        front = live & (c_ > F(0))
        fx, fy = a / c_, b / c_
        inside = front & (fx > F(-1)) & (fx < F(W)) & (fy > F(-1)) & (fy < F(H))
        x0, y0 = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0, fy - y0
        ix = np.where(inside, x0, F(0)).astype(np.int64)
        iy = np.where(inside, y0, F(0)).astype(np.int64)
        sw = np.zeros((H, W), F)
        sn = np.zeros((H, W), F)
        sc = [np.zeros((H, W), F) for _ in range(3)]
        hids = id_word(hai)
        hgood = guide_good(hnd, hai) & (hids != MISS)
        taps = []
        for j in (0, 1):                                                             # 4
            for i in (0, 1):
                qx, qy = ix + i, iy + j
                q_in = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                hq, ndq = hist[cy, cx], hnd[cy, cx]
                u = (ax if i else F(1) - ax) * (ay if j else F(1) - ay)
                held = hq[..., 3] > F(0)
                surf = hgood[cy, cx]
                same = hids[cy, cx] == ids
                facing = ((nd[..., 0] * ndq[..., 0] + nd[..., 1] * ndq[..., 1]) + nd[..., 2] * ndq[..., 2]) >= cos_min
                if kz != F(0):
                    qb = pixel_base(hcam, cx.astype(F), cy.astype(F))
                    dq = [qb[c] - o_h[c] for c in range(3)]
                    t_exp = ((w[0] * dq[0] + w[1] * dq[1]) + w[2] * dq[2]) / ((dq[0] * dq[0] + dq[1] * dq[1]) + dq[2] * dq[2])
                    near = np.abs(t_exp - ndq[..., 3]) <= kz * t_exp
                else:
                    near = np.ones((H, W), bool)
                use = inside & q_in & held & surf & same & facing & near
                sw = np.where(use, sw + u, sw)
                for c in range(3):
                    sc[c] = np.where(use, sc[c] + u * hq[..., c], sc[c])
                sn = np.where(use, sn + u * hq[..., 3], sn)
                taps.append(dict(considered=inside, q_in=q_in, qx=qx, qy=qy, held=held, surf=surf, same=same,
                                 facing=facing, near=near, use=use))
        got = inside & (sw > F(0))                                                   # 5
        Hc = [sc[c] / sw for c in range(3)]
        n_hist = np.where(max_history < sn / sw, max_history, sn / sw)               # g_min(sn / sw, max_history)
        n_out = n_c + n_hist                                                         # 6
        alpha = n_hist / n_out
        out = np.empty((H, W, 4), F)
        only = got & (n_c == F(0))
        for c in range(3):
            blend = C[..., c] + alpha * (Hc[c] - C[..., c])
            out[..., c] = np.where(got, np.where(only, Hc[c], blend), C[..., c])
        out[..., 3] = np.where(got, np.where(only, n_hist, n_out), n_c)
    status = np.full((H, W), NOT_REPROJECTED, np.int32)
    status[live & ~front] = BEHIND
    status[front & ~inside] = OUTSIDE
    status[inside & ~got] = NO_TAP
    status[got & only] = HISTORY_ONLY
    status[got & ~only] = BLENDED
    return out, dict(status=status, taps=taps, n_c=n_c, n_hist=np.where(got, n_hist, F(0)), fx=fx, fy=fy, live=live)


def sole_causes(info):
    """For each of the tap tests, whether some tap inside the image with history held on a surface failed
    that test alone."""
    out = {k: False for k in ("same", "facing", "near")}
    for tp in info["taps"]:
        ok = tp["considered"] & tp["q_in"] & tp["held"] & tp["surf"]
        for k in out:
            others = [tp[o] for o in out if o != k]
            out[k] = out[k] or bool((ok & ~tp[k] & others[0] & others[1]).any())
    return out


# ---- synthetic inputs: a wall of two coplanar quads at z = -5 (split at x = 0, with a hole to the right that
# shows the background) and a sphere in front of it ------------------------------------------------------

QUAD, SPHERE = 2, 1                     # the prim types' low id bits (any two distinct values do here)
WALL_L, WALL_R, BALL = QUAD | (0 << 16), QUAD | (1 << 16), SPHERE | (0 << 16)
WALL_Z, HOLE_X, HOLE_Y = -5.0, 2.2, 1.2   # the hole: x > HOLE_X and |y| < HOLE_Y
BALL_C, BALL_R = np.array([0.0, 0.0, -3.0]), 0.8


def camera(W, H, pos, yaw=0.0, pitch=0.0, roll=0.0, vfov=80.0):
    """A 28-float camera block looking down -z, turned by yaw (about y), pitch (about x) and roll (about the
    view axis), in degrees; up_left is the centre of pixel (0, 0)."""
    cy, sy = np.cos(np.radians(yaw)), np.sin(np.radians(yaw))
    cp, sp = np.cos(np.radians(pitch)), np.sin(np.radians(pitch))
    cr, sr = np.cos(np.radians(roll)), np.sin(np.radians(roll))
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    R = Ry @ Rx @ Rz
    right, up, fwd = R @ [1.0, 0, 0], R @ [0, 1.0, 0], R @ [0, 0, -1.0]
    vh = 2.0 * np.tan(np.radians(vfov) / 2.0)
    vw = vh * W / H
    du, dv = right * vw / W, -up * vh / H
    pos = np.asarray(pos, np.float64)
    ul = pos + fwd - right * vw / 2 + up * vh / 2 + 0.5 * (du + dv)
    ubo = np.zeros(28, F)
    ubo[0:4] = (vw, vh, W / H, 0.0)
    ubo[4:7], ubo[8:11], ubo[12:15], ubo[16:19] = pos, ul, du, dv
    return ubo


def raycast(cam, W, H):
    """-> (normal_depth, albedo_id) [H, W, 4] float32 for the synthetic scene, in rt_render_features' form:
    t in units of |d|, N turned against the ray, a miss N = 0, t = -1, id MISS."""
    o, ul, du, dv = (v.astype(np.float64) for v in cam_parts(cam))
    ys, xs = np.mgrid[0:H, 0:W]
    base = ul + du * xs[..., None] + dv * ys[..., None]
    d = base - o
    nd = np.zeros((H, W, 4), F)
    nd[..., 3] = -1.0
    ai = np.zeros((H, W, 4), F)
    ai[..., :3] = (0.5, 0.7, 1.0)
    ids = np.full((H, W), MISS, np.uint32)
    best = np.full((H, W), np.inf)
    with np.errstate(all="ignore"):
        tw = (WALL_Z - o[2]) / d[..., 2]
        p = o + d * tw[..., None]
        on = (tw > 1e-3) & ~((p[..., 0] > HOLE_X) & (np.abs(p[..., 1]) < HOLE_Y))
        best = np.where(on, tw, best)
        n_wall = np.where(d[..., 2:3] < 0, [0.0, 0.0, 1.0], [0.0, 0.0, -1.0])
        oc = o - BALL_C
        qa, qb, qc = (d * d).sum(-1), (d * oc).sum(-1), (oc * oc).sum() - BALL_R ** 2
        disc = qb * qb - qa * qc
        ts = (-qb - np.sqrt(disc)) / qa
        ball = (disc > 0) & (ts > 1e-3) & (ts < best)
    wall = on & ~ball
    nd[wall, :3] = n_wall[wall]
    nd[wall, 3] = tw[wall]
    ai[wall, :3] = np.where(p[wall, 0:1] < 0, [0.8, 0.2, 0.2], [0.2, 0.8, 0.2])
    ids[wall] = np.where(p[wall, 0] < 0, WALL_L, WALL_R)
    pb = o + d * ts[..., None]
    nd[ball, :3] = ((pb - BALL_C) / BALL_R)[ball]
    nd[ball, 3] = ts[ball]
    ai[ball, :3] = (0.3, 0.3, 0.9)
    ids[ball] = BALL
    ai.view(np.uint32)[..., 3] = ids
    return nd, ai

"""The expected first-hit buffers of rt_render_features (rt.h), built on the CPU from the oracle's
per-operation entry points alone (pyoracle.eval_op / eval_builtin), for tests/test_features_host.py
and tests/test_gpu_features.py.  A helper, not a conftest.

Camera rays are numpy float32 from the scene's camera block (numpy does not contract).  The candidate
prims are the BVH's leaf ids with the constant media left out, so a prim that is only a medium's
boundary never appears.  One eval_op batch per prim type tests every candidate against every pixel
with ray_t.max infinite; the pixel's hit is the smallest t.  A closer root does not depend on
ray_t.max (a sphere's root selection only ever moves to the farther root; a plane's t is one
quotient), so this equals the walk's shrinking-interval result.  N, p and the sphere's
(p - c) * (1 / r) are restated in numpy float32; the albedo comes from the oracle's texture op (solid,
checker, Perlin and image textures through its texture_color on the scene's own texel tables) with the
sphere_uv op for a sphere's image uv.

A pixel whose two smallest t (over different prims) are equal to the bit is tied: the walk's visit
order decides which prim keeps it, so only its t is compared and its id must be one of the tied prims.
The front / back decision g_dot(d, n) < 0 is taken from a float64 dot product; where that is too close
to zero to decide the float32 fused chain's sign, a sphere pixel is compared up to the sign of N (and
a light's emission, which depends on that decision, is not compared).
"""
import functools
import types

import numpy as np

import pyoracle
import rtamd

F = np.float32
MISS = 0xFFFFFFFF
SPHERE, QUAD, MEDIUM, BOX = 1, 2, 3, 4
MAT_DIFFUSE_LIGHT = 3
TEX_IMAGE = 1
INF = 3.402823e38   # RT_INFINITY
_SCENE = rtamd.Scene   # the class, whatever a tool binds rtamd.Scene to later

# (scene, W, H) of the GPU comparison, and the largest share of tied pixels the helper accepts per
# scene (counted on the CPU at these sizes: 13 of 1024 on scenes 6 and 7 -- the Cornell box's edges, where
# two quads meet -- and none on scenes 0, 2, 3 and 8; scene 8's cap leaves room for its abutting ground boxes)
CASES = [(6, 32, 32), (7, 32, 32), (0, 32, 18), (2, 32, 18), (3, 32, 18), (8, 32, 24)]
TIE_CAPS = {6: 0.02, 7: 0.02, 0: 0.0, 2: 0.0, 3: 0.0, 8: 0.05, 9: 0.05}


def camera_rays(camera, W, H):
    """(o [3], d [H, W, 3]) float32: coord = (up_left + du * x) + dv * y, d = coord - camera_pos."""
    cam = np.asarray(camera, F)
    pos, ul, du, dv = cam[4:7], cam[8:11], cam[12:15], cam[16:19]
    fx = np.arange(W, dtype=F)[None, :, None]
    fy = np.arange(H, dtype=F)[:, None, None]
    coord = (ul[None, None, :] + du[None, None, :] * fx) + dv[None, None, :] * fy
    return pos.copy(), (coord - pos[None, None, :]).astype(F)


def leaf_prims(scene):
    """The BVH's leaf ids as sorted unique index arrays per solid prim type; media skipped."""
    nodes = np.frombuffer(scene.buffers[1], np.int32).reshape(-1, 8)
    out = {SPHERE: set(), QUAD: set(), BOX: set()}
    for left, right in nodes[:, 6:8]:
        if (left & 0xFFFF) == 0:
            continue   # an inner node
        for pid in (int(left), int(right)):
            ty, ix = pid & 0xFFFF, (pid >> 16) & 0xFFFF
            if ty in out:
                out[ty].add(ix)
    return {ty: np.array(sorted(s), np.int64) for ty, s in out.items()}


def _texture_colors(scene, tex_ids, p, uv):
    """texture_color(p, id, uv) per row through the oracle's texture op: one batch per texture slot, the
    slot's texels as the op's slot 0."""
    n = len(tex_ids)
    out = np.zeros((n, 3), F)
    tex_ids = np.asarray(tex_ids, np.int64)
    slots = (tex_ids >> 12) & 7
    by_slot = {t.slot: t for t in scene.textures}
    for slot in np.unique(slots):
        m = slots == slot
        t = by_slot.get(int(slot))
        if t is None:
            continue   # no texture uploaded: every texel reads 0
        word = ((tex_ids[m] & ~np.int64(0xFFFF << 12)) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        d = np.zeros((int(m.sum()), 3), F)
        d[:, :2] = uv[m]
        rows = pyoracle.op_rows(p[m], d, word=word)
        texels = np.frombuffer(t.data, np.uint8)
        w = pyoracle.eval_op("texture", rows, tex=(t.format, t.width, t.height, texels))
        out[m] = np.ascontiguousarray(w[:, 0:3]).view(F)
    return out


def _reference_once(scene, W=None, H=None, seed=1):
    """reference() without the cache (reference.__wrapped__, as tools/reproject_quality.py calls it: a scene id
    is built through rtamd.Scene as it is bound at the call)."""
    if isinstance(scene, _SCENE):
        assert (W is None or W == scene.width) and (H is None or H == scene.height)
        return _reference(scene)
    built = rtamd.Scene(int(scene), W, H, seed=seed)
    try:
        return _reference(built)
    finally:
        built.close()


_reference_cached = functools.lru_cache(maxsize=None)(_reference_once)


def reference(scene, W=None, H=None, seed=1):
    """The expected buffers of a built-in scene (its id, at W x H; computed once per process) or of an
    rtamd.Scene (at its own size, computed at every call; the scene stays the caller's):
    t [H, W] f32 (-1 on a miss), hit [H, W] bool, id [H, W] u32, ids_ok [H, W] list of the ids a tied
    pixel may hold, N [H, W, 3], A [H, W, 3], tied [H, W] bool, sign_free [H, W] bool (N up to its sign),
    a_free [H, W] bool (A not compared), background [3]."""
    if isinstance(scene, _SCENE):
        return _reference_once(scene, W, H)
    return _reference_cached(scene, W, H, seed)


reference.__wrapped__ = _reference_once
reference.cache_clear = _reference_cached.cache_clear


def _reference(scene):
    W, H = scene.width, scene.height
    o, d = camera_rays(scene.camera, W, H)
    n_px = W * H
    dd = d.reshape(n_px, 3)
    oo = np.broadcast_to(o, (n_px, 3))
    prims = leaf_prims(scene)
    recs = {SPHERE: np.frombuffer(scene.buffers[0], np.uint8).reshape(-1, 48),
            QUAD: np.frombuffer(scene.buffers[2], np.uint8).reshape(-1, 80),
            BOX: np.frombuffer(scene.buffers[4], np.uint8).reshape(-1, 480)}
    opname = {SPHERE: "sphere", QUAD: "quad", BOX: "box"}
    # per candidate prim and pixel: t (inf where missed), and what the hit leaves (face, alpha, beta)
    cand_t, cand_id, cand_face, cand_uv = [], [], [], []
    for ty in (SPHERE, QUAD, BOX):
        idx = prims[ty]
        if idx.size == 0:
            continue
        k = idx.size
        step = max(1, (1 << 19) // n_px)   # prims per batch: about half a million rows at most
        parts = []
        for i0 in range(0, k, step):
            sub = idx[i0:i0 + step]
            rows = pyoracle.op_rows(np.tile(oo, (sub.size, 1)), np.tile(dd, (sub.size, 1)), tmin=0.001, tmax=INF, time=0.0)
            rb = np.repeat(recs[ty][sub], n_px, axis=0)
            parts.append(pyoracle.eval_op(opname[ty], rows, rb).reshape(sub.size, n_px, 8))
        w = np.concatenate(parts, 0)
        hit = w[..., 0] != 0
        t = np.where(hit, np.ascontiguousarray(w[..., 1]).view(F), F(np.inf))
        cand_t.append(t)
        cand_id.append(np.broadcast_to(((idx.astype(np.uint32) << 16) | np.uint32(ty))[:, None], (k, n_px)))
        if ty == BOX:
            cand_face.append(w[..., 2].astype(np.uint32))
            cand_uv.append(np.ascontiguousarray(w[..., 3:5]).view(F))
        elif ty == QUAD:
            cand_face.append(np.zeros((k, n_px), np.uint32))
            cand_uv.append(np.ascontiguousarray(w[..., 2:4]).view(F))
        else:
            cand_face.append(np.zeros((k, n_px), np.uint32))
            cand_uv.append(np.zeros((k, n_px, 2), F))
    if cand_t:
        T = np.concatenate(cand_t, 0)
        ID = np.concatenate(cand_id, 0) | (np.concatenate(cand_face, 0) << 4)
        UV = np.concatenate(cand_uv, 0)
    else:
        T = np.full((1, n_px), np.inf, F)
        ID = np.zeros((1, n_px), np.uint32)
        UV = np.zeros((1, n_px, 2), F)
    best = np.argmin(T, axis=0)
    px = np.arange(n_px)
    tb = T[best, px]
    hit = np.isfinite(tb)
    same = (T.view(np.uint32) == tb.view(np.uint32)[None, :]) & hit[None, :]
    tied = same.sum(0) > 1
    ids = np.where(hit, ID[best, px], np.uint32(MISS)).astype(np.uint32)
    ids_ok = [set(ID[same[:, i], i].tolist()) if hit[i] else {MISS} for i in range(n_px)]
    uv = UV[best, px]

    t = np.where(hit, tb, F(-1.0)).astype(F)
    N = np.zeros((n_px, 3), F)
    A = np.tile(np.asarray(scene.background, F), (n_px, 1))
    sign_free = np.zeros(n_px, bool)
    a_free = np.zeros(n_px, bool)
    ty_px, ix_px, face_px = ids & 0xF, ids >> 16, (ids >> 4) & 7
    with np.errstate(all="ignore"):
        p = (oo + dd * np.where(hit, tb, F(0.0))[:, None]).astype(F)
    material = np.zeros(n_px, np.int64)
    tex_id = np.zeros(n_px, np.int64)
    emis = np.zeros((n_px, 3), F)
    tuv = uv.copy()
    # spheres: on = (p - center) * (1 / radius), center = center1 + center_vec * 0
    m = hit & (ty_px == SPHERE)
    if m.any():
        r = np.ascontiguousarray(recs[SPHERE][ix_px[m]])
        rf, ri = r.view(F).reshape(-1, 12), r.view(np.int32).reshape(-1, 12)
        center = rf[:, 0:3] + rf[:, 4:7] * F(0.0)
        rel = (p[m] - center).astype(F)
        N[m] = rel * (F(1.0) / rf[:, 7])[:, None]
        material[m], tex_id[m], emis[m] = ri[:, 11], ri[:, 3], rf[:, 8:11]
        img = ((ri[:, 3] >> 28) & 0xF) == TEX_IMAGE
        if img.any():
            u, v = pyoracle.sphere_uvs(rel[img])
            sub = np.flatnonzero(m)[img]
            tuv[sub, 0], tuv[sub, 1] = u, v
    # quads and box faces: the record's normal; material, texture and emission of quads[0]
    for ty in (QUAD, BOX):
        m = hit & (ty_px == ty)
        if not m.any():
            continue
        r = np.ascontiguousarray(recs[ty][ix_px[m]])
        rf, ri = r.view(F).reshape(len(r), -1), r.view(np.int32).reshape(len(r), -1)
        f0 = (face_px[m] * 20).astype(np.int64)
        N[m] = np.stack([rf[np.arange(len(r)), f0 + c] for c in range(3)], 1)
        material[m], tex_id[m], emis[m] = ri[:, 7], ri[:, 11], rf[:, 16:19]
    # front / back from a float64 dot product; too close to call: free
    d64, n64 = dd.astype(np.float64), N.astype(np.float64)
    dot = (d64 * n64).sum(1)
    mag = np.abs(d64 * n64).sum(1)
    unsure = hit & (np.abs(dot) <= mag * 2.0 ** -20)
    front = dot < 0.0
    assert not (unsure & (ty_px != SPHERE)).any(), "a quad's front / back decision is too close to call"
    sign_free = unsure
    N = np.where((front | ~hit)[:, None], N, -N).astype(F)
    light = hit & (((material >> 16) & 0xFFFF) == MAT_DIFFUSE_LIGHT)
    a_free = unsure & light
    tm = hit & ~light
    if tm.any():
        A[tm] = _texture_colors(scene, tex_id[tm], p[tm], tuv[tm])
    A[light] = np.where(front[light][:, None], emis[light], F(0.0))
    return types.SimpleNamespace(
        t=t.reshape(H, W), hit=hit.reshape(H, W), id=ids.reshape(H, W),
        ids_ok=[ids_ok[y * W:(y + 1) * W] for y in range(H)], N=N.reshape(H, W, 3), A=A.reshape(H, W, 3),
        tied=tied.reshape(H, W), sign_free=sign_free.reshape(H, W), a_free=a_free.reshape(H, W),
        background=np.asarray(scene.background, F).copy())


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def check(ref, nd, alb, ids):
    """Assert device buffers (RenderContext.read_features()) against a reference(): t and hit / miss
    bit-exact on every pixel; id exact, or one of the tied prims; N and A bit-exact on untied pixels
    (N up to its sign where sign_free, A skipped where a_free)."""
    H, W = ref.t.shape
    assert nd.shape == (H, W, 4) and alb.shape == (H, W, 3) and ids.shape == (H, W)
    assert np.array_equal((ids != MISS), ref.hit), "hit / miss differs"
    bad_t = np.argwhere(bits(nd[..., 3]) != bits(ref.t))
    assert bad_t.size == 0, f"t differs at {bad_t[:5].tolist()}"
    for y in range(H):
        for x in range(W):
            assert int(ids[y, x]) in ref.ids_ok[y][x], f"id {int(ids[y, x]):#x} at ({x}, {y}) not in {ref.ids_ok[y][x]}"
    exact = ~ref.tied
    assert np.array_equal(ids[exact], ref.id[exact])
    n_same = (bits(nd[..., :3]) == bits(ref.N)).all(-1)
    n_flip = (bits(nd[..., :3]) == bits(-ref.N)).all(-1)
    n_ok = n_same | (ref.sign_free & n_flip) | ~exact
    assert n_ok.all(), f"N differs at {np.argwhere(~n_ok)[:5].tolist()}"
    a_ok = (bits(alb) == bits(ref.A)).all(-1) | ~exact | ref.a_free
    assert a_ok.all(), f"A differs at {np.argwhere(~a_ok)[:5].tolist()}"

"""rt_reproject_host (rt.h; csrc/rt_reproject_math.h on the host) against tests/reproject_ref.py, the NumPy
float32 restatement written from rt.h, bit for bit on synthetic buffers -- a wall of two coplanar quads and
a sphere in front of it, ray-cast in NumPy for two cameras -- and what reprojection means on them.  No GPU.
"""
import ctypes
import functools

import numpy as np
import pytest

import rtamd
from rtamd import _lib
import reproject_ref as R

F = np.float32

# history pose, current pose: a sideways shift and a small turn (yaw, pitch and a roll that takes taps off every edge)
POSE_H = dict(pos=(0.0, 0.0, 0.0))
POSE_C = dict(pos=(0.7, 0.1, 0.0), yaw=2.0, pitch=0.0, roll=16.0)
SHAPES = [(13, 9), (32, 18)]   # 13x9: partial tiles both ways


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def colours(ai, rng, lo=0.2):
    """A colour per surface id plus a little noise, in [lo, 1]."""
    ids = R.id_word(ai)
    base = np.stack([((ids >> s) & 7).astype(F) / F(14) for s in (0, 16, 2)], axis=-1) + F(lo)
    return np.clip(base + rng.random(base.shape, dtype=F) * F(0.3), lo, 1.0).astype(F)


@functools.lru_cache(maxsize=None)
def case(W, H, pose_h=None, clean=False):
    """Inputs of one reprojection.  Unless clean: history pixels with n = 0, a wall patch whose history depth is
    off by 30 %, non-finite current pixels, unequal tile counts with a 0 among them."""
    rng = np.random.default_rng(W * 100 + H)
    hcam = R.camera(W, H, **(dict(pose_h) if pose_h else POSE_H))
    cam = R.camera(W, H, **POSE_C)
    hnd, hai = R.raycast(hcam, W, H)
    nd, ai = R.raycast(cam, W, H)
    hist = np.empty((H, W, 4), F)
    hist[..., :3] = colours(hai, rng)
    hist[..., 3] = 8.0
    image = np.empty((H, W, 4), F)
    image[..., :3] = colours(ai, rng)
    image[..., 3] = 1.0
    nt = ((W + 7) // 8) * ((H + 7) // 8)
    tf = np.full(nt, 2, np.int32)
    if not clean:
        hist[H // 2, :: 3, 3] = 0.0
        hist[1, 1, 3] = -2.0
        wall = np.argwhere(R.id_word(hai) == R.WALL_R)
        for y, x in wall[len(wall) // 3: len(wall) // 3 + max(3, W // 4)]:
            hnd[y, x, 3] *= F(1.3)
        image[H // 2, W // 2 + 2, 0] = np.nan
        image[H - 2, 2, 1] = np.inf
        image[2, W - 3, 2] = -np.inf
        tf = (np.arange(nt, dtype=np.int32) % 3 + 1).astype(np.int32)
        tf[nt - 1] = 0
    for a in (hist, hnd, hai, image, nd, ai, tf, hcam, cam):
        a.setflags(write=False)
    return dict(hist=hist, hnd=hnd, hai=hai, hcam=hcam, image=image, tf=tf, nd=nd, ai=ai, cam=cam)


def run_both(c, **prm):
    got = rtamd.reproject_host(c["hist"], c["hnd"], c["hai"], c["hcam"], c["image"], c["tf"], c["nd"], c["ai"], c["cam"], **prm)
    full = dict(zip(("cos_min", "kz", "max_history"), R.DEFAULTS))
    full.update({k: v for k, v in prm.items() if v is not None})
    ref, info = R.reproject(c["hist"], c["hnd"], c["hai"], c["hcam"], c["image"], c["tf"], c["nd"], c["ai"], c["cam"], **full)
    return got, ref, info


# ---- 1. bit for bit, with every branch taken -----------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_matches_numpy_bit_for_bit(shape):
    W, H = shape
    c = case(W, H)
    got, ref, info = run_both(c)
    assert same_bits(got, ref), np.argwhere((got.view(np.uint32) != ref.view(np.uint32)).any(axis=-1))[:5]
    st = info["status"]
    for s in (R.NOT_REPROJECTED, R.OUTSIDE, R.NO_TAP, R.HISTORY_ONLY, R.BLENDED):
        assert (st == s).any(), s
    ids = R.id_word(c["ai"])
    assert (ids == R.MISS).any() and (R.id_word(c["hai"]) == R.MISS).any()                    # misses on both sides
    assert (~np.isfinite(c["image"][..., :3])).any() and (info["n_c"] == 0).any()            # a non-finite current pixel
    assert ((c["tf"] == 0).any()) and (c["hist"][..., 3] <= 0).any()                          # counts of 0, history n = 0
    taps = info["taps"]
    for name, off in (("left", lambda t: t["qx"] < 0), ("right", lambda t: t["qx"] >= W),
                      ("top", lambda t: t["qy"] < 0), ("bottom", lambda t: t["qy"] >= H)):
        assert any((t["considered"] & off(t)).any() for t in taps), f"no tap off the {name} edge"
    assert any((t["considered"] & t["q_in"] & ~t["held"]).any() for t in taps)                # a tap on n = 0
    assert any((t["considered"] & t["q_in"] & t["held"] & ~t["surf"]).any() for t in taps)    # a tap on a history miss
    assert R.sole_causes(info) == {"same": True, "facing": True, "near": True}
    assert any(t["use"].any() for t in taps) and any((t["considered"] & ~t["use"]).any() for t in taps)
    # the other parameter paths: the depth test off, a tight normal test, a low cap
    for prm in (dict(kz=0.0), dict(cos_min=0.999, kz=0.02), dict(max_history=3.0), dict(cos_min=-1.0, kz=5.0, max_history=1e6)):
        got, ref, _ = run_both(c, **prm)
        assert same_bits(got, ref), prm


def test_a_camera_turned_away_rejects_behind():
    W, H = SHAPES[0]
    c = case(W, H, pose_h=(("pos", (0.0, 0.0, 0.0)), ("yaw", 150.0)))
    got, ref, info = run_both(c)
    assert same_bits(got, ref)
    live = info["live"]
    assert live.any() and (info["status"][live] == R.BEHIND).all()
    exp = c["image"].copy()
    exp[..., 3] = info["n_c"]
    assert same_bits(got, exp)                                                                 # (C, n_c) everywhere


def test_defaults_and_null_params():
    c = case(*SHAPES[0])
    got = rtamd.reproject_host(c["hist"], c["hnd"], c["hai"], c["hcam"], c["image"], c["tf"], c["nd"], c["ai"], c["cam"])
    cm, kz, mh = rtamd.render.REPROJECT_DEFAULTS
    assert (cm, kz, mh) == R.DEFAULTS
    assert same_bits(got, run_both(c, cos_min=cm, kz=kz, max_history=mh)[0])
    assert same_bits(rtamd.history_from_image(c["image"], c["tf"]), R.history_from_image(c["image"], c["tf"]))


# ---- 2. what it means ---------------------------------------------------------------------------------

def history_ids_around(c, W, H):
    """In float64: for each current pixel, the four history ids around its world point's projection into the
    history view (MISS outside the image), and whether the projection is in front of the history camera."""
    o, ul, du, dv = (v.astype(np.float64) for v in R.cam_parts(c["cam"]))
    oh, ulh, duh, dvh = (v.astype(np.float64) for v in R.cam_parts(c["hcam"]))
    ys, xs = np.mgrid[0:H, 0:W]
    P = o + (ul + du * xs[..., None] + dv * ys[..., None] - o) * c["nd"][..., 3:4].astype(np.float64)
    abc = np.linalg.solve(np.stack([duh, dvh, ulh - oh], axis=1), (P - oh).reshape(-1, 3).T).T.reshape(H, W, 3)
    with np.errstate(all="ignore"):
        fx, fy = abc[..., 0] / abc[..., 2], abc[..., 1] / abc[..., 2]
    hids = R.id_word(c["hai"])
    out = np.full((H, W, 4), R.MISS, np.uint32)
    x0 = np.floor(np.nan_to_num(fx)).astype(int)
    y0 = np.floor(np.nan_to_num(fy)).astype(int)
    for k, (j, i) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        qx, qy = x0 + i, y0 + j
        ok = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
        out[..., k] = np.where(ok, hids[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)], R.MISS)
    return out, abc[..., 2] > 0


def test_disoccluded_wall_keeps_its_own_pixels_and_shared_wall_adds_counts():
    W, H = SHAPES[1]
    c = case(W, H, clean=True)
    got, ref, info = run_both(c)
    assert same_bits(got, ref)
    ids = R.id_word(c["ai"])
    around, front = history_ids_around(c, W, H)
    wall = (ids == R.WALL_L) | (ids == R.WALL_R)
    hidden = wall & front & (around == R.BALL).all(axis=-1)          # the sphere hid this wall point in the history view
    assert hidden.sum() >= 3
    n_c = R.tile_counts(c["tf"], W, H).astype(F)
    assert same_bits(got[hidden][:, :3], c["image"][hidden][:, :3]) and (got[hidden][:, 3] == n_c[hidden]).all()
    shared = wall & front & (around == ids[..., None]).all(axis=-1)  # all four taps on the same wall quad
    assert shared.sum() >= W * H // 8
    assert np.allclose(got[shared][:, 3], n_c[shared] + 8.0, rtol=1e-6, atol=0)     # n_c + min(n_h = 8, 64)
    a = 8.0 / (n_c[shared] + 8.0)
    lo = np.minimum(c["image"][shared][:, :3], 0.2)                   # a blend of the pixel and history colours >= 0.2
    assert (got[shared][:, :3] >= lo - 1e-6).all() and (got[shared][:, :3] <= 1.0 + 1e-6).all()
    assert (np.abs(got[shared][:, :3] - c["image"][shared][:, :3]) <= a[:, None] * 0.8 + 1e-6).all()
    # max_history caps n_hist
    capped, ref3, _ = run_both(c, max_history=3.0)
    assert same_bits(capped, ref3)
    assert np.allclose(capped[shared][:, 3], n_c[shared] + 3.0, rtol=1e-6, atol=0)
    assert (capped[..., 3] <= n_c + 3.0 + 1e-5).all()


def test_kz_zero_switches_the_depth_test_off():
    W, H = SHAPES[1]
    c = case(W, H)
    on, _, info_on = run_both(c)
    off, ref_off, info_off = run_both(c, kz=0.0)
    assert same_bits(off, ref_off)
    assert all(t["near"].all() for t in info_off["taps"])
    more = sum(int(t["use"].sum()) for t in info_off["taps"]) - sum(int(t["use"].sum()) for t in info_on["taps"])
    assert more > 0 and not same_bits(on, off)                         # the taps the depth test alone had rejected
    assert R.sole_causes(info_on)["near"] and not R.sole_causes(info_off)["near"]


def test_same_camera_is_the_exact_blend():
    W, H = SHAPES[1]
    base = case(W, H, clean=True)
    c = dict(base, hcam=base["cam"], hnd=base["nd"], hai=base["ai"])   # the history seen from the current camera
    rng = np.random.default_rng(5)
    hist = np.empty((H, W, 4), F)
    hist[..., :3] = colours(c["ai"], rng)
    hist[..., 3] = 8.0
    c["hist"] = hist
    got, ref, info = run_both(c)
    assert same_bits(got, ref)
    hit = R.id_word(c["ai"]) != R.MISS
    assert (info["status"][hit] == R.BLENDED).all()
    n_c = R.tile_counts(c["tf"], W, H).astype(np.float64)
    C, Hh = c["image"][..., :3].astype(np.float64), hist[..., :3].astype(np.float64)
    exact = C + (8.0 / (n_c + 8.0))[..., None] * (Hh - C)
    # not bit-equal: M is rounded, so fx is x only to a few ulp and a neighbour enters with a weight of that size
    assert np.allclose(got[hit][:, :3], exact[hit], rtol=1e-4, atol=0)
    assert np.allclose(got[hit][:, 3], n_c[hit] + 8.0, rtol=1e-4, atol=0)
    assert same_bits(got[~hit][:, :3], c["image"][~hit][:, :3])


# ---- 3. arguments -------------------------------------------------------------------------------------------

def raw_call(c, params=None, hcam=None, n_tiles=None, W=None, H=None):
    L = rtamd.amd()
    fp = lambda a: np.ascontiguousarray(a, F).ctypes.data_as(_lib.c_float_p)  # noqa: E731
    h, w = c["image"].shape[:2]
    out = np.zeros((h, w, 4), F)
    tf = np.ascontiguousarray(c["tf"], np.int32)
    return L.rt_reproject_host(fp(c["hist"]), fp(c["hnd"]), fp(c["hai"]), fp(c["hcam"] if hcam is None else hcam),
                               fp(c["image"]), tf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                               tf.size if n_tiles is None else n_tiles, fp(c["nd"]), fp(c["ai"]), fp(c["cam"]),
                               w if W is None else W, h if H is None else H, params, fp(out))


def params(cos_min=0.9, kz=0.1, max_history=64.0, reserved=None):
    p = _lib.RtReprojectParams()
    p.cos_min, p.kz, p.max_history = cos_min, kz, max_history
    if reserved is not None:
        p.reserved[reserved] = 1
    return ctypes.byref(p)


def test_bad_parameters_and_a_singular_camera_are_invalid_arguments():
    c = case(*SHAPES[0])
    assert raw_call(c) == 0 and raw_call(c, params()) == 0
    assert raw_call(c, params(cos_min=-1.0, kz=0.0, max_history=1e-3)) == 0
    nan, inf = float("nan"), float("inf")
    for bad in (dict(cos_min=1.5), dict(cos_min=-1.01), dict(cos_min=nan), dict(kz=-0.1), dict(kz=nan), dict(kz=inf),
                dict(max_history=0.0), dict(max_history=-1.0), dict(max_history=inf), dict(max_history=nan),
                dict(reserved=0), dict(reserved=4)):
        assert raw_call(c, params(**bad)) == -1, bad
    flat = np.array(c["hcam"])
    flat[16:19] = flat[12:15] * F(2)                                   # pixel_delta_v parallel to pixel_delta_u: det 0
    assert raw_call(c, hcam=flat) == -1
    with pytest.raises(ValueError):
        R.matrix(flat)
    broken = np.array(c["hcam"])
    broken[8] = np.inf                                                 # det not finite
    assert raw_call(c, hcam=broken) == -1
    assert raw_call(c, n_tiles=c["tf"].size - 1) == -1
    assert raw_call(c, W=0) == -1
    neg = dict(c, tf=np.where(np.arange(c["tf"].size) == 0, -1, c["tf"]).astype(np.int32))
    assert raw_call(neg) == -1
    with pytest.raises(rtamd.RTError) as e:
        rtamd.reproject_host(c["hist"], c["hnd"], c["hai"], flat, c["image"], c["tf"], c["nd"], c["ai"], c["cam"])
    assert e.value.code == -1


def test_params_struct_has_the_header_layout_and_null_contexts_are_rejected():
    assert ctypes.sizeof(_lib.RtReprojectParams) == 32
    L = rtamd.amd()
    assert L.rt_history_capture(None, 0) == -1
    assert L.rt_reproject(None, None) == -1
    out = np.zeros(4, F)
    assert L.rt_read_reprojected(None, out.ctypes.data_as(_lib.c_float_p)) == -1


def test_recorded_resources_and_defaults():
    import json
    import os
    import re
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rows = [ln for ln in open(os.path.join(repo, "profiles", "reproject_resources.txt")) if "reproject_kernel" in ln]
    assert len(rows) == 1
    f = {k: int(v) for k, v in re.findall(r"(VGPR|SGPR|spillV|spillS|scratch|LDS)\s+(\d+)", rows[0])}
    assert f["scratch"] == 0 and f["spillV"] == 0 and f["spillS"] == 0 and f["LDS"] == 0 and 0 < f["VGPR"] <= 128 and f["SGPR"] > 0
    rec = json.load(open(os.path.join(repo, "profiles", "reproject_quality.json")))
    d = rec["defaults"]
    assert rec["library_defaults_are_the_best"] and (d["cos_min"], d["kz"], d["max_history"]) == R.DEFAULTS
    assert rec["ratio_at_defaults"] == min(rec["grid"].values()) < 0.5

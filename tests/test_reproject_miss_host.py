"""The misses reprojected by direction on the host (rt.h rt_set_reproject_misses, rt_reproject_misses_host) against
tests/reproject_miss_ref.py, the NumPy float32 restatement written from rt.h, bit for bit, and what the rule
means case by case.  No GPU.
"""
import ctypes
import functools

import numpy as np
import pytest

import rtamd
from rtamd import _lib
import reproject_ref as R
import reproject_miss_ref as MR

F = np.float32
SHAPES = [(13, 9), (32, 18)]
POSE_H = dict(pos=(0.0, 0.0, 0.0))
# a sideways move (directions keep their pixel), and a yaw past the half field of view: directions at the frame's
# leading edge point behind the history view (c <= 0)
MOVES = dict(sideways=dict(pos=(0.7, 0.1, 0.0)), yaw=dict(pos=(0.3, 0.0, 0.1), yaw=-50.0, roll=4.0))
BACKGROUND = (0.5, 0.7, 1.0)   # reproject_ref.raycast's


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def view(cam, W, H):
    """reproject_ref's wall and sphere under a sky: every ray that climbs more than 0.15 per unit of depth, or
    does not head for the wall at all, is a miss -- a property of the direction, as a real background is."""
    nd, ai = R.raycast(cam, W, H)
    o, ul, du, dv = (v.astype(np.float64) for v in R.cam_parts(cam))
    ys, xs = np.mgrid[0:H, 0:W]
    d = ul + du * xs[..., None] + dv * ys[..., None] - o
    sky = (d[..., 1] > 0.15 * np.abs(d[..., 2])) & (R.id_word(ai) != R.BALL)
    nd, ai = nd.copy(), ai.copy()
    nd[sky] = (0.0, 0.0, 0.0, -1.0)
    ai[sky, :3] = BACKGROUND
    ai.view(np.uint32)[sky, 3] = R.MISS
    return nd, ai


@functools.lru_cache(maxsize=None)
def case(W, H, move):
    rng = np.random.default_rng(W * 100 + H + len(move))
    hcam, cam = R.camera(W, H, **POSE_H), R.camera(W, H, **MOVES[move])
    hnd, hai = view(hcam, W, H)
    nd, ai = view(cam, W, H)
    hmiss = R.id_word(hai) == R.MISS
    hist = np.empty((H, W, 4), F)
    hist[..., :3] = rng.random((H, W, 3), dtype=F)
    hist[..., 3] = 8.0
    hist[1, ::3, 3] = 0.0                                 # history n = 0, misses among them
    hist[H // 2, ::4, 3] = 0.0
    hist[0, 1, 0] = np.nan                                # a history colour that is not finite, on a miss
    hist[2, W - 2, 2] = np.inf
    hai[0, W // 2, 1] = np.nan                            # a history feature word that is not finite
    hnd[3, 2, 0] = np.inf
    # a history background that differs in one channel's bits, over a block of the sky
    hai[:2, W // 2 + 1:W // 2 + 4, 2] = np.nextafter(F(BACKGROUND[2]), F(2))
    hs2 = (rng.random((H, W), dtype=F) * F(0.2)).astype(F)
    hs2[::2, 1::3] = -1.0
    hs2[1::4, ::5] = np.nan
    image = np.empty((H, W, 4), F)
    image[..., :3] = rng.random((H, W, 3), dtype=F)
    image[..., 3] = 1.0
    image[0, 3, 0] = np.nan
    image[H - 2, 2, 1] = np.inf
    ai[1, 0, 0] = np.nan                                  # a current feature word that is not finite
    m2 = (rng.random((H, W, 4), dtype=F) * F(0.5)).astype(F)
    m2[1, 2, 3] = np.nan
    nt = ((W + 7) // 8) * ((H + 7) // 8)
    tf = (np.arange(nt, dtype=np.int32) % 3 + 1).astype(np.int32)
    tf[nt - 1] = 0
    if nt > 2:
        tf[1] = 0                                         # a tile of the sky with no frame of its own
    assert hmiss.any() and (~hmiss).any()
    c = dict(hist=hist, hnd=hnd, hai=hai, hs2=hs2, hcam=hcam, image=image, m2=m2, tf=tf, nd=nd, ai=ai, cam=cam)
    for a in c.values():
        a.setflags(write=False)
    return c


def host(c, var, misses=True, **prm):
    if var:
        return rtamd.reproject_variance_host(c["hist"], c["hnd"], c["hai"], c["hs2"], c["hcam"], c["image"], c["m2"], c["tf"],
                                             c["nd"], c["ai"], c["cam"], misses=misses, **prm)
    return rtamd.reproject_host(c["hist"], c["hnd"], c["hai"], c["hcam"], c["image"], c["tf"], c["nd"], c["ai"], c["cam"],
                                misses=misses, **prm), None


def ref(c, var, **prm):
    kw = dict(hs2=c["hs2"], m2=c["m2"]) if var else {}
    return MR.reproject(c["hist"], c["hnd"], c["hai"], c["hcam"], c["image"], c["tf"], c["nd"], c["ai"], c["cam"], **kw, **prm)


PRMS = ({}, dict(kz=0.0), dict(cos_min=0.999, kz=0.02), dict(max_history=3.0))


# ---- 1. the host entry against the restatement, bit for bit ----------------------------------------------

@pytest.mark.parametrize("move", sorted(MOVES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_matches_numpy_bit_for_bit(shape, move):
    c = case(*shape, move)
    for var in (False, True):
        for prm in PRMS:
            rgbn, s2 = host(c, var, **prm)
            want, want_s2, info = ref(c, var, **prm)
            assert same_bits(rgbn, want), (var, prm, int((rgbn.view(np.uint32) != want.view(np.uint32)).any(axis=-1).sum()))
            if var:
                assert same_bits(s2, want_s2), prm
                assert same_bits(rgbn, host(c, False, **prm)[0])         # the word is the no-variance form's
    # what the inputs hold and which branches ran (over the shapes and moves together where one cannot hold all)
    _, _, info = ref(c, True)
    st, miss, taps = info["status"], info["miss"], info["taps"]
    assert miss.any() and (~miss).any()
    assert (st[miss] == R.BLENDED).any() and (st[miss] == R.NO_TAP).any()
    assert any((t["considered"] & t["q_in"] & ~t["sky"]).any() for t in taps)                # a hit tap under a miss pixel
    assert any((t["considered"] & t["q_in"] & t["sky"] & ~t["held"]).any() for t in taps)    # history n = 0
    assert (c["tf"] == 0).any() and len(set(c["tf"].tolist())) >= 3
    assert (c["hist"][..., 3].max() > 3.0)                                                  # max_history = 3 clamps
    if move == "yaw":
        assert (st[miss] == R.BEHIND).any() and (st[miss] == R.OUTSIDE).any()
    if shape == (32, 18):
        assert (st[miss] == R.HISTORY_ONLY).any()
        assert any((t["considered"] & ~t["q_in"]).any() for t in taps)                       # taps at -1 or at W / H
    if move == "sideways":
        assert any((t["considered"] & t["q_in"] & t["sky"] & t["held"] & ~t["same"]).any() for t in taps)   # another background


def test_a_miss_accepts_no_hit_tap_and_a_hit_no_miss_tap():
    """History that is a hit everywhere leaves every miss pixel with its own frames; history that is a miss
    everywhere leaves every hit pixel so."""
    W, H = SHAPES[1]
    c = dict(case(W, H, "sideways"))
    solid_nd = np.zeros((H, W, 4), F)
    solid_nd[..., 2], solid_nd[..., 3] = 1.0, 5.0
    solid_ai = rtamd.pack_albedo_id(np.full((H, W, 3), BACKGROUND, F), np.full((H, W), R.WALL_L, np.uint32))
    empty_nd = np.zeros((H, W, 4), F)
    empty_nd[..., 3] = -1.0
    empty_ai = rtamd.pack_albedo_id(np.full((H, W, 3), BACKGROUND, F), np.full((H, W), R.MISS, np.uint32))
    n_c = MR.reproject(c["hist"], c["hnd"], c["hai"], c["hcam"], c["image"], c["tf"], c["nd"], c["ai"], c["cam"])[2]["n_c"]
    miss = MR.miss_pixels(c["nd"], c["ai"])
    hit = R.guide_good(c["nd"], c["ai"]) & ~miss
    for var in (False, True):
        rgbn, _ = host(dict(c, hnd=solid_nd, hai=solid_ai), var)
        assert np.array_equal(rgbn[..., 3][miss], n_c[miss]) and (rgbn[..., 3][hit] > n_c[hit]).any()
        rgbn, _ = host(dict(c, hnd=empty_nd, hai=empty_ai), var)
        assert np.array_equal(rgbn[..., 3][hit], n_c[hit]) and (rgbn[..., 3][miss] > n_c[miss]).any()


# ---- 2. hit pixels are untouched --------------------------------------------------------------------------

@pytest.mark.parametrize("move", sorted(MOVES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_hit_pixels_keep_their_bits(shape, move):
    c = case(*shape, move)
    keep = ~MR.miss_pixels(c["nd"], c["ai"])              # hits, and pixels that are not guide-good
    assert keep.any() and (~keep).any()
    for var in (False, True):
        for prm in PRMS:
            on, on_s2 = host(c, var, **prm)
            off, off_s2 = host(c, var, misses=False, **prm)
            assert same_bits(on[keep], off[keep]), (var, prm)
            assert not same_bits(on[~keep], off[~keep])
            if var:
                assert same_bits(on_s2[keep], off_s2[keep]), prm


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_with_no_miss_the_result_is_the_existing_entries(shape):
    """reproject_ref's wall without the sky, seen where the hole is out of view: no current pixel is a miss."""
    W, H = shape
    c = dict(case(W, H, "sideways"))
    cam = R.camera(W, H, pos=(-6.0, 0.1, 0.0), yaw=8.0)
    nd, ai = R.raycast(cam, W, H)
    assert not (R.id_word(ai) == R.MISS).any()
    c.update(nd=nd, ai=ai, cam=cam)
    for var in (False, True):
        on, on_s2 = host(c, var)
        off, off_s2 = host(c, var, misses=False)
        assert same_bits(on, off) and (not var or same_bits(on_s2, off_s2))


# ---- 3. the same camera over an all-miss view ------------------------------------------------------------

@pytest.mark.parametrize("max_history,n_c", [(64.0, 2), (3.0, 2), (8.0, 1), (64.0, 0)])
def test_same_camera_all_miss_interior(max_history, n_c):
    """n_h = 8 in every history pixel: u * 8 and the sums of such products are exact, so sn / sw is 8 whatever the
    weights, and n_out = n_c + g_min(8, max_history) (n_hist itself where the pixel has no frame)."""
    W, H = 24, 16
    cam = R.camera(W, H, pos=(0.0, 0.0, 0.0))
    nd = np.zeros((H, W, 4), F)
    nd[..., 3] = -1.0
    ai = rtamd.pack_albedo_id(np.full((H, W, 3), BACKGROUND, F), np.full((H, W), R.MISS, np.uint32))
    rng = np.random.default_rng(5)
    hist = np.empty((H, W, 4), F)
    hist[..., :3] = rng.random((H, W, 3), dtype=F)
    hist[..., 3] = 8.0
    image = np.empty((H, W, 4), F)
    image[..., :3] = rng.random((H, W, 3), dtype=F)
    image[..., 3] = 1.0
    c = dict(hist=hist, hnd=nd, hai=ai, hs2=np.full((H, W), 0.04, F), hcam=cam, image=image,
             m2=np.full((H, W, 4), 0.09, F), tf=np.full(6, n_c, np.int32), nd=nd, ai=ai, cam=cam)
    want = F(n_c) + min(F(8.0), F(max_history))
    for var in (False, True):
        rgbn, s2 = host(c, var, max_history=max_history)
        assert (rgbn[1:-1, 1:-1, 3] == want).all(), (var, np.unique(rgbn[..., 3]))
        off, _ = host(c, var, misses=False, max_history=max_history)
        assert (off[..., 3] == F(n_c)).all()
        if var:
            assert (s2[1:-1, 1:-1] >= 0).all()
    # under another background the history is refused: every pixel keeps (C, n_c)
    other = rtamd.pack_albedo_id(np.full((H, W, 3), (0.5, 0.7, 0.99), F), np.full((H, W), R.MISS, np.uint32))
    rgbn, _ = host(dict(c, hai=other), False, max_history=max_history)
    assert (rgbn[..., 3] == F(n_c)).all() and same_bits(rgbn[..., :3], image[..., :3])


# ---- 4. the arguments -------------------------------------------------------------------------------------

def test_bad_arguments_are_refused():
    W, H = SHAPES[0]
    c = case(W, H, "sideways")
    L = rtamd.amd()
    fp = lambda a: np.ascontiguousarray(a, F).ctypes.data_as(_lib.c_float_p)  # noqa: E731
    ip = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))  # noqa: E731
    out, s2 = np.zeros((H, W, 4), F), np.zeros((H, W), F)
    nt = c["tf"].size

    def call(**kw):
        g = lambda k, v: kw.get(k, v)   # noqa: E731
        return L.rt_reproject_misses_host(g("hist", fp(c["hist"])), g("hnd", fp(c["hnd"])), g("hai", fp(c["hai"])),
                                          g("hs2", fp(c["hs2"])), g("hcam", fp(c["hcam"])), g("image", fp(c["image"])),
                                          g("m2", fp(c["m2"])), g("tf", ip(c["tf"])), g("nt", nt), g("nd", fp(c["nd"])),
                                          g("ai", fp(c["ai"])), g("cam", fp(c["cam"])), g("w", W), g("h", H), g("p", None),
                                          g("out", fp(out)), g("s2", fp(s2)))

    assert call() == 0
    assert call(hs2=None, m2=None, s2=None) == 0                       # the no-variance form
    # the NULL-mix rule: all three or none
    for mix in (dict(hs2=None), dict(m2=None), dict(s2=None), dict(hs2=None, m2=None), dict(hs2=None, s2=None),
                dict(m2=None, s2=None)):
        assert call(**mix) == -1, mix
    flat = np.array(c["hcam"])
    flat[16:19] = flat[12:15] * F(2)                                   # a singular history camera

    def params(cos_min=0.9, kz=0.1, max_history=64.0, reserved=None):
        p = _lib.RtReprojectParams()
        p.cos_min, p.kz, p.max_history = cos_min, kz, max_history
        if reserved is not None:
            p.reserved[reserved] = 1
        return ctypes.byref(p)

    assert call(p=params()) == 0
    nan, inf = float("nan"), float("inf")
    for none in ({}, dict(hs2=None, m2=None, s2=None)):
        for bad in (dict(hist=None), dict(hnd=None), dict(hai=None), dict(hcam=None), dict(image=None), dict(tf=None),
                    dict(nd=None), dict(ai=None), dict(cam=None), dict(out=None), dict(nt=nt + 1), dict(w=0), dict(h=0),
                    dict(hcam=fp(flat)), dict(tf=ip(np.where(np.arange(nt) == 0, -1, c["tf"])))):
            assert call(**dict(none, **bad)) == -1, (none, bad)
        for bad in (dict(cos_min=1.5), dict(cos_min=nan), dict(kz=-0.1), dict(kz=inf), dict(max_history=0.0),
                    dict(max_history=nan)):
            assert call(**dict(none, p=params(**bad))) == -1, bad
        # every reserved slot is refused, as in the existing entries: the switch is not in the struct
        for slot in range(5):
            assert call(**dict(none, p=params(reserved=slot))) == -1, slot
    with pytest.raises(rtamd.RTError) as e:
        host(dict(c, hcam=flat), True)
    assert e.value.code == -1
    assert L.rt_set_reproject_misses(None, 1) == -1


# ---- 5. what the switch does to the refined pose's selection ---------------------------------------------

def test_fewer_tiles_qualify_for_refinement_with_the_switch_on():
    """tests/test_gpu_reproject_miss.py's refined pose on the CPU: scene 8 at 40x24 after a 0.05 move, 8 oracle frames
    behind the history, 1 frame at B, tiles holding a pixel short of 1 + 3 frames (rt_tile_reach_host, rt_refine_select)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import reproject_quality as Q
    e = Q.experiment(8, 40, 24, 8, 1, 0.05)
    picked = {}
    for misses in (False, True):
        out = rtamd.reproject_host(e["hist"], e["hnd"], e["hai"], e["hcam"], e["image"], e["tf"], e["nd"], e["ai"], e["cam"],
                                   misses=misses)
        picked[misses] = rtamd.refine_select(rtamd.tile_reach_host(out, 4.0))
        miss = ~e["hit"]
        assert miss.any() and (~miss).any()
        assert ((out[..., 3][miss] > 1.0).mean() > 0.9) == misses
    assert picked[True].size == 15
    assert 0 < picked[True].sum() < picked[False].sum() <= 15, (picked[True].sum(), picked[False].sum())
    assert not (picked[True] & ~picked[False]).any()      # the on selection is a subset of the off one

"""The variance carried through reprojection and the preview filter over the reprojected view on the host
(rt.h rt_history_variance_host, rt_reproject_variance_host, rt_denoise_reprojected_host) against
tests/reproject_var_ref.py, the NumPy float32 restatement written from rt.h, bit for bit, and what the
definition means case by case.  No GPU.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

import rtamd
from rtamd import _lib
import reproject_ref as R
import reproject_var_ref as V

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
POSE_H = dict(pos=(0.0, 0.0, 0.0))
POSE_C = dict(pos=(0.7, 0.1, 0.0), yaw=2.0, pitch=0.0, roll=16.0)   # tests/test_reproject_host.py's move
SHAPES = [(13, 9), (21, 17)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def colours(ai, rng, lo=0.2):
    ids = R.id_word(ai)
    base = np.stack([((ids >> s) & 7).astype(F) / F(14) for s in (0, 16, 2)], axis=-1) + F(lo)
    return np.clip(base + rng.random(base.shape, dtype=F) * F(0.3), lo, 1.0).astype(F)


@functools.lru_cache(maxsize=None)
def case(W, H):
    """Seeded inputs of one reprojection with variance: misses, NaN / inf in rgb and M2.w, zero and unequal tile
    counts, history pixels with n = 0, unknown history s2 (negative and NaN), taps outside the image."""
    rng = np.random.default_rng(W * 100 + H + 7)
    hcam, cam = R.camera(W, H, **POSE_H), R.camera(W, H, **POSE_C)
    hnd, hai = R.raycast(hcam, W, H)
    nd, ai = R.raycast(cam, W, H)
    hist = np.empty((H, W, 4), F)
    hist[..., :3] = colours(hai, rng)
    hist[..., 3] = 8.0
    hist[H // 2, ::3, 3] = 0.0
    hs2 = (rng.random((H, W), dtype=F) * F(0.2)).astype(F)
    hs2[::2, 1::3] = -1.0
    hs2[:H // 2 + 1, :W // 2] = -1.0                      # a block: pixels all of whose taps are unknown
    hs2[1::4, ::5] = np.nan
    hs2[0, 0] = 0.0
    image = np.empty((H, W, 4), F)
    image[..., :3] = colours(ai, rng)
    image[..., 3] = 1.0
    image[H // 2, W // 2 + 2, 0] = np.nan
    image[H - 2, 2, 1] = np.inf
    image[2, W - 3, 2] = -np.inf
    m2 = (rng.random((H, W, 4), dtype=F) * F(0.5)).astype(F)
    m2[1, 2, 3] = np.nan
    m2[H - 1, W - 1, 3] = np.inf
    m2[3, 3, 3] = -0.25                                   # a negative M2.w clamps at +0
    nt = ((W + 7) // 8) * ((H + 7) // 8)
    tf = (np.arange(nt, dtype=np.int32) % 3 + 1).astype(np.int32)   # 1 (own s2 unknown), 2, 3
    tf[nt - 1] = 0
    c = dict(hist=hist, hnd=hnd, hai=hai, hs2=hs2, hcam=hcam, image=image, m2=m2, tf=tf, nd=nd, ai=ai, cam=cam)
    for a in c.values():
        a.setflags(write=False)
    return c


def host_reproject(c, **prm):
    return rtamd.reproject_variance_host(c["hist"], c["hnd"], c["hai"], c["hs2"], c["hcam"], c["image"], c["m2"], c["tf"],
                                         c["nd"], c["ai"], c["cam"], **prm)


def ref_reproject(c, **prm):
    full = dict(zip(("cos_min", "kz", "max_history"), R.DEFAULTS))
    full.update(prm)
    return V.reproject(c["hist"], c["hnd"], c["hai"], c["hs2"], c["hcam"], c["image"], c["m2"], c["tf"], c["nd"], c["ai"],
                       c["cam"], **full)


def ref_filter(rgbn, s2, nd, ai, guides=True, **prm):
    """The restated level 0, then rt_denoise's levels (restated in tests/test_denoise_host.py) over exactly it."""
    V0, cls = V.level0(rgbn, s2, ai)
    image, m2, tf = V.as_moments(rgbn, V0)
    if guides is None:
        return rtamd.denoise_host(image, m2, tf, **prm), cls
    return rtamd.denoise_guided_host(image, m2, tf, nd, ai, guides=guides, **prm), cls


def check_filter(rgbn, s2, nd, ai):
    """Guided at the defaults, unguided and at other parameters -> the level-0 classes."""
    for guides, prm in ((True, {}), (None, {}), ((0.0, 0.0, 0.0), {}), ((2.0, 0.5, 0.25), dict(levels=2, k=1.5)),
                        (None, dict(levels=5, k=4.0)), (True, dict(levels=1))):
        got = rtamd.denoise_reprojected_host(rgbn, s2, nd, ai, guides=guides, **prm)
        zero = guides is not None and guides is not True and not any(guides)
        ref, cls = ref_filter(rgbn, s2, nd, ai, guides=None if zero else guides, **prm)
        assert same_bits(got, ref), (guides, prm, int((got.view(np.uint32) != ref.view(np.uint32)).any(axis=-1).sum()))
    return cls


# ---- 1. the host functions against the restatement, bit for bit ------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_matches_numpy_bit_for_bit(shape):
    W, H = shape
    c = case(W, H)
    assert same_bits(rtamd.history_variance_host(c["image"], c["m2"], c["tf"]), V.history_s2(c["image"], c["m2"], c["tf"]))
    for prm in ({}, dict(kz=0.0), dict(cos_min=0.999, kz=0.02), dict(max_history=3.0)):
        rgbn, s2 = host_reproject(c, **prm)
        ref, ref_s2, info = ref_reproject(c, **prm)
        assert same_bits(rgbn, ref) and same_bits(s2, ref_s2), prm
        # the result word is rt_reproject_host's
        plain = rtamd.reproject_host(c["hist"], c["hnd"], c["hai"], c["hcam"], c["image"], c["tf"], c["nd"], c["ai"], c["cam"], **prm)
        assert same_bits(rgbn, plain), prm
    rgbn, s2 = host_reproject(c)
    _, _, info = ref_reproject(c)
    # what the inputs hold, and every rule of the result's s2
    ids = R.id_word(c["ai"])
    assert (ids == R.MISS).any() and (R.id_word(c["hai"]) == R.MISS).any()
    assert (~np.isfinite(c["image"][..., :3])).any() and (~np.isfinite(c["m2"][..., 3])).any()
    assert (c["tf"] == 0).any() and len(set(c["tf"].tolist())) >= 3 and (c["hist"][..., 3] <= 0).any()
    assert (c["hs2"] < 0).any() and np.isnan(c["hs2"]).any()
    taps = info["taps"]
    assert any((t["considered"] & ~t["q_in"]).any() for t in taps)                          # taps outside the image
    assert info["tap_unknown"].any()                                                         # an accepted tap with s2 unknown
    rule, own, hs = info["rule"], info["s2_c"] >= 0, info["s2_hist"] >= 0
    assert (rule == V.OWN).any() and (rule == V.HISTORY).any()
    blend = rule == V.BLEND
    for a in (True, False):
        for b in (True, False):
            assert (blend & (own == a) & (hs == b)).any(), (a, b)                            # both, either, neither known
    assert ((s2 >= 0) & blend).any() and (~(s2 >= 0) & blend).any()
    # the filter over this view: every level-0 class
    cls = check_filter(rgbn, s2, c["nd"], c["ai"])
    assert all((cls == k).any() for k in (V.BAD, V.KNOWN, V.SPATIAL))


@functools.lru_cache(maxsize=None)
def oracle_experiment(frames_b):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import reproject_filter_quality as T
    return T, T.experiment(6, 16, 16, 8, frames_b)


@pytest.mark.parametrize("frames_b", [1, 2])
def test_the_oracle_experiment_matches_numpy_bit_for_bit(frames_b):
    """The quality tool's experiment (scene 6, oracle frames and moments, a sideways move) at 16x16."""
    T, e = oracle_experiment(frames_b)
    c = dict(e, tf=np.full(4, e["tf"], np.int32))
    assert same_bits(e["hs2"], V.history_s2(e["hist"], T.moments_of(T.Q.scene_at(6, 16, 16), 8, T.SEED), 8))
    rgbn, s2 = T.reproject(e)
    ref, ref_s2, info = ref_reproject(c)
    assert same_bits(rgbn, ref) and same_bits(s2, ref_s2)
    assert same_bits(rgbn, T.Q.reproject(e))
    assert (info["rule"] == V.BLEND).any() and (info["rule"] == V.OWN).any() and (s2 >= 0).any()
    cls = check_filter(rgbn, s2, e["nd"], e["ai"])
    assert (cls == V.KNOWN).any()
    if frames_b == 1:
        assert (cls == V.SPATIAL).any()            # one frame: a fresh pixel has no variance of its own


# ---- 2. the s2 cases one by one --------------------------------------------------------------------------

def same_view(W=16, H=8, n_h=8.0, n_c=2, hs2=0.04, m2w=0.09, miss_cols=2):
    """The history seen from the current camera, one surface (id 5) with `miss_cols` columns of misses on the
    right: every hit pixel blends with its own history pixel."""
    cam = R.camera(W, H, pos=(0.0, 0.0, 0.0))
    nd = np.zeros((H, W, 4), F)
    nd[..., 2], nd[..., 3] = 1.0, 5.0
    ids = np.full((H, W), 5, np.uint32)
    if miss_cols:
        ids[:, -miss_cols:] = R.MISS
        nd[:, -miss_cols:] = (0.0, 0.0, 0.0, -1.0)
    ai = rtamd.pack_albedo_id(np.full((H, W, 3), 0.5, F), ids)
    rng = np.random.default_rng(3)
    hist = np.empty((H, W, 4), F)
    hist[..., :3] = rng.random((H, W, 3), dtype=F)
    hist[..., 3] = n_h
    image = np.empty((H, W, 4), F)
    image[..., :3] = rng.random((H, W, 3), dtype=F)
    image[..., 3] = 1.0
    m2 = np.zeros((H, W, 4), F)
    m2[..., 3] = m2w
    return dict(hist=hist, hnd=nd, hai=ai, hs2=np.full((H, W), hs2, F), hcam=cam, image=image, m2=m2,
                tf=np.full(((W + 7) // 8) * ((H + 7) // 8), n_c, np.int32), nd=nd, ai=ai, cam=cam)


def test_the_s2_cases_one_by_one():
    c = same_view()
    hit = R.id_word(c["ai"]) != R.MISS
    own = F(0.09) / (F(2) - F(1))
    rgbn, s2 = host_reproject(c)
    assert (rgbn[..., 3][hit] > 2.0).all()
    # not reprojected (a miss): the pixel's own s2
    assert (s2[~hit] == own).all() and (rgbn[..., 3][~hit] == 2.0).all()
    # both known: between the two, and the count-weighted mean to rounding
    assert ((s2[hit] > 0.04) & (s2[hit] < own)).all()
    exact = (2.0 * float(own) + 8.0 * float(F(0.04))) / 10.0
    assert np.allclose(s2[hit], exact, rtol=1e-4, atol=0)
    # n_c == 0: the history's
    _, s2 = host_reproject(dict(c, tf=np.zeros_like(c["tf"])))
    assert np.allclose(s2[hit], 0.04, rtol=1e-5, atol=0) and (s2[~hit] == -1.0).all()
    # own unknown (one frame; M2.w not finite): the history's
    for d in (dict(tf=np.ones_like(c["tf"])), dict(m2=np.full_like(c["m2"], np.nan))):
        _, s2 = host_reproject(dict(c, **d))
        assert np.allclose(s2[hit], 0.04, rtol=1e-5, atol=0) and (s2[~hit] == -1.0).all(), d
    # history unknown (negative, NaN): the pixel's own
    for unknown in (-1.0, np.nan, -np.inf):
        _, s2 = host_reproject(dict(c, hs2=np.full_like(c["hs2"], unknown)))
        assert (s2 == own).all(), unknown
    # both unknown
    _, s2 = host_reproject(dict(c, hs2=np.full_like(c["hs2"], -3.0), tf=np.ones_like(c["tf"])))
    assert (s2 == -1.0).all()
    # rejected (the history holds another surface): the pixel's own, and the count did not grow
    other = c["hai"].copy()
    other.view(np.uint32)[..., 3] = np.where(hit, 6, R.MISS)
    rgbn, s2 = host_reproject(dict(c, hai=other))
    assert (s2 == own).all() and (rgbn[..., 3] == 2.0).all()


@pytest.mark.parametrize("const", [0.04, 0.0, 1.0e-30, 3.0e30])
def test_the_same_constant_on_both_sides_is_kept_exactly(const):
    """ss / sws with every s equal is not that s to the bit in general, so the taps here carry all the weight in
    one: the history seen from the same camera is exact wherever one tap's weight is 1; everywhere else the
    result stays within an ulp or two of the constant."""
    c = same_view(hs2=const, m2w=const)           # n_c = 2: own s2 = const / 1
    rgbn, s2 = host_reproject(c)
    _, ref_s2, info = ref_reproject(c)
    assert same_bits(s2, ref_s2)
    hit = R.id_word(c["ai"]) != R.MISS
    k = F(const)
    assert (s2[~hit] == k).all()
    ax = info["fx"] - np.floor(info["fx"])
    ay = info["fy"] - np.floor(info["fy"])
    exact = hit & (ax == 0) & (ay == 0)           # the projection lands on the pixel: u = 1 * 1, ss / sws = s
    assert exact.any() and (s2[exact] == k).all()
    assert np.allclose(s2[hit], k, rtol=4e-7, atol=0)


# ---- 3. level 0 ------------------------------------------------------------------------------------------

def flat_view(W=13, H=9, n=4.0, seed=2):
    rng = np.random.default_rng(seed)
    rgbn = np.empty((H, W, 4), F)
    rgbn[..., :3] = F(0.4) + rng.random((H, W, 3), dtype=F) * F(0.2)
    rgbn[..., 3] = n
    nd = np.zeros((H, W, 4), F)
    nd[..., 2], nd[..., 3] = 1.0, 5.0
    ai = rtamd.pack_albedo_id(np.full((H, W, 3), 0.5, F), np.full((H, W), 5, np.uint32))
    return rgbn, nd, ai


def through_rt_denoise(rgbn, V0, levels=1):
    image, m2, tf = V.as_moments(rgbn, V0)
    return rtamd.denoise_host(image, m2, tf, levels=levels)


def test_level0_known_variance_is_s2_over_n():
    rgbn, nd, ai = flat_view()
    rgbn[..., 3] = np.arange(1, 13 * 9 + 1, dtype=F).reshape(9, 13)
    s2 = (np.random.default_rng(4).random((9, 13), dtype=F) * F(0.1)).astype(F)
    s2[2, 2] = 0.0
    got = rtamd.denoise_reprojected_host(rgbn, s2, nd, ai, levels=1, guides=None)
    assert same_bits(got, through_rt_denoise(rgbn, (s2 / rgbn[..., 3]).astype(F)))
    assert not same_bits(got[..., :3], rgbn[..., :3])


def test_level0_spatial_estimate_does_not_cross_an_id_boundary():
    rgbn, nd, ai = flat_view(W=16, H=12, n=1.0)
    ai = ai.copy()
    ai.view(np.uint32)[:, 8:, 3] = 6
    rgbn[:, 8:, :3] += F(10.0)                    # a step that would dominate any spread taken across it
    s2 = np.full((12, 16), -1.0, F)
    V0, cls = V.level0(rgbn, s2, ai)
    assert (cls == V.SPATIAL).all()
    y = V.lum(rgbn).astype(np.float64)
    for (yy, xx) in ((5, 7), (5, 8), (0, 0), (11, 15)):
        x0, x1 = (max(0, xx - 2), min(8, xx + 3)) if xx < 8 else (max(8, xx - 2), min(16, xx + 3))
        patch = y[max(0, yy - 2):min(12, yy + 3), x0:x1]
        assert np.isclose(V0[yy, xx], patch.var(ddof=1), rtol=1e-4), (yy, xx)
    assert V0.max() < 0.1                          # nowhere the step's 100
    for guides in (None, True):
        got = rtamd.denoise_reprojected_host(rgbn, s2, nd, ai, levels=1, guides=guides)
        ref, _ = ref_filter(rgbn, s2, nd, ai, guides=guides, levels=1)
        assert same_bits(got, ref)


def test_level0_fewer_than_two_taps_is_plus_zero():
    rgbn, nd, ai = flat_view()
    ai = ai.copy()
    ai.view(np.uint32)[4, 6, 3] = 77              # a pixel alone on its surface
    lone = np.zeros((9, 13), bool)
    lone[4, 6] = True
    s2 = np.where(lone, F(-1.0), F(0.05)).astype(F)
    V0, cls = V.level0(rgbn, s2, ai)
    assert cls[4, 6] == V.SPATIAL and V0[4, 6] == 0.0 and not np.signbit(V0[4, 6])
    expect = np.where(lone, F(0.0), F(0.05) / rgbn[..., 3]).astype(F)
    got = rtamd.denoise_reprojected_host(rgbn, s2, nd, ai, levels=1, guides=None)
    assert same_bits(got, through_rt_denoise(rgbn, expect))
    # a 1x1 image: one tap
    one = rtamd.denoise_reprojected_host(rgbn[:1, :1], s2[:1, :1] * 0 - 1, nd[:1, :1], ai[:1, :1])
    assert same_bits(one[..., :3], rgbn[:1, :1, :3]) and one[0, 0, 3] == 1.0


def test_level0_a_bad_pixel_passes_through_and_is_never_a_tap():
    rgbn, nd, ai = flat_view(n=1.0)
    rgbn[3, 3, 1] = np.nan
    rgbn[5, 8, 0] = np.inf
    rgbn[1, 10, 3] = 0.0                           # n = 0: nothing behind the pixel
    rgbn[7, 1, 3] = -2.0
    rgbn[7, 5, 3] = np.nan
    rgbn[6, 10, :3] = 1.0e3                        # finite, good, and it shows in its neighbours' spread
    s2 = np.full((9, 13), -1.0, F)
    bad = np.zeros((9, 13), bool)
    for p in ((3, 3), (5, 8), (1, 10), (7, 1), (7, 5)):
        bad[p] = True
    V0, cls = V.level0(rgbn, s2, ai)
    assert np.array_equal(cls == V.BAD, bad) and (cls[~bad] == V.SPATIAL).all()
    assert np.isfinite(V0[4, 4]) and V0[4, 4] < 0.1     # beside the NaN and the inf: they were not taps
    assert V0[5, 10] > 1.0e4                            # beside the outlier: it was
    for levels in (1, 3):
        for guides in (None, True):
            got = rtamd.denoise_reprojected_host(rgbn, s2, nd, ai, levels=levels, guides=guides)
            ref, _ = ref_filter(rgbn, s2, nd, ai, guides=guides, levels=levels)
            assert same_bits(got, ref)
            assert same_bits(got[bad][:, :3], rgbn[bad][:, :3]) and (got[..., 3] == 1.0).all()
    # with the bad pixels' values replaced the good pixels come out the same: they were never taps
    other = rgbn.copy()
    for p in ((1, 10), (7, 1), (7, 5)):            # bad by their n: they stay bad with any rgb
        other[p][:3] = 123.0
    a = rtamd.denoise_reprojected_host(rgbn, s2, nd, ai, guides=None)
    b = rtamd.denoise_reprojected_host(other, s2, nd, ai, guides=None)
    assert same_bits(a[~bad], b[~bad])


@pytest.mark.parametrize("known", [True, False])
def test_a_constant_image_comes_back_unchanged(known):
    rgbn = np.empty((23, 37, 4), F)
    rgbn[...] = np.array([0.3, 1.7, 0.011, 3.0], F)
    nd = np.zeros((23, 37, 4), F)
    nd[..., 2], nd[..., 3] = 1.0, 5.0
    ai = rtamd.pack_albedo_id(np.full((23, 37, 3), 0.5, F), np.full((23, 37), 5, np.uint32))
    s2 = np.full((23, 37), 0.2 if known else -1.0, F)
    for guides in (None, True):
        for levels in (1, 3, 5):
            out = rtamd.denoise_reprojected_host(rgbn, s2, nd, ai, levels=levels, guides=guides)
            assert same_bits(out[..., :3], rgbn[..., :3]) and (out[..., 3] == 1.0).all()


def test_smoothing_of_a_noisy_flat_one_frame_view():
    """A flat 64x64 signal with iid noise (sigma 0.05 per channel), n = 1, s2 unknown everywhere, one id: the
    spatial estimate alone drives the filter.  Measured on the host path at the defaults: RMSE after / before
    = 0.1368 (profiles/reproject_filter_quality.json, flat_noise); the bound is halfway between that and 1."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import json
    import reproject_filter_quality as T
    ratio = T.flat_noise_ratio()
    rec = json.load(open(os.path.join(REPO, "profiles", "reproject_filter_quality.json")))["flat_noise"]
    print(f"smoothing of a one-frame view: RMSE after / before = {ratio:.4f} (recorded {rec['ratio']})")
    assert rec["ratio"] == MEASURED_FLAT_RATIO and {k: rec[k] for k in T.FLAT} == T.FLAT
    assert ratio <= (MEASURED_FLAT_RATIO + 1.0) / 2.0


MEASURED_FLAT_RATIO = 0.1368


# ---- 4. arguments ----------------------------------------------------------------------------------------

def fp(a):
    return np.ascontiguousarray(a, F).ctypes.data_as(_lib.c_float_p)


def ip(a):
    return np.ascontiguousarray(a, np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def test_argument_errors_of_the_three_host_functions():
    L = rtamd.amd()
    W, H = SHAPES[0]
    c = case(W, H)
    nt = c["tf"].size
    s2 = np.zeros((H, W), F)
    out = np.zeros((H, W, 4), F)

    def hv(**kw):
        return L.rt_history_variance_host(kw.get("image", fp(c["image"])), kw.get("m2", fp(c["m2"])), kw.get("tf", ip(c["tf"])),
                                          kw.get("nt", nt), kw.get("w", W), kw.get("h", H), kw.get("out", fp(s2)))

    assert hv() == 0
    for bad in (dict(image=None), dict(m2=None), dict(tf=None), dict(out=None), dict(nt=nt - 1), dict(w=0), dict(h=-1),
                dict(w=1 << 20), dict(tf=ip(np.where(np.arange(nt) == 1, -1, c["tf"])))):
        assert hv(**bad) == -1, bad

    def rv(**kw):
        g = lambda k, v: kw.get(k, v)   # noqa: E731
        return L.rt_reproject_variance_host(g("hist", fp(c["hist"])), g("hnd", fp(c["hnd"])), g("hai", fp(c["hai"])),
                                            g("hs2", fp(c["hs2"])), g("hcam", fp(c["hcam"])), g("image", fp(c["image"])),
                                            g("m2", fp(c["m2"])), g("tf", ip(c["tf"])), g("nt", nt), g("nd", fp(c["nd"])),
                                            g("ai", fp(c["ai"])), g("cam", fp(c["cam"])), g("w", W), g("h", H), g("p", None),
                                            g("out", fp(out)), g("s2", fp(s2)))

    assert rv() == 0
    flat = np.array(c["hcam"])
    flat[16:19] = flat[12:15] * F(2)              # a singular history camera
    rp = _lib.RtReprojectParams()
    rp.cos_min, rp.kz, rp.max_history = 1.5, 0.1, 64.0
    rsv = _lib.RtReprojectParams()
    rsv.cos_min, rsv.kz, rsv.max_history = 0.9, 0.1, 64.0
    rsv.reserved[1] = 1
    for bad in (dict(hist=None), dict(hnd=None), dict(hai=None), dict(hs2=None), dict(hcam=None), dict(image=None), dict(m2=None),
                dict(tf=None), dict(nd=None), dict(ai=None), dict(cam=None), dict(out=None), dict(s2=None), dict(nt=nt + 1),
                dict(w=0), dict(h=0), dict(hcam=fp(flat)), dict(p=ctypes.byref(rp)), dict(p=ctypes.byref(rsv)),
                dict(tf=ip(np.where(np.arange(nt) == 0, -1, c["tf"])))):
        assert rv(**bad) == -1, bad
    with pytest.raises(rtamd.RTError) as e:
        host_reproject(dict(c, hcam=flat))
    assert e.value.code == -1

    rgbn, var = host_reproject(c)

    def dr(**kw):
        g = lambda k, v: kw.get(k, v)   # noqa: E731
        return L.rt_denoise_reprojected_host(g("rgbn", fp(rgbn)), g("s2", fp(var)), g("nd", fp(c["nd"])), g("ai", fp(c["ai"])),
                                             g("w", W), g("h", H), g("p", None), g("g", None), g("out", fp(out)))

    assert dr() == 0
    dp = _lib.RtDenoiseParams()
    dp.levels, dp.k = 6, 3.0
    dk = _lib.RtDenoiseParams()
    dk.levels, dk.k = 3, 0.0
    dres = _lib.RtDenoiseParams()
    dres.levels, dres.k = 3, 3.0
    dres.reserved[0] = 1
    gneg = _lib.RtGuideParams()
    gneg.kn, gneg.kz, gneg.ka = -1.0, 1.0, 1.0
    gres = _lib.RtGuideParams()
    gres.kn, gres.kz, gres.ka = 0.5, 1.0, 1.0
    gres.reserved[4] = 1
    for bad in (dict(rgbn=None), dict(s2=None), dict(nd=None), dict(ai=None), dict(out=None), dict(w=0), dict(h=0),
                dict(w=1 << 20), dict(p=ctypes.byref(dp)), dict(p=ctypes.byref(dk)), dict(p=ctypes.byref(dres)),
                dict(g=ctypes.byref(gneg)), dict(g=ctypes.byref(gres))):
        assert dr(**bad) == -1, bad
    with pytest.raises(rtamd.RTError) as e:
        rtamd.denoise_reprojected_host(rgbn, var, c["nd"], c["ai"], levels=0)
    assert e.value.code == -1


def test_null_contexts_are_rejected():
    L = rtamd.amd()
    out = np.zeros(4, F)
    assert L.rt_set_history_variance(None, 1) == -1
    assert L.rt_read_reprojected_variance(None, out.ctypes.data_as(_lib.c_float_p)) == -1
    assert L.rt_denoise_reprojected(None, None, None) == -1


def test_recorded_resources():
    """profiles/reproject_var_resources.txt: no scratch, no spills, no LDS in the two new kernels and the new
    prologue, and the parent's kernels beside them with the figures of profiles/reproject_resources.txt."""
    import re
    rows = {}
    for ln in open(os.path.join(REPO, "profiles", "reproject_var_resources.txt")):
        if " VGPR " in ln:
            rows[ln.split()[0]] = {k: int(v) for k, v in re.findall(r"(VGPR|SGPR|spillV|spillS|scratch|LDS)\s+(\d+)", ln)}

    def one(part):
        hits = [v for k, v in rows.items() if part in k]
        assert len(hits) == 1, part
        return hits[0]

    for new in ("history_var_kernel", "reproject_var_kernel", "dn_prologue_reprojected_kernel"):
        f = one(new)
        assert f["scratch"] == 0 and f["spillV"] == 0 and f["spillS"] == 0 and f["LDS"] == 0 and 0 < f["VGPR"] <= 64, (new, f)
    for ln in open(os.path.join(REPO, "profiles", "reproject_resources.txt")):
        name = ln.split()[0]
        assert rows[name] == {k: int(v) for k, v in re.findall(r"(VGPR|SGPR|spillV|spillS|scratch|LDS)\s+(\d+)", ln)}, name

"""CPU tests of the guided preview filter (rt.h rt_denoise_guided_host) and of the first-hit reference
the GPU tests compare against (tests/features_ref.py): the identity with rt_denoise_host at k = 0, a
numpy float32 restatement of rt.h's guide factor bit for bit, argument checks and the struct layout,
a synthetic albedo step no tap may cross, and the caps on tied pixels in the reference.
"""
import ctypes

import numpy as np
import pytest

import rtamd
from rtamd import _lib

import features_ref
from test_denoise_host import F, gmax0, make_inputs, n_tiles, same_bits, shifted

MISS = np.uint32(0xFFFFFFFF)


def make_guides(W, H, seed, miss=True, bad=True):
    """Seeded random first-hit buffers: unit-ish normals, depths with a step, albedo with a soft edge,
    ids of hits; with `miss` a block of miss pixels (N = 0, t = -1, id RT_FEATURE_MISS), with `bad` a few
    pixels whose N, t or A is not finite."""
    rng = np.random.default_rng(seed + 1000)
    nd = np.empty((H, W, 4), F)
    n = rng.standard_normal((H, W, 3)).astype(F)
    nd[..., :3] = n / np.sqrt((n * n).sum(-1, keepdims=True)).astype(F)
    nd[..., 3] = F(2.0) + rng.random((H, W), dtype=F)
    nd[H // 2:, :, 3] += F(3.0)
    alb = rng.random((H, W, 3), dtype=F) * F(0.3)
    alb[:, : W // 3] += F(0.5)
    ids = (rng.integers(1, 4, (H, W)).astype(np.uint32) | (rng.integers(0, 50, (H, W)).astype(np.uint32) << 16))
    if miss:
        y0, x0 = H // 4, W // 2
        nd[y0:y0 + max(2, H // 3), x0:, :3] = F(0.0)
        nd[y0:y0 + max(2, H // 3), x0:, 3] = F(-1.0)
        alb[y0:y0 + max(2, H // 3), x0:] = np.array([0.7, 0.8, 1.0], F)
        ids[y0:y0 + max(2, H // 3), x0:] = MISS
    if bad:
        nd[0, 1, 0] = np.nan
        nd[H - 1, W - 2, 3] = np.inf
        alb[H // 2, 0, 2] = -np.inf
    return nd, rtamd.pack_albedo_id(alb, ids)


def guide_weight_numpy(nd, ai, dy, dx, kn, kz, ka):
    """rt.h's g of the tap at offset (dy, dx) for every pixel, numpy float32 in the stated order."""
    one, zero = F(1.0), F(0.0)
    good = np.isfinite(nd).all(-1) & np.isfinite(ai[..., :3]).all(-1)
    hit = np.ascontiguousarray(ai).view(np.uint32)[..., 3] != MISS
    ndq, aiq = shifted(nd, dy, dx, F(0)), shifted(ai, dy, dx, F(0))
    goodq, hitq = shifted(good, dy, dx, False), shifted(hit, dy, dx, False)
    with np.errstate(all="ignore"):
        gn = gmax0(one - F(kn) * (one - ((nd[..., 0] * ndq[..., 0] + nd[..., 1] * ndq[..., 1]) + nd[..., 2] * ndq[..., 2])))
        tm = np.where(nd[..., 3] < ndq[..., 3], ndq[..., 3], nd[..., 3]).astype(F)   # g_max(t_p, t_q)
        gz = gmax0(one - F(kz) * (np.abs(nd[..., 3] - ndq[..., 3]) / (tm + F(1e-30))))
        ga = gmax0(one - F(ka) * ((np.abs(ai[..., 0] - aiq[..., 0]) + np.abs(ai[..., 1] - aiq[..., 1])) +
                                  np.abs(ai[..., 2] - aiq[..., 2])))
    gn = np.where(hit & (F(kn) != zero), gn, one).astype(F)
    gz = np.where(hit & (F(kz) != zero), gz, one).astype(F)
    ga = np.where(F(ka) != zero, ga, one).astype(F)
    g = ((gn * gz) * ga).astype(F)
    g = np.where(hit != hitq, zero, g)
    return np.where(good & goodq, g, one).astype(F)


def denoise_guided_numpy(image, m2, tile_frames, nd, ai, levels, k, kn, kz, ka):
    """test_denoise_host.denoise_numpy with rt.h's guide factor on each tap's weight."""
    image = np.asarray(image, F)
    H, W = image.shape[:2]
    tx, ty = (W + 7) // 8, (H + 7) // 8
    n = np.repeat(np.repeat(np.asarray(tile_frames, np.int32).reshape(ty, tx), 8, 0), 8, 1)[:H, :W]
    k = F(k)
    on = kn != 0 or kz != 0 or ka != 0   # all three 0: no guide applies at all
    h5 = {-2: F(0.0625), -1: F(0.25), 0: F(0.375), 1: F(0.25), 2: F(0.0625)}
    k3 = {-1: F(1.0), 0: F(2.0), 1: F(1.0)}
    h0 = F(0.140625)
    with np.errstate(all="ignore"):
        C = [image[..., c].copy() for c in range(3)]
        m2w = np.asarray(m2, F)[..., 3]
        good = np.isfinite((C[0] + C[1]) + C[2]) & np.isfinite(m2w)
        V = gmax0(m2w / (n.astype(F) * (n - 1).astype(F)))
        for lv in range(levels):
            s = 1 << lv
            acc, ws = np.zeros((H, W), F), np.zeros((H, W), F)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    use = shifted(good, dy, dx, False)
                    u = k3[dy] * k3[dx]
                    acc = np.where(use, acc + u * shifted(V, dy, dx, F(0)), acc)
                    ws = np.where(use, ws + u, ws)
            Vb = acc / ws
            yp = (C[0] + C[1]) + C[2]
            sw = np.zeros((H, W), F)
            sc = [np.zeros((H, W), F) for _ in range(3)]
            sv = np.zeros((H, W), F)
            for dy in (-2, -1, 0, 1, 2):
                for dx in (-2, -1, 0, 1, 2):
                    if dx == 0 and dy == 0:
                        continue
                    use = shifted(good, s * dy, s * dx, False)
                    Cq = [shifted(C[c], s * dy, s * dx, F(0)) for c in range(3)]
                    yq = (Cq[0] + Cq[1]) + Cq[2]
                    d = np.abs(yp - yq) / (k * np.sqrt(Vb + shifted(Vb, s * dy, s * dx, F(0))) + F(1e-30))
                    w = (h5[dy] * h5[dx]) * gmax0(F(1.0) - d)
                    if on:
                        w = w * guide_weight_numpy(nd, ai, s * dy, s * dx, kn, kz, ka)
                    sw = np.where(use, sw + w, sw)
                    for c in range(3):
                        sc[c] = np.where(use, sc[c] + w * (Cq[c] - C[c]), sc[c])
                    sv = np.where(use, sv + (w * w) * shifted(V, s * dy, s * dx, F(0)), sv)
            den = h0 + sw
            C = [np.where(good, C[c] + sc[c] / den, C[c]) for c in range(3)]
            V = np.where(good, ((h0 * h0) * V + sv) / (den * den), V)
        out = np.empty((H, W, 4), F)
        for c in range(3):
            out[..., c] = C[c]
        out[..., 3] = F(1.0)
    return out


@pytest.mark.parametrize("shape", [(16, 16), (13, 9)])
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_zero_guides_equal_unguided(shape, levels):
    W, H = shape
    img, m2, tf = make_inputs(W, H, seed=7 + levels)
    nd, ai = make_guides(W, H, seed=levels)
    ref = rtamd.denoise_host(img, m2, tf, levels=levels, k=3.0)
    out = rtamd.denoise_guided_host(img, m2, tf, nd, ai, levels=levels, k=3.0, guides=(0.0, 0.0, 0.0))
    assert same_bits(out, ref)


@pytest.mark.parametrize("shape", [(16, 16), (13, 9), (37, 23)])
@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("ks", [(1.0, 0.0, 0.0), (0.0, 2.0, 0.0), (0.0, 0.0, 1.5), (0.5, 4.0, 3.0)])
def test_host_matches_numpy_restatement(shape, levels, ks):
    W, H = shape
    img, m2, tf = make_inputs(W, H, seed=21)          # holds bad pixels (NaN / inf image, NaN M2)
    nd, ai = make_guides(W, H, seed=3)                # a miss block and non-finite guide pixels
    out = rtamd.denoise_guided_host(img, m2, tf, nd, ai, levels=levels, k=3.0, guides=ks)
    ref = denoise_guided_numpy(img, m2, tf, nd, ai, levels, 3.0, *ks)
    assert same_bits(out, ref)
    # and the guides do something here: the unguided result differs
    assert not same_bits(out, rtamd.denoise_host(img, m2, tf, levels=levels, k=3.0))


def _call_host(W, H, gp, n_tiles_arg=None, dp=None):
    img, m2, tf = make_inputs(W, H, seed=1, bad=False)
    nd, ai = make_guides(W, H, seed=1)
    out = np.empty_like(img)
    fp = ctypes.POINTER(ctypes.c_float)
    return _lib.amd().rt_denoise_guided_host(
        img.ctypes.data_as(fp), m2.ctypes.data_as(fp), tf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
        n_tiles(W, H) if n_tiles_arg is None else n_tiles_arg, nd.ctypes.data_as(fp), ai.ctypes.data_as(fp), W, H,
        dp, None if gp is None else ctypes.byref(gp), out.ctypes.data_as(fp))


def test_parameter_validation():
    def gp(kn=0.5, kz=0.5, ka=0.5, reserved=None):
        p = _lib.RtGuideParams()
        p.kn, p.kz, p.ka = kn, kz, ka
        if reserved is not None:
            p.reserved[reserved] = 1
        return p

    assert _call_host(16, 16, gp()) == 0
    assert _call_host(16, 16, None) == 0   # NULL: the defaults
    for bad in (gp(kn=-1.0), gp(kz=float("nan")), gp(ka=float("inf")), gp(kn=float("-inf")), gp(ka=-0.25),
                gp(reserved=0), gp(reserved=4)):
        assert _call_host(16, 16, bad) == -1
    assert _call_host(16, 16, gp(), n_tiles_arg=3) == -1
    dp = _lib.RtDenoiseParams()
    dp.levels, dp.k = 3, 3.0
    dp.reserved[2] = 1
    assert _call_host(16, 16, gp(), dp=ctypes.byref(dp)) == -1


def test_struct_layout():
    P = _lib.RtGuideParams
    assert (P.kn.offset, P.kz.offset, P.ka.offset, P.reserved.offset) == (0, 4, 8, 12)
    assert ctypes.sizeof(P) == 32


def test_albedo_step_is_not_crossed():
    """Flat luminance with iid noise of variance 3 * 0.05^2 = 0.0075 in y, stated to the filter as
    V_0 = 2^-7 (M2.w = 2^-6 at n = 2), and an albedo step of 1.8 in |dA| down the middle.  With ka = 1
    every tap across the step has ga = g_max(0, 1 - 1.8) = 0 and every tap inside a half has g = 1, so
    a half's pixels equal the filter run on that half alone (one level: the next level's 3x3 variance
    average, which is not guided, would see across the step).  Unguided they do not."""
    W, H = 16, 16
    rng = np.random.default_rng(5)
    img = np.ones((H, W, 4), F)
    img[..., :3] = F(0.5) + (rng.standard_normal((H, W, 3)) * 0.05).astype(F)
    m2 = np.zeros((H, W, 4), F)
    m2[..., 3] = F(2.0 ** -6)
    nd = np.zeros((H, W, 4), F)
    nd[..., 2] = F(1.0)
    nd[..., 3] = F(4.0)
    alb = np.full((H, W, 3), 0.2, F)
    alb[:, W // 2:] = F(0.8)
    ai = rtamd.pack_albedo_id(alb, np.full((H, W), 2, np.uint32))
    guided = rtamd.denoise_guided_host(img, m2, 2, nd, ai, levels=1, k=3.0, guides=(0.0, 0.0, 1.0))
    plain = rtamd.denoise_host(img, m2, 2, levels=1, k=3.0)
    for sl in (slice(0, W // 2), slice(W // 2, W)):
        alone = rtamd.denoise_host(np.ascontiguousarray(img[:, sl]), np.ascontiguousarray(m2[:, sl]), 2, levels=1, k=3.0)
        assert same_bits(guided[:, sl], alone)
    beside = slice(W // 2 - 2, W // 2 + 2)
    assert not same_bits(plain[:, beside], guided[:, beside])
    # the noise is smoothed all the same: the guided result is closer to the flat 0.5 than the input
    assert np.abs(guided[..., :3] - 0.5).mean() < 0.7 * np.abs(img[..., :3] - 0.5).mean()


@pytest.mark.parametrize("case", features_ref.CASES, ids=lambda c: f"scene{c[0]}_{c[1]}x{c[2]}")
def test_reference_tie_caps(case):
    """The share of tied pixels (two candidate prims at the same t, to the bit) stays under the caps:
    a comparison cannot hide behind ties."""
    scene_id, W, H = case
    ref = features_ref.reference(scene_id, W, H)
    tied = int(ref.tied.sum())
    cap = features_ref.TIE_CAPS[scene_id]
    assert tied <= cap * W * H, f"scene {scene_id} {W}x{H}: {tied} tied pixels of {W * H}"


def test_render_kernels_compile_to_what_they_did():
    """`make -C raytracing-book_amd resources` of the parent commit and of this one: every kernel of
    rt_kernel.hip and rt_moments.hip (the render_persistent and fold instances among them) reads the
    same -- the first-hit pass is a translation unit of its own and adds nothing to their headers."""
    import os
    prof = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
    parent = open(os.path.join(prof, "features_resources_parent.txt")).read().splitlines()
    this = open(os.path.join(prof, "features_resources_this.txt")).read().splitlines()
    assert sum("Function Name" in ln and "render_persistent" in ln for ln in this) > 0
    assert sum("Function Name" in ln and "fold" in ln for ln in this) > 0
    assert parent == this

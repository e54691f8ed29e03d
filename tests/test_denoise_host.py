"""CPU tests of the variance-guided a-trous preview filter (rt.h rt_denoise ... rt_denoise_host): the
host reference against a numpy float32 restatement of rt.h's definition, bit for bit; the exact
properties (identity at zero variance, constants kept); the smoothing it is there for; argument
checks without a device; and the render kernels' resource usage, which the filter must not change
(it lives in its own translation units).  tests/test_gpu_denoise.py reuses the restatement and the
input generator.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import rtamd
from rtamd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILES = os.path.join(REPO, "profiles")
F = np.float32

SHAPES = [(5, 3), (13, 9), (37, 23), (64, 40)]   # (W, H): below the stencil, odd, no multiple of 8, several tiles
LEVELS = [1, 2, 3, 4, 5]                          # step 16 exceeds every one of them
KS = [0.75, 3.0, 4.5]


def n_tiles(W, H):
    return ((W + 7) // 8) * ((H + 7) // 8)


def make_inputs(W, H, seed, bad=True, counts="mixed"):
    """A seeded random image, M2 and per-tile counts.  The image has a soft edge so that taps are
    both accepted and rejected; with `bad`, NaN and inf in the image and NaN and negative values in
    M2 (a negative finite M2.w is a good pixel of variance 0)."""
    rng = np.random.default_rng(seed)
    img = rng.random((H, W, 4), dtype=F) * F(0.5)
    img[:, W // 2:, :3] += F(0.75)
    img[..., 3] = F(1.0)
    m2 = (rng.random((H, W, 4), dtype=F) * F(2.0)).astype(F)
    m2[rng.random((H, W)) < 0.2] *= F(40.0)
    if bad:
        k = max(1, W * H // 24)
        for what in range(4):
            ys, xs = rng.integers(0, H, k), rng.integers(0, W, k)
            if what == 0:
                img[ys, xs, rng.integers(0, 3, k)] = np.nan
            elif what == 1:
                img[ys, xs, rng.integers(0, 3, k)] = np.inf
            elif what == 2:
                m2[ys, xs, 3] = np.nan
            else:
                m2[ys, xs, 3] = F(-0.5)
        m2[0, 0, 3] = -np.inf
    nt = n_tiles(W, H)
    tf = rng.integers(2, 41, nt).astype(np.int32) if counts == "mixed" else np.full(nt, counts, np.int32)
    return img, m2, tf


def shifted(a, dy, dx, fill):
    """q(p) = a[p + (dy, dx)] where that lies in the array, `fill` elsewhere."""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    y0, y1 = max(0, -dy), min(H, H - dy)
    x0, x1 = max(0, -dx), min(W, W - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def gmax0(t):
    """rt_glsl.h g_max(0, t) = 0 < t ? t : 0."""
    return np.where(F(0.0) < t, t, F(0.0)).astype(F)


def denoise_numpy(image, m2, tile_frames, levels=3, k=3.0):
    """rt.h's definition in numpy float32, every operation in the stated order."""
    image = np.asarray(image, F)
    H, W = image.shape[:2]
    tx, ty = (W + 7) // 8, (H + 7) // 8
    n = np.repeat(np.repeat(np.asarray(tile_frames, np.int32).reshape(ty, tx), 8, 0), 8, 1)[:H, :W]
    k = F(k)
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
    assert out.dtype == F
    return out


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32))


def where_differs(a, b):
    d = (np.ascontiguousarray(a, F).view(np.uint32) != np.ascontiguousarray(b, F).view(np.uint32)).any(axis=-1)
    ys, xs = np.nonzero(d)
    return f"{int(d.sum())} pixels differ" + (f", first at y={ys[0]} x={xs[0]}: {a[ys[0], xs[0]]} vs {b[ys[0], xs[0]]}"
                                              if len(ys) else "")


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_matches_numpy_bit_for_bit(shape, levels, k):
    W, H = shape
    img, m2, tf = make_inputs(W, H, seed=1000 * W + 10 * H + levels)
    got = rtamd.denoise_host(img, m2, tf, levels=levels, k=k)
    ref = denoise_numpy(img, m2, tf, levels=levels, k=k)
    assert same_bits(got, ref), where_differs(got, ref)
    # the bad pixels came through with their input bits, and something was filtered
    bad = ~(np.isfinite((img[..., 0] + img[..., 1]) + img[..., 2]) & np.isfinite(m2[..., 3]))
    assert bad.any() and same_bits(got[bad][:, :3], img[bad][:, :3])
    assert not same_bits(got[~bad][:, :3], img[~bad][:, :3])


def test_defaults_are_levels_3_k_3():
    img, m2, tf = make_inputs(37, 23, seed=5)
    assert same_bits(rtamd.denoise_host(img, m2, tf), denoise_numpy(img, m2, tf, levels=3, k=3.0))
    assert same_bits(rtamd.denoise_host(img, m2, tf), rtamd.denoise_host(img, m2, tf, levels=3, k=3.0))
    assert rtamd.render.DENOISE_DEFAULTS == (3, 3.0)


@pytest.mark.parametrize("levels", [1, 3, 5])
def test_zero_variance_is_the_identity(levels):
    img, _, tf = make_inputs(37, 23, seed=7, bad=False)
    img[..., 3] = F(0.25)   # w is not passed through: the output's is 1
    out = rtamd.denoise_host(img, np.zeros_like(img), tf, levels=levels)
    assert same_bits(out[..., :3], img[..., :3])
    assert np.all(out[..., 3] == 1.0)


@pytest.mark.parametrize("levels", [1, 3, 5])
def test_constant_image_is_kept(levels):
    _, m2, tf = make_inputs(37, 23, seed=9, bad=False)
    m2[3, 4, 3] = F(3.0e38)   # a variance whose sums overflow still accepts, and moves nothing
    img = np.empty((23, 37, 4), F)
    img[...] = np.array([0.3, 1.7, 0.011, 1.0], F)
    out = rtamd.denoise_host(img, m2, tf, levels=levels, k=0.5)
    assert same_bits(out, img)


def noisy_flat(W, H, n, sigma, seed):
    """A flat signal plus iid Gaussian noise of standard deviation sigma per channel, as the mean of n
    frames would hold it, and the M2 that states the noise's true variance: var(y) = 3 sigma^2 is
    M2.w / (n (n - 1))."""
    rng = np.random.default_rng(seed)
    signal = np.empty((H, W, 4), F)
    signal[...] = np.array([0.5, 0.4, 0.3, 1.0], F)
    img = signal.copy()
    img[..., :3] += rng.normal(0.0, sigma, (H, W, 3)).astype(F)
    m2 = np.zeros((H, W, 4), F)
    m2[..., :3] = F(sigma * sigma * n * (n - 1))
    m2[..., 3] = F(3.0 * sigma * sigma * n * (n - 1))
    return signal, img, m2


def rmse(a, b):
    """Over the pixels where both are finite."""
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float(np.sqrt(np.mean(d[np.isfinite(d).all(axis=-1)] ** 2)))


def test_smoothing_of_a_noisy_flat_signal():
    """The bound is the issue's 0.5.  Measured on the host path with the defaults: 64x64, 16 frames,
    sigma 0.05: ratio 0.161; so 0.5 holds with margin and stays."""
    signal, img, m2 = noisy_flat(64, 64, 16, 0.05, seed=11)
    out = rtamd.denoise_host(img, m2, 16)
    ratio = rmse(out, signal) / rmse(img, signal)
    print(f"smoothing: RMSE after / before = {ratio:.4f}")
    assert ratio <= 0.5


# --- arguments, layout, NULL contexts -------------------------------------------------------------

def params(levels=3, k=3.0, reserved=None):
    p = _lib.RtDenoiseParams()
    p.levels, p.k = levels, k
    for i, v in enumerate(reserved or ()):
        p.reserved[i] = v
    return p


def test_denoise_host_rejects_bad_arguments():
    L = rtamd.amd()
    W, H = 13, 9
    img, m2, tf = make_inputs(W, H, seed=3)
    out = np.empty_like(img)
    fp = lambda a: a.ctypes.data_as(_lib.c_float_p)
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    nt = n_tiles(W, H)
    ok = lambda **kw: L.rt_denoise_host(kw.get("image", fp(img)), kw.get("m2", fp(m2)), kw.get("tf", ip(tf)),
                                        kw.get("nt", nt), kw.get("w", W), kw.get("h", H), kw.get("p", None),
                                        kw.get("out", fp(out)))
    assert ok() == 0
    assert ok(p=ctypes.byref(params())) == 0
    for name in ("image", "m2", "tf", "out"):
        assert ok(**{name: None}) == -1, name
    for w, h in ((0, H), (W, 0), (-1, H), (W, -4), (65537, H)):
        assert ok(w=w, h=h) == -1, (w, h)
    for bad_nt in (nt - 1, nt + 1, 0, -1):
        assert ok(nt=bad_nt) == -1
    assert ok(w=W + 8) == -1   # another tile column: n_tiles no longer matches
    for count in (1, 0, -5):
        t2 = tf.copy()
        t2[-1] = count
        assert ok(tf=ip(t2)) == -1, count
    for levels in (0, -1, 6, 100):
        assert ok(p=ctypes.byref(params(levels=levels))) == -1, levels
    for k in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert ok(p=ctypes.byref(params(k=k))) == -1, k
    for slot in range(6):
        r = [0] * 6
        r[slot] = 1
        assert ok(p=ctypes.byref(params(reserved=r))) == -1, slot
    for levels in (1, 5):
        assert ok(p=ctypes.byref(params(levels=levels, k=1e-3))) == 0
    with pytest.raises(rtamd.RTError):
        rtamd.denoise_host(img, m2, tf, levels=6)
    with pytest.raises(rtamd.RTError):
        rtamd.denoise_host(img, m2, 1)


def test_params_struct_has_the_header_layout():
    P = _lib.RtDenoiseParams
    assert ctypes.sizeof(P) == 32
    assert (P.levels.offset, P.k.offset, P.reserved.offset) == (0, 4, 8)
    assert P.reserved.size == 24


def test_null_context_calls_are_rejected():
    L = rtamd.amd()
    buf = (ctypes.c_float * 4)()
    assert L.rt_denoise(None, None) == -1
    assert L.rt_denoise(None, ctypes.byref(params())) == -1
    assert L.rt_read_denoised(None, buf) == -1


# --- the render kernels compile exactly as before ------------------------------------------------

def parse_resources(text):
    """`make resources` output -> {kernel: {field: value}} (the -Rpass-analysis remarks)."""
    out, cur = {}, None
    for ln in text.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: .*?\s{2,}([A-Za-z][\w \[\]/-]*?): (\S+)", ln)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return out


FIELDS = ("VGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")


def test_recorded_render_kernel_resources_are_identical():
    """profiles/denoise_resources_{parent,this}.txt: `make -C raytracing-book_amd resources` on the
    parent commit and on this one; every render_persistent instance, every field."""
    a, b = (parse_resources(open(os.path.join(PROFILES, f"denoise_resources_{w}.txt")).read()) for w in ("parent", "this"))
    a, b = ({k: v for k, v in r.items() if "render_persistent" in k} for r in (a, b))
    assert len(a) >= 10 and sorted(a) == sorted(b)
    for kname in a:
        for f in FIELDS:
            assert f in a[kname], (kname, f)
            assert a[kname][f] == b[kname][f], (kname, f, a[kname][f], b[kname][f])

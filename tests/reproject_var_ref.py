"""NumPy float32 restatement of the variance carried through reprojection (rt.h rt_set_history_variance) and of
rt_denoise_reprojected's level 0, written from rt.h alone, every operation in float32 in the header's order, so
that rt_history_variance_host, rt_reproject_variance_host and rt_denoise_reprojected_host (and through them the
kernels) can be compared bit for bit.  The result word and the taps' acceptance are tests/reproject_ref.py's.

The levels after level 0 are rt_denoise's, which tests/test_denoise_host.py restates; `as_moments` turns a
level 0 into inputs of rt_denoise_host / rt_denoise_guided_host that give exactly that level 0 there, so a
level 0 stated here is compared through the filtered image.
"""
import numpy as np

import reproject_ref as R

F = np.float32
# which rule gave a result pixel's s2
OWN, HISTORY, BLEND = range(3)
# level-0 classes
BAD, KNOWN, SPATIAL = range(3)


def history_s2(image, m2, tile_frames):
    """history_s2 of rt.h per pixel -> [H, W] float32."""
    img = np.ascontiguousarray(image, F)
    H, W = img.shape[:2]
    m2w = np.ascontiguousarray(m2, F)[..., 3]
    n = np.where(np.isfinite(img[..., :3]).all(axis=-1), R.tile_counts(tile_frames, W, H).astype(F), F(0))
    with np.errstate(all="ignore"):
        v = m2w / (n - F(1))
        known = (n >= F(2)) & np.isfinite(m2w)
        return np.where(known, np.where(F(0) < v, v, F(0)), F(-1)).astype(F)


def reproject(hist, hnd, hai, hs2, hcam, image, m2, tile_frames, nd, ai, cam, **prm):
    """-> (rgbn [H, W, 4], s2 [H, W], info): info is reproject_ref's plus `rule` (OWN / HISTORY / BLEND),
    `s2_c`, `s2_hist` and `tap_unknown` (some accepted tap's history s2 was unknown)."""
    out, info = R.reproject(hist, hnd, hai, hcam, image, tile_frames, nd, ai, cam, **prm)
    hs2 = np.ascontiguousarray(hs2, F)
    H, W = hs2.shape
    s2_c = history_s2(image, m2, tile_frames)
    with np.errstate(all="ignore"):
        fx, fy = info["fx"], info["fy"]
        ax, ay = fx - np.floor(fx), fy - np.floor(fy)
        ss, sws = np.zeros((H, W), F), np.zeros((H, W), F)
        tap_unknown = np.zeros((H, W), bool)
        for tp, (j, i) in zip(info["taps"], ((0, 0), (0, 1), (1, 0), (1, 1))):
            s = hs2[np.clip(tp["qy"], 0, H - 1), np.clip(tp["qx"], 0, W - 1)]
            u = (ax if i else F(1) - ax) * (ay if j else F(1) - ay)
            kn = tp["use"] & (s >= F(0))
            tap_unknown |= tp["use"] & ~(s >= F(0))
            ss = np.where(kn, ss + u * s, ss)
            sws = np.where(kn, sws + u, sws)
        s2_hist = np.where(sws > F(0), ss / sws, F(-1)).astype(F)
        st = info["status"]
        n_c, n_hist = info["n_c"], info["n_hist"]
        alpha = n_hist / (n_c + n_hist)
        blend = np.where(~(s2_c >= F(0)), s2_hist, np.where(~(s2_hist >= F(0)), s2_c, s2_c + alpha * (s2_hist - s2_c)))
        s2 = np.where(st == R.HISTORY_ONLY, s2_hist, np.where(st == R.BLENDED, blend, s2_c)).astype(F)
    rule = np.where(st == R.HISTORY_ONLY, HISTORY, np.where(st == R.BLENDED, BLEND, OWN))
    info = dict(info, rule=rule, s2_c=s2_c, s2_hist=s2_hist, tap_unknown=tap_unknown)
    return out, s2, info


def lum(c):
    return (c[..., 0] + c[..., 1]) + c[..., 2]


def shifted(a, dy, dx):
    """a[p + (dy, dx)], read at the clamped position."""
    H, W = a.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    return a[np.clip(ys + dy, 0, H - 1), np.clip(xs + dx, 0, W - 1)]


def level0(rgbn, s2, ai):
    """Level 0 of rt_denoise_reprojected -> (V_0 [H, W] float32 with -1 at bad pixels, class [H, W])."""
    Rv = np.ascontiguousarray(rgbn, F)
    s2 = np.ascontiguousarray(s2, F)
    H, W = s2.shape
    ids = R.id_word(ai)
    ys, xs = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        y, n = lum(Rv), Rv[..., 3]
        bad = ~(np.isfinite(y) & (n > F(0)))
        known = (s2 >= F(0)) & np.isfinite(s2)
        taps = []
        cnt, sy = np.zeros((H, W), F), np.zeros((H, W), F)
        for dy in (-2, -1, 0, 1, 2):
            for dx in (-2, -1, 0, 1, 2):
                inside = (ys + dy >= 0) & (ys + dy < H) & (xs + dx >= 0) & (xs + dx < W)
                use = inside & ~shifted(bad, dy, dx) & (shifted(ids, dy, dx) == ids)
                yq = shifted(y, dy, dx)
                cnt = np.where(use, cnt + F(1), cnt)
                sy = np.where(use, sy + yq, sy)
                taps.append((use, yq))
        m = sy / cnt
        sd = np.zeros((H, W), F)
        for use, yq in taps:
            e = yq - m
            sd = np.where(use, sd + e * e, sd)
        spatial = np.where(cnt < F(2), F(0), (sd / (cnt - F(1))) / n)
        V = np.where(bad, F(-1), np.where(known, s2 / n, spatial)).astype(F)
    cls = np.where(bad, BAD, np.where(known, KNOWN, SPATIAL))
    return V, cls


def as_moments(rgbn, V0):
    """(image, m2, tile_frames) whose rt_denoise level 0 is exactly (rgb, V0): n = 2 in every tile and
    M2.w = 2 V0, so g_max(0, M2.w / (2 * 1)) is V0 to the bit (V0 >= 0, finite and not within a factor 2 of
    overflow); a bad pixel (V0 < 0) gets M2.w = NaN."""
    image = np.ascontiguousarray(rgbn, F).copy()
    m2 = np.zeros_like(image)
    with np.errstate(all="ignore"):
        m2[..., 3] = np.where(V0 < F(0), F(np.nan), V0 * F(2))
    assert np.isfinite(m2[..., 3][V0 >= 0]).all() and np.array_equal((m2[..., 3] / F(2))[V0 >= 0], V0[V0 >= 0])
    return image, m2, 2

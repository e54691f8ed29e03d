"""NumPy float32 restatement of the misses reprojected by direction (rt.h rt_set_reproject_misses), written from
rt.h alone: steps 2m and 4m for a guide-good miss pixel, every operation in float32 in the header's order, so that
rt_reproject_misses_host (and through it the two kernels) can be compared bit for bit.  A hit pixel's word and s2
are tests/reproject_ref.py's and tests/reproject_var_ref.py's, taken from there unchanged.
"""
import numpy as np

import reproject_ref as R
import reproject_var_ref as RV

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def miss_pixels(nd, ai):
    """The pixels the rule applies to: guide-good and a miss."""
    nd, ai = np.ascontiguousarray(nd, F), np.ascontiguousarray(ai, F)
    return R.guide_good(nd, ai) & (R.id_word(ai) == R.MISS)


def _miss_path(hist, hnd, hai, hs2, hcam, image, m2, tile_frames, nd, ai, cam, max_history):
    """Steps 2m, 3, 4m, 5 and 6 at every pixel (the caller keeps the guide-good misses)."""
    H, W = image.shape[:2]
    M = R.matrix(hcam)
    o = R.cam_parts(cam)[0]
    ys, xs = np.mgrid[0:H, 0:W]
    var = hs2 is not None
    with np.errstate(all="ignore"):
        C = image[..., :3]
        n_c = np.where(np.isfinite(C).all(axis=-1), R.tile_counts(tile_frames, W, H).astype(F), F(0))
        live = miss_pixels(nd, ai)
        base = R.pixel_base(cam, xs.astype(F), ys.astype(F))                           # 2m
        w = [base[c] - o[c] for c in range(3)]
        a, b, c_ = [(M[r, 0] * w[0] + M[r, 1] * w[1]) + M[r, 2] * w[2] for r in range(3)]   # 3
        front = live & (c_ > F(0))
        fx, fy = a / c_, b / c_
        inside = front & (fx > F(-1)) & (fx < F(W)) & (fy > F(-1)) & (fy < F(H))
        x0, y0 = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0, fy - y0
        ix = np.where(inside, x0, F(0)).astype(np.int64)
        iy = np.where(inside, y0, F(0)).astype(np.int64)
        sw, sn = np.zeros((H, W), F), np.zeros((H, W), F)
        sc = [np.zeros((H, W), F) for _ in range(3)]
        ss, sws = np.zeros((H, W), F), np.zeros((H, W), F)
        hmiss = miss_pixels(hnd, hai)
        ab, hab = bits(ai), bits(hai)
        taps = []
        for j in (0, 1):                                                               # 4m
            for i in (0, 1):
                qx, qy = ix + i, iy + j
                q_in = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                hq = hist[cy, cx]
                u = (ax if i else F(1) - ax) * (ay if j else F(1) - ay)
                held = hq[..., 3] > F(0)
                sky = hmiss[cy, cx]
                same = (hab[cy, cx, :3] == ab[..., :3]).all(axis=-1)
                use = inside & q_in & held & sky & same
                sw = np.where(use, sw + u, sw)
                for c in range(3):
                    sc[c] = np.where(use, sc[c] + u * hq[..., c], sc[c])
                sn = np.where(use, sn + u * hq[..., 3], sn)
                if var:
                    s = hs2[cy, cx]
                    kn = use & (s >= F(0))
                    ss = np.where(kn, ss + u * s, ss)
                    sws = np.where(kn, sws + u, sws)
                taps.append(dict(considered=inside, q_in=q_in, held=held, sky=sky, same=same, use=use))
        got = inside & (sw > F(0))                                                     # 5
        Hc = [sc[c] / sw for c in range(3)]
        n_hist = np.where(max_history < sn / sw, max_history, sn / sw)
        n_out = n_c + n_hist                                                           # 6
        alpha = n_hist / n_out
        only = got & (n_c == F(0))
        out = np.empty((H, W, 4), F)
        for c in range(3):
            blend = C[..., c] + alpha * (Hc[c] - C[..., c])
            out[..., c] = np.where(got, np.where(only, Hc[c], blend), C[..., c])
        out[..., 3] = np.where(got, np.where(only, n_hist, n_out), n_c)
        s2 = None
        if var:
            s2_c = RV.history_s2(image, m2, tile_frames)
            s2_hist = np.where(sws > F(0), ss / sws, F(-1)).astype(F)
            mix = np.where(~(s2_c >= F(0)), s2_hist, np.where(~(s2_hist >= F(0)), s2_c, s2_c + alpha * (s2_hist - s2_c)))
            s2 = np.where(got, np.where(only, s2_hist, mix), s2_c).astype(F)
    status = np.full((H, W), R.NOT_REPROJECTED, np.int32)
    status[live & ~front] = R.BEHIND
    status[front & ~inside] = R.OUTSIDE
    status[inside & ~got] = R.NO_TAP
    status[got & only] = R.HISTORY_ONLY
    status[got & ~only] = R.BLENDED
    return out, s2, dict(live=live, status=status, taps=taps, n_c=n_c)


def reproject(hist, hnd, hai, hcam, image, tile_frames, nd, ai, cam, hs2=None, m2=None, cos_min=R.DEFAULTS[0],
              kz=R.DEFAULTS[1], max_history=R.DEFAULTS[2]):
    """rt_reproject_misses_host -> (rgbn [H, W, 4], s2 [H, W] or None without hs2 / m2, info).  info: `miss` the
    pixels the rule applied to, `status` (reproject_ref's codes) and `taps` there, `hit_info` reproject_ref's."""
    assert (hs2 is None) == (m2 is None)
    hist, hnd, hai, image, nd, ai = (np.ascontiguousarray(a, F) for a in (hist, hnd, hai, image, nd, ai))
    prm = dict(cos_min=cos_min, kz=kz, max_history=max_history)
    if hs2 is None:
        out, hit_info = R.reproject(hist, hnd, hai, hcam, image, tile_frames, nd, ai, cam, **prm)
        s2 = None
    else:
        hs2, m2 = np.ascontiguousarray(hs2, F), np.ascontiguousarray(m2, F)
        out, s2, hit_info = RV.reproject(hist, hnd, hai, hs2, hcam, image, m2, tile_frames, nd, ai, cam, **prm)
    m_out, m_s2, m = _miss_path(hist, hnd, hai, hs2, hcam, image, m2, tile_frames, nd, ai, cam, F(max_history))
    sel = m["live"]
    out = np.where(sel[..., None], m_out, out).astype(F)
    if s2 is not None:
        s2 = np.where(sel, m_s2, s2).astype(F)
    return out, s2, dict(miss=sel, status=m["status"], taps=m["taps"], n_c=m["n_c"], hit_info=hit_info)

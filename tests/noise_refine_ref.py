"""A NumPy restatement of the noise records and the noise-target selection, written from include/rt/rt.h
(rt_noise_tiles / rt_refine_noise_select) and from nothing else: the records in float32, every tile's 64 lanes at
once, the xor butterfly as index permutations, each step one float32 operation in the order the header writes it;
the selection and its stats in float64, tiles in index order.
"""
import math

import numpy as np

from refine_ref import FLT_MAX, lanes

F = np.float32
NOISE_DTYPE = np.dtype([("v_sum", "<f4"), ("y_sum", "<f4"), ("known_px", "<u2"), ("thin_px", "<u2"), ("bad_px", "<u2"),
                        ("pixels", "<u2")])


def finite(a):
    return np.abs(a) <= FLT_MAX


def tile_noise(rgbn, s2, min_count):
    """rt_tile_noise_host's records for a result [H, W, 4] float32 and its s2 [H, W]."""
    R = np.ascontiguousarray(rgbn, F)
    H, W = R.shape[:2]
    r, g, b, n = (lanes(R[..., c], W, H, F(0)) for c in range(4))
    s = lanes(np.ascontiguousarray(s2, F), W, H, F(0))
    inside = lanes(np.ones((H, W), bool), W, H, False)
    mc = F(min_count)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        y = ((r + g).astype(F) + b).astype(F)
        good = inside & finite(y) & (n > F(0)) & finite(n)
        known = good & (s >= F(0)) & finite(s)
        thin = good & (~known | ~(n >= mc))
        v = np.where(known, (s / np.where(known, n, F(1))).astype(F), F(0)).astype(F)
        yv = np.where(good, y, F(0)).astype(F)
        lane = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            v = (v + v[:, lane ^ off]).astype(F)
            yv = (yv + yv[:, lane ^ off]).astype(F)
    out = np.zeros(n.shape[0], NOISE_DTYPE)
    out["v_sum"] = v[:, 0]
    out["y_sum"] = yv[:, 0]
    out["known_px"] = known.sum(axis=1)
    out["thin_px"] = thin.sum(axis=1)
    out["bad_px"] = (inside & ~good).sum(axis=1)
    out["pixels"] = inside.sum(axis=1)
    return out


def noise_select(tiles, target, active=None):
    """rt_refine_noise_select: (active uint8 per tile, the stats as a dict)."""
    t = np.asarray(tiles, NOISE_DTYPE)
    sum_v = sum_y = 0.0
    for rec in t:                                   # in index order, in double
        sum_v += float(rec["v_sum"])
        sum_y += float(rec["y_sum"])
    known, thin = int(t["known_px"].astype(np.int64).sum()), int(t["thin_px"].astype(np.int64).sum())
    bad, pixels = int(t["bad_px"].astype(np.int64).sum()), int(t["pixels"].astype(np.int64).sum())
    good = pixels - bad
    ybar = sum_y / good if good > 0 else 0.0
    lim = float(F(target)) * ybar
    out = np.zeros(t.size, np.uint8)
    for i, rec in enumerate(t):
        G, K = int(rec["pixels"]) - int(rec["bad_px"]), int(rec["known_px"])
        on = (active is None or bool(active[i])) and G > 0
        if on and int(rec["thin_px"]) < 1:
            with np.errstate(over="ignore", invalid="ignore"):
                on = K > 0 and bool(np.float64(rec["v_sum"]) / np.float64(K) > np.float64(lim) * np.float64(lim))
        out[i] = 1 if on else 0
    if known == 0:
        noise = math.inf
    elif sum_v == 0.0:
        noise = 0.0
    elif ybar == 0.0:
        noise = math.inf
    else:
        with np.errstate(over="ignore", invalid="ignore"):
            noise = float(np.sqrt(np.float64(sum_v) / np.float64(known)) / np.float64(ybar))
    return out, dict(sum_v=sum_v, sum_y=sum_y, known=known, thin=thin, bad=bad, pixels=pixels, rounds=0, converged=0,
                     noise=noise)

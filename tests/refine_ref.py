"""A NumPy float32 restatement of the reach records and the tile selection, written from include/rt/rt.h
(rt_reach_tiles / rt_refine_select) and from nothing else: every tile's 64 lanes at once, the xor butterfly
as index permutations, each step one float32 operation in the order the header writes it.
"""
import numpy as np

F = np.float32
FLT_MAX = np.finfo(F).max
REACH_DTYPE = np.dtype([("n_min", "<f4"), ("n_sum", "<f4"), ("short_px", "<u4"), ("pixels", "<u4")])


def tiles_of(W, H):
    return (W + 7) // 8, (H + 7) // 8


def lanes(a, W, H, fill):
    """[H, W] -> [tiles, 64]: tiles row-major, lane ty * 8 + tx; lanes outside the image hold `fill`."""
    tx, ty = tiles_of(W, H)
    p = np.full((ty * 8, tx * 8), fill, a.dtype)
    p[:H, :W] = a
    return p.reshape(ty, 8, tx, 8).transpose(0, 2, 1, 3).reshape(ty * tx, 64)


def g_min(a, b):
    return np.where(b < a, b, a)


def tile_reach(rgbn, min_count):
    """rt_tile_reach_host's records for a result [H, W, 4] float32."""
    r = np.ascontiguousarray(rgbn, F)
    H, W = r.shape[:2]
    n = lanes(r[..., 3], W, H, F(0))
    inside = lanes(np.ones((H, W), bool), W, H, False)
    mc = F(min_count)
    with np.errstate(invalid="ignore"):
        good = inside & (n > F(0)) & (np.abs(n) <= FLT_MAX)
        short = inside & ~(n >= mc)
    v_min = np.where(good, n, F(np.inf)).astype(F)
    v_sum = np.where(good, n, F(0)).astype(F)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        with np.errstate(over="ignore"):
            v_sum = (v_sum + v_sum[:, lane ^ off]).astype(F)
        v_min = g_min(v_min, v_min[:, lane ^ off]).astype(F)
    out = np.zeros(n.shape[0], REACH_DTYPE)
    out["n_min"] = v_min[:, 0]
    out["n_sum"] = v_sum[:, 0]
    out["short_px"] = short.sum(axis=1)
    out["pixels"] = inside.sum(axis=1)
    return out


def refine_select(short_px, min_pixels=1, max_tiles=0):
    """rt_refine_select: (active uint8 per tile, the threshold t it ended at)."""
    s = np.asarray(short_px, np.int64)
    t = min_pixels
    if max_tiles > 0:
        while int((s >= t).sum()) > max_tiles:
            t += 1
    assert min_pixels <= t <= 65
    return (s >= t).astype(np.uint8), t

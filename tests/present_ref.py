"""The presented frame (rt.h rt_present) restated in NumPy float32, operation by operation, and the inputs the
host and the device tests share.  The gamma table is not recomputed here: it is read off rts_tonemap_rgb8,
the display path the library had before the frame existed, applied to the ramp b / 255.
"""
import functools

import numpy as np

import rtamd

F = np.float32
SOURCES = ("image", "denoised", "reprojected", "moved")
EXPOSURES = (1.0, 0.5, 3.0)


def code(f):
    """rt.h step 3: 0 if !(f > 0), 255 if f >= 1, else rint(f * 255) in float32, ties to even."""
    f = np.asarray(f, F)
    with np.errstate(invalid="ignore"):
        low, high = ~(f > 0), f >= 1
    mid = ~low & ~high
    v = np.rint(np.where(mid, f, F(0)) * F(255)).astype(np.int64)
    return np.where(low, 0, np.where(high, 255, v))


@functools.lru_cache(maxsize=None)
def table():
    """The 256-entry table, from rts_tonemap_rgb8 over the ramp: the ramp's codes are 0..255 in order, so the
    bytes that come back are the table's entries in order."""
    ramp = (np.arange(256) / 255.0).astype(F)
    assert np.array_equal(code(ramp), np.arange(256))
    img = np.zeros((1, 256, 4), F)
    img[0, :, 0] = ramp
    lut = rtamd.tonemap_rgb8(img)[0, :, 0].copy()
    assert lut.shape == (256,) and lut.dtype == np.uint8
    return lut


def tile_counts_per_pixel(tile_frames, w, h):
    tx, ty = (w + 7) // 8, (h + 7) // 8
    tf = np.asarray(tile_frames, np.int32).reshape(ty, tx)
    return np.repeat(np.repeat(tf, 8, axis=0), 8, axis=1)[:h, :w]


def present(source, image=None, denoised=None, reprojected=None, tile_frames=None, exposure=1.0):
    """-> (rgba8 [H, W, 4] uint8, float copy [H, W, 4] float32)."""
    if source == "moved":
        R, D = np.asarray(reprojected, F), np.asarray(denoised, F)
        h, w = R.shape[:2]
        n_t = tile_counts_per_pixel(tile_frames, w, h).astype(F)
        with np.errstate(invalid="ignore"):
            fresh = ~(R[..., 3] > n_t)
        c = np.where(fresh[..., None], D[..., :3], R[..., :3])
        wgt = np.where(fresh, F(1), F(0))
    else:
        src = np.asarray(dict(image=image, denoised=denoised, reprojected=reprojected)[source], F)
        c = src[..., :3]
        wgt = np.ones(src.shape[:2], F)
    with np.errstate(invalid="ignore", over="ignore"):
        e = (c * F(exposure)).astype(F)
    flt = np.concatenate([e, wgt[..., None]], axis=-1).astype(F)
    out = np.empty(flt.shape, np.uint8)
    out[..., :3] = table()[code(e)]
    out[..., 3] = 255
    return out, flt


# ---- the rounding image: 70 x 11, 2310 channel values ----------------------------------------------------

ROUNDING_W, ROUNDING_H = 70, 11


@functools.lru_cache(maxsize=None)
def rounding_values():
    """For every k in 0..254 float32((k + 0.5) / 255) and its two float32 neighbours (765 values), then NaN,
    +-inf, -0, a negative value, exactly 1 and a value above 1."""
    mid = ((np.arange(255) + 0.5) / 255.0).astype(F)
    trip = np.stack([np.nextafter(mid, F(0)), mid, np.nextafter(mid, F(2))], axis=1).astype(F)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, -0.25, 1.0, 1.5], F)
    return trip, special


def rounding_ties(trip):
    """Per k, which of the three values multiply (in float32) to exactly k + 0.5."""
    prod = (trip * F(255)).astype(F)
    return prod == (np.arange(255, dtype=F) + F(0.5))[:, None]


@functools.lru_cache(maxsize=None)
def rounding_image():
    trip, special = rounding_values()
    n = ROUNDING_W * ROUNDING_H * 3
    vals = np.concatenate([trip.ravel(), special])
    fill = np.random.default_rng(7).random(n - vals.size).astype(F)   # the rest: plain values in [0, 1)
    img = np.ones((ROUNDING_H, ROUNDING_W, 4), F)
    img[..., :3] = np.concatenate([vals, fill]).reshape(ROUNDING_H, ROUNDING_W, 3)
    img.setflags(write=False)
    return img


# ---- the synthetic RT_PRESENT_MOVED case: 13 x 9, partial tiles in both directions --------------------

MOVED_W, MOVED_H = 13, 9
MOVED_TILE_FRAMES = (2, 3, 1, 4)


@functools.lru_cache(maxsize=None)
def moved_case():
    """-> dict(reprojected, denoised, tile_frames): R.w below, equal to and above the tile's count, and NaN."""
    rng = np.random.default_rng(11)
    w, h = MOVED_W, MOVED_H
    R = rng.random((h, w, 4)).astype(F) * F(1.25) - F(0.125)
    D = rng.random((h, w, 4)).astype(F) * F(1.25) - F(0.125)
    D[..., 3] = 1.0
    tf = np.array(MOVED_TILE_FRAMES, np.int32)
    n_t = tile_counts_per_pixel(tf, w, h).astype(F)
    kind = (np.arange(w)[None, :] + np.arange(h)[:, None]) % 4
    R[..., 3] = np.select([kind == 0, kind == 1, kind == 2], [n_t - F(0.5), n_t, n_t + F(0.25)], F(np.nan))
    for a in (R, D):
        a.setflags(write=False)
    return dict(reprojected=R, denoised=D, tile_frames=tf, kind=kind)

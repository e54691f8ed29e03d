"""Tile masks, per-tile frame counts and the adaptive loop on the device (rt.h rt_set_active_tiles ...
rt_render_adaptive; render kernel unit_geo, fold_tiles_kernel in rt_moments.hip).

A sample's bits depend on its pixel, its frame and the scene alone, so everything here is compared
bit for bit with plain renders: a tile that holds n frames equals the plain n-frame render there.
Image 68x44: 9x6 tiles with a partial right column (4 wide), a partial bottom row (4 high) and a
partial corner.  Depth 5, seed 1.  Every case asserts the launch's active tile count
(rt_debug_last_launch), so none can pass on the unmasked path.
"""
import functools
import math

import numpy as np
import pytest

import rtamd
from helpers import bit_equal, gpu_image, mismatch_report

pytestmark = pytest.mark.gpu

W, H = 68, 44
TX, TY = 9, 6
NT = TX * TY
SEED = 1


def context(scene, spp, options=None, **kw):
    ctx = rtamd.RenderContext(options=options, **kw)
    ctx.upload_scene(scene)
    ctx.set_params(max_depth=5, spp=spp)
    ctx.resize(scene.width, scene.height)
    return ctx


def render(ctx, first, n):
    ctx.render(first, rtamd.frame_rand_factors(SEED, first - 1, n))


def pixels_of(tiles):
    """Per-tile flags [NT] -> per-pixel bool [H, W]."""
    t = np.asarray(tiles).astype(bool).reshape(TY, TX)
    return np.repeat(np.repeat(t, 8, axis=0), 8, axis=1)[:H, :W]


def pattern(base):
    """A distinct positive finite float per word: bits base + index (x * 0 is then +0, a zero image's)."""
    bits = np.uint32(base) + np.arange(H * W * 4, dtype=np.uint32)
    out = bits.view(np.float32).reshape(H, W, 4).copy()
    assert np.isfinite(out).all() and (out > 0).all()
    return out


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def seeded_mask(seed):
    """About 40% of the tiles, with tile 0, the last tile, a right-edge and a bottom-edge tile."""
    rng = np.random.default_rng(seed)
    m = (rng.random(NT) < 0.4).astype(np.uint8)
    for t in (0, NT - 1, 2 * TX + TX - 1, (TY - 1) * TX + 3):
        m[t] = 1
    m[1] = 0   # and tile 0's neighbours stay out
    m[TX] = 0
    assert 0.3 * NT <= m.sum() <= 0.55 * NT
    return m


@functools.lru_cache(maxsize=None)
def scene_of(sid):
    return rtamd.Scene(sid, W, H, seed=SEED)


@functools.lru_cache(maxsize=None)
def plain_image(sid, frames, sparse=True):
    return gpu_image(scene_of(sid), frames, spp=64, options=None if sparse else {"sparse_stage": 0})


@functools.lru_cache(maxsize=None)
def plain_series(sid):
    """Plain renders with the moments on, extended in batches of 8 to 40 frames: image, moments and
    tile sums at F = 8, 16, 24, 32, 40 (calls tests/test_gpu_moments.py pins)."""
    ctx = context(scene_of(sid), 64)
    ctx.set_moments(True)
    out = {}
    for F in (8, 16, 24, 32, 40):
        render(ctx, F - 7, 8)
        assert ctx.last_launch()["tiles_active"] == NT
        out[F] = dict(image=ctx.read_image(), m2=ctx.read_moments(), tiles=ctx.tile_sums())
    ctx.close()
    return out


@functools.lru_cache(maxsize=None)
def plain_state(sid, frames, sparse=True):
    """One plain launch of `frames` frames with the moments on: image and moments."""
    ctx = context(scene_of(sid), 64, options=None if sparse else {"sparse_stage": 0})
    ctx.set_moments(True)
    render(ctx, 1, frames)
    out = dict(image=ctx.read_image(), m2=ctx.read_moments())
    ctx.close()
    return out


# ---- 1. a masked render is exact ------------------------------------------------------------------

MASKED = [(6, False, True), (6, True, True), (0, False, True), (0, True, True), (8, False, True), (8, True, True),
          (6, False, False), (6, True, False)]


@pytest.mark.parametrize("sid,mom,sparse", MASKED)
def test_masked_render_is_exact(gpu, sid, mom, sparse):
    mask = seeded_mask(11 + sid)
    px = pixels_of(mask)
    ctx = context(scene_of(sid), 64, options=None if sparse else {"sparse_stage": 0})
    pat, pat2 = pattern(0x3F800000), pattern(0x40000000)
    if mom:
        ctx.set_moments(True)
    ctx.write_image(pat)
    if mom:
        ctx.write_moments(pat2, 5)   # every tile: 5 frames held, so the moments stay readable
    ctx.set_active_tiles(mask)
    render(ctx, 1, 12)
    ctx.sync()
    info = ctx.last_launch()
    img = ctx.read_image()
    counts = ctx.read_tile_frames()
    m2 = ctx.read_moments() if mom else None
    ctx.close()
    print(f"scene {sid} moments {mom} sparse {sparse}: launch {info}")
    assert info["tiles_active"] == int(mask.sum()) < NT
    assert info["staged"] == 1 and info["sparse"] == (1 if sparse else 0)
    if sid == 8:
        assert info["block"] == 1024 and info["box_interior"] == 1, info
    if sid == 0:
        assert info["sphere_pairs"] == 1, info
    ref = plain_image(sid, 12, sparse)
    assert bit_equal(img[px], ref[px]), mismatch_report(np.where(px[..., None], img, 0), np.where(px[..., None], ref, 0))
    assert same_bits(img[~px], pat[~px])   # every other word still holds its pattern
    assert list(counts) == [12 if a else (5 if mom else 0) for a in mask]
    if mom:
        ref2 = plain_state(sid, 12, sparse)["m2"]
        assert bit_equal(m2[px], ref2[px])
        assert same_bits(m2[~px], pat2[~px])


# ---- 2. corners of the mask -----------------------------------------------------------------------

def one_tile(t):
    m = np.zeros(NT, np.uint8)
    m[t] = 1
    return m


@pytest.mark.parametrize("name,mask", [("tile0", one_tile(0)), ("corner", one_tile(NT - 1)),
                                       ("all", np.ones(NT, np.uint8)), ("none", np.zeros(NT, np.uint8))])
@pytest.mark.parametrize("mom", [False, True])
def test_mask_corners(gpu, name, mask, mom):
    sid = 6
    px = pixels_of(mask)
    ctx = context(scene_of(sid), 64)
    if mom:
        ctx.set_moments(True)
    pat = pattern(0x3F800000)
    ctx.write_image(pat)
    ctx.set_active_tiles(mask)
    render(ctx, 1, 12)          # RT_OK with no active tile too
    ctx.sync()
    ns = ctx.last_render_ns()
    info = ctx.last_launch()
    img = ctx.read_image()
    counts = ctx.read_tile_frames()
    ctx.close()
    assert info["tiles_active"] == int(mask.sum())
    assert ns >= 0
    ref = plain_image(sid, 12)
    assert bit_equal(img[px], ref[px])
    assert same_bits(img[~px], pat[~px])
    assert list(counts) == [12 if a else 0 for a in mask]
    if name == "all":
        assert info["tiles_active"] == 54 and bit_equal(img, ref)
    if name == "none":
        assert same_bits(img, pat)
    if name == "corner":
        assert int(px.sum()) == 16


# ---- 3. extending under a mask ---------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["two_launches", "one_frame_moments", "one_frame_in_place"])
def test_extending(gpu, mode):
    sid = 6
    mom = mode != "one_frame_in_place"
    mask = seeded_mask(5)
    px = pixels_of(mask)
    ctx = context(scene_of(sid), 64)
    if mom:
        ctx.set_moments(True)
    if mode == "two_launches":
        render(ctx, 1, 8)
        assert ctx.last_launch()["tiles_active"] == NT
        ctx.set_active_tiles(mask)
        render(ctx, 9, 8)
        assert ctx.last_launch()["tiles_active"] == int(mask.sum())
    else:
        for f in range(1, 9):
            render(ctx, f, 1)
        ctx.set_active_tiles(mask)
        for f in range(9, 17):
            render(ctx, f, 1)
            info = ctx.last_launch()
            assert info["tiles_active"] == int(mask.sum()) and info["chunks"] == 1
            assert info["staged"] == (1 if mom else 0), info   # moments off: the one-chunk in-place path
    counts = ctx.read_tile_frames()
    img = ctx.read_image()
    assert list(counts) == [16 if a else 8 for a in mask]
    s = plain_series(sid)
    exp = np.where(px[..., None], s[16]["image"], s[8]["image"])
    assert bit_equal(img, exp), mismatch_report(img, exp)
    if mom:
        m2 = ctx.read_moments()
        exp2 = np.where(px[..., None], s[16]["m2"], s[8]["m2"])
        assert bit_equal(m2, exp2), mismatch_report(m2, exp2)
        tiles = ctx.tile_sums()
        want = s[8]["tiles"].copy()
        want[mask.astype(bool)] = s[16]["tiles"][mask.astype(bool)]
        assert tiles.tobytes() == want.tobytes()
        assert ctx.noise() == rtamd.noise_from_tile_sums_frames(tiles, counts)
        assert ctx.noise()["frames"] == 16
    ctx.close()


# ---- 4. the loop against its own replay --------------------------------------------------------------

def good_pixels(t):
    return float(int(t["pixels"]) - int(t["bad"]))


def select_ref(tiles, active, F, min_frames, target):
    """rt.h's rule in Python floats (doubles), tiles in index order."""
    sy = sp = 0.0
    for t in tiles:
        sy += float(t["y"])
        sp += good_pixels(t)
    ybar = sy / sp if sp > 0.0 else 0.0
    lim = float(np.float32(target)) * ybar
    out = []
    for t, a in zip(tiles, active):
        keep = bool(a)
        if keep and F >= min_frames:
            pt = good_pixels(t)
            if pt == 0.0:
                keep = False
            else:
                v = float(t["m2y"]) / (float(F) * (float(F) - 1.0)) / pt
                keep = not (v <= lim * lim)
        out.append(1 if keep else 0)
    return out


def noise_frames_ref(tiles, counts):
    var = sy = 0.0
    px = bad = 0
    for t, n in zip(tiles, counts):
        n = float(n)
        var += float(t["m2y"]) / (n * (n - 1.0))
        sy += float(t["y"])
        px += int(t["pixels"])
        bad += int(t["bad"])
    return math.sqrt(max(0.0, var) * float(px - bad)) / sy


def median_target(sid):
    """The median over tiles of sqrt(v_t) / ybar at F = 16 of the plain render, as the ABI's float."""
    tiles = plain_series(sid)[16]["tiles"]
    sy = sum(float(t["y"]) for t in tiles)
    sp = sum(good_pixels(t) for t in tiles)
    ybar = sy / sp
    rel = [math.sqrt(max(0.0, float(t["m2y"])) / (16.0 * 15.0) / good_pixels(t)) / ybar for t in tiles]
    return float(np.float32(np.median(rel)))


def replay_loop(sid, target, max_frames=40, batch=8, min_frames=8):
    s = plain_series(sid)
    active = [1] * NT
    counts = [0] * NT
    cur = s[8]["tiles"].copy()
    done = converged = 0
    while done < max_frames:
        done += batch
        for t in range(NT):
            if active[t]:
                counts[t] = done
                cur[t] = s[done]["tiles"][t]
        active = select_ref(cur, active, done, min_frames, target)
        if not any(active):
            converged = 1
            break
    return dict(counts=counts, done=done, converged=converged, tiles=cur, noise=noise_frames_ref(cur, counts))


@functools.lru_cache(maxsize=None)
def adaptive_run(sid, max_frames=40):
    ctx = context(scene_of(sid), 64)
    ctx.set_moments(True)
    done, last = ctx.render_adaptive(median_target(sid), max_frames, 8, min_frames=8, seed=SEED)
    out = dict(done=done, last=last, counts=ctx.read_tile_frames(), image=ctx.read_image(), m2=ctx.read_moments(),
               tiles=ctx.tile_sums(), launch=ctx.last_launch())
    ctx.close()
    return out


@pytest.mark.parametrize("sid", [6, 8])
def test_loop_against_its_replay(gpu, sid):
    target = median_target(sid)
    rep = replay_loop(sid, target)
    counts = np.array(rep["counts"])
    print(f"scene {sid}: target {target:.6g}, replay counts {sorted(set(rep['counts']))}, "
          f"{int((counts <= 16).sum())} tiles <= 16 frames, {int((counts > 16).sum())} above; done {rep['done']}")
    # the case is not vacuous: tiles on both sides of 16 frames
    assert (counts <= 16).sum() * 4 >= NT and (counts > 16).sum() * 4 >= NT
    run = adaptive_run(sid)
    assert list(run["counts"]) == rep["counts"]
    s = plain_series(sid)
    exp_img, exp_m2 = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
    for n in sorted(set(rep["counts"])):
        px = pixels_of(counts == n)
        exp_img[px], exp_m2[px] = s[n]["image"][px], s[n]["m2"][px]
    assert bit_equal(run["image"], exp_img), mismatch_report(run["image"], exp_img)
    assert bit_equal(run["m2"], exp_m2), mismatch_report(run["m2"], exp_m2)
    assert run["tiles"].tobytes() == rep["tiles"].tobytes()
    assert run["done"] == rep["done"] and run["last"]["converged"] == rep["converged"]
    assert run["last"]["noise"] == rep["noise"]
    assert run["last"]["frames"] == max(rep["counts"])
    assert run["launch"]["tiles_active"] < NT   # the last batch ran under a mask


# ---- 5. determinism ----------------------------------------------------------------------------------

def test_adaptive_is_deterministic(gpu):
    a = adaptive_run(6)
    adaptive_run.cache_clear()
    b = adaptive_run(6)
    assert a is not b
    assert list(a["counts"]) == list(b["counts"]) and a["done"] == b["done"] and a["last"] == b["last"]
    assert bit_equal(a["image"], b["image"]) and bit_equal(a["m2"], b["m2"])


# ---- 6. state rules ------------------------------------------------------------------------------------

def rt_err(code, fn):
    with pytest.raises(rtamd.RTError) as e:
        fn()
    assert e.value.code == code, e.value


def test_state_rules(gpu):
    mask = seeded_mask(3)
    two = rtamd.RenderContext(devices=(0, 0))
    two.resize(W, H)
    rt_err(-3, lambda: two.set_active_tiles(mask))            # RT_ERR_STATE: a multi-device context
    rt_err(-3, two.read_tile_frames)
    two.close()
    part = rtamd.RenderContext(rank=0, world=2, stripe_rows=8)
    part.resize(W, H)
    rt_err(-3, lambda: part.set_active_tiles(np.ones(NT, np.uint8)))   # ... a partition
    part.close()
    sid = 6
    target = median_target(sid)
    ctx = context(scene_of(sid), 64)
    rt_err(-1, lambda: ctx.set_active_tiles(mask[:-1]))       # RT_ERR_INVALID_ARG: n_tiles
    rt_err(-1, lambda: ctx.write_tile_frames(np.ones(NT + 1, np.int32)))
    rt_err(-3, lambda: ctx.render_adaptive(target, 16, 8, min_frames=8))   # the moments are off
    ctx.set_moments(True)
    ctx.set_active_tiles(mask)
    rt_err(-3, lambda: ctx.render_adaptive(target, 16, 8, min_frames=8))   # a caller mask is set
    rt_err(-1, lambda: ctx.render_adaptive(target, 16, 8, min_frames=1))
    ctx.resize(W, H)                                          # clears the mask
    render(ctx, 1, 4)
    assert ctx.last_launch()["tiles_active"] == NT
    assert list(ctx.read_tile_frames()) == [4] * NT
    # an adaptive run of at most 24 frames: tiles at the largest count and tiles that stopped before
    done, last = ctx.render_adaptive(target, 24, 8, min_frames=8, seed=SEED)
    counts = ctx.read_tile_frames()
    rep = replay_loop(sid, target, max_frames=24)
    assert done == rep["done"] and last["converged"] == rep["converged"] and list(counts) == rep["counts"]
    hi = int(counts.max())
    at_max = counts == hi
    assert hi > 16 and 0 < at_max.sum() < NT
    render(ctx, 1, 2)
    assert ctx.last_launch()["tiles_active"] == NT            # no mask is left set
    ctx.write_image(plain_series(sid)[8]["image"])            # (any image: the counts are what matters)
    ctx.write_moments(plain_series(sid)[8]["m2"], 8)
    ctx.write_tile_frames(counts)
    assert list(ctx.read_tile_frames()) == list(counts)
    rt_err(-3, lambda: ctx.render_adaptive(target, 8, 8, min_frames=8, first_frame=hi - 7))   # not the largest count + 1
    # resuming at the largest count + 1 samples only the tiles that hold it
    done, last = ctx.render_adaptive(target, 8, 8, min_frames=8, seed=SEED, first_frame=hi + 1)
    after = ctx.read_tile_frames()
    assert done == 8 and ctx.last_launch()["tiles_active"] == int(at_max.sum())
    assert list(after) == [hi + 8 if m else int(c) for m, c in zip(at_max, counts)]
    # a plain render that does not start at frame 1 extends only the tiles at its first frame - 1: the
    # others lose their count and the moments are invalid
    render(ctx, hi + 9, 2)
    left = ctx.read_tile_frames()
    assert list(left) == [hi + 10 if m else 0 for m in at_max]
    rt_err(-3, ctx.read_moments)
    rt_err(-3, ctx.noise)
    ctx.close()


# ---- 7. the mirrors: the executor and the command line run the same loop -----------------------------------

def test_executor_and_command_line(gpu):
    import os
    import re
    import subprocess
    sid, cap = 6, 64
    target = median_target(sid)
    ctx = context(scene_of(sid), cap)
    ctx.set_moments(True)
    done, last = ctx.render_adaptive(target, cap, 8, min_frames=8, seed=SEED)
    counts = ctx.read_tile_frames()
    ctx.close()
    assert len(set(counts)) > 1 and done == int(counts.max())
    tw = np.minimum(8, W - 8 * np.arange(TX))
    th = np.minimum(8, H - 8 * np.arange(TY))
    samples = int(((th[:, None] * tw[None, :]).ravel() * counts.astype(np.int64)).sum())
    d = context(scene_of(sid), cap)
    d.set_moments(True)
    ex = rtamd.RaytraceExecutor(d, seed=SEED)
    ex.setSamplePerPixel(cap)
    st = ex.raytraceAdaptive(target, batch=8, min_frames=8)
    assert ex.getNumSamples() == done and st == last and list(d.read_tile_frames()) == list(counts)
    assert ex.sampleComplete() == bool(last["converged"] or done == cap)
    d.close()
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracing-book_amd", "bin", "rtrender")
    r = subprocess.run([exe, "-s", str(sid), "-r", f"{W}:{H}", "-spp", str(cap), "-md", "5", "--seed", str(SEED),
                        "--frames-per-launch", "8", "--noise", f"{target:.9g}", "--adaptive", "--min-frames", "8"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = re.search(r"Adaptive: (\d+) frames, (\d+) of (\d+) samples, noise (\S+) \((converged|sample cap reached)\)", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) == done and int(m.group(2)) == samples and int(m.group(3)) == W * H * done
    assert float(m.group(4)) == pytest.approx(last["noise"], rel=1e-5)
    assert m.group(5) == ("converged" if last["converged"] else "sample cap reached")

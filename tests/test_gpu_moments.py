"""Per-pixel sample moments and the noise-target loop on the device (rt.h rt_set_moments ...
rt_render_until; kernels in raytracing-book_amd/csrc/rt_moments.hip).

Every case: depth 5, seed 1, small images.  The folds are replayed in numpy float32 from the
staged colours (rt_debug_read_samples), so image and moments are checked bit for bit; the tile
reduction is replayed in its fixed butterfly order.
"""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import rtamd
from helpers import bit_equal, gpu_image, mismatch_report, oracle_image

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "raytracing-book_amd", "bin", "rtrender")
W, H = 24, 20   # partial tiles in y
SEED = 1


def context(scene, spp, options=None, **kw):
    ctx = rtamd.RenderContext(options=options, **kw)
    ctx.upload_scene(scene)
    ctx.set_params(max_depth=5, spp=spp)
    ctx.resize(scene.width, scene.height)
    return ctx


def render(ctx, first, n):
    ctx.render(first, rtamd.frame_rand_factors(SEED, first - 1, n))


def replay(mean, m2, samples, first_frame):
    """The recurrence of the folds (rt_moments.hip mean_step, moment_step) in float32, one operation at a time."""
    mean, m2 = mean.astype(np.float32).copy(), m2.astype(np.float32).copy()
    with np.errstate(all="ignore"):
        for f in range(samples.shape[0]):
            fc = first_frame + f
            n1, n = np.float32(fc - 1), np.float32(fc)
            c = samples[f, ..., :3]
            old = mean[..., :3]
            new = (old * n1 + c) / n
            if fc == 1:
                m2[:] = 0.0
            else:
                m2[..., :3] = m2[..., :3] + (c - old) * (c - new)
                ys = (c[..., 0] + c[..., 1]) + c[..., 2]
                yo = (old[..., 0] + old[..., 1]) + old[..., 2]
                yn = (new[..., 0] + new[..., 1]) + new[..., 2]
                m2[..., 3] = m2[..., 3] + (ys - yo) * (ys - yn)
            mean[..., :3] = new
            mean[..., 3] = 1.0
    assert mean.dtype == np.float32 and m2.dtype == np.float32
    return mean, m2


@functools.lru_cache(maxsize=None)
def two_launches(sid, sparse):
    """Frames 1..11, then 12..16, moments on: image, moments and staged colours after each."""
    scene = rtamd.Scene(sid, W, H, seed=SEED)
    ctx = context(scene, 16, options=None if sparse else {"sparse_stage": 0})
    ctx.set_moments(True)
    out = []
    for first, n in ((1, 11), (12, 5)):
        render(ctx, first, n)
        out.append(dict(first=first, n=n, image=ctx.read_image(), m2=ctx.read_moments(), samples=ctx.read_samples(),
                        launch=ctx.last_launch()))
    ctx.close()
    return scene, out


CASES = [(6, True), (0, True), (8, True), (6, False)]


@pytest.mark.parametrize("sid,sparse", CASES)
def test_image_untouched(gpu, sid, sparse):
    scene, runs = two_launches(sid, sparse)
    for r in runs:
        assert r["launch"]["staged"] == 1 and r["launch"]["sparse"] == (1 if sparse else 0)
    img = runs[1]["image"]
    plain = gpu_image(scene, 16, chunks=[11, 5], options=None if sparse else {"sparse_stage": 0})
    assert bit_equal(img, plain), mismatch_report(img, plain)
    ref = oracle_image(scene, 16)
    assert bit_equal(img, ref), mismatch_report(img, ref)


@pytest.mark.parametrize("sid,sparse", CASES)
def test_moments_exact(gpu, sid, sparse):
    _, runs = two_launches(sid, sparse)
    mean = np.zeros((H, W, 4), np.float32)
    m2 = np.zeros((H, W, 4), np.float32)
    for r in runs:
        assert r["samples"].shape == (r["n"], H, W, 4)
        mean, m2 = replay(mean, m2, r["samples"], r["first"])
        assert bit_equal(r["image"], mean), mismatch_report(r["image"], mean)
        assert bit_equal(r["m2"], m2), mismatch_report(r["m2"], m2)
    assert np.nanmax(runs[1]["m2"]) > 0.0


FW, FH = 20, 12          # 3 x 2 tiles: partial ones at the right and at the bottom
FOLD_MASK = (0, 2, 5)    # a full tile, a right-edge tile, the corner tile


def fold_pattern(base):
    """A distinct positive finite float per word (x * 0 is then +0, a zero image's)."""
    return (np.uint32(base) + np.arange(FH * FW * 4, dtype=np.uint32)).view(np.float32).reshape(FH, FW, 4).copy()


@functools.lru_cache(maxsize=None)
def fold_run(n, sparse, masked, mom):
    """Scene 6, frames 1..n over a pattern image (and pattern moments), under FOLD_MASK or no mask."""
    ctx = context(rtamd.Scene(6, FW, FH, seed=SEED), 16, options=None if sparse else {"sparse_stage": 0})
    if mom:
        ctx.set_moments(True)
    ctx.write_image(fold_pattern(0x3F800000))
    if mom:
        ctx.write_moments(fold_pattern(0x40000000), 5)
    if masked:
        mask = np.zeros(6, np.uint8)
        mask[list(FOLD_MASK)] = 1
        ctx.set_active_tiles(mask)
    render(ctx, 1, n)
    ctx.sync()
    out = dict(launch=ctx.last_launch(), image=ctx.read_image(), m2=ctx.read_moments() if mom else None)
    out["samples"] = ctx.read_samples() if out["launch"]["staged"] else None
    ctx.close()
    return out


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", [1, 3, 8, 11])   # in place / the tail alone / one block of eight / a block and a tail
def test_one_fold_body(gpu, n, masked):
    """The staged folds (rt_moments.hip fold_pixel: per pixel or per active tile, mean alone or with the
    moments, dense or sparse) against the numpy restatement of the staged colours, bit for bit; the image
    bits do not depend on the moments or on sparse staging; a masked fold leaves every other word alone."""
    px = np.zeros((FH, FW), bool)
    for t in (FOLD_MASK if masked else range(6)):
        px[(t // 3) * 8:(t // 3) * 8 + 8, (t % 3) * 8:(t % 3) * 8 + 8] = True
    pat, pat2 = fold_pattern(0x3F800000), fold_pattern(0x40000000)
    runs = {(sparse, mom): fold_run(n, sparse, masked, mom) for sparse in (False, True) for mom in (False, True)}
    staged_runs = 0
    for (sparse, mom), r in runs.items():
        ll = r["launch"]
        print(f"n {n} masked {masked} sparse {sparse} moments {mom}: {ll}")
        assert ll["tiles_active"] == (3 if masked else 6)
        if mom:
            assert ll["staged"] == 1
        assert not ll["staged"] or ll["sparse"] == (1 if sparse else 0)
        if r["samples"] is not None:
            staged_runs += 1
            s = r["samples"]
            assert s.shape == (n, FH, FW, 4)
            mean, m2 = replay(pat, pat2, s, 1)
            assert bit_equal(r["image"][px], mean[px]), mismatch_report(r["image"], np.where(px[..., None], mean, pat))
            if mom:
                assert bit_equal(r["m2"][px], m2[px])
            if n >= 3:   # both kinds of colour: sparse staging stores the one and flags the other
                zero = (s[..., :3].view(np.uint32) == 0).all(axis=-1)[:, px]
                assert zero.any() and not zero.all()
        assert np.array_equal(r["image"][~px].view(np.uint32), pat[~px].view(np.uint32))
        if mom:
            assert np.array_equal(r["m2"][~px].view(np.uint32), pat2[~px].view(np.uint32))
    assert staged_runs >= 2
    first = runs[(True, True)]["image"]
    for key, r in runs.items():
        assert bit_equal(r["image"], first), (key, mismatch_report(r["image"], first))
    assert bit_equal(runs[(False, True)]["m2"], runs[(True, True)]["m2"])


def test_moments_mean_what_they_say(gpu):
    """Scene 0, frames 1..16: M2 against the float64 two-pass sum of squared deviations of the same
    samples, |M2 - M2_ref| <= 8 n 2^-24 (M2_ref + n mean^2) per finite pixel and channel."""
    _, runs = two_launches(0, True)
    s = np.concatenate([runs[0]["samples"], runs[1]["samples"]]).astype(np.float64)
    n = s.shape[0]
    assert n == 16
    c = np.concatenate([s[..., :3], s[..., :3].sum(axis=-1, keepdims=True)], axis=-1)   # x, y, z, channel sum
    with np.errstate(all="ignore"):
        mean = c.mean(axis=0)
        ref = ((c - mean) ** 2).sum(axis=0)
        got = runs[1]["m2"].astype(np.float64)
        bound = 8.0 * n * 2.0 ** -24 * (ref + n * mean ** 2)
        ok = np.isfinite(ref) & np.isfinite(got)
        assert ok.mean() > 0.9
        err = np.abs(got - ref)
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    print(f"moments vs float64 two-pass: max |err| / bound = {ratio[ok].max():.4f} over {int(ok.sum())} values")
    assert (err[ok] <= bound[ok]).all(), f"max |err| / bound = {ratio[ok].max()}"
    assert ref[ok].max() > 0.0


def test_one_frame_launches(gpu):
    scene = rtamd.Scene(0, W, H, seed=SEED)
    a = context(scene, 5)
    a.set_moments(True)
    for f in range(1, 6):
        render(a, f, 1)
        ll = a.last_launch()
        assert ll["staged"] == 1 and ll["chunks"] == 1, ll
    b = context(scene, 5)
    b.set_moments(True)
    render(b, 1, 5)
    assert b.last_launch()["staged"] == 1
    img_a, m2_a, img_b, m2_b = a.read_image(), a.read_moments(), b.read_image(), b.read_moments()
    a.close()
    b.close()
    assert bit_equal(img_a, img_b), mismatch_report(img_a, img_b)
    assert bit_equal(m2_a, m2_b), mismatch_report(m2_a, m2_b)
    assert bit_equal(img_a, gpu_image(scene, 5))


def tile_sums_ref(img, m2):
    """tile_sums_kernel in numpy: lane ty * 8 + tx, x += x[lane ^ off] for off = 32 .. 1."""
    h, w = img.shape[:2]
    tx, ty = (w + 7) // 8, (h + 7) // 8
    out = np.zeros(tx * ty, rtamd.TILE_SUM_DTYPE)
    lanes = np.arange(64)
    with np.errstate(all="ignore"):
        for t in range(tx * ty):
            sm, sy = np.zeros(64, np.float32), np.zeros(64, np.float32)
            bad = pixels = 0
            for l in range(64):
                x, y = (t % tx) * 8 + (l & 7), (t // tx) * 8 + (l >> 3)
                if x >= w or y >= h:
                    continue
                pixels += 1
                lum = np.float32(np.float32(img[y, x, 0] + img[y, x, 1]) + img[y, x, 2])
                if np.isfinite(lum) and np.isfinite(m2[y, x, 3]):
                    sm[l], sy[l] = m2[y, x, 3], lum
                else:
                    bad += 1
            for off in (32, 16, 8, 4, 2, 1):
                sm = sm + sm[lanes ^ off]
                sy = sy + sy[lanes ^ off]
            assert len(set(sm.view(np.uint32))) == 1 and len(set(sy.view(np.uint32))) == 1
            out[t] = (sm[0], sy[0], bad, pixels)
    return out


def test_reduction_exact(gpu):
    w, h = 20, 12
    rng = np.random.default_rng(7)
    img = (rng.random((h, w, 4), dtype=np.float32) * np.float32(3.0)).astype(np.float32)
    m2 = (rng.random((h, w, 4), dtype=np.float32) * np.exp(rng.normal(0, 4, (h, w, 4))).astype(np.float32))
    m2 = m2.astype(np.float32)
    img[0, 0, 1] = np.nan
    img[3, 9, 0] = np.inf
    img[11, 19, 2] = -np.inf
    img[5, 17, :3] = np.float32(3e38)        # finite channels, their sum is not
    m2[2, 2, 3] = np.nan
    m2[9, 4, 3] = np.inf
    m2[10, 18, 3] = -np.inf
    m2[1, 1, 3] = np.float32(-0.75)          # negative but finite: summed as it is
    m2[8, 8, 3] = np.float32(-1e-3)
    m2[4, 4, 0] = np.nan                     # not a component the sums read
    ctx = rtamd.RenderContext()
    ctx.resize(w, h)
    ctx.set_moments(True)
    ctx.write_image(img)
    ctx.write_moments(m2, 7)
    got = ctx.tile_sums()
    back = ctx.read_moments()
    stats = ctx.noise()
    ctx.close()
    assert bit_equal(back, m2)
    ref = tile_sums_ref(img, m2)
    assert got.shape == ref.shape == (6,)
    assert got.tobytes() == ref.tobytes(), (got, ref)
    assert int(got["pixels"].sum()) == w * h and int(got["bad"].sum()) == 7
    assert list(got["pixels"]) == [64, 64, 32, 32, 32, 16]
    assert stats == rtamd.noise_from_tile_sums(ref, 7)


def rt_err_state(fn):
    with pytest.raises(rtamd.RTError) as e:
        fn()
    assert e.value.code == -3, e.value   # RT_ERR_STATE


def test_state_rules(gpu):
    scene = rtamd.Scene(0, W, H, seed=SEED)
    ctx = context(scene, 8)
    ctx.set_moments(True)
    rt_err_state(ctx.noise)                       # before any render
    rt_err_state(ctx.read_moments)
    render(ctx, 1, 4)
    first = ctx.noise()
    assert first["frames"] == 4 and first["noise"] > 0 and first["pixels"] == W * H
    render(ctx, 7, 2)                             # a gap: frames 5, 6 never rendered
    rt_err_state(ctx.noise)
    render(ctx, 1, 4)                             # works again after a render from frame 1
    again = ctx.noise()
    assert again == first
    render(ctx, 5, 2)                             # extends
    assert ctx.noise()["frames"] == 6
    ctx.write_image(ctx.read_image())
    rt_err_state(ctx.noise)
    rt_err_state(ctx.tile_sums)
    render(ctx, 1, 1)                             # one frame: no variance yet
    rt_err_state(ctx.noise)
    assert not ctx.read_moments().any()
    ctx.resize(W, H)
    rt_err_state(ctx.read_moments)
    ctx.set_moments(False)
    rt_err_state(ctx.noise)
    render(ctx, 1, 1)
    assert ctx.last_launch()["staged"] == 0       # moments off: one frame in place, as ever
    ctx.close()
    two = rtamd.RenderContext(devices=(0, 0))
    rt_err_state(lambda: two.set_moments(True))
    two.close()


def test_partition(gpu):
    """Ranks 0 and 1 of world 2 with 8-row stripes, one after the other: their tiles are the
    single context's tiles, so the tile sums agree as multisets of bit patterns."""
    scene = rtamd.Scene(0, 20, 32, seed=SEED)
    single = context(scene, 8)
    single.set_moments(True)
    render(single, 1, 8)
    whole = single.tile_sums()
    whole_noise = single.noise()
    single.close()
    parts = []
    for rank in range(2):
        ctx = context(scene, 8, rank=rank, world=2, stripe_rows=8)
        ctx.set_moments(True)
        render(ctx, 1, 8)
        assert ctx.local_rows == 16
        parts.append(ctx.tile_sums())
        ctx.close()
    both = np.concatenate(parts)
    assert both.size == whole.size == 12
    assert sorted(t.tobytes() for t in both) == sorted(t.tobytes() for t in whole)
    summed = rtamd.noise_from_tile_sums(both, 8)
    assert summed["pixels"] == whole_noise["pixels"] == 20 * 32 and summed["bad"] == whole_noise["bad"]
    assert summed["noise"] == pytest.approx(whole_noise["noise"], rel=1e-12)


def test_until_loop(gpu):
    scene = rtamd.Scene(0, W, H, seed=SEED)
    batch, cap = 4, 32
    a = context(scene, cap)
    a.set_moments(True)
    noises, images = [], []
    for k in range(cap // batch):
        render(a, 1 + k * batch, batch)
        noises.append(a.noise()["noise"])
        images.append(a.read_image())
    a.close()
    assert all(np.isfinite(noises)) and min(noises) > 0
    # the target is a float in the ABI: the float at or just above noise_3
    target = np.float32(noises[2])
    if float(target) < noises[2]:
        target = np.nextafter(target, np.float32(np.inf))
    stop = next(k for k, v in enumerate(noises) if v <= float(target))
    assert stop <= 2
    b = context(scene, cap)
    b.set_moments(True)
    done, last = b.render_until(float(target), cap, batch, seed=SEED)
    img = b.read_image()
    b.close()
    assert done == (stop + 1) * batch and last["converged"] == 1 and last["frames"] == done
    assert last["noise"] == noises[stop]
    assert bit_equal(img, images[stop]), mismatch_report(img, images[stop])
    c = context(scene, cap)
    c.set_moments(True)
    done, last = c.render_until(0.0, cap, batch, seed=SEED)
    img = c.read_image()
    c.close()
    assert done == cap and last["converged"] == 0 and last["noise"] == noises[-1]
    assert bit_equal(img, images[-1])
    # the executor mirror: the same loop, samplePerPixel as the cap
    d = context(scene, cap)
    d.set_moments(True)
    ex = rtamd.RaytraceExecutor(d, seed=SEED)
    ex.setSamplePerPixel(cap)
    st = ex.raytraceUntil(float(target), batch)
    assert st["converged"] == 1 and ex.getNumSamples() == (stop + 1) * batch and ex.sampleComplete()
    d.close()
    # the command line prints the same frame count
    r = subprocess.run([BIN, "-s", "0", "-r", f"{W}:{H}", "-spp", str(cap), "-md", "5", "--seed", str(SEED),
                        "--frames-per-launch", str(batch), "--noise", f"{float(target):.9g}"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = re.search(r"Noise target: (\d+) frames, noise (\S+) \((converged|sample cap reached)\)", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) == (stop + 1) * batch and m.group(3) == "converged"
    assert float(m.group(2)) == pytest.approx(noises[stop], rel=1e-5)
    r = subprocess.run([BIN, "-s", "0", "-r", f"{W}:{H}", "-spp", "8", "--noise", "0.5", "--devices", "0,0"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--noise" in r.stderr

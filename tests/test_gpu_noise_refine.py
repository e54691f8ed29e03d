"""The moved view rendered to a noise target, on the device (rt.h rt_noise_tiles / rt_read_tile_noise /
rt_render_moved_to_noise; rt_refine.hip): the records against rt_tile_noise_host and the NumPy restatement bit for
bit, a real move's records, the one call per pose against the public calls made one by one, a stopped tile's bits
against a plain render's, the extremes, everything else left as it was, and the state rules.  The shapes and the
move are test_gpu_reproject_var.py's; renders are depth 5, seed 1.
"""
import ctypes

import numpy as np
import pytest

import rtamd
from rtamd import _lib
from helpers import bit_equal, mismatch_report
import noise_refine_ref as NR
from test_gpu_present import held, moved_to_b, read_denoised
from test_gpu_reproject_var import CASES, context, render, rt_err, scene_of, view

pytestmark = pytest.mark.gpu

F = np.float32
FLT_MAX = float(np.finfo(F).max)
MIN_COUNTS = (2.0, 4.0, 1e9)
MAX_ROUNDS = 3


def same_records(a, b):
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


def at_a(scene, variance=True, frames=8):
    ctx = context(scene, variance=variance)
    ctx.set_moments(True)
    render(ctx, 1, frames)
    ctx.render_features()
    return ctx


def per_pixel(tiles, w, h):
    """One value per 8x8 tile (row-major) -> [h, w]."""
    tx, ty = (w + 7) // 8, (h + 7) // 8
    return np.repeat(np.repeat(np.asarray(tiles).reshape(ty, tx), 8, axis=0), 8, axis=1)[:h, :w]


def per_tile_count(mask, w, h):
    """[h, w] bool -> the number of set pixels per 8x8 tile, row-major."""
    tx, ty = (w + 7) // 8, (h + 7) // 8
    p = np.zeros((ty * 8, tx * 8), np.int64)
    p[:h, :w] = mask
    return p.reshape(ty, 8, tx, 8).sum(axis=(1, 3)).ravel()


def host_records(ctx, mc):
    return rtamd.tile_noise_host(ctx.read_reprojected(), ctx.read_reprojected_variance(), mc)


# ---- 1. the device against the host function and the restatement ---------------------------------------------

def check_records(ctx, w, h):
    rp, s2 = ctx.read_reprojected(), ctx.read_reprojected_variance()
    nt = ((w + 7) // 8) * ((h + 7) // 8)
    n = rp[..., 3]
    with np.errstate(invalid="ignore"):
        y = ((rp[..., 0] + rp[..., 1]).astype(F) + rp[..., 2]).astype(F)
        good = (np.abs(y) <= FLT_MAX) & (n > 0) & (np.abs(n) <= FLT_MAX)
        known = good & (s2 >= 0) & (np.abs(s2) <= FLT_MAX)
    for mc in MIN_COUNTS:
        ctx.noise_tiles(mc)
        got = ctx.read_tile_noise()
        ref = rtamd.tile_noise_host(rp, s2, mc)
        assert got.shape == (nt,) and same_records(got, ref), (mc, got, ref)
        assert same_records(ref, NR.tile_noise(rp, s2, mc))                   # the host is the restatement here too
        assert got["pixels"].sum() == w * h
        ctx.reach_tiles(mc)                                                   # the count criterion's records, side by side
        reach = ctx.read_tile_reach()
        assert (got["thin_px"].astype(int) >= reach["short_px"].astype(int) - got["bad_px"]).all(), mc
        assert same_records(ctx.read_tile_noise(), got)                       # ... and both are held
        if (known == good).all():                                             # every good pixel's s2 is known: thin is short
            with np.errstate(invalid="ignore"):
                assert np.array_equal(got["thin_px"], per_tile_count(good & (n < F(mc)), w, h)), mc
    assert np.array_equal(got["thin_px"], got["pixels"] - got["bad_px"])      # nothing reaches 1e9
    assert bit_equal(ctx.read_reprojected(), rp) and bit_equal(ctx.read_reprojected_variance(), s2)
    return known, good


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"scene{c[0]}_{c[1]}x{c[2]}")
def test_device_matches_the_host(gpu, case):
    sid, w, h = case
    ctx, _ = moved_to_b(case)
    check_records(ctx, w, h)
    ctx.close()
    # where every good pixel's variance is known (2 frames at B): thin_px is the count below min_count
    ctx, _ = moved_to_b(case, frames_b=2)
    known, good = check_records(ctx, w, h)
    assert (known == good).all() and good.any()
    ctx.close()


def test_device_matches_the_host_with_the_misses_reprojected(gpu):
    sid, w, h = case = CASES[0]
    ctx, _ = moved_to_b(case)
    ctx.noise_tiles(2.0)
    off = ctx.read_tile_noise()
    ctx.set_reproject_misses(True)
    ctx.reproject()
    check_records(ctx, w, h)
    ctx.noise_tiles(2.0)
    on = ctx.read_tile_noise()
    assert on["thin_px"].sum() < off["thin_px"].sum()                         # the background keeps its history
    ctx.close()


# ---- 2. a real move is not a trivial case --------------------------------------------------------------------

def test_a_real_move_is_not_trivial(gpu):
    w = h = 32
    ctx, _ = moved_to_b((6, w, h))
    ctx.noise_tiles(2.0)
    got = ctx.read_tile_noise()
    print("thin_px", got["thin_px"].tolist(), "known_px", got["known_px"].tolist())
    assert 0 < (got["thin_px"] > 0).sum() < got.size
    assert 0 < got["known_px"].sum() < w * h
    ctx.close()


# ---- 3. one call against the public calls one by one ---------------------------------------------------------

def median_target(rec):
    """The median over the tiles with a known pixel of sqrt(v_t) / ybar: about half of them lie above it."""
    K = rec["known_px"].astype(np.float64)
    ybar = rec["y_sum"].astype(np.float64).sum() / (rec["pixels"].astype(np.int64) - rec["bad_px"]).sum()
    v_t = rec["v_sum"].astype(np.float64)[K > 0] / K[K > 0]
    return float(F(np.median(np.sqrt(v_t)) / ybar))


def to_b_by_steps(steps, scene, rf, n, hist):
    steps.history_capture(hist)
    steps.set_camera(scene.camera)
    steps.render(1, rf[:n])
    steps.render_features()
    steps.reproject()


def rounds_by_steps(steps, rf, n, target, batch, max_rounds, mc=2.0):
    """rt_render_moved_to_noise's loop through the public calls -> (rounds, tiles in round 1, tile-frames, stats)."""
    nt = steps.read_tile_frames().size
    active = np.ones(nt, np.uint8)
    r = first = spent = 0
    while True:
        steps.noise_tiles(mc)
        rec = steps.read_tile_noise()
        host = host_records(steps, mc)                                        # the host path on read-backs
        assert same_records(rec, host), r
        sel, stats = rtamd.refine_noise_select(rec, target, active)
        ref_sel, ref_stats = NR.noise_select(host, target, active)
        assert np.array_equal(sel, ref_sel) and stats == ref_stats, r        # ... selects the same tiles each round
        assert not (sel & ~active).any()                                      # the set only shrinks
        active = sel
        if not sel.any():
            stats["converged"] = 1
            break
        if r == max_rounds:
            break
        done = n + r * batch
        assert set(steps.read_tile_frames()[sel == 1].tolist()) == {done}     # every active tile holds that many
        steps.set_active_tiles(None if sel.all() else sel)
        steps.render(done + 1, rf[done:done + batch])
        steps.set_active_tiles(None)
        steps.reproject()
        if r == 0:
            first = int(sel.sum())
        spent += int(sel.sum()) * batch
        r += 1
    stats["rounds"] = r
    return r, first, spent, stats


def same_state(one, steps, camera, tag):
    assert bit_equal(one.read_reprojected(), steps.read_reprojected()), tag
    assert bit_equal(one.read_reprojected_variance(), steps.read_reprojected_variance()), tag
    assert bit_equal(read_denoised(one), read_denoised(steps)), tag
    assert np.array_equal(one.read_tile_frames(), steps.read_tile_frames()), tag
    va, vb = view(one, camera), view(steps, camera)
    for key in ("image", "m2", "nd", "ai"):
        assert bit_equal(va[key], vb[key]), (tag, key, mismatch_report(va[key], vb[key]))


@pytest.mark.parametrize("batch", [1, 2], ids=["batch1", "batch2"])
def test_render_moved_to_noise_is_the_public_calls_one_by_one(gpu, batch):
    sid, w, h = 6, 32, 32
    a = scene_of(sid, w, h, 0)
    one, steps = at_a(a), at_a(a)
    target = None
    spent_all = 0
    for pose, (n, hist) in enumerate(((1, "image"), (2, "reprojected"), (1, "reprojected"))):
        scene = scene_of(sid, w, h, pose + 1)
        rf = rtamd.frame_rand_factors(1, 10 * pose, n + batch * MAX_ROUNDS)
        to_b_by_steps(steps, scene, rf, n, hist)
        if target is None:
            target = median_target(host_records(steps, 2.0))                  # from the data: splits the first pose's tiles
            assert 0.0 < target < FLT_MAX
        r, first, spent, stats = rounds_by_steps(steps, rf, n, target, batch, MAX_ROUNDS)
        steps.denoise_reprojected()
        ref8 = steps.present("moved", exposure=0.5, keep_float=True)
        reff = steps.read_presented_float()
        got8, info = one.render_moved(scene.camera, rf, keep_float=True, exposure=0.5,
                                      noise_refine=dict(target_noise=target, batch_frames=batch, max_rounds=MAX_ROUNDS))
        gotf = one.read_presented_float()
        print(pose, info)
        assert (info["rounds_done"], info["tiles_refined"], info["tile_frames_spent"]) == (r, first, spent), (pose, info)
        assert {k: info[k] for k in stats} == stats, (pose, info, stats)
        assert np.array_equal(got8, ref8), (pose, np.argwhere(got8 != ref8)[:4])
        assert bit_equal(gotf, reff), (pose, mismatch_report(gotf, reff))
        same_state(one, steps, scene.camera, pose)
        tf = one.read_tile_frames()
        assert tf.min() >= n and tf.max() == n + r * batch and tf.astype(np.int64).sum() - n * tf.size == spent
        spent_all += spent
    assert spent_all > 0
    for ctx in (one, steps):
        ctx.close()


# ---- 4. a stopped tile holds a plain render's bits -----------------------------------------------------------

def test_stopped_tiles_hold_the_bits_of_a_plain_render(gpu):
    # the median target of test 3 with batch_frames 1: the tiles under it stop with the pose's one frame, the
    # thin ones get a second at least, so two distinct counts occur without falling back to the lower quartile
    sid, w, h, n, batch = 6, 32, 32, 1, 1
    a, b = scene_of(sid, w, h, 0), scene_of(sid, w, h, 1)
    rf = rtamd.frame_rand_factors(1, 0, n + batch * MAX_ROUNDS)
    probe = at_a(a)
    to_b_by_steps(probe, b, rf, n, "image")
    target = median_target(host_records(probe, 2.0))
    probe.close()
    ctx = at_a(a)
    _, info = ctx.render_moved(b.camera, rf, noise_refine=dict(target_noise=target, batch_frames=batch, max_rounds=MAX_ROUNDS))
    tf = ctx.read_tile_frames()
    counts = sorted(set(tf.tolist()))
    print("counts", counts, info)
    assert len(counts) >= 2 and counts[0] >= n and counts[-1] == n + info["rounds_done"] * batch
    img, m2 = ctx.read_image(), ctx.read_moments()
    plain = context(b)
    plain.set_moments(True)
    for c in counts:
        plain.render(1, rf[:c])
        at_c = per_pixel(tf, w, h) == c
        for got, ref in ((img, plain.read_image()), (m2, plain.read_moments())):
            assert bit_equal(got[at_c], ref[at_c]), (c, mismatch_report(got[at_c], ref[at_c]))
    plain.close()
    # the last reproject saw the counts: a pixel the history does not reach holds its tile's frames
    rp = ctx.read_reprojected()
    n_t = per_pixel(tf, w, h).astype(F)
    fresh = rp[..., 3] <= n_t
    assert fresh.any() and (rp[..., 3][fresh] == n_t[fresh]).all()
    ctx.close()


# ---- 5. the extremes -----------------------------------------------------------------------------------------

def raw_to_noise(ctx, camera, rf, n, refine=None, outs=True):
    cam = np.ascontiguousarray(camera, F).ravel()
    rf = np.ascontiguousarray(rf, F)
    rounds, tiles, spent, stats = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int64(-1), _lib.RtMovedNoiseStats()
    ref = lambda v: ctypes.byref(v) if outs else None  # noqa: E731
    ctx._check(ctx._L.rt_render_moved_to_noise(ctx._h, cam.ctypes.data_as(_lib.c_float_p), int(n), rf.ctypes.data_as(_lib.c_float_p),
                                               None if refine is None else ctypes.byref(refine), None, None, None, None,
                                               ref(rounds), ref(tiles), ref(spent), ref(stats)))
    return ctx.read_presented(), (rounds.value, tiles.value, spent.value), stats.as_dict()


def noise_params(target_noise=0.1, min_count=0.0, batch_frames=1, max_rounds=4, reserved=()):
    p = _lib.RtNoiseRefineParams()
    p.target_noise, p.min_count, p.batch_frames, p.max_rounds = target_noise, min_count, batch_frames, max_rounds
    for i, r in enumerate(reserved):
        p.reserved[i] = r
    return p


def test_extremes(gpu):
    sid, w, h = 6, 32, 32
    a, b = scene_of(sid, w, h, 0), scene_of(sid, w, h, 1)
    rf = rtamd.frame_rand_factors(1, 0, 5)
    # the plain moved view, its records and its figures
    plain = at_a(a)
    ref = plain.render_moved(b.camera, rf[:1])
    plain.noise_tiles(2.0)
    rec = plain.read_tile_noise()
    thin = rec["thin_px"] > 0
    assert 0 < thin.sum() < rec.size
    # FLT_MAX: the variance never asks for a frame, the thin tiles get exactly one
    ctx = at_a(a)
    _, info = ctx.render_moved(b.camera, rf, noise_refine=dict(target_noise=FLT_MAX, batch_frames=1, max_rounds=4))
    assert info["converged"] == 1 and 1 <= info["rounds_done"] <= 2, info
    assert np.array_equal(ctx.read_tile_frames(), np.where(thin, 2, 1)), info
    assert info["tiles_refined"] == thin.sum() == info["tile_frames_spent"] and info["thin"] == 0
    ctx.close()
    # max_rounds 0: a noise figure and nothing else
    _, stats0 = rtamd.refine_noise_select(rec, 0.05)
    for rounds0 in (dict(target_noise=0.05, max_rounds=0), dict(target_noise=0.05, max_rounds=0, batch_frames=3, min_count=2.0)):
        ctx = at_a(a)
        frame, info = ctx.render_moved(b.camera, rf[:1], noise_refine=rounds0)
        assert np.array_equal(frame, ref)
        assert (info["rounds_done"], info["tiles_refined"], info["tile_frames_spent"], info["converged"]) == (0, 0, 0, 0)
        assert {k: info[k] for k in stats0} == stats0 and 0.0 < info["noise"] < float("inf")
        assert ctx.read_tile_frames().tolist() == [1] * 16
        for got, want in ((ctx.read_image(), plain.read_image()), (ctx.read_moments(), plain.read_moments()),
                          (ctx.read_reprojected(), plain.read_reprojected()), (read_denoised(ctx), read_denoised(plain))):
            assert bit_equal(got, want)
        ctx.close()
    # refine NULL: rt_render_moved
    ctx = at_a(a)
    frame, outs, stats = raw_to_noise(ctx, b.camera, rf[:1], 1, None)
    assert np.array_equal(frame, ref) and outs == (0, 0, 0) and stats["noise"] == 0.0 and stats["pixels"] == 0
    bare = at_a(a)                                                           # ... with every output NULL
    assert np.array_equal(raw_to_noise(bare, b.camera, rf[:1], 1, None, outs=False)[0], ref)
    assert np.array_equal(raw_to_noise(bare, scene_of(sid, w, h, 2).camera, rf, 1, noise_params(target_noise=FLT_MAX), outs=False)[0],
                          bare.read_presented())
    bare.close()
    for got, want in ((ctx.read_image(), plain.read_image()), (ctx.read_moments(), plain.read_moments()),
                      (ctx.read_reprojected(), plain.read_reprojected()),
                      (ctx.read_reprojected_variance(), plain.read_reprojected_variance()), (read_denoised(ctx), read_denoised(plain))):
        assert bit_equal(got, want)
    rt_err(-3, ctx.read_tile_noise, "rt_noise_tiles")                         # no record was made
    ctx.close()
    plain.close()


# ---- 6. nothing else moves -----------------------------------------------------------------------------------

def test_everything_else_keeps_its_bits(gpu):
    case = (6, 32, 32)

    def run(noising):
        ctx, b = moved_to_b(case, frames_b=2)
        frame = ctx.present("moved", exposure=0.5, keep_float=True)
        ctx.reach_tiles(4.0)
        reach = ctx.read_tile_reach()
        before = held(ctx)
        hist = None
        if noising:
            for mc in MIN_COUNTS:
                ctx.noise_tiles(mc)
                assert ctx.read_tile_noise().shape == (16,)
            after = held(ctx)
            for k in ("image", "m2", "nd", "ai", "rp", "s2", "den"):
                assert bit_equal(before[k], after[k]), (k, mismatch_report(before[k], after[k]))
            assert list(before["tf"]) == list(after["tf"])
            assert same_records(ctx.read_tile_reach(), reach)                 # the reach records are still held
            assert np.array_equal(ctx.read_presented(), frame)               # the frame held, and what it binds to
            assert np.array_equal(ctx.present("moved", exposure=0.5, keep_float=True), frame)
        ctx.history_capture("reprojected")                                   # the history takes the same result
        flt = ctx.read_presented_float()
        render(ctx, 3, 2)                                                    # later frames
        ctx.reproject()
        out = dict(image=ctx.read_image(), m2=ctx.read_moments(), tf=list(ctx.read_tile_frames()), last=ctx.last_launch(),
                   rp=ctx.read_reprojected(), s2=ctx.read_reprojected_variance(), flt=flt, den=ctx.denoise(guides=True))
        ctx.close()
        return out

    yes, no = run(True), run(False)
    for k in ("image", "m2", "rp", "s2", "flt", "den"):
        assert bit_equal(yes[k], no[k]), (k, mismatch_report(yes[k], no[k]))
    assert yes["tf"] == no["tf"] == [4] * 16 and yes["last"] == no["last"]


# ---- 7. state and arguments ----------------------------------------------------------------------------------

def test_state_rules(gpu):
    scene, b = scene_of(6, 32, 32, 0), scene_of(6, 32, 32, 1)
    rf = rtamd.frame_rand_factors(1, 0, 5)
    two = rtamd.RenderContext(devices=(0, 0))
    two.upload_scene(scene)
    two.resize(32, 32)
    rt_err(-3, lambda: two.noise_tiles(2.0), "1-device")                     # a two-slot context
    rt_err(-3, two.read_tile_noise, "1-device")
    rt_err(-3, lambda: raw_to_noise(two, b.camera, rf, 1, noise_params()), "1-device")
    two.close()
    part = rtamd.RenderContext(rank=0, world=2, stripe_rows=8)
    part.upload_scene(scene)
    part.resize(32, 32)
    rt_err(-3, lambda: part.noise_tiles(2.0), "rt_set_partition")            # a partition
    rt_err(-3, part.read_tile_noise, "rt_set_partition")
    rt_err(-3, lambda: raw_to_noise(part, b.camera, rf, 1, noise_params()), "rt_set_partition")
    part.close()
    bare = rtamd.RenderContext()
    rt_err(-3, lambda: bare.noise_tiles(2.0), "no image")                    # no rt_resize yet
    bare.close()
    novar, _ = moved_to_b((6, 32, 32), variance=False)                       # a result without s2
    rt_err(-3, lambda: novar.noise_tiles(2.0), "rt_set_history_variance")
    rt_err(-3, lambda: raw_to_noise(novar, b.camera, rf, 1, noise_params()), "rt_set_history_variance")
    novar.close()

    ctx = at_a(scene)
    rt_err(-3, lambda: ctx.noise_tiles(2.0), "rt_reproject")                 # no result held
    rt_err(-3, ctx.read_tile_noise, "rt_noise_tiles")
    for mc in (0.0, -1.0, float("nan"), float("inf")):
        rt_err(-1, lambda: ctx.noise_tiles(mc), "min_count")
    # bad parameters: RT_ERR_INVALID_ARG before anything is queued, the counts untouched
    for bad in (dict(target_noise=-0.5), dict(target_noise=float("nan")), dict(target_noise=float("inf")), dict(min_count=-1.0),
                dict(min_count=float("nan")), dict(min_count=float("inf")), dict(batch_frames=0), dict(batch_frames=-2),
                dict(max_rounds=-1), dict(reserved=(1,)), dict(reserved=(0, 0, 0, 2)),
                dict(batch_frames=2 ** 30, max_rounds=2)):
        rt_err(-1, lambda: raw_to_noise(ctx, b.camera, rf, 1, noise_params(**bad)), "rt_render_moved_to_noise")
    assert ctx.read_tile_frames().tolist() == [8] * 16
    with pytest.raises(ValueError):
        ctx.render_moved(b.camera, rf, noise_refine=dict(target_noise=0.1, rounds=2))
    with pytest.raises(ValueError):
        ctx.render_moved(b.camera, rf, refine=dict(extra_frames=1), noise_refine=dict(target_noise=0.1))
    # a caller mask set on entry: refused, and left as it was
    mask = np.zeros(16, np.uint8)
    mask[3] = 1
    ctx.set_active_tiles(mask)
    rt_err(-3, lambda: raw_to_noise(ctx, b.camera, rf, 1, noise_params()), "tile mask")
    assert ctx.read_tile_frames().tolist() == [8] * 16
    render(ctx, 9, 1)
    assert ctx.last_launch()["tiles_active"] == 1 and ctx.read_tile_frames().tolist() == [8, 8, 8, 9] + [8] * 12
    ctx.set_active_tiles(None)
    # a pose to the target: no mask is left, a render from frame 1 samples every tile
    _, outs, stats = raw_to_noise(ctx, b.camera, rf, 1, noise_params(target_noise=FLT_MAX))
    assert 0 < outs[1] < 16 and sorted(set(ctx.read_tile_frames().tolist())) == [1, 2] and stats["converged"] == 1
    render(ctx, 1, 4)                                                        # (4 frames: a history whose variance is known)
    assert ctx.read_tile_frames().tolist() == [4] * 16 and ctx.last_launch()["tiles_active"] == 16
    # a step's refusal inside the loop comes back unchanged, and no mask is left: back to A, where the history
    # reaches a part of the view, with a rand factor that the masked render refuses
    ctx.render_features()
    bad_rf = np.array([0.5, 2048.0, 0.5, 0.5, 0.5], F)
    rt_err(-1, lambda: raw_to_noise(ctx, scene.camera, bad_rf, 1, noise_params(target_noise=FLT_MAX)))
    sel, _ = rtamd.refine_noise_select(ctx.read_tile_noise(), FLT_MAX)       # the records of the pose that was refused
    assert 0 < sel.sum() < 16
    render(ctx, 1, 1)
    assert ctx.read_tile_frames().tolist() == [1] * 16 and ctx.last_launch()["tiles_active"] == 16
    ctx.close()

    # the records: a short cap; a new rt_reproject, either switch and rt_resize drop them
    ctx, _ = moved_to_b((6, 32, 32))
    ctx.noise_tiles(2.0)
    n = ctypes.c_int()
    ctx._check(ctx._L.rt_read_tile_noise(ctx._h, None, 0, ctypes.byref(n)))
    assert n.value == 16
    out = np.zeros(16, rtamd.TILE_NOISE_DTYPE)
    rt_err(-4, lambda: ctx._check(ctx._L.rt_read_tile_noise(ctx._h, out.ctypes.data_as(ctypes.POINTER(_lib.RtTileNoise)), 15,
                                                            ctypes.byref(n))), "too small")
    first = ctx.read_tile_noise()
    ctx.reproject()
    rt_err(-3, ctx.read_tile_noise, "rt_noise_tiles")
    ctx.noise_tiles(2.0)
    assert same_records(ctx.read_tile_noise(), first)
    ctx.set_reproject_misses(True)                                           # the result dropped: so are its records
    rt_err(-3, ctx.read_tile_noise, "rt_noise_tiles")
    rt_err(-3, lambda: ctx.noise_tiles(2.0), "rt_reproject")
    ctx.reproject()
    ctx.noise_tiles(2.0)
    ctx.read_tile_noise()
    ctx.set_reproject_misses(True)                                           # the same value: nothing changes
    ctx.read_tile_noise()
    ctx.set_history_variance(False)
    rt_err(-3, ctx.read_tile_noise, "rt_noise_tiles")
    rt_err(-3, lambda: ctx.noise_tiles(2.0), "rt_reproject")
    ctx.set_history_variance(True)
    ctx.history_capture()
    ctx.reproject()
    ctx.noise_tiles(2.0)
    ctx.resize(32, 32)                                                       # rt_resize frees everything
    rt_err(-3, ctx.read_tile_noise, "rt_noise_tiles")
    rt_err(-3, lambda: ctx.noise_tiles(2.0), "rt_reproject")
    ctx.close()

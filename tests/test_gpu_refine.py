"""Extra frames where a moved view's history does not reach, on the device (rt.h rt_reach_tiles /
rt_read_tile_reach / rt_render_moved_refined; rt_refine.hip): the records against rt_tile_reach_host bit for
bit, the tiles chosen on a real move, a refined tile's bits against a plain render's, the one call per pose
against the public calls made one by one, no refinement against rt_render_moved, everything else left as it
was, and the state rules.  The shapes and the move are test_gpu_reproject_var.py's; renders are depth 5, seed 1.
"""
import ctypes

import numpy as np
import pytest

import rtamd
from rtamd import _lib
from helpers import bit_equal, mismatch_report
import refine_ref as RR
from test_gpu_present import held, moved_to_b, read_denoised
from test_gpu_reproject_var import CASES, context, render, rt_err, scene_of, view

pytestmark = pytest.mark.gpu

F = np.float32
MIN_COUNTS = (1.5, 4.0, 1e9)
# scene 6 at 32x32 after the quarter-viewport move, min_count 4: the top row and the left column of the 4x4 tiles
SCENE6_SHORT = [15, 8, 8, 9, 8, 0, 0, 0, 8, 0, 0, 0, 8, 0, 0, 0]


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


# ---- 1. the device against the host function -----------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=lambda c: f"scene{c[0]}_{c[1]}x{c[2]}")
def test_device_matches_the_host(gpu, case):
    sid, w, h = case
    ctx, _ = moved_to_b(case)
    rp = ctx.read_reprojected()
    nt = ((w + 7) // 8) * ((h + 7) // 8)
    for mc in MIN_COUNTS:
        ctx.reach_tiles(mc)
        got = ctx.read_tile_reach()
        ref = rtamd.tile_reach_host(rp, mc)
        assert got.shape == (nt,) and same_records(got, ref), (mc, got, ref)
        assert same_records(ref, RR.tile_reach(rp, mc))                       # the host is the restatement here too
        assert got["pixels"].sum() == w * h
    assert np.array_equal(got["short_px"], got["pixels"])                     # nothing reaches 1e9
    assert bit_equal(ctx.read_reprojected(), rp)
    ctx.close()


# ---- 2. the tiles chosen on a real move ----------------------------------------------------------------------

def test_selected_tiles_on_scene_6(gpu):
    ctx, b = moved_to_b((6, 32, 32))
    ctx.reach_tiles(4.0)
    got = ctx.read_tile_reach()
    ref = rtamd.tile_reach_host(ctx.read_reprojected(), 4.0)
    assert same_records(got, ref)
    print("short_px", got["short_px"].tolist())
    assert got["short_px"].tolist() == SCENE6_SHORT
    sel = rtamd.refine_select(got)
    assert np.array_equal(sel, rtamd.refine_select(ref)) and np.array_equal(sel, RR.refine_select(ref["short_px"])[0])
    assert 0 < sel.sum() < 16 and sel.sum() == 7
    assert sel.reshape(4, 4)[0].all() and sel.reshape(4, 4)[:, 0].all() and not sel.reshape(4, 4)[1:, 1:].any()
    capped = rtamd.refine_select(got, max_tiles=3)                            # the five 8s go together
    assert capped.sum() < sel.sum() and sorted(got["short_px"][capped == 1].tolist()) == [9, 15]
    ctx.close()
    # the same tiles through the one call: the automatic count of 1 + 3 frames is 4
    one = at_a(scene_of(6, 32, 32, 0))
    _, tiles = one.render_moved(b.camera, rtamd.frame_rand_factors(1, 0, 4), refine=dict(extra_frames=3))
    assert tiles == 7 and np.array_equal(one.read_tile_frames(), np.where(sel == 1, 4, 1))
    one.close()
    one = at_a(scene_of(6, 32, 32, 0))
    _, tiles = one.render_moved(b.camera, rtamd.frame_rand_factors(1, 0, 4), refine=dict(extra_frames=3, max_tiles=3))
    assert tiles == 2 and np.array_equal(one.read_tile_frames(), np.where(capped == 1, 4, 1))
    one.close()


# ---- 3. a refined tile holds a plain render's bits -----------------------------------------------------------

def test_refined_tiles_hold_the_bits_of_a_plain_render(gpu):
    w = h = 32
    a, b = scene_of(6, w, h, 0), scene_of(6, w, h, 1)
    rf = rtamd.frame_rand_factors(1, 0, 4)
    ctx = at_a(a)
    _, tiles = ctx.render_moved(b.camera, rf, keep_float=True, refine=dict(extra_frames=3))
    tf = ctx.read_tile_frames()
    assert sorted(set(tf.tolist())) == [1, 4] and (tf == 4).sum() == tiles
    plain = context(b)
    plain.set_moments(True)
    plain.render(1, rf[:1])
    img1, m1 = plain.read_image(), plain.read_moments()
    plain.render(1, rf)
    img4, m4 = plain.read_image(), plain.read_moments()
    plain.close()
    refined = per_pixel(tf, w, h) == 4
    img, m2 = ctx.read_image(), ctx.read_moments()
    for got, four, one in ((img, img4, img1), (m2, m4, m1)):
        assert bit_equal(got[refined], four[refined]), mismatch_report(got[refined], four[refined])
        assert bit_equal(got[~refined], one[~refined]), mismatch_report(got[~refined], one[~refined])
    assert not bit_equal(img4[refined], img1[refined])                       # the extra frames did change those tiles
    # the second reproject saw the refined counts: a pixel the history does not reach holds its tile's 4 frames
    rp = ctx.read_reprojected()
    n_t = per_pixel(tf, w, h).astype(F)
    fresh = rp[..., 3] <= n_t
    assert (fresh & refined).any() and (rp[..., 3][fresh & refined] == 4).all()
    assert not (fresh & ~refined).any()                                      # every tile with a short pixel was refined
    assert (rp[..., 3][~fresh] > n_t[~fresh]).all()
    # ... and the frame takes the filtered buffer exactly there
    flt = ctx.read_presented_float()
    assert np.array_equal(flt[..., 3] == 1, fresh) and np.array_equal(flt[..., 3] == 0, ~fresh)
    den = read_denoised(ctx)
    assert bit_equal(flt[fresh][:, :3], den[fresh][:, :3]) and bit_equal(flt[~fresh][:, :3], rp[~fresh][:, :3])
    ctx.close()


# ---- 4. one call against the public calls one by one ---------------------------------------------------------

@pytest.mark.parametrize("variance", [True, False], ids=["variance_on", "variance_off"])
def test_render_moved_refined_is_the_public_calls_one_by_one(gpu, variance):
    sid, w, h = 6, 32, 32
    a = scene_of(sid, w, h, 0)
    one, steps = at_a(a, variance), at_a(a, variance)
    source = "moved" if variance else "reprojected"
    poses = [(scene_of(sid, w, h, 1), 1, "image", dict(extra_frames=3)),
             (scene_of(sid, w, h, 2), 2, "reprojected", dict(extra_frames=1, min_pixels=4)),
             (scene_of(sid, w, h, 3), 1, "reprojected", dict(extra_frames=2, min_count=2.5, max_tiles=3))]
    refined_any = 0
    for pose, (scene, n, hist, refine) in enumerate(poses):
        k = refine["extra_frames"]
        rf = rtamd.frame_rand_factors(1, 10 * pose, n + k)
        got8, tiles = one.render_moved(scene.camera, rf, keep_float=True, exposure=0.5, refine=refine)
        gotf = one.read_presented_float()
        steps.history_capture(hist)
        steps.set_camera(scene.camera)
        steps.render(1, rf[:n])
        steps.render_features()
        steps.reproject()
        steps.reach_tiles(refine.get("min_count") or float(n + k))
        reach = steps.read_tile_reach()
        sel = rtamd.refine_select(reach, refine.get("min_pixels", 1), refine.get("max_tiles", 0))
        if sel.any():
            steps.set_active_tiles(None if sel.all() else sel)
            steps.render(n + 1, rf[n:])
            steps.set_active_tiles(None)
            steps.reproject()
        if variance:
            steps.denoise_reprojected()
        ref8 = steps.present(source, exposure=0.5, keep_float=True)
        reff = steps.read_presented_float()
        assert tiles == int(sel.sum()), (pose, tiles, sel)
        refined_any += tiles
        assert np.array_equal(got8, ref8), (pose, np.argwhere(got8 != ref8)[:4])
        assert bit_equal(gotf, reff), (pose, mismatch_report(gotf, reff))
        assert bit_equal(one.read_reprojected(), steps.read_reprojected()), pose
        if variance:
            assert bit_equal(one.read_reprojected_variance(), steps.read_reprojected_variance()), pose
            assert bit_equal(read_denoised(one), read_denoised(steps)), pose
        assert np.array_equal(one.read_tile_frames(), steps.read_tile_frames()), pose
        assert np.array_equal(one.read_tile_frames(), np.where(sel == 1, n + k, n)), pose
        va, vb = view(one, scene.camera), view(steps, scene.camera)
        for key in ("image", "m2", "nd", "ai"):
            assert bit_equal(va[key], vb[key]), (pose, key)
    assert refined_any > 0
    for ctx in (one, steps):
        ctx.close()


# ---- 5. no refinement is rt_render_moved ---------------------------------------------------------------------

def raw_refined(ctx, camera, rf, n, refine=None, tiles=None):
    cam = np.ascontiguousarray(camera, F).ravel()
    rf = np.ascontiguousarray(rf, F)
    ctx._check(ctx._L.rt_render_moved_refined(ctx._h, cam.ctypes.data_as(_lib.c_float_p), int(n), rf.ctypes.data_as(_lib.c_float_p),
                                              None if refine is None else ctypes.byref(refine), None, None, None, None,
                                              None if tiles is None else ctypes.byref(tiles)))
    return ctx.read_presented()


def test_no_refinement_is_render_moved(gpu):
    sid, w, h = 6, 32, 32
    a = scene_of(sid, w, h, 0)
    plain, null, zero, pyz = at_a(a), at_a(a), at_a(a), at_a(a)
    for pose, n in ((1, 1), (2, 2)):
        scene = scene_of(sid, w, h, pose)
        rf = rtamd.frame_rand_factors(1, 0, n)
        ref = plain.render_moved(scene.camera, rf)
        tiles = ctypes.c_int(-1)
        assert np.array_equal(raw_refined(null, scene.camera, rf, n, None, tiles), ref) and tiles.value == 0
        p = _lib.RtRefineParams()
        p.min_count, p.min_pixels, p.max_tiles = 3.0, 2, 5               # set, and unused: extra_frames is 0
        assert np.array_equal(raw_refined(zero, scene.camera, rf, n, p), ref)
        frame, t = pyz.render_moved(scene.camera, rf, refine=dict(extra_frames=0, max_tiles=2))
        assert np.array_equal(frame, ref) and t == 0
        for ctx in (null, zero, pyz):
            assert bit_equal(ctx.read_reprojected(), plain.read_reprojected()), pose
            assert bit_equal(ctx.read_reprojected_variance(), plain.read_reprojected_variance()), pose
            assert bit_equal(read_denoised(ctx), read_denoised(plain)), pose
            assert bit_equal(ctx.read_image(), plain.read_image()) and bit_equal(ctx.read_moments(), plain.read_moments())
            assert ctx.read_tile_frames().tolist() == plain.read_tile_frames().tolist() == [n] * 16
            rt_err(-3, ctx.read_tile_reach, "rt_reach_tiles")            # no record was made
    for ctx in (plain, null, zero, pyz):
        ctx.close()


# ---- 6. nothing else moves -----------------------------------------------------------------------------------

def test_everything_else_keeps_its_bits(gpu):
    case = (6, 32, 32)

    def run(reaching):
        ctx, b = moved_to_b(case, frames_b=2)
        frame = ctx.present("moved", exposure=0.5, keep_float=True)
        before = held(ctx)
        if reaching:
            for mc in MIN_COUNTS:
                ctx.reach_tiles(mc)
                assert ctx.read_tile_reach().shape == (16,)
            after = held(ctx)
            for k in ("image", "m2", "nd", "ai", "rp", "s2", "den"):
                assert bit_equal(before[k], after[k]), (k, mismatch_report(before[k], after[k]))
            assert list(before["tf"]) == list(after["tf"])
            assert np.array_equal(ctx.read_presented(), frame)               # the frame held, and what it binds to
            assert np.array_equal(ctx.present("moved", exposure=0.5, keep_float=True), frame)
            ctx.history_capture("reprojected")                               # the history takes the same result
        else:
            ctx.history_capture("reprojected")
        flt = ctx.read_presented_float()
        render(ctx, 3, 2)                                                    # later frames
        ctx.reproject()
        out = dict(image=ctx.read_image(), m2=ctx.read_moments(), tf=list(ctx.read_tile_frames()), last=ctx.last_launch(),
                   rp=ctx.read_reprojected(), flt=flt, den=ctx.denoise(guides=True))
        ctx.close()
        return out

    yes, no = run(True), run(False)
    for k in ("image", "m2", "rp", "flt", "den"):
        assert bit_equal(yes[k], no[k]), (k, mismatch_report(yes[k], no[k]))
    assert yes["tf"] == no["tf"] == [4] * 16 and yes["last"] == no["last"]


# ---- 7. state and arguments ----------------------------------------------------------------------------------

def refine_params(min_count=0.0, extra_frames=1, min_pixels=0, max_tiles=0, reserved=()):
    p = _lib.RtRefineParams()
    p.min_count, p.extra_frames, p.min_pixels, p.max_tiles = min_count, extra_frames, min_pixels, max_tiles
    for i, r in enumerate(reserved):
        p.reserved[i] = r
    return p


def test_state_rules(gpu):
    scene, b = scene_of(6, 32, 32, 0), scene_of(6, 32, 32, 1)
    rf = rtamd.frame_rand_factors(1, 0, 4)
    two = rtamd.RenderContext(devices=(0, 0))
    two.upload_scene(scene)
    two.resize(32, 32)
    rt_err(-3, lambda: two.reach_tiles(4.0), "1-device")                    # a two-slot context
    rt_err(-3, two.read_tile_reach, "1-device")
    rt_err(-3, lambda: raw_refined(two, b.camera, rf, 1, refine_params(extra_frames=3)), "1-device")
    two.close()
    part = rtamd.RenderContext(rank=0, world=2, stripe_rows=8)
    part.upload_scene(scene)
    part.resize(32, 32)
    rt_err(-3, lambda: part.reach_tiles(4.0), "rt_set_partition")           # a partition
    rt_err(-3, part.read_tile_reach, "rt_set_partition")
    rt_err(-3, lambda: raw_refined(part, b.camera, rf, 1, refine_params(extra_frames=3)), "rt_set_partition")
    part.close()
    bare = rtamd.RenderContext()
    rt_err(-3, lambda: bare.reach_tiles(4.0), "no image")                   # no rt_resize yet
    bare.close()

    ctx = at_a(scene)
    rt_err(-3, lambda: ctx.reach_tiles(4.0), "rt_reproject")                # no result held
    rt_err(-3, ctx.read_tile_reach, "rt_reach_tiles")
    for mc in (0.0, -1.0, float("nan"), float("inf")):
        rt_err(-1, lambda: ctx.reach_tiles(mc), "min_count")
    # bad parameters: RT_ERR_INVALID_ARG before anything is queued, the counts untouched
    for bad in (dict(extra_frames=-1), dict(min_pixels=65), dict(min_pixels=-1), dict(max_tiles=-1), dict(min_count=-1.0),
                dict(min_count=float("nan")), dict(min_count=float("inf")), dict(reserved=(1,)), dict(reserved=(0, 0, 0, 2))):
        rt_err(-1, lambda: raw_refined(ctx, b.camera, rf, 1, refine_params(**bad)), "rt_render_moved_refined")
    assert ctx.read_tile_frames().tolist() == [8] * 16
    # a caller mask set on entry
    mask = np.zeros(16, np.uint8)
    mask[3] = 1
    ctx.set_active_tiles(mask)
    rt_err(-3, lambda: raw_refined(ctx, b.camera, rf, 1, refine_params(extra_frames=3)), "tile mask")
    ctx.set_active_tiles(None)
    assert ctx.read_tile_frames().tolist() == [8] * 16
    # a refined pose: min_pixels 0 means 1; no mask is left, a render from frame 1 samples every tile
    tiles = ctypes.c_int(-1)
    raw_refined(ctx, b.camera, rf, 1, refine_params(extra_frames=3), tiles)
    assert 0 < tiles.value < 16 and sorted(set(ctx.read_tile_frames().tolist())) == [1, 4]
    render(ctx, 1, 1)
    assert ctx.read_tile_frames().tolist() == [1] * 16 and ctx.last_launch()["tiles_active"] == 16
    # a step's refusal comes back unchanged, and no mask is left: back to A, where the history reaches a part of
    # the view (2 frames there, 1 elsewhere), with a rand factor that the masked render refuses
    ctx.render_features()
    bad_rf = np.array([0.5, 2048.0, 0.5, 0.5], F)
    rt_err(-1, lambda: raw_refined(ctx, scene.camera, bad_rf, 1, refine_params(min_count=1.5, extra_frames=3)))
    sel = rtamd.refine_select(ctx.read_tile_reach())                        # the records of the pose that was refused
    assert 0 < sel.sum() < 16
    render(ctx, 1, 1)
    assert ctx.read_tile_frames().tolist() == [1] * 16 and ctx.last_launch()["tiles_active"] == 16
    ctx.close()

    # the records: a short cap, and a new rt_reproject drops them
    ctx, _ = moved_to_b((6, 32, 32))
    ctx.reach_tiles(4.0)
    n = ctypes.c_int()
    ctx._check(ctx._L.rt_read_tile_reach(ctx._h, None, 0, ctypes.byref(n)))
    assert n.value == 16
    out = np.zeros(16, rtamd.TILE_REACH_DTYPE)
    rt_err(-4, lambda: ctx._check(ctx._L.rt_read_tile_reach(ctx._h, out.ctypes.data_as(ctypes.POINTER(_lib.RtTileReach)), 15,
                                                            ctypes.byref(n))), "too small")
    first = ctx.read_tile_reach()
    ctx.reproject()
    rt_err(-3, ctx.read_tile_reach, "rt_reach_tiles")
    ctx.reach_tiles(4.0)
    assert same_records(ctx.read_tile_reach(), first)
    ctx.set_history_variance(False)                                          # the result dropped: so are its records
    rt_err(-3, ctx.read_tile_reach, "rt_reach_tiles")
    rt_err(-3, lambda: ctx.reach_tiles(4.0), "rt_reproject")
    ctx.set_history_variance(True)
    ctx.history_capture()
    ctx.reproject()
    ctx.reach_tiles(4.0)
    ctx.resize(32, 32)                                                       # rt_resize frees everything
    rt_err(-3, ctx.read_tile_reach, "rt_reach_tiles")
    rt_err(-3, lambda: ctx.reach_tiles(4.0), "rt_reproject")
    ctx.close()

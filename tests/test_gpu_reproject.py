"""Temporal reprojection on the device (rt.h rt_history_capture / rt_reproject / rt_read_reprojected;
rt_reproject.hip) against rt_reproject_host bit for bit, the state rules of the history and the result, that
nothing else in the context moves, and the recorded quality experiment.  Renders are depth 5, seed 1.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import rtamd
from rtamd import _lib
from helpers import bit_equal, mismatch_report

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SEED = 1
MISS = 0xFFFFFFFF
SHIFT = 0.25   # a camera move: this share of the viewport's width along pixel_delta_u (tools/reproject_quality.py's)
CASES = [(6, 32, 32), (8, 13, 9), (0, 32, 18)]   # 13x9: partial tiles in both directions


@functools.lru_cache(maxsize=None)
def scene_of(sid, w, h, moves=0):
    """The scene seen after `moves` camera moves: camera_pos and up_left shifted by the same vector."""
    scene = rtamd.Scene(sid, w, h, seed=SEED)
    if moves:
        cam = scene.camera.copy()
        v = cam[12:15] * F(SHIFT * w * moves)
        cam[4:7] += v
        cam[8:11] += v
        scene.override_camera(cam)
    return scene


def context(scene, spp=16, **kw):
    ctx = rtamd.RenderContext(**kw)
    ctx.upload_scene(scene)
    ctx.set_params(max_depth=5, spp=spp)
    ctx.resize(scene.width, scene.height)
    return ctx


def render(ctx, first, n, seed=SEED):
    ctx.render(first, rtamd.frame_rand_factors(seed, first - 1, n))


def rt_err(code, fn, names=None):
    with pytest.raises(rtamd.RTError) as e:
        fn()
    assert e.value.code == code, e.value
    if names:
        assert names in str(e.value), e.value


def view(ctx, cam):
    """What the host path needs of the current view."""
    nd, ai = ctx.read_features_raw()
    return dict(image=ctx.read_image(), tf=ctx.read_tile_frames(), nd=nd, ai=ai, cam=np.array(cam, F))


def host(hist, hv, cv, **prm):
    return rtamd.reproject_host(hist, hv["nd"], hv["ai"], hv["cam"], cv["image"], cv["tf"], cv["nd"], cv["ai"], cv["cam"], **prm)


def counts_px(tf, w, h):
    tx, ty = (w + 7) // 8, (h + 7) // 8
    return np.repeat(np.repeat(np.asarray(tf).reshape(ty, tx), 8, axis=0), 8, axis=1)[:h, :w].astype(F)


def rejected_share(out, cv):
    """The share of hit pixels whose count did not grow."""
    h, w = out.shape[:2]
    hit = np.ascontiguousarray(cv["ai"]).view(np.uint32)[..., 3] != MISS
    return float((out[..., 3][hit] <= counts_px(cv["tf"], w, h)[hit]).mean())


def move_to(ctx, scene, first=1, n=2):
    ctx.set_camera(scene.camera)
    render(ctx, first, n)
    ctx.render_features()


# ---- 1. the device against the host reference ---------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=lambda c: f"scene{c[0]}_{c[1]}x{c[2]}")
def test_device_matches_the_host_and_a_chain_of_moves(gpu, case):
    sid, w, h = case
    a, b, c = (scene_of(sid, w, h, k) for k in (0, 1, 2))
    ctx = context(a)
    ctx.set_moments(True)
    render(ctx, 1, 8)
    ctx.render_features()
    va = view(ctx, a.camera)
    ctx.history_capture()
    move_to(ctx, b)                                      # the history survives rt_set_camera and the render
    ctx.reproject()
    got = ctx.read_reprojected()
    vb = view(ctx, b.camera)
    assert list(va["tf"]) == [8] * len(va["tf"]) and list(vb["tf"]) == [2] * len(vb["tf"])
    ref = host(rtamd.history_from_image(va["image"], va["tf"]), va, vb)
    assert bit_equal(got, ref), mismatch_report(got, ref)
    share = rejected_share(got, vb)
    print(f"scene {sid} {w}x{h}: rejected share of hit pixels {share:.3f}")
    assert share < 0.5
    assert (got[..., 3] > 2.0).any() and not bit_equal(got[..., :3], vb["image"][..., :3])
    # other parameters, the depth test off among them
    for prm in (dict(kz=0.0), dict(cos_min=0.99, kz=0.02, max_history=4.0)):
        ctx.reproject(**prm)
        out = ctx.read_reprojected()
        exp = host(rtamd.history_from_image(va["image"], va["tf"]), va, vb, **prm)
        assert bit_equal(out, exp), (prm, mismatch_report(out, exp))
    # the chain: the result becomes the history, the camera moves again with one frame
    ctx.reproject()
    ctx.history_capture("reprojected")
    move_to(ctx, c, n=1)
    ctx.reproject()
    got2 = ctx.read_reprojected()
    vc = view(ctx, c.camera)
    ref2 = host(ref, vb, vc)
    assert bit_equal(got2, ref2), mismatch_report(got2, ref2)
    assert (got2[..., 3] > 3.0).any()                    # counts carried over two moves: 1 + (2 + 8)
    # nothing of the view was written
    again = view(ctx, c.camera)
    assert all(bit_equal(again[k], vc[k]) for k in ("image", "nd", "ai")) and list(again["tf"]) == list(vc["tf"])
    ctx.close()


def test_unequal_tile_counts(gpu):
    sid, w, h = 0, 32, 18
    a, b = scene_of(sid, w, h, 0), scene_of(sid, w, h, 1)
    nt = 4 * 3
    ctx = context(a)
    ctx.set_moments(True)
    render(ctx, 1, 4)
    ctx.set_active_tiles(np.arange(nt) % 2)              # every other tile goes on to 8 frames
    render(ctx, 5, 4)
    ctx.set_active_tiles(None)
    ctx.render_features()
    va = view(ctx, a.camera)
    assert sorted(set(va["tf"].tolist())) == [4, 8]
    ctx.history_capture()
    ctx.set_camera(b.camera)
    render(ctx, 1, 1)
    ctx.set_active_tiles((np.arange(nt) % 3 == 0))
    render(ctx, 2, 2)
    ctx.set_active_tiles(None)
    ctx.render_features()
    ctx.reproject()
    got = ctx.read_reprojected()
    vb = view(ctx, b.camera)
    assert sorted(set(vb["tf"].tolist())) == [1, 3]
    hist = rtamd.history_from_image(va["image"], va["tf"])
    assert sorted(set(hist[..., 3].ravel().tolist())) == [4.0, 8.0]
    ref = host(hist, va, vb)
    assert bit_equal(got, ref), mismatch_report(got, ref)
    grown = got[..., 3] > counts_px(vb["tf"], w, h)
    assert grown.any() and (got[..., 3][grown] <= counts_px(vb["tf"], w, h)[grown] + 8.0 + 1e-4).all()
    ctx.close()


# ---- 2. state ----------------------------------------------------------------------------------------

def test_state_rules(gpu):
    scene, moved = scene_of(6, 32, 32, 0), scene_of(6, 32, 32, 1)
    ctx = rtamd.RenderContext()
    ctx.upload_scene(scene)
    rt_err(-3, ctx.history_capture, "rt_resize")                          # no image
    rt_err(-3, ctx.reproject, "rt_resize")
    rt_err(-3, ctx.read_reprojected, "rt_reproject")
    ctx.close()
    two = rtamd.RenderContext(devices=(0, 0))
    two.upload_scene(scene)
    two.resize(32, 32)
    rt_err(-3, two.history_capture)                                       # a two-slot context
    rt_err(-3, two.reproject)
    two.close()
    part = rtamd.RenderContext(rank=0, world=2, stripe_rows=8)
    part.upload_scene(scene)
    part.resize(32, 32)
    rt_err(-3, part.history_capture, "rt_set_partition")                  # a partition
    rt_err(-3, part.reproject, "rt_set_partition")
    part.close()

    ctx = context(scene)
    render(ctx, 1, 4)
    ctx.render_features()
    rt_err(-3, ctx.history_capture, "rt_set_moments")                     # the moments are off
    ctx.set_moments(True)
    rt_err(-3, ctx.history_capture, "rt_render")                          # on, but no tile holds a frame
    render(ctx, 1, 4)
    ctx.set_camera(scene.camera)
    rt_err(-3, ctx.history_capture, "rt_render_features")                 # stale features
    ctx.render_features()
    rt_err(-3, lambda: ctx.history_capture("reprojected"), "rt_reproject")   # no result to take
    rt_err(-3, ctx.reproject, "rt_history_capture")                       # no history
    rt_err(-1, lambda: ctx.history_capture(2))
    ctx.history_capture()
    ctx.reproject()
    same_view = ctx.read_reprojected()
    # bad parameters: RT_ERR_INVALID_ARG, the result stays
    for bad in (dict(cos_min=1.5), dict(kz=-1.0), dict(kz=float("nan")), dict(max_history=0.0), dict(max_history=float("inf"))):
        rt_err(-1, lambda: ctx.reproject(**bad))
    rp = _lib.RtReprojectParams()
    rp.cos_min, rp.kz, rp.max_history = 0.9, 0.1, 64.0
    rp.reserved[2] = 1
    assert ctx._L.rt_reproject(ctx._h, ctypes.byref(rp)) == -1
    assert bit_equal(ctx.read_reprojected(), same_view)
    # the history survives rt_set_camera, rt_set_params, rt_set_bvh_mode and later renders; the features do not
    ctx.set_camera(moved.camera)
    rt_err(-3, ctx.reproject, "rt_render_features")
    rt_err(-3, lambda: ctx.history_capture("reprojected"), "rt_render_features")
    ctx.set_params(background=(0.25, 0.5, 0.75))
    ctx.set_bvh_mode(1)
    ctx.set_bvh_mode(0)
    render(ctx, 1, 2)
    ctx.render_features()
    ctx.reproject()
    assert (ctx.read_reprojected()[..., 3] > 2.0).any()
    ctx.set_moments(False)
    rt_err(-3, ctx.reproject, "rt_set_moments")
    ctx.set_moments(True)
    render(ctx, 1, 2)
    ctx.reproject()
    held = ctx.read_reprojected()
    # rt_upload_texture and rt_upload_buffer drop the history (the result stays readable)
    data = scene.buffers[2]
    assert ctx._L.rt_upload_buffer(ctx._h, 2, ctypes.create_string_buffer(data, len(data)), len(data)) == 0
    ctx.render_features()
    rt_err(-3, ctx.reproject, "rt_history_capture")
    assert bit_equal(ctx.read_reprojected(), held)
    ctx.history_capture()
    ctx.reproject()
    t = scene.textures[0]
    assert ctx._L.rt_upload_texture(ctx._h, t.slot, t.format, t.width, t.height, ctypes.create_string_buffer(t.data, len(t.data))) == 0
    ctx.render_features()
    rt_err(-3, ctx.reproject, "rt_history_capture")
    # rt_resize frees the history and the result
    ctx.history_capture()
    ctx.reproject()
    ctx.resize(32, 32)
    rt_err(-3, ctx.read_reprojected, "rt_reproject")
    ctx.set_camera(scene.camera)
    render(ctx, 1, 2)
    ctx.render_features()
    rt_err(-3, ctx.reproject, "rt_history_capture")
    ctx.close()


def test_nothing_else_moves(gpu):
    a, b = scene_of(6, 32, 32, 0), scene_of(6, 32, 32, 1)

    def run(with_reprojection):
        ctx = context(a)
        ctx.set_moments(True)
        render(ctx, 1, 4)
        ctx.render_features()
        launch = ctx.last_launch()
        if with_reprojection:
            ctx.history_capture()
        first = ctx.denoise(guides=True)
        ctx.set_camera(b.camera)
        render(ctx, 1, 2)
        ctx.render_features()
        if with_reprojection:
            ctx.reproject()
            ctx.history_capture("reprojected")
        render(ctx, 3, 2)
        if with_reprojection:
            ctx.reproject()
        den = ctx.denoise(guides=True)
        if with_reprojection:
            ctx.history_capture()
            ctx.reproject(kz=0.0)
            assert (ctx.read_reprojected()[..., 3] > 4.0).any()
        nd, ai = ctx.read_features_raw()
        out = dict(image=ctx.read_image(), m2=ctx.read_moments(), frames=list(ctx.read_tile_frames()), nd=nd, ai=ai,
                   first=first, den=den, launch=launch, last=ctx.last_launch())
        ctx.close()
        return out

    x, y = run(True), run(False)
    assert x["frames"] == y["frames"] == [4] * 16
    for k in ("image", "m2", "nd", "ai", "first", "den"):
        assert bit_equal(x[k], y[k]), (k, mismatch_report(x[k], y[k]))
    assert x["launch"] == y["launch"] and x["last"] == y["last"]   # the same launches, with the same buffers behind them


# ---- 3. the recorded experiment ------------------------------------------------------------------------

def rms_y(a, b):
    ya, yb = [(v[..., 0].astype(np.float64) + v[..., 1]) + v[..., 2] for v in (a, b)]
    d = ya - yb
    return float(np.sqrt(np.mean(d[np.isfinite(d)] ** 2)))


def test_quality_after_a_move(gpu):
    """tools/reproject_quality.py's experiment on the device with the default parameters: the reprojected image's
    RMS error of y against a long render at the new camera is at most the raw image's times
    min(1, 2 x the ratio the CPU run recorded); the factor 2 covers the different random frames."""
    rec = json.load(open(os.path.join(REPO, "profiles", "reproject_quality.json")))
    assert rec["library_defaults_are_the_best"]
    d = rec["defaults"]
    assert (d["cos_min"], d["kz"], d["max_history"]) == rtamd.render.REPROJECT_DEFAULTS
    sid, w, h = rec["scene"], rec["width"], rec["height"]
    assert (sid, w, h, rec["frames_a"], rec["frames_b"], rec["ref_frames"], rec["shift"]) == (6, 32, 32, 64, 2, 1024, SHIFT)
    a, b = scene_of(sid, w, h, 0), scene_of(sid, w, h, 1)
    ref_ctx = context(b, 1024)
    render(ref_ctx, 1, 1024, seed=rec["ref_seed"])
    ref = ref_ctx.read_image()
    ref_ctx.close()
    ctx = context(a, 64)
    ctx.set_moments(True)
    render(ctx, 1, 64)
    ctx.render_features()
    ctx.history_capture()
    ctx.set_params(spp=2)
    move_to(ctx, b, n=2)
    ctx.reproject()
    out, raw = ctx.read_reprojected(), ctx.read_image()
    ctx.reproject(d["cos_min"], d["kz"], d["max_history"])
    assert bit_equal(ctx.read_reprojected(), out)                     # NULL params are the recorded defaults
    ctx.close()
    e_raw, e_out = rms_y(raw, ref), rms_y(out, ref)
    bound = min(1.0, 2.0 * rec["ratio_at_defaults"])
    print(f"scene {sid} {w}x{h}: RMS y raw {e_raw:.4f}, reprojected {e_out:.4f}, ratio {e_out / e_raw:.4f} "
          f"(CPU: {rec['ratio_at_defaults']}, bound {bound:.4f})")
    assert e_out <= e_raw * bound

"""The variance carried through reprojection and the preview filter over the reprojected view on the device
(rt.h rt_set_history_variance / rt_read_reprojected_variance / rt_denoise_reprojected; rt_reproject.hip,
rt_denoise.hip) against the host references bit for bit, the switch on against off, the state rules, and the
recorded quality experiment.  Renders are depth 5, seed 1.
"""
import functools
import json
import os

import numpy as np
import pytest

import rtamd
from helpers import bit_equal, mismatch_report
import reproject_var_ref as V

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SEED = 1
MISS = 0xFFFFFFFF
SHIFT = 0.25   # a camera move: this share of the viewport's width along pixel_delta_u (tools/reproject_quality.py's)
# 13x9: partial tiles in both directions; 70 crosses the filter's 64-wide workgroup, 11 is below step-4 reach
CASES = [(6, 32, 32), (8, 13, 9), (0, 70, 11)]
ZERO = (0.0, 0.0, 0.0)


@functools.lru_cache(maxsize=None)
def scene_of(sid, w, h, moves=0):
    scene = rtamd.Scene(sid, w, h, seed=SEED)
    if moves:
        cam = scene.camera.copy()
        v = cam[12:15] * F(SHIFT * w * moves)
        cam[4:7] += v
        cam[8:11] += v
        scene.override_camera(cam)
    return scene


def context(scene, spp=16, variance=True, **kw):
    ctx = rtamd.RenderContext(**kw)
    ctx.upload_scene(scene)
    ctx.set_params(max_depth=5, spp=spp)
    ctx.resize(scene.width, scene.height)
    if variance:
        ctx.set_history_variance(True)
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
    return dict(image=ctx.read_image(), m2=ctx.read_moments(), tf=ctx.read_tile_frames(), nd=nd, ai=ai, cam=np.array(cam, F))


def move_to(ctx, scene, first=1, n=1):
    ctx.set_camera(scene.camera)
    render(ctx, first, n)
    ctx.render_features()


def host(hist, hs2, hv, cv):
    return rtamd.reproject_variance_host(hist, hv["nd"], hv["ai"], hs2, hv["cam"], cv["image"], cv["m2"], cv["tf"], cv["nd"],
                                         cv["ai"], cv["cam"])


def compare(ctx, hist, hs2, hv, cv, tag):
    """The device's result word, s2 and filtered buffers against the host's -> (rgbn, s2, info, level-0 classes)."""
    ref, ref_s2 = host(hist, hs2, hv, cv)
    got, got_s2 = ctx.read_reprojected(), ctx.read_reprojected_variance()
    assert bit_equal(got, ref), (tag, mismatch_report(got, ref))
    assert bit_equal(got_s2, ref_s2), (tag, mismatch_report(got_s2, ref_s2))
    for guides in (True, ZERO):
        out = ctx.denoise_reprojected(guides=guides)
        exp = rtamd.denoise_reprojected_host(ref, ref_s2, cv["nd"], cv["ai"], guides=guides)
        assert bit_equal(out, exp), (tag, guides, mismatch_report(out, exp))
    assert bit_equal(ctx.denoise_reprojected(guides=ZERO), ctx.denoise_reprojected(guides=None))
    out = ctx.denoise_reprojected(levels=5, k=1.5, guides=(2.0, 0.5, 0.25))
    exp = rtamd.denoise_reprojected_host(ref, ref_s2, cv["nd"], cv["ai"], levels=5, k=1.5, guides=(2.0, 0.5, 0.25))
    assert bit_equal(out, exp), (tag, mismatch_report(out, exp))
    _, _, info = V.reproject(hist, hv["nd"], hv["ai"], hs2, hv["cam"], cv["image"], cv["m2"], cv["tf"], cv["nd"], cv["ai"],
                             cv["cam"], cos_min=0.9, kz=0.1, max_history=64.0)
    _, cls = V.level0(ref, ref_s2, cv["ai"])
    return ref, ref_s2, info, cls


# ---- 1. the device against the host references --------------------------------------------------------

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
    hist = rtamd.history_from_image(va["image"], va["tf"])
    hs2 = rtamd.history_variance_host(va["image"], va["m2"], va["tf"])
    assert (hs2 >= 0).any()
    # one frame at B: a pixel's own variance is unknown, the history's is what it has
    move_to(ctx, b, n=1)
    ctx.reproject()
    vb1 = view(ctx, b.camera)
    assert set(vb1["tf"].tolist()) == {1}
    r1, s1, info1, cls1 = compare(ctx, hist, hs2, va, vb1, "one frame at B")
    own1 = info1["s2_c"] >= 0
    assert not own1.any()
    assert ((cls1 == V.KNOWN) & (info1["rule"] != V.OWN)).any()      # known from the history
    assert (cls1 == V.SPATIAL).any()                                 # the spatial fallback, on the fresh pixels
    assert ((cls1 == V.SPATIAL) == ~(s1 >= 0)).all() and (cls1 != V.BAD).all()
    # two frames at B: the fresh pixels know their own
    render(ctx, 2, 1)
    ctx.reproject()
    vb2 = view(ctx, b.camera)
    assert set(vb2["tf"].tolist()) == {2}
    r2, s2, info2, cls2 = compare(ctx, hist, hs2, va, vb2, "two frames at B")
    assert ((cls2 == V.KNOWN) & (info2["rule"] == V.OWN) & (info2["s2_c"] >= 0)).any()   # known from the pixel's own moments
    assert ((info2["rule"] == V.BLEND) & (info2["s2_c"] >= 0) & (info2["s2_hist"] >= 0)).any()
    # the chain: the one-frame result becomes the history (its fresh pixels carry no variance), the camera moves again
    render(ctx, 1, 1)
    ctx.reproject()
    assert bit_equal(ctx.read_reprojected(), r1) and bit_equal(ctx.read_reprojected_variance(), s1)
    ctx.history_capture("reprojected")
    move_to(ctx, c, n=1)
    ctx.reproject()
    vc = view(ctx, c.camera)
    r3, s3, info3, cls3 = compare(ctx, r1, s1, vb1, vc, "second move")
    assert info3["tap_unknown"].any()                                # an accepted tap whose history s2 is unknown
    assert (r3[..., 3] > 2.0).any() and (cls3 == V.KNOWN).any() and (cls3 == V.SPATIAL).any()
    # nothing of the view was written
    again = view(ctx, c.camera)
    assert all(bit_equal(again[k], vc[k]) for k in ("image", "m2", "nd", "ai")) and list(again["tf"]) == list(vc["tf"])
    ctx.close()


# ---- 2. the switch on against off ---------------------------------------------------------------------

def test_switch_on_leaves_everything_else_as_it_was(gpu):
    a, b = scene_of(6, 32, 32, 0), scene_of(6, 32, 32, 1)

    def run(mode):
        """mode: "on", "off" (reprojection without the variance) or None (a context that calls none of it)."""
        ctx = context(a, variance=mode == "on")
        ctx.set_moments(True)
        render(ctx, 1, 4)
        ctx.render_features()
        launch = ctx.last_launch()
        out = {}
        if mode:
            ctx.history_capture()
        ctx.set_camera(b.camera)
        render(ctx, 1, 2)
        ctx.render_features()
        if mode:
            ctx.reproject()
            out["rp"] = ctx.read_reprojected()
            before = view(ctx, b.camera)
            if mode == "on":
                out["s2"] = ctx.read_reprojected_variance()
                out["filtered"] = ctx.denoise_reprojected()
                assert not bit_equal(out["filtered"][..., :3], out["rp"][..., :3])
            ctx.history_capture("reprojected")
            ctx.reproject()
            after = view(ctx, b.camera)
            assert all(bit_equal(before[k], after[k]) for k in ("image", "m2", "nd", "ai")) and list(before["tf"]) == list(after["tf"])
            out["rp_chain"] = ctx.read_reprojected()
        den = ctx.denoise(guides=True)                                   # rt_denoise_guided over the image, as ever
        render(ctx, 3, 2)                                                # later frames
        nd, ai = ctx.read_features_raw()
        out.update(image=ctx.read_image(), m2=ctx.read_moments(), frames=list(ctx.read_tile_frames()), nd=nd, ai=ai, den=den,
                   launch=launch, last=ctx.last_launch())
        ctx.close()
        return out

    on, off, never = run("on"), run("off"), run(None)
    assert bit_equal(on["rp"], off["rp"]), mismatch_report(on["rp"], off["rp"])   # the result word is the switch-off one
    assert bit_equal(on["rp_chain"], off["rp_chain"]) and (on["rp_chain"][..., 3] > on["rp"][..., 3]).any()
    assert (on["s2"] >= 0).any()
    assert on["frames"] == off["frames"] == never["frames"] == [4] * 16
    for k in ("image", "m2", "nd", "ai", "den"):
        assert bit_equal(on[k], never[k]), (k, mismatch_report(on[k], never[k]))
        assert bit_equal(off[k], never[k]), (k, mismatch_report(off[k], never[k]))
    assert on["launch"] == off["launch"] == never["launch"] and on["last"] == off["last"] == never["last"]


# ---- 3. state ------------------------------------------------------------------------------------------

def test_state_rules(gpu):
    scene, moved = scene_of(6, 32, 32, 0), scene_of(6, 32, 32, 1)
    two = rtamd.RenderContext(devices=(0, 0))
    two.upload_scene(scene)
    two.resize(32, 32)
    two.set_history_variance(True)
    rt_err(-3, two.denoise_reprojected, "1-device")                       # a two-slot context
    rt_err(-3, two.read_reprojected_variance)
    two.close()
    part = rtamd.RenderContext(rank=0, world=2, stripe_rows=8)
    part.upload_scene(scene)
    part.resize(32, 32)
    part.set_history_variance(True)
    rt_err(-3, part.denoise_reprojected, "rt_set_partition")              # a partition
    part.close()

    ctx = context(scene, variance=False)
    ctx.set_moments(True)
    render(ctx, 1, 4)
    ctx.render_features()
    # the switch off: reprojection as it was, and nothing for the filter to run over
    ctx.history_capture()
    ctx.reproject()
    off = ctx.read_reprojected()
    rt_err(-3, ctx.read_reprojected_variance, "rt_set_history_variance")
    rt_err(-3, ctx.denoise_reprojected, "rt_set_history_variance")
    ctx.set_history_variance(False)                                       # no change: nothing dropped
    assert bit_equal(ctx.read_reprojected(), off)
    # changing the value drops the history and the result
    ctx.set_history_variance(True)
    rt_err(-3, ctx.read_reprojected, "rt_reproject")
    rt_err(-3, ctx.read_reprojected_variance, "rt_reproject")
    rt_err(-3, ctx.reproject, "rt_history_capture")
    rt_err(-3, lambda: ctx.history_capture("reprojected"), "rt_reproject")
    rt_err(-3, ctx.denoise_reprojected, "rt_reproject")                   # the filter before any reproject
    ctx.history_capture()
    rt_err(-3, ctx.denoise_reprojected, "rt_reproject")                   # ... and with a history but no result
    ctx.reproject()
    assert bit_equal(ctx.read_reprojected(), off)
    s2 = ctx.read_reprojected_variance()
    assert s2.shape == (32, 32) and (s2 >= 0).all()                       # four frames everywhere
    first = ctx.denoise_reprojected()
    ctx.set_history_variance(True)                                        # no change again
    assert bit_equal(ctx.read_reprojected_variance(), s2)
    # bad parameters: RT_ERR_INVALID_ARG
    for bad in (dict(levels=0), dict(levels=6), dict(k=0.0), dict(k=float("nan")), dict(guides=(-1.0, 0.0, 0.0)),
                dict(guides=(0.0, float("inf"), 0.0))):
        rt_err(-1, lambda: ctx.denoise_reprojected(**bad))
    # the features rendered again since the reproject, even for the same camera
    ctx.render_features()
    rt_err(-3, ctx.denoise_reprojected, "rendered again")
    assert bit_equal(ctx.read_reprojected_variance(), s2)                 # the result itself stays
    ctx.reproject()
    assert bit_equal(ctx.denoise_reprojected(), first)
    # stale features (a camera move)
    ctx.set_camera(moved.camera)
    rt_err(-3, ctx.denoise_reprojected, "rt_render_features")
    render(ctx, 1, 1)
    ctx.render_features()
    rt_err(-3, ctx.denoise_reprojected, "rendered again")
    ctx.reproject()
    one = ctx.denoise_reprojected()                                       # one frame per pixel: no minimum count
    assert np.isfinite(one).all() and (ctx.read_reprojected_variance() < 0).any()
    rt_err(-3, lambda: ctx.denoise(), "two frames")                       # rt_denoise still refuses it
    # the result is rt_read_denoised's, held under its rules
    held = np.empty((32, 32, 4), F)
    ctx._check(ctx._L.rt_read_denoised(ctx._h, held.ctypes.data_as(rtamd._lib.c_float_p)))
    assert bit_equal(held, one)
    # switching off drops history and result; the buffers of the filter are not the switch's
    ctx.set_history_variance(False)
    rt_err(-3, ctx.read_reprojected, "rt_reproject")
    rt_err(-3, ctx.denoise_reprojected, "rt_set_history_variance")
    ctx.set_history_variance(True)
    ctx.history_capture()
    ctx.reproject()
    ctx.denoise_reprojected()
    # rt_resize frees everything
    ctx.resize(32, 32)
    rt_err(-3, ctx.read_reprojected_variance, "rt_reproject")
    rt_err(-3, ctx.denoise_reprojected, "rt_reproject")
    rt_err(-3, lambda: ctx._check(ctx._L.rt_read_denoised(ctx._h, held.ctypes.data_as(rtamd._lib.c_float_p))), "rt_denoise")
    ctx.close()


# ---- 4. the recorded experiment --------------------------------------------------------------------------

def rms_y(a, b, mask=None):
    ya, yb = [(v[..., 0].astype(np.float64) + v[..., 1]) + v[..., 2] for v in (a, b)]
    d = ya - yb
    ok = np.isfinite(d) if mask is None else np.isfinite(d) & mask
    return float(np.sqrt(np.mean(d[ok] ** 2)))


@functools.lru_cache(maxsize=None)
def long_render_at_b(sid, w, h, frames, seed):
    ctx = context(scene_of(sid, w, h, 1), frames, variance=False)
    render(ctx, 1, frames, seed=seed)
    ref = ctx.read_image()
    ctx.close()
    return ref


@pytest.mark.parametrize("frames_b", [1, 2])
def test_quality_of_the_filtered_view_after_a_move(gpu, frames_b):
    """tools/reproject_filter_quality.py's experiment on the device.  The device's image is the oracle's and the
    filter is the host's, so the ratios are the CPU run's (profiles/reproject_filter_quality.json) but for the
    moments, which the tool rebuilds to within an ulp or two.  RMS error of y of the filtered view over that of
    the unfiltered reprojected view, each bound halfway between the recorded ratio and 1:
      fresh pixels (n_out <= frames at B), guided at the library's defaults: recorded 0.4591 (1 frame), 0.3178 (2);
      whole image at the grid's best setting (levels 4 / 2, k 1): recorded 0.9934, 0.9942.
    At the library's defaults the whole-image ratio is above 1 (recorded 1.0723, 1.0653: DESIGN.md section 4 says
    why); it is printed, not asserted."""
    rec_all = json.load(open(os.path.join(REPO, "profiles", "reproject_filter_quality.json")))
    rec = rec_all["runs"][f"frames_b={frames_b}"]
    sid, w, h = rec_all["scene"], rec_all["width"], rec_all["height"]
    assert (sid, w, h, rec_all["frames_a"], rec_all["ref_frames"], rec_all["shift"]) == (6, 32, 32, 64, 1024, SHIFT)
    assert (rec_all["denoise_defaults"]["levels"], rec_all["denoise_defaults"]["k"]) == rtamd.render.DENOISE_DEFAULTS
    ref = long_render_at_b(sid, w, h, rec_all["ref_frames"], rec_all["ref_seed"])
    a, b = scene_of(sid, w, h, 0), scene_of(sid, w, h, 1)
    ctx = context(a, 64)
    ctx.set_moments(True)
    render(ctx, 1, 64)
    ctx.render_features()
    ctx.history_capture()
    ctx.set_params(spp=frames_b)
    move_to(ctx, b, n=frames_b)
    ctx.reproject()
    out = ctx.read_reprojected()
    fresh = out[..., 3] <= F(frames_b)
    assert int(fresh.sum()) == rec["fresh_pixels"]
    best = dict(part.split("=") for part in rec["grid_best"].split(","))
    at_defaults = ctx.denoise_reprojected()
    at_best = ctx.denoise_reprojected(levels=int(best["levels"]), k=float(best["k"]))
    ctx.close()
    e_whole, e_fresh = rms_y(out, ref), rms_y(out, ref, fresh)
    got = dict(fresh=rms_y(at_defaults, ref, fresh) / e_fresh, whole=rms_y(at_defaults, ref) / e_whole,
               best_whole=rms_y(at_best, ref) / e_whole)
    r_def, r_best = rec["filtered_over_reprojected"]["guided_defaults"], rec["grid_guided"][rec["grid_best"]]
    print(f"scene {sid} {w}x{h}, {frames_b} frame(s) at B: filtered / reprojected RMS y: fresh {got['fresh']:.4f} "
          f"(CPU {r_def['fresh']}), whole {got['whole']:.4f} (CPU {r_def['whole']}), whole at {rec['grid_best']} "
          f"{got['best_whole']:.4f} (CPU {r_best['whole']})")
    assert r_def["fresh"] < 1.0 and r_best["whole"] < 1.0
    assert got["fresh"] <= (r_def["fresh"] + 1.0) / 2.0
    assert got["best_whole"] <= (r_best["whole"] + 1.0) / 2.0

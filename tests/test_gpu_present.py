"""The presented frame on the device (rt.h rt_present / rt_read_presented / rt_read_presented_float /
rt_bind_device_present / rt_render_moved; rt_present.hip) against rt_present_host bit for bit, the
RT_PRESENT_MOVED rule on real moves, the rounding input against rts_tonemap_rgb8, everything else left as it
was, the state rules, a bound torch tensor, and the one call per pose against the public calls made one by
one.  The shapes are test_gpu_reproject_var.py's; renders are depth 5, seed 1.
"""
import ctypes

import numpy as np
import pytest

import rtamd
from rtamd import _lib
from helpers import bit_equal, mismatch_report
import present_ref as P
from test_gpu_reproject_var import CASES, context, move_to, render, rt_err, scene_of, view

pytestmark = pytest.mark.gpu

F = np.float32


def read_denoised(ctx):
    out = np.empty((ctx.height, ctx.width, 4), F)
    ctx._check(ctx._L.rt_read_denoised(ctx._h, out.ctypes.data_as(_lib.c_float_p)))
    return out


def moved_to_b(case, frames_a=8, frames_b=1, variance=True):
    """A context at pose B after one move: history from `frames_a` frames at A, `frames_b` at B, reprojected
    and (with the variance) filtered."""
    sid, w, h = case
    a, b = scene_of(sid, w, h, 0), scene_of(sid, w, h, 1)
    ctx = context(a, variance=variance)
    ctx.set_moments(True)
    render(ctx, 1, frames_a)
    ctx.render_features()
    ctx.history_capture()
    move_to(ctx, b, n=frames_b)
    ctx.reproject()
    if variance:
        ctx.denoise_reprojected()
    return ctx, b


def held(ctx):
    """Everything the frame is made from, and everything it must leave alone."""
    v = view(ctx, np.zeros(28, F))
    v.update(rp=ctx.read_reprojected(), s2=ctx.read_reprojected_variance(), den=read_denoised(ctx))
    return v


def sources_of(v):
    return dict(image=v["image"], denoised=v["den"], reprojected=v["rp"], tile_frames=v["tf"])


# ---- 1. the device against the host function, over a chain of poses ------------------------------------

@pytest.mark.parametrize("case", CASES, ids=lambda c: f"scene{c[0]}_{c[1]}x{c[2]}")
def test_device_matches_the_host(gpu, case):
    ctx, _ = moved_to_b(case)
    v = held(ctx)
    src = sources_of(v)
    assert set(v["tf"].tolist()) == {1}
    for source in P.SOURCES:
        for exposure in P.EXPOSURES:
            ref8, reff = rtamd.present_host(source, exposure=exposure, keep_float=True, **src)
            res8, resf = P.present(source, exposure=exposure, **src)
            assert np.array_equal(ref8, res8) and bit_equal(reff, resf)       # the host is the restatement here too
            tag = (source, exposure)
            got8 = ctx.present(source, exposure=exposure)
            assert got8.shape == ref8.shape and got8.dtype == np.uint8
            assert np.array_equal(got8, ref8), (tag, np.argwhere(got8 != ref8)[:4])
            rt_err(-3, ctx.read_presented_float, "keep_float")                # no float copy was asked for
            got8 = ctx.present(source, exposure=exposure, keep_float=True)
            gotf = ctx.read_presented_float()
            assert np.array_equal(got8, ref8), (tag, np.argwhere(got8 != ref8)[:4])
            assert bit_equal(gotf, reff), (tag, mismatch_report(gotf, reff))
    # the composite: the filtered buffer where the count did not grow, the reprojected view elsewhere
    ctx.present("moved", keep_float=True)
    f = ctx.read_presented_float()
    w1, w0 = f[..., 3] == 1, f[..., 3] == 0
    assert (w1 | w0).all()
    assert bit_equal(f[w1][:, :3], v["den"][w1][:, :3]) and bit_equal(f[w0][:, :3], v["rp"][w0][:, :3])
    n_t = P.tile_counts_per_pixel(v["tf"], case[1], case[2]).astype(F)
    assert np.array_equal(w1, v["rp"][..., 3] <= n_t)
    if case[0] == 6:
        assert w1.any() and w0.any()
        assert not bit_equal(v["den"][w1][:, :3], v["rp"][w1][:, :3])        # the filter did change the fresh pixels
    # NULL parameters: the image at exposure 1
    ctx._check(ctx._L.rt_present(ctx._h, None))
    assert np.array_equal(ctx.read_presented(), rtamd.present_host("image", image=v["image"]))
    ctx.close()


def test_rounding_input_equals_rts_tonemap_rgb8(gpu):
    img = P.rounding_image()
    ctx = rtamd.RenderContext()
    ctx.resize(P.ROUNDING_W, P.ROUNDING_H)
    ctx.write_image(img)
    got = ctx.present("image", keep_float=True)
    flt = ctx.read_presented_float()
    ctx.close()
    ref = rtamd.tonemap_rgb8(img)
    assert np.array_equal(got[..., :3], ref), np.argwhere(got[..., :3] != ref)[:4]
    assert (got[..., 3] == 255).all()
    assert bit_equal(flt[..., :3], img[..., :3]) and (flt[..., 3] == 1).all()


# ---- 2. nothing else moves ------------------------------------------------------------------------------

def test_everything_else_keeps_its_bits(gpu):
    case = (6, 32, 32)

    def run(presenting):
        ctx, b = moved_to_b(case, frames_b=2)
        before = held(ctx)
        if presenting:
            for source in P.SOURCES:
                for keep in (False, True):
                    ctx.present(source, exposure=0.5, keep_float=keep)
            after = held(ctx)
            for k in ("image", "m2", "nd", "ai", "rp", "s2", "den"):
                assert bit_equal(before[k], after[k]), (k, mismatch_report(before[k], after[k]))
            assert list(before["tf"]) == list(after["tf"])
        render(ctx, 3, 2)                                                    # later frames
        out = dict(image=ctx.read_image(), m2=ctx.read_moments(), tf=list(ctx.read_tile_frames()), last=ctx.last_launch(),
                   den=ctx.denoise(guides=True))
        ctx.close()
        return out

    yes, no = run(True), run(False)
    for k in ("image", "m2", "den"):
        assert bit_equal(yes[k], no[k]), (k, mismatch_report(yes[k], no[k]))
    assert yes["tf"] == no["tf"] == [4] * 16 and yes["last"] == no["last"]


# ---- 3. state -------------------------------------------------------------------------------------------

def raw_present(ctx, source=0, exposure=1.0, keep_float=0, reserved=()):
    p = _lib.RtPresentParams()
    p.source, p.exposure, p.keep_float = source, exposure, keep_float
    for i, r in enumerate(reserved):
        p.reserved[i] = r
    ctx._check(ctx._L.rt_present(ctx._h, ctypes.byref(p)))


def test_state_rules(gpu):
    scene = scene_of(6, 32, 32, 0)
    two = rtamd.RenderContext(devices=(0, 0))
    two.upload_scene(scene)
    two.resize(32, 32)
    rt_err(-3, two.present, "1-device")                                   # a two-slot context
    rt_err(-3, lambda: two.bind_device_present(None), "1-device")
    rt_err(-3, two.read_presented)
    rt_err(-3, two.read_presented_float)
    two.close()
    part = rtamd.RenderContext(rank=0, world=2, stripe_rows=8)
    part.upload_scene(scene)
    part.resize(32, 32)
    rt_err(-3, part.present, "rt_set_partition")                          # a partition
    part.close()
    bare = rtamd.RenderContext()
    rt_err(-3, bare.present, "no image")                                  # no rt_resize yet
    bare.close()

    ctx = context(scene)
    rt_err(-3, ctx.read_presented, "rt_present")                          # nothing presented yet
    rt_err(-3, lambda: ctx.present("denoised"), "rt_denoise")
    rt_err(-3, lambda: ctx.present("reprojected"), "rt_reproject")
    rt_err(-3, lambda: ctx.present("moved"), "rt_reproject")
    black = ctx.present("image")                                          # the image alone is enough
    assert (black[..., :3] == 0).all() and (black[..., 3] == 255).all()
    rt_err(-3, ctx.read_presented_float, "keep_float")
    # bad parameters: RT_ERR_INVALID_ARG, and the frame held stays
    for bad in (dict(source=4), dict(source=-1), dict(exposure=0.0), dict(exposure=-2.0), dict(exposure=float("nan")),
                dict(exposure=float("inf")), dict(reserved=(1,)), dict(reserved=(0, 0, 0, 0, 3))):
        rt_err(-1, lambda: raw_present(ctx, **bad), "rt_present")
    assert np.array_equal(ctx.read_presented(), black)
    ctx.close()

    ctx, b = moved_to_b((6, 32, 32), frames_b=2)
    first = ctx.present("moved", keep_float=True)
    ctx.present("moved")                                                  # a frame without the copy drops the copy
    rt_err(-3, ctx.read_presented_float, "keep_float")
    # the denoised buffer must be rt_denoise_reprojected's, from the result now held
    ctx.denoise(guides=True)                                              # rt_denoise_guided wrote it since
    rt_err(-3, lambda: ctx.present("moved"), "rt_denoise_reprojected")
    ctx.present("denoised")                                               # ... which the plain source does not mind
    ctx.denoise()
    rt_err(-3, lambda: ctx.present("moved"), "rt_denoise_reprojected")
    ctx.denoise_reprojected()
    assert np.array_equal(ctx.present("moved"), first)
    ctx.reproject()                                                       # another result: the buffer is the old one's
    rt_err(-3, lambda: ctx.present("moved"), "rt_denoise_reprojected")
    ctx.present("reprojected")
    ctx.denoise_reprojected()
    assert np.array_equal(ctx.present("moved"), first)
    # dropping the result (the variance switch) refuses both sources that read it
    ctx.set_history_variance(False)
    rt_err(-3, lambda: ctx.present("reprojected"), "rt_reproject")
    rt_err(-3, lambda: ctx.present("moved"), "rt_reproject")
    ctx.history_capture()
    ctx.reproject()                                                       # a result without variance: no filter ran over it
    rt_err(-3, lambda: ctx.present("moved"), "rt_denoise_reprojected")
    ctx.present("reprojected")
    ctx.set_history_variance(True)
    ctx.history_capture()
    ctx.reproject()
    ctx.denoise_reprojected()
    ctx.present("moved")
    # the moments off: no tile counts
    ctx.set_moments(False)
    rt_err(-3, lambda: ctx.present("moved"), "rt_set_moments")
    # rt_resize frees everything
    ctx.present("image")
    ctx.resize(32, 32)
    rt_err(-3, ctx.read_presented, "rt_present")
    rt_err(-3, lambda: ctx.present("moved"), "rt_reproject")
    ctx.close()


# ---- 4. a bound torch tensor on a torch stream ----------------------------------------------------------

def test_bound_torch_tensor_and_stream(gpu):
    import torch
    case = (6, 32, 32)
    ctx, _ = moved_to_b(case)
    ref = ctx.present("moved", exposure=0.5)                              # through the internal buffer
    frame = torch.zeros((32, 32, 4), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=0)
    ctx.set_stream(stream.cuda_stream)
    rt_err(-1, lambda: ctx.bind_device_present(frame.data_ptr(), frame.numel() - 1), "too small")
    ctx.bind_device_present(frame.data_ptr(), frame.numel())
    rt_err(-3, ctx.read_presented, "rt_present")                          # the frame held was the other buffer's
    ctx._check(ctx._L.rt_present(ctx._h, rtamd.render._present_params("moved", 0.5, False)))
    stream.synchronize()
    got = frame.cpu().numpy()
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:4]
    assert np.array_equal(ctx.read_presented(), ref)
    # unbinding returns to the internal buffer: the tensor is written no more
    frame.zero_()
    torch.cuda.synchronize()
    ctx.bind_device_present(None)
    rt_err(-3, ctx.read_presented, "rt_present")
    assert np.array_equal(ctx.present("moved", exposure=0.5), ref)
    torch.cuda.synchronize()
    assert not frame.cpu().numpy().any()
    ctx.set_stream(None)
    ctx.close()


# ---- 5. one call per pose ---------------------------------------------------------------------------------

@pytest.mark.parametrize("variance", [True, False], ids=["variance_on", "variance_off"])
def test_render_moved_is_the_public_calls_one_by_one(gpu, variance):
    sid, w, h = 6, 32, 32
    a, b, c = (scene_of(sid, w, h, k) for k in (0, 1, 2))

    def at_a():
        ctx = context(a, variance=variance)
        ctx.set_moments(True)
        render(ctx, 1, 8)
        ctx.render_features()
        return ctx

    one, steps, plain = at_a(), at_a(), at_a()
    source = "moved" if variance else "reprojected"
    for pose, (scene, frames, hist) in enumerate([(b, 1, "image"), (c, 2, "reprojected")]):
        rf = rtamd.frame_rand_factors(1, 0, frames)
        got8 = one.render_moved(scene.camera, rf, keep_float=True, exposure=0.5)
        gotf = one.read_presented_float()
        steps.history_capture(hist)
        steps.set_camera(scene.camera)
        steps.render(1, rf)
        steps.render_features()
        steps.reproject()
        if variance:
            steps.denoise_reprojected()
        ref8 = steps.present(source, exposure=0.5, keep_float=True)
        reff = steps.read_presented_float()
        assert np.array_equal(got8, ref8), (pose, np.argwhere(got8 != ref8)[:4])
        assert bit_equal(gotf, reff), (pose, mismatch_report(gotf, reff))
        if variance:
            assert (gotf[..., 3] == 1).any() and (gotf[..., 3] == 0).any()
        else:
            assert (gotf[..., 3] == 1).all()
        # NULL parameters all the way: the library's choice of the source, exposure 1
        assert np.array_equal(plain.render_moved(scene.camera, rf), steps.present(source))
        for k in ("image", "m2", "nd", "ai"):
            va, vb = view(one, scene.camera), view(steps, scene.camera)
            assert bit_equal(va[k], vb[k]), (pose, k)
        assert bit_equal(one.read_reprojected(), steps.read_reprojected())
    assert (one.read_reprojected()[..., 3] > 10.0).any()                  # 2 + (1 + 8): the second pose built on the first's result
    if not variance:
        # RT_PRESENT_MOVED without the variance: rt_present's refusal, unchanged
        rt_err(-3, lambda: one.render_moved(b.camera, rtamd.frame_rand_factors(1, 0, 1), source="moved"), "rt_denoise_reprojected")
    # a step's refusal comes back unchanged: no features for the pose being left
    bare = context(a, variance=variance)
    bare.set_moments(True)
    render(bare, 1, 2)
    rt_err(-3, lambda: bare.render_moved(b.camera, rtamd.frame_rand_factors(1, 0, 1)), "rt_render_features")
    rt_err(-1, lambda: one.render_moved(b.camera, rtamd.frame_rand_factors(1, 0, 1), exposure=0.0), "rt_present")
    for ctx in (one, steps, plain, bare):
        ctx.close()

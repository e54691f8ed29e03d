#!/usr/bin/env python3
"""What carrying the variance through reprojection and filtering the reprojected view cost (rt.h
rt_set_history_variance, rt_denoise_reprojected) at 1920x1080 on scene 8, measured as tools/reproject_cost.py
measures reprojection itself: the device time of each call between two events on the context's stream, medians
of two windows of calls.

    python tools/reproject_filter_cost.py [--out profiles/reproject_filter_cost.json]

With the switch off rt_reproject and rt_history_capture launch the kernels they always launched, so their
figures are set beside the ones profiles/reproject_cost.json recorded for the parent: the same kernel, within
the spread of the two windows.  With the switch on rt_reproject reads 4 more bytes per pixel of its own (M2.w,
one float of a float4 it does not otherwise touch: 16 bytes of traffic), 4 per tap of the history's s2, and
writes 4; rt_history_capture from the image reads M2.w and writes 4 bytes, from the result copies 4 more.
rt_denoise_reprojected is one prologue kernel (36 bytes read and 16 written per pixel where s2 is known, the 25
taps' 32 bytes each from the caches where it is not) and then rt_denoise_guided's levels unchanged; rt_denoise_guided
over the same image is timed beside it.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-book_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from reproject_cost import stream_ms  # noqa: E402


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--scene", type=int, default=8)
    p.add_argument("--width", type=int, default=1920)
    p.add_argument("--height", type=int, default=1080)
    p.add_argument("--frames", type=int, default=8, help="frames behind the history")
    p.add_argument("--frames-b", type=int, default=2, help="frames at the new camera (rt_denoise_guided needs two)")
    p.add_argument("--shift", type=float, default=0.05, help="the camera move, in viewport widths along pixel_delta_u")
    p.add_argument("--calls", type=int, default=50)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import numpy as np
    import torch
    import rtamd
    assert torch.cuda.is_available(), "no HIP device: the cost is a device measurement"
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream(device=0)
    scene = rtamd.Scene(a.scene, a.width, a.height, seed=1)
    ctx = rtamd.RenderContext()
    ctx.upload_scene(scene)
    ctx.set_params(max_depth=5, spp=a.frames)
    ctx.resize(a.width, a.height)
    ctx.set_stream(stream.cuda_stream)
    ctx.set_moments(True)
    res = {"tool": "reproject_filter_cost", "timing": "device events on the context's stream around each call",
           "config": {k: getattr(a, k) for k in ("scene", "width", "height", "frames", "frames_b", "shift", "calls", "warmup")}}
    cam_a = scene.camera.copy()
    cam_b = cam_a.copy()
    v = cam_b[12:15] * np.float32(a.shift * a.width)
    cam_b[4:7] += v
    cam_b[8:11] += v

    def ms(call):
        return stream_ms(torch, stream, call, a.calls, a.warmup)

    def at_a():
        ctx.set_camera(cam_a)
        ctx.render(1, rtamd.frame_rand_factors(1, 0, a.frames))
        ctx.render_features()

    def at_b():
        ctx.set_camera(cam_b)
        ctx.render(1, rtamd.frame_rand_factors(1, 0, a.frames_b))
        ctx.render_features()

    with torch.cuda.stream(stream):
        for mode in ("off", "on", "off_again", "on_again"):   # the two windows of each, interleaved
            ctx.set_history_variance(mode.startswith("on"))
            at_a()
            r = {"history_capture_ms": ms(ctx.history_capture)}
            at_b()
            r["reproject_ms"] = ms(ctx.reproject)
            r["history_capture_from_reprojected_ms"] = ms(lambda: ctx.history_capture("reprojected"))
            if mode.startswith("on"):
                ctx.reproject()
                r["denoise_reprojected_ms"] = ms(lambda: ctx._check(ctx._L.rt_denoise_reprojected(ctx._h, None, None)))
                r["denoise_guided_ms"] = ms(lambda: ctx._check(ctx._L.rt_denoise_guided(ctx._h, None, None)))
                res["s2_unknown_pixels"] = int((~(ctx.read_reprojected_variance() >= 0)).sum())
                # one frame at the new camera: the pixels the history does not reach take the 25-tap estimate
                at_a()
                ctx.history_capture()
                ctx.set_camera(cam_b)
                ctx.render(1, rtamd.frame_rand_factors(1, 0, 1))
                ctx.render_features()
                ctx.reproject()
                r["denoise_reprojected_one_frame_ms"] = ms(lambda: ctx._check(ctx._L.rt_denoise_reprojected(ctx._h, None, None)))
                res["s2_unknown_pixels_one_frame"] = int((~(ctx.read_reprojected_variance() >= 0)).sum())
            res[mode] = r
    ctx.close()
    parent = json.load(open(os.path.join(REPO, "profiles", "reproject_cost.json")))
    res["parent"] = {k: parent[k]["median"] for k in ("reproject_ms", "reproject_ms_again", "history_capture_ms", "history_capture_ms_again")}
    off = [res["off"]["reproject_ms"]["median"], res["off_again"]["reproject_ms"]["median"]]
    on = [res["on"]["reproject_ms"]["median"], res["on_again"]["reproject_ms"]["median"]]
    par = [res["parent"]["reproject_ms"], res["parent"]["reproject_ms_again"]]
    spread = max(abs(off[0] - off[1]), abs(par[0] - par[1]))
    res["reproject_off_ms"] = round(sum(off) / 2, 5)
    res["reproject_parent_ms"] = round(sum(par) / 2, 5)
    res["reproject_off_minus_parent_ms"] = round(sum(off) / 2 - sum(par) / 2, 5)
    res["window_spread_ms"] = round(spread, 5)
    res["reproject_off_within_spread_of_parent"] = bool(abs(sum(off) / 2 - sum(par) / 2) <= spread)
    res["reproject_on_minus_off_ms"] = round(sum(on) / 2 - sum(off) / 2, 5)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What temporal reprojection costs (rt.h rt_reproject, rt_history_capture) at 1920x1080 on scene 8: the device
time of each call between two events on the context's stream (medians of two windows of calls), beside a
one-frame rt_render launch timed the same way on the same context in the same run -- the yardstick: the
launch reprojection stands beside after a camera move, which this feature leaves as it was.

    python tools/reproject_cost.py [--out profiles/reproject_cost.json]

rt_reproject reads, per pixel, 3 float4 of its own (image, normal_depth, albedo_id), up to 12 of the history
(four taps in three buffers; neighbouring lanes share most of them) and writes one: 64 bytes of compulsory
traffic, 256 with every tap counted.  rt_history_capture reads 48 and writes 48.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-book_amd"))

HBM_BYTES_PER_S = 6.3e12   # achievable streaming rate of the MI355X's HBM


def stream_ms(torch, stream, call, calls, warmup):
    """Each call between two events on `stream`: its device time, queueing gaps included."""
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ev = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        torch.cuda.synchronize()
        ev.append((e0, e1))
    ms = [a.elapsed_time(b) for a, b in ev]
    return {"median": round(statistics.median(ms), 5), "min": round(min(ms), 5), "max": round(max(ms), 5), "calls": len(ms)}


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--scene", type=int, default=8)
    p.add_argument("--width", type=int, default=1920)
    p.add_argument("--height", type=int, default=1080)
    p.add_argument("--frames", type=int, default=8, help="frames behind the history")
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
    px = a.width * a.height
    res = {"tool": "reproject_cost", "timing": "device events on the context's stream around each call",
           "config": {k: getattr(a, k) for k in ("scene", "width", "height", "frames", "shift", "calls", "warmup")}}
    with torch.cuda.stream(stream):
        ctx.render(1, rtamd.frame_rand_factors(1, 0, a.frames))
        ctx.render_features()
        res["history_capture_ms"] = stream_ms(torch, stream, ctx.history_capture, a.calls, a.warmup)
        cam = scene.camera.copy()
        v = cam[12:15] * np.float32(a.shift * a.width)
        cam[4:7] += v
        cam[8:11] += v
        ctx.set_camera(cam)
        rf1 = rtamd.frame_rand_factors(1, 0, 1)
        # the yardstick first and again last: a one-frame launch (frame 1 every time) at the new camera
        res["render_one_frame_ms"] = stream_ms(torch, stream, lambda: ctx.render(1, rf1), a.calls, a.warmup)
        ctx.render_features()
        res["reproject_ms"] = stream_ms(torch, stream, ctx.reproject, a.calls, a.warmup)
        res["history_capture_ms_again"] = stream_ms(torch, stream, lambda: ctx.history_capture("reprojected"), a.calls, a.warmup)
        res["reproject_ms_again"] = stream_ms(torch, stream, ctx.reproject, a.calls, a.warmup)   # the spread between two windows
        res["render_one_frame_ms_again"] = stream_ms(torch, stream, lambda: ctx.render(1, rf1), a.calls, a.warmup)
        out = ctx.read_reprojected()
    nd, alb, ids = ctx.read_features()
    hit = ids != 0xFFFFFFFF
    res["hit_pixels"] = int(hit.sum())
    res["reprojected_pixels"] = int((out[..., 3][hit] > 1.0).sum())
    ctx.close()
    res["reproject_bytes_per_pixel"] = {"compulsory": 64, "every_tap": 256}
    res["reproject_byte_floor_ms"] = round(px * 64 / HBM_BYTES_PER_S * 1e3, 5)
    res["reproject_every_tap_ms"] = round(px * 256 / HBM_BYTES_PER_S * 1e3, 5)
    res["history_capture_byte_floor_ms"] = round(px * 96 / HBM_BYTES_PER_S * 1e3, 5)
    res["reproject_below_one_frame_render"] = bool(
        max(res["reproject_ms"]["median"], res["reproject_ms_again"]["median"])
        < min(res["render_one_frame_ms"]["median"], res["render_one_frame_ms_again"]["median"]))
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the presented frame costs (rt.h rt_present) at 1920x1080 on scene 8 after a camera move: the device
time of rt_present for each source, with and without the float copy, between two events on the context's
stream (medians of two windows of calls), beside a one-frame rt_render launch timed the same way on the same
context in the same run -- the yardstick.  Then the wall time of rt_present(RT_PRESENT_MOVED) +
rt_read_presented against the path it replaces: rt_read_reprojected, rt_read_denoised, the composite in NumPy
and rts_tonemap_rgb8 on the host.  Last, on the -DRT_AB_KNOBS library, the gamma table read from its device
buffer against the table staged into LDS per workgroup (RT_PRESENT_LUT=lds), the two placements interleaved.

    python tools/present_cost.py [--out profiles/present_cost.json]

RT_PRESENT_MOVED reads, per pixel, two float4 and writes one dword: 36 bytes of compulsory traffic (the tile
count and the table stay in the caches); the single-buffer sources 20; the float copy adds 16.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-book_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from reproject_cost import HBM_BYTES_PER_S, stream_ms  # noqa: E402

SOURCES = ("image", "denoised", "reprojected", "moved")
BYTES = {"image": 20, "denoised": 20, "reprojected": 20, "moved": 36}


def wall_ms(call, calls, warmup):
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "calls": len(ms)}


def moved_context(rtamd, np, a, stream, ab=False):
    """A context at the pose after the move: reprojected and filtered, everything rt_present reads held."""
    scene = rtamd.Scene(a.scene, a.width, a.height, seed=1)
    ctx = rtamd.RenderContext(ab=ab)
    ctx.upload_scene(scene)
    ctx.set_params(max_depth=5, spp=a.frames)
    ctx.resize(a.width, a.height)
    ctx.set_stream(stream.cuda_stream)
    ctx.set_moments(True)
    ctx.set_history_variance(True)
    ctx.render(1, rtamd.frame_rand_factors(1, 0, a.frames))
    ctx.render_features()
    ctx.history_capture()
    cam = scene.camera.copy()
    v = cam[12:15] * np.float32(a.shift * a.width)
    cam[4:7] += v
    cam[8:11] += v
    ctx.set_camera(cam)
    ctx.render(1, rtamd.frame_rand_factors(1, 0, 1))
    ctx.render_features()
    ctx.reproject()
    ctx.denoise_reprojected()
    return ctx


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--scene", type=int, default=8)
    p.add_argument("--width", type=int, default=1920)
    p.add_argument("--height", type=int, default=1080)
    p.add_argument("--frames", type=int, default=8, help="frames behind the history")
    p.add_argument("--shift", type=float, default=0.05, help="the camera move, in viewport widths along pixel_delta_u")
    p.add_argument("--calls", type=int, default=50)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--wall-calls", type=int, default=10)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import numpy as np
    import torch
    import rtamd
    from rtamd.render import _present_params
    assert torch.cuda.is_available(), "no HIP device: the cost is a device measurement"
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream(device=0)
    px = a.width * a.height
    res = {"tool": "present_cost", "timing": "device events on the context's stream around each call",
           "config": {k: getattr(a, k) for k in ("scene", "width", "height", "frames", "shift", "calls", "warmup", "wall_calls")}}

    def present(ctx, source, keep):
        pp = _present_params(source, 1.0, keep)
        return lambda: ctx._check(ctx._L.rt_present(ctx._h, pp))

    with torch.cuda.stream(stream):
        ctx = moved_context(rtamd, np, a, stream)
        rf1 = rtamd.frame_rand_factors(1, 0, 1)
        one_frame = lambda: ctx.render(1, rf1)  # noqa: E731  (frame 1 every time: the image stays a one-frame image)
        res["render_one_frame_ms"] = stream_ms(torch, stream, one_frame, a.calls, a.warmup)
        for window in ("present_ms", "present_ms_again"):   # two windows: the spread between them
            res[window] = {}
            for source in SOURCES:
                for keep in (False, True):
                    key = source + ("+float" if keep else "")
                    res[window][key] = stream_ms(torch, stream, present(ctx, source, keep), a.calls, a.warmup)
        res["render_one_frame_ms_again"] = stream_ms(torch, stream, one_frame, a.calls, a.warmup)
        res["byte_floor_ms"] = {s + ("+float" if k else ""): round(px * (BYTES[s] + (16 if k else 0)) / HBM_BYTES_PER_S * 1e3, 5)
                                for s in SOURCES for k in (False, True)}

        # the whole way to the host: the frame as 4 bytes per pixel, against the path it replaces
        def on_device():
            ctx._check(ctx._L.rt_present(ctx._h, _present_params("moved", 1.0, False)))
            return ctx.read_presented()

        tf = ctx.read_tile_frames()
        ty, tx = (a.height + 7) // 8, (a.width + 7) // 8
        n_t = np.repeat(np.repeat(tf.reshape(ty, tx), 8, 0), 8, 1)[:a.height, :a.width].astype(np.float32)

        def on_host():
            rp, dn = ctx.read_reprojected(), read_denoised(ctx, np, rtamd)
            fresh = ~(rp[..., 3] > n_t)
            return rtamd.tonemap_rgb8(np.where(fresh[..., None], dn, rp))

        got, ref = on_device(), on_host()
        assert np.array_equal(got[..., :3], ref), "the device frame is not the host path's"
        res["moved_to_host_wall_ms"] = {"present_and_read_presented": wall_ms(on_device, a.wall_calls, 2),
                                        "read_two_buffers_compose_tonemap_on_host": wall_ms(on_host, a.wall_calls, 2)}
        res["readback_bytes"] = {"present_and_read_presented": px * 4, "host_path": px * 32}
        res["fresh_pixels"] = int((~(ctx.read_reprojected()[..., 3] > n_t)).sum())
        ctx.close()

        # where the table lives: the A/B library holds both placements; interleaved windows on one context
        ab = moved_context(rtamd, np, a, stream, ab=True)
        place = {"device_buffer": [], "lds": []}
        for rnd in range(2):
            for name in ("device_buffer", "lds"):
                if name == "lds":
                    os.environ["RT_PRESENT_LUT"] = "lds"
                else:
                    os.environ.pop("RT_PRESENT_LUT", None)
                place[name].append({src: stream_ms(torch, stream, present(ab, src, False), a.calls, a.warmup)
                                    for src in ("image", "moved")})
        os.environ.pop("RT_PRESENT_LUT", None)
        frame_a = ab.present("moved")
        os.environ["RT_PRESENT_LUT"] = "lds"
        frame_b = ab.present("moved")
        os.environ.pop("RT_PRESENT_LUT", None)
        assert np.array_equal(frame_a, frame_b), "the two placements give different frames"
        res["table_placement_ms"] = place
        ab.close()
    res["present_below_one_frame_render"] = bool(
        max(v["median"] for w in ("present_ms", "present_ms_again") for v in res[w].values())
        < min(res["render_one_frame_ms"]["median"], res["render_one_frame_ms_again"]["median"]))
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def read_denoised(ctx, np, rtamd):
    out = np.empty((ctx.height, ctx.width, 4), np.float32)
    ctx._check(ctx._L.rt_read_denoised(ctx._h, out.ctypes.data_as(rtamd._lib.c_float_p)))
    return out


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What rendering the moved view to a noise target costs (rt.h rt_noise_tiles / rt_render_moved_to_noise) at
1920x1080 on scene 8 after a 0.05-viewport move (tools/refine_cost.py's setting): device time between two events on
the context's stream, medians of two interleaved windows of calls, of noise_tiles_kernel beside reach_kernel and a
one-frame full rt_render timed the same way on the same context in the same run -- the yardsticks are the parent's
kernels, never the new one.  The kernel's traffic gives a floor: 16 bytes per pixel of the result (whole 128-byte
lines) and 4 of s2 at the streaming rate the other cost tools use; the ratio to it is reported, not asserted.
Then wall times: a whole pose through rt_render_moved_to_noise at a few targets against rt_render_moved, each
followed by rt_sync, the camera going back and forth between the two poses, with rt_set_reproject_misses off and on,
and the rounds, tiles and tile-frames each pose took.

    python tools/noise_refine_cost.py [--out profiles/noise_refine_cost.json]
"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-book_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from present_cost import wall_ms  # noqa: E402
from reproject_cost import HBM_BYTES_PER_S, stream_ms  # noqa: E402

TARGETS = (0.5, 0.2, 0.1)


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
    p.add_argument("--batch", type=int, default=1)
    p.add_argument("--rounds", type=int, default=4)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import numpy as np
    import torch
    import rtamd
    from rtamd import _lib
    assert torch.cuda.is_available(), "no HIP device: the cost is a device measurement"
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream(device=0)
    px = a.width * a.height
    res = {"tool": "noise_refine_cost", "timing": "device events on the context's stream around each call; wall times with rt_sync",
           "config": {k: getattr(a, k) for k in ("scene", "width", "height", "frames", "shift", "calls", "warmup", "wall_calls",
                                                 "batch", "rounds")}}
    scene = rtamd.Scene(a.scene, a.width, a.height, seed=1)
    cam_a = scene.camera.copy()
    cam_b = cam_a.copy()
    v = cam_b[12:15] * np.float32(a.shift * a.width)
    cam_b[4:7] += v
    cam_b[8:11] += v
    rf1 = rtamd.frame_rand_factors(1, 0, 1)

    def at_a(misses=False):
        ctx = rtamd.RenderContext()
        ctx.upload_scene(scene)
        ctx.set_params(max_depth=5, spp=a.frames)
        ctx.resize(a.width, a.height)
        ctx.set_stream(stream.cuda_stream)
        ctx.set_moments(True)
        ctx.set_history_variance(True)
        ctx.set_reproject_misses(misses)
        ctx.render(1, rtamd.frame_rand_factors(1, 0, a.frames))
        ctx.render_features()
        return ctx

    with torch.cuda.stream(stream):
        ctx = at_a()
        ctx.history_capture()
        ctx.set_camera(cam_b)
        ctx.render(1, rf1)
        ctx.render_features()
        ctx.reproject()
        nt = int(ctx.read_tile_frames().size)
        res["tiles"] = nt
        # two interleaved windows: render, reach, noise, then the three again
        for tag in ("", "_again"):
            res["render_one_frame_ms" + tag] = stream_ms(torch, stream, lambda: ctx.render(1, rf1), a.calls, a.warmup)
            res["reach_ms" + tag] = stream_ms(torch, stream, lambda: ctx.reach_tiles(2.0), a.calls, a.warmup)
            res["noise_tiles_ms" + tag] = stream_ms(torch, stream, lambda: ctx.noise_tiles(2.0), a.calls, a.warmup)
        res["reproject_ms"] = stream_ms(torch, stream, ctx.reproject, a.calls, a.warmup)
        floor_bytes = px * 16 + px * 4
        res["noise_tiles_bytes"] = {"result_read_as_cache_lines": px * 16, "s2_read": px * 4, "written": nt * 16}
        res["noise_tiles_byte_floor_ms"] = round(floor_bytes / HBM_BYTES_PER_S * 1e3, 5)
        noise_med = min(res["noise_tiles_ms"]["median"], res["noise_tiles_ms_again"]["median"])
        reach_med = min(res["reach_ms"]["median"], res["reach_ms_again"]["median"])
        frame_med = min(res["render_one_frame_ms"]["median"], res["render_one_frame_ms_again"]["median"])
        res["noise_tiles_over_floor"] = round(noise_med / res["noise_tiles_byte_floor_ms"], 3)
        res["noise_tiles_over_reach"] = round(noise_med / reach_med, 3)
        res["noise_tiles_over_one_frame"] = round(noise_med / frame_med, 5)

        def records():
            ctx.noise_tiles(2.0)
            return ctx.read_tile_noise()

        res["readback_wall_ms"] = {"noise_tiles_and_read_tile_noise": wall_ms(records, a.wall_calls, 2)}
        rec = records()
        _, stats = rtamd.refine_noise_select(rec, 0.0)
        res["moved_view"] = {"noise": stats["noise"], "thin_pixels": stats["thin"], "known_pixels": stats["known"],
                             "tiles_with_a_thin_pixel": int((rec["thin_px"] > 0).sum())}
        ctx.close()

        # a whole pose, back and forth between the two cameras, each call followed by rt_sync
        def poses(target, misses):
            c = at_a(misses)
            cams = [cam_b, cam_a]
            state = {"i": 0, "log": []}
            rf = np.ascontiguousarray(rtamd.frame_rand_factors(1, 0, 1 + a.batch * a.rounds), np.float32)
            prm = _lib.RtNoiseRefineParams()
            prm.batch_frames, prm.max_rounds = a.batch, a.rounds
            rounds, tiles, spent, st = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), _lib.RtMovedNoiseStats()

            def call():
                cam = np.ascontiguousarray(cams[state["i"] % 2], np.float32)
                state["i"] += 1
                fp = _lib.c_float_p
                if target is None:
                    c._check(c._L.rt_render_moved(c._h, cam.ctypes.data_as(fp), 1, rf.ctypes.data_as(fp), None, None, None, None))
                else:
                    prm.target_noise = target
                    c._check(c._L.rt_render_moved_to_noise(c._h, cam.ctypes.data_as(fp), 1, rf.ctypes.data_as(fp), ctypes.byref(prm),
                                                           None, None, None, None, ctypes.byref(rounds), ctypes.byref(tiles),
                                                           ctypes.byref(spent), ctypes.byref(st)))
                    state["log"].append((rounds.value, tiles.value, spent.value, st.converged, round(st.noise, 5)))
                c.sync()

            out = wall_ms(call, a.wall_calls, 2)
            if target is not None:
                log = state["log"][2:]
                out.update(rounds=[x[0] for x in log], tiles_first_round=[x[1] for x in log], tile_frames_spent=[x[2] for x in log],
                           converged=[x[3] for x in log], noise=[x[4] for x in log],
                           full_frame_equivalents=round(float(np.median([x[2] for x in log])) / nt, 4))
            c.close()
            return out

        res["pose_wall_ms"] = {}
        for misses in (False, True):
            key = "misses_on" if misses else "misses_off"
            e = {"render_moved": poses(None, misses)}
            for t in TARGETS:
                e[f"to_noise_{t}"] = poses(t, misses)
            e["render_moved_again"] = poses(None, misses)
            res["pose_wall_ms"][key] = e
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

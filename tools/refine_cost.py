#!/usr/bin/env python3
"""What the extra frames after a move cost (rt.h rt_reach_tiles / rt_render_moved_refined) at 1920x1080 on
scene 8 after a 0.05-viewport move (tools/present_cost.py's setting): device time between two events on the
context's stream (medians of two windows of calls) of the reach kernel, of the masked K-frame rt_render over the
tiles rt_refine_select chooses for K in {1, 3, 7}, of the unmasked K-frame launch and of the second rt_reproject,
beside a one-frame full rt_render timed the same way on the same context in the same run -- the yardstick.
Then wall times: rt_read_tile_reach (the sync and 16 bytes per tile) against rt_read_reprojected (16 bytes per
pixel, what a caller would need without the records), and a whole pose through rt_render_moved_refined against
rt_render_moved, each followed by rt_sync, the camera going back and forth between the two poses.

    python tools/refine_cost.py [--out profiles/refine_cost.json]

The claim under test: K extra frames on the selected tiles cost less than K full frames.  The ratio is written
down whichever way it falls.
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

EXTRA = (1, 3, 7)


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
    from rtamd import _lib
    assert torch.cuda.is_available(), "no HIP device: the cost is a device measurement"
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream(device=0)
    px = a.width * a.height
    res = {"tool": "refine_cost", "timing": "device events on the context's stream around each call; wall times with rt_sync",
           "config": {k: getattr(a, k) for k in ("scene", "width", "height", "frames", "shift", "calls", "warmup", "wall_calls")}}
    scene = rtamd.Scene(a.scene, a.width, a.height, seed=1)
    cam_a = scene.camera.copy()
    cam_b = cam_a.copy()
    v = cam_b[12:15] * np.float32(a.shift * a.width)
    cam_b[4:7] += v
    cam_b[8:11] += v
    rf1 = rtamd.frame_rand_factors(1, 0, 1)

    def at_a():
        ctx = rtamd.RenderContext()
        ctx.upload_scene(scene)
        ctx.set_params(max_depth=5, spp=a.frames)
        ctx.resize(a.width, a.height)
        ctx.set_stream(stream.cuda_stream)
        ctx.set_moments(True)
        ctx.set_history_variance(True)
        ctx.render(1, rtamd.frame_rand_factors(1, 0, a.frames))
        ctx.render_features()
        return ctx

    def one_frame_at_b(ctx):
        ctx.set_active_tiles(None)
        ctx.render(1, rf1)

    with torch.cuda.stream(stream):
        ctx = at_a()
        ctx.history_capture()
        ctx.set_camera(cam_b)
        ctx.render(1, rf1)
        ctx.render_features()
        ctx.reproject()
        nt = int(ctx.read_tile_frames().size)
        res["tiles"] = nt
        res["render_one_frame_ms"] = stream_ms(torch, stream, lambda: ctx.render(1, rf1), a.calls, a.warmup)
        for window in ("reach_ms", "reach_ms_again"):
            res[window] = stream_ms(torch, stream, lambda: ctx.reach_tiles(4.0), a.calls, a.warmup)
        res["reach_bytes"] = {"read": px * 4, "read_as_cache_lines": px * 16, "written": nt * 16}
        res["reach_byte_floor_ms"] = round(px * 16 / HBM_BYTES_PER_S * 1e3, 5)
        res["reproject_ms"] = stream_ms(torch, stream, ctx.reproject, a.calls, a.warmup)
        res["extra"] = {}
        for k in EXTRA:
            one_frame_at_b(ctx)
            ctx.reproject()
            ctx.reach_tiles(float(1 + k))                       # the automatic count of a 1-frame pose
            reach = ctx.read_tile_reach()
            sel = rtamd.refine_select(reach)
            rfk = rtamd.frame_rand_factors(1, 1, k)
            e = {"min_count": 1 + k, "tiles_selected": int(sel.sum()), "share_of_tiles": round(float(sel.mean()), 5),
                 "short_pixels": int(reach["short_px"].sum()), "share_of_pixels_short": round(float(reach["short_px"].sum()) / px, 5)}
            # (frames 2 .. 1 + k again and again: only the time is read; the counts are restored below)
            for window in ("masked_ms", "masked_ms_again"):
                ctx.set_active_tiles(sel)
                e[window] = stream_ms(torch, stream, lambda: ctx.render(2, rfk), a.calls, a.warmup)
                ctx.set_active_tiles(None)
                e[window.replace("masked", "full")] = stream_ms(torch, stream, lambda: ctx.render(2, rfk), a.calls, a.warmup)
            # the refined state as the call leaves it, for the second reproject
            one_frame_at_b(ctx)
            ctx.set_active_tiles(sel)
            ctx.render(2, rfk)
            ctx.set_active_tiles(None)
            e["second_reproject_ms"] = stream_ms(torch, stream, ctx.reproject, a.calls, a.warmup)
            m = min(e["masked_ms"]["median"], e["masked_ms_again"]["median"])
            f = min(e["full_ms"]["median"], e["full_ms_again"]["median"])
            e["masked_over_full"] = round(m / f, 4)
            e["masked_over_k_one_frame_launches"] = round(m / (k * res["render_one_frame_ms"]["median"]), 4)
            res["extra"][str(k)] = e
        one_frame_at_b(ctx)
        res["render_one_frame_ms_again"] = stream_ms(torch, stream, lambda: ctx.render(1, rf1), a.calls, a.warmup)

        # the sync and the readback: the records against the whole result
        ctx.reproject()

        def records():
            ctx.reach_tiles(4.0)
            return ctx.read_tile_reach()

        res["readback_wall_ms"] = {"reach_tiles_and_read_tile_reach": wall_ms(records, a.wall_calls, 2),
                                   "read_reprojected": wall_ms(ctx.read_reprojected, a.wall_calls, 2)}
        res["readback_bytes"] = {"read_tile_reach": nt * 16, "read_reprojected": px * 16}
        ctx.close()

        # a whole pose, back and forth between the two cameras, each call followed by rt_sync
        def poses(k):
            c = at_a()
            cams = [cam_b, cam_a]
            state = {"i": 0, "tiles": []}
            rf = np.ascontiguousarray(rtamd.frame_rand_factors(1, 0, 1 + k), np.float32)
            prm = _lib.RtRefineParams()
            prm.extra_frames = k
            tiles = ctypes.c_int()

            def call():
                cam = np.ascontiguousarray(cams[state["i"] % 2], np.float32)
                state["i"] += 1
                fp = _lib.c_float_p
                if k:
                    c._check(c._L.rt_render_moved_refined(c._h, cam.ctypes.data_as(fp), 1, rf.ctypes.data_as(fp), ctypes.byref(prm),
                                                          None, None, None, None, ctypes.byref(tiles)))
                    state["tiles"].append(tiles.value)
                else:
                    c._check(c._L.rt_render_moved(c._h, cam.ctypes.data_as(fp), 1, rf.ctypes.data_as(fp), None, None, None, None))
                c.sync()

            out = wall_ms(call, a.wall_calls, 2)
            if k:
                out["tiles_refined"] = state["tiles"][2:]
            c.close()
            return out

        res["pose_wall_ms"] = {"render_moved": poses(0)}
        for k in EXTRA:
            res["pose_wall_ms"][f"render_moved_refined_{k}"] = poses(k)
        res["pose_wall_ms"]["render_moved_again"] = poses(0)
    res["masked_below_full_for_every_k"] = bool(all(e["masked_over_full"] < 1.0 for e in res["extra"].values()))
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What reprojecting the misses by direction costs and what it saves (rt.h rt_set_reproject_misses) at 1920x1080 on
scene 8 after a 0.05-viewport move, by tools/reproject_cost.py's method: device time between two events on the
context's stream, medians of two windows of calls.

1. The four reproject instances (reproject_kernel, reproject_miss_kernel, and the two that carry the variance) beside
   a one-frame full rt_render timed the same way on the same context in the same run -- the yardstick.
2. With the switch off and on (tools/refine_cost.py's measurements): the tiles rt_refine_select chooses for
   K in {1, 3, 7} extra frames, the masked K-frame rt_render over them against the unmasked K-frame launch, and the
   wall time of a whole pose through rt_render_moved and through rt_render_moved_refined, each followed by rt_sync,
   the camera going back and forth between the two poses.  With the switch on the selection is a small share of the
   tiles: the masked launch's cost there is written down whichever way it falls.

    python tools/reproject_miss_cost.py [--out profiles/reproject_miss_cost.json]
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
    res = {"tool": "reproject_miss_cost",
           "timing": "device events on the context's stream around each call; wall times with rt_sync",
           "config": {k: getattr(a, k) for k in ("scene", "width", "height", "frames", "shift", "calls", "warmup", "wall_calls")}}
    scene = rtamd.Scene(a.scene, a.width, a.height, seed=1)
    cam_a = scene.camera.copy()
    cam_b = cam_a.copy()
    v = cam_b[12:15] * np.float32(a.shift * a.width)
    cam_b[4:7] += v
    cam_b[8:11] += v
    rf1 = rtamd.frame_rand_factors(1, 0, 1)

    def at_a(variance, misses):
        ctx = rtamd.RenderContext()
        ctx.upload_scene(scene)
        ctx.set_params(max_depth=5, spp=a.frames)
        ctx.resize(a.width, a.height)
        ctx.set_stream(stream.cuda_stream)
        ctx.set_moments(True)
        ctx.set_history_variance(variance)
        ctx.set_reproject_misses(misses)
        ctx.render(1, rtamd.frame_rand_factors(1, 0, a.frames))
        ctx.render_features()
        return ctx

    def moved(ctx):
        ctx.history_capture()
        ctx.set_camera(cam_b)
        ctx.render(1, rf1)
        ctx.render_features()

    with torch.cuda.stream(stream):
        # 1. the four instances and the yardstick, one context after the other in one run
        inst = {}
        for variance in (False, True):
            ctx = at_a(variance, False)
            moved(ctx)
            key = "render_one_frame_ms" + ("_with_variance_context" if variance else "")
            res[key] = stream_ms(torch, stream, lambda: ctx.render(1, rf1), a.calls, a.warmup)
            ctx.render_features()
            for misses in (False, True, False, True):        # off, on, and both again: four windows interleaved
                ctx.set_reproject_misses(misses)
                name = "reproject" + ("_miss" if misses else "") + ("_var" if variance else "") + "_kernel"
                inst.setdefault(name, []).append(stream_ms(torch, stream, ctx.reproject, a.calls, a.warmup))
            res[key + "_again"] = stream_ms(torch, stream, lambda: ctx.render(1, rf1), a.calls, a.warmup)
            if not variance:
                ctx.render_features()
                ctx.set_reproject_misses(False)
                ctx.reproject()
                off = ctx.read_reprojected()
                ctx.set_reproject_misses(True)
                ctx.reproject()
                on = ctx.read_reprojected()
                _, _, ids = ctx.read_features()
                miss = ids == 0xFFFFFFFF
                res["pixels"] = {"all": px, "miss": int(miss.sum()),
                                 "count_did_not_grow_off": int((off[..., 3] <= 1.0).sum()),
                                 "count_did_not_grow_on": int((on[..., 3] <= 1.0).sum())}
            ctx.close()
        res["instances_ms"] = {k: {"windows": w, "lower_median": min(x["median"] for x in w),
                                   "higher_median": max(x["median"] for x in w)} for k, w in inst.items()}
        res["reproject_every_tap_ms"] = round(px * 256 / HBM_BYTES_PER_S * 1e3, 5)
        res["reproject_byte_floor_ms"] = round(px * 64 / HBM_BYTES_PER_S * 1e3, 5)

        # 2. the refinement with the switch off and on
        res["refine"] = {}
        for misses in (False, True):
            r = {}
            ctx = at_a(True, misses)
            moved(ctx)
            ctx.reproject()
            nt = int(ctx.read_tile_frames().size)
            r["tiles"] = nt
            r["render_one_frame_ms"] = stream_ms(torch, stream, lambda: ctx.render(1, rf1), a.calls, a.warmup)
            r["extra"] = {}
            for k in EXTRA:
                ctx.set_active_tiles(None)
                ctx.render(1, rf1)
                ctx.reproject()
                ctx.reach_tiles(float(1 + k))                   # the automatic count of a 1-frame pose
                reach = ctx.read_tile_reach()
                sel = rtamd.refine_select(reach)
                rfk = rtamd.frame_rand_factors(1, 1, k)
                e = {"min_count": 1 + k, "tiles_selected": int(sel.sum()), "share_of_tiles": round(float(sel.mean()), 5),
                     "short_pixels": int(reach["short_px"].sum()),
                     "share_of_pixels_short": round(float(reach["short_px"].sum()) / px, 5)}
                if sel.any():
                    # (frames 2 .. 1 + k again and again: only the time is read)
                    for window in ("masked_ms", "masked_ms_again"):
                        ctx.set_active_tiles(sel)
                        e[window] = stream_ms(torch, stream, lambda: ctx.render(2, rfk), a.calls, a.warmup)
                        ctx.set_active_tiles(None)
                        e[window.replace("masked", "full")] = stream_ms(torch, stream, lambda: ctx.render(2, rfk), a.calls, a.warmup)
                    m = min(e["masked_ms"]["median"], e["masked_ms_again"]["median"])
                    f = min(e["full_ms"]["median"], e["full_ms_again"]["median"])
                    e["masked_over_full"] = round(m / f, 4)
                    e["masked_over_k_one_frame_launches"] = round(m / (k * r["render_one_frame_ms"]["median"]), 4)
                    e["masked_ms_per_selected_tile_share"] = round(m / f / max(float(sel.mean()), 1e-9), 4)
                r["extra"][str(k)] = e
            ctx.set_active_tiles(None)
            ctx.close()

            # a whole pose, back and forth between the two cameras, each call followed by rt_sync
            def poses(k):
                c = at_a(True, misses)
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
                        c._check(c._L.rt_render_moved_refined(c._h, cam.ctypes.data_as(fp), 1, rf.ctypes.data_as(fp),
                                                              ctypes.byref(prm), None, None, None, None, ctypes.byref(tiles)))
                        state["tiles"].append(tiles.value)
                    else:
                        c._check(c._L.rt_render_moved(c._h, cam.ctypes.data_as(fp), 1, rf.ctypes.data_as(fp), None, None, None, None))
                    c.sync()

                out = wall_ms(call, a.wall_calls, 2)
                if k:
                    out["tiles_refined"] = state["tiles"][2:]
                c.close()
                return out

            r["pose_wall_ms"] = {"render_moved": poses(0)}
            for k in EXTRA:
                r["pose_wall_ms"][f"render_moved_refined_{k}"] = poses(k)
            r["pose_wall_ms"]["render_moved_again"] = poses(0)
            res["refine"]["on" if misses else "off"] = r
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

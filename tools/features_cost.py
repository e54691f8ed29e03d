#!/usr/bin/env python3
"""What the first-hit pass costs (rt.h rt_render_features) at 1920x1080 on scene 8: the host wall time
of rt_render_features + rt_sync (medians of two windows of calls), beside a one-frame rt_render launch
+ rt_sync in the same session (the yardstick: the pass traces one ray per pixel and shades nothing);
a guided rt_denoise_guided call beside an unguided rt_denoise after a 16-frame render; and, from a
profiler run of the same command, the kernels.

    python tools/features_cost.py [--out profiles/features_cost.json]
    rocprofv3 --kernel-trace --stats -d <dir> -o ft --output-format csv -- python tools/features_cost.py --calls 10
    python tools/features_cost.py --merge <dir>/.../ft_kernel_stats.csv --out profiles/features_cost.json   # no device

The byte floor of the pass is its 32 bytes of output per pixel.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-book_amd"))

HBM_BYTES_PER_S = 6.3e12   # achievable streaming rate of the MI355X's HBM


def wall_ms(ctx, call, calls, warmup):
    ms = []
    for k in range(warmup + calls):
        ctx.sync()
        t = time.perf_counter()
        call()
        ctx.sync()
        dt = (time.perf_counter() - t) * 1e3
        if k >= warmup:
            ms.append(dt)
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "calls": len(ms)}


def merge(path):
    """rocprofv3's kernel stats CSV -> the pass's, the filter's and the render's kernels."""
    keys = ("features_kernel", "dn_prologue_kernel", "dn_vb_kernel", "dn_filter_guided_kernel", "dn_filter_kernel",
            "render_persistent", "fold_moments_kernel", "fold_pixels_kernel")
    out = {}
    for row in csv.DictReader(open(path)):
        name = row["Name"]
        short = next((k for k in keys if k in name), None)
        if short is None:
            continue
        if short.startswith("dn_filter") and "<" in name:
            short += name[name.index("<"):name.index(">") + 1]   # <final>
        if short in out:   # several instances of one template: keep them apart
            short = f"{short}#{sum(1 for k in out if k.startswith(short))}"
        out[short] = {"calls": int(row["Calls"]), "avg_ms": round(float(row["AverageNs"]) * 1e-6, 5),
                      "min_ms": round(float(row["MinNs"]) * 1e-6, 5), "max_ms": round(float(row["MaxNs"]) * 1e-6, 5),
                      "total_ms": round(float(row["TotalDurationNs"]) * 1e-6, 4)}
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--scene", type=int, default=8)
    p.add_argument("--width", type=int, default=1920)
    p.add_argument("--height", type=int, default=1080)
    p.add_argument("--frames", type=int, default=16)
    p.add_argument("--calls", type=int, default=50)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--merge", default=None, help="a rocprofv3 kernel stats CSV of this command: add its figures to --out (no device)")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if a.merge:
        res = json.load(open(a.out))
        res["kernels"] = merge(a.merge)
        res["kernels_note"] = "rocprofv3 --kernel-trace --stats over a run of this tool, in a run of its own"
    else:
        import rtamd
        scene = rtamd.Scene(a.scene, a.width, a.height, seed=1)
        ctx = rtamd.RenderContext()
        ctx.upload_scene(scene)
        ctx.set_params(max_depth=5, spp=a.frames)
        ctx.resize(a.width, a.height)
        px = a.width * a.height
        res = {"tool": "features_cost", "config": {k: getattr(a, k) for k in ("scene", "width", "height", "frames", "calls", "warmup")}}
        rf1 = rtamd.frame_rand_factors(1, 0, 1)
        # the yardstick first and again last: a one-frame launch (frame 1 every time) + rt_sync
        res["render_one_frame_wall_ms"] = wall_ms(ctx, lambda: ctx.render(1, rf1), a.calls, a.warmup)
        res["features_wall_ms"] = wall_ms(ctx, ctx.render_features, a.calls, a.warmup)
        res["features_wall_ms_again"] = wall_ms(ctx, ctx.render_features, a.calls, a.warmup)   # the spread between two windows
        res["render_one_frame_wall_ms_again"] = wall_ms(ctx, lambda: ctx.render(1, rf1), a.calls, a.warmup)
        # the filter, unguided beside guided (the default guides), after a render with the moments on
        ctx.set_moments(True)
        ctx.render(1, rtamd.frame_rand_factors(1, 0, a.frames))
        ctx.sync()
        L, h = ctx._L, ctx._h
        res["denoise_wall_ms"] = wall_ms(ctx, lambda: L.rt_denoise(h, None), a.calls, a.warmup)
        res["denoise_guided_wall_ms"] = wall_ms(ctx, lambda: L.rt_denoise_guided(h, None, None), a.calls, a.warmup)
        res["denoise_wall_ms_again"] = wall_ms(ctx, lambda: L.rt_denoise(h, None), a.calls, a.warmup)
        nd, alb, ids = ctx.read_features()
        res["hit_pixels"] = int((ids != 0xFFFFFFFF).sum())
        ctx.close()
        res["features_byte_floor_ms"] = round(px * 32 / HBM_BYTES_PER_S * 1e3, 5)
        res["features_bytes_per_pixel"] = 32
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

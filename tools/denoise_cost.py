#!/usr/bin/env python3
"""What the preview filter costs (rt.h rt_denoise) at 1920x1080: the host wall time of one rt_denoise
(the call plus rt_sync, no read-back) after a 16-frame render of scene 8 with the moments on, for the
defaults and for each number of levels; and, from a profiler run of the same command, its kernels.

    python tools/denoise_cost.py [--out profiles/denoise_cost.json]
    rocprofv3 --kernel-trace --stats -d <dir> -o dn --output-format csv -- python tools/denoise_cost.py --calls 10 --no-sweep
    python tools/denoise_cost.py --merge <dir>/.../dn_kernel_stats.csv --out profiles/denoise_cost.json   # no device

The byte floor is one 16-byte read and one 16-byte write per pixel per level.  bench.py stays the
yardstick of the flagship number; with the filter never called the render path is the parent's.
"""
import argparse
import csv
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-book_amd"))

HBM_BYTES_PER_S = 6.3e12   # achievable streaming rate of the MI355X's HBM


def wall_ms(ctx, params, calls, warmup):
    L, h = ctx._L, ctx._h
    ms = []
    for k in range(warmup + calls):
        ctx.sync()
        t = time.perf_counter()
        rc = L.rt_denoise(h, params)
        ctx.sync()
        dt = (time.perf_counter() - t) * 1e3
        assert rc == 0, rc
        if k >= warmup:
            ms.append(dt)
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "calls": len(ms)}


def merge(path):
    """rocprofv3's kernel stats CSV -> the filter's kernels: calls, average and total time."""
    out = {}
    for row in csv.DictReader(open(path)):
        name = row["Name"]
        if "dn_" not in name and "fold_moments" not in name and "fold_pixels" not in name:
            continue
        short = next(k for k in ("dn_prologue_kernel", "dn_vb_kernel", "dn_filter_kernel", "fold_moments_kernel", "fold_pixels_kernel") if k in name)
        if "<" in name and short.startswith("dn_filter"):
            short += name[name.index("<"):name.index(">") + 1]   # <final>
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
    p.add_argument("--no-sweep", action="store_true", help="only the defaults (a profiler run: the kernels of levels 3)")
    p.add_argument("--merge", default=None, help="a rocprofv3 kernel stats CSV of this command: add its figures to --out (no device)")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if a.merge:
        res = json.load(open(a.out))
        res["kernels"] = merge(a.merge)
        res["kernels_note"] = "rocprofv3 --kernel-trace --stats over a run of this tool (--no-sweep: the defaults' three levels)"
    else:
        import rtamd
        from rtamd import _lib
        scene = rtamd.Scene(a.scene, a.width, a.height, seed=1)
        ctx = rtamd.RenderContext()
        ctx.upload_scene(scene)
        ctx.set_params(max_depth=5, spp=a.frames)
        ctx.resize(a.width, a.height)
        ctx.set_moments(True)
        ctx.render(1, rtamd.frame_rand_factors(1, 0, a.frames))
        ctx.sync()
        px = a.width * a.height
        res = {"tool": "denoise_cost", "config": {k: getattr(a, k) for k in ("scene", "width", "height", "frames", "calls", "warmup")},
               "levels_wall_ms": {}}
        res["defaults_wall_ms"] = wall_ms(ctx, None, a.calls, a.warmup)
        res["defaults_wall_ms_again"] = wall_ms(ctx, None, a.calls, a.warmup)   # the spread between two windows
        for levels in (() if a.no_sweep else (1, 2, 3, 4, 5)):
            prm = _lib.RtDenoiseParams()
            prm.levels, prm.k = levels, 3.0
            res["levels_wall_ms"][str(levels)] = wall_ms(ctx, ctypes.byref(prm), a.calls, a.warmup)
        ctx.close()
        res["byte_floor_ms_per_level"] = round(px * 32 / HBM_BYTES_PER_S * 1e3, 5)
        res["byte_floor_ms_defaults"] = round(3 * px * 32 / HBM_BYTES_PER_S * 1e3, 5)
        res["parent_fold_moments_kernel_ms"] = 0.233
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

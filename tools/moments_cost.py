#!/usr/bin/env python3
"""What the per-pixel sample moments cost (rt.h rt_set_moments, rt_noise), on the benchmark's own
shape: scene 8, 1920x1080, 64 frames per step, depth 5 (bench.py preset c3).

Three figures, each the median device time of a step (rt_last_render_ns: the render kernel and
its fold) over --steps steps after --warmup:
  off      moments off (run twice, `off` and `off_again`, so the run-to-run spread is known)
  on       moments on: every launch staged and folded with the moments (fold_pixels_kernel<true>)
  noise    host time of one rt_noise() after a step (tile sums kernel + readback + the host sum)

    python tools/moments_cost.py [--out profiles/moments_cost.json]
    python tools/moments_cost.py --lib <a previous revision's librtamd.so> --modes off   # the parent's figure
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/moments_cost.py --modes on # fold kernels' times

bench.py stays the yardstick of the flagship number; this tool only attributes the feature's cost.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-book_amd"))


def measure(rtamd, args, moments, lib=None):
    scene = rtamd.Scene(args.scene, args.width, args.height, seed=args.seed)
    ctx = rtamd.RenderContext(devices=(args.device,), lib=lib)
    ctx.upload_scene(scene)
    ctx.set_params(max_depth=args.depth, spp=args.spp_total)
    ctx.resize(args.width, args.height)
    if moments:
        ctx.set_moments(True)
    F = args.frames_per_step
    factors = rtamd.frame_rand_factors(args.seed, 0, F * (args.warmup + args.steps))
    step_ms, noise_ms, noise = [], [], None
    frame = 1
    for k in range(args.warmup + args.steps):
        ctx.render(frame, factors[frame - 1:frame - 1 + F])
        frame += F
        ctx.sync()
        ms = ctx.last_render_ns() * 1e-6
        if moments:
            t = time.perf_counter()
            noise = ctx.noise()
            dt = (time.perf_counter() - t) * 1e3
        if k >= args.warmup:
            step_ms.append(ms)
            if moments:
                noise_ms.append(dt)
    launch = ctx.last_launch()
    ctx.close()
    out = {"step_ms_median": round(statistics.median(step_ms), 4), "step_ms_min": round(min(step_ms), 4),
           "step_ms_max": round(max(step_ms), 4), "steps": len(step_ms),
           "staged": launch["staged"], "chunks": launch["chunks"]}
    if moments:
        out.update({"noise_call_ms_median": round(statistics.median(noise_ms), 4),
                    "noise_call_ms_min": round(min(noise_ms), 4), "noise_call_ms_max": round(max(noise_ms), 4),
                    "noise_after_last_step": noise["noise"], "frames": noise["frames"], "bad_pixels": noise["bad"]})
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--scene", type=int, default=8)
    p.add_argument("--width", type=int, default=1920)
    p.add_argument("--height", type=int, default=1080)
    p.add_argument("--spp-total", type=int, default=4096)
    p.add_argument("--frames-per-step", type=int, default=64)
    p.add_argument("--depth", type=int, default=5)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--steps", type=int, default=8)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--modes", default="off,on,off_again", help="comma-separated: off, on, off_again")
    p.add_argument("--lib", default=None, help="another build of librtamd.so (a previous revision: modes off only)")
    p.add_argument("--out", default=None, help="also write the JSON here")
    args = p.parse_args()
    import rtamd
    res = {"tool": "moments_cost", "config": {k: getattr(args, k) for k in
                                               ("scene", "width", "height", "spp_total", "frames_per_step", "depth",
                                                "seed", "steps", "warmup")},
           "lib": "other" if args.lib else "this"}
    for mode in [m for m in args.modes.split(",") if m]:
        if mode not in ("off", "on", "off_again"):
            p.error(f"unknown mode {mode}")
        res[mode] = measure(rtamd, args, mode == "on", lib=args.lib)
    if "off" in res and "on" in res:
        res["on_minus_off_ms"] = round(res["on"]["step_ms_median"] - res["off"]["step_ms_median"], 4)
        res["on_over_off"] = round(res["on"]["step_ms_median"] / res["off"]["step_ms_median"], 5)
    if "off" in res and "off_again" in res:
        res["off_spread_ms"] = round(abs(res["off"]["step_ms_median"] - res["off_again"]["step_ms_median"]), 4)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

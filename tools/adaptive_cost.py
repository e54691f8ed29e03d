#!/usr/bin/env python3
"""What tile masks and the adaptive loop cost and save (rt.h rt_set_active_tiles, rt_render_adaptive),
on the benchmark's shape: 1920x1080, 64 frames per step, depth 5 (bench.py preset c3 is scene 8).

Four parts, each figure a device time (rt_last_render_ns: the render kernel and its fold) unless
it says wall:
  default   ms per step without a mask, this library against --parent-lib (a build of the parent
            commit), the two sides alternating, --runs runs each (fresh context, mean over --steps
            steps after --warmup); bar: this mean <= parent mean + the parent's own max - min
  all_ones  the list path with every tile active against no mask, same library, alternating
  sparse    50 / 10 / 1 % of the tiles active, at random and as one compact block: ms per launch
            and Msamples/s over the sampled pixels
  end2end   the noise rt_render_until reaches at 256 frames as the target; then rt_render_until
            and rt_render_adaptive(min_frames 16, batch 16) to that target: frames, samples, wall
            time, final rt_noise; and the adaptive loop run from its primitives with rt_noise read
            after each batch: where the image-level figure first reaches the target

    python tools/adaptive_cost.py --scene 8 [--parent-lib <librtamd.so of the parent>] [--out <json>]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-book_amd"))


def new_context(rtamd, args, scene, lib=None, moments=False):
    ctx = rtamd.RenderContext(devices=(args.device,), lib=lib)
    ctx.upload_scene(scene)
    ctx.set_params(max_depth=args.depth, spp=args.spp_total)
    ctx.resize(args.width, args.height)
    if moments:
        ctx.set_moments(True)
    return ctx


def steps_ms(rtamd, args, ctx, n_steps, warmup):
    """Device ms of each of n_steps launches of frames_per_step frames (after warmup), frames going on."""
    F = args.frames_per_step
    out, frame = [], 1
    for k in range(warmup + n_steps):
        ctx.render(frame, rtamd.frame_rand_factors(args.seed, frame - 1, F))
        frame += F
        ctx.sync()
        if k >= warmup:
            out.append(ctx.last_render_ns() * 1e-6)
    return out


def spread(v):
    return {"mean": round(statistics.mean(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "runs": [round(x, 4) for x in v]}


def part_default(rtamd, args, scene):
    sides = [("this", None)] + ([("parent", args.parent_lib)] if args.parent_lib else [])
    runs = {name: [] for name, _ in sides}
    for r in range(args.runs):
        for name, lib in (sides if r % 2 == 0 else sides[::-1]):   # alternate, and who goes first
            ctx = new_context(rtamd, args, scene, lib=lib)
            runs[name].append(statistics.mean(steps_ms(rtamd, args, ctx, args.steps, args.warmup)))
            ctx.close()
    out = {name: spread(v) for name, v in runs.items()}
    if "parent" in out:
        p = out["parent"]
        out["bar_ms"] = round(p["mean"] + (p["max"] - p["min"]), 4)
        out["this_over_parent"] = round(out["this"]["mean"] / p["mean"], 5)
        out["meets_bar"] = bool(out["this"]["mean"] <= out["bar_ms"])
    return out


def part_all_ones(rtamd, args, scene, n_tiles):
    runs = {"no_mask": [], "all_ones": []}
    order = ["no_mask", "all_ones"]
    for r in range(args.runs):
        for name in (order if r % 2 == 0 else order[::-1]):
            ctx = new_context(rtamd, args, scene)
            if name == "all_ones":
                ctx.set_active_tiles(np.ones(n_tiles, np.uint8))
            runs[name].append(statistics.mean(steps_ms(rtamd, args, ctx, args.steps, args.warmup)))
            assert ctx.last_launch()["tiles_active"] == n_tiles
            ctx.close()
    out = {name: spread(v) for name, v in runs.items()}
    out["all_ones_minus_no_mask_ms"] = round(out["all_ones"]["mean"] - out["no_mask"]["mean"], 4)
    return out


def tile_pixels(args, tx):
    """Pixels of each tile of the image (partial tiles at the right and bottom edges)."""
    ty = (args.height + 7) // 8
    w = np.minimum(8, args.width - 8 * np.arange(tx))
    h = np.minimum(8, args.height - 8 * np.arange(ty))
    return (h[:, None] * w[None, :]).ravel()


def part_sparse(rtamd, args, scene, tx, ty):
    n_tiles = tx * ty
    px = tile_pixels(args, tx)
    rng = np.random.default_rng(args.seed)
    F = args.frames_per_step
    ctx = new_context(rtamd, args, scene)
    full = statistics.median(steps_ms(rtamd, args, ctx, args.steps, args.warmup))
    out = {"full": {"ms": round(full, 4), "msamples_per_s": round(args.width * args.height * F / full * 1e-3, 1)}}
    for frac in (0.5, 0.1, 0.01):
        k = max(1, round(frac * n_tiles))
        rnd = np.zeros(n_tiles, np.uint8)
        rnd[rng.choice(n_tiles, k, replace=False)] = 1
        bw = min(tx, max(1, round((k * tx / ty) ** 0.5)))   # one block of the image's aspect, centred
        bh = min(ty, max(1, round(k / bw)))
        blk = np.zeros((ty, tx), np.uint8)
        blk[(ty - bh) // 2:(ty - bh) // 2 + bh, (tx - bw) // 2:(tx - bw) // 2 + bw] = 1
        for name, mask in (("random", rnd), ("block", blk.ravel())):
            ctx.set_active_tiles(mask)
            ms = statistics.median(steps_ms(rtamd, args, ctx, args.steps, args.warmup))
            ll = ctx.last_launch()
            assert ll["tiles_active"] == int(mask.sum())
            samples = int(px[mask.astype(bool)].sum()) * F
            out[f"{name}_{frac:g}"] = {"tiles": int(mask.sum()), "ms": round(ms, 4), "chunks": ll["chunks"],
                                       "msamples_per_s": round(samples / ms * 1e-3, 1),
                                       "rate_over_full": round(samples / ms / (args.width * args.height * F / full), 4)}
    ctx.close()
    return out


def part_end2end(rtamd, args, scene, tx):
    px = tile_pixels(args, tx)
    ctx = new_context(rtamd, args, scene, moments=True)
    _, st = ctx.render_until(0.0, 256, 16, seed=args.seed)
    target = float(np.nextafter(np.float32(st["noise"]), np.float32(np.inf)))   # the ABI's float, not below it
    ctx.close()
    out = {"target_noise": target, "noise_at_256": st["noise"]}
    for name in ("until", "adaptive", "until_again", "adaptive_again"):
        ctx = new_context(rtamd, args, scene, moments=True)
        ctx.render(1, rtamd.frame_rand_factors(args.seed, 0, 1))   # first-launch costs stay out of the wall time
        ctx.sync()
        t = time.perf_counter()
        if name.startswith("until"):
            done, st = ctx.render_until(target, args.cap, 16, seed=args.seed)
        else:
            done, st = ctx.render_adaptive(target, args.cap, 16, min_frames=16, seed=args.seed)
        wall = (time.perf_counter() - t) * 1e3
        counts = ctx.read_tile_frames()
        ctx.close()
        out[name] = {"frames": done, "samples": int((px * counts.astype(np.int64)).sum()), "wall_ms": round(wall, 3),
                     "noise": st["noise"], "converged": st["converged"],
                     "tiles_by_frames": {str(int(v)): int(n) for v, n in zip(*np.unique(counts, return_counts=True))}
                     if name.startswith("adaptive") else None}
    # rt_render_adaptive stops when every tile meets the limit on its own, which is stricter than the
    # image-level figure rt_render_until stops at.  The same loop from its primitives, reading rt_noise
    # after each batch: where the image-level figure first reaches the target (wall time up to there,
    # the extra rt_noise calls included).
    for name in ("adaptive_to_image_target", "adaptive_to_image_target_again"):
        ctx = new_context(rtamd, args, scene, moments=True)
        ctx.render(1, rtamd.frame_rand_factors(args.seed, 0, 1))
        ctx.sync()
        active = np.ones(px.size, np.uint8)
        done, hit = 0, None
        t = time.perf_counter()
        while done < args.cap and active.any():
            ctx.set_active_tiles(None if active.all() else active)
            ctx.render(done + 1, rtamd.frame_rand_factors(args.seed, done, 16))
            done += 16
            st = ctx.noise()
            if st["noise"] <= target:
                hit = (time.perf_counter() - t) * 1e3
                break
            active = rtamd.adaptive_select(ctx.tile_sums(), active, done, 16, target)
        counts = ctx.read_tile_frames()
        ctx.close()
        out[name] = {"frames": done, "samples": int((px * counts.astype(np.int64)).sum()),
                     "wall_ms": None if hit is None else round(hit, 3), "noise": st["noise"], "reached": hit is not None}
    u = min(out["until"]["wall_ms"], out["until_again"]["wall_ms"])
    r = [out[k]["wall_ms"] for k in ("adaptive_to_image_target", "adaptive_to_image_target_again") if out[k]["reached"]]
    if r:
        out["speedup_wall_to_image_target"] = round(u / min(r), 4)
        out["samples_ratio_to_image_target"] = round(out["adaptive_to_image_target"]["samples"] / out["until"]["samples"], 4)
    a = min(out["adaptive"]["wall_ms"], out["adaptive_again"]["wall_ms"])
    out["speedup_wall"] = round(u / a, 4)
    out["samples_ratio"] = round(out["adaptive"]["samples"] / out["until"]["samples"], 4)
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
    p.add_argument("--steps", type=int, default=6)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--runs", type=int, default=3, help="runs of each side (alternating)")
    p.add_argument("--cap", type=int, default=2048, help="end2end: the frame cap of both loops")
    p.add_argument("--parts", default="default,all_ones,sparse,end2end")
    p.add_argument("--parent-lib", default=None, help="librtamd.so built from the parent commit")
    p.add_argument("--out", default=None, help="also write (merge by scene into) this JSON file")
    args = p.parse_args()
    import rtamd
    scene = rtamd.Scene(args.scene, args.width, args.height, seed=args.seed)
    tx, ty = (args.width + 7) // 8, (args.height + 7) // 8
    res = {"tool": "adaptive_cost", "config": {k: getattr(args, k) for k in
                                                ("scene", "width", "height", "spp_total", "frames_per_step", "depth",
                                                 "seed", "steps", "warmup", "runs", "cap")}}
    parts = [x for x in args.parts.split(",") if x]
    if "default" in parts:
        res["default"] = part_default(rtamd, args, scene)
    if "all_ones" in parts:
        res["all_ones"] = part_all_ones(rtamd, args, scene, tx * ty)
    if "sparse" in parts:
        res["sparse"] = part_sparse(rtamd, args, scene, tx, ty)
    if "end2end" in parts:
        res["end2end"] = part_end2end(rtamd, args, scene, tx)
    print(json.dumps(res), flush=True)
    if args.out:
        merged = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                merged = json.load(f)
        merged[f"scene{args.scene}"] = res
        with open(args.out, "w") as f:
            f.write(json.dumps(merged, indent=1) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What rendering the moved view to a noise target (rt_render_moved_to_noise) is worth, measured on the CPU with
the oracle and the host functions: tools/refine_quality.py's experiment (64 oracle frames at camera A, a
quarter-viewport move, 1 frame at camera B) on scenes 6 and 8 at its two sizes.  The masked rounds are emulated tile
by tile: a tile that holds c frames takes image and moments from a plain oracle render of c frames at B (a stopped
tile holds the bits of a plain render: rt.h, tests/test_gpu_noise_refine.py); each round reprojects with the variance,
reduces with rt_tile_noise_host at min_count 2 and selects with rt_refine_noise_select, batch_frames 1, 4 rounds at most.

Against a 1024-frame render at B with another seed, the RMS error of y = (r + g) + b of the RT_PRESENT_MOVED
composite, over the pixels fresh before any refinement and over the whole image, of
  the plain pose,
  the pose rendered to each target,
  the count criterion (rt_tile_reach_host at the automatic count n + k, rt_refine_select, k extra frames) at the k in
  1 .. 8 whose tile-frames k * T come nearest the noise criterion's, and
  a plain pose of equal samples: n + floor and n + ceil of tile-frames / tiles frames on every tile.
Whatever comes out is written down, also where the noise target does not win.

    python tools/noise_refine_quality.py [--out profiles/noise_refine_quality.json]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import refine_quality as RQ  # noqa: E402  (puts the package, the oracle and tests/ on the path)
import reproject_filter_quality as RF  # noqa: E402
import reproject_quality as Q  # noqa: E402
import pyoracle  # noqa: E402
import rtamd  # noqa: E402

F = np.float32
FRAMES_B, BATCH, ROUNDS, MIN_COUNT = 1, 1, 4, 2.0
TARGETS = (0.5, 0.2, 0.1)
COUNT_EXTRA = range(1, 9)
SCENES = (6, 8)
SIZES = ((32, 32), (128, 128))


def measure(sid, w, h):
    t0 = time.time()
    n = FRAMES_B
    a = Q.scene_at(sid, w, h)
    cam_a = a.camera.copy()
    cam_b = Q.moved_camera(cam_a, w)
    b = Q.scene_at(sid, w, h, cam_b)
    img_a, m2_a = RQ.frames_and_moments(a, RF.FRAMES_A, RF.SEED)
    hnd, hai, _ = Q.features_at(sid, w, h)
    nd, ai, _ = Q.features_at(sid, w, h, cam_b)
    e = dict(hist=rtamd.history_from_image(img_a, RF.FRAMES_A), hnd=hnd, hai=hai, hcam=cam_a, nd=nd, ai=ai, cam=cam_b)
    e["hs2"] = rtamd.history_variance_host(e["hist"], m2_a, RF.FRAMES_A)
    ref = pyoracle.render(pyoracle.OracleScene(b, max_depth=5, spp=RF.REF_FRAMES),
                          rtamd.frame_rand_factors(RF.REF_SEED, 0, RF.REF_FRAMES))
    nt = ((w + 7) // 8) * ((h + 7) // 8)
    plain = {}

    def plain_pose(frames):
        if frames not in plain:
            plain[frames] = RQ.frames_and_moments(b, frames, RF.SEED)
        return plain[frames]

    def by_tiles(tf):
        """Image and moments of tiles that hold tf[t] frames each."""
        per = RQ.per_pixel(tf, w, h)
        image, m2 = np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)
        for c in sorted(set(tf.tolist())):
            ic, mc = plain_pose(c)
            at = (per == c)[..., None]
            image, m2 = np.where(at, ic, image), np.where(at, mc, m2)
        return image, m2

    def reprojected(tf):
        image, m2 = by_tiles(tf)
        return rtamd.reproject_variance_host(e["hist"], e["hnd"], e["hai"], e["hs2"], e["hcam"], image, m2, tf, e["nd"], e["ai"],
                                             e["cam"])

    def composite(tf):
        image, m2 = by_tiles(tf)
        return RQ.composite(e, image, m2, tf)

    tf0 = np.full(nt, n, np.int32)
    comp0, rgbn0 = composite(tf0)
    fresh = rgbn0[..., 3] <= F(n)                       # fresh before any refinement: one mask for every figure

    def rms(x):
        return dict(fresh=round(RF.rms_y(x, ref, fresh), 6), whole=round(RF.rms_y(x, ref), 6))

    rec = dict(width=w, height=h, tiles=nt, pixels=w * h, fresh_pixels=int(fresh.sum()), frames_b=n, rms_plain=rms(comp0),
               targets={})
    # the count criterion at every k: its tiles and its tile-frames
    count = {}
    for k in COUNT_EXTRA:
        sel = rtamd.refine_select(rtamd.tile_reach_host(rgbn0, float(n + k)))
        count[k] = (sel, k * int(sel.sum()))
    for target in TARGETS:
        tf = tf0.copy()
        active = np.ones(nt, np.uint8)
        r, first, spent, per_round = 0, 0, 0, []
        while True:
            rgbn, s2 = reprojected(tf)
            active, stats = rtamd.refine_noise_select(rtamd.tile_noise_host(rgbn, s2, MIN_COUNT), target, active)
            if r == 0:
                noise0 = stats["noise"]
            if not active.any() or r == ROUNDS:
                break
            tf[active == 1] += BATCH
            per_round.append(int(active.sum()))
            first = first or int(active.sum())
            spent += int(active.sum()) * BATCH
            r += 1
        t = dict(rounds=r, converged=int(not active.any()), tiles_first_round=first, tiles_per_round=per_round,
                 tile_frames_spent=spent, samples_per_pixel_spent=round(n + spent / nt, 4), noise_plain=round(noise0, 5),
                 noise_last=round(stats["noise"], 5), rms_to_noise=rms(composite(tf)[0]))
        # the count criterion at the nearest equal cost
        k = min(COUNT_EXTRA, key=lambda q: (abs(count[q][1] - spent), q))
        sel = count[k][0]
        t["count_criterion"] = dict(extra_frames=k, tiles_selected=int(sel.sum()), tile_frames_spent=count[k][1],
                                    rms=rms(composite(np.where(sel == 1, n + k, n).astype(np.int32))[0]))
        lo, hi = n + math.floor(spent / nt), n + math.ceil(spent / nt)
        t["equal_samples_frames"] = dict(floor=lo, ceil=hi)
        t["rms_equal_samples_floor"] = rms(composite(np.full(nt, lo, np.int32))[0])
        t["rms_equal_samples_ceil"] = rms(composite(np.full(nt, hi, np.int32))[0])
        for name, other in (("over_plain", rec["rms_plain"]), ("over_count_criterion", t["count_criterion"]["rms"]),
                            ("over_equal_samples_ceil", t["rms_equal_samples_ceil"])):
            t["to_noise_" + name] = {m: round(t["rms_to_noise"][m] / other[m], 4) if other[m] else None for m in ("fresh", "whole")}
        t["beats_count_criterion_on_whole"] = bool(t["rms_to_noise"]["whole"] < t["count_criterion"]["rms"]["whole"])
        t["beats_equal_samples_on_whole"] = bool(t["rms_to_noise"]["whole"] < t["rms_equal_samples_ceil"]["whole"])
        rec["targets"][str(target)] = t
    rec["cpu_seconds"] = round(time.time() - t0, 1)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "noise_refine_quality.json"))
    ap.add_argument("--scenes", default=",".join(str(s) for s in SCENES))
    ap.add_argument("--sizes", default=",".join(f"{w}x{h}" for w, h in SIZES))
    a = ap.parse_args()
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    rec = dict(what="RMS error of y against a long render at camera B with another seed, over the pixels fresh before any "
                    "refinement (n_out <= frames at B) and over the whole image: the RT_PRESENT_MOVED composite of the plain pose, "
                    "of the pose rendered to a noise target (rt_tile_noise_host at min_count 2, rt_refine_noise_select, the masked "
                    "rounds emulated tile by tile from plain oracle renders), of the count criterion at the nearest equal "
                    "tile-frames and of plain poses of equal samples; oracle frames at one stratification grid, "
                    "tests/features_ref.py features, rt_reproject_variance_host, rt_denoise_reprojected_host, rt_present_host",
               frames_a=RF.FRAMES_A, frames_b=FRAMES_B, batch_frames=BATCH, max_rounds=ROUNDS, min_count=MIN_COUNT,
               spp_grid=RQ.SPP, ref_frames=RF.REF_FRAMES, seed=RF.SEED, ref_seed=RF.REF_SEED, shift=Q.SHIFT, scenes={})
    for sid in (int(s) for s in a.scenes.split(",")):
        rec["scenes"][str(sid)] = {}
        for w, h in sizes:
            rec["scenes"][str(sid)][f"{w}x{h}"] = measure(sid, w, h)
            print(sid, w, h, json.dumps(rec["scenes"][str(sid)][f"{w}x{h}"]), flush=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

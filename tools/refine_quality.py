#!/usr/bin/env python3
"""What the extra frames of rt_render_moved_refined are worth after a camera move, measured on the CPU with the
oracle and the host functions: tools/present_quality.py's experiment (scene 6 at 32x32, 64 oracle frames at
camera A, a quarter-viewport move, 1 frame at camera B), then rt_tile_reach_host and rt_refine_select at the
automatic count n + k, and for k in {1, 3, 7} the refined pose: image, moments and tile counts taken tile by tile
from oracle renders of n and of n + k frames at B (a refined tile holds the bits of a plain n + k-frame render:
rt.h, tests/test_gpu_refine.py), reprojected again, filtered and composed by rt_present_host.

Against a 1024-frame render at B with another seed, the RMS error of y = (r + g) + b over the pixels that were
fresh before the refinement and over the whole image, of
  the composite without refinement,
  the composite with refinement, and
  the equal-cost alternative: a plain pose whose every tile gets the same number of frames.  The refinement
  spends k * T / NT frames per tile on average (T of NT tiles chosen), which is no whole number: the plain pose
  is measured at n + floor(k T / NT) and at n + ceil(k T / NT) frames, the second spending more than the
  refinement does.
Every render uses one stratification grid (spp = SPP), as a context does whose rt_set_params stays put.  The
second size says how the share of tiles chosen and the gain move with the resolution.

    python tools/refine_quality.py [--out profiles/refine_quality.json]
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

import reproject_filter_quality as RF  # noqa: E402  (puts the package, the oracle and tests/ on the path)
import reproject_quality as Q  # noqa: E402
import pyoracle  # noqa: E402
import rtamd  # noqa: E402

F = np.float32
SPP = 16               # the stratification grid of every render here
FRAMES_B = 1
EXTRA = (1, 3, 7)
SIZES = ((32, 32), (128, 128))


def frames_and_moments(scene, frames, seed):
    """(image, M2) over frames 1 .. n at the fixed grid: the oracle's frames folded by rt_moments.hip's update."""
    o = pyoracle.OracleScene(scene, max_depth=5, spp=SPP)
    rf = rtamd.frame_rand_factors(seed, 0, frames)
    H, W = scene.height, scene.width
    mean = np.zeros((H, W, 3), F)
    m2 = np.zeros((H, W, 4), F)
    for f in range(1, frames + 1):
        c = (pyoracle.render(o, rf[f - 1:f], first_frame=f)[..., :3] * F(f)).astype(F)
        nw = ((mean * F(f - 1) + c) / F(f)).astype(F)
        if f > 1:
            m2[..., :3] += (c - mean) * (c - nw)
            ys, yo, yn = [(a[..., 0] + a[..., 1]) + a[..., 2] for a in (c, mean, nw)]
            m2[..., 3] += (ys - yo) * (ys - yn)
        mean = nw
    image = pyoracle.render(o, rf)
    return image, m2


def per_pixel(tiles, w, h):
    tx, ty = (w + 7) // 8, (h + 7) // 8
    return np.repeat(np.repeat(np.asarray(tiles).reshape(ty, tx), 8, axis=0), 8, axis=1)[:h, :w]


def composite(e, image, m2, tf):
    """The pose as presented: reprojected with the variance, filtered at the defaults, composed -> (floats, rgbn)."""
    rgbn, s2 = rtamd.reproject_variance_host(e["hist"], e["hnd"], e["hai"], e["hs2"], e["hcam"], image, m2, tf, e["nd"], e["ai"],
                                             e["cam"])
    den = rtamd.denoise_reprojected_host(rgbn, s2, e["nd"], e["ai"])
    _, comp = rtamd.present_host("moved", reprojected=rgbn, denoised=den, tile_frames=tf, keep_float=True)
    return comp, rgbn


def measure(w, h):
    t0 = time.time()
    sid, n = RF.SCENE, FRAMES_B
    a = Q.scene_at(sid, w, h)
    cam_a = a.camera.copy()
    cam_b = Q.moved_camera(cam_a, w)
    b = Q.scene_at(sid, w, h, cam_b)
    img_a, m2_a = frames_and_moments(a, RF.FRAMES_A, RF.SEED)
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
            image, m2 = frames_and_moments(b, frames, RF.SEED)
            plain[frames] = (image, m2) + composite(e, image, m2, np.full(nt, frames, np.int32))
        return plain[frames]

    image1, m21, comp0, rgbn0 = plain_pose(n)
    fresh = rgbn0[..., 3] <= F(n)                       # fresh before any refinement: one mask for every figure

    def rms(x):
        return dict(fresh=round(RF.rms_y(x, ref, fresh), 6), whole=round(RF.rms_y(x, ref), 6))

    base = rms(comp0)
    rec = dict(width=w, height=h, tiles=nt, pixels=w * h, fresh_pixels=int(fresh.sum()), frames_b=n,
               rms_unrefined=base, extra={})
    for k in EXTRA:
        reach = rtamd.tile_reach_host(rgbn0, float(n + k))
        sel = rtamd.refine_select(reach)
        t = int(sel.sum())
        image_k, m2_k, _, _ = plain_pose(n + k)
        mask = per_pixel(sel, w, h).astype(bool)[..., None]
        tf = np.where(sel == 1, n + k, n).astype(np.int32)
        comp, rgbn = composite(e, np.where(mask, image_k, image1), np.where(mask, m2_k, m21), tf)
        assert (rgbn[..., 3][fresh & mask[..., 0]] == n + k).all()        # the fresh pixels of a refined tile hold n + k frames
        kp = k * t / nt
        lo, hi = n + math.floor(kp), n + math.ceil(kp)
        r = dict(min_count=n + k, tiles_selected=t, share_of_tiles=round(t / nt, 4),
                 short_px=reach["short_px"].tolist() if nt <= 16 else None,
                 fresh_pixels_in_selected_tiles=int((fresh & mask[..., 0]).sum()),
                 samples_per_pixel_spent=round(n + kp, 4), rms_refined=rms(comp),
                 equal_cost_frames=dict(floor=lo, ceil=hi),
                 rms_equal_cost_floor=rms(plain_pose(lo)[2]), rms_equal_cost_ceil=rms(plain_pose(hi)[2]))
        r["refined_over_unrefined"] = {m: round(r["rms_refined"][m] / base[m], 4) for m in ("fresh", "whole")}
        r["refined_over_equal_cost_floor"] = {m: round(r["rms_refined"][m] / r["rms_equal_cost_floor"][m], 4) for m in ("fresh", "whole")}
        r["refined_over_equal_cost_ceil"] = {m: round(r["rms_refined"][m] / r["rms_equal_cost_ceil"][m], 4) for m in ("fresh", "whole")}
        r["refinement_beats_equal_cost_on_fresh"] = bool(r["rms_refined"]["fresh"] < r["rms_equal_cost_ceil"]["fresh"])
        rec["extra"][str(k)] = r
    rec["cpu_seconds"] = round(time.time() - t0, 1)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "refine_quality.json"))
    ap.add_argument("--sizes", default=",".join(f"{w}x{h}" for w, h in SIZES))
    a = ap.parse_args()
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    rec = dict(what="RMS error of y against a long render at camera B with another seed, over the pixels fresh before the "
                    "refinement (n_out <= frames at B) and over the whole image: the RT_PRESENT_MOVED composite of the plain "
                    "pose, of the pose refined on the tiles rt_refine_select chooses from rt_tile_reach_host at min_count "
                    "n + k, and of plain poses of equal cost; oracle frames at one stratification grid, "
                    "tests/features_ref.py features, rt_reproject_variance_host, rt_denoise_reprojected_host, rt_present_host",
               scene=RF.SCENE, frames_a=RF.FRAMES_A, frames_b=FRAMES_B, spp_grid=SPP, ref_frames=RF.REF_FRAMES, seed=RF.SEED,
               ref_seed=RF.REF_SEED, shift=Q.SHIFT, sizes={})
    for w, h in sizes:
        rec["sizes"][f"{w}x{h}"] = measure(w, h)
    print(json.dumps(rec))
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

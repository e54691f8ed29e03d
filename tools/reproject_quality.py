#!/usr/bin/env python3
"""What temporal reprojection is worth after a camera move, measured on the CPU: oracle renders, the
first-hit buffers of tests/features_ref.py at both cameras, and rt_reproject_host.

Scene 6 at 32x32: 64 frames at camera A are the history; the camera moves (camera_pos and up_left shifted by
the same vector, SHIFT viewport widths sideways); 2 frames at camera B are the new view's own image.  Against
a 1024-frame render at B with another seed, the RMS error of y = (r + g) + b of the raw 2-frame image and of
the reprojected one, over a grid of (cos_min, kz, max_history).  The defaults of rt.h (RT_REPROJECT_DEFAULT_*)
are the grid's best setting -- among equal ratios the strictest: the largest cos_min, the smallest kz that is
not 0, the smallest max_history -- and tests/test_gpu_reproject.py repeats the experiment on the device.

    python tools/reproject_quality.py [--out profiles/reproject_quality.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-book_amd"))
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import pyoracle  # noqa: E402
import rtamd  # noqa: E402

F = np.float32
SCENE, W, H = 6, 32, 32
FRAMES_A, FRAMES_B, REF_FRAMES, SEED, REF_SEED = 64, 2, 1024, 1, 2
SHIFT = 0.25   # of the viewport's width, along pixel_delta_u
COS_MIN, KZ, MAX_HISTORY = (0.0, 0.5, 0.9, 0.99), (0.0, 0.02, 0.1, 0.5), (8.0, 16.0, 32.0, 64.0, 128.0)


def moved_camera(ubo, width, shift=SHIFT):
    """The 28-float block with camera_pos and up_left shifted by `shift` viewport widths along pixel_delta_u."""
    cam = np.array(ubo, F)
    v = cam[12:15] * F(shift * width)
    cam[4:7] += v
    cam[8:11] += v
    return cam


def scene_at(sid, w, h, camera=None):
    scene = rtamd.Scene(sid, w, h, seed=SEED)
    if camera is not None:
        scene.override_camera(camera)
    return scene


def oracle_frames(scene, frames, seed):
    return pyoracle.render(pyoracle.OracleScene(scene, max_depth=5, spp=frames), rtamd.frame_rand_factors(seed, 0, frames))


def features_at(sid, w, h, camera=None):
    """(normal_depth, albedo_id, hit) of tests/features_ref.py's CPU first-hit pass, from `camera`."""
    import features_ref
    real = rtamd.Scene   # reference() builds its own Scene: hand it one with this camera

    def scene_with_camera(i, ww, hh, seed=1):
        scene = real(i, ww, hh, seed=seed)
        if camera is not None:
            scene.override_camera(camera)
        return scene

    rtamd.Scene = scene_with_camera
    try:
        ft = features_ref.reference.__wrapped__(sid, w, h)
    finally:
        rtamd.Scene = real
    nd = np.concatenate([ft.N, ft.t[..., None]], -1).astype(F)
    return nd, rtamd.pack_albedo_id(ft.A, ft.id), ft.hit


def rms_y(a, b):
    ya, yb = [(x[..., 0].astype(np.float64) + x[..., 1]) + x[..., 2] for x in (a, b)]
    d = ya - yb
    ok = np.isfinite(d)
    return float(np.sqrt(np.mean(d[ok] ** 2)))


def experiment(sid, w, h, frames_a, frames_b, shift=SHIFT):
    """The host path of one camera move -> dict of the inputs of rt_reproject_host and the raw image at B."""
    a = scene_at(sid, w, h)
    cam_a = a.camera.copy()
    cam_b = moved_camera(cam_a, w, shift)
    img_a = oracle_frames(a, frames_a, SEED)
    hnd, hai, _ = features_at(sid, w, h)
    b = scene_at(sid, w, h, cam_b)
    img_b = oracle_frames(b, frames_b, SEED)
    nd, ai, hit = features_at(sid, w, h, cam_b)
    return dict(hist=rtamd.history_from_image(img_a, frames_a), hnd=hnd, hai=hai, hcam=cam_a, image=img_b, tf=frames_b,
                nd=nd, ai=ai, cam=cam_b, hit=hit, scene_b=b)


def reproject(e, **prm):
    return rtamd.reproject_host(e["hist"], e["hnd"], e["hai"], e["hcam"], e["image"], e["tf"], e["nd"], e["ai"], e["cam"], **prm)


def rejected_share(e, out):
    """The share of hit pixels whose count did not grow: rejected, or never reprojected."""
    return float((out[..., 3][e["hit"]] <= e["tf"]).mean())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "reproject_quality.json"))
    a = ap.parse_args()
    e = experiment(SCENE, W, H, FRAMES_A, FRAMES_B)
    ref = oracle_frames(e["scene_b"], REF_FRAMES, REF_SEED)
    raw = rms_y(e["image"], ref)
    grid = {}
    for cm in COS_MIN:
        for kz in KZ:
            for mh in MAX_HISTORY:
                grid[f"cos_min={cm:g},kz={kz:g},max_history={mh:g}"] = round(rms_y(reproject(e, cos_min=cm, kz=kz, max_history=mh), ref) / raw, 4)

    def strictness(key):
        cm, kz, mh = (float(part.split("=")[1]) for part in key.split(","))
        return (grid[key], -cm, kz == 0.0, kz, mh)

    best = min(grid, key=strictness)
    cm, kz, mh = (float(part.split("=")[1]) for part in best.split(","))
    dflt = reproject(e)   # the library's defaults (NULL params)
    at_defaults = round(rms_y(dflt, ref) / raw, 4)
    rec = dict(what="RMS error of y of the reprojected image / of the raw image at camera B, against a long render at B with "
                    "another seed; oracle frames, tests/features_ref.py features, rt_reproject_host",
               rule="the grid's smallest ratio; among equal ratios the largest cos_min, the smallest kz that is not 0, the "
                    "smallest max_history",
               scene=SCENE, width=W, height=H, frames_a=FRAMES_A, frames_b=FRAMES_B, ref_frames=REF_FRAMES, seed=SEED,
               ref_seed=REF_SEED, shift=SHIFT, rms_raw=raw, rms_reprojected_at_defaults=rms_y(dflt, ref),
               ratio_at_defaults=at_defaults, defaults=dict(cos_min=cm, kz=kz, max_history=mh), best_key=best,
               library_defaults_are_the_best=bool(at_defaults == grid[best]),
               rejected_share_of_hit_pixels=round(rejected_share(e, dflt), 4), hit_pixels=int(e["hit"].sum()), grid=grid)
    print(json.dumps({k: v for k, v in rec.items() if k != "grid"}))
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

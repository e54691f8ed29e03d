#!/usr/bin/env python3
"""What the preview filter is worth over a reprojected view, measured on the CPU: tools/reproject_quality.py's
experiment (scene 6 at 32x32, 64 oracle frames at camera A, the same sideways move), the moments of
tools/denoise_quality.py's moments_of at both cameras, rt_reproject_variance_host and
rt_denoise_reprojected_host.

With 1 frame and with 2 frames at camera B, against a 1024-frame render at B with another seed, the RMS error
of y = (r + g) + b of the raw image, of the reprojected view and of the reprojected view filtered (guided at
the library's defaults, and unguided), over the whole image and over the fresh pixels alone (n_out <= the
frames at B: disoccluded strips, the background, rejected taps), and a grid of levels x k.  Also the flat
64x64 signal with iid noise, one frame per pixel and no variance known, that tests/test_reproject_var_host.py
asserts.  tests/test_gpu_reproject_var.py repeats the experiment on the device.

    python tools/reproject_filter_quality.py [--out profiles/reproject_filter_quality.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import reproject_quality as Q  # noqa: E402  (puts the package, the oracle and tests/ on the path)
from denoise_quality import moments_of  # noqa: E402
import rtamd  # noqa: E402

F = np.float32
SCENE, W, H = Q.SCENE, Q.W, Q.H
FRAMES_A, FRAMES_B, REF_FRAMES, SEED, REF_SEED = Q.FRAMES_A, (1, 2), Q.REF_FRAMES, Q.SEED, Q.REF_SEED
LEVELS, KS = (1, 2, 3, 4), (1.0, 2.0, 3.0, 4.0)
FLAT = dict(width=64, height=64, sigma=0.05, seed=11)


def experiment(sid, w, h, frames_a, frames_b, shift=Q.SHIFT):
    """reproject_quality's experiment plus what the variance needs: the history's s2 and the moments at B."""
    e = Q.experiment(sid, w, h, frames_a, frames_b, shift)
    m2_a = moments_of(Q.scene_at(sid, w, h), frames_a, SEED)
    e["hs2"] = rtamd.history_variance_host(e["hist"], m2_a, frames_a)
    e["m2"] = moments_of(e["scene_b"], frames_b, SEED)
    return e


def reproject(e, **prm):
    """-> (rgbn, s2) of rt_reproject_variance_host."""
    return rtamd.reproject_variance_host(e["hist"], e["hnd"], e["hai"], e["hs2"], e["hcam"], e["image"], e["m2"], e["tf"],
                                         e["nd"], e["ai"], e["cam"], **prm)


def filtered(e, rgbn, s2, guides=True, levels=None, k=None):
    return rtamd.denoise_reprojected_host(rgbn, s2, e["nd"], e["ai"], levels=levels, k=k, guides=guides)


def rms_y(a, b, mask=None):
    ya, yb = [(x[..., 0].astype(np.float64) + x[..., 1]) + x[..., 2] for x in (a, b)]
    d = ya - yb
    ok = np.isfinite(d) if mask is None else np.isfinite(d) & mask
    return float(np.sqrt(np.mean(d[ok] ** 2)))


def fresh_pixels(e, rgbn):
    """The pixels whose count did not grow: not reprojected, or rejected."""
    return rgbn[..., 3] <= F(e["tf"])


def flat_noise(width, height, sigma, seed):
    """A flat signal with iid Gaussian noise per channel as a one-frame view with nothing known about its
    variance: (signal, rgbn with n = 1, s2 = -1, normal_depth, albedo_id of one surface)."""
    rng = np.random.default_rng(seed)
    signal = np.empty((height, width, 4), F)
    signal[...] = np.array([0.5, 0.4, 0.3, 1.0], F)
    rgbn = signal.copy()
    rgbn[..., :3] += rng.normal(0.0, sigma, (height, width, 3)).astype(F)
    s2 = np.full((height, width), -1.0, F)
    nd = np.zeros((height, width, 4), F)
    nd[..., 2], nd[..., 3] = 1.0, 5.0
    ai = rtamd.pack_albedo_id(np.full((height, width, 3), 0.5, F), np.full((height, width), 2, np.uint32))
    return signal, rgbn, s2, nd, ai


def flat_noise_ratio(**kw):
    """RMSE of rgb after / before rt_denoise_reprojected_host at the defaults on flat_noise."""
    signal, rgbn, s2, nd, ai = flat_noise(**dict(FLAT, **kw))
    out = rtamd.denoise_reprojected_host(rgbn, s2, nd, ai)

    def rmse(a):
        d = a[..., :3].astype(np.float64) - signal[..., :3].astype(np.float64)
        return float(np.sqrt(np.mean(d ** 2)))

    return rmse(out) / rmse(rgbn)


def measure(frames_b, ref=None):
    """One run of the experiment -> (record, ref)."""
    e = experiment(SCENE, W, H, FRAMES_A, frames_b)
    if ref is None:
        ref = Q.oracle_frames(e["scene_b"], REF_FRAMES, REF_SEED)
    rgbn, s2 = reproject(e)
    fresh = fresh_pixels(e, rgbn)
    raw, rep = rms_y(e["image"], ref), rms_y(rgbn, ref)
    rep_fresh = rms_y(rgbn, ref, fresh)

    def ratios(out):
        return dict(whole=round(rms_y(out, ref) / rep, 4), fresh=round(rms_y(out, ref, fresh) / rep_fresh, 4))

    grid = {}
    for lv in LEVELS:
        for k in KS:
            grid[f"levels={lv},k={k:g}"] = ratios(filtered(e, rgbn, s2, levels=lv, k=k))
    best = min(grid, key=lambda key: (grid[key]["whole"], grid[key]["fresh"]))
    rec = dict(frames_b=frames_b, pixels=int(fresh.size), fresh_pixels=int(fresh.sum()),
               s2_known_pixels=int((s2 >= 0).sum()), rms_raw=raw, rms_reprojected=rep, rms_reprojected_fresh=rep_fresh,
               reprojected_over_raw=round(rep / raw, 4),
               filtered_over_reprojected=dict(guided_defaults=ratios(filtered(e, rgbn, s2)),
                                              unguided_defaults=ratios(filtered(e, rgbn, s2, guides=None))),
               grid_guided=grid, grid_best=best)
    return rec, ref


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "reproject_filter_quality.json"))
    a = ap.parse_args()
    runs, ref = {}, None
    for fb in FRAMES_B:
        runs[f"frames_b={fb}"], ref = measure(fb, ref)
    rec = dict(what="RMS error of y against a long render at camera B with another seed: the reprojected view filtered by "
                    "rt_denoise_reprojected_host over the unfiltered reprojected view, over the whole image and over the fresh "
                    "pixels (n_out <= frames at B); oracle frames, tests/features_ref.py features, moments_of moments, "
                    "rt_reproject_variance_host",
               scene=SCENE, width=W, height=H, frames_a=FRAMES_A, ref_frames=REF_FRAMES, seed=SEED, ref_seed=REF_SEED,
               shift=Q.SHIFT, denoise_defaults=dict(levels=rtamd.render.DENOISE_DEFAULTS[0], k=rtamd.render.DENOISE_DEFAULTS[1]),
               flat_noise=dict(FLAT, frames=1, ratio=round(flat_noise_ratio(), 4)), runs=runs)
    print(json.dumps({k: ({r: {x: y for x, y in v.items() if x != "grid_guided"} for r, v in rec[k].items()} if k == "runs" else v)
                      for k, v in rec.items()}))
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

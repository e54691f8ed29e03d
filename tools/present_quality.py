#!/usr/bin/env python3
"""What the composite of rt_present's RT_PRESENT_MOVED is worth after a camera move, measured on the CPU with
the host functions: tools/reproject_filter_quality.py's experiment (scene 6 at 32x32, 64 oracle frames at
camera A, a quarter-viewport move, 1 and 2 frames at camera B, the filter guided at the library's defaults),
then rt_present_host over the reprojected view and the filtered buffer.

Against a 1024-frame render at B with another seed, the RMS error of y = (r + g) + b of the composite (the
float copy: the filtered buffer on the fresh pixels, n_out <= the frames at B, the reprojected view elsewhere),
of the filtered buffer alone and of the unfiltered reprojected view, over the whole image and over the fresh
pixels; the composite is also checked to be the reprojected view bit for bit on every other pixel, and its
bytes to be rts_tonemap_rgb8's of the composed floats.

    python tools/present_quality.py [--out profiles/present_quality.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import reproject_filter_quality as RF  # noqa: E402  (puts the package, the oracle and tests/ on the path)
import reproject_quality as Q  # noqa: E402
import rtamd  # noqa: E402

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def measure(frames_b, ref=None):
    """One run of the experiment -> (record, ref)."""
    e = RF.experiment(RF.SCENE, RF.W, RF.H, RF.FRAMES_A, frames_b)
    if ref is None:
        ref = Q.oracle_frames(e["scene_b"], RF.REF_FRAMES, RF.REF_SEED)
    rgbn, s2 = RF.reproject(e)
    den = RF.filtered(e, rgbn, s2)
    frame, comp = rtamd.present_host("moved", reprojected=rgbn, denoised=den, tile_frames=e["tf"], keep_float=True)
    fresh = RF.fresh_pixels(e, rgbn)
    assert np.array_equal(comp[..., 3] == 1, fresh) and np.array_equal(comp[..., 3] == 0, ~fresh)
    rest_equal = bool(np.array_equal(bits(comp[~fresh][:, :3]), bits(rgbn[~fresh][:, :3])))
    fresh_is_filtered = bool(np.array_equal(bits(comp[fresh][:, :3]), bits(den[fresh][:, :3])))
    bytes_equal = bool(np.array_equal(frame[..., :3], rtamd.tonemap_rgb8(comp)))
    rep, rep_fresh = RF.rms_y(rgbn, ref), RF.rms_y(rgbn, ref, fresh)

    def ratios(out):
        return dict(whole=round(RF.rms_y(out, ref) / rep, 4), fresh=round(RF.rms_y(out, ref, fresh) / rep_fresh, 4))

    rec = dict(frames_b=frames_b, pixels=int(fresh.size), fresh_pixels=int(fresh.sum()), other_pixels=int((~fresh).sum()),
               rms_reprojected=rep, rms_reprojected_fresh=rep_fresh,
               composite_over_reprojected=ratios(comp), filtered_over_reprojected=ratios(den),
               composite_is_reprojected_elsewhere=rest_equal, composite_is_filtered_on_fresh=fresh_is_filtered,
               bytes_are_tonemap_of_composite=bytes_equal)
    return rec, ref


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "present_quality.json"))
    a = ap.parse_args()
    runs, ref = {}, None
    for fb in RF.FRAMES_B:
        runs[f"frames_b={fb}"], ref = measure(fb, ref)
    rec = dict(what="RMS error of y against a long render at camera B with another seed, over the unfiltered reprojected "
                    "view's: the composite rt_present_host makes under RT_PRESENT_MOVED (its float copy) and the filtered "
                    "buffer alone (rt_denoise_reprojected_host, guided at the defaults), over the whole image and over the "
                    "fresh pixels (n_out <= frames at B); oracle frames, tests/features_ref.py features, moments_of moments",
               scene=RF.SCENE, width=RF.W, height=RF.H, frames_a=RF.FRAMES_A, ref_frames=RF.REF_FRAMES, seed=RF.SEED,
               ref_seed=RF.REF_SEED, shift=Q.SHIFT, runs=runs)
    print(json.dumps(rec))
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

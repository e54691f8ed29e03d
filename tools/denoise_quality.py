"""What the preview filter is worth, measured on the CPU: oracle renders plus rt_denoise_host.

The GPU image is bit-exact with the oracle, so the ratio RMSE(filtered) / RMSE(raw) against a long
reference render is measured here and tests/test_gpu_denoise.py asserts it on the device with a bound
halfway between the measured ratio and 1.  The oracle exports no per-frame colours: frame f's colour is
rebuilt as f times a one-frame render started at frame f (the running mean of a zero image, c / f), which
is c to within an ulp or two, and M2 follows from rt_moments.hip's Welford update in float32.  The
filter's input image is the oracle's own 16-frame render.

    python tools/denoise_quality.py [--out profiles/denoise_quality.json]

--guided measures rt_denoise_guided's guide strengths instead: for scenes 8, 6, 0 and 2 the same 16 oracle
frames and long reference, the first-hit buffers of tests/features_ref.py (the oracle's per-operation
entry points), and rt_denoise_guided_host over a grid of (kn, kz, ka) at the filter's default levels and k.
The defaults of rt.h (RT_GUIDE_DEFAULT_*) are the setting with the best scene-0 ratio among those no worse
than the unguided filter on the other three scenes; tests/test_gpu_features.py asserts it on the device.

    python tools/denoise_quality.py --guided [--out profiles/denoise_guided_quality.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-book_amd"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

import pyoracle  # noqa: E402
import rtamd  # noqa: E402

F = np.float32
CASES = [(8, 96, 54), (6, 64, 64), (0, 96, 54)]   # scene, W, H; the first two are the asserted ones
FRAMES, REF_FRAMES, SEED, REF_SEED = 16, 1024, 1, 2


def moments_of(scene, frames, seed):
    """M2 over frames 1 .. n by rt_moments.hip's update, from the rebuilt per-frame colours."""
    o = pyoracle.OracleScene(scene, max_depth=5, spp=frames)
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
    return m2


def rmse(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    ok = np.isfinite(d).all(axis=-1)
    return float(np.sqrt(np.mean(d[ok] ** 2)))


GUIDED_CASES = CASES + [(2, 96, 54)]
GUIDE_KN, GUIDE_KZ, GUIDE_KA = (0.0, 0.5, 1.0, 2.0, 4.0, 8.0), (0.0, 1.0, 4.0, 16.0), (0.0, 0.5, 1.0, 2.0, 4.0, 8.0)


def guided_main(out):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import features_ref  # noqa: E402
    cases = []
    for sid, W, H in GUIDED_CASES:
        scene = rtamd.Scene(sid, W, H, seed=SEED)
        raw = pyoracle.render(pyoracle.OracleScene(scene, max_depth=5, spp=FRAMES), rtamd.frame_rand_factors(SEED, 0, FRAMES))
        ref = pyoracle.render(pyoracle.OracleScene(scene, max_depth=5, spp=REF_FRAMES),
                              rtamd.frame_rand_factors(REF_SEED, 0, REF_FRAMES))
        m2 = moments_of(scene, FRAMES, SEED)
        ft = features_ref.reference(sid, W, H, seed=SEED)
        nd = np.concatenate([ft.N, ft.t[..., None]], -1).astype(F)
        ai = rtamd.pack_albedo_id(ft.A, ft.id)
        before = rmse(raw, ref)
        unguided = round(rmse(rtamd.denoise_host(raw, m2, FRAMES), ref) / before, 4)
        grid = {}
        for kn in GUIDE_KN:
            for kz in GUIDE_KZ:
                for ka in GUIDE_KA:
                    den = rtamd.denoise_guided_host(raw, m2, FRAMES, nd, ai, guides=(kn, kz, ka))
                    grid[f"kn={kn:g},kz={kz:g},ka={ka:g}"] = round(rmse(den, ref) / before, 4)
        assert grid["kn=0,kz=0,ka=0"] == unguided
        rec = dict(scene=sid, width=W, height=H, frames=FRAMES, ref_frames=REF_FRAMES, seed=SEED, ref_seed=REF_SEED,
                   rmse_raw=before, ratio_unguided=unguided, tied_pixels=int(ft.tied.sum()), grid=grid)
        print(json.dumps({k: v for k, v in rec.items() if k != "grid"}), flush=True)
        cases.append(rec)
    by = {c["scene"]: c for c in cases}
    ok = [key for key in by[0]["grid"] if all(by[s]["grid"][key] <= by[s]["ratio_unguided"] for s in (8, 6, 2))]
    best = min(ok, key=lambda key: (by[0]["grid"][key], key))
    helps = by[0]["grid"][best] < by[0]["ratio_unguided"]
    kn, kz, ka = (float(part.split("=")[1]) for part in best.split(","))
    chosen = dict(kn=kn, kz=kz, ka=ka) if helps else dict(kn=0.0, kz=0.0, ka=0.0)
    s0 = by[0]
    guided0 = s0["grid"][best] if helps else s0["ratio_unguided"]
    summary = dict(defaults=chosen, beats_unguided_on_scene0=bool(helps), best_key=best,
                   ratios_at_defaults={str(s): by[s]["grid"][best] if helps else by[s]["ratio_unguided"] for s in by},
                   ratios_unguided={str(s): by[s]["ratio_unguided"] for s in by},
                   scene0_bound=round((guided0 + s0["ratio_unguided"]) / 2.0, 4))
    print(json.dumps(summary))
    with open(out, "w") as f:
        json.dump(dict(what="RMSE(guided filter) / RMSE(raw) against a long render with another seed, over (kn, kz, ka) at levels 3, "
                            "k 3; oracle frames, tests/features_ref.py features, rt_denoise_guided_host",
                       rule="best on scene 0 among the settings no worse than unguided on scenes 8, 6 and 2; scene0_bound is "
                            "halfway between the guided and the unguided scene-0 ratio",
                       **summary, cases=cases), f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--guided", action="store_true", help="the (kn, kz, ka) grid of rt_denoise_guided")
    a = ap.parse_args()
    if a.guided:
        return guided_main(a.out or os.path.join(REPO, "profiles", "denoise_guided_quality.json"))
    a.out = a.out or os.path.join(REPO, "profiles", "denoise_quality.json")
    cases = []
    for sid, W, H in CASES:
        scene = rtamd.Scene(sid, W, H, seed=SEED)
        raw = pyoracle.render(pyoracle.OracleScene(scene, max_depth=5, spp=FRAMES), rtamd.frame_rand_factors(SEED, 0, FRAMES))
        ref = pyoracle.render(pyoracle.OracleScene(scene, max_depth=5, spp=REF_FRAMES),
                              rtamd.frame_rand_factors(REF_SEED, 0, REF_FRAMES))
        m2 = moments_of(scene, FRAMES, SEED)
        before = rmse(raw, ref)
        grid = {}
        for levels in (1, 2, 3, 4, 5):
            for k in (1.0, 2.0, 3.0, 4.0, 6.0):
                grid[f"levels={levels},k={k:g}"] = round(rmse(rtamd.denoise_host(raw, m2, FRAMES, levels=levels, k=k), ref) / before, 4)
        ratio = rmse(rtamd.denoise_host(raw, m2, FRAMES), ref) / before
        rec = dict(scene=sid, width=W, height=H, frames=FRAMES, ref_frames=REF_FRAMES, seed=SEED, ref_seed=REF_SEED,
                   rmse_raw=before, ratio_defaults=round(ratio, 4), bound=round((1.0 + round(ratio, 4)) / 2.0, 4),
                   asserted=bool(ratio <= 0.9 and sid != 0), grid=grid)
        print(json.dumps(rec))
        cases.append(rec)
    with open(a.out, "w") as f:
        json.dump(dict(what="RMSE(filtered) / RMSE(raw) against a long render with another seed; oracle frames + rt_denoise_host",
                       defaults=dict(levels=3, k=3.0), cases=cases), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

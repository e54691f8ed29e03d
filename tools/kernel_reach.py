"""Which render_persistent instances can rt_render launch?  Host only (rt_debug_plan_scene, then
rt_debug_plan_kernel): every subset of at most three of the thirteen option settings below, over five
built-in scenes and seven of tests/adversarial.py at 61x45, with and without a tile mask.  For each entry of
the kernel table the first (scene, options) that reached it, and the entries never reached, go to
profiles/kernel_matrix.json (tests/test_kernel_matrix.py reads it; tests/kernel_matrix.py is the table
the GPU suite runs).
Usage: python tools/kernel_reach.py [--out profiles/kernel_matrix.json]"""
import argparse
import itertools
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "oracle", "raytracing-book_amd"):
    sys.path.insert(0, os.path.join(REPO, p))

import adversarial  # noqa: E402
import rtamd  # noqa: E402
from test_launch_plan import PKO, plan, table  # noqa: E402

W, H, FRAMES = 61, 45, 3
MASK = [0, 19, 47]
SETTINGS = [("fastdiv", 0), ("compact_boxes", 0), ("big_wg", 0), ("sphere_pairs", 0), ("sphere_pairs", 2),
            ("shade_lds", 0), ("sparse_stage", 0), ("box_interior", 0), ("lds_node_cap", 4096), ("sph_lds", 0),
            ("leaf_prefetch", 0), ("stage_tiles", 0), ("tl_small_lds", 0)]


def scenes():
    out = [(f"s{k}", rtamd.Scene(k, W, H, seed=1)) for k in (0, 2, 6, 7, 8)]
    out += [("edges", adversarial.edges(W=W, H=H)), ("edges_rotated", adversarial.edges(rotated=True, W=W, H=H)),
            ("extent_inside_2^20", adversarial.extent(0.95 * 2 ** 20, W=W, H=H)),
            ("extent_past_2^20", adversarial.extent(1.1 * 2 ** 20, W=W, H=H)),
            ("bvh_4k_lds", adversarial.sphere_cloud(4000, 4, W=W, H=H)),
            ("bvh_9k_two_level", adversarial.sphere_cloud(9000, 9, W=W, H=H)),
            ("spine_face_0.0019", adversarial.spine(0.0019, W=W, H=H))]
    return out


def subsets():
    for n in range(4):
        for c in itertools.combinations(SETTINGS, n):
            if len({k for k, _ in c}) == n:
                yield dict(c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kernel_matrix.json"))
    a = ap.parse_args()
    t0 = time.time()
    tab = table()
    first, plans, refused = {}, 0, 0
    built = scenes()
    for name, sc in built:
        for opts in subsets():
            for mask in (None, MASK):
                got = rtamd.plan_scene(sc, FRAMES, options=opts, mask=mask, spp=4096, waves=4096)
                out, _ = plan(got["pk"][None, :], [0])
                plans += 1
                if got["launched"] != 1 or out[0][PKO["OK"]] != 1:
                    refused += 1
                    continue
                k = (int(out[0][PKO["BLOCK"]]), int(out[0][PKO["OPT"]]))
                assert k in tab, k
                first.setdefault(k, {"scene": name, "options": opts, "mask": mask})
    doc = {"tool": "python tools/kernel_reach.py", "width": W, "height": H, "frames": FRAMES, "spp": 4096, "waves": 4096,
           "scenes": [n for n, _ in built], "settings": [list(s) for s in SETTINGS], "max_options": 3,
           "plans": plans, "refused": refused, "table": len(tab),
           "reached": [{"block": b, "opt": o, **first[(b, o)]} for b, o in sorted(first)],
           "never_reached": [[b, o] for b, o in sorted(set(tab) - set(first))]}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"{plans} plans, {len(first)} of {len(tab)} entries reached, never: {doc['never_reached']}, "
          f"{time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()

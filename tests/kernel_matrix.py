"""Which scene and options launch which render_persistent instance (test infrastructure; a plain module).

The release library compiles 56 instances: the 28 X(BLOCK, OPT) entries of RT_RENDER_KERNELS
(csrc/rt_plan.h) and their tile-mask twins (OPT | RT_OPT_MASK).  ROWS names, for every unmasked entry
rt_render can reach, one scene with options under which plan_kernel chooses it at 61x45; the same row
under a tile mask chooses the twin.  61x45 is 8x6 = 48 tiles whose right column is 5 pixels wide and
whose bottom row is 5 pixels high.  tests/test_kernel_matrix.py keeps this table true on the host;
tests/test_gpu_kernel_matrix.py launches every entry and compares its image with the CPU oracle.

DEAD are the four instances no rt_render call can launch (tests/test_kernel_matrix.py says why).
"""
import functools

import numpy as np

import adversarial
import rtamd
from test_launch_plan import LI, PKO, plan

W, H = 61, 45
TX, TY = 8, 6
NT = TX * TY
FRAMES = 6          # two launches of LAUNCH frames
LAUNCH = 3
DEPTH = 5
MASK = [0, 7, 19, 40, 47]   # both corners' tiles, a right-edge tile (7), a bottom-edge tile (40), an interior one
REST = [t for t in range(NT) if t not in MASK]   # the twins' last launch: every other tile, six frames at once
STD, BOXQ, MASKED = 128, 256, 512   # RT_OPT_STD, RT_OPT_BOXQ, RT_OPT_MASK

# (block, OPT) -> (scene, options)
ROWS = {
    (1024, 11): ("s8", {"fastdiv": 0, "compact_boxes": 0}),
    (1024, 15): ("s8", {"compact_boxes": 0, "shade_lds": 0}),
    (1024, 27): ("s0", {"fastdiv": 0, "lds_node_cap": 4096}),
    (1024, 31): ("s0", {"lds_node_cap": 4096}),
    (1024, 43): ("s8", {"fastdiv": 0}),
    (1024, 47): ("s8", {"shade_lds": 0}),
    (1024, 59): ("s8", {"fastdiv": 0, "lds_node_cap": 4096}),
    (1024, 63): ("s8", {"lds_node_cap": 4096}),
    (1024, 75): ("s8", {"fastdiv": 0, "compact_boxes": 0, "sphere_pairs": 2}),
    (1024, 79): ("s8", {"compact_boxes": 0, "sphere_pairs": 2, "shade_lds": 0}),
    (1024, 111): ("s8", {"sphere_pairs": 2}),
    (1024, 143): ("s8", {"compact_boxes": 0}),
    (1024, 175): ("s8", {"box_interior": 0}),
    (1024, 207): ("s8", {"compact_boxes": 0, "sphere_pairs": 2}),
    (1024, 431): ("s8", {}),
    (512, 11): ("s0", {"fastdiv": 0, "sphere_pairs": 0}),
    (512, 15): ("s0", {"sphere_pairs": 0, "shade_lds": 0}),
    (512, 43): ("s8", {"fastdiv": 0, "big_wg": 0}),
    (512, 47): ("s8", {"big_wg": 0}),
    (512, 75): ("s0", {"fastdiv": 0}),
    (512, 79): ("s0", {"shade_lds": 0}),
    (512, 111): ("s8", {"big_wg": 0, "sphere_pairs": 2}),
    (512, 143): ("s0", {"sphere_pairs": 0}),
    (512, 175): ("edges", {"box_interior": 0}),
    (512, 207): ("s0", {}),
    (512, 431): ("edges", {}),
}

# how a launch stages its frames; an RT_OPT_STD kernel is chosen under "staged" alone (plan_kernel's std_cfg
# needs the sparse staging), under the other three the same row takes its sibling without RT_OPT_STD
STAGING = {
    "staged": {},
    "dense": {"sparse_stage": 0},
    "ordered1": {"stage_tiles": 0, "chunk_target": 1},
    "direct": {"chunk_target": 0},
}

DEAD = {(1024, 159), (1024, 191), (1024, 671), (1024, 703)}   # the two-level kernels with RT_OPT_STD, and twins


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "edges":
        return adversarial.edges(W=W, H=H)
    return rtamd.Scene(int(name[1:]), W, H, seed=1)


def kernel_under(row, state, masked):
    """The (block, opt) a row's launch takes under a staging state, with or without a tile mask."""
    block, opt = row
    if state != "staged":
        opt &= ~(STD | BOXQ)
    return block, opt | (MASKED if masked else 0)


# (512, 47) is reached with two LDS layouts: on s8 with big_wg 0 not every table fits 512 threads' LDS, so the
# global-memory forms of the shared device functions run; on edges under "direct" everything is staged
EXTRA = {(512, 47): [("edges", {}, "direct")]}


def configurations(kernel):
    """[(label, scene name, options, mask or None)] a kernel (block, opt; RT_OPT_MASK for the twin) is run
    under: its row as "staged" for an RT_OPT_STD entry, under all four staging states for the others, and
    EXTRA's."""
    row, masked = (kernel[0], kernel[1] & ~MASKED), bool(kernel[1] & MASKED)
    name, options = ROWS[row]
    runs = [(name, options, s) for s in (["staged"] if row[1] & STD else STAGING)]
    runs += EXTRA.get(row, [])
    return [(f"{n} {o or 'defaults'} {s}", n, {**o, **STAGING[s]}, MASK if masked else None) for n, o, s in runs]


def kernels():
    """Every reachable instance: ROWS and their mask twins, in the order of the ids."""
    return [(b, o | m) for m in (0, MASKED) for b, o in ROWS]


def planned(scene, frames, first_frame, options, mask, prev, waves, free_bytes, spp=FRAMES):
    """What rt_render would launch (tests/test_gpu_scene_plan.py predicted, with the kernel): the whole
    rt_debug_last_launch as a list, the first-leaf words, the tile counts after, and (block, opt)."""
    prev = np.asarray(prev, np.int32)
    uniform = len(set(prev.tolist())) == 1
    got = rtamd.plan_scene(scene, frames, first_frame=first_frame, options=options, mask=mask, prev_frames=int(prev.min()),
                           prev_tile_frames=None if uniform else prev, waves=waves, free_bytes=free_bytes, spp=spp)
    assert got["launched"] == 1
    out, info = plan(got["pk"][None, :], [0])
    assert out[0][PKO["OK"]] == 1, (options, mask)
    for f in ("bvh_mode", "box_vnodes", "collapsed", "rebuilt"):
        info[0][LI[f]] = got[f]
    kernel = (int(out[0][PKO["BLOCK"]]), int(out[0][PKO["OPT"]]))
    return [int(x) for x in info[0]], [x & 0xFFFFFFFF for x in got["first_leaf"]], got["tile_frames"], kernel

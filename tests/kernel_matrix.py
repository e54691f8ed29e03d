"""Which scene and options launch which render_persistent instance (test infrastructure; a plain module).

The release library compiles 56 instances: the 28 X(BLOCK, OPT) entries of RT_RENDER_KERNELS
(csrc/rt_plan.h) and their tile-mask twins (OPT | RT_OPT_MASK).  ROWS names, for every unmasked entry
rt_render can reach, one scene with options under which plan_kernel chooses it at 61x45; the same row
under a tile mask chooses the twin.  61x45 is 8x6 = 48 tiles whose right column is 5 pixels wide and
whose bottom row is 5 pixels high.  tests/test_kernel_matrix.py keeps this table true on the host;
tests/test_gpu_kernel_matrix.py launches every entry and compares its image with the CPU oracle.

DEAD are the four instances no rt_render call can launch (tests/test_kernel_matrix.py says why).

planned() and launch() are the launch check the GPU files share (tests/test_gpu_random_scenes.py too): what the
host plans for a launch, and one rt_render held to that plan field by field.
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


def planned(scene, frames, first_frame, options, mask, prev, waves, free_bytes, spp=FRAMES, partition=None):
    """What rt_render would launch (tests/test_gpu_scene_plan.py predicted, with the kernel): the whole
    rt_debug_last_launch as a list, the first-leaf words, the tile counts after, and (block, opt).
    partition: (rank, world, stripe_rows) of a stripe-partitioned context."""
    prev = np.asarray(prev, np.int32)
    uniform = len(set(prev.tolist())) == 1
    part = {} if partition is None else dict(zip(("rank", "world", "stripe_rows"), partition))
    got = rtamd.plan_scene(scene, frames, first_frame=first_frame, options=options, mask=mask, prev_frames=int(prev.min()),
                           prev_tile_frames=None if uniform else prev, waves=waves, free_bytes=free_bytes, spp=spp, **part)
    assert got["launched"] == 1
    out, info = plan(got["pk"][None, :], [0])
    assert out[0][PKO["OK"]] == 1, (options, mask)
    for f in ("bvh_mode", "box_vnodes", "collapsed", "rebuilt"):
        info[0][LI[f]] = got[f]
    kernel = (int(out[0][PKO["BLOCK"]]), int(out[0][PKO["OPT"]]))
    return [int(x) for x in info[0]], [x & 0xFFFFFFFF for x in got["first_leaf"]], got["tile_frames"], kernel


def launch(ctx, kernel, label, scene, options, mask, first, frames, waves, partition=None):
    """One rt_render of `frames` frames from `first` on a device context (the GPU tests' step): planned on the
    host first, from the device's free memory and `waves`, then all 21 reported fields, the first-leaf words and
    the tile counts equal to the plan, whose kernel is `kernel` (None: whichever the plan names).  Returns the
    planned (block, opt).  Under a partition (rt_read_tile_frames does not serve one) the counts are the frames
    rendered so far, first - 1 in every tile of the stripe, and are not read back."""
    import torch
    if partition is None:
        before = ctx.read_tile_frames()
    else:
        before = np.full(((ctx.width + 7) // 8) * ((ctx.local_rows + 7) // 8), first - 1, np.int32)
    free_bytes = torch.cuda.mem_get_info(0)[0]
    want_launch, want_leaf, want_frames, want_kernel = planned(scene, frames, first, options, mask, before, waves,
                                                               free_bytes, partition=partition)
    assert kernel is None or want_kernel == kernel, f"{label}: frame {first} plans {want_kernel}"
    ctx.render(first, rtamd.frame_rand_factors(1, first - 1, frames))
    ctx.sync()
    ll, fl = ctx.last_launch(), ctx.first_leaf()
    got_launch = [ll[n] for n in rtamd.render.LAUNCH_FIELDS]
    print(want_kernel, label, "mask" if mask is not None else "full", first, got_launch)
    assert len(got_launch) == 21 and got_launch == want_launch, \
        (label, first, dict(zip(rtamd.render.LAUNCH_FIELDS, want_launch)), ll)
    assert [fl["armed"], fl["link"], fl["types"], fl["prims"]] == want_leaf, (label, first, fl)
    if partition is None:
        assert np.array_equal(ctx.read_tile_frames(), want_frames), (label, first)
    else:
        assert (np.asarray(want_frames) == first - 1 + frames).all() and len(want_frames) == before.size, (label, first)
    return want_kernel

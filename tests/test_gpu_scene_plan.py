"""What a real render reports against what the host predicts for the same inputs (csrc/rt_args.h):
rt_debug_last_launch and rt_debug_first_leaf after rt_render must equal rt_debug_plan_scene followed by
rt_debug_plan_kernel, fed the scene, the options, the mask, the device's resident waves (16 per CU) and its
free memory; rt_read_tile_frames must equal the predicted counts after a masked render and an unmasked one.
Scenes 8, 6 and 0 at 64x48, 3 frames: defaults, a node cap (option lds_node_cap 98304; and 16384, under
which scene 8 takes the two-level walk) and a 3-tile mask.  The images themselves are the parity suites'
business.
"""
import numpy as np
import pytest
import torch

import rtamd
from test_launch_plan import LI, plan

pytestmark = pytest.mark.gpu

W, H, FRAMES = 64, 48, 3
MASK = [5, 17, 44]
CASES = {"defaults": ({}, None), "lds_node_cap": ({"lds_node_cap": 98304}, None), "mask3": ({}, MASK),
         "two_level": ({"lds_node_cap": 16384}, None)}   # (scene 8: the cap that reaches the two-level walk)


def predicted(scene, frames, first_frame, options, mask, prev):
    """(the whole rt_debug_last_launch as a list, the first-leaf words, the tile counts after)"""
    waves = torch.cuda.get_device_properties(0).multi_processor_count * 16
    free_bytes = torch.cuda.mem_get_info(0)[0]
    uniform = len(set(prev.tolist())) == 1
    got = rtamd.plan_scene(scene, frames, first_frame=first_frame, options=options, mask=mask, prev_frames=int(prev.min()),
                           prev_tile_frames=None if uniform else prev, waves=waves, free_bytes=free_bytes, spp=FRAMES)
    assert got["launched"] == 1
    out, info = plan(got["pk"][None, :], [0])
    assert out[0][0] == 1
    for f in ("bvh_mode", "box_vnodes", "collapsed", "rebuilt"):
        info[0][LI[f]] = got[f]
    return [int(x) for x in info[0]], [x & 0xFFFFFFFF for x in got["first_leaf"]], got["tile_frames"]


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("sid", [8, 6, 0])
def test_render_reports_what_the_host_predicts(sid, case):
    options, mask = CASES[case]
    scene = rtamd.Scene(sid, W, H, seed=1)
    ctx = rtamd.RenderContext(devices=(0,), options=options or None)
    ctx.upload_scene(scene)
    ctx.set_params(max_depth=5, spp=FRAMES)
    ctx.resize(W, H)
    try:
        steps = [(mask, 1), (None, FRAMES + 1)] if mask is not None else [(None, 1)]
        for m, first in steps:
            before = ctx.read_tile_frames()
            want_launch, want_leaf, want_frames = predicted(scene, FRAMES, first, options, m, before)
            if m is not None:
                active = np.zeros(before.size, np.uint8)
                active[m] = 1
                ctx.set_active_tiles(active)
            else:
                ctx.set_active_tiles(None)
            ctx.render(first, rtamd.frame_rand_factors(1, first - 1, FRAMES))
            ctx.sync()
            ll, fl = ctx.last_launch(), ctx.first_leaf()
            got_launch = [ll[n] for n in rtamd.render.LAUNCH_FIELDS]
            print(sid, case, first, got_launch, fl)
            assert got_launch == want_launch, (dict(zip(rtamd.render.LAUNCH_FIELDS, want_launch)), ll)
            assert [fl["armed"], fl["link"], fl["types"], fl["prims"]] == want_leaf
            assert np.array_equal(ctx.read_tile_frames(), want_frames)
    finally:
        ctx.close()

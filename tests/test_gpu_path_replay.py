"""The path loop replayed link by link (tests/path_replay.py) with the device's own ops -- CAMERA_RAY, then per
bounce the plain closest-hit walk (RT_SOP_TRACE) and SHADE form 0 -- against what the render kernel staged for
the same frames (rt_debug_read_samples), frame by frame, and against its image, bit for bit.  The render runs
under the default options, so its walks go through the launch plan's spine, first-leaf, collapse, rebuild and
pre-test-node machinery; the replay's walk is the plain link walk from the root.  The oracle takes no part."""
import numpy as np
import pytest

import path_replay
import rtamd
import trace_cases

pytestmark = pytest.mark.gpu

W, H, FRAMES = 16, 12, 4
SCENES = ["scene6", "scene7", "scene8", "knot"]


def _scene(name):
    if name == "knot":
        return trace_cases.scene("knot")
    return rtamd.Scene(int(name[5:]), W, H, seed=1), rtamd.spp_uniforms(FRAMES)


@pytest.mark.parametrize("depth", [5, 1, 2])
@pytest.mark.parametrize("name", SCENES)
def test_replay_with_the_devices_ops_equals_its_render(gpu, name, depth):
    sc, uni = _scene(name)
    rf = rtamd.frame_rand_factors(1, 0, FRAMES)
    ctx = rtamd.RenderContext(devices=(0,))
    try:
        ctx.upload_scene(sc)
        ctx.set_params(max_depth=depth, uniforms=uni)
        ctx.resize(W, H)
        ctx.set_moments(True)          # staged colours are kept: the image's bits do not depend on it
        ctx.render(1, rf)
        ctx.sync()
        ll = ctx.last_launch()
        samples, image = ctx.read_samples(), ctx.read_image()
        got_image, curs = path_replay.render(path_replay.DeviceOps(ctx), W, H, depth, sc.background, rf)
    finally:
        ctx.close()
    print(name, depth, ll)
    assert ll["staged"] == 1 and samples.shape == (FRAMES, H, W, 4)
    for k in range(FRAMES):
        assert path_replay.same_bits(curs[k], samples[k][..., :3]), f"{name} depth {depth}: frame {k + 1}'s samples differ"
    assert path_replay.same_bits(got_image, image), f"{name} depth {depth}: the image differs"
    if name == "scene8":
        # the one tree here large enough for the launch plan's walk machinery (scenes 6, 7 and the knot have 7 to 21
        # nodes: no spine, nothing to collapse or rebuild): the render's walks started past the spine, over rebuilt and
        # collapsed inner nodes, with the boxes' pre-tests as nodes
        assert ll["spine"] > 0 and ll["collapsed"] > 0 and ll["rebuilt"] == 1 and ll["box_vnodes"] > 0, ll

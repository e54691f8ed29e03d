"""The trimmed scene-8 kernels (rt_kernel_common.h RT_WT_DISPATCH: the leaf stage computes a slot record's
LDS address by selects instead of a branch cascade) against their untrimmed twins and the CPU oracle,
bit for bit.

The trimmed code is compiled into the RT_OPT_BOXQ instantiations, so option box_interior = 0 runs
the twin without it (rt_debug_last_launch's box_interior says which ran).  Scene 8's leaves hold
every slot type the address serves: spheres, compact boxes, media, and the quads and empty slots
that select no table.
"""
import numpy as np
import pytest

import pyoracle
import rtamd
from helpers import bit_equal, mismatch_report

pytestmark = pytest.mark.gpu


def render(scene, frames, options=None, depth=5, spp=None, **part):
    ctx = rtamd.RenderContext(devices=(0,), options=options, **part)
    ctx.upload_scene(scene)
    ctx.set_params(max_depth=depth, spp=spp or frames)
    ctx.resize(scene.width, scene.height)
    ctx.render(1, rtamd.frame_rand_factors(1, 0, frames))
    img, info = ctx.read_image(), ctx.last_launch()
    ctx.close()
    return img, info


@pytest.mark.parametrize("seed", [1, 3])
def test_scene8_on_off_oracle(gpu, seed):
    scene = rtamd.Scene(8, 48, 27, seed=seed)
    on, info_on = render(scene, 4)
    off, info_off = render(scene, 4, {"box_interior": 0})
    assert info_on["box_interior"] == 1 and info_off["box_interior"] == 0, f"{info_on} {info_off}"
    assert info_on["leaf_prefetch"] == 1, info_on   # the leaf stage's prefetched form: where the address changed
    ref = pyoracle.render(pyoracle.OracleScene(scene, max_depth=5, spp=4), rtamd.frame_rand_factors(1, 0, 4))
    assert bit_equal(on, off), "on vs off: " + mismatch_report(on, off)
    assert bit_equal(on, ref), "on vs oracle: " + mismatch_report(on, ref)
    assert float(np.nanmean(on[..., :3])) > 0.01


def test_scene8_deep_paths_on_off_oracle(gpu):
    """Depth 12 and 6 frames: longer paths, so more walks from inside the media and the box of spheres."""
    scene = rtamd.Scene(8, 40, 24, seed=1)
    on, info_on = render(scene, 6, depth=12)
    off, info_off = render(scene, 6, {"box_interior": 0}, depth=12)
    assert info_on["box_interior"] == 1 and info_off["box_interior"] == 0, f"{info_on} {info_off}"
    ref = pyoracle.render(pyoracle.OracleScene(scene, max_depth=12, spp=6), rtamd.frame_rand_factors(1, 0, 6))
    assert bit_equal(on, off), "on vs off: " + mismatch_report(on, off)
    assert bit_equal(on, ref), "on vs oracle: " + mismatch_report(on, ref)


def test_scene8_one_rank_of_eight_stripes(gpu):
    """Rank 3 of 8 with 8-row stripes at 64x72 (ordered / staged chunks over few tiles): on = off = the
    oracle's render of the same stripes."""
    scene = rtamd.Scene(8, 64, 72, seed=1)
    part = dict(rank=3, world=8, stripe_rows=8)
    on, info_on = render(scene, 4, **part)
    off, info_off = render(scene, 4, {"box_interior": 0}, **part)
    assert info_on["box_interior"] == 1 and info_off["box_interior"] == 0, f"{info_on} {info_off}"
    ref = pyoracle.render(pyoracle.OracleScene(scene, max_depth=5, spp=4), rtamd.frame_rand_factors(1, 0, 4), **part)
    ref = ref[rtamd.stripe_rows_of(72, 3, 8, 8)]   # the oracle writes the rank's rows of the full image
    assert on.shape[0] == rtamd.local_rows(72, 3, 8, 8) == 8
    assert bit_equal(on, off), "on vs off: " + mismatch_report(on, off)
    assert bit_equal(on, ref), "on vs oracle: " + mismatch_report(on, ref)


def test_scene6_runs_an_untrimmed_kernel(gpu):
    """Scene 6 has no compact-box kernel: it reports box_interior 0 either way and equals the oracle."""
    scene = rtamd.Scene(6, 48, 27, seed=1)
    img, info = render(scene, 4)
    assert info["box_interior"] == 0, info
    ref = pyoracle.render(pyoracle.OracleScene(scene, max_depth=5, spp=4), rtamd.frame_rand_factors(1, 0, 4))
    assert bit_equal(img, ref), mismatch_report(img, ref)


def test_scene8_1080p_on_off(gpu):
    """A whole 1080p image of scene 8 (another seed than tests/test_gpu_box_test.py's gate), 8 frames."""
    scene = rtamd.Scene(8, 1920, 1080, seed=2)
    on, info_on = render(scene, 8, spp=4096)
    off, info_off = render(scene, 8, {"box_interior": 0}, spp=4096)
    assert info_on["box_interior"] == 1 and info_off["box_interior"] == 0, f"{info_on} {info_off}"
    assert info_on["block"] == 1024, info_on
    assert bit_equal(on, off), mismatch_report(on, off)

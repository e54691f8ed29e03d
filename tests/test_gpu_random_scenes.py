"""tests/random_scenes.py on the device, against the CPU oracle bit for bit: one test per family, its scenes from
the smallest n up.  Per scene, at 29x21 (ragged right column and bottom row of tiles), depth 5, spp 6:
  * at default options two launches, frames 1-3 then 4-6 (the running mean across launches), each checked as
    tests/test_gpu_kernel_matrix.py checks its launches (kernel_matrix.launch): planned on the host from the
    scene, the device's resident waves and its free memory, then all 21 rt_debug_last_launch fields, the four
    first-leaf words and the tile counts equal to the plan; the image equals the oracle's;
  * the same under one option set of test_gpu_adversarial.OFF and under one of kernel_matrix.STAGING's three
    non-default states, each rotating over the scene index, against the same oracle image;
  * every fourth scene through the tile-mask twin: from an image of distinct bit patterns tiles 0, 3, 8, 11
    (both corners, a right-edge and a bottom-edge tile), the words outside them untouched, then the other
    eight tiles through the same twin and the whole image equal to the oracle's;
  * every fourth scene (another fourth) as rank 1 of 3 with stripes of 8 rows: the oracle's rows 8-15;
  * with n <= 200 the first-hit buffers (rt_render_features) equal tests/features_ref.py's brute-force closest
    hit with no tied pixel allowed, on the reference tree and under set_bvh_mode("sah").  rt_features.hip
    traces at time 0, which is the reference's, so the moving spheres are in.
No tolerance anywhere; one context per configuration.
"""
import time

import numpy as np
import pytest
import torch

import features_ref
import kernel_matrix as km
import random_scenes as rs
import rtamd
from helpers import bit_equal, mismatch_report
from test_gpu_adversarial import OFF

pytestmark = pytest.mark.gpu

BY_FAMILY = rs.by_family()
OPTION_SETS = [o for o in OFF if o]
STAGINGS = ["dense", "ordered1", "direct"]
PARTITION = (1, 3, 8)   # rank, world, stripe_rows


def variations(index):
    """What scene `index` runs beside its default render: (option set, staging state, mask twin?, partition?)."""
    return (OPTION_SETS[index % len(OPTION_SETS)], STAGINGS[index % len(STAGINGS)], index % 4 == 0, index % 4 == 2)


def test_every_variation_meets_every_family():
    assert len(OPTION_SETS) == 9 and set(STAGINGS) == set(km.STAGING) - {"staged"}
    for family, rows in BY_FAMILY.items():
        v = [variations(i) for i, _ in rows]
        assert len({tuple(sorted(o.items())) for o, _, _, _ in v}) == len(OPTION_SETS), family
        assert {s for _, s, _, _ in v} == set(STAGINGS), family
        assert sum(m for _, _, m, _ in v) >= 4 and sum(p for _, _, _, p in v) >= 4, family
    for o in OPTION_SETS:   # every non-empty set on at least ten scenes
        assert sum(variations(i)[0] == o for i in range(len(rs.SCENES))) >= 10, o


def pattern(base=0x3F800000):
    """A distinct positive finite float per word: bits base + index (tests/test_gpu_kernel_matrix.py pattern)."""
    bits = np.uint32(base) + np.arange(rs.H * rs.W * 4, dtype=np.uint32)
    out = bits.view(np.float32).reshape(rs.H, rs.W, 4).copy()
    assert np.isfinite(out).all() and (out > 0).all()
    return out


def pixels_of(tiles):
    """Tile indices -> per-pixel bool [H, W]."""
    t = np.zeros(rs.NT, bool)
    t[tiles] = True
    return np.repeat(np.repeat(t.reshape(rs.TY, rs.TX), 8, axis=0), 8, axis=1)[:rs.H, :rs.W]


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def context(scene, options=None, **kw):
    ctx = rtamd.RenderContext(devices=(0,), options=options or None, **kw)
    ctx.upload_scene(scene)
    ctx.set_params(max_depth=rs.DEPTH, spp=rs.FRAMES)
    ctx.resize(rs.W, rs.H)
    return ctx


def run_full(label, scene, ref, options, waves, partition=None):
    """Two launches of three frames, each equal to its plan; the image (a partition: its rows) equals the oracle's."""
    kw = {} if partition is None else dict(zip(("rank", "world", "stripe_rows"), partition))
    ctx = context(scene, options, **kw)
    try:
        if partition is None:   # (rt_read_tile_frames does not serve a partition)
            start = ctx.read_tile_frames()
            assert start.size == rs.NT and not start.any()
        kernels = [km.launch(ctx, None, label, scene, options, None, first, rs.LAUNCH, waves, partition=partition)
                   for first in (1, rs.LAUNCH + 1)]
        assert kernels[0] == kernels[1], (label, kernels)
        img = ctx.read_image()
        if partition is None:
            assert (ctx.read_tile_frames() == rs.FRAMES).all()
        else:
            ref = ref[rtamd.stripe_rows_of(rs.H, *partition)]
        assert img.shape == ref.shape and bit_equal(img, ref), f"{label} {kernels[0]}: {mismatch_report(img, ref)}"
        return kernels[0]
    finally:
        ctx.close()


def run_masked(label, scene, ref, waves):
    """The mask twin, as tests/test_gpu_kernel_matrix.py run(): the four tiles over a pattern, then the rest."""
    ctx = context(scene)
    try:
        pat = pattern()
        ctx.write_image(pat)
        active = np.zeros(rs.NT, np.uint8)
        active[rs.MASK] = 1
        ctx.set_active_tiles(active)
        start = ctx.read_tile_frames()
        assert start.size == rs.NT and not start.any()
        kernels = [km.launch(ctx, None, label, scene, {}, rs.MASK, first, rs.LAUNCH, waves) for first in (1, rs.LAUNCH + 1)]
        assert kernels[0] == kernels[1] and kernels[0][1] & km.MASKED, (label, kernels)
        img, counts = ctx.read_image(), ctx.read_tile_frames()
        px = pixels_of(rs.MASK)
        assert int(px.sum()) == 64 + 2 * 40 + 25   # tile 3: 5 wide, tile 8: 5 high, tile 11: 5 x 5
        assert bit_equal(img[px], ref[px]), \
            f"{label}: {mismatch_report(np.where(px[..., None], img, 0), np.where(px[..., None], ref, 0))}"
        assert same_bits(img[~px], pat[~px]), f"{label}: words outside the active tiles changed"
        want = start.copy()
        want[rs.MASK] = rs.FRAMES
        assert np.array_equal(counts, want), (label, counts)
        active = np.ones(rs.NT, np.uint8)
        active[rs.MASK] = 0
        ctx.set_active_tiles(active)
        rest = km.launch(ctx, None, label + " rest", scene, {}, rs.REST, 1, rs.FRAMES, waves)
        assert rest == kernels[0], (label, rest, kernels)
        img = ctx.read_image()
        assert (ctx.read_tile_frames() == rs.FRAMES).all()
        assert bit_equal(img, ref), f"{label} rest: {mismatch_report(img, ref)}"
    finally:
        ctx.close()


def features(scene, bvh_mode=None):
    ctx = context(scene)
    try:
        if bvh_mode:
            ctx.set_bvh_mode(bvh_mode)
        ctx.render_features()
        return ctx.read_features()
    finally:
        ctx.close()


def run_features(label, scene):
    """The first-hit buffers against the brute-force closest hit, no tie allowed (a tie would let a wrong prim id
    through; the seeds of tests/random_scenes.py have none), on the reference tree and on the SAH tree."""
    ref = features_ref.reference(scene)
    assert not ref.tied.any(), f"{label}: {int(ref.tied.sum())} tied pixels: replace the seed"
    nd0, alb0, ids0 = features(scene)
    features_ref.check(ref, nd0, alb0, ids0)
    miss = ids0 == features_ref.MISS
    assert (nd0[miss] == np.array([0, 0, 0, -1], np.float32)).all() and (alb0[miss] == ref.background).all()
    nd, alb, ids = features(scene, "sah")
    assert bit_equal(nd[..., 3], nd0[..., 3]), label
    assert np.array_equal(ids, ids0), label
    features_ref.check(ref, nd, alb, ids)


@pytest.mark.parametrize("family", rs.FAMILIES)
def test_family_matches_oracle(gpu, family):
    waves = torch.cuda.get_device_properties(0).multi_processor_count * 16
    reached = set()
    t_oracle = t_feat = 0.0
    t0 = time.perf_counter()
    for index, args in BY_FAMILY[family]:
        scene = rs.built(index)
        t = time.perf_counter()
        ref = rs.oracle(index)[0]
        t_oracle += time.perf_counter() - t
        label = f"{index} {args}"
        options, staging, masked, partitioned = variations(index)
        reached.add(run_full(label, scene, ref, {}, waves))
        reached.add(run_full(f"{label} {options}", scene, ref, options, waves))
        reached.add(run_full(f"{label} {staging}", scene, ref, km.STAGING[staging], waves))
        if masked:
            run_masked(label + " mask", scene, ref, waves)
        if partitioned:
            run_full(label + " rank 1 of 3", scene, ref, {}, waves, partition=PARTITION)
        if args[1] <= rs.FEATURES_MAX_N:
            t = time.perf_counter()
            run_features(label, scene)
            t_feat += time.perf_counter() - t
    print(f"family {family}: {len(BY_FAMILY[family])} scenes, {time.perf_counter() - t0:.2f} s "
          f"(oracle {t_oracle:.2f} s, first-hit part {t_feat:.2f} s), kernels {sorted(reached)}")

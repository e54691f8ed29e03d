"""From scene bytes to the kernel arguments on the host (csrc/rt_args.h, through rt_debug_plan_scene; no
GPU needed): what rt_render assembles for a scene -- the walk's trees, the scene's half of the argument
block, the unit split, the reported launch fields and the frame counts.

tests/golden/scene_plan.npz holds what the commit before rt_args.cpp assembled inside rt_render
(tests/golden/scene_plan.md): scenes 0-9 at 1920x1080 / 64 frames and at 64x48 / 3 frames, and on scenes
8, 6 and 0 each layout option alone, both rebuild modes, sphere pairs off / forced, a node cap, the SAH
tree, the moments, tile masks, a partition and frame sequences.  rt_debug_plan_scene must give every row
alike.  The frame-count rule is checked against its restatement below, not against the library.
"""
import itertools
import json
import os
import zlib

import numpy as np
import pytest

import rtamd
from test_launch_plan import PK

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "scene_plan.npz")
LI = {n: k for k, n in enumerate(rtamd.render.LAUNCH_FIELDS)}
SCENE_FIELDS = ("bvh_mode", "box_vnodes", "collapsed", "rebuilt")   # rt_debug_last_launch's, filled by rt_render


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    g = {k: z[k] for k in z.files}
    g["rows"] = json.loads(str(z["rows"]))
    return g


def frames_in(packed, nt):
    """A row's recorded counts -> (uniform count, per-tile array or None).  -1 pads a uniform count."""
    if packed[1] == -1:
        return int(packed[0]), None
    v = packed[:nt].astype(np.int32)
    return (int(v[0]), None) if (v == v[0]).all() else (int(v.min()), v)


def run_row(g, k, scenes):
    r = g["rows"][k]
    key = (r["scene"], r["width"], r["height"])
    if key not in scenes:
        scenes[key] = rtamd.Scene(r["scene"], r["width"], r["height"], seed=1)
    nt = ((r["width"] + 7) // 8) * ((rtamd.local_rows(r["height"], r["rank"], r["world"], r["stripe_rows"]) + 7) // 8)
    before = g["frames_before"][k]
    prev, prev_tiles = (0, None) if before[0] == -2 else frames_in(before, nt)   # -2: a partition (not readable)
    return rtamd.plan_scene(scenes[key], r["n_frames"], first_frame=r["first_frame"], options=r["options"],
                            bvh_mode=r["bvh_mode"], moments=r["moments"], mask=r["mask"], prev_frames=prev,
                            prev_tile_frames=prev_tiles, rank=r["rank"], world=r["world"], stripe_rows=r["stripe_rows"],
                            max_depth=r["max_depth"], spp=r["spp"], waves=int(g["waves"]), free_bytes=int(g["free_bytes"]),
                            want_links=True, want_args=True), nt


def test_fixture_holds_the_rows_the_comparison_stands_on(golden):
    rows = golden["rows"]
    names = {r["name"].split("#")[0] for r in rows}
    assert {f"s{s}_1080p" for s in range(10)} | {f"s{s}_small" for s in range(10)} <= names
    for s in (8, 6, 0):
        for tag in ("compact_boxes_0", "box_pretest_0", "fastdiv_0", "spine_0", "collapse_0", "first_leaf_0",
                    "box_interior_0", "box_vnodes_0", "shade_lds_0", "perlin_packed_0", "big_wg_0", "leaf_prefetch_0",
                    "rebuild_0", "rebuild_1", "sphere_pairs_0", "sphere_pairs_2", "lds_node_cap", "two_level", "sah", "moments", "mask3",
                    "mask_empty", "world2_rank1", "frames"):
            assert f"s{s}_{tag}" in names, (s, tag)
    assert len(str(golden["parent"])) == 40
    assert golden["args"].shape[0] == len(rows) == golden["last_launch"].shape[0]
    assert golden["first_leaf"][:, 0].any() and golden["last_launch"][:, LI["collapsed"]].any()
    assert golden["last_launch"][:, LI["box_vnodes"]].any() and golden["last_launch"][:, LI["bvh_mode"]].any()


def test_plan_scene_equals_the_parent_on_every_row(golden):
    """Every non-pointer byte of the first launch's argument block but the rand factors, the four pointers the
    launch decision asks about, the scene's last_launch fields, the first-leaf words, the links and the frame
    counts.  The other pointers' null / non-null states (the fixture's `pointers`) belong to the device's
    buffers: no context-free entry has them."""
    scenes = {}
    ptr = {str(n): k for k, n in enumerate(golden["pointer_names"])}
    for k, r in enumerate(golden["rows"]):
        got, nt = run_row(golden, k, scenes)
        name = r["name"]
        assert got["launched"] == (r["launches"] > 0), name
        bad = np.nonzero(got["args"] != golden["args"][k])[0]
        assert bad.size == 0, (name, "argument block differs at bytes", bad[:8])
        if got["launched"]:
            for pk, p in (("SAMPLES", "samples"), ("SFLAGS", "sflags"), ("WBUF", "wbuf"), ("TILE_LIST", "tile_list")):
                assert got["pk"][PK[pk]] == golden["pointers"][k][ptr[p]], (name, p)
            for f in SCENE_FIELDS:
                assert got[f] == golden["last_launch"][k][LI[f]], (name, f)
            assert [x & 0xFFFFFFFF for x in got["first_leaf"]] == [int(x) & 0xFFFFFFFF for x in golden["first_leaf"][k]], name
        assert got["links"].size == 4 * golden["links_f4"][k], name
        assert zlib.crc32(got["links"].tobytes()) == golden["links_crc"][k], name
        after = golden["frames_after"][k]
        if after[0] != -2:
            lo, tiles = frames_in(after, nt)
            want = tiles if tiles is not None else np.full(nt, lo, np.int32)
            assert np.array_equal(got["tile_frames"], want), (name, got["tile_frames"], want)


def test_plan_scene_then_plan_kernel_reports_the_parents_launch(golden):
    """rt_debug_plan_scene's pk fed to rt_debug_plan_kernel, with the scene's four fields, is the whole
    rt_debug_last_launch the parent reported."""
    from test_launch_plan import plan
    scenes = {}
    for k, r in enumerate(golden["rows"]):
        got, _ = run_row(golden, k, scenes)
        if not got["launched"]:
            continue
        out, info = plan(got["pk"][None, :], [0])
        assert out[0][0] == 1, r["name"]
        for f in SCENE_FIELDS:
            info[0][LI[f]] = got[f]
        assert np.array_equal(info[0], golden["last_launch"][k]), (r["name"], info[0], golden["last_launch"][k])


def rule(before, mask, first_frame, n_frames):
    """The frame-count rule (csrc/rt_args.h, SceneState group 5) restated: a sampled tile restarts from frame 1,
    extends from its count + 1, else becomes invalid; the others keep theirs."""
    after = list(before)
    for t in (range(len(before)) if mask is None else mask):
        c = before[t]
        after[t] = first_frame - 1 + n_frames if first_frame == 1 or (c > 0 and first_frame == c + 1) else 0
    return after


def test_frame_counts_follow_the_rule():
    """4 tiles (a 16x16 image): previous counts uniform or per tile, no mask / one tile / two / none, and
    first_frame 1, count + 1 of some tile, and a gap: 240 cases against the restatement above."""
    scene = rtamd.Scene(6, 16, 16, seed=1)
    befores = [[0] * 4, [3] * 4, [3, 0, 3, 5], [2, 2, 4, 4], [0, 0, 0, 7]]
    masks = [None, [2], [0, 3], []]
    n = 0
    for before, mask, first, nf in itertools.product(befores, masks, (1, 3, 4, 6), (1, 2, 5)):
        uniform = len(set(before)) == 1
        got = rtamd.plan_scene(scene, nf, first_frame=first, mask=mask, prev_frames=min(before),
                               prev_tile_frames=None if uniform else before)
        assert list(got["tile_frames"]) == rule(before, mask, first, nf), (before, mask, first, nf)
        assert got["launched"] == (mask != []), (mask,)
        n += 1
    assert n == 240


def test_argument_errors():
    scene = rtamd.Scene(6, 16, 16, seed=1)
    for kw in (dict(first_frame=0), dict(mask=[4]), dict(mask=[1, 1]), dict(mask=[-1]), dict(width=-1), dict(world=2, rank=2),
               dict(max_depth=-1), dict(bvh_mode=2), dict(options={"sphere_pairs": 3}), dict(options={"kernel_variant": 37})):
        with pytest.raises(rtamd.RTError):
            rtamd.plan_scene(scene, 2, **kw)
    assert rtamd.plan_scene(scene, 2, options={"kernel_variant": 37}, ab=True)["pk"][PK["VARIANT"]] == 37
    assert rtamd.plan_scene(scene, 0)["launched"] == 0

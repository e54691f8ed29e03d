"""tests/random_scenes.py on the host (no GPU): every scene of SCENES builds, rt_debug_plan_scene accepts it at
default options, the CPU oracle renders it and the image carries radiance; and over the whole list the planner
is driven, by what the scenes contain alone, through the kernels, launch fields and prim tests that
tests/test_gpu_random_scenes.py then runs on the device.  Planned as that file renders: 29x21, a launch of 3
frames, spp 6, depth 5, the MI355X's 4096 resident waves.
"""
import functools

import numpy as np
import pytest

import kernel_matrix as km
import random_scenes as rs
import rtamd
from test_launch_plan import LI

WAVES, FREE = 256 * 16, 1 << 38
BY_FAMILY = rs.by_family()


@functools.lru_cache(maxsize=None)
def plan_of(index):
    """(last_launch list, first-leaf words, (block, opt)) of SCENES[index]'s first launch at default options."""
    launch, leaf, counts, kernel = km.planned(rs.built(index), rs.LAUNCH, 1, {}, None, np.zeros(rs.NT, np.int32),
                                              WAVES, FREE, spp=rs.FRAMES)
    assert (counts == rs.LAUNCH).all() and counts.size == rs.NT
    return launch, leaf, kernel


def lit_share(img):
    """The share of pixels with a non-zero colour (a NaN is no colour)."""
    rgb = img[..., :3]
    return float(((rgb != 0) & ~np.isnan(rgb)).any(-1).mean())


def test_list_shape():
    assert len(rs.SCENES) == len(set(rs.SCENES)) == 152 and set(BY_FAMILY) == set(rs.FAMILIES) and len(rs.FAMILIES) == 8
    assert rs.W % 8 == 5 and rs.H % 8 == 5 and rs.NT == ((rs.W + 7) // 8) * ((rs.H + 7) // 8) == 12
    assert set(rs.MASK) == {0, rs.TX - 1, (rs.TY - 1) * rs.TX, rs.NT - 1}
    for family, rows in BY_FAMILY.items():
        ns = [a[1] for _, a in rows]
        assert ns == sorted(ns) and set(ns) == set(rs.SIZES) >= {1, 2, 3, 9, 40, 200, 1000, 2500}, family
        assert {a[3] for _, a in rows} == {4.0, 300000.0} and {a[4] for _, a in rows} == {False, True}, family
        for n in rs.SIZES:   # every size at both spreads
            assert {a[3] for _, a in rows if a[1] == n and not a[4]} == {4.0, 300000.0}, (family, n)
        assert [i for i, _ in rows] == list(range(rows[0][0], rows[0][0] + len(rows)))   # one block of SCENES


def test_scene_is_deterministic():
    for index in (0, 60, 125, 151):
        a, b = rs.scene(*rs.SCENES[index]), rs.built(index)
        assert all(a.buffers[k] == b.buffers[k] for k in range(6)) and np.array_equal(a.camera, b.camera)
        assert [t.data for t in a.textures] == [t.data for t in b.textures]
        a.close()


@pytest.mark.parametrize("family", rs.FAMILIES)
def test_family_builds_plans_renders_and_is_lit(family):
    for index, args in BY_FAMILY[family]:
        scene = rs.built(index)
        info = scene.info
        n = args[1] + (1 if args[4] else 0)
        assert info["n_bvh_prims"] == n, (args, info)   # media count once: their boundaries sit in no leaf
        assert (info["width"], info["height"]) == (rs.W, rs.H)
        launch, leaf, kernel = plan_of(index)
        assert launch[LI["tiles_active"]] == rs.NT and launch[LI["block"]] == kernel[0] and not kernel[1] & km.MASKED
        img, counters = rs.oracle(index)
        assert counters["samples"] == rs.W * rs.H * rs.FRAMES
        assert lit_share(img) >= 0.25, (args, lit_share(img))


def test_what_the_families_contain():
    """Prim kinds, light counts, defocus, materials and textures, read back from the packed records."""
    lights, defocus, mats, tex_types = {}, {}, {}, {}
    for family, rows in BY_FAMILY.items():
        for index, args in rows:
            s = rs.built(index)
            lights.setdefault(family, set()).add(min(s.info["n_lights"], 2))
            defocus.setdefault(family, set()).add(bool(s.camera[3] > 0))
            sph = np.frombuffer(s.buffers[0], np.int32).reshape(-1, 12)
            quads = np.frombuffer(s.buffers[2], np.int32).reshape(-1, 20)
            mats.setdefault(family, set()).update(((sph[:, 11] >> 16) & 0xFFFF).tolist(), ((quads[:, 7] >> 16) & 0xFFFF).tolist())
            tex_types.setdefault(family, set()).update(((sph[:, 3] >> 28) & 0xF).tolist())
    for family in rs.FAMILIES:
        assert lights[family] == {0, 1, 2} and defocus[family] == {False, True}, family   # no, one, several lights
    big = {f: rs.built(BY_FAMILY[f][-1][0]).info for f in rs.FAMILIES}   # the 2500-prim scene
    assert big["spheres"]["n_quads"] <= 2 and big["spheres"]["n_boxes"] == 0 and big["spheres"]["n_media"] == 0
    assert big["boxes"]["n_spheres"] <= 1 and big["boxes"]["n_boxes"] > 2400
    assert big["quads"]["n_quads"] == 2500
    for family in rs.MIXED:
        i = big[family]
        assert min(i["n_spheres"], i["n_quads"], i["n_boxes"], i["n_media"]) > 100, (family, i)
    for family in ("textured", "mixed"):   # sphere records: lambertian, metal, dielectric, light; image, checker, Perlin, solid
        assert mats[family] >= {0, 1, 2, 3} and tex_types[family] >= {1, 2, 3, 4}, (family, mats[family], tex_types[family])
    assert tex_types["spheres"] <= {0, 4}   # solid colours only (0: a dielectric or a light has no texture)


def test_instances_reached_at_default_options():
    kernels = {plan_of(i)[2] for i in range(len(rs.SCENES))}
    assert kernels == rs.REACHED and len(kernels) >= 19
    assert kernels <= set(km.ROWS)
    # today the matrix reaches these through an option alone (shade_lds 0, lds_node_cap, compact_boxes 0, big_wg 0,
    # fastdiv 0); here prims that outgrow LDS and an extent past 2^20 do
    assert {(512, 47), (1024, 47), (1024, 63), (512, 79), (1024, 79), (1024, 15), (512, 43), (512, 75)} <= kernels
    for k in kernels:
        assert km.ROWS[k][1] or k in ((1024, 431), (512, 207), (512, 431)), k


def test_launch_fields_take_both_sides():
    seen = {f: set() for f in rtamd.render.LAUNCH_FIELDS}
    armed = set()
    for i in range(len(rs.SCENES)):
        launch, leaf, _ = plan_of(i)
        for f in seen:
            seen[f].add(launch[LI[f]])
        armed.add(leaf[0])
    for f in ("fastdiv", "rebuilt", "sphere_pairs", "box_interior", "leaf_prefetch"):
        assert seen[f] == {0, 1}, (f, seen[f])
    assert armed == {0, 1}
    for f in ("collapsed", "spine", "box_vnodes"):
        assert 0 in seen[f] and max(seen[f]) > 0, (f, seen[f])
    assert seen["shape"] == {2, 5}
    assert seen["walk_frac"] == {8, 32, 48}
    assert seen["block"] == {512, 1024}
    assert len(seen["shade_lds"]) >= 4, seen["shade_lds"]


def test_fastdiv_follows_the_extent():
    """The planner drops the shared-reciprocal division because of the scene, not an option: a spread of 300000
    puts coordinates past 2^20."""
    for i, args in enumerate(rs.SCENES):
        if not args[4]:
            assert plan_of(i)[0][LI["fastdiv"]] == (1 if args[3] == 4.0 else 0), args


def test_mixed_families_run_every_prim_test():
    for family in rs.MIXED:
        full = [a for i, a in BY_FAMILY[family]
                if all(rs.oracle(i)[1][c] > 0 for c in ("sphere_tests", "quad_tests", "box_tests", "medium_tests"))]
        assert full, family

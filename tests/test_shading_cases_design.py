"""The shading cases (tests/adversarial.py shading_cases) aim where they claim (no GPU): by the oracle's
counters, plain geometry and the host-side launch plan (rt_debug_plan_scene)."""
import numpy as np
import pytest

import adversarial
import pyoracle
import rtamd
from rtamd.render import plan_scene
from test_adversarial_design import camera_rays
from test_launch_plan import PK

CASES = adversarial.shading_cases()
UV_ALWAYS_AT = 80   # rt_kernel_args (csrc/rt_device.h): nine pointers, n_nodes, lights_count, then uv_always


def launch_facts(case, lib=None):
    """Asserts what the default launch of the case must show in rt_debug_plan_scene's RT_PK_* inputs and
    argument block; returns them."""
    p = plan_scene(case.scene, case.frames, max_depth=case.depth, want_args=True, lib=lib)
    pk = p["pk"]
    uv_always = int(p["args"][UV_ALWAYS_AT:UV_ALWAYS_AT + 4].view(np.int32)[0])
    assert p["launched"] == 1
    if case.name == "media_box_all_compact":
        assert pk[PK["BOX_ALL_CMP"]] == 1 and pk[PK["MEDIA_SPH"]] == 0 and pk[PK["N_MEDIA"]] == 1, pk
    if case.name == "media_64":
        assert pk[PK["N_MEDIA"]] == 64 and pk[PK["MEDIA_LDS"]] >= 0, pk
    if case.name == "media_65":
        assert pk[PK["N_MEDIA"]] == 65 and pk[PK["MEDIA_LDS"]] == -1, pk
    if case.name == "textures_edges":
        assert pk[PK["PERLIN_LDS"]] >= 0, pk
    assert uv_always == (1 if case.name == "media_image_texture" else 0), (case.name, uv_always)
    return pk, uv_always


@pytest.fixture(scope="module")
def rendered():
    out = {}
    for c in CASES:
        o = pyoracle.OracleScene(c.scene, max_depth=c.depth, uniforms=c.uniforms)
        out[c.name] = pyoracle.render(o, rtamd.frame_rand_factors(1, 0, c.frames), counters=True)
    return out


def test_sizes_are_small():
    for c in CASES:
        assert c.scene.width <= 64 and c.scene.height <= 48 and c.frames <= 4 and c.depth <= 5, c.name


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_launch_path(case):
    launch_facts(case)


def test_nan_only_where_a_shading_point_lies_inside_a_light(rendered):
    for name, (img, _) in rendered.items():
        nan = int(np.isnan(img[..., :3]).any(axis=-1).sum())
        if name == "light_inside":
            assert nan >= 50, nan   # the quad's strip inside the sphere, seen directly and through the glass
        else:
            assert nan == 0, (name, nan)


def test_counters_show_the_targets(rendered):
    for name, (_, cnt) in rendered.items():
        assert cnt["light_bytes"] > 0, name                      # every case samples its lights
        media = name.startswith("media_") or name == "lights_many"
        assert (cnt["medium_tests"] > 0) == media, (name, cnt["medium_tests"])
    assert rendered["media_65"][1]["medium_tests"] > 5000 and rendered["media_64"][1]["medium_tests"] > 5000


def test_lights_many_registers_five_lights_one_moving():
    s = next(c for c in CASES if c.name == "lights_many").scene
    lights = np.frombuffer(s.buffers[5], np.int32)
    assert lights[0] == 5, lights[:8]
    sph = np.frombuffer(s.buffers[0], np.float32).reshape(-1, 12)
    assert (np.abs(sph[:, 4:7]).sum(axis=1) > 0).sum() == 1      # center_vec != 0: the moving light


def test_grid_rays_meet_quad_edges_and_checker_boundaries():
    """textures_edges, from the scene's own camera block, quad records and checker texel: the camera rays that
    meet the image quad with alpha or beta exactly 0 or 1, and those that meet the checker floor with a
    coordinate exactly on a cell boundary (p / scale a whole number), computed in float64 from the float32
    records (exact for these binary fractions)."""
    s = next(c for c in CASES if c.name == "textures_edges").scene
    o, d = camera_rays(s)
    o, d = o.astype(np.float64), d.astype(np.float64).reshape(-1, 3)
    quads = np.frombuffer(s.buffers[2], np.float32).reshape(-1, 20)
    ids = quads.view(np.int32)[:, 11]
    kind = (ids >> 28) & 0xF
    assert (kind == 1).sum() == 1 and (kind == 2).sum() == 1
    iq, fq = int(np.argmax(kind == 1)), int(np.argmax(kind == 2))    # the image quad, the checker floor

    def plane_hits(rec):
        n, dd, q, u, v = (rec[0:3].astype(np.float64), float(rec[3]), rec[4:7].astype(np.float64),
                          rec[8:11].astype(np.float64), rec[12:15].astype(np.float64))
        with np.errstate(all="ignore"):                                  # rays parallel to the plane: inf / NaN, never inside
            t = (dd - n @ o) / (d @ n)
            p = o + d * t[:, None]
            w = np.cross(u, v)
            w = w / (w @ w)
            al, be = np.cross(p - q, v) @ w, np.cross(u, p - q) @ w   # Quad.java's plane coordinates
            return t, p, al, be, (t >= 0.001) & (al >= 0) & (al <= 1) & (be >= 0) & (be <= 1)

    t, p, al, be, inside = plane_hits(quads[iq])
    edge = inside & ((al == 0) | (al == 1) | (be == 0) | (be == 1))
    corners = inside & ((al == 0) | (al == 1)) & ((be == 0) | (be == 1))
    assert inside.sum() == 45 and edge.sum() == 24 and corners.sum() == 4, (inside.sum(), edge.sum(), corners.sum())

    tex = next(x for x in s.textures if x.slot == ((ids[fq] >> 12) & 0xFFFF))
    scale = np.frombuffer(tex.data, np.uint8)[((ids[fq] & 0xFFF) * 3 + 2) * 3] / 255.0   # the checker's third texel, red
    assert scale == 1.0
    tf, pf, _, _, on_floor = plane_hits(quads[fq])
    on_floor &= ~(inside & (t < tf))                                  # not behind the image quad
    cell = pf / scale
    whole = cell == np.round(cell)
    assert on_floor.sum() > 1000 and (whole[on_floor, 1]).all()       # y = -2 is a boundary for every floor hit
    assert (pf[on_floor, 0] < 0).sum() > 400                          # negative x: truncation toward zero matters
    on_z, on_xz = on_floor & whole[:, 2], on_floor & whole[:, 2] & whole[:, 0]
    assert on_z.sum() >= 3 * 32 and on_xz.sum() >= 16 + 8 + 4, (on_z.sum(), on_xz.sum())

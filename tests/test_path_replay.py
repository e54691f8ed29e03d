"""The path loop replayed link by link (tests/path_replay.py) with the CPU oracle's own ops -- CAMERA_RAY, then
TRACE and SHADE per bounce, the fold in numpy float32 -- against the oracle's render, bit for bit (NaN
positions included).  Every op the replay uses is pinned to float64 on its own (tests/test_shade_ref64.py,
tests/test_trace_ref64.py), so this pins the oracle's sample end to end without following a chaotic path in
float64: what remains in the oracle's ray_color / shade_pixel besides those ops is the loop the replay restates
from compute.glsl:298-358 -- rf, time and the uv source threaded through, acc * background on a miss, vec3(0)
when max_depth runs out, the fold (prev * (n - 1) + cur) / n.  No GPU.

A capped subset (512 rows each) of the replay's own TRACE rows (its bounce rays) of scenes 7 and 8 also goes
through the float64 walk, by test_trace_ref64's rules for decided rows."""
import numpy as np
import pytest

import path_replay
import pyoracle
import rtamd
import trace_cases

W, H, FRAMES = 16, 12, 4
SCENES = ["scene6", "scene7", "scene8", "knot"]
_made = {}


def made(name, depth):
    """(scene, uniforms, OracleScene at max_depth = depth, rand factors)."""
    if (name, depth) not in _made:
        if name == "knot":
            sc, uni = trace_cases.scene("knot")
        else:
            sc, uni = rtamd.Scene(int(name[5:]), W, H, seed=1), rtamd.spp_uniforms(FRAMES)
        assert (sc.width, sc.height) == (W, H)
        rf = rtamd.frame_rand_factors(1, 0, FRAMES)
        _made[name, depth] = (sc, uni, pyoracle.OracleScene(sc, max_depth=depth, uniforms=uni), rf)
    return _made[name, depth]


@pytest.mark.parametrize("depth", [5, 1, 2])
@pytest.mark.parametrize("name", SCENES)
def test_replay_with_the_oracles_ops_equals_its_render(name, depth):
    sc, _, osc, rf = made(name, depth)
    ops = path_replay.OracleOps(osc)
    image, want, curs = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32), []
    for k in range(FRAMES):   # frames 1..4, each compared as the render leaves it
        curs.append(path_replay.sample(ops, W, H, depth, sc.background, k + 1, rf[k]))
        image = path_replay.fold(image, curs[-1], k + 1)
        pyoracle.render(osc, rf[k:k + 1], first_frame=k + 1, image=want)
        assert path_replay.same_bits(image, want), f"{name} depth {depth}: frame {k + 1} differs from oracle_render"
    curs = np.stack(curs)
    if depth == 5:
        # the run is not trivial: paths end by a miss, by the shading and by running out of depth
        assert np.isfinite(curs).any() and (curs != 0).any()


def test_depth_runs_out_to_black():
    """max_depth 1 on the knot: a pixel whose first hit scatters on has colour vec3(0), not acc * background."""
    sc, _, osc, rf = made("knot", 1)
    rec = []
    _, curs = path_replay.render(path_replay.OracleOps(osc), W, H, 1, sc.background, rf[:1], record=rec)
    w = pyoracle.eval_shade_op(osc, "trace", rec[0])
    hit = (w[:, 0] != 0).reshape(H, W)
    assert hit.any() and (~hit).any()
    bg = np.asarray(sc.background, np.float32)
    assert (curs[0][~hit] == bg).all()                       # acc = 1 on the first bounce
    lit = (curs[0][hit] != 0).any(axis=1)                    # a first hit on the light ends the path with its colour
    assert (~lit).any(), "no pixel's path ran out of depth"


@pytest.mark.parametrize("name", ["scene7", "scene8"])
def test_replays_bounce_rays_against_float64(name):
    import test_trace_ref64
    sc, uni, osc, rf = made(name, 5)
    rec = []
    path_replay.render(path_replay.OracleOps(osc), W, H, 5, sc.background, rf, record=rec)
    rows = np.concatenate(rec[1:])   # bounce rays above all: everything after the first frame's camera rays
    assert len(rows) >= 1024
    rows = rows[np.random.default_rng(5).choice(len(rows), 512, replace=False)]
    res = test_trace_ref64.check(sc, osc, rows, f"{name} replay rows", "random")   # asserts the decided rows agree
    print(f"{name}: {res}")
    # Bounce rays start on surfaces at these scenes' scale of 555, and scene 7's fogs are box-bounded: the second
    # boundary pass meets the first pass's side again within 0.0001, far below the rounding bound there, so about a
    # seventh of scene 7's rows and a sixteenth of scene 8's are undecided (scene 8: 78 of 512 rows are out of scope
    # besides, NaN or a zero direction).  The 5 % cap is the random sets'; here the decided rows must only be most.
    assert res["undecided_share"] < 0.5 and res["out_of_scope"] < len(rows) // 2, res
    assert res["draws"] > 0 and 0.01 <= res["worst_error_over_bound"]["t"] <= 1.0, res

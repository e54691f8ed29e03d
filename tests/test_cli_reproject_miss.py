"""rtrender --moves --move-misses (raytracing-book_amd/host/rt_main.cpp): the option and its misuse on the CPU; on
the device, each pose's <output stem>.moveNN.png against the same render_moved() calls made from Python with
set_reproject_misses(), and without the option against the calls without it."""
import numpy as np
import pytest

import rtamd
from test_cli import read_png, run

W, H, SEED = 40, 24, 1
F = np.float32
MOVES = ["--moves", "2", "--move-shift", "0.05", "--move-frames", "1", "-o", "x.png"]


def test_help_lists_the_option():
    r = run("--help")
    assert r.returncode == 0, r.stderr
    assert any(ln.split()[:1] == ["--move-misses"] and len(ln.split()) > 2 for ln in r.stdout.splitlines()[1:])


@pytest.mark.parametrize("args,msg", [
    (["--move-misses"], "--move-misses goes with --moves"),
    (["--move-misses", "-o", "x.png"], "--move-misses goes with --moves"),
    (["--move-misses", "--move-refine", "2"], "go with --moves"),
    (["--moves", "2", "--move-misses", "-o", "x.png"], "--moves needs --move-shift <S> and --move-frames <N>"),
    (MOVES[:-2] + ["--move-misses"], "--moves needs -o <png>"),
])
def test_misuse_is_refused_before_anything_renders(args, msg):
    r = run(*args)
    assert r.returncode == 1 and msg in r.stderr, (r.stdout, r.stderr)
    assert "All samples have completed" not in r.stdout


def python_run(sid, spp, moves, shift, frames, misses, refine=None):
    """What rtrender --moves [--move-misses] [--move-refine] does, through the Python binding -> one frame per pose."""
    scene = rtamd.Scene(sid, W, H, seed=SEED)
    ctx = rtamd.RenderContext()
    ctx.upload_scene(scene)
    ctx.set_params(max_depth=5, spp=spp)
    ctx.resize(W, H)
    ctx.set_moments(True)
    ctx.set_history_variance(True)
    if misses:
        ctx.set_reproject_misses(True)
    ctx.render_features()
    ctx.render(1, rtamd.frame_rand_factors(SEED, 0, spp))
    cam = np.array(scene.camera, F)
    per = frames + (refine["extra_frames"] if refine else 0)
    out = []
    for k in range(moves):
        v = cam[12:15] * F(shift * W)
        cam[4:7] += v
        cam[8:11] += v
        got = ctx.render_moved(cam, rtamd.frame_rand_factors(SEED, spp + k * per, per), refine=refine)
        out.append(got if refine else (got, None))
    ctx.close()
    return out


@pytest.mark.gpu
def test_each_pose_png_is_the_pose_with_and_without_the_option(gpu, tmp_path):
    frames = {}
    for misses in (False, True):
        out = tmp_path / ("on.png" if misses else "off.png")
        args = ["-s", 8, "-r", f"{W}:{H}", "-spp", 8, "-md", 5, "-o", out, "--moves", 2, "--move-shift", 0.05, "--move-frames", 1]
        r = run(*(args + ["--move-misses"] if misses else args))
        assert r.returncode == 0, r.stderr
        poses = python_run(8, 8, 2, 0.05, 1, misses)
        frames[misses] = []
        for k, (frame, _) in enumerate(poses, 1):
            png = read_png(tmp_path / f"{out.stem}.move{k:02d}.png")
            assert np.array_equal(png, frame[..., :3]), (misses, k)
            assert f"Move {k}/2: 1 frame(s), saved to: " in r.stdout
            frames[misses].append(png)
    assert not np.array_equal(frames[True][0], frames[False][0])              # the option shows


@pytest.mark.gpu
def test_the_option_with_move_refine_names_fewer_tiles(gpu, tmp_path):
    tiles = {}
    for misses in (False, True):
        out = tmp_path / ("on.png" if misses else "off.png")
        args = ["-s", 8, "-r", f"{W}:{H}", "-spp", 8, "-md", 5, "-o", out, "--moves", 1, "--move-shift", 0.05, "--move-frames", 1,
                "--move-refine", 3]
        r = run(*(args + ["--move-misses"] if misses else args))
        assert r.returncode == 0, r.stderr
        (frame, n), = python_run(8, 8, 1, 0.05, 1, misses, refine=dict(extra_frames=3))
        assert np.array_equal(read_png(tmp_path / f"{out.stem}.move01.png"), frame[..., :3]), misses
        assert f"Move 1/1: 1 frame(s), +3 on {n} of 15 tiles, saved to: " in r.stdout
        tiles[misses] = n
    assert tiles[True] < tiles[False]

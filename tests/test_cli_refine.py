"""rtrender --moves --move-refine (raytracing-book_amd/host/rt_main.cpp): the options and their misuse on the
CPU; on the device, each pose's line and <output stem>.moveNN.png against the same render_moved(refine=...)
calls made from Python."""
import numpy as np
import pytest

import rtamd
from test_cli import read_png, run

W, H, SEED = 40, 24, 1
F = np.float32
MOVES = ["--moves", "2", "--move-shift", "0.25", "--move-frames", "1", "-o", "x.png"]


def test_help_lists_the_refine_options():
    r = run("--help")
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    for opt in ("--move-refine <arg>", "--move-refine-count <arg>", "--move-refine-tiles <arg>"):
        assert any(ln.split()[:len(opt.split())] == opt.split() and len(ln.split()) > 2 for ln in lines[1:]), opt


@pytest.mark.parametrize("args,msg", [
    (["--move-refine", "2"], "go with --moves"),
    (["--move-refine-count", "4"], "go with --moves"),
    (["--move-refine-tiles", "4"], "go with --moves"),
    (MOVES + ["--move-refine-count", "4"], "go with --move-refine"),
    (MOVES + ["--move-refine-tiles", "4"], "go with --move-refine"),
    (MOVES + ["--move-refine", "0"], "--move-refine must be at least 1"),
    (MOVES + ["--move-refine=-3"], "--move-refine must be at least 1"),
    (MOVES + ["--move-refine", "2147483647"], "--move-refine is too large"),
    (MOVES + ["--move-refine", "2", "--move-refine-count", "0"], "--move-refine-count must be a finite number > 0"),
    (MOVES + ["--move-refine", "2", "--move-refine-count=-1"], "--move-refine-count must be a finite number > 0"),
    (MOVES + ["--move-refine", "2", "--move-refine-count", "nan"], "--move-refine-count must be a finite number > 0"),
    (MOVES + ["--move-refine", "2", "--move-refine-count", "inf"], "--move-refine-count must be a finite number > 0"),
    (MOVES + ["--move-refine", "2", "--move-refine-count", "4x"], "--move-refine-count must be a finite number > 0"),
    (MOVES + ["--move-refine", "2", "--move-refine-tiles", "0"], "--move-refine-tiles must be at least 1"),
    (MOVES + ["--move-refine", "2", "--move-refine-tiles=-2"], "--move-refine-tiles must be at least 1"),
])
def test_misuse_is_refused_before_anything_renders(args, msg):
    r = run(*args)
    assert r.returncode == 1 and msg in r.stderr, (r.stdout, r.stderr)
    assert "All samples have completed" not in r.stdout


def python_run(sid, spp, moves, shift, frames, refine):
    """What rtrender --moves --move-refine does, through the Python binding -> (frame, tiles refined) per pose."""
    scene = rtamd.Scene(sid, W, H, seed=SEED)
    ctx = rtamd.RenderContext()
    ctx.upload_scene(scene)
    ctx.set_params(max_depth=5, spp=spp)
    ctx.resize(W, H)
    ctx.set_moments(True)
    ctx.set_history_variance(True)
    ctx.render_features()
    ctx.render(1, rtamd.frame_rand_factors(SEED, 0, spp))
    cam = np.array(scene.camera, F)
    per = frames + refine["extra_frames"]
    out = []
    for k in range(moves):
        v = cam[12:15] * F(shift * W)
        cam[4:7] += v
        cam[8:11] += v
        out.append(ctx.render_moved(cam, rtamd.frame_rand_factors(SEED, spp + k * per, per), refine=refine))
    ctx.close()
    return out


@pytest.mark.gpu
def test_each_move_line_and_png_is_the_refined_pose(gpu, tmp_path):
    out = tmp_path / "out.png"
    r = run("-s", 6, "-r", f"{W}:{H}", "-spp", 8, "-md", 5, "-o", out, "--moves", 2, "--move-shift", 0.25, "--move-frames", 1,
            "--move-refine", 3, "--move-refine-count", 4, "--move-refine-tiles", 15)
    assert r.returncode == 0, r.stderr
    poses = python_run(6, 8, 2, 0.25, 1, dict(extra_frames=3, min_count=4.0, max_tiles=15))
    nt = ((W + 7) // 8) * ((H + 7) // 8)
    for k, (frame, tiles) in enumerate(poses, 1):
        png = read_png(tmp_path / f"out.move{k:02d}.png")
        assert np.array_equal(png, frame[..., :3]), k
        assert 0 < tiles <= nt == 15                                         # the leading edge is always fresh
        assert f"Move {k}/2: 1 frame(s), +3 on {tiles} of {nt} tiles, saved to: " in r.stdout

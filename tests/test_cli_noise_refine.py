"""rtrender --moves --move-noise (raytracing-book_amd/host/rt_main.cpp): the options and their misuse on the CPU;
on the device, each pose's line and <output stem>.moveNN.png against the same render_moved(noise_refine=...) calls
made from Python."""
import numpy as np
import pytest

import rtamd
from test_cli import read_png, run

W, H, SEED = 40, 24, 1
F = np.float32
MOVES = ["--moves", "2", "--move-shift", "0.25", "--move-frames", "1", "-o", "x.png"]
NOISE = MOVES + ["--move-noise", "0.1"]


def test_help_lists_the_noise_options():
    r = run("--help")
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    for opt in ("--move-noise <arg>", "--move-noise-batch <arg>", "--move-noise-rounds <arg>", "--move-noise-count <arg>"):
        assert any(ln.split()[:len(opt.split())] == opt.split() and len(ln.split()) > 2 for ln in lines[1:]), opt


@pytest.mark.parametrize("args,msg", [
    (["--move-noise", "0.1"], "go with --moves"),
    (["--move-noise-batch", "2"], "go with --moves"),
    (["--move-noise-rounds", "2"], "go with --moves"),
    (["--move-noise-count", "4"], "go with --moves"),
    (MOVES + ["--move-noise-batch", "2"], "go with --move-noise"),
    (MOVES + ["--move-noise-rounds", "2"], "go with --move-noise"),
    (MOVES + ["--move-noise-count", "4"], "go with --move-noise"),
    (NOISE + ["--move-refine", "2"], "--move-noise and --move-refine do not combine"),
    (MOVES + ["--move-noise=-0.5"], "--move-noise must be a finite number >= 0"),
    (MOVES + ["--move-noise", "nan"], "--move-noise must be a finite number >= 0"),
    (MOVES + ["--move-noise", "inf"], "--move-noise must be a finite number >= 0"),
    (MOVES + ["--move-noise", "0.1x"], "--move-noise must be a finite number >= 0"),
    (NOISE + ["--move-noise-batch", "0"], "--move-noise-batch must be at least 1"),
    (NOISE + ["--move-noise-batch=-2"], "--move-noise-batch must be at least 1"),
    (NOISE + ["--move-noise-rounds=-1"], "--move-noise-rounds must be at least 0"),
    (NOISE + ["--move-noise-batch", "65536", "--move-noise-rounds", "65536"], "is too large"),
    (NOISE + ["--move-noise-count", "0"], "--move-noise-count must be a finite number > 0"),
    (NOISE + ["--move-noise-count=-1"], "--move-noise-count must be a finite number > 0"),
    (NOISE + ["--move-noise-count", "nan"], "--move-noise-count must be a finite number > 0"),
    (NOISE + ["--move-noise-count", "inf"], "--move-noise-count must be a finite number > 0"),
    (NOISE + ["--move-noise-count", "4x"], "--move-noise-count must be a finite number > 0"),
])
def test_misuse_is_refused_before_anything_renders(args, msg):
    r = run(*args)
    assert r.returncode == 1 and msg in r.stderr, (r.stdout, r.stderr)
    assert "All samples have completed" not in r.stdout


def python_run(sid, spp, moves, shift, frames, noise_refine):
    """What rtrender --moves --move-noise does, through the Python binding -> (frame, info) per pose."""
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
    per = frames + noise_refine["batch_frames"] * noise_refine["max_rounds"]
    out = []
    for k in range(moves):
        v = cam[12:15] * F(shift * W)
        cam[4:7] += v
        cam[8:11] += v
        out.append(ctx.render_moved(cam, rtamd.frame_rand_factors(SEED, spp + k * per, per), noise_refine=noise_refine))
    ctx.close()
    return out


@pytest.mark.gpu
def test_each_move_line_and_png_is_the_pose_rendered_to_the_target(gpu, tmp_path):
    out = tmp_path / "out.png"
    r = run("-s", 6, "-r", f"{W}:{H}", "-spp", 8, "-md", 5, "-o", out, "--moves", 2, "--move-shift", 0.25, "--move-frames", 1,
            "--move-noise", 0.05, "--move-noise-batch", 2, "--move-noise-rounds", 3, "--move-noise-count", 3)
    assert r.returncode == 0, r.stderr
    poses = python_run(6, 8, 2, 0.25, 1, dict(target_noise=0.05, batch_frames=2, max_rounds=3, min_count=3.0))
    nt = ((W + 7) // 8) * ((H + 7) // 8)
    for k, (frame, info) in enumerate(poses, 1):
        png = read_png(tmp_path / f"out.move{k:02d}.png")
        assert np.array_equal(png, frame[..., :3]), k
        assert 0 < info["tiles_refined"] <= nt == 15 and 1 <= info["rounds_done"] <= 3   # the leading edge is always thin
        end = "converged" if info["converged"] else "round cap reached"
        line = (f"Move {k}/2: 1 frame(s), +{info['tile_frames_spent']} tile-frame(s) in {info['rounds_done']} round(s) on "
                f"{info['tiles_refined']} of {nt} tiles, noise {info['noise']:.6g} ({end}), saved to: ")
        assert line in r.stdout, (line, r.stdout)


@pytest.mark.gpu
def test_defaults_are_batch_1_rounds_4_count_automatic(gpu, tmp_path):
    out = tmp_path / "out.png"
    r = run("-s", 6, "-r", f"{W}:{H}", "-spp", 8, "-md", 5, "-o", out, "--moves", 1, "--move-shift", 0.25, "--move-frames", 2,
            "--move-noise", 0.02)
    assert r.returncode == 0, r.stderr
    (frame, info), = python_run(6, 8, 1, 0.25, 2, dict(target_noise=0.02, batch_frames=1, max_rounds=4))
    assert np.array_equal(read_png(tmp_path / "out.move01.png"), frame[..., :3])
    end = "converged" if info["converged"] else "round cap reached"
    assert (f"Move 1/1: 2 frame(s), +{info['tile_frames_spent']} tile-frame(s) in {info['rounds_done']} round(s) on "
            f"{info['tiles_refined']} of 15 tiles, noise {info['noise']:.6g} ({end}), saved to: ") in r.stdout, r.stdout

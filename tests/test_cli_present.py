"""rtrender --moves (raytracing-book_amd/host/rt_main.cpp): the options and their misuse on the CPU; on the
device, the <output stem>.moveNN.png files it writes against the same render_moved calls made from Python."""
import numpy as np
import pytest

import rtamd
from test_cli import read_png, run

W, H, SEED = 40, 24, 1
F = np.float32


def test_help_lists_the_move_options():
    r = run("--help")
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    for opt in ("--moves <arg>", "--move-shift <arg>", "--move-frames <arg>"):
        assert any(ln.split()[:len(opt.split())] == opt.split() and len(ln.split()) > 2 for ln in lines[1:]), opt


@pytest.mark.parametrize("args,msg", [
    (["--moves", "2"], "--moves needs --move-shift <S> and --move-frames <N>"),
    (["--moves", "2", "--move-shift", "0.25"], "--moves needs --move-shift <S> and --move-frames <N>"),
    (["--moves", "2", "--move-frames", "1"], "--moves needs --move-shift <S> and --move-frames <N>"),
    (["--move-shift", "0.25"], "go with --moves"),
    (["--move-frames", "1"], "go with --moves"),
    (["--moves", "0", "--move-shift", "0.25", "--move-frames", "1", "-o", "x.png"], "--moves must be at least 1"),
    (["--moves=-1", "--move-shift", "0.25", "--move-frames", "1", "-o", "x.png"], "--moves must be at least 1"),
    (["--moves", "2", "--move-shift", "0.25", "--move-frames", "0", "-o", "x.png"], "--move-frames must be at least 1"),
    (["--moves", "2", "--move-shift", "nan", "--move-frames", "1", "-o", "x.png"], "--move-shift must be a finite number"),
    (["--moves", "2", "--move-shift", "inf", "--move-frames", "1", "-o", "x.png"], "--move-shift must be a finite number"),
    (["--moves", "2", "--move-shift=-inf", "--move-frames", "1", "-o", "x.png"], "--move-shift must be a finite number"),
    (["--moves", "2", "--move-shift", "0.2x", "--move-frames", "1", "-o", "x.png"], "--move-shift must be a finite number"),
    (["--moves", "2", "--move-shift", "0.25", "--move-frames", "1", "-o", "x.png", "--devices", "0,0"],
     "--moves renders on one device"),
    (["--moves", "2", "--move-shift", "0.25", "--move-frames", "1"], "--moves needs -o"),
])
def test_misuse_is_refused_before_anything_renders(args, msg, tmp_path):
    r = run(*args)
    assert r.returncode == 1 and msg in r.stderr, (r.stdout, r.stderr)
    assert "All samples have completed" not in r.stdout


def python_run(sid, spp, moves, shift, frames):
    """What rtrender --moves does, through the Python binding -> the presented frame of every pose."""
    scene = rtamd.Scene(sid, W, H, seed=SEED)
    ctx = rtamd.RenderContext()
    ctx.upload_scene(scene)
    ctx.set_params(max_depth=5, spp=spp)
    ctx.resize(W, H)
    ctx.set_moments(True)
    ctx.set_history_variance(True)
    ctx.render_features()
    ctx.render(1, rtamd.frame_rand_factors(SEED, 0, spp))
    image = ctx.read_image()
    cam = np.array(scene.camera, F)
    out = []
    for k in range(moves):
        v = cam[12:15] * F(shift * W)
        cam[4:7] += v
        cam[8:11] += v
        out.append(ctx.render_moved(cam, rtamd.frame_rand_factors(SEED, spp + k * frames, frames)))
    ctx.close()
    return image, out


@pytest.mark.gpu
def test_each_move_png_is_the_presented_frame(gpu, tmp_path):
    out = tmp_path / "out.png"
    r = run("-s", 6, "-r", f"{W}:{H}", "-spp", 8, "-md", 5, "-o", out, "--moves", 2, "--move-shift", 0.25, "--move-frames", 1)
    assert r.returncode == 0, r.stderr
    image, frames = python_run(6, 8, 2, 0.25, 1)
    assert np.array_equal(read_png(out), rtamd.tonemap_rgb8(image))       # the normal output is as it was
    pngs = [read_png(tmp_path / f"out.move{k:02d}.png") for k in (1, 2)]
    for k, (png, frame) in enumerate(zip(pngs, frames), 1):
        assert (frame[..., 3] == 255).all()
        assert np.array_equal(png, frame[..., :3]), k
        assert f"Move {k}/2: 1 frame(s), saved to: " in r.stdout
    assert not np.array_equal(pngs[0], pngs[1])                            # the camera did move
    assert not (tmp_path / "out.move03.png").exists()

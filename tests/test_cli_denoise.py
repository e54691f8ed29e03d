"""rtrender --denoise (raytracing-book_amd/host/rt_main.cpp): the options and their misuse on the CPU;
on the device, the PNGs it writes against the same calls made from Python."""
import os

import numpy as np
import pytest

import rtamd
from helpers import oracle_image
from test_cli import read_png, run

W, H, SEED = 40, 24, 1


def test_help_lists_the_denoise_options():
    r = run("--help")
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    for opt in ("--denoise", "--denoise-levels <arg>", "--denoise-k <arg>", "--raw-output <arg>"):
        assert any(ln.split()[:len(opt.split())] == opt.split() and len(ln.split()) > 2 for ln in lines[1:]), opt


@pytest.mark.parametrize("args,msg", [
    (["--denoise-k", "2"], "go with --denoise"),
    (["--denoise-levels", "2"], "go with --denoise"),
    (["--raw-output", "x.png"], "go with --denoise"),
    (["--denoise", "--denoise-levels", "0"], "--denoise-levels must be 1..5"),
    (["--denoise", "--denoise-levels", "6"], "--denoise-levels must be 1..5"),
    (["--denoise", "--denoise-k", "0"], "--denoise-k must be a finite number > 0"),
    (["--denoise", "--denoise-k", "nan"], "--denoise-k must be a finite number > 0"),
    (["--denoise", "--denoise-k", "inf"], "--denoise-k must be a finite number > 0"),
    (["--denoise", "--denoise-k", "3x"], "--denoise-k must be a finite number > 0"),
    (["--denoise", "-spp", "1"], "--denoise needs -spp >= 2"),
    (["--denoise", "--devices", "0,0"], "--denoise renders on one device"),
])
def test_misuse_is_refused_before_anything_renders(args, msg):
    r = run(*args)
    assert r.returncode == 1 and msg in r.stderr, (r.stdout, r.stderr)


def python_run(sid, spp, levels=None, k=None, adaptive=None):
    ctx = rtamd.RenderContext()
    ctx.upload_scene(rtamd.Scene(sid, W, H, seed=SEED))
    ctx.set_params(max_depth=5, spp=spp)
    ctx.resize(W, H)
    ctx.set_moments(True)
    if adaptive:
        ctx.render_adaptive(adaptive, spp, 8, min_frames=8, seed=SEED)
    else:
        ctx.render(1, rtamd.frame_rand_factors(SEED, 0, spp))
    out = ctx.read_image(), ctx.denoise(levels=levels, k=k), ctx.read_tile_frames()
    ctx.close()
    return out


@pytest.mark.gpu
def test_output_is_the_filtered_image_and_raw_output_the_rendered_one(gpu, tmp_path):
    out, raw = tmp_path / "out.png", tmp_path / "raw.png"
    r = run("-s", 6, "-r", f"{W}:{H}", "-spp", 8, "-md", 5, "-o", out, "--denoise", "--raw-output", raw,
            "--frames-per-launch", 3)
    assert r.returncode == 0, r.stderr
    assert "Denoise: levels 3, k 3" in r.stdout
    assert f"The unfiltered image has been saved to: {os.path.realpath(raw)}" in r.stdout
    img, den, _ = python_run(6, 8)
    assert np.array_equal(read_png(raw), rtamd.tonemap_rgb8(img))
    assert np.array_equal(read_png(out), rtamd.tonemap_rgb8(den))
    assert not np.array_equal(read_png(out), read_png(raw))
    # the image's bits do not change with the moments on
    assert np.array_equal(read_png(raw), rtamd.tonemap_rgb8(oracle_image(rtamd.Scene(6, W, H, seed=SEED), 8, spp=8)))
    # the parameters reach the filter
    r = run("-s", 6, "-r", f"{W}:{H}", "-spp", 8, "-md", 5, "-o", out, "--denoise", "--denoise-levels", 5,
            "--denoise-k", 1.5)
    assert r.returncode == 0 and "Denoise: levels 5, k 1.5" in r.stdout, r.stderr
    assert np.array_equal(read_png(out), rtamd.tonemap_rgb8(python_run(6, 8, levels=5, k=1.5)[1]))


@pytest.mark.gpu
def test_preview_updates_are_filtered_once_two_frames_exist(gpu, tmp_path):
    prev, out = tmp_path / "prev.png", tmp_path / "out.png"
    r = run("-s", 6, "-r", f"{W}:{H}", "-spp", 2, "-md", 5, "--denoise", "--preview", prev, "--preview-every", 1)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("Sample: ") == 2    # frame 1 as rendered (no variance yet), frame 2 filtered
    assert np.array_equal(read_png(prev), rtamd.tonemap_rgb8(python_run(6, 2)[1]))
    r = run("-s", 6, "-r", f"{W}:{H}", "-spp", 8, "-md", 5, "--denoise", "--preview", prev, "--preview-every", 3, "-o", out)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(read_png(prev), read_png(out))
    assert np.array_equal(read_png(out), rtamd.tonemap_rgb8(python_run(6, 8)[1]))


@pytest.mark.gpu
def test_with_the_noise_target_and_the_adaptive_loop(gpu, tmp_path):
    out = tmp_path / "out.png"
    target = 0.05
    img, den, counts = python_run(0, 32, adaptive=target)
    r = run("-s", 0, "-r", f"{W}:{H}", "-spp", 32, "-md", 5, "--frames-per-launch", 8, "--noise", target, "--adaptive",
            "--min-frames", 8, "--denoise", "-o", out)
    assert r.returncode == 0, r.stderr
    assert "Adaptive: " in r.stdout
    assert np.array_equal(read_png(out), rtamd.tonemap_rgb8(den))
    r = run("-s", 0, "-r", f"{W}:{H}", "-spp", 16, "-md", 5, "--frames-per-launch", 8, "--noise", 1e-6, "--denoise", "-o", out)
    assert r.returncode == 0 and "Noise target: 16 frames" in r.stdout, r.stderr
    assert np.array_equal(read_png(out), rtamd.tonemap_rgb8(python_run(0, 16)[1]))

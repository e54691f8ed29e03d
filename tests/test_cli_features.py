"""rtrender --denoise-guides and --features-output (raytracing-book_amd/host/rt_main.cpp): the options
and their misuse on the CPU; on the device, one run whose PNGs are checked against the same calls made
from Python."""
import os

import numpy as np
import pytest

import rtamd
from test_cli import read_png, run

W, H, SEED = 32, 32, 1


def test_help_lists_the_feature_options():
    r = run("--help")
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    for opt in ("--denoise-guides", "--denoise-kn <arg>", "--denoise-kz <arg>", "--denoise-ka <arg>",
                "--features-output <arg>"):
        assert any(ln.split()[:len(opt.split())] == opt.split() and len(ln.split()) > 2 for ln in lines[1:]), opt


@pytest.mark.parametrize("args,msg", [
    (["--denoise-guides"], "--denoise-guides goes with --denoise"),
    (["--denoise", "--denoise-kn", "1"], "go with --denoise-guides"),
    (["--denoise", "--denoise-kz", "1"], "go with --denoise-guides"),
    (["--denoise-ka", "1"], "go with --denoise-guides"),
    (["--denoise", "--denoise-guides", "--denoise-kn=-1"], "--denoise-kn must be a finite number >= 0"),
    (["--denoise", "--denoise-guides", "--denoise-kz", "nan"], "--denoise-kz must be a finite number >= 0"),
    (["--denoise", "--denoise-guides", "--denoise-ka", "inf"], "--denoise-ka must be a finite number >= 0"),
    (["--denoise", "--denoise-guides", "--denoise-ka", "2x"], "--denoise-ka must be a finite number >= 0"),
    (["--features-output", "x", "--devices", "0,0"], "--features-output renders on one device"),
])
def test_misuse_is_refused_before_anything_renders(args, msg):
    r = run(*args)
    assert r.returncode == 1 and msg in r.stderr, (r.stdout, r.stderr)


@pytest.mark.gpu
def test_feature_images_and_guided_output(gpu, tmp_path):
    out, prefix = tmp_path / "out.png", tmp_path / "ft"
    r = run("-s", 6, "-r", f"{W}:{H}", "-spp", 8, "-md", 5, "-o", out, "--denoise", "--denoise-guides",
            "--denoise-ka", 2, "--features-output", prefix)
    assert r.returncode == 0, r.stderr
    assert "Denoise guides: kn 0.5, kz 1, ka 2" in r.stdout
    ctx = rtamd.RenderContext()
    ctx.upload_scene(rtamd.Scene(6, W, H, seed=SEED))
    ctx.set_params(max_depth=5, spp=8)
    ctx.resize(W, H)
    ctx.set_moments(True)
    ctx.render_features()
    ctx.render(1, rtamd.frame_rand_factors(SEED, 0, 8))
    den = ctx.denoise(guides=(0.5, 1.0, 2.0))
    nd, alb, ids = ctx.read_features()
    ctx.close()
    assert np.array_equal(read_png(out), rtamd.tonemap_rgb8(den))
    normal, albedo, depth = (read_png(f"{prefix}_{n}.png") for n in ("normal", "albedo", "depth"))
    for img, name in ((normal, "normal"), (albedo, "albedo"), (depth, "depth")):
        assert img.shape == (H, W, 3), name
        assert f"A first-hit feature image has been saved to: {os.path.realpath(f'{prefix}_{name}.png')}" in r.stdout
    assert np.array_equal(normal, np.clip(np.floor((nd[..., :3] * np.float32(0.5) + np.float32(0.5)) * np.float32(255.0)
                                                   + np.float32(0.5)), 0, 255).astype(np.uint8))
    a4 = np.concatenate([alb, np.ones((H, W, 1), np.float32)], -1)
    assert np.array_equal(albedo, rtamd.tonemap_rgb8(a4))
    hit = ids != 0xFFFFFFFF
    assert hit.any() and (depth[~hit] == 0).all() and depth.max() == 255
    assert (depth[..., 0] == depth[..., 1]).all() and (depth[..., 1] == depth[..., 2]).all()

"""rt_present_host (rt.h; csrc/rt_present_math.h over host/rt_gamma_lut.h's table) on the CPU: against the
NumPy float32 restatement bit for bit, against rts_tonemap_rgb8 byte for byte on an input that rounds half
to even in both directions, the RT_PRESENT_MOVED rule on a synthetic case, and the argument checks.
"""
import ctypes

import numpy as np
import pytest

import rtamd
from rtamd import _lib
from helpers import bit_equal, mismatch_report
import present_ref as P

F = np.float32


def test_the_table_is_a_monotone_256_entry_table():
    lut = P.table()
    assert lut.shape == (256,) and lut.dtype == np.uint8
    assert lut[0] == 0 and lut[255] == 255
    assert (np.diff(lut.astype(np.int32)) >= 0).all()          # monotone: no two entries change places
    assert len(set(lut.tolist())) > 128                        # and not a constant run
    # it is Texture.saveAsPNG's: (byte)((float)pow(b / 255, 1 / 2.2) * 255f), truncated
    exp = ((np.arange(256) / 255.0) ** (1.0 / 2.2)).astype(F) * F(255)
    assert np.array_equal(lut, exp.astype(np.int32).astype(np.uint8))


def buffers(w, h, seed):
    """Three float buffers with values below 0, above 1 and not finite among them, and tile counts."""
    rng = np.random.default_rng(seed)
    out = {}
    for name in ("image", "denoised", "reprojected"):
        a = rng.random((h, w, 4)).astype(F) * F(1.5) - F(0.25)
        a[rng.integers(0, h), rng.integers(0, w), rng.integers(0, 3)] = np.nan
        a[rng.integers(0, h), rng.integers(0, w), rng.integers(0, 3)] = np.inf
        a[rng.integers(0, h), rng.integers(0, w), rng.integers(0, 3)] = -np.inf
        out[name] = a
    nt = ((w + 7) // 8) * ((h + 7) // 8)
    out["tile_frames"] = rng.integers(0, 4, nt).astype(np.int32)
    out["reprojected"][..., 3] = rng.integers(0, 6, (h, w)).astype(F)
    out["reprojected"][0, 0, 3] = np.nan
    return out


@pytest.mark.parametrize("source", P.SOURCES)
@pytest.mark.parametrize("exposure", P.EXPOSURES)
@pytest.mark.parametrize("size", [(13, 9), (70, 11), (32, 32)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_matches_the_restatement(source, exposure, size):
    b = buffers(*size, seed=3)
    ref8, reff = P.present(source, exposure=exposure, **b)
    got8, gotf = rtamd.present_host(source, exposure=exposure, keep_float=True, **b)
    assert np.array_equal(got8, ref8), np.argwhere(got8 != ref8)[:4]
    assert bit_equal(gotf, reff), mismatch_report(gotf, reff)
    assert (got8[..., 3] == 255).all()
    # without the float copy the bytes are the same; buffers the source does not read may be absent
    need = dict(image=("image",), denoised=("denoised",), reprojected=("reprojected",),
                moved=("reprojected", "denoised", "tile_frames"))[source]
    assert np.array_equal(rtamd.present_host(source, exposure=exposure, **{k: b[k] for k in need}), ref8)
    if exposure == 1.0:   # the factor 1 keeps every finite value's bits
        src = b["image" if source == "image" else "denoised" if source == "denoised" else "reprojected"]
        if source != "moved":
            assert bit_equal(gotf[..., :3], src[..., :3])


def test_rounding_input_rounds_half_to_even_in_both_directions():
    trip, special = P.rounding_values()
    ties = P.rounding_ties(trip)
    assert ties.any(axis=1).all()                                  # every k has a value that lands on k + 0.5
    k = np.arange(255)
    assert int((k % 2 == 0).sum()) == 128 and int((k % 2 == 1).sum()) == 127
    tie_vals = trip[ties]
    tie_k = np.broadcast_to(k[:, None], ties.shape)[ties]
    got = P.code(tie_vals)
    assert (got[tie_k % 2 == 0] == tie_k[tie_k % 2 == 0]).all()    # even k: the tie rounds down to k
    assert (got[tie_k % 2 == 1] == tie_k[tie_k % 2 == 1] + 1).all()  # odd k: up to k + 1
    img = P.rounding_image()
    assert img.shape == (11, 70, 4) and img[..., :3].size == 2310
    flat = img[..., :3].ravel()
    assert bit_equal(flat[:765], trip.ravel()) and bit_equal(flat[765:772], special)


def test_image_at_exposure_1_is_rts_tonemap_rgb8():
    img = P.rounding_image()
    ref = rtamd.tonemap_rgb8(img)
    got, flt = rtamd.present_host("image", image=img, keep_float=True)
    assert np.array_equal(got[..., :3], ref), np.argwhere(got[..., :3] != ref)[:4]
    assert (got[..., 3] == 255).all()
    assert bit_equal(flt[..., :3], img[..., :3]) and (flt[..., 3] == 1).all()
    assert np.array_equal(P.present("image", image=img)[0], got)
    # the same through the other single-buffer sources
    assert np.array_equal(rtamd.present_host("denoised", denoised=img), got)
    assert np.array_equal(rtamd.present_host("reprojected", reprojected=img), got)


def test_moved_rule():
    c = P.moved_case()
    R, D, tf, kind = c["reprojected"], c["denoised"], c["tile_frames"], c["kind"]
    assert R.shape == (9, 13, 4) and tf.size == 4                   # partial tiles in both directions
    n_t = P.tile_counts_per_pixel(tf, 13, 9).astype(F)
    below, equal, above, nan = R[..., 3] < n_t, R[..., 3] == n_t, R[..., 3] > n_t, np.isnan(R[..., 3])
    assert below.any() and equal.any() and above.any() and nan.any()
    assert (below | equal | above | nan).all()
    for x0, y0 in ((0, 0), (8, 0), (0, 8), (8, 8)):                  # ... in every tile
        t = (slice(y0, y0 + 8), slice(x0, x0 + 8))
        assert below[t].any() and equal[t].any() and above[t].any() and nan[t].any()
    for exposure in P.EXPOSURES:
        got8, gotf = rtamd.present_host("moved", exposure=exposure, keep_float=True, reprojected=R, denoised=D, tile_frames=tf)
        ref8, reff = P.present("moved", exposure=exposure, reprojected=R, denoised=D, tile_frames=tf)
        assert np.array_equal(got8, ref8) and bit_equal(gotf, reff), mismatch_report(gotf, reff)
    got8, gotf = rtamd.present_host("moved", keep_float=True, reprojected=R, denoised=D, tile_frames=tf)
    fresh = gotf[..., 3] == 1
    assert np.array_equal(fresh, ~above) and np.array_equal(gotf[..., 3] == 0, above)
    assert bit_equal(gotf[fresh][:, :3], D[fresh][:, :3]) and bit_equal(gotf[~fresh][:, :3], R[~fresh][:, :3])
    # the bytes are the composed buffer's
    comp = np.where(fresh[..., None], D, R)
    assert np.array_equal(got8[..., :3], rtamd.tonemap_rgb8(comp))
    # a scalar count stands for every tile
    assert np.array_equal(rtamd.present_host("moved", reprojected=R, denoised=D, tile_frames=2),
                          rtamd.present_host("moved", reprojected=R, denoised=D, tile_frames=[2] * 4))


def raw_call(source=0, exposure=1.0, keep_float=0, reserved=None, w=13, h=9, image=True, denoised=True, reprojected=True,
             tile_frames=True, n_tiles=None, out=True, flt=True, counts=None, null_params=False):
    """rt_present_host called directly -> its status."""
    L = rtamd.amd()
    p = _lib.RtPresentParams()
    p.source, p.exposure, p.keep_float = source, exposure, keep_float
    for i, v in enumerate(reserved or ()):
        p.reserved[i] = v
    n = max(1, w * h)
    buf = np.full((n, 4), 0.5, F)
    nt = ((w + 7) // 8) * ((h + 7) // 8)
    tf = np.asarray(counts if counts is not None else [2] * max(1, nt), np.int32)
    o8, of = np.zeros((n, 4), np.uint8), np.zeros((n, 4), F)
    fp = lambda on: buf.ctypes.data_as(_lib.c_float_p) if on else None  # noqa: E731
    return L.rt_present_host(fp(image), fp(denoised), fp(reprojected),
                             tf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if tile_frames else None,
                             nt if n_tiles is None else n_tiles, w, h, None if null_params else ctypes.byref(p),
                             o8.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if out else None,
                             of.ctypes.data_as(_lib.c_float_p) if flt else None)


def test_good_calls_and_null_params():
    assert raw_call() == 0
    assert raw_call(null_params=True, denoised=False, reprojected=False, tile_frames=False, flt=False) == 0
    for s in range(4):
        assert raw_call(source=s, keep_float=1) == 0
    # NULL params: the image at exposure 1
    img = P.rounding_image()
    out = np.zeros((11, 70, 4), np.uint8)
    rc = rtamd.amd().rt_present_host(img.ctypes.data_as(_lib.c_float_p), None, None, None, 0, 70, 11, None,
                                     out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), None)
    assert rc == 0 and np.array_equal(out[..., :3], rtamd.tonemap_rgb8(img))


@pytest.mark.parametrize("bad", [
    dict(source=4), dict(source=-1), dict(source=1 << 20),
    dict(exposure=0.0), dict(exposure=-1.0), dict(exposure=float("nan")), dict(exposure=float("inf")),
    dict(exposure=-0.0),
    dict(reserved=[1]), dict(reserved=[0, 0, 0, 0, 7]),
    dict(out=False),
    dict(keep_float=1, flt=False),
    dict(source=0, image=False), dict(source=1, denoised=False), dict(source=2, reprojected=False),
    dict(source=3, reprojected=False), dict(source=3, denoised=False), dict(source=3, tile_frames=False),
    dict(source=3, n_tiles=3), dict(source=3, counts=[2, 2, -1, 2]),
    dict(w=0), dict(h=0), dict(w=-3), dict(w=65537, h=1),
], ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_bad_arguments_are_refused(bad):
    assert raw_call(**bad) == -1   # RT_ERR_INVALID_ARG


def test_recorded_quality_and_resources():
    """profiles/present_quality.json (tools/present_quality.py, CPU) holds the composite's figures, and
    profiles/present_resources.txt the compiler's report: no kernel of rt_present.hip uses scratch."""
    import json
    import os
    import re
    prof = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
    rec = json.load(open(os.path.join(prof, "present_quality.json")))
    assert (rec["scene"], rec["width"], rec["height"], rec["frames_a"], rec["shift"]) == (6, 32, 32, 64, 0.25)
    for fb, fresh, whole, filtered in ((1, 0.4591, 0.9995, 1.0723), (2, 0.3178, 0.9974, 1.0653)):
        r = rec["runs"][f"frames_b={fb}"]
        assert (r["fresh_pixels"], r["other_pixels"]) == (64, 960)
        assert r["composite_over_reprojected"] == dict(whole=whole, fresh=fresh)
        assert r["filtered_over_reprojected"] == dict(whole=filtered, fresh=fresh)
        assert r["composite_is_reprojected_elsewhere"] and r["composite_is_filtered_on_fresh"]
        assert r["bytes_are_tonemap_of_composite"]
    text = open(os.path.join(prof, "present_resources.txt")).read()
    release = text.split("## flags: -DRT_AB_KNOBS")[0]
    assert len(re.findall(r"Function Name: \S*present_kernel", release)) == 8      # <source, keep_float>
    assert len(re.findall(r"Function Name: \S*present_kernel", text)) == 24
    assert set(re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)) == {"0"}
    assert set(re.findall(r"VGPRs Spill: (\d+)", text)) == {"0"} and set(re.findall(r"SGPRs Spill: (\d+)", text)) == {"0"}
    assert set(re.findall(r"LDS Size \[bytes/block\]: (\d+)", release)) == {"0"}


def test_python_wrapper_raises_on_a_bad_parameter():
    img = P.rounding_image()
    for kw in (dict(source=7), dict(exposure=0.0), dict(exposure=float("nan"))):
        with pytest.raises(rtamd.RTError) as e:
            rtamd.present_host(**dict(dict(source="image", image=img), **kw))
        assert e.value.code == -1

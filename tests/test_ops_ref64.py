"""The CPU oracle's per-operation entry points against the float64 reference (tests/ref64.py), op by op
(no GPU): the oracle is a restatement of the reference's GLSL and the kernel a second one made to agree
with it, so a mistake they share passes every parity test; ref64 is written from the shader text alone.

Per op, over the batches of tests/ops_cases.py:
  * classification (hit / miss, box face, checker parity) must agree on every row float64 decides (its
    decision margin exceeds the rounding bound); at most 10 % of a random set may be undecided, and an
    edge set has no undecided row within float64's scope;
  * values (t, t1, t2, alpha, beta, u, v, turbulence, rgb) must lie within ref64's derived rounding
    bound: the worst |error| / bound per op is printed, must not exceed 1, and must reach 1/100 (a
    looser bound would not catch a few-ulp mistake).  profiles/ops_ref64.json records the ratios
    (`python tests/test_ops_ref64.py` rewrites it).
"""
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    _repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_repo, os.path.join(_repo, "oracle"), os.path.join(_repo, "raytracing-book_amd")]

import ops_cases
import pyoracle
import ref64

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(REPO, "profiles", "ops_ref64.json")


def _ratio(got, ref, mask):
    """|got - ref| / bound over mask; a zero bound demands equality (0, or inf when it differs)."""
    got = np.asarray(got, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        err, b = np.abs(got - ref.v), ref.bound()
        r = np.where(b == 0.0, np.where(err == 0.0, 0.0, np.inf), err / b)
    r = np.where(np.isnan(r), np.inf, r)
    return np.where(mask, r, 0.0)


def evaluate(batch):
    """(agree [n] bool: the classification matches, decided [n], scope [n], {value name: ratio [n]})."""
    op, rows, recs = batch.op, batch.rows, batch.recs
    if op == "sphere":
        R = ref64.hit_sphere(recs, rows)
        hit, t = pyoracle.hit_spheres(recs, rows)
        both = hit & R["hit"]
        return hit == R["hit"], R["path"], {"t": _ratio(t, R["t"], both)}
    if op == "medium_sphere":
        R = ref64.medium_boundary_hits(recs, rows)
        ok, t1, t2 = pyoracle.medium_boundary_hits(recs, rows)
        both = ok & R["ok"]
        return ok == R["ok"], R["path"], {"t1": _ratio(t1, R["t1"], both), "t2": _ratio(t2, R["t2"], both)}
    if op == "quad":
        R = ref64.hit_quad(recs, rows)
        hit, t, al, be = pyoracle.hit_quads(recs, rows)
        both = hit & R["hit"]
        return hit == R["hit"], R["path"], {"t": _ratio(t, R["t"], both), "alpha": _ratio(al, R["alpha"], both),
                                              "beta": _ratio(be, R["beta"], both)}
    if op == "box":
        R = ref64.hit_box(recs, rows)
        hit, t, face, al, be = pyoracle.hit_boxes(recs, rows)
        both = hit & R["hit"]
        agree = (hit == R["hit"]) & (~both | (face == R["face"]))
        same = both & (face == R["face"])
        return agree, R["path"], {"t": _ratio(t, R["t"], same), "alpha": _ratio(al, R["alpha"], same),
                                  "beta": _ratio(be, R["beta"], same)}
    if op == "node":
        R = ref64.hit_aabb(recs, rows)
        return pyoracle.hit_aabbs(recs, rows) == R["hit"], R["path"], {}
    if op == "perlin":
        R = ref64.perlin_turb(batch.tex[3], rows[:, 0:3])
        got = pyoracle.perlin_turbs(batch.tex[3], rows[:, 0:3])
        return np.ones(len(rows), bool), R["path"], {"turbulence": _ratio(got, R["turb"], R["path"].scope)}
    if op == "sphere_uv":
        R = ref64.sphere_uv(rows[:, 0:3])
        u, v = pyoracle.sphere_uvs(rows[:, 0:3])
        return np.ones(len(rows), bool), R["path"], {"u": _ratio(u, R["u"], R["u_scope"]), "v": _ratio(v, R["v"], R["path"].scope)}
    if op == "texture" and (rows.view(np.int32)[0, 9] >> 28) == pyoracle.TEXTYPE_IMAGE:
        fmt, w, h, texels = batch.tex
        R = ref64.texture_bilinear(fmt, w, h, texels, rows[:, 3:5])
        got = pyoracle.texture_bilinears(fmt, w, h, texels, rows[:, 3:5])
        return np.ones(len(rows), bool), R["path"], {"rgb"[c]: _ratio(got[:, c], R["rgb"][c], R["path"].scope) for c in range(3)}
    if op == "texture":
        R = ref64.checker_parity(ops_cases.checker_scale_of(batch), rows[:, 0:3])
        which = rows.view(np.int32)[:, 9] & 0xFFF
        odd = pyoracle.checker_parities(ops_cases.CHECKER_SCALES, rows[:, 0:3], which)
        return odd == R["odd"], R["path"], {}
    raise ValueError(op)


def run_op(name):
    """Every batch of op `name`: asserts the classification rules, returns (worst ratio per value,
    undecided share of the random sets)."""
    worst, n_random, n_undecided = {}, 0, 0
    for b in ops_cases.ALL[name]():
        agree, path, ratios = evaluate(b)
        decided, scope = path.decided, path.scope
        bad = decided & ~agree
        assert not bad.any(), f"{b!r}: oracle and float64 disagree on decided rows {np.nonzero(bad)[0][:8]}"
        if b.kind == "random":
            n_random += len(decided)
            n_undecided += int((~decided).sum())
        if b.kind == "edge":
            und = scope & ~decided
            assert scope.any(), f"{b!r}: no row of the edge set is in float64's scope"
            assert not und.any(), f"{b!r}: edge rows {np.nonzero(und)[0][:8]} are undecided (margins {path.margin[und][:8]})"
        for k, r in ratios.items():
            r = np.where(decided, r, 0.0)
            over = r > 1.0
            assert not over.any(), f"{b!r}: {k} off by {r[over][:4]} x its rounding bound at rows {np.nonzero(over)[0][:4]}"
            worst[k] = max(worst.get(k, 0.0), float(r.max()))
    share = n_undecided / max(n_random, 1)
    return worst, share


@pytest.mark.parametrize("name", list(ops_cases.ALL))
def test_oracle_against_float64(name):
    worst, share = run_op(name)
    print(f"{name}: undecided share of the random sets {share:.4f}; worst error / bound "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert share <= 0.10, f"{name}: {share:.3f} of the random rows are undecided"
    for k, v in worst.items():
        assert v <= 1.0, (name, k, v)
        assert v >= 0.01, f"{name}.{k}: worst error / bound {v:.4f} < 1/100: the bound is too loose"


def test_single_row_exports_agree_with_the_batch_entry():
    """oracle_hit_box, oracle_medium_boundary_hits, oracle_texture_bilinear and oracle_checker_parity, one row
    at a time, give oracle_eval_op's words (which the tests above pin to float64)."""
    import ctypes
    L = pyoracle.lib()
    fp = ctypes.POINTER(ctypes.c_float)
    f3 = lambda a: np.ascontiguousarray(a, np.float32).ctypes.data_as(fp)   # noqa: E731
    b = [x for x in ops_cases.box_batches() if x.name == "edges"][0]
    hit, t, face, al, be = pyoracle.hit_boxes(b.recs, b.rows)
    for i in range(len(b.rows)):
        tt, ff, uv = ctypes.c_float(), ctypes.c_int(), np.zeros(2, np.float32)
        o, d = b.rows[i, 0:3].copy(), b.rows[i, 3:6].copy()
        rec = np.ascontiguousarray(b.recs[i])
        got = L.oracle_hit_box(rec.ctypes.data, f3(o), f3(d), float(b.rows[i, 6]), float(b.rows[i, 7]), ctypes.byref(tt), ctypes.byref(ff), f3(uv))
        assert got == int(hit[i])
        if got:
            assert (tt.value, ff.value, uv[0], uv[1]) == (t[i], face[i], al[i], be[i])
    m = [x for x in ops_cases.medium_sphere_batches() if x.name == "edges"][0]
    ok, t1, t2 = pyoracle.medium_boundary_hits(m.recs, m.rows)
    assert ok.tolist() == [False, True, False, True, True, True, False] and (t1[1], t2[1]) == (3.0, 5.0)
    for i in range(len(m.rows)):
        a, c = ctypes.c_float(), ctypes.c_float()
        o, d = m.rows[i, 0:3].copy(), m.rows[i, 3:6].copy()
        rec = np.ascontiguousarray(m.recs[i])
        got = L.oracle_medium_boundary_hits(rec.ctypes.data, float(m.rows[i, 8]), f3(o), f3(d), ctypes.byref(a), ctypes.byref(c))
        assert got == int(ok[i]) and (not got or (a.value, c.value) == (t1[i], t2[i]))
    x = [x for x in ops_cases.texel_batches() if x.name == "rgba_3x2_edges"][0]
    fmt, w, h, texels = x.tex
    want = pyoracle.texture_bilinears(fmt, w, h, texels, x.rows[:, 3:5])
    tb = np.ascontiguousarray(texels)
    for i in range(len(x.rows)):
        rgb = np.zeros(3, np.float32)
        L.oracle_texture_bilinear(fmt, w, h, tb.ctypes.data, float(x.rows[i, 3]), float(x.rows[i, 4]), f3(rgb))
        assert np.array_equal(rgb, want[i])
    c = [x for x in ops_cases.checker_batches() if x.name == "edges"][0]
    which = c.rows.view(np.int32)[:, 9] & 0xFFF
    odd = pyoracle.checker_parities(ops_cases.CHECKER_SCALES, c.rows[:, 0:3], which)
    for i in range(len(c.rows)):
        assert L.oracle_checker_parity(float(ops_cases.CHECKER_SCALES[which[i]]), *(float(v) for v in c.rows[i, 0:3])) == int(odd[i])
    assert odd.any() and not odd.all()


@pytest.mark.parametrize("name", ["quad", "box"])
def test_one_lane_per_wave_has_a_tiny_numerator(name):
    """The one_lane_out batches are what they claim: in every wave lane 17's alpha numerator is non-zero and
    below 2^-100, the other lanes' numerators are at least 0.5, and the hook reports the fd regime."""
    from rtamd._lib import debug_eval_op
    b = [x for x in ops_cases.ALL[name]() if x.name == "one_lane_out"][0]
    out = ops_cases.lanes_out_of_regime(b).reshape(-1, 64)
    assert (out.sum(axis=1) == 1).all() and out[:, 17].all()
    assert (pyoracle.eval_op(b.op, b.rows, b.recs)[:, 0] == 1).all()   # and every row hits
    _, flags = debug_eval_op(pyoracle.OPS[b.op], 0, b.rows, b.recs, device=-1)
    assert flags[0] == 1 and (name == "quad" or flags[1] == len(b.rows))


def test_recorded_ratios_cover_every_op():
    rec = json.load(open(PROFILE))
    assert set(rec["ops"]) == set(ops_cases.ALL)
    for name, r in rec["ops"].items():
        assert r["undecided_share"] <= 0.10
        for k, v in r["worst_error_over_bound"].items():
            assert 0.01 <= v <= 1.0, (name, k, v)


if __name__ == "__main__":
    out = {"what": "tests/test_ops_ref64.py: the CPU oracle's worst |error| / derived rounding bound per value, and the "
                   "share of the random rows float64 cannot decide (u = 2^-24; tests/ref64.py derives the bounds)",
           "ops": {}}
    for name in ops_cases.ALL:
        worst, share = run_op(name)
        out["ops"][name] = {"undecided_share": round(share, 5),
                            "worst_error_over_bound": {k: round(v, 4) for k, v in worst.items()}}
        print(name, out["ops"][name])
    with open(PROFILE, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")

"""The CPU oracle's sampling, light, camera and shading entry points (oracle_eval_shade_op) against the
float64 reference written from the shader text (tests/ref64_shade.py), op by op, no GPU, by the rules of
tests/test_ops_ref64.py:
  * oracle and float64 classify every decided row alike -- hit / miss, path ended or not, and the number
    of draws: "rf after" must be rf advanced by exactly that many float32 additions of 0.001;
  * every value lies within its derived rounding bound; the worst |error| / bound per value is at most 1
    and at least 1/100;
  * at most 10 % of a random set is undecided, and no in-scope row of an edge set is.
rand itself is pinned as a float32 composition (ref64_shade.rand32) with the oracle's own sine.
profiles/shade_ref64.json records the ratios (`python tests/test_shade_ref64.py` rewrites it).
"""
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    _repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_repo, os.path.join(_repo, "oracle"), os.path.join(_repo, "raytracing-book_amd"),
                    os.path.join(_repo, "tests")]

import pyoracle
import ref64_shade as R
import shade_cases
from test_ops_ref64 import _ratio

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(REPO, "profiles", "shade_ref64.json")
OPS = ["onb", "unit_vec", "medium_tail", "light_pdf", "light_dir", "camera_ray", "shade"]   # rand: its own test
_oscenes = {}


def oracle_scene(name):
    if name not in _oscenes:
        sc, uni = shade_cases.scene(name)
        _oscenes[name] = (pyoracle.OracleScene(sc, uniforms=uni), R.RefScene(sc, *uni))
    return _oscenes[name]


def _f(w):
    return np.ascontiguousarray(w).view(np.float32)


def evaluate(b):
    """(reference result, oracle classification dict, oracle values dict, oracle rf after or None)."""
    osc, S = oracle_scene(b.scene)
    w = pyoracle.eval_shade_op(osc, b.op, b.rows)
    r = b.rows
    seq = shade_cases.draws(r)
    if b.op == "onb":
        return R.onb(r[:, 0:3], r[:, 3:6]), {}, dict(zip("xyz", (_f(w[:, k]) for k in range(3)))), None
    if b.op == "unit_vec":
        return R.unit_vec(seq), {}, dict(zip("xyz", (_f(w[:, k]) for k in range(3)))), _f(w[:, 3])
    if b.op == "medium_tail":
        ref = R.medium_tail(r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4], r[:, 5], seq)
        return ref, dict(hit=w[:, 0] != 0), dict(t=_f(w[:, 1])), _f(w[:, 2])
    if b.op == "light_pdf":
        return R.light_pdf(S, r[:, 0:3], r[:, 3:6], r[:, 8]), {}, dict(pdf=_f(w[:, 0])), None
    if b.op == "light_dir":
        return R.light_dir(S, r[:, 0:3], seq), {}, dict(zip("xyz", (_f(w[:, k]) for k in range(3)))), _f(w[:, 3])
    if b.op == "camera_ray":
        ref = R.camera_ray(S, r[:, 9], r[:, 10], r.view(np.int32)[:, 19], seq)
        names = ("ox", "oy", "oz", "dx", "dy", "dz")
        return ref, dict(time=_f(w[:, 0])), dict(zip(names, (_f(w[:, k]) for k in range(1, 7)))), _f(w[:, 7])
    if b.op == "shade":
        ref = R.shade(S, r, seq)
        vals = dict(zip(("r", "g", "b"), (_f(w[:, k]) for k in (1, 2, 3))))
        vals.update(zip(("ox", "oy", "oz", "dx", "dy", "dz", "ar", "ag", "ab"), (_f(w[:, k]) for k in range(1, 10))))
        return ref, dict(ended=w[:, 0] != 0), vals, _f(w[:, 10])
    raise ValueError(b.op)


def run_op(name):
    worst, n_random, n_undecided = {}, 0, 0
    for b in shade_cases.batches(name):
        if b.kind == "device":   # rows float64 cannot decide by construction: device against oracle only
            continue
        ref, cls, vals, rf_after = evaluate(b)
        path = ref["path"]
        decided, scope = path.decided, path.scope
        agree = np.ones(len(b.rows), bool)
        for k, v in cls.items():
            agree &= v == ref["cls"][k]
        if rf_after is not None:   # the draw count: rf advanced by that many float32 additions of 0.001
            agree &= rf_after == R.advance_rf(b.rows[:, pyoracle.SOP_RF], ref["cls"]["count"])
        bad = decided & ~agree
        assert not bad.any(), f"{b!r}: oracle and float64 disagree on decided rows {np.nonzero(bad)[0][:8]}"
        if b.kind == "random":
            n_random += len(decided)
            n_undecided += int((~decided).sum())
        else:
            und = scope & ~decided
            assert scope.any(), f"{b!r}: no row of the edge set is in float64's scope"
            assert not und.any(), f"{b!r}: edge rows {np.nonzero(und)[0][:8]} are undecided (margins {path.margin[und][:8]})"
        for k, e in ref["val"].items():
            r = np.where(decided & ref["mask"][k], _ratio(vals[k], e, decided & ref["mask"][k]), 0.0)
            over = r > 1.0
            assert not over.any(), f"{b!r}: {k} off by {r[over][:4]} x its rounding bound at rows {np.nonzero(over)[0][:4]}"
            worst[k] = max(worst.get(k, 0.0), float(r.max()))
    return worst, n_undecided / max(n_random, 1)


@pytest.mark.parametrize("name", OPS)
def test_oracle_against_float64(name):
    worst, share = run_op(name)
    print(f"{name}: undecided share of the random sets {share:.4f}; worst error / bound "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert share <= 0.10, f"{name}: {share:.3f} of the random rows are undecided"
    for k, v in worst.items():
        assert v <= 1.0, (name, k, v)
        assert v >= 0.01, f"{name}.{k}: worst error / bound {v:.4f} < 1/100: the bound is too loose"


def test_rand_is_the_float32_composition():
    """oracle_rand_sequence, and the rand op's six draws and rf after, are random.glsl:2-7 composed in float32
    from the oracle's own sine and rt_glsl.h's stated dot."""
    sin32 = lambda x: pyoracle.eval_builtin("sin", x)   # noqa: E731
    for b in shade_cases.batches("rand"):
        r = b.rows
        want, rf = R.rand32(r[:, 9], r[:, 10], r[:, 11], 6, sin32)
        w = pyoracle.eval_shade_op(oracle_scene(b.scene)[0], "rand", r)
        assert np.array_equal(_f(w[:, 0:6]), want) and np.array_equal(_f(w[:, 6]), rf), b
        assert np.array_equal(shade_cases.draws(r, 6), want), b
        assert ((want >= 0) & (want < 1)).all()


def test_the_hook_refuses_rows_outside_its_guard():
    """px, py outside [0, 16384), rf outside [0, 4096) or any of them not finite: RT_ERR_INVALID_ARG before
    anything is launched (device < 0: the host half alone); a row inside the guard passes it."""
    import rtamd
    from rtamd._lib import debug_eval_shade_op
    ok = pyoracle.shade_rows(3, px=[0, 16383, 5], py=[0, 8191, 16383], rf=[0, 4095.5, 1])
    ok[:, 0:9] = np.nan   # the other fields are free
    for op in range(9):
        debug_eval_shade_op(None, op, 0, ok, device=-1)
    for col, bad in ((9, np.nan), (9, np.inf), (9, -1.0), (9, 16384.0), (10, np.nan), (10, -0.5), (10, 16384.0),
                     (11, np.nan), (11, np.inf), (11, -0.001), (11, 4096.0)):
        rows = ok.copy()
        rows[1, col] = bad
        for op in (0, 2, 6, 7, 8):
            with pytest.raises(rtamd.RTError):
                debug_eval_shade_op(None, op, 0, rows, device=-1)
    with pytest.raises(rtamd.RTError):
        debug_eval_shade_op(None, 7, 2, ok, device=-1)   # shade has forms 0 and 1
    debug_eval_shade_op(None, 8, 1, ok, device=-1)       # ... and so has the walk (the scene decides whether 1 may run)
    with pytest.raises(rtamd.RTError):
        debug_eval_shade_op(None, 8, 2, ok, device=-1)
    with pytest.raises(rtamd.RTError):
        debug_eval_shade_op(None, 2, 1, ok, device=-1)


def test_recorded_ratios_cover_every_op():
    rec = json.load(open(PROFILE))
    assert set(rec["ops"]) == set(OPS)
    for name, r in rec["ops"].items():
        assert r["undecided_share"] <= 0.10
        for k, v in r["worst_error_over_bound"].items():
            assert 0.01 <= v <= 1.0, (name, k, v)


if __name__ == "__main__":
    out = {"what": "tests/test_shade_ref64.py: the CPU oracle's worst |error| / derived rounding bound per value of "
                   "oracle_eval_shade_op, and the share of the random rows float64 cannot decide (u = 2^-24; "
                   "tests/ref64_shade.py derives the bounds)", "ops": {}}
    for name in OPS:
        try:
            worst, share = run_op(name)
        except AssertionError as e:
            print(name, "FAILED:", str(e)[:300])
            continue
        out["ops"][name] = {"undecided_share": round(share, 5),
                            "worst_error_over_bound": {k: round(v, 4) for k, v in worst.items()}}
        print(name, out["ops"][name])
    with open(PROFILE, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")

"""The CPU oracle's closest-hit walk (oracle_eval_shade_op's RT_SOP_TRACE: the trace_through_bvh that ray_color
calls) against the float64 walk written from the shader text (tests/ref64_trace.py), no GPU, by the rules of
tests/test_shade_ref64.py, on every batch of tests/trace_cases.py:
  * on decided rows the oracle and float64 agree on hit / miss, the closest prim's tif, the uv source's kind and
    index, the number of nodes visited, of leaf slots tested, the visit hash (restated here from
    oracle/rt_oracle.h: FNV-1a over the node indices in visit order) and the number of draws: "rf after" must be
    rf advanced by exactly that many float32 additions of 0.001;
  * t and the uv source's values lie within their derived rounding bounds (a quad source's third word and an
    untouched source are kept bit for bit);
  * at most 5 % of a scene's random rows are undecided, and no in-scope row of an edge set is.  The plain rule --
    every comparison on the row's way has margin, node tests included -- leaves 6.5 % of the scene "five"'s random rows
    undecided (a ray that meets a floor or a wall meets, at that very t, the boxes of the nodes standing on it), so a
    node test without margin is followed both ways (ref64_trace.walk states the rule) and such a row's visit counts
    and hash are left uncompared; both shares are recorded;
  * each edge set gives what trace_cases built it for (EXPECT).
An exact tie -- bound 0 on both t -- is decided: of two spheres the first visited stays (t < ray_t.max), of two
quads the second replaces it (t <= ray_t.max; interval.glsl).
profiles/trace_ref64.json records the shares and the worst |error| / bound (`python tests/test_trace_ref64.py`
rewrites it).
"""
import json
import os
import sys
import time

import numpy as np
import pytest

if __name__ == "__main__":
    _repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_repo, os.path.join(_repo, "oracle"), os.path.join(_repo, "raytracing-book_amd"),
                    os.path.join(_repo, "tests")]

import pyoracle
import ref64_shade
import ref64_trace
import shade_cases
import trace_cases
from test_ops_ref64 import _ratio
from trace_cases import BOX, MEDIUM, QUAD, SPHERE

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(REPO, "profiles", "trace_ref64.json")
CAP = 0.05
_oscenes = {}


def _f(w):
    return np.ascontiguousarray(w).view(np.float32)


def oracle_scene(name):
    if name not in _oscenes:
        sc, uni = trace_cases.scene(name)
        _oscenes[name] = (sc, pyoracle.OracleScene(sc, uniforms=uni))
    return _oscenes[name]


def check(sc, osc, rows, label, kind):
    """Compare the oracle's walk of `rows` with float64's; dict(undecided_share, out_of_scope, worst ratios)."""
    w = pyoracle.eval_shade_op(osc, "trace", rows)
    ref = ref64_trace.walk(ref64_shade.RefScene(sc), sc.buffers[1], rows, shade_cases.draws(rows, trace_cases.N_DRAWS))
    path, cls = ref["path"], ref["cls"]
    plain, scope = path.decided, path.scope
    decided = plain | ref["relaxed"]   # the relaxed rule (ref64_trace.walk): a node test without margin followed both ways
    got = dict(hit=w[:, 0] != 0, tif=w[:, 2].astype(np.int64), uvk=w[:, 3].view(np.int32).astype(np.int64),
               visits=w[:, 8].astype(np.int64), slots=w[:, 9].astype(np.int64), hash=w[:, 10].astype(np.int64))
    agree = np.ones(len(rows), bool)
    for k, v in got.items():
        # the visit counts and hash depend on the doubtful node tests' outcomes: compared under the plain rule only
        agree &= (v == cls[k]) | (~plain if k in ("visits", "slots", "hash") else False)
    agree &= _f(w[:, 7]) == ref64_shade.advance_rf(rows[:, pyoracle.SOP_RF], cls["count"])
    # what the walk did not write stays as it came in, bit for bit: the whole source, or a quad source's third word
    kept = ~ref["written"]
    agree &= ~kept | (w[:, 3:7] == rows.view(np.uint32)[:, 15:19]).all(axis=1)
    agree &= kept | ((cls["uvk"] >> 16) == 1) | (w[:, 6] == rows.view(np.uint32)[:, 18])
    bad = decided & ~agree
    assert not bad.any(), (f"{label}: oracle and float64 disagree on decided rows {np.nonzero(bad)[0][:8]}: oracle "
                           f"{ {k: v[bad][:3] for k, v in got.items()} } float64 { {k: cls[k][bad][:3] for k in got} }")
    if kind != "random":
        und = scope & ~decided
        assert scope.any(), f"{label}: no row of the edge set is in float64's scope"
        assert not und.any(), f"{label}: edge rows {np.nonzero(und)[0][:8]} are undecided (margins {path.margin[und][:8]})"
    worst = {}
    vals = dict(t=_f(w[:, 1]), uva=_f(w[:, 4]), uvb=_f(w[:, 5]), uvc=_f(w[:, 6]))
    for k, e in ref["val"].items():
        mask = decided & ref["mask"][k] & (ref["written"] if k != "t" else True)
        r = _ratio(vals[k], e, mask)
        over = r > 1.0
        assert not over.any(), f"{label}: {k} off by {r[over][:4]} x its rounding bound at rows {np.nonzero(over)[0][:4]}"
        worst[k] = float(r.max()) if len(r) else 0.0
    return dict(rows=len(rows), undecided_share=float((scope & ~decided).sum()) / max(len(rows), 1),
                undecided_share_plain_rule=float((scope & ~plain).sum()) / max(len(rows), 1),
                out_of_scope=int((~scope).sum()), hits=int(cls["hit"].sum()), draws=int(cls["count"].sum()),
                worst_error_over_bound=worst)


def run_batch(b):
    sc, osc = oracle_scene(b.scene)
    return check(sc, osc, b.rows, repr(b), b.kind)


@pytest.mark.parametrize("name", list(trace_cases.RANDOM_N))
def test_random_rows_against_float64(name):
    b = [x for x in trace_cases.batches() if x.kind == "random" and x.scene == name][0]
    res = run_batch(b)
    print(f"{name}: {res}")
    assert res["undecided_share"] <= CAP, f"{name}: {res['undecided_share']:.3f} of the random rows are undecided"
    assert res["hits"] >= len(b.rows) // 10 and res["hits"] < len(b.rows), res
    if any(k[0] == MEDIUM for k in trace_cases.slot_rank(trace_cases.scene(name)[0])):
        assert res["draws"] > 0, "no medium of the scene drew"
    # t's worst error lies between a hundredth of its bound and the bound: the bound is neither missed nor idle
    assert 0.01 <= res["worst_error_over_bound"]["t"] <= 1.0, res


# What each edge set of the knot must give, whoever computes it (float64 here; the oracle must agree, and the device
# the oracle): rows -> (hit, tif, uv kind_idx, draws) with None = not stated
def _tif(typ, idx, side=0):
    return typ | side << 4 | idx << 16


EXPECT = {
    "tie_spheres": [(1, _tif(SPHERE, 1), 1 << 16 | 1, 0), (1, _tif(SPHERE, 2), 1 << 16 | 2, 0)],   # the first visited stays
    "tie_quads": [(1, _tif(QUAD, 0), 2 << 16, 0)] * 2,                                             # the second replaces it
    "tmin": [(1, _tif(QUAD, 0), 2 << 16, 0), (0, 0, 0, 0), (1, _tif(QUAD, 0), 2 << 16, 0)] * 1
            + [(1, _tif(QUAD, 0), 2 << 16, 0), (0, 0, 0, 0)],
    "slab_sign": [(0, 0, 0, 0), (1, _tif(QUAD, 2), 2 << 16, 0)],
    "zero_dir": [(0, 0, 0, 0)] * 10,
    "stale_uv": [(1, _tif(MEDIUM, 0), 2 << 16, None)] * 4 + [(1, _tif(MEDIUM, 0), 1 << 16 | 5, None)] * 4,
    "pruned_medium": [(1, _tif(QUAD, 3), 2 << 16, 0)] * 3,
    "zero_draw": [(None, None, None, 2)] * 6,          # the first test draws 0 and cannot scatter; alone in its leaf, it is tested again
}


@pytest.mark.parametrize("name", list(trace_cases.edge_sets()))
def test_edge_rows_against_float64(name):
    b = [x for x in trace_cases.batches() if x.name == name][0]
    sc, osc = oracle_scene(b.scene)
    if b.kind == "device":   # 0 * inf in a slab: outside float64's scope; what the set was built for is asked of the oracle
        w = pyoracle.eval_shade_op(osc, "trace", b.rows)
        for k, (hit, tif, uvk, _) in enumerate(EXPECT.get(name, [])):
            assert (int(w[k, 0]), int(w[k, 2]), int(w[k, 3])) == (hit, tif, uvk), (name, k, w[k])
        assert (w[:, 7] == b.rows.view(np.uint32)[:, pyoracle.SOP_RF]).all()
        return
    res = run_batch(b)
    print(f"{name}: {res}")
    if name not in EXPECT:
        return
    cls = ref64_trace.walk(ref64_shade.RefScene(sc), sc.buffers[1], b.rows, shade_cases.draws(b.rows, trace_cases.N_DRAWS))["cls"]
    w = pyoracle.eval_shade_op(osc, "trace", b.rows)
    assert len(EXPECT[name]) == len(b.rows)
    for k, (hit, tif, uvk, draws) in enumerate(EXPECT[name]):
        for what, want, r64, orc in (("hit", hit, int(cls["hit"][k]), int(w[k, 0])), ("tif", tif, int(cls["tif"][k]), int(w[k, 2])),
                                     ("uvk", uvk, int(cls["uvk"][k]), int(w[k, 3]))):
            assert want is None or (r64 == want and orc == want), f"{name} row {k}: {what} float64 {r64:#x} oracle {orc:#x}, expected {want:#x}"
        if draws is not None:
            rf = ref64_shade.advance_rf(b.rows[k:k + 1, pyoracle.SOP_RF], np.array([draws]))[0]
            assert cls["count"][k] == draws and _f(w[k:k + 1, 7])[0] == rf, f"{name} row {k}: {cls['count'][k]} draws, expected {draws}"
        if name == "stale_uv":   # more draws than none: the fog scattered
            assert cls["count"][k] >= 1
    if name == "stale_uv":       # the quad's third word is the one the row came with
        assert (_f(w[:4, 6]) == 3.0).all()
    if name == "zero_draw":
        assert (shade_cases.draws(b.rows, 1)[:, 0] == 0.0).all()


def test_every_medium_of_the_knot_is_alone_in_its_leaf():
    """So that each one's second test runs, and draws, whenever the first did not scatter."""
    sc = trace_cases.scene("knot")[0]
    assert sorted(trace_cases.singleton_media(sc)) == [0, 1, 2]
    assert any(int(m[1]) == BOX for m in shade_cases.records(sc)[3].view(np.int32))      # a box-bounded one
    assert 16 <= len(trace_cases.nodes(sc)) < 100


def test_recorded_shares_are_within_the_cap():
    rec = json.load(open(PROFILE))
    names = {repr(b) for b in trace_cases.batches() if b.kind != "device"}
    assert set(rec["batches"]) == names
    for name, r in rec["batches"].items():
        assert r["undecided_share"] <= (CAP if "random" in name else 0.0), (name, r)
        for k, v in r["worst_error_over_bound"].items():
            assert v <= 1.0, (name, k, v)


if __name__ == "__main__":
    out = {"what": "tests/test_trace_ref64.py: per batch of tests/trace_cases.py the share of rows the float64 walk "
                   "(tests/ref64_trace.py) cannot decide -- by the plain rule (every comparison on the row's way has "
                   "margin, node tests included) and with a node test without margin followed both ways, its visit "
                   "counts and hash then uncompared; the cap is 5 % of a random set, none of an edge set --, the rows "
                   "outside float64's scope, and the CPU oracle's worst |error| / derived rounding bound (u = 2^-24)",
           "batches": {}}
    t0 = time.time()
    for b in trace_cases.batches():
        if b.kind == "device":
            continue
        r = run_batch(b)
        r["undecided_share"] = round(r["undecided_share"], 5)
        r["undecided_share_plain_rule"] = round(r["undecided_share_plain_rule"], 5)
        r["worst_error_over_bound"] = {k: round(v, 4) for k, v in r["worst_error_over_bound"].items()}
        out["batches"][repr(b)] = r
        print(repr(b), r)
    print(f"{time.time() - t0:.1f} s")
    with open(PROFILE, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")

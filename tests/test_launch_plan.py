"""The render launch decision as a host function (rt_plan.h plan_kernel, through rt_debug_plan_kernel;
no GPU needed): which render_persistent instantiation a launch runs, with how much LDS, what it
refuses and what rt_debug_last_launch reports.

tests/golden/launch_plan.npz holds what the commit before plan_kernel decided (its rt_launch_render,
launches recorded instead of made; tests/golden/launch_plan.md) over an enumerated input space: both
libraries, every kernel variant, division regime, box records, sphere pairs, tile mask, staging state,
workgroup size, two-level walk, and LDS layouts that make the default configuration hold and fail
through each of its terms, with the over-size refusals.  plan_kernel must decide every row alike; and,
computed on this code alone, it must choose nothing outside the table of instantiations and leave no
entry of the table unused.
"""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import rtamd
from test_adaptive_host import FIELDS, render_instances

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "launch_plan.npz")
PROFILES = os.path.join(REPO, "profiles")
BOXQ, MASK = 256, 512


def header_enum(prefix):
    """The names of rt_debug.h's enum that ends with `prefix`N, in order (the header documents the arrays)."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "rt", "rt_debug.h")).read(), flags=re.S)
    for body in re.findall(r"enum\s*\{(.*?)\}", text, flags=re.S):
        names = re.findall(r"\b(%s[A-Z0-9_]+)\b" % prefix, body)
        if names and names[-1] == prefix + "N":
            return {n[len(prefix):]: k for k, n in enumerate(names[:-1])}
    raise AssertionError(prefix)


PK, PKO = header_enum("RT_PK_"), header_enum("RT_PKO_")
LI = {n: k for k, n in enumerate(rtamd.render.LAUNCH_FIELDS)}


def plan(inputs, ab):
    """rt_debug_plan_kernel for rows of inputs -> (plan [n, RT_PKO_N], info [n, 21])."""
    L = rtamd.amd()
    inputs = np.ascontiguousarray(inputs, np.int32)
    out = np.zeros((len(inputs), len(PKO)), np.int32)
    info = np.zeros((len(inputs), 21), np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    for k in range(len(inputs)):
        rc = L.rt_debug_plan_kernel(inputs[k].ctypes.data_as(ip), len(PK), int(ab[k]), out[k].ctypes.data_as(ip),
                                    len(PKO), info[k].ctypes.data_as(ip), None, 0, None)
        assert rc == 0
    return out, info


def table():
    L = rtamd.amd()
    n = ctypes.c_int()
    one, o, inf = np.zeros(len(PK), np.int32), np.zeros(len(PKO), np.int32), np.zeros(21, np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    args = (one.ctypes.data_as(ip), len(PK), 0, o.ctypes.data_as(ip), len(PKO), inf.ctypes.data_as(ip))
    assert L.rt_debug_plan_kernel(*args, None, 0, ctypes.byref(n)) == 0
    t = np.zeros((n.value, 2), np.int32)
    assert L.rt_debug_plan_kernel(*args, t.ctypes.data_as(ip), n.value - 1, None) == -4   # RT_ERR_LIMIT: a short table
    assert L.rt_debug_plan_kernel(*args, t.ctypes.data_as(ip), n.value, None) == 0
    return [(int(b), int(o)) for b, o in t]


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    g = {k: z[k] for k in ("ab", "inputs", "plan", "info")}
    g["parent"] = str(z["parent"])
    assert g["inputs"].shape[1] == len(PK) and g["plan"].shape[1] == len(PKO) and g["info"].shape[1] == 21
    g["got_plan"], g["got_info"] = plan(g["inputs"], g["ab"])
    return g


def test_fixture_covers_the_input_space(golden):
    """The rows the comparison and the closure below stand on."""
    i, p, ab = golden["inputs"], golden["plan"], golden["ab"]
    assert re.fullmatch(r"[0-9a-f]{40}", golden["parent"])
    assert set(ab) == {0, 1} and set(i[ab == 0][:, PK["VARIANT"]]) == {0}
    assert set(i[ab == 1][:, PK["VARIANT"]]) == {0, 37, 30, 61, 39, 38, 31, 69}
    for name, vals in (("FASTDIV", {0, 1}), ("BOX_ALL_CMP", {0, 1}), ("BOX_INTERIOR", {0, 1}), ("SPH_PAIRS", {0, 1, 2}),
                       ("TILE_LIST", {0, 1}), ("BLOCK", {512, 1024}), ("LEAF_PF", {0, 1}), ("MEDIA_SPH", {0, 1})):
        assert set(i[ab == 0][:, PK[name]]) == vals, name
    staging = {tuple(r) for r in i[:, [PK["SAMPLES"], PK["SFLAGS"], PK["WBUF"]]]}
    assert staging == {(1, 1, 0), (1, 0, 0), (0, 0, 1), (0, 0, 0)}
    for name in ("SPH_LDS", "SPH_MAT_LDS", "MEDIA_LDS", "TEX_LDS", "BOX_MAT_LDS", "BOX_CMP_LDS"):
        assert (i[:, PK[name]] < 0).any() and (i[:, PK[name]] >= 0).any(), name
    ok = p[:, PKO["OK"]] == 1
    assert set(p[ok & (ab == 1)][:, PKO["SHAPE"]]) == {0, 1, 2, 3, 4, 5} and set(p[ok & (ab == 0)][:, PKO["SHAPE"]]) == {2, 5}
    assert set(p[ok & (ab == 1)][:, PKO["STATS"]]) == {0, 1}
    none = (i[:, PK["SAMPLES"]] == 0) & (i[:, PK["WBUF"]] == 0)
    assert not ok[none & (p[:, PKO["POOL"]] == 1)].any() and not ok[none & (ab == 0)].any()   # pooled: refused
    big = i[:, PK["LDS_END_F4"]] * 16 > 160 * 1024                                         # over-size: refused
    assert big.any() and not ok[big & (ab == 0)].any() and (~ok).sum() > 1000 and ok.sum() > 1000


def test_plan_equals_the_parent_on_every_row(golden):
    for name, k in PKO.items():
        bad = np.nonzero(golden["got_plan"][:, k] != golden["plan"][:, k])[0]
        assert bad.size == 0, (name, bad[:5], golden["inputs"][bad[:1]], golden["got_plan"][bad[:1]], golden["plan"][bad[:1]])
    for name, k in LI.items():
        bad = np.nonzero(golden["got_info"][:, k] != golden["info"][:, k])[0]
        assert bad.size == 0, (name, bad[:5], golden["inputs"][bad[:1]])


def test_every_plan_is_in_the_table_and_every_entry_is_planned(golden):
    """Closure, on this code's answers alone: no missing instantiation and no dead one."""
    t = table()
    assert len(t) == 56 and len(set(t)) == 56
    assert all((b, o ^ MASK) in t for b, o in t)                         # every entry has its mask twin
    p, ab = golden["got_plan"], golden["ab"]
    ok = p[:, PKO["OK"]] == 1
    stream = ok & (p[:, PKO["POOL"]] == 1) & np.isin(p[:, PKO["SHAPE"]], (2, 5))
    assert (ab[ok] == 1)[~stream[ok]].all()                              # the release library plans nothing else
    chosen = {(int(b), int(o)) for b, o in p[stream & (p[:, PKO["STATS"]] == 0)][:, [PKO["BLOCK"], PKO["OPT"]]]}
    assert chosen == set(t)
    release = {(int(b), int(o)) for b, o in p[stream & (ab == 0)][:, [PKO["BLOCK"], PKO["OPT"]]]}
    assert release == set(t)
    twins = {(int(b), int(o)) for b, o in p[stream & (p[:, PKO["STATS"]] == 1)][:, [PKO["BLOCK"], PKO["OPT"]]]}
    assert twins == {(b, o & ~BOXQ) for b, o in t}                       # the stats twins: the table without BOXQ
    rest = p[ok & ~stream]
    assert (rest[:, PKO["BLOCK"]] == 512).all() and (rest[:, PKO["OPT"]] == 0).all()


def test_reports_that_follow_the_chosen_kernel(golden):
    """box_interior is the kernel's RT_OPT_BOXQ bit; sphere_pairs is its RT_OPT_SPAIR bit except where the
    spheres are not staged (the report then says 0 while the pair kernel runs: kept as it was)."""
    p, inf, i = golden["got_plan"], golden["got_info"], golden["inputs"]
    ok = p[:, PKO["OK"]] == 1
    assert ((p[ok][:, PKO["OPT"]] & BOXQ != 0) == (inf[ok][:, LI["box_interior"]] == 1)).all()
    spair = p[:, PKO["OPT"]] & 64 != 0
    staged = i[:, PK["SPH_LDS"]] >= 0
    assert (inf[ok & staged][:, LI["sphere_pairs"]] == spair[ok & staged]).all()
    assert (ok & spair & ~staged).any() and not inf[ok & ~staged][:, LI["sphere_pairs"]].any()
    assert (inf[ok][:, LI["tiles_active"]] == i[ok][:, PK["N_ACTIVE"]]).all()


def test_golden_scenes_report_the_recorded_launches():
    """Scenes 0-9 as tools/lib_ab.py renders them (1920x1080, 64 frames, spp 4096), through rt_debug_plan_scene
    and then rt_debug_plan_kernel: every scene is planned, and the scenes profiles/pass_blocks_lib_ab_1.log
    holds (8, 0, 6: what that call rendered) report every rt_debug_last_launch field the release library logged
    on the MI355X (256 CUs: 4096 resident waves).  No field is left out: the free memory, the one input that
    needs the device, changes only the frames per launch, which the report does not carry."""
    logged = {}
    for ln in open(os.path.join(PROFILES, "pass_blocks_lib_ab_1.log")):
        m = re.match(r"scene (\d+) raytracing-book_amd/lib/librtamd\.so: last_launch (\{.*\})", ln)
        if m:
            logged[int(m.group(1))] = json.loads(m.group(2))
    assert set(logged) == {8, 0, 6}
    for sid in range(10):
        sc = rtamd.Scene(sid, 1920, 1080, seed=1)
        got = rtamd.plan_scene(sc, 64, spp=4096, waves=256 * 16)
        assert got["launched"] == 1
        out, info = plan(got["pk"][None, :], [0])
        assert out[0][PKO["OK"]] == 1, sid
        report = {n: int(info[0][k]) for n, k in LI.items()}
        report.update({f: got[f] for f in ("bvh_mode", "box_vnodes", "collapsed", "rebuilt")})
        report["shape_name"] = rtamd.render.SHAPES[report["shape"]]
        assert report["tiles_active"] == 135 * 240 and report["staged"] == 1, sid
        if sid in logged:
            assert report == logged[sid], (sid, report, logged[sid])


def test_argument_errors():
    L = rtamd.amd()
    ip = ctypes.POINTER(ctypes.c_int)
    one, o, inf = np.zeros(len(PK), np.int32), np.zeros(len(PKO), np.int32), np.zeros(21, np.int32)
    a = (one.ctypes.data_as(ip), len(PK), 0, o.ctypes.data_as(ip), len(PKO), inf.ctypes.data_as(ip), None, 0, None)
    assert L.rt_debug_plan_kernel(*a) == 0 and o[PKO["OK"]] == 0          # no active tile: refused
    for k, v in ((0, None), (1, len(PK) - 1), (3, None), (4, len(PKO) + 1), (5, None), (7, -1)):
        b = list(a)
        b[k] = v
        assert L.rt_debug_plan_kernel(*b) == -1, k


def test_recorded_resources_are_identical():
    """profiles/launch_plan_resources_{parent,this}.txt: `make -C raytracing-book_amd resources` on the parent
    commit and on the commit that moved the launch decision to the host: the same render_persistent instances
    (the names carry <MINW, STATS, BLOCK, OPT>) with the same VGPRs, spills, scratch, LDS and occupancy.
    The folds changed (one body, rt_moments.hip): none of them uses scratch or spills."""
    pa = open(os.path.join(PROFILES, "launch_plan_resources_parent.txt")).read()
    th = open(os.path.join(PROFILES, "launch_plan_resources_this.txt")).read()
    a, b = render_instances(pa), render_instances(th)
    assert len(a) == 56 and set(a) == set(b)
    for k in a:
        for f in FIELDS:
            assert f in a[k], (k, f)
            assert a[k][f] == b[k][f], (k, f, a[k][f], b[k][f])
    names = {(int(m.group(1)), int(m.group(2))) for m in
             (re.search(r"render_persistentILi4ELb0ELi(\d+)ELi(\d+)EEEvPK", k) for k in a)}
    assert names == set(table())                                          # the table is what is instantiated
    folds = {}
    cur = None
    for ln in th.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
        m = re.search(r"(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", ln)
        if m and cur and "fold_" in cur:
            folds.setdefault(cur, {})[m.group(1)] = int(m.group(2))
    assert len(folds) == 4 and all(v == 0 for d in folds.values() for v in d.values()), folds

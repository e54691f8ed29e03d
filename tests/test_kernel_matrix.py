"""tests/kernel_matrix.py against the planner, on the host (rt_debug_plan_scene, then rt_debug_plan_kernel;
no GPU): the table of (scene, options) rows that tests/test_gpu_kernel_matrix.py launches must keep choosing
the kernels it names, cover every instantiation rt_render can reach, and leave out exactly the four it cannot.
Planned as the GPU test renders: 61x45, two launches of 3 frames (first_frame 1, then 4), spp 6, and the
MI355X's 4096 resident waves.
"""
import json
import os

import numpy as np
import pytest

import kernel_matrix as km
from test_launch_plan import LI, table

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVES, FREE = 256 * 16, 1 << 38
TL = 16   # RT_OPT_TL


def prev_counts(first_frame, mask):
    """The per-tile counts before a launch of the GPU test: none, or LAUNCH frames in the tiles rendered."""
    prev = np.zeros(km.NT, np.int32)
    if first_frame > 1:
        prev[km.MASK if mask is not None else slice(None)] = first_frame - 1
    return prev


_MEMO = {}


def plan_of(name, options, masked, first):
    """(last_launch list, (block, opt)) of one launch, planned once per distinct configuration."""
    key = (name, tuple(sorted(options.items())), masked, first)
    if key not in _MEMO:
        mask = km.MASK if masked else None
        launch, _, counts, kernel = km.planned(km.scene(name), km.LAUNCH, first, options, mask, prev_counts(first, mask),
                                               WAVES, FREE)
        assert np.array_equal(counts, prev_counts(first + km.LAUNCH, mask)), key
        _MEMO[key] = (launch, kernel)
    return _MEMO[key]


@pytest.fixture(scope="module")
def plans():
    """(row, state, masked, first_frame) -> (last_launch list, (block, opt)), every combination planned once."""
    out = {}
    for row, (name, options) in km.ROWS.items():
        for state, extra in km.STAGING.items():
            for masked in (False, True):
                for first in (1, km.LAUNCH + 1):
                    out[(row, state, masked, first)] = plan_of(name, {**options, **extra}, masked, first)
    return out


def test_table_shape():
    assert len(km.ROWS) == 26 and len(km.kernels()) == 52 and len(set(km.kernels())) == 52
    assert km.W % 8 == 5 and km.H % 8 == 5 and km.NT == ((km.W + 7) // 8) * ((km.H + 7) // 8) == 48
    assert set(km.MASK) == {0, km.TX - 1, 2 * km.TX + 3, (km.TY - 1) * km.TX, km.NT - 1}
    n = {k: len(km.configurations(k)) for k in km.kernels()}
    for (block, opt), c in n.items():
        row = (block, opt & ~km.MASKED)
        assert c == (1 if opt & km.STD else 4 + len(km.EXTRA.get(row, []))), (block, opt, c)
    assert sorted(n.values()).count(5) == 2   # (512, 47) and its twin: two LDS layouts
    for row, extra in km.EXTRA.items():
        assert row in km.ROWS and not row[1] & km.STD and all(s in km.STAGING for _, _, s in extra)


def test_every_row_plans_the_kernel_it_names(plans):
    """Each row x staging state x {no mask, mask}: the named (block, opt), or for an RT_OPT_STD row under a
    state other than "staged" its sibling without RT_OPT_STD; the same kernel for first_frame 1 and for the
    launch that extends it (first_frame 4), which is what the GPU test renders."""
    for (row, state, masked, first), (launch, kernel) in plans.items():
        assert kernel == km.kernel_under(row, state, masked), (row, state, masked, first, kernel)
        assert launch[LI["tiles_active"]] == (len(km.MASK) if masked else km.NT)
        assert launch[LI["block"]] == row[0]
        assert kernel[1] & km.MASKED == (km.MASKED if masked else 0)
    for (row, state, masked, first), (launch, kernel) in plans.items():
        if first == 1:
            again = plans[(row, state, masked, km.LAUNCH + 1)]
            assert again[1] == kernel and again[0] == launch, (row, state, masked)
    for row, extra in km.EXTRA.items():   # the extra configurations come from the STD rows' other states
        for name, options, state in extra:
            src = [r for r, (n, o) in km.ROWS.items() if (n, o) == (name, options)]
            assert len(src) == 1 and km.kernel_under(src[0], state, False) == row


def test_the_gpu_configurations_plan_their_kernel():
    """What tests/test_gpu_kernel_matrix.py iterates over: every configuration of every id plans that id."""
    for kernel in km.kernels():
        for label, name, options, mask in km.configurations(kernel):
            for first in (1, km.LAUNCH + 1):
                got = plan_of(name, options, mask is not None, first)[1]
                assert got == kernel, (kernel, label, first, got)
            if mask is not None:   # a twin's last launch: the other 43 tiles, six frames at once
                prev = prev_counts(km.FRAMES + 1, mask)
                launch, _, counts, got = km.planned(km.scene(name), km.FRAMES, 1, options, km.REST, prev, WAVES, FREE)
                assert got == kernel and launch[LI["tiles_active"]] == len(km.REST) == 43, (kernel, label, got)
                assert (counts == km.FRAMES).all()


def test_closure(plans):
    """The union of everything planned is the table of instantiations without DEAD, exactly: a new
    instantiation without a row fails here, and so does a dead entry that becomes reachable."""
    t = set(table())
    assert len(t) == 56 and km.DEAD < t and len(km.DEAD) == 4
    chosen = {kernel for _, kernel in plans.values()}
    assert chosen == t - km.DEAD
    assert chosen == set(km.kernels())
    assert {(b, o ^ km.MASKED) for b, o in km.DEAD} == km.DEAD


def test_every_kernel_without_std_is_planned_under_every_staging_state(plans):
    seen = {}
    for (row, state, masked, first), (_, kernel) in plans.items():
        seen.setdefault(kernel, set()).add(state)
    for kernel, states in seen.items():
        assert states == ({"staged"} if kernel[1] & km.STD else set(km.STAGING)), (kernel, states)
    assert sum(1 for k in seen if not k[1] & km.STD) == 36
    # and by the kernel's own row (the configurations the GPU test runs), not only by an STD row's fall
    for kernel in km.kernels():
        if not kernel[1] & km.STD:
            row = (kernel[0], kernel[1] & ~km.MASKED)
            for state in km.STAGING:
                assert plans[(row, state, bool(kernel[1] & km.MASKED), 1)][1] == kernel


def test_two_level_rows_stage_no_shading_tables(plans):
    """Why DEAD is dead, as far as this table shows it: every row planned as the two-level walk (shape 5)
    reports shade_lds 0 and a kernel without RT_OPT_STD.  rt_plan.cpp plan_lds stages the shading tables only
    `if (in.shade_lds && pooled && !tl)`, and plan_kernel's std_cfg ends `&& a.tex_lds >= 0`; rt_args.cpp gives
    both the same node count, so they agree on what is two-level."""
    tl_rows = 0
    for (row, state, masked, first), (launch, kernel) in plans.items():
        if launch[LI["shape"]] == 5:
            tl_rows += 1
            assert kernel[1] & TL and launch[LI["shade_lds"]] == 0 and not kernel[1] & km.STD, (row, state, masked)
        else:
            assert launch[LI["shape"]] == 2 and not kernel[1] & TL
    assert tl_rows == 4 * 4 * 2 * 2   # four two-level rows x states x mask x launches
    assert all(o & TL and o & km.STD for _, o in km.DEAD)


def test_recorded_enumeration_reaches_nothing_more():
    """profiles/kernel_matrix.json (tools/kernel_reach.py: every subset of at most three of thirteen option
    settings over twelve scenes, with and without a mask): what it never reached is DEAD, and each entry's
    recorded first configuration is read, not planned again."""
    doc = json.load(open(os.path.join(REPO, "profiles", "kernel_matrix.json")))
    assert doc["table"] == 56 and doc["max_options"] == 3 and len(doc["scenes"]) == 12 and len(doc["settings"]) == 13
    assert {tuple(k) for k in doc["never_reached"]} == km.DEAD
    reached = {(r["block"], r["opt"]) for r in doc["reached"]}
    assert reached == set(km.kernels()) and len(doc["reached"]) == 52
    assert doc["plans"] > 12 * 300 * 2 and all(len(r["options"]) <= 3 for r in doc["reached"])

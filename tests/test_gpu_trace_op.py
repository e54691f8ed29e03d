"""The plain closest-hit walk on the device (rt_debug_eval_shade_op's RT_SOP_TRACE: the link walk from the
root over the context's plain link buffer, the generic leaf tests with media on, then the uv hand-over),
one lane per row, against the CPU oracle's trace_through_bvh word for word: every row of
tests/trace_cases.py -- the ones tests/test_trace_ref64.py pins to float64, the undecided ones and the ones
outside float64's scope (NaN, inf) -- on each scene, in each form the scene allows.  The oracle's words 8..10
(its visit counts and hash) describe the reference's stack walk and are absent on the device (rt_debug.h).
NaN positions must match; payloads are free.  For each batch the oracle runs first.

Form 0 (leaf_prims_t<false, false>) must give the same words with the box bounds pre-test on and off; form 1
(the shared-reciprocal divisions) is refused unless the scene is in that regime."""
import numpy as np
import pytest

import pyoracle
import rtamd
import trace_cases
from rtamd._lib import debug_eval_shade_op

pytestmark = pytest.mark.gpu

OP = pyoracle.SHADE_OPS["trace"]
SCENES = list(trace_cases.RANDOM_N)


def _same(a, b):
    fa, fb = a.view(np.float32), b.view(np.float32)
    return (a == b) | (np.isnan(fa) & np.isnan(fb))


@pytest.fixture(scope="module")
def contexts(gpu):
    made = {}

    def get(name):
        if name not in made:
            sc, uni = trace_cases.scene(name)
            ctx = rtamd.RenderContext(devices=(0,))
            ctx.upload_scene(sc)
            ctx.set_params(max_depth=5, uniforms=uni)
            ctx.resize(sc.width, sc.height)
            made[name] = (ctx, pyoracle.OracleScene(sc, uniforms=uni))
        return made[name]

    yield get
    for ctx, _ in made.values():
        ctx.close()


def _fastdiv(ctx):
    """Whether the scene is in the shared-reciprocal regime: what a render of it reports."""
    ctx.render(1, rtamd.frame_rand_factors(1, 0, 1))
    ctx.sync()
    return ctx.last_launch()["fastdiv"] == 1


@pytest.mark.parametrize("name", SCENES)
def test_device_walk_equals_the_oracle(contexts, name):
    ctx, osc = contexts(name)
    fd = _fastdiv(ctx)
    ran = []
    for b in trace_cases.batches():
        if b.scene != name:
            continue
        want = pyoracle.eval_shade_op(osc, "trace", b.rows)          # the oracle first
        want[:, 8:11] = 0                                            # absent on the device
        for form, pretest in ((0, 1), (0, 0)) + (((1, 1),) if fd else ()):
            ctx.set_option("box_pretest", pretest)
            got = debug_eval_shade_op(ctx, OP, form, b.rows)
            bad = ~_same(got, want).all(axis=1)
            assert not bad.any(), (f"{b!r} form {form} pretest {pretest}: rows {np.nonzero(bad)[0][:8]} differ: device "
                                   f"{got[bad][:2]} vs oracle {want[bad][:2]}")
            ran.append((b.name, form, pretest))
        ctx.set_option("box_pretest", 1)
        if not fd:
            with pytest.raises(rtamd.RTError):
                debug_eval_shade_op(ctx, OP, 1, b.rows)
    print(name, "fastdiv", fd, ran)
    assert ran


def test_form_1_runs_somewhere_and_guard_applies(contexts):
    assert any(_fastdiv(contexts(n)[0]) for n in SCENES), "no scene is in the shared-reciprocal regime: form 1 never ran"
    ctx, _ = contexts("knot")
    rows = pyoracle.shade_rows(2, o=[[8, 0, 4]] * 2, d=[[0, 0, -1]] * 2, px=[1, 2], py=[3, 4], rf=[0.5, np.nan])
    with pytest.raises(rtamd.RTError):
        debug_eval_shade_op(ctx, OP, 0, rows)
    rows[1, pyoracle.SOP_RF] = 0.5
    with pytest.raises(rtamd.RTError):
        debug_eval_shade_op(ctx, OP, 2, rows)
    # outside the shared-reciprocal regime (here: the option off, so no launch would take those forms) form 1 is refused
    assert _fastdiv(ctx)
    debug_eval_shade_op(ctx, OP, 1, rows)
    ctx.set_option("fastdiv", 0)
    try:
        with pytest.raises(rtamd.RTError):
            debug_eval_shade_op(ctx, OP, 1, rows)
        debug_eval_shade_op(ctx, OP, 0, rows)
    finally:
        ctx.set_option("fastdiv", 1)

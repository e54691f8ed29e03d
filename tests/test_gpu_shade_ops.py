"""The render kernels' sampling, light, camera and shading functions on the device, one lane per row
(rt_debug_eval_shade_op, bound to a context's scene), against the CPU oracle's oracle_eval_shade_op word for
word: every row of tests/shade_cases.py -- the rows tests/test_shade_ref64.py pins to float64 and the ones
it leaves out as undecided or out of float64's scope (NaN, textures) -- in every form of the op.  NaN
positions must match; payloads are free.  For each batch the oracle runs first.

shade has two forms: 0 is shade<false, false, false, false>, 1 is shade<false, false, false, true>, the
compact-box kernels' trim whose no-light branch folds the mixture's constants and skips lights_random.
Form 1 must equal form 0 and the oracle on the no-light scene, where its own branch runs, and on the
scenes with lights, where it takes the shared code.  One word is exempt by construction: on the no-light
scene a row whose mixture draw is below 0.5 never reads rf again (the path ends, or goes on along
vec3(0)), and form 1 leaves out lights_random's one draw there, so its rf after is exactly one float32
addition of 0.001 short of form 0's -- asserted as such, not skipped."""
import numpy as np
import pytest

import pyoracle
import rtamd
import shade_cases
from rtamd._lib import debug_eval_shade_op

pytestmark = pytest.mark.gpu

# words compared per op (the rest stay 0 on both sides and are compared too)
N_WORDS = 12


def _same(a, b):
    fa, fb = a.view(np.float32), b.view(np.float32)
    return (a == b) | (np.isnan(fa) & np.isnan(fb))


@pytest.fixture(scope="module")
def contexts(gpu):
    made = {}

    def get(name):
        if name not in made:
            sc, uni = shade_cases.scene(name)
            ctx = rtamd.RenderContext(devices=(0,))
            ctx.upload_scene(sc)
            ctx.set_params(max_depth=5, uniforms=uni)
            ctx.resize(sc.width, sc.height)
            made[name] = (ctx, pyoracle.OracleScene(sc, uniforms=uni), int(np.frombuffer(bytes(sc.buffers[5]), np.int32)[0]))
        return made[name]

    yield get
    for ctx, _, _ in made.values():
        ctx.close()


@pytest.mark.parametrize("name", list(shade_cases.ALL))
def test_device_equals_the_oracle(contexts, name):
    op = pyoracle.SHADE_OPS[name]
    ran_nolight = False
    for b in shade_cases.batches(name):
        ctx, osc, n_lights = contexts(b.scene)
        want = pyoracle.eval_shade_op(osc, name, b.rows)          # the oracle first: its loops ended
        for form in ((0, 1) if name == "shade" else (0,)):
            got = debug_eval_shade_op(ctx, op, form, b.rows)
            same = _same(got, want)
            if name == "shade" and form == 1 and n_lights == 0:
                # rows that drew the mixture below 0.5: the oracle and form 0 drew once more in lights_random
                w0 = want.view(np.float32)
                zero_d = (want[:, 0] == 0) & ((want[:, 4:7] & 0x7FFFFFFF) == 0).all(axis=1)
                short = ~same[:, 10] & (got.view(np.float32)[:, 10] + np.float32(0.001) == w0[:, 10])
                dead = short & ((want[:, 0] == 1) | zero_d)
                same[:, 10] |= dead
                ran_nolight |= bool(dead.any())
            bad = ~same.all(axis=1)
            assert not bad.any(), (f"{b!r} form {form}: rows {np.nonzero(bad)[0][:8]} differ: device "
                                   f"{got[bad][:2]} vs oracle {want[bad][:2]}")
    if name == "shade":
        assert ran_nolight, "no row took form 1's no-light branch with a mixture draw below 0.5"


def test_rows_outside_the_guard_are_refused_with_a_context(contexts):
    ctx, _, _ = contexts("zoo0")
    rows = pyoracle.shade_rows(2, px=[1, 2], py=[3, 4], rf=[0.5, np.nan])
    with pytest.raises(rtamd.RTError):
        debug_eval_shade_op(ctx, pyoracle.SHADE_OPS["unit_vec"], 0, rows)
    rows = pyoracle.shade_rows(1, tif=1 | 4000 << 16, px=1, py=1, rf=0.5)   # no such sphere
    with pytest.raises(rtamd.RTError):
        debug_eval_shade_op(ctx, pyoracle.SHADE_OPS["shade"], 0, rows)

"""The render kernels' own operations on the device, one lane per row (rt_debug_eval_op), against the CPU
oracle's per-operation entry points, bit for bit: every row of tests/ops_cases.py -- the rows
tests/test_ops_ref64.py pins to float64, and the ones it has to leave out as undecided or out of
float64's scope -- in every device form of the op (plain / shared-reciprocal, full / compact /
compact-q box, aabb_fast / aabb_pk / exact slab, global / packed Perlin).  The host flags the hook
returns say that each batch took the form it was built for."""
import numpy as np
import pytest

import ops_cases
import pyoracle
import rtamd
from rtamd._lib import debug_eval_op

pytestmark = pytest.mark.gpu

# output words per op: (the classification words, the value words that count where word 0 is 1)
WORDS = {"sphere": ([0], [1]), "medium_sphere": ([0], [1, 2]), "quad": ([0], [1, 2, 3]), "box": ([0], [1, 2, 3, 4]),
         "node": ([0], []), "perlin": ([0], []), "sphere_uv": ([0, 1], []), "texture": ([0, 1, 2], [])}


def _same(a, b):
    """Equal words, or NaN on both sides (NaNs stick, their payload is not pinned)."""
    fa, fb = a.view(np.float32), b.view(np.float32)
    return (a == b) | (np.isnan(fa) & np.isnan(fb))


def _check(batch, form, got, want, rows=None):
    always, on_hit = WORDS[batch.op]
    sel = np.ones(len(want), bool) if rows is None else rows
    for k in always:
        bad = sel & ~_same(got[:, k], want[:, k])
        assert not bad.any(), (f"{batch!r} form {form}: word {k} differs at rows {np.nonzero(bad)[0][:8]}: "
                               f"{got[bad][:4, k]} vs oracle {want[bad][:4, k]}")
    hit = sel & (want[:, 0] == 1)
    for k in on_hit:
        same = _same(got[:, k], want[:, k])
        if batch.op == "box" and form >= 2 and k >= 3:
            # the compact record rebuilds a face's system up to the sign of its zeros, which can only turn a zero
            # alpha or beta into the zero of the other sign (rt_kernel_common.h boxc_face): +-0 are one value here
            same |= ((got[:, k] | want[:, k]) & 0x7FFFFFFF) == 0
        bad = hit & ~same
        assert not bad.any(), (f"{batch!r} form {form}: word {k} differs on hits at rows {np.nonzero(bad)[0][:8]}: "
                               f"{got[bad][:4, k].view(np.float32)} vs oracle {want[bad][:4, k].view(np.float32)}")


def _forms(batch, flags):
    """The device forms valid for the batch, each with the rows it is defined on (None: all)."""
    fd = flags[0] == 1
    op = batch.op
    if op == "sphere":
        return [(0, None), (2, None)] + ([(1, None), (3, None)] if fd else [])
    if op in ("medium_sphere", "quad"):
        return [(0, None)] + ([(1, None)] if fd else [])
    if op == "box":
        f = [(0, None)] + ([(1, None)] if fd else [])
        if flags[1] == len(batch.rows):
            f += [(2, None)] + ([(3, None), (4, None)] if fd else [])
        return f
    if op == "node":
        # aabb_fast / aabb_pk are the walk's forms for rays without a -inf in 1 / d (the others take the slab form)
        with np.errstate(divide="ignore", over="ignore"):
            ok = ~(np.float32(1.0) / batch.rows[:, 3:6] == -np.inf).any(axis=1)
        return [(0, ok), (1, ok), (2, None)]
    if op == "perlin":
        return [(0, None)] + ([(1, None)] if flags[1] else [])
    return [(0, None)]


@pytest.mark.parametrize("name", list(ops_cases.ALL))
def test_device_forms_equal_the_oracle(gpu, name):
    for b in ops_cases.ALL[name]():
        op = pyoracle.OPS[b.op]
        want = pyoracle.eval_op(b.op, b.rows, b.recs, b.tex)
        _, flags = debug_eval_op(op, 0, b.rows, b.recs, b.tex, device=-1, lib=gpu)
        # the batch is what it was built to be: in or out of the shared-reciprocal regime, compact or not, and
        # with the rows outside the sphere forms' wave-wide regime where they were put
        if b.fd is not None:
            assert flags[0] == b.fd, (b, flags)
        if b.compact is not None:
            assert (flags[1] == (len(b.rows) if b.op == "box" else 1)) == b.compact, (b, flags)
        if b.out_rows is not None:
            assert flags[3] == b.out_rows, (b, flags)
            if b.name == "one_lane_out":
                assert flags[2] == len(b.rows) // 64 == b.out_rows   # one such lane in every wave
        if b.delta is not None:
            # a quad / box wave with one lane's numerator non-zero and below 2^-100 (the hook sees no numerators:
            # computed from the rows), the other 63 far inside the regime
            out = ops_cases.lanes_out_of_regime(b).reshape(-1, 64)
            assert (out.sum(axis=1) == 1).all() and out[:, 17].all() and (want[:, 0] == 1).all(), b
        forms = _forms(b, flags)
        if b.delta is not None:
            assert [f for f, _ in forms] == ([0, 1, 2, 3, 4] if b.op == "box" else [0, 1]), (b, forms)
        if b.kind == "random" and b.fd:
            assert len(forms) > 1, (b, "the fd form must run on the random set")
        for form, rows in forms:
            got, _ = debug_eval_op(op, form, b.rows, b.recs, b.tex, device=0, lib=gpu)
            _check(b, form, got, want, rows)


def test_forms_the_records_do_not_allow_are_refused(gpu):
    """A compact form on a box that is not compact, and the packed Perlin form on a table that does not pack."""
    b = [x for x in ops_cases.box_batches() if x.name == "rotated_edges"][0]
    with pytest.raises(rtamd.RTError):
        debug_eval_op(pyoracle.OPS["box"], 2, b.rows, b.recs, device=0, lib=gpu)
    p = [x for x in ops_cases.perlin_batches() if x.name == "unpackable"][0]
    with pytest.raises(rtamd.RTError):
        debug_eval_op(pyoracle.OPS["perlin"], 1, p.rows, tex=p.tex, device=0, lib=gpu)

"""Shading parity: light sampling over several lights (a moving sphere light among them), a shading point
inside a light sphere (NaN, Q11), the media tables in LDS and in global memory, a box-bounded medium among
compact boxes, stale uv under an image-textured medium (Q9, uv_always) and the checker / Perlin / image /
moving-sphere texture paths (tests/adversarial.py shading_cases), through the C ABI, bit for bit against the
CPU oracle -- with the default options and with each of shade_lds, fastdiv, compact_boxes, leaf_prefetch,
sphere_pairs, zero_dir_end and perlin_packed off.  Each case's launch path is asserted."""
import numpy as np
import pytest

import adversarial
import pyoracle
import rtamd
from helpers import bit_equal, mismatch_report
from test_gpu_adversarial import oracle, render
from test_shading_cases_design import launch_facts

pytestmark = pytest.mark.gpu

CASES = adversarial.shading_cases()
OFF = [{}, {"shade_lds": 0}, {"fastdiv": 0}, {"compact_boxes": 0}, {"leaf_prefetch": 0}, {"sphere_pairs": 0},
       {"zero_dir_end": 0}, {"perlin_packed": 0}]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_shading_case_matches_oracle(gpu, case):
    ref = oracle(case)
    launch_facts(case, lib=gpu)   # the host-side plan of the default launch takes the path the case is for
    for opts in OFF:
        out, info = render(case, opts)
        assert bit_equal(out, ref), f"{case.name} {opts or 'default'}: {mismatch_report(out, ref)}"
        if not opts:
            for k, v in case.expect.items():
                assert info[k] == v, f"{case.name}: launch {k} = {info[k]}, expected {v} ({info})"
    if case.name == "light_inside":
        assert np.isnan(ref).any() and np.array_equal(np.isnan(out), np.isnan(ref))

"""profiles/pass_blocks_resources_{parent,this}.txt: `make -C raytracing-book_amd resources` on the parent
commit and on the commit that added the per-pass trim of shade()'s mixture (rt_kernel_common.h
RT_PB_NOLIGHT).  The trim is compiled into the RT_OPT_BOXQ instantiations alone: every other render
kernel's report is the parent's, and those four keep the shape their speed depends on -- at most 128
VGPRs, no spilled register, no scratch, 4 waves per SIMD, no static LDS.  (No GPU needed.)
"""
import os

from test_adaptive_host import FIELDS, render_instances
from test_walk_trim_resources import BOXQ, opt_of

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILES = os.path.join(REPO, "profiles")


def test_only_the_boxq_kernels_changed():
    a = render_instances(open(os.path.join(PROFILES, "pass_blocks_resources_parent.txt")).read())
    b = render_instances(open(os.path.join(PROFILES, "pass_blocks_resources_this.txt")).read())
    assert len(a) == 56 and set(a) == set(b)
    boxq = [k for k in a if opt_of(k) & BOXQ]
    assert len(boxq) == 4                                      # 512 and 1024 threads, each with its mask twin
    for k in a:
        if k in boxq:
            continue
        for f in FIELDS:
            assert a[k][f] == b[k][f], (k, f, a[k][f], b[k][f])
    for k in boxq:
        r = b[k]
        assert int(r["VGPRs"]) <= 128, (k, r)
        assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (k, r)
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["LDS Size [bytes/block]"]) == 0, (k, r)
        assert int(r["Occupancy [waves/SIMD]"]) == 4, (k, r)


def test_the_parent_report_is_the_previous_change_s_result():
    """The parent of this change is the commit profiles/first_leaf_resources_this.txt reports."""
    a = render_instances(open(os.path.join(PROFILES, "pass_blocks_resources_parent.txt")).read())
    b = render_instances(open(os.path.join(PROFILES, "first_leaf_resources_this.txt")).read())
    assert a == b

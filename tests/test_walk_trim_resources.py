"""profiles/walk_trim_resources_{parent,this}.txt: `make -C raytracing-book_amd resources` on the parent
commit and on the commit that trimmed the scene-8 kernels (rt_kernel_common.h RT_WT_*).  The trimmed code
is compiled into the RT_OPT_BOXQ instantiations alone: every other render kernel's report is the parent's,
and the trimmed ones keep the shape their speed depends on -- at most 128 VGPRs, no spilled register, no
scratch, 4 waves per SIMD, no static LDS.  (No GPU needed.)
"""
import os
import re

from test_adaptive_host import FIELDS, render_instances

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILES = os.path.join(REPO, "profiles")
BOXQ = 256


def opt_of(name):
    m = re.search(r"render_persistentILi4ELb0ELi(\d+)ELi(\d+)EEEvPK", name)
    assert m, name
    return int(m.group(2))


def test_only_the_trimmed_kernels_changed():
    a = render_instances(open(os.path.join(PROFILES, "walk_trim_resources_parent.txt")).read())
    b = render_instances(open(os.path.join(PROFILES, "walk_trim_resources_this.txt")).read())
    assert len(a) == 56 and set(a) == set(b)
    trimmed = [k for k in a if opt_of(k) & BOXQ]
    assert len(trimmed) == 4                                   # 512 and 1024 threads, each with its mask twin
    for k in a:
        if k in trimmed:
            continue
        for f in FIELDS:
            assert a[k][f] == b[k][f], (k, f, a[k][f], b[k][f])
    for k in trimmed:
        r = b[k]
        assert int(r["VGPRs"]) <= 128, (k, r)
        assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (k, r)
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["LDS Size [bytes/block]"]) == 0, (k, r)
        assert int(r["Occupancy [waves/SIMD]"]) == 4, (k, r)

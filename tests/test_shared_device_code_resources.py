"""profiles/shared_device_code_resources_{parent,this}.txt: `make -C raytracing-book_amd resources` on the
parent commit and on the commit that made the hit record, the uv hand-over and the pixel base shared
helpers (rt_kernel_common.h hit_surface, walk_uv, pixel_base) and split rt_kernel_launch.h off, folded to
one line per kernel (tools/fold_resources.py).  A refactor: all 56 render kernels keep every field of the
parent's report, and the off-path kernels that call the helpers (first-hit pass, op-by-op evaluators)
keep their registers, spills and scratch.  profiles/shared_device_code_isa.txt holds the instruction
comparison (tools/isa_compare.py): no function's instruction count or opcode histogram moved.
(No GPU needed.)
"""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILES = os.path.join(REPO, "profiles")
FIELDS = ("vgprs", "vgpr_spill", "sgpr_spill", "scratch", "lds", "occupancy")
OFF_PATH = ("features_kernel", "eval_op_kernel", "eval_shade_op_kernel")


def report(name):
    """{kernel: {field: value}} of a folded report."""
    out = {}
    for ln in open(os.path.join(PROFILES, f"shared_device_code_resources_{name}.txt")):
        if ln.strip() and not ln.startswith("#"):
            kernel, *fields = ln.split()
            out[kernel] = dict(f.split("=") for f in fields)
            assert set(out[kernel]) == set(FIELDS), ln
    return out


def test_every_render_kernel_keeps_its_resources():
    a, b = report("parent"), report("this")
    ra, rb = ({k: v for k, v in r.items() if "render_persistent" in k} for r in (a, b))
    assert len(ra) == 56 and set(ra) == set(rb)
    for k in ra:
        for f in FIELDS:
            assert ra[k][f] == rb[k][f], (k, f, ra[k][f], rb[k][f])


def test_off_path_kernels_keep_registers_spills_and_scratch():
    a, b = report("parent"), report("this")
    for name in OFF_PATH:
        ka = [k for k in a if name in k]
        assert len(ka) == 1 and ka[0] in b, (name, ka)
        for f in ("vgprs", "vgpr_spill", "sgpr_spill", "scratch"):
            assert a[ka[0]][f] == b[ka[0]][f], (name, f, a[ka[0]][f], b[ka[0]][f])


def test_ab_library_report_is_recorded():
    """The A/B units' report (-DRT_AB_KNOBS), equal on both commits and so recorded once."""
    r = report("ab")
    assert len(r) == 120 and sum("render_persistent_ab" in k for k in r) > 0


def test_no_function_changed_its_instruction_count_or_histogram():
    """The recorded tools/isa_compare.py runs: release rt_kernel.s, then the A/B library's two units."""
    text = open(os.path.join(PROFILES, "shared_device_code_isa.txt")).read()
    totals = re.findall(r"^functions (\d+) differing_in_count_or_histogram (\d+)$", text, re.M)
    assert len(totals) == 3 and int(totals[0][0]) == 61
    assert all(int(d) == 0 for _, d in totals), totals
    rows = re.findall(r"^\S+ insts (\d+) (\d+) opcodes (\d+) (\d+) histogram_delta (\d+) ", text, re.M)
    assert len(rows) == 61
    for r in rows:
        assert r[0] == r[1] and r[2] == r[3] and r[4] == "0", r

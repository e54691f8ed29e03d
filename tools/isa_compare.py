"""Per-function instruction count and opcode histogram of two device-only assembly files of the same
source (make asm), and how many functions differ in either; then, for the functions whose counts and
histograms agree, how many instruction lines still differ (register names, operand order).

usage: python tools/isa_compare.py A.s B.s
"""
import collections
import re
import sys


def functions(path):
    """{function: [instruction lines]} -- the lines between a function's label and its .Lfunc_end."""
    funcs, cur, names = {}, None, set()
    for line in open(path):
        t = re.match(r"^\s*\.type\s+([\w$.]+),@function", line)
        if t:
            names.add(t.group(1))
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and m.group(1) in names:
            cur = funcs.setdefault(m.group(1), [])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            s = line.split(";")[0].strip()
            if s and not s.startswith(".") and not s.endswith(":"):
                cur.append(s)
    return {k: v for k, v in funcs.items() if v}


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    differ = 0
    for name in sorted(set(a) | set(b)):
        ia, ib = a.get(name, []), b.get(name, [])
        ha, hb = (collections.Counter(s.split()[0] for s in x) for x in (ia, ib))
        same = len(ia) == len(ib) and ha == hb
        differ += not same
        lines = sum(x != y for x, y in zip(ia, ib)) if same else -1
        ops = sum((ha - hb).values()) + sum((hb - ha).values())
        print(f"{name} insts {len(ia)} {len(ib)} opcodes {len(ha)} {len(hb)} histogram_delta {ops} "
              f"lines_differing {lines if same else 'n/a'}")
    print(f"functions {len(set(a) | set(b))} differing_in_count_or_histogram {differ}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())

"""`make -C raytracing-book_amd resources` output on stdin -> one line per kernel on stdout:
its name, then VGPRs, VGPRs Spill, SGPRs Spill, ScratchSize, LDS Size and Occupancy as field=value.

usage: make -s -C raytracing-book_amd resources | python tools/fold_resources.py
"""
import re
import sys

FIELDS = {"VGPRs": "vgprs", "VGPRs Spill": "vgpr_spill", "SGPRs Spill": "sgpr_spill", "ScratchSize [bytes/lane]": "scratch",
          "LDS Size [bytes/block]": "lds", "Occupancy [waves/SIMD]": "occupancy"}

rows = {}
for ln in sys.stdin:
    m = re.search(r"Function Name: (\S+)", ln)
    if m:
        cur = rows.setdefault(m.group(1), {})
        continue
    m = re.search(r"remark:\s+([A-Za-z][\w \[\]/-]*?): (\S+)", ln)
    if m and m.group(1) in FIELDS:
        cur[FIELDS[m.group(1)]] = m.group(2)
for name, r in rows.items():
    print(name, " ".join(f"{k}={r[k]}" for k in FIELDS.values()))

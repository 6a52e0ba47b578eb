#!/usr/bin/env python3
"""VGPRs / VGPR spills / scratch per k_trace variant from a
`-Rpass-analysis=kernel-resource-usage` remark stream on stdin: the depth-8 variants,
named by the TraceVariant arguments of their mangled names (trace_variant.hpp: the
family's number, Li8, then Lb0 / Lb1 for 5-word records and the material table in
LDS, t / i for 16- / 32-bit ids, Lb1 for NOEMIT).  With an argument, the kernels
whose mangled name contains it instead (e.g. `svgf` for post.hip's)."""
import re
import sys

only = sys.argv[1] if len(sys.argv) > 1 else None
cur, rows = None, {}
for line in sys.stdin:
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = m.group(1)
        rows[cur] = {}
        continue
    m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
    if m and cur:
        rows[cur][m.group(1).strip()] = int(m.group(2))
for k, v in rows.items():
    if only is not None:
        if only in k:
            print(f"{k[:60]:60s} VGPRs {v.get('VGPRs', 0):4d} spill {v.get('VGPRs Spill', 0):3d} "
                  f"scratch {v.get('ScratchSize', 0):5d} waves {v.get('Occupancy', 0)}")
    elif "k_trace" in k and "ELi8E" in k:
        print(f"{k.split('TraceFamilyE')[1][:24]:24s} VGPRs {v.get('VGPRs', 0):4d} spill {v.get('VGPRs Spill', 0):3d} "
              f"scratch {v.get('ScratchSize', 0):5d} waves {v.get('Occupancy', 0)}")

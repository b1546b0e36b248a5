#!/usr/bin/env python3
"""Summarise a rocprofv3 --kernel-trace CSV per (kernel, grid size): calls, average / min /
max duration, registers and LDS.  Grid size separates the launches of one kernel at different
problem sizes (e.g. the 1M-frame and the 2^26-frame biquad launches of bench.py), which the
stock --stats summary averages together.

    python tools/summarize_trace.py gpurun_out/prof/<pid>_kernel_trace.csv > profiles/<name>.md
    python tools/summarize_trace.py <csv> --intervals k_biquad_sine_runs     # start-to-start of consecutive launches

--intervals: for the launches of one kernel (substring of its name) at its most frequent grid, the time from one
launch's start to the next one's, where no other kernel ran in between -- a kernel's duration leaves out whatever the
boundary between two dependent launches costs (dispatch, the write-back of dirty cache lines)."""

import csv
import re
import sys
from collections import defaultdict


def short(name: str) -> str:
    name = name.replace("(anonymous namespace)::", "").replace("void ", "")
    return re.sub(r"\(.*\)$", "", name)


def main(path):
    groups = defaultdict(list)
    meta = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            key = (short(row["Kernel_Name"]), int(row["Grid_Size_X"]), int(row["Grid_Size_Y"]),
                   int(row["Grid_Size_Z"]), int(row["Workgroup_Size_X"]))
            groups[key].append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
            meta[key] = (row["VGPR_Count"], row["Accum_VGPR_Count"], row["SGPR_Count"], row["LDS_Block_Size"])
    total = sum(sum(v) for v in groups.values())
    print("| kernel | grid (threads) | wg | calls | avg us | min us | max us | total ms | % | vgpr | agpr | sgpr | lds B |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for key, v in sorted(groups.items(), key=lambda kv: -sum(kv[1])):
        name, gx, gy, gz, wg = key
        vg, ag, sg, lds = meta[key]
        print(f"| {name} | {gx}x{gy}x{gz} | {wg} | {len(v)} | {sum(v) / len(v) / 1e3:.2f} | "
              f"{min(v) / 1e3:.2f} | {max(v) / 1e3:.2f} | {sum(v) / 1e6:.3f} | {100.0 * sum(v) / total:.1f} | "
              f"{vg} | {ag} | {sg} | {lds} |")


def intervals(path, match):
    rows = []
    with open(path) as f:
        for row in csv.DictReader(f):
            rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), short(row["Kernel_Name"]),
                         int(row["Grid_Size_X"])))
    rows.sort()
    grids = defaultdict(int)
    for _, _, name, gx in rows:
        if match in name:
            grids[gx] += 1
    if not grids:
        print(f"no launch of a kernel matching {match}")
        return
    grid = max(grids, key=grids.get)
    s2s, dur, gap = [], [], []
    for a, b in zip(rows, rows[1:]):
        if match in a[2] and match in b[2] and a[3] == grid and b[3] == grid:
            s2s.append(b[0] - a[0])
            dur.append(a[1] - a[0])
            gap.append(b[0] - a[1])
    if not s2s:
        print(f"no two consecutive launches of {match} at grid {grid}")
        return
    # the stream's launches follow each other at once only while the host keeps up: the shorter half is the device's pace
    med = lambda v: sorted(v)[len(v) // 2] / 1e3
    print("| kernel | grid (threads) | pairs | start-to-start us: median | min | duration us: median | end-to-start us: median | min |")
    print("|---|---|---|---|---|---|---|---|")
    print(f"| {match} | {grid} | {len(s2s)} | {med(s2s):.2f} | {min(s2s) / 1e3:.2f} | {med(dur):.2f} | {med(gap):.2f} | "
          f"{min(gap) / 1e3:.2f} |")


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[2] == "--intervals":
        intervals(sys.argv[1], sys.argv[3])
    else:
        main(sys.argv[1])

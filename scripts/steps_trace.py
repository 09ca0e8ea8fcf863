"""usage: python scripts/steps_trace.py DIR   (DIR: a `rocprofv3 --kernel-trace --stats --output-format csv -d DIR` directory)

The figures profiles/steps_groups.txt records for a bench.py run: the fused first passes of the timed regions (the largest grid
of k_sample_lw_fast in the trace), their spacing start to start, their durations, how much consecutive ones overlap, the gap
between one's end and the next one's start where they do not, and the hard-row grids' (k_sample_hw) durations.  All in us.
"""

from __future__ import annotations

import csv
import glob
import os
import statistics
import sys


def q(v, p):
    v = sorted(v)
    return v[min(len(v) - 1, int(p * len(v)))] if v else float("nan")


def line(name, v):
    if not v:
        return f"  {name}: none"
    return f"  {name}: n {len(v)}, median {statistics.median(v):.2f}, p10 {q(v, 0.1):.2f}, p90 {q(v, 0.9):.2f}, min {min(v):.2f}, max {max(v):.2f}"


def main() -> None:
    files = glob.glob(os.path.join(sys.argv[1], "**", "*kernel_trace.csv"), recursive=True)
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            rows += list(csv.DictReader(fh))
    ks = [(r["Kernel_Name"], int(r["Start_Timestamp"]) / 1e3, int(r["End_Timestamp"]) / 1e3,
           int(r.get("Grid_Size") or r.get("Grid_Size_X") or 0)) for r in rows]
    ks.sort(key=lambda k: k[1])
    first = [k for k in ks if "k_sample_lw_fast" in k[0]]
    hard = [k for k in ks if "k_sample_hw" in k[0]]
    if not first:
        print("no k_sample_lw_fast in the trace")
        return
    # the timed regions' groups: the commonest duration class among the long kernels (groups of the --steps call)
    durs = [e - s for _, s, e, _ in first]
    big = statistics.median(sorted(durs)[len(durs) // 2:])
    grp = [k for k in first if (k[2] - k[1]) > 0.7 * big]
    print(f"{len(first)} first-pass kernels, {len(grp)} of them long groups (> 0.7 x {big:.1f} us); {len(hard)} hard-row grids")
    spacing, overlap, gap = [], [], []
    for a, b in zip(grp, grp[1:]):
        d = b[1] - a[1]
        if d > 3 * big:  # another timed region / call: not a neighbour
            continue
        spacing.append(d)
        (overlap if a[2] > b[1] else gap).append(abs(a[2] - b[1]))
    print(line("first pass, start to start", spacing))
    print(line("first pass, duration", [e - s for _, s, e, _ in grp]))
    print(line("overlap of consecutive first passes (next starts before this ends)", overlap))
    print(line("gap between consecutive first passes (next starts after this ends)", gap))
    t0, t1 = grp[0][1], grp[-1][2]
    hw = [e - s for _, s, e, _ in hard if t0 <= s <= t1 + 200]
    print(line("hard-row grid, duration (inside the long groups' span)", hw))
    names = {}
    for n, s, e, _ in ks:
        if t0 <= s <= t1 + 200:
            names.setdefault(n.split("(")[0][:70], []).append(e - s)
    tot = sum(sum(v) for v in names.values())
    for n, v in sorted(names.items(), key=lambda kv: -sum(kv[1]))[:6]:
        print(f"  {sum(v) / tot * 100:5.1f} %  {len(v):5d} x {statistics.median(v):8.2f} us  {n}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Per (kernel, blocks) launch counts and mean durations from a rocprofv3 kernel trace (`--kernel-trace --output-format csv`), over the
second half of the trace (the benchmark's timed steps, not its warm-up and set-up), with the summed kernel time.

    python3 tools/trace_by_grid.py <dir or *_kernel_trace.csv> [substring ...]

With substrings only the kernels whose name contains one of them are listed (the total still covers every kernel)."""
import collections
import csv
import glob
import os
import sys


def main():
    src = sys.argv[1]
    path = src if os.path.isfile(src) else sorted(glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True))[0]
    want = sys.argv[2:]
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    rows = rows[len(rows) // 2:]
    acc = collections.defaultdict(lambda: [0, 0.0])
    total = 0.0
    for r in rows:
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        blocks = int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"])) * max(1, int(r.get("Grid_Size_Y", 1) or 1)) * max(1, int(r.get("Grid_Size_Z", 1) or 1))
        a = acc[(r["Kernel_Name"], blocks)]
        a[0] += 1
        a[1] += us
        total += us
    print(f"{len(rows)} launches in the second half of the trace, {total / 1e3:.2f} ms of kernel time")
    print(f"{'kernel':62s} {'blocks':>6s} {'count':>6s} {'mean us':>9s} {'share':>6s}")
    for (name, blocks), (n, us) in sorted(acc.items(), key=lambda kv: -kv[1][1]):
        if want and not any(w in name for w in want):
            continue
        print(f"{name[:62]:62s} {blocks:6d} {n:6d} {us / n:9.2f} {100 * us / total:5.1f}%")


if __name__ == "__main__":
    main()

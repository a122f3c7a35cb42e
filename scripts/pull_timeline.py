#!/usr/bin/env python3
"""Where do the hub passes of a pull round run against its main pull kernel?

Reads a `rocprofv3 --kernel-trace --output-format csv` kernel trace and, for
the last K pull rounds with hubs (a round ends with its k_hub_final), prints
the intervals of the round's main pull kernel (k_expand*), its k_hub_partial
and its k_hub_final, in microseconds from the main kernel's start, and whether
the chunks' interval lies inside the main kernel's.
usage: pull_timeline.py <kernel_trace.csv> [K = 6]"""
import csv
import sys


def main():
    rows = []
    for r in csv.DictReader(open(sys.argv[1], newline="")):
        name = r["Kernel_Name"]
        short = name.split("(")[0].replace("void gp::", "").replace("gp::", "")
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short))
    rows.sort()
    last = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    finals = [i for i, r in enumerate(rows) if r[2].startswith("k_hub_final")]
    print("| round's main kernel | main µs | k_hub_partial [start, end] µs | k_hub_final [start, end] µs | chunks inside main | main start .. final end µs |")
    print("|---|---|---|---|---|---|")
    for i in finals[-last:]:
        f = rows[i]
        part = next((r for r in reversed(rows[:i]) if r[2].startswith("k_hub_partial")), None)
        mains = [r for r in rows if r[2].startswith("k_expand") and r[0] < f[0]]
        if not part or not mains:
            continue
        m = max(mains)
        t0 = m[0]
        us = lambda t: (t - t0) / 1e3
        inside = part[0] >= m[0] - 50_000 and part[1] <= m[1]   # (launched first: may start a few µs ahead)
        print(f"| `{m[2]}` | {us(m[1]):.1f} | `{part[2]}` [{us(part[0]):.1f}, {us(part[1]):.1f}] | "
              f"[{us(f[0]):.1f}, {us(f[1]):.1f}] | {'yes' if inside else 'no'} | {(f[1] - min(t0, part[0])) / 1e3:.1f} |")


if __name__ == "__main__":
    main()

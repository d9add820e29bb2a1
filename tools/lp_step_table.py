#!/usr/bin/env python
"""The kernels of ONE mini-batch link-prediction step from a rocprofv3 csv run of `lp_minibatch_probe.py --trace-step`
(--kernel-trace --marker-trace): the kernel dispatches inside the `lp_step` roctx range, as a markdown table (name,
calls, total and mean µs), in launch order of first appearance.

    python tools/lp_step_table.py TRACE_DIR [--out profiles/lp_minibatch_kernels.md]"""
import argparse
import collections
import csv
import glob
import os


def _rows(d, suffix):
    fs = glob.glob(os.path.join(d, "**", f"*{suffix}"), recursive=True)
    if not fs:
        raise SystemExit(f"no *{suffix} under {d}")
    with open(fs[0]) as f:
        return list(csv.DictReader(f))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace_dir")
    ap.add_argument("--out", default=os.path.join("profiles", "lp_minibatch_kernels.md"))
    a = ap.parse_args()
    marks = [r for r in _rows(a.trace_dir, "marker_api_trace.csv") if "lp_step" in r.get("Function", "")]
    if not marks:
        raise SystemExit("no lp_step range in the marker trace")
    t0 = min(int(r["Start_Timestamp"]) for r in marks)
    t1 = max(int(r["End_Timestamp"]) for r in marks)
    ks = [r for r in _rows(a.trace_dir, "kernel_trace.csv") if t0 <= int(r["Start_Timestamp"]) <= t1]
    ks.sort(key=lambda r: int(r["Start_Timestamp"]))
    agg = collections.OrderedDict()
    for r in ks:
        e = agg.setdefault(r["Kernel_Name"], [0, 0])
        e[0] += 1
        e[1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    busy = sum(v[1] for v in agg.values())
    lines = ["# One mini-batch link-prediction step (FB15k-237 shape, masked batch 3), kernels",
             "",
             "`rocprofv3 --kernel-trace --marker-trace` of `tools/lp_minibatch_probe.py --trace-step`: the dispatches "
             f"inside the step's roctx range. {len(ks)} kernels, {busy / 1e3:.1f} µs of kernel time in a "
             f"{(t1 - t0) / 1e3:.1f} µs range.",
             "",
             "| kernel | calls | total µs | mean µs |",
             "|---|---:|---:|---:|"]
    for name, (n, ns) in agg.items():
        short = name if len(name) <= 90 else name[:87] + "..."
        lines.append(f"| `{short}` | {n} | {ns / 1e3:.1f} | {ns / 1e3 / n:.1f} |")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()

"""Per-kernel dispatch counts and median / min / max durations from the kernel trace of a profiler run (dev tool): reads every
*kernel_trace.csv under the directory given (rocprofv3 --kernel-trace -f csv -d DIR: columns Kernel_Name, Start_Timestamp, End_Timestamp in
ns) and prints one line per kernel, the largest total first.  profiles/expr_filter_prof.txt's first block is its output over a
`tools/prof_expr_filter.py --pass-only` run."""
import csv
import glob
import statistics
import sys

rows = {}
for path in glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(path)):
        rows.setdefault(r["Kernel_Name"], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
print("# kernel dispatches (kernel trace): name, dispatches, median / min / max ms")
for k, v in sorted(rows.items(), key=lambda kv: -sum(kv[1])):
    print(f"{k[:60]:60s} n {len(v):4d}  median_ms {statistics.median(v):9.4f}  min_ms {min(v):9.4f}  max_ms {max(v):9.4f}")

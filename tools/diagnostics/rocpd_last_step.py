"""The kernel table of ONE training step from a rocprofv3 (--kernel-trace --stats) database of a `bench.py` run: the dispatches from the
first `build_x` launch of the last step's rollout (T of them per step) to the end of the trace (its optimizer launches included),
aggregated by kernel name (Name, Calls, TotalDurationUs, AverageUs, Percentage) -- the per-process `top_kernels` view also counts the
setup / warm-up steps and the parameter initialisation.
usage: python tools/diagnostics/rocpd_last_step.py <results.db> <out.csv> <T>"""
import csv
import sqlite3
import sys
from collections import OrderedDict

db, out, T = sys.argv[1], sys.argv[2], int(sys.argv[3])
con = sqlite3.connect(db)
ks = con.execute("select name, duration from kernels order by start").fetchall()
marks = [i for i, k in enumerate(ks) if "build_x_flat_kernel" in k[0] or "build_x_kernel" in k[0]]
if len(marks) < T:
    sys.exit("fewer build_x launches than one step has")
agg = OrderedDict()
for name, dur in ks[marks[-T]:]:
    c, t = agg.get(name, (0, 0))
    agg[name] = (c + 1, t + dur)
total = sum(t for _, t in agg.values())
with open(out, "w", newline="") as f:
    w = csv.writer(f)
    w.writerow(["Name", "Calls", "TotalDurationUs", "AverageUs", "Percentage"])
    for name, (c, t) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        w.writerow([name, c, round(t / 1e3, 1), round(t / c / 1e3, 1), round(100.0 * t / total, 3)])
native = sum(t for n, (c, t) in agg.items() if "p4c::" in n)
print(f"{sum(c for c, _ in agg.values())} dispatches, {total / 1e6:.2f} ms of kernel time, p4c share {native / total:.3f} -> {out}")

"""Dev tool: per-leg kernel statistics of a `rocprofv3 --kernel-trace -d DIR -o half -- python tools/bench_half.py ...` run, read
from the rocpd database it writes, restricted to each leg's timed phase (its first float32 batch onwards: the float16 sweep is
left out, so both indexes count the same calls).  Legs start at the ground-truth GEMM that follows the previous leg's idle gap.

  python tools/summarize_half_trace.py DIR/half_results.db out.csv [--legs sift,glove,deep]"""
import csv
import sqlite3
import sys

db, out_path = sys.argv[1], sys.argv[2]
names = (sys.argv[sys.argv.index("--legs") + 1] if "--legs" in sys.argv else "sift,glove,deep").split(",")
ks = list(sqlite3.connect(db).execute("select name, start, end, duration, lds_size, vgpr_count, grid_x, workgroup_x from kernels order by start"))
cuts = [0] + [i + 1 for i in range(len(ks) - 1) if ks[i + 1][0].startswith("Cijk") and ks[i + 1][1] - ks[i][2] > 2e9] + [len(ks)]
legs = [ks[cuts[j]:cuts[j + 1]] for j in range(len(cuts) - 1)]
assert len(legs) == len(names), (len(legs), names)
rows = []
for name, L in zip(names, legs):
    first32 = min(i for i, k in enumerate(L) if "dt_f32::k_search" in k[0])
    agg = {}
    for k in L[first32:]:
        if not any(s in k[0] for s in ("k_search", "k_brute", "k_finalize", "k_route")):
            continue
        a = agg.setdefault(k[0], [0, 0.0, 1e18, 0, k[5], k[4], k[6] // k[7]])
        a[0] += 1
        a[1] += k[3]
        a[2] = min(a[2], k[3])
        a[3] = max(a[3], k[3])
    for n, (cnt, tot, mn, mx, vg, lds, wg) in sorted(agg.items()):
        rows.append(dict(leg=name, kernel=n, dispatches=cnt, total_us=round(tot / 1e3, 1), mean_us=round(tot / cnt / 1e3, 1),
                         min_us=round(mn / 1e3, 1), max_us=round(mx / 1e3, 1), vgpr=vg, lds_bytes=lds, workgroups=wg))
with open(out_path, "w", newline="") as f:
    w = csv.DictWriter(f, fieldnames=list(rows[0]))
    w.writeheader()
    w.writerows(rows)

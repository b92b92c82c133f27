"""Exact windows on the headline tree index (`set_exact_windows`): the doubling graph search against the exact scan
(k_brute) and the dense path (window / cover groups on the matrix cores) for the SAME batches of one index.
  set      bench.py's headline workload (make_data: 10^6 x 128 SIFT-like rows, distinct labels), VamanaRangeFilterTreeIndex
           <Float | Float16 | UInt8>Euclidian (--dtype; the same rows rounded / as bytes), cutoff 1000, split 2, R = 64, L = 500;
           10 000 queries, k = 10, "optimized_postfilter"
  windows  drawn as bench.py draws them (make_windows, the per-fraction seed 2000 + p), fractions 2^-11 .. 2^-2 (--fractions), each at
           the (beam, multiplier) profiles/r06_bench_n1.json records as that fraction's best setting (--settings)
  legs     off    the option off (limit 0): the graph search
           scan   limit = the window size, WANN_NO_GEMM=1: every query is one exact scan
           dense  limit = the window size: the dense path takes what its gates let it take, the scan the rest
           idle   limit = 1 024 where the windows are wider: no query is flagged, the dense launches run empty (what the option
                  costs a batch it does nothing for)
           alternately on ONE index, each leg twice; per leg the median of 21 device-buffer calls (device ms from HIP events =
           counters()["device_ms"], wall beside it), recall@10 against exact ground truth, and the exact-window counters
The switches are flipped between calls, so the tool runs with WANN_TEST_HOOKS=1 (both builds alike).
On a build without the option (a checkout of the parent commit) only the off leg runs: that build on the same box in the same job is
the baseline -- run this file there first with --out, then here with --baseline <that json>; this tree's off leg is reported beside
it.  "exact wins" at a fraction: the slower run of the better exact leg beats the faster run of the parent's leg by more than any
leg's two runs differ.  `crossover`: the widest fraction up to which exact wins at every fraction from the narrowest on.
Run from the repo root.  Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

os.environ["WANN_TEST_HOOKS"] = "1"
os.environ.pop("WANN_NO_GEMM", None)
os.environ.pop("WANN_DENSE_ALWAYS", None)

import numpy as np  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--dtype", default="float32", choices=("float32", "float16", "uint8"))
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--nq", type=int, default=10_000)
ap.add_argument("--fractions", default="-11,-10,-9,-8,-7,-6,-5,-4,-3,-2")
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--settings", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "r06_bench_n1.json"),
                help="a bench.py --full line: per_fraction gives every fraction's (beam, multiplier)")
ap.add_argument("--out", default=None)
ap.add_argument("--baseline", default=None, help="JSON this tool wrote on the parent commit's build (same box, same job): the wins are taken against it")
args = ap.parse_args()

import torch  # noqa: E402
import rangefilteredann_amd  # noqa: E402,F401
import window_ann as wa  # noqa: E402
from bench import ground_truth, make_data, make_windows, recall_of  # noqa: E402

SFX = {"float32": "FloatEuclidian", "float16": "Float16Euclidian", "uint8": "UInt8Euclidian"}[args.dtype]
ELEM = {"float32": np.float32, "float16": np.float16, "uint8": np.uint8}[args.dtype]
n, d, nq, k = args.n, args.d, args.nq, 10
X32, Q32, labels = make_data(n, d, nq)
X, Q = X32.astype(ELEM), Q32.astype(ELEM)
ls = np.sort(labels)
t0 = time.time()
idx = getattr(wa, "VamanaRangeFilterTreeIndex" + SFX)(X, labels, cutoff=1000, split_factor=2, build_params=wa.BuildParams(64, 500, 1.0, ""))
build_s = time.time() - t0
has_option = hasattr(idx, "set_exact_windows")
dev = torch.device("cuda:0")
Xt = torch.from_numpy(X.astype(np.float32)).to(dev)  # (integer-valued rows: the float32 ground truth is exact for all three types)
x2 = (Xt * Xt).sum(1)
labt = torch.from_numpy(labels).to(dev)
Qt = torch.from_numpy(Q.astype(np.float32)).to(dev)
it, dt = torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev)
settings = json.load(open(args.settings))["per_fraction"]
MIN_DENSE = 1024  # kCoverMinWindow = kGroupMinWindow


def leg(name, Wt, qp, limit, gt, gcnt):
    if name == "scan":
        os.environ["WANN_NO_GEMM"] = "1"
    else:
        os.environ.pop("WANN_NO_GEMM", None)
    if has_option:
        idx.set_exact_windows(limit)

    def call():
        idx.batch_search_device(Qt.data_ptr(), Wt.data_ptr(), nq, 0, "optimized_postfilter", qp, it.data_ptr(), dt.data_ptr(), 0)
    for _ in range(2):
        call()
    wall, devms = [], []
    for _ in range(args.reps):
        t = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t) * 1e3)
        devms.append(idx.counters()["device_ms"])
    c = idx.counters()
    r = dict(device_ms=round(float(np.median(devms)), 3), device_ms_min=round(min(devms), 3), device_ms_max=round(max(devms), 3),
             wall_ms=round(float(np.median(wall)), 3), recall_at_10=round(recall_of(torch, gt, gcnt, it), 4),
             beam_searches=int(c["beam_searches"]), brute_rows=int(c["brute_rows"]))
    if has_option:
        r["exact"] = {k_: int(v) for k_, v in idx.exact_window_counters().items()}
    return r, it.cpu().numpy().copy(), dt.cpu().numpy().view(np.uint32).copy()


base = json.load(open(args.baseline)) if args.baseline else None
out = dict(workload=f"VamanaRangeFilterTreeIndex{SFX} {n} x {d} (bench.py make_data), cutoff 1000, split 2, R 64, L 500; {nq} queries, distinct "
                    f"windows (bench.py make_windows), k = {k}, optimized_postfilter", has_option=has_option, timed_calls_per_leg=args.reps,
           build_s=round(build_s, 1), device_bytes=int(idx.device_bytes()), settings_from=os.path.basename(args.settings), fractions={})
for p in (int(x) for x in args.fractions.split(",")):
    W = make_windows(ls, nq, p, 2000 + p)
    Wt = torch.from_numpy(W).to(dev)
    gt, gcnt = ground_truth(torch, Xt, x2, labt, Qt, Wt, k)
    s = settings[f"2^{p}"]
    qp = wa.QueryParams(k, int(s["beam"]), 1.35, 10_000_000, 10_000, int(s["mult"]), 10000, None, False)
    w = max(1, int(n * 2.0 ** p))
    limit = w + 1  # (make_windows: labels_sorted[st] .. labels_sorted[st + w], both ends inside)
    names = ["off"] + (["scan", "dense"] + (["idle"] if w >= MIN_DENSE else []) if has_option else [])
    row = dict(window_points=w, beam=int(s["beam"]), mult=int(s["mult"]), limit=limit, legs={nm: [] for nm in names})
    rows_of = {}
    for _ in range(2):  # the legs alternate; each runs twice
        for nm in names:
            r, ids, dd = leg(nm, Wt, qp, {"off": 0, "scan": limit, "dense": limit, "idle": MIN_DENSE}[nm], gt, gcnt)
            row["legs"][nm].append(r)
            rows_of[nm] = (ids, dd)
    ms = {nm: [x["device_ms"] for x in row["legs"][nm]] for nm in names}
    row["spread_ms"] = {nm: round(abs(v[0] - v[1]), 3) for nm, v in ms.items()}
    if has_option:
        row["dense_rows_equal_scan_rows"] = bool(np.array_equal(rows_of["scan"][0], rows_of["dense"][0]) and np.array_equal(rows_of["scan"][1], rows_of["dense"][1]))
        if "idle" in names:
            row["idle_rows_equal_off_rows"] = bool(np.array_equal(rows_of["off"][0], rows_of["idle"][0]) and np.array_equal(rows_of["off"][1], rows_of["idle"][1]))
            row["idle_minus_off_ms"] = round(min(ms["idle"]) - min(ms["off"]), 3)
        if base and str(p) in base["fractions"]:
            pm = [x["device_ms"] for x in base["fractions"][str(p)]["legs"]["off"]]
            spread = max(list(row["spread_ms"].values()) + [abs(pm[0] - pm[1])])
            better = min(("scan", "dense"), key=lambda nm: max(ms[nm]))
            row["parent_off_ms"] = pm
            row["parent_recall_at_10"] = base["fractions"][str(p)]["legs"]["off"][0]["recall_at_10"]
            row["parent_and_this_tree_off_agree"] = bool(abs(min(pm) - min(ms["off"])) <= max(abs(pm[0] - pm[1]), row["spread_ms"]["off"], 0.01))
            row["better_exact_leg"] = better
            row["ratio_parent_over_exact"] = round(min(pm) / max(ms[better]), 2)
            row["exact_wins"] = bool(min(pm) - max(ms[better]) > spread)
    out["fractions"][str(p)] = row
    print(f"[bench_exact_windows] 2^{p}: " + json.dumps(row), file=sys.stderr, flush=True)
if has_option:
    idx.set_exact_windows(0)
    os.environ.pop("WANN_NO_GEMM", None)
    won = [p for p, r in sorted(((int(p_), r_) for p_, r_ in out["fractions"].items()))]
    cross = None
    for p in won:
        if not out["fractions"][str(p)].get("exact_wins"):
            break
        cross = p
    out["crossover"] = cross  # (None: no baseline given, or exact does not win at the narrowest fraction)
line = json.dumps(out)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
print(line)

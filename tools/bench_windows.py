"""PrefilterIndex batches of DISTINCT wide windows: the exact scan (k_brute, one wave per query) against the cover path of the
dense prefilter path (`set_dense_windows`: queries grouped by 2 048-position block, scored on the matrix cores).
  set      configs[1]-like: 10^6 x 128 SIFT-like rows (integer valued), distinct labels; --dtype float32 | float16 | uint8
           (the same rows rounded / as bytes), Euclidian; 10 000 queries
  windows  drawn like bench.py draws them (make_windows), fractions 2^-9 .. 2^0 (--fractions "-9,-6,-3,0")
  legs     option off and on ALTERNATELY, each leg twice, median of 21 device-buffer calls per leg (device time from HIP
           events = counters()["device_ms"], wall beside it), rows of the two legs compared bit for bit
On a build without the option (a checkout of the parent commit) only the scan legs run: that build on the same box is the
baseline of every ratio, this tree's option-off leg is reported beside it (--baseline <json of the parent's run> merges them).
--sweep: the crossover instead of the fractions -- batches of nq queries whose windows of w positions start uniformly in a
stretch of the label order sized so that about q windows touch every 2 048-position block (nq x w / q positions, at most n):
nq in 32 .. 10 000, w in 1 024 .. 65 536, q in 16 .. 512; scan against cover path, device ms, as above.
Kernel times: run this tool once more under `rocprofv3 --kernel-trace --stats` (a run of its own, never with --pmc) with
--fractions -3 --reps 3.  Run from the repo root.  Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--dtype", default="float32", choices=("float32", "float16", "uint8"))
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--nq", type=int, default=10_000)
ap.add_argument("--fractions", default="-9,-8,-7,-6,-5,-4,-3,-2,-1,0")
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--sweep", action="store_true")
ap.add_argument("--out", default=None)
ap.add_argument("--baseline", default=None, help="JSON this tool wrote on the parent commit's build (same box): ratios are taken against it")
args = ap.parse_args()

import torch  # noqa: E402
import rangefilteredann_amd  # noqa: E402,F401
import window_ann as wa  # noqa: E402
from bench import make_windows  # noqa: E402
from util import sift_like  # noqa: E402

CLASS = {"float32": "FloatEuclidian", "float16": "Float16Euclidian", "uint8": "UInt8Euclidian"}[args.dtype]
ELEM = {"float32": np.float32, "float16": np.float16, "uint8": np.uint8}[args.dtype]
n, d, nq, k = args.n, args.d, args.nq, 10
gen = sift_like(n, d, 3)
X, Q = gen(n).astype(ELEM), gen(nq).astype(ELEM)
rng = np.random.default_rng(4)
labels = ((rng.permutation(n) + 0.5) / n).astype(np.float32)
ls = np.sort(labels)
idx = getattr(wa, "PrefilterIndex" + CLASS)(X, labels)
has_option = hasattr(idx, "set_dense_windows")
qp = wa.QueryParams(k, 10, 1.35, 10**7, 10**4, 1, 10000, None, False)
dev = torch.device("cuda:0")
Qt = torch.from_numpy(Q.astype(np.float32)).to(dev)
it, dt = torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev)


def leg(Wt, on, reps):
    if has_option:
        idx.set_dense_windows(on)
    for _ in range(2):
        idx.batch_search_device(Qt.data_ptr(), Wt.data_ptr(), nq, 0, "", qp, it.data_ptr(), dt.data_ptr(), 0)
    wall, devms = [], []
    for _ in range(reps):
        t = time.perf_counter()
        idx.batch_search_device(Qt.data_ptr(), Wt.data_ptr(), nq, 0, "", qp, it.data_ptr(), dt.data_ptr(), 0)
        wall.append((time.perf_counter() - t) * 1e3)
        devms.append(idx.counters()["device_ms"])
    c = idx.counters()
    r = dict(device_ms=round(float(np.median(devms)), 3), device_ms_min=round(min(devms), 3), device_ms_max=round(max(devms), 3),
             wall_ms=round(float(np.median(wall)), 3), brute_rows=int(c["brute_rows"]), gemm_queries=int(c["gemm_queries"]))
    if has_option:
        r["cover"] = {k_: int(v) for k_, v in idx.dense_window_counters().items()}
    return r, it.cpu().numpy().copy(), dt.cpu().numpy().view(np.uint32).copy()


def emit(out):
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if args.sweep:
    out = dict(workload=f"{n} x {d} {args.dtype} Euclidian, windows of w positions, about q per 2 048-position block, k = {k}", timed_calls_per_leg=args.reps,
               cases=[])
    Q_all, it_all, dt_all = Qt, it, dt
    for nq_s in (32, 128, 512, 2048, 10000):
        for w in (1024, 2048, 8192, 65536):
            for q in (16, 32, 128, 512):
                if q > nq_s:
                    continue
                # a window of w positions touches about w / 2048 + 1 blocks: the stretch that gives q windows per block
                span = int(min(n - w - 2, max(2048, nq_s * (w + 2048) / q)))
                if nq_s * (w + 2048) / span < q * 0.9:
                    continue  # (the whole label order is too long for q windows per block)
                r = np.random.default_rng(nq_s + w + q)
                st = r.integers(1, span, size=nq_s)
                W = np.stack([ls[st], ls[st + w]], 1).astype(np.float32)
                Wt = torch.from_numpy(W).to(dev)
                nq, Qt, it, dt = nq_s, Q_all[:nq_s], it_all[:nq_s], dt_all[:nq_s]
                s0, ids0, d0 = leg(Wt, False, args.reps)
                c0, ids1, d1 = leg(Wt, True, args.reps)
                s1 = leg(Wt, False, args.reps)[0]
                c1 = leg(Wt, True, args.reps)[0]
                row = dict(nq=nq_s, w=w, q_per_block=q, scan_ms=[s0["device_ms"], s1["device_ms"]], cover_ms=[c0["device_ms"], c1["device_ms"]],
                           cover_queries=c0["cover"]["queries"], passes=c0["cover"]["passes"], unproven=c0["cover"]["unproven"],
                           rows_equal=bool(np.array_equal(ids0, ids1) and np.array_equal(d0, d1)))
                spread = max(abs(s0["device_ms"] - s1["device_ms"]), abs(c0["device_ms"] - c1["device_ms"]))
                row["cover_wins"] = bool(min(row["scan_ms"]) - max(row["cover_ms"]) > spread)
                out["cases"].append(row)
                print("[bench_windows] " + json.dumps(row), file=sys.stderr, flush=True)
    idx.set_dense_windows(False)
    emit(out)
    sys.exit(0)

base = json.load(open(args.baseline)) if args.baseline else None
out = dict(workload=f"{n} x {d} {args.dtype} Euclidian, {nq} queries, distinct windows (bench.py make_windows), k = {k}", has_option=has_option,
           timed_calls_per_leg=args.reps, fractions={})
for p in (int(x) for x in args.fractions.split(",")):
    W = make_windows(ls, nq, p, 1000 + p)
    Wt = torch.from_numpy(W).to(dev)
    # (a scan leg of seconds is not repeated 21 times: at most ~20 s per leg)
    first, ids0, d0 = leg(Wt, False, 1)
    reps = max(1, min(args.reps, int(20_000 / max(first["device_ms"], 1e-3))))
    row = dict(window_points=int(n * 2.0 ** p), reps=reps)
    scan = [leg(Wt, False, reps)[0]]
    if has_option:
        on1, ids1, d1 = leg(Wt, True, reps)
        scan.append(leg(Wt, False, reps)[0])
        on2 = leg(Wt, True, reps)[0]
        row["cover"] = [on1, on2]
        row["rows_equal"] = bool(np.array_equal(ids0, ids1) and np.array_equal(d0, d1))
    else:
        scan.append(leg(Wt, False, reps)[0])
    row["scan"] = scan
    s = [x["device_ms"] for x in scan]
    row["scan_spread_ms"] = round(abs(s[0] - s[1]), 3)
    if has_option:
        cv = [x["device_ms"] for x in row["cover"]]
        row["cover_spread_ms"] = round(abs(cv[0] - cv[1]), 3)
        row["ratio_this_tree_scan_over_cover"] = round(min(s) / min(cv), 2)
        if base and str(p) in base["fractions"]:
            ps = [x["device_ms"] for x in base["fractions"][str(p)]["scan"]]
            row["parent_scan_ms"] = ps
            row["ratio_parent_scan_over_cover"] = round(min(ps) / min(cv), 2)
            row["parent_and_this_tree_scan_agree"] = bool(abs(min(ps) - min(s)) <= max(abs(ps[0] - ps[1]), row["scan_spread_ms"], 0.01))
    out["fractions"][str(p)] = row
    print(f"[bench_windows] 2^{p}: " + json.dumps(row), file=sys.stderr, flush=True)
if has_option:
    idx.set_dense_windows(False)
emit(out)

"""Dev tool: what wann_set_dense_window_norms costs and gains on tools/bench_prefilter.py's adversarial shape (100 clusters of 10 000
unit rows, d = 100, float32, squared L2, 99 queries per cluster, window = the cluster, k = 10):
  outlier     257 more rows at the END of the label order, in no window, the last of them of norm 2^30 (256 positions behind the last
              window) -- the index's largest norm is its, and without the switch no proof settles: every query ends in the scan
  no_outlier  the same set with that row at unit norm -- the price of the table lookup
Legs per set, one index, one process, alternating: off, on, off, on; a leg is 3 warm-up calls + WANN_PF_REPS (21) timed ones, device
time from the HIP events round the batch (counters()["device_ms"]) and the host clock round the synchronising call.  Ids and
distance bits of every leg are compared with the first.  `first_on_call_ms` is the first call with the switch on less the leg's
median: the one-time build of the table (wall; it includes whatever else a first call pays).
On a build without the switch (a checkout of the parent commit) the off legs alone run: that build in the same job is the baseline
-- run this file there first with --out, then here with --baseline <that json>.  "on wins": with the outlier the slower on leg beats
the faster run of the parent's call by more than any leg's two runs differ.  Run from the repo root; prints one JSON object."""
import argparse, json, os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, REPO)
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--baseline", default=None, help="JSON this tool wrote on the parent commit's build (same box, same job)")
args = ap.parse_args()
import torch
import window_ann as wa

NCLU, PER, D, K, REPS = 100, 10000, 100, 10, int(os.environ.get("WANN_PF_REPS", "21"))
rng = np.random.default_rng(0)
cent = rng.standard_normal((NCLU, D)).astype(np.float32)
X = cent[np.repeat(np.arange(NCLU), PER)] + 0.1 * rng.standard_normal((NCLU * PER, D)).astype(np.float32)
X /= np.linalg.norm(X, axis=1, keepdims=True)
labels = (np.repeat(np.arange(NCLU), PER) - 0.5 + rng.random(NCLU * PER)).astype(np.float32)
PAD = 256  # rows no window holds between the last window and the extra row (the last of the label order)
X = np.concatenate([X, X[:PAD + 1]])
labels = np.concatenate([labels, (NCLU + 0.6 + 0.001 * np.arange(PAD + 1)).astype(np.float32)])
qc = np.repeat(np.arange(NCLU), 99)
Q = cent[(qc + 1 + rng.integers(0, NCLU - 1, qc.size)) % NCLU] + 0.1 * rng.standard_normal((qc.size, D)).astype(np.float32)
Q /= np.linalg.norm(Q, axis=1, keepdims=True)
W = np.stack([qc - 0.5, qc + 0.5], 1).astype(np.float32)
nq, dev = len(Q), torch.device("cuda:0")
qp = wa.QueryParams(K, K, 1.35, 10**7, 10**4, 1, 10000, None, False)
Qt, Wt = torch.from_numpy(Q).to(dev), torch.from_numpy(W).to(dev)
it, dt = torch.empty((nq, K), dtype=torch.int32, device=dev), torch.empty((nq, K), dtype=torch.float32, device=dev)
HAS = hasattr(wa.PrefilterIndexFloatEuclidian, "set_dense_window_norms")


def legs(outlier, order):
    Xs = X.copy()
    if outlier:
        Xs[-1] *= np.float32(2.0 ** 30)
    idx = wa.PrefilterIndexFloatEuclidian(Xs, labels)
    out, first = [], None
    for on in order:
        if HAS:
            assert idx.set_dense_window_norms(on) is on
        wall, devms = [], []
        for r in range(3 + REPS):
            t = time.perf_counter()
            idx.batch_search_device(Qt.data_ptr(), Wt.data_ptr(), nq, 0, "", qp, it.data_ptr(), dt.data_ptr(), 0)  # (synchronises)
            if r == 0:
                first_ms = (time.perf_counter() - t) * 1e3
            if r >= 3:
                wall.append((time.perf_counter() - t) * 1e3)
                devms.append(idx.counters()["device_ms"])
        c = idx.counters()
        rows = (it.cpu().numpy().copy(), dt.cpu().numpy().view(np.uint32).copy())
        first = first or rows
        out.append(dict(window_norms=on, device_ms_median=round(float(np.median(devms)), 4), device_ms_min=round(min(devms), 4), device_ms_max=round(max(devms), 4),
                        wall_ms_median=round(float(np.median(wall)), 4), first_call_ms=round(first_ms, 4), gemm_queries=int(c["gemm_queries"]),
                        gemm_unproven=int(c["gemm_unproven"]), gemm_rescued=int(c["gemm_rescued"]),
                        rows_equal_first_leg=bool(np.array_equal(rows[0], first[0]) and np.array_equal(rows[1], first[1]))))
    return out


order = [False, True, False, True] if HAS else [False, False]
res = dict(workload=f"adversarial {NCLU}x{PER} + 1 row, d={D} float32 Euclidian, {nq} queries, window = 1 cluster, k = {K}", has_switch=HAS,
           legs="wann_set_dense_window_norms off / on, alternating, one index per set, one process" if HAS else "the build has no switch: two off legs",
           timed_calls_per_leg=REPS, outlier=legs(True, order), no_outlier=legs(False, order))
if HAS:
    on1 = next(l for l in res["outlier"] if l["window_norms"])
    res["first_on_call_ms_less_median"] = round(on1["first_call_ms"] - on1["wall_ms_median"], 4)
if args.baseline:
    base = json.load(open(args.baseline))
    res["parent"] = dict(outlier=base["outlier"], no_outlier=base["no_outlier"])
    med = lambda ls: [l["device_ms_median"] for l in ls]
    on, off, par = med([l for l in res["outlier"] if l["window_norms"]]), med([l for l in res["outlier"] if not l["window_norms"]]), med(base["outlier"])
    spread = max(max(x) - min(x) for x in (on, off, par))
    res["outlier_summary"] = dict(on_ms=on, off_ms=off, parent_ms=par, largest_spread_of_a_leg_ms=round(spread, 4), on_wins=bool(min(par) - max(on) > spread))
print(json.dumps(res))
if args.out:
    json.dump(res, open(args.out, "w"), indent=1)

"""Dev tool: what wann_set_dense_centred costs and gains on tools/bench_prefilter.py's adversarial shape (100 clusters of 10 000 unit
rows, d = 100 or --d D, float32, squared L2, 99 queries per cluster, window = the cluster, k = 10), with mu added to rows and queries:
  mu = 0   data that does not need centring -- the price of the subtraction,
  mu = 64  a common offset no uncentred proof settles -- the switch off is the parent commit's call: every query ends in the scan.
Legs per mu, one index, one process, alternating: off, on, off, on; a leg is 3 warm-up calls + WANN_PF_REPS (21) timed ones, device
time from the HIP events round the batch (counters()["device_ms"]) and the host clock round the synchronising call.  Ids and
distance bits of every leg are compared with the first.  WANN_PF_ONLY=on / off runs mu = 0 with that setting alone (for a kernel
trace: the score kernel's time per launch).  --legs off,off: other legs than off,on,off,on (a build without the kernel under test as
the reference of the same job).  Run from the repo root; prints one JSON object."""
import argparse, json, os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, REPO)
import torch
import window_ann as wa

ap = argparse.ArgumentParser()
ap.add_argument("--d", type=int, default=100)
ap.add_argument("--legs", default="off,on,off,on")
args = ap.parse_args()
NCLU, PER, D, K, REPS = 100, 10000, args.d, 10, int(os.environ.get("WANN_PF_REPS", "21"))
rng = np.random.default_rng(0)
cent = rng.standard_normal((NCLU, D)).astype(np.float32)
X = cent[np.repeat(np.arange(NCLU), PER)] + 0.1 * rng.standard_normal((NCLU * PER, D)).astype(np.float32)
X /= np.linalg.norm(X, axis=1, keepdims=True)
labels = (np.repeat(np.arange(NCLU), PER) - 0.5 + rng.random(NCLU * PER)).astype(np.float32)
qc = np.repeat(np.arange(NCLU), 99)
Q = cent[(qc + 1 + rng.integers(0, NCLU - 1, qc.size)) % NCLU] + 0.1 * rng.standard_normal((qc.size, D)).astype(np.float32)
Q /= np.linalg.norm(Q, axis=1, keepdims=True)
W = np.stack([qc - 0.5, qc + 0.5], 1).astype(np.float32)
nq, dev = len(Q), torch.device("cuda:0")
qp = wa.QueryParams(K, K, 1.35, 10**7, 10**4, 1, 10000, None, False)
Wt = torch.from_numpy(W).to(dev)
it, dt = torch.empty((nq, K), dtype=torch.int32, device=dev), torch.empty((nq, K), dtype=torch.float32, device=dev)


def legs(mu, order):
    idx = wa.PrefilterIndexFloatEuclidian(X + np.float32(mu), labels)
    Qt = torch.from_numpy(Q + np.float32(mu)).to(dev)
    out, first = [], None
    for on in order:
        assert idx.set_dense_centred(on) is on
        wall, devms = [], []
        for r in range(3 + REPS):
            t = time.perf_counter()
            idx.batch_search_device(Qt.data_ptr(), Wt.data_ptr(), nq, 0, "", qp, it.data_ptr(), dt.data_ptr(), 0)  # (synchronises)
            if r >= 3:
                wall.append((time.perf_counter() - t) * 1e3)
                devms.append(idx.counters()["device_ms"])
        c = idx.counters()
        rows = (it.cpu().numpy().copy(), dt.cpu().numpy().view(np.uint32).copy())
        first = first or rows
        out.append(dict(centred=on, device_ms_median=round(float(np.median(devms)), 4), device_ms_min=round(min(devms), 4), device_ms_max=round(max(devms), 4),
                        wall_ms_median=round(float(np.median(wall)), 4), gemm_queries=int(c["gemm_queries"]), gemm_unproven=int(c["gemm_unproven"]),
                        gemm_rescued=int(c["gemm_rescued"]), rows_equal_first_leg=bool(np.array_equal(rows[0], first[0]) and np.array_equal(rows[1], first[1]))))
    return out


only = os.environ.get("WANN_PF_ONLY")
if only in ("on", "off"):
    print(json.dumps(dict(mu=0, calls=3 + REPS, leg=legs(0.0, [only == "on"])[0])))
    sys.exit(0)
order = [leg == "on" for leg in args.legs.split(",")]
res = {f"mu={mu:g}": legs(mu, order) for mu in (0.0, 64.0)}
print(json.dumps(dict(workload=f"adversarial {NCLU}x{PER} d={D} float32 Euclidian + mu, {nq} queries, window = 1 cluster, k = {K}",
                      legs=f"wann_set_dense_centred {args.legs}, one index per mu, one process", timed_calls_per_leg=REPS, **res)))

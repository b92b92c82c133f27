"""BASELINE.json configs[4]: adversarial-style data (100 clusters x 10 000 points, d = 100, unit norm, MIPS, 9 900 cross-cluster
queries; experiments/generate_advserial_dataset.py:8-69), PrefilterIndex brute force (src/prefiltering.h:154-204):
  (i)  native windows [c - 0.5, c + 0.5] = one cluster = 1 % of the points: dense MFMA path vs the exact per-query scan
  (ii) synthetic 2^-12 windows (244 points): the exact scan kernel k_brute against its HBM roofline
each against the REAL reference at its best thread count (child processes: the reference fixes its thread count at first use).
--dtype float32 | float16 | uint8 | int8 (default float32) selects the element type of the point set: float16 rounds the same
set (MIPS), the byte types quantise it -- round(127 x) for int8 (MIPS), + 128 for uint8 (Euclidian), queries likewise -- and run
on the int8 MFMA with exact scores.  Every leg is timed as the median of repeated calls (min / max beside it: the spread).
--dim D sets the row length (default 100; 512 = RedCaps, 768 / 1024 / 1536 = the long rows of k_gemm_scores_long (float32), k_gemm_scores_hslab (float16) and k_gemm_scores_bslab (uint8 / int8)), --clusters C
the number of clusters (default 100), --metric l2 | mips the metric of the float types (default mips).  WANN_PF_CACHE=<dir> keeps
the generated set there for the next run of the same shape; WANN_PF_ONLY=mfma times the dense leg alone (runs under a profiler),
WANN_PF_ONLY=scan the exact-scan leg alone, twice (the baseline run of a parent build); WANN_PF_NO_REF=1 leaves the CPU reference out.
--byte-exact: the float32 index is fed the integer values of the uint8 leg, round(127 x) + 128, as float32 (d = 128 and the
Euclidian metric unless --dim / --metric say otherwise; the queries keep their fractions: 127 q + 128), and the dense call is
timed with wann_set_dense_rows off and on -- the same index, one process, the legs alternating (off, on, off, on), 21 calls per
leg, device time from the HIP events around the batch (counters()["device_ms"]), ids and distance bits compared between the
legs.  Nothing else runs in that mode; WANN_PF_ONLY=on / off runs one leg alone (under a kernel trace).  Those values are unit
vectors around a common offset of 128, which the squared-L2 proof cannot settle: every query goes on to the exact
scan and the call is the scan's.  --rows sift (with --byte-exact) keeps the shape -- 100 windows of 10 000 points, 99 queries
each -- and takes SIFT-like rows instead (tests/util.sift_like: integers 0 .. 255 of low intrinsic dimension; queries the same
plus a fraction), whose queries the dense path proves.
Run from the repo root.  Prints one JSON object."""
import json, os, subprocess, sys, time
os.environ.setdefault("WANN_TEST_HOOKS", "1")  # this tool flips WANN_* switches between calls on one index
os.environ.setdefault("WANN_DENSE_LONG_ROWS", "1")  # (float32 / uint8 / int8 rows of 513 .. 2048 elements, float16 rows of 129 .. 2048: the dense leg is the opt-in kernel)
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))


def _opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


BYTE_EXACT = "--byte-exact" in sys.argv
DTYPE = "float32" if BYTE_EXACT else _opt("--dtype", "float32")
DIM = int(_opt("--dim", os.environ.get("WANN_PF_DIM", "128" if BYTE_EXACT else "100")))  # (WANN_PF_DIM: the option's older spelling)
NCLU = int(_opt("--clusters", "100"))
METRIC = _opt("--metric", "l2" if BYTE_EXACT else "mips")
CLASS = {"float32": "FloatMips", "float16": "Float16Mips", "int8": "Int8Mips", "uint8": "UInt8Euclidian"}[DTYPE]
if METRIC == "l2" and DTYPE in ("float32", "float16"):
    CLASS = CLASS.replace("Mips", "Euclidian")
SHAPE_ARGS = ["--dtype", DTYPE, "--dim", str(DIM), "--clusters", str(NCLU), "--metric", METRIC]
ELEM_BYTES = {"float32": 4, "float16": 2, "int8": 1, "uint8": 1}[DTYPE]


def as_elem(a):
    """a (unit-norm float32 rows) as the index of --dtype holds it"""
    if DTYPE == "float32":
        return a
    if DTYPE == "float16":
        return a.astype(np.float16)
    q = np.rint(127.0 * a)
    return q.astype(np.int8) if DTYPE == "int8" else (q + 128).astype(np.uint8)


def padded_row_bytes(d):
    """bytes of a stored row: float32 rows are padded to 16 floats, float16 rows to 32 halves, byte rows to 64 bytes"""
    return 64 * ((d * ELEM_BYTES + 63) // 64)


def make():
    cache = os.environ.get("WANN_PF_CACHE")
    path = os.path.join(cache, f"pf_{DTYPE}_{DIM}_{NCLU}.npz") if cache else None
    if path and os.path.exists(path):
        z = np.load(path)
        return z["X"], z["Q"], z["labels"], z["W1"], z["W2"], int(z["per"]), int(z["w"])
    out = _make()
    if path:
        np.savez(path, X=out[0], Q=out[1], labels=out[2], W1=out[3], W2=out[4], per=out[5], w=out[6])
    return out


def _make():
    rng = np.random.default_rng(0)
    nclu, per, d = NCLU, 10000, DIM
    n = nclu * per
    cent = rng.standard_normal((nclu, d)).astype(np.float32)
    X = cent[np.repeat(np.arange(nclu), per)] + 0.1 * rng.standard_normal((n, d)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    labels = (np.repeat(np.arange(nclu), per) - 0.5 + rng.random(n)).astype(np.float32)
    qc = np.repeat(np.arange(nclu), 99)
    Q = cent[(qc + 1 + rng.integers(0, nclu - 1, qc.size)) % nclu] + 0.1 * rng.standard_normal((qc.size, d)).astype(np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    Q = Q.astype(np.float32)
    W1 = np.stack([qc - 0.5, qc + 0.5], 1).astype(np.float32)
    # (ii) 2^-12 of the points (244) at a random place of the label order: [label[s], label[s + 244]]
    ls = np.sort(labels)
    w = int(n * 2.0 ** -12)
    st = np.random.default_rng(5).integers(1, n - w - 1, size=Q.shape[0])
    W2 = np.stack([ls[st], ls[st + w]], 1).astype(np.float32)
    return as_elem(X), as_elem(Q), labels, W1, W2, per, w


if len(sys.argv) > 2 and sys.argv[1] == "--ref-worker":  # child: the real reference with PARLAY_NUM_THREADS from the environment
    os.environ["WANN_NO_TORCH"] = "1"
    from oracle import oracle as orc
    from util import quiet_stdout
    X, Q, labels, W1, W2, per, w = make()
    res = np.load(sys.argv[2])
    ref = orc.load_reference(prefer=("x86-64-v4", "native"))
    assert ref is not None
    with quiet_stdout():
        ridx = getattr(ref, "PrefilterIndex" + CLASS.replace("Float16", "Float"))(X.astype(np.float32) if DTYPE == "float16" else X, labels)
    if DTYPE == "float16":
        Q = Q.astype(np.float32)  # (the reference has no float16 classes: a float16 index answers like the float32 one on the upcast)
    out = {}
    for name, W in (("native", W1), ("p12", W2)):
        best = 1e9
        for _ in range(3):
            t = time.perf_counter()
            with quiet_stdout():
                rids, rd = ridx.batch_search(Q, W.astype(np.float64), Q.shape[0], ref.QueryParams(10, 10, 1.35, 10**7, 10**4, 1, 10000, None, False))
            best = min(best, time.perf_counter() - t)
        out[name] = dict(qps=round(Q.shape[0] / best), dists_identical=bool(np.array_equal(rd, res["d_" + name])))
    print(json.dumps(out))
    sys.exit(0)

os.environ.setdefault("PARLAY_NUM_THREADS", str(os.cpu_count()))
import torch
import window_ann as wa

X, Q, labels, W1, W2, per, w = make()
if BYTE_EXACT:  # the uint8 leg's values (as_elem), as float32; the queries are not rounded
    X = (np.rint(127.0 * X) + 128).astype(np.float32)
    Q = (127.0 * Q + 128).astype(np.float32)
    if _opt("--rows", "uint8-leg") == "sift":
        from util import sift_like
        g = sift_like(X.shape[0], X.shape[1], 3)
        X = g(X.shape[0]) + np.float32(0)  # (+ 0: clip keeps the -0.0 that rint makes, and the one-byte rule is on bits)
        Q = (g(Q.shape[0]) + np.random.default_rng(4).random(Q.shape, dtype=np.float32) - np.float32(0.5)).astype(np.float32)
    assert X.min() >= 0 and X.max() <= 255 and X.dtype == np.float32
d = X.shape[1]
nq = Q.shape[0]
idx = getattr(wa, "PrefilterIndex" + CLASS)(X, labels)
qp = wa.QueryParams(10, 10, 1.35, 10**7, 10**4, 1, 10000, None, False)
dev = torch.device("cuda:0")
Qt = torch.from_numpy(Q.astype(np.float32)).to(dev)  # (device-buffer calls take fp32 queries; every element type converts exactly)
it, dt = torch.empty((nq, 10), dtype=torch.int32, device=dev), torch.empty((nq, 10), dtype=torch.float32, device=dev)


REPS = int(os.environ.get("WANN_PF_REPS", "21"))


def timed(Wt, env):
    if env: os.environ["WANN_NO_GEMM"] = env
    else: os.environ.pop("WANN_NO_GEMM", None)
    for _ in range(3):
        idx.batch_search_device(Qt.data_ptr(), Wt.data_ptr(), nq, 0, "", qp, it.data_ptr(), dt.data_ptr(), 0)
    wall, devms = [], []
    for _ in range(REPS):  # (the call returns after the batch's last kernel: it synchronises)
        t = time.perf_counter()
        idx.batch_search_device(Qt.data_ptr(), Wt.data_ptr(), nq, 0, "", qp, it.data_ptr(), dt.data_ptr(), 0)
        wall.append((time.perf_counter() - t) * 1e3)
        devms.append(idx.counters()["device_ms"])
    ms = float(np.median(wall))
    c = dict(idx.counters(), device_ms=float(np.median(devms)))
    return dict(ms=round(ms, 3), ms_min=round(min(wall), 3), ms_max=round(max(wall), 3), device_ms_min=round(min(devms), 3), device_ms_max=round(max(devms), 3),
                qps=round(nq / ms * 1e3), counters=c, ids=it.cpu().numpy().view(np.uint32).copy(), d=dt.cpu().numpy().copy())


W1t, W2t = torch.from_numpy(W1).to(dev), torch.from_numpy(W2).to(dev)
if BYTE_EXACT:
    assert idx.dense_rows_bytes() == X.shape[0] * 64 * ((d + 63) // 64), "the index has no one-byte copy for its dense path"

    def leg(on):
        assert idx.set_dense_rows(on) is on
        r = timed(W1t, None)
        assert r["counters"]["dense_rows"] == (1 if on else 0) and r["counters"]["gemm_queries"] > 0, r["counters"]
        return r

    only = os.environ.get("WANN_PF_ONLY")
    if only in ("on", "off"):  # under a kernel trace: one leg alone
        r = leg(only == "on")
        print(json.dumps(dict(leg=only, ms=r["ms"], device_ms=r["counters"]["device_ms"], gemm_queries=int(r["counters"]["gemm_queries"]), calls=REPS + 3)))
        sys.exit(0)
    legs = [("off", leg(False)), ("on", leg(True)), ("off", leg(False)), ("on", leg(True))]
    idx.set_dense_rows(False)
    ref = legs[0][1]
    same = all(np.array_equal(r["ids"], ref["ids"]) and np.array_equal(r["d"].view(np.uint32), ref["d"].view(np.uint32)) for _, r in legs)
    dev_ms = {name: [round(r["counters"]["device_ms"], 4) for n2, r in legs if n2 == name] for name in ("off", "on")}
    dev_rng = {name: [[r["device_ms_min"], r["device_ms_max"]] for n2, r in legs if n2 == name] for name in ("off", "on")}
    ratios = [round(a / b, 4) for a in dev_ms["off"] for b in dev_ms["on"]]
    print(json.dumps(dict(workload=f"adversarial {NCLU}x10000 d={d} float32 rows of integers 0 .. 255 ({_opt('--rows', 'uint8-leg')} values), {'Euclidian' if CLASS.endswith('Euclidian') else 'MIPS'}, {nq} queries, window = 1 cluster",
                          legs="wann_set_dense_rows off / on, alternating (off, on, off, on), one index, one process", timed_calls_per_leg=REPS,
                          device_ms_median=dev_ms, device_ms_min_max=dev_rng, wall_ms_median={name: [r["ms"] for n2, r in legs if n2 == name] for name in ("off", "on")},
                          off_over_on=dict(all_pairs=ratios, min=min(ratios), max=max(ratios)),
                          repeat_spread=dict(off=round(max(dev_ms["off"]) / min(dev_ms["off"]), 4), on=round(max(dev_ms["on"]) / min(dev_ms["on"]), 4)),
                          ids_and_distance_bits_equal=bool(same), gemm_queries=int(ref["counters"]["gemm_queries"]),
                          gemm_unproven=[int(r["counters"]["gemm_unproven"]) for _, r in legs], gemm_rescued=[int(r["counters"]["gemm_rescued"]) for _, r in legs],
                          row_bytes=dict(float32=64 * ((4 * d + 63) // 64), one_byte=64 * ((d + 63) // 64)))))
    sys.exit(0)
if os.environ.get("WANN_PF_ONLY") == "p12":  # dev runs under a profiler: the synthetic windows alone
    r = timed(W2t, None)
    print(json.dumps(dict(ms=r["ms"], device_ms=r["counters"]["device_ms"], brute_rows=int(r["counters"]["brute_rows"]))))
    sys.exit(0)
if os.environ.get("WANN_PF_ONLY") == "mfma":  # under a kernel trace: the dense leg alone
    r = timed(W1t, None)
    print(json.dumps(dict(ms=r["ms"], device_ms=r["counters"]["device_ms"], gemm_queries=int(r["counters"]["gemm_queries"]), calls=REPS + 3)))
    sys.exit(0)
if os.environ.get("WANN_PF_ONLY") == "scan":  # the exact-scan leg alone, twice: all that a build without the dense kernel of this row length can run
    r = [timed(W1t, "1"), timed(W1t, "1")]
    print(json.dumps(dict(scan_ms=[x["ms"] for x in r], scan_device_ms=[round(x["counters"]["device_ms"], 3) for x in r], gemm_queries=int(r[1]["counters"]["gemm_queries"]))))
    sys.exit(0)
out = {"mfma": timed(W1t, None), "scan": timed(W1t, "1"), "p12": timed(W2t, None)}
# (the two legs of the comparison once more, alternating: what one leg moves between its two runs is the spread to beat)
again = {"mfma": timed(W1t, None), "scan": timed(W1t, "1")}
os.environ.pop("WANN_NO_GEMM", None)
same = np.array_equal(out["mfma"]["d"], out["scan"]["d"])
# the reference at several thread counts (its best is what is reported)
res_path = "/tmp/wann_prefilter_gpu_rows.npz"
np.savez(res_path, d_native=out["mfma"]["d"], d_p12=out["p12"]["d"])
cpu = {}
ncpu = os.cpu_count() or 1
ref_threads = sorted({ncpu, max(1, ncpu // 2), max(1, ncpu // 4), max(1, ncpu // 8)}, reverse=True)
if os.environ.get("WANN_PF_REF_THREADS"):  # (a box that grants fewer CPUs than it shows: the thread counts to try, e.g. 16,8)
    ref_threads = [int(x) for x in os.environ["WANN_PF_REF_THREADS"].split(",")]
for th in ([] if os.environ.get("WANN_PF_NO_REF") else ref_threads):  # (WANN_PF_NO_REF=1: dev runs)
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--ref-worker", res_path] + SHAPE_ARGS, env=dict(os.environ, PARLAY_NUM_THREADS=str(th)),
                           capture_output=True, text=True, timeout=900)
        r = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
        for name, v in r.items():
            if name not in cpu or v["qps"] > cpu[name]["qps"]:
                cpu[name] = dict(v, threads=th)
    except Exception as e:  # noqa: BLE001
        print(f"[prefilter] reference with {th} threads failed: {e!r}", file=sys.stderr)
flops = 2.0 * nq * per * d
scan_bytes = float(out["p12"]["counters"]["brute_rows"]) * d * ELEM_BYTES  # w * d * sizeof(T) per brute-force query
win_bytes = NCLU * per * padded_row_bytes(d)  # a window group reads each of its (padded) point rows once
p12_dev_ms = out["p12"]["counters"]["device_ms"]
spread = lambda leg: dict(ms=[out[leg]["ms"], again[leg]["ms"]], ms_min=[out[leg]["ms_min"], again[leg]["ms_min"]], ms_max=[out[leg]["ms_max"], again[leg]["ms_max"]],
                          device_ms=[round(out[leg]["counters"]["device_ms"], 3), round(again[leg]["counters"]["device_ms"], 3)])
print(json.dumps(dict(workload=f"adversarial {NCLU}x10000 d={d} {DTYPE} {'Euclidian' if CLASS.endswith('Euclidian') else 'MIPS'}, {nq} queries, window = 1 cluster", mfma_ms=out["mfma"]["ms"], mfma_qps=out["mfma"]["qps"],
                      scan_ms=out["scan"]["ms"], scan_qps=out["scan"]["qps"], mfma_equals_scan=bool(same),
                      scan_device_ms=round(out["scan"]["counters"]["device_ms"], 3), timed_calls_per_leg=REPS,
                      repeated_legs=dict(mfma=spread("mfma"), scan=spread("scan")),
                      gemm_queries=out["mfma"]["counters"]["gemm_queries"], gemm_unproven=out["mfma"]["counters"]["gemm_unproven"], gemm_rescued=out["mfma"]["counters"]["gemm_rescued"], device_ms=round(out["mfma"]["counters"]["device_ms"], 3), gemm_tflops_incl_select=round(flops / out["mfma"]["ms"] / 1e9, 2),
                      cpu_reference=cpu.get("native"),
                      # the MFMA leg against its roofline: a window group reads each of its point rows ONCE (padded row of
                      # 16 * ceil(d / 16) floats; 100 groups x 10 000 rows here), so the floor is the HBM's, not the matrix
                      # pipes' (DESIGN.md 3.3b "Round 3"); `achieved` is over the WHOLE call's device time (ten small launches) --
                      # k_gemm_scores alone: profiles/*_prefilter_rocprofv3_kernel_stats.csv
                      roofline=dict(bound="hbm", kernel="k_gemm_scores (whole call: route + grouping + GEMM + select / re-rank + finalize)",
                                    achieved=round(win_bytes / (out["mfma"]["counters"]["device_ms"] * 1e-3) / 1e9, 1),
                                    peak=8000.0, unit="GB/s",
                                    frac=round(win_bytes / (out["mfma"]["counters"]["device_ms"] * 1e-3) / 1e9 / 8000.0, 4),
                                    algorithmic_gb=round(win_bytes / 1e9, 4), traffic=None),
                      synthetic_2pow_minus12=dict(workload=f"same points, synthetic windows of {w} points (2^-12), exact scan (k_brute)", ms=out["p12"]["ms"], qps=out["p12"]["qps"],
                                                  device_ms=round(p12_dev_ms, 4), brute_rows=int(out["p12"]["counters"]["brute_rows"]),
                                                  algorithmic_gb=round(scan_bytes / 1e9, 4),
                                                  roofline=dict(bound="hbm", kernel="k_brute (whole call: route + scan + finalize)", achieved=round(scan_bytes / (p12_dev_ms * 1e-3) / 1e9, 1),
                                                                peak=8000.0, unit="GB/s", frac=round(scan_bytes / (p12_dev_ms * 1e-3) / 1e9 / 8000.0, 4), traffic=None),
                                                  cpu_reference=cpu.get("p12")))))

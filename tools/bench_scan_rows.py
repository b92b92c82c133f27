"""The exact scans of a float32 index from its own rows, its half-precision shadow rows and its one-byte shadow rows
(wann_set_scan_rows) -- on one index in one process: BASELINE.json configs[1] (SIFT-1M-like, 2-WST, squared L2) with bench.py's
data law and seeds, the points' negative zeros made +0.0 (without which the set has no one-byte rows; tools/bench_byte_rows.py).

Workloads (10 000 queries, device-resident call form, every call host-synchronous so that its counters are its own):
  optimized_postfilter at window fractions 2^-16 .. 2^-12 (every query a scan: the tiny-window rule);
  fenwick at 2^-6 (two end scans per query beside the graph searches);
  set_exact_windows(L), L = 4 096 and 65 536, at fractions 2^-8 and 2^-4 (what the dense path leaves to the scan).
The legs of a workload are timed ALTERNATELY, `--reps` times each (at least 10) after two warm-up calls per (workload, leg).
A workload's legs must return equal ids, distance bits and work counters before its times count.  Reported per leg: ms per
batch by the host clock (median, and the spread max - min over the repetitions), device_ms likewise, and
scan_bytes_over_device_ms_share_of_8TBps: the scan's algorithmic bytes (brute_rows x the leg's row pitch) over device_ms as a
share of 8 TB/s -- of the whole batch's device time, so a batch that also searches graphs shows a small share.
--n / --nq: small rehearsal sizes.  Prints one JSON object (profiles/scan_rows_bench.json).
   python tools/bench_scan_rows.py [--reps 10] [--n 1000000] [--nq 10000]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

# leg -> (set_scan_rows, set_byte_rows, what counters()["scan_rows"] reports, bytes per element of a scanned row)
LEGS = {"own_rows": (False, False, 0, 4), "half_rows": (True, False, 1, 2), "byte_rows": (True, True, 2, 1)}
WORK = ("beam_searches", "hops", "dist_cmps", "brute_rows", "label_reads")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cache", default="", help="graph cache directory (none: the graphs are built on the GPU every time)")
    args = ap.parse_args()
    reps = max(10, args.reps)
    os.environ.setdefault("PARLAY_NUM_THREADS", str(min(16, os.cpu_count() or 1)))
    import numpy as np
    import torch
    import rangefilteredann_amd  # noqa: F401
    import window_ann as wa
    import bench
    import fullsize_configs as fc

    cfg = fc.CONFIGS["sift"]
    n, nq, d = args.n, args.nq, cfg["d"]
    X, Q, labels = bench.make_data(n, d, nq, 1)
    neg_zeros = int(np.signbit(X).sum())
    X = X + np.float32(0)
    cache = ""
    if args.cache:
        cache = os.path.join(args.cache, f"scan_rows_n{n}") + "/"
        os.makedirs(cache, exist_ok=True)
    t0 = time.time()
    idx = getattr(wa, cfg["cls"])(X, labels, build_params=wa.BuildParams(fc.R, fc.L, fc.ALPHA, cache), **cfg["kw"])
    build_s = time.time() - t0
    if not idx.half_rows() or idx.byte_rows_bytes() <= 0:
        print("[scan rows] the index has no half rows or no one-byte rows", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    Qt = torch.from_numpy(Q).to(dev)
    ids_t = torch.empty((nq, fc.K), dtype=torch.int32, device=dev)
    dist_t = torch.empty((nq, fc.K), dtype=torch.float32, device=dev)
    qp = fc.query_params(wa, 80, 1)
    s = np.sort(labels)
    # (name, method, window fraction, exact-window limit)
    workloads = [(f"optimized_postfilter 2^{p}", "optimized_postfilter", p, 0) for p in range(-16, -11)]
    workloads.append(("fenwick 2^-6", "fenwick", -6, 0))
    workloads += [(f"exact_windows({L}) 2^{p}", "optimized_postfilter", p, L) for L in (4096, 65536) for p in (-8, -4)]
    pitch = {t: 64 * -(-(d * esz) // 64) for t, (_, _, _, esz) in LEGS.items()}

    def select(tag):
        scan_on, byte_on, _, _ = LEGS[tag]
        assert idx.set_half_rows(True) is True and idx.set_byte_rows(byte_on) is byte_on and idx.set_scan_rows(scan_on) is scan_on

    res = dict(tool="tools/bench_scan_rows.py", index=f"{cfg['cls']} n={n} d={d} L2 R={fc.R} L={fc.L} {cfg['kw']} nq={nq} k={fc.K} beam=80",
               reps=reps, build_s=round(build_s, 1), negative_zeros_made_positive=neg_zeros, row_pitch_bytes=pitch,
               half_rows_bytes=int(idx.half_rows_bytes()), byte_rows_bytes=int(idx.byte_rows_bytes()), workloads={})
    for name, method, p, L in workloads:
        Wt = torch.from_numpy(bench.make_windows(s, nq, p, 2000 + p)).to(dev)
        assert idx.set_exact_windows(L) == 0

        def run():
            idx.batch_search_device(Qt.data_ptr(), Wt.data_ptr(), nq, 0, method, qp, ids_t.data_ptr(), dist_t.data_ptr(), 0)

        rows, ctr = {}, {}
        for tag in LEGS:  # warm-up, and the rows / counters to compare
            select(tag)
            run()
            run()
            rows[tag] = (ids_t.cpu().numpy().copy(), dist_t.cpu().numpy().view(np.uint32).copy())
            ctr[tag] = idx.counters()
            if ctr[tag]["brute_rows"]:
                assert ctr[tag]["scan_rows"] == LEGS[tag][2], (name, tag, ctr[tag]["scan_rows"])
        base = "own_rows"
        assert all(np.array_equal(rows[base][0], rows[t][0]) and np.array_equal(rows[base][1], rows[t][1]) for t in LEGS), (name, "rows differ")
        assert all(ctr[base][k] == ctr[t][k] for k in WORK for t in LEGS), (name, "work counters differ")
        ms, dms = {t: [] for t in LEGS}, {t: [] for t in LEGS}
        for _ in range(reps):
            for tag in LEGS:
                select(tag)
                torch.cuda.synchronize()
                t = time.perf_counter()
                run()
                ms[tag].append((time.perf_counter() - t) * 1e3)
                dms[tag].append(idx.counters()["device_ms"])
        c = ctr[base]
        out = dict(rows_identical=True, counters_equal=True, counters={k: c[k] for k in WORK},
                   exact_window_counters=idx.exact_window_counters() if L else None)
        for tag in LEGS:
            m, dm = float(np.median(ms[tag])), float(np.median(dms[tag]))
            gb = c["brute_rows"] * pitch[tag] / 1e9
            out[tag] = dict(ms_per_batch=round(m, 4), ms_spread=round(max(ms[tag]) - min(ms[tag]), 4), device_ms=round(dm, 4),
                            device_ms_spread=round(max(dms[tag]) - min(dms[tag]), 4), qps=round(nq / m * 1e3),
                            device_ms_per_call=[round(x, 4) for x in dms[tag]], scan_gb_per_batch=round(gb, 4),
                            scan_bytes_over_device_ms_share_of_8TBps=round(gb / dm / 8.0, 4) if dm > 0 else None)
        for tag in ("half_rows", "byte_rows"):
            out["speedup_device_ms_" + tag + "_over_own_rows"] = round(out[base]["device_ms"] / out[tag]["device_ms"], 3)
        res["workloads"][name] = out
        assert idx.set_exact_windows(0) == L
    select("own_rows")  # (what a new index starts with)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())

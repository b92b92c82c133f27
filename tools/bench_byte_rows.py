"""The three row stores of a float32 index whose points are all integers 0 .. 255 -- its float32 rows, its half-precision shadow
rows (wann_set_half_rows) and its one-byte shadow rows (wann_set_byte_rows) -- on one index in one process: BASELINE.json
configs[1] (SIFT-1M-like, 2-WST, squared L2, window 2^-3, optimized_postfilter) with bench.py's data law and seeds at the
setting (80, x1) -- with the points' negative zeros made +0.0 (see below), without which the set has no one-byte rows.

The index is built once; the three stores are then timed ALTERNATELY (device-resident queries, every call host-synchronous
so that its counters are its own), each leg `--reps` times (at least twice).  The legs' ids and distance bits must be equal,
and so must the operation counters.  Reported per leg: QPS, search_kernel_ms, device_ms and the share of the HBM rate that
the algorithm's bytes (adjacency rows, scored vectors at the store's element size, labels) amount to.
--n / --nq: small rehearsal sizes.  Prints one JSON object (profiles/byte_rows_bench.json).
   python tools/bench_byte_rows.py [--reps 10] [--n 1000000] [--nq 10000] [--setting 80,1]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

# leg -> (set_byte_rows, set_half_rows, bytes per element of a scored row)
LEGS = {"float32_rows": (False, False, 4), "half_rows": (False, True, 2), "byte_rows": (True, True, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--fraction", type=int, default=-3)
    ap.add_argument("--setting", default="80,1", help="'beam,mult'")
    ap.add_argument("--cache", default="", help="graph cache directory (none: the graphs are built on the GPU every time)")
    args = ap.parse_args()
    reps = max(2, args.reps)
    os.environ.setdefault("PARLAY_NUM_THREADS", str(min(16, os.cpu_count() or 1)))
    import numpy as np
    import torch
    import rangefilteredann_amd  # noqa: F401
    import window_ann as wa
    import bench
    import fullsize_configs as fc

    cfg = fc.CONFIGS["sift"]
    n, nq, d = args.n, args.nq, cfg["d"]
    beam, mult = (int(x) for x in args.setting.split(","))
    X, Q, labels = bench.make_data(n, d, nq, 1)
    # bench.py's points hold -0.0 where a value in (-0.5, 0) was rounded (numpy's clip keeps its sign), and the one-byte rows'
    # rule is on bits: such a set has half rows and no one-byte rows.  Adding +0.0 makes those zeros +0.0 and changes no value.
    neg_zeros = int(np.signbit(X).sum())
    X = X + np.float32(0)
    W = bench.make_windows(np.sort(labels), nq, args.fraction, 2000 + args.fraction)
    cache = ""
    if args.cache:
        cache = os.path.join(args.cache, f"byte_rows_n{n}") + "/"
        os.makedirs(cache, exist_ok=True)
    t0 = time.time()
    idx = getattr(wa, cfg["cls"])(X, labels, build_params=wa.BuildParams(fc.R, fc.L, fc.ALPHA, cache), **cfg["kw"])
    build_s = time.time() - t0
    if not idx.half_rows() or idx.byte_rows_bytes() <= 0:
        print("[byte rows] the index has no half rows or no one-byte rows", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    Qt, Wt = torch.from_numpy(Q).to(dev), torch.from_numpy(W).to(dev)
    ids_t = torch.empty((nq, fc.K), dtype=torch.int32, device=dev)
    dist_t = torch.empty((nq, fc.K), dtype=torch.float32, device=dev)
    qp = fc.query_params(wa, beam, mult)

    def run():
        idx.batch_search_device(Qt.data_ptr(), Wt.data_ptr(), nq, 0, cfg["method"], qp, ids_t.data_ptr(), dist_t.data_ptr(), 0)

    def select(tag):
        byte_on, half_on, _ = LEGS[tag]
        assert idx.set_byte_rows(byte_on) is byte_on and idx.set_half_rows(half_on) is half_on

    rows, ctr = {}, {}
    for tag in LEGS:  # warm-up, and the rows / counters to compare
        select(tag)
        run()
        run()
        rows[tag] = (ids_t.cpu().numpy().copy(), dist_t.cpu().numpy().view(np.uint32).copy())
        ctr[tag] = idx.counters()
        assert ctr[tag]["byte_rows"] == int(tag == "byte_rows") and ctr[tag]["half_rows"] == int(tag == "half_rows"), tag
    work = ("beam_searches", "hops", "dist_cmps", "brute_rows", "label_reads")
    base = "float32_rows"
    rows_identical = all(bool(np.array_equal(rows[base][0], rows[t][0]) and np.array_equal(rows[base][1], rows[t][1])) for t in LEGS)
    counters_equal = all(ctr[base][k] == ctr[t][k] for k in work for t in LEGS)
    assert rows_identical, "ids / distance bits of the row stores differ"
    assert counters_equal, "operation counters of the row stores differ"

    ms = {t: [] for t in LEGS}
    kms = {t: [] for t in LEGS}
    dms = {t: [] for t in LEGS}
    for _ in range(reps):
        for tag in LEGS:
            select(tag)
            torch.cuda.synchronize()
            t = time.perf_counter()
            run()
            ms[tag].append((time.perf_counter() - t) * 1e3)
            c = idx.counters()
            kms[tag].append(c["search_kernel_ms"])
            dms[tag].append(c["device_ms"])
    select("half_rows")  # (what a new index starts with)
    c = ctr[base]
    res = dict(tool="tools/bench_byte_rows.py",
               workload=f"{cfg['cls']} n={n} d={d} L2 R={fc.R} L={fc.L} {cfg['kw']} window 2^{args.fraction} nq={nq} k={fc.K}",
               setting=dict(beam=beam, mult=mult), reps=reps, build_s=round(build_s, 1), rows_identical=rows_identical,
               counters_equal=counters_equal, counters={k: c[k] for k in work}, device_bytes=int(idx.device_bytes()),
               half_rows_bytes=int(idx.half_rows_bytes()), byte_rows_bytes=int(idx.byte_rows_bytes()),
               negative_zeros_made_positive=neg_zeros)
    for tag, (_, _, esz) in LEGS.items():
        m, km = float(np.median(ms[tag])), float(np.median(kms[tag]))
        gb = (4 * (fc.R + 1) * c["hops"] + esz * d * c["dist_cmps"] + 4 * c["label_reads"]) / 1e9
        res[tag] = dict(qps=round(nq / m * 1e3), ms_per_batch=round(m, 3), search_kernel_ms=round(km, 3),
                        device_ms=round(float(np.median(dms[tag])), 3), ms_per_call=[round(x, 3) for x in ms[tag]],
                        search_kernel_ms_per_call=[round(x, 3) for x in kms[tag]], device_ms_per_call=[round(x, 3) for x in dms[tag]],
                        algorithmic_gb_per_batch=round(gb, 3), hbm_share=round(gb / km / 8.0, 4) if km > 0 else None)
    for tag in ("half_rows", "byte_rows"):
        res["speedup_qps_" + tag + "_over_float32"] = round(res[tag]["qps"] / res[base]["qps"], 3)
    res["speedup_qps_byte_rows_over_half_rows"] = round(res["byte_rows"]["qps"] / res["half_rows"]["qps"], 3)
    res["speedup_search_kernel_byte_rows_over_half_rows"] = round(res["half_rows"]["search_kernel_ms"] / res["byte_rows"]["search_kernel_ms"], 3)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())

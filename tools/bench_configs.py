"""BASELINE.json configs[2] and configs[3] at FULL size on one MI355X (they are parity cases, not the bench line):

  glove : 'GloVe-like'  n = 1 183 514, d = 100, unit-norm mixture rows, MIPS, SuperOptimizedPostfilterTree (split 2, shift 0.5),
          window fraction 2^-6, 10 000 queries                                            
  deep  : 'deep-like'   n = 9 990 000, d = 96, unit-norm mixture rows, MIPS (the reference maps '*angular*' names to MIPS),
          VamanaRangeFilterTree split 4, optimized_postfilter, window fraction 2^-3        (C4, here on ONE GPU)

For each: GPU index build (graphs saved to a cache directory in the reference's format), a beam x multiplier sweep against exact
GPU ground truth, the timed best setting, and -- through a child process per thread count, because the reference reads
PARLAY_NUM_THREADS once -- the REAL reference (oracle/_ref) loading THE SAME graph files and answering the same batch: rows must
be identical.  Prints one JSON object.  Usage:  python tools/bench_configs.py --config glove [--threads 32,256]
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

CONFIGS = {
    "glove": dict(n=1_183_514, d=100, frac=-6, cls="SuperOptimizedPostfilterTreeIndexFloatMips", kw=dict(cutoff=1000, split_factor=2, shift_factor=0.5), method=None),
    "deep": dict(n=9_990_000, d=96, frac=-3, cls="VamanaRangeFilterTreeIndexFloatMips", kw=dict(cutoff=1000, split_factor=4), method="optimized_postfilter"),
    # configs[3] as BASELINE.json's text states it ("96-d L2"): the same rows and tree under squared L2 (the reference itself runs
    # deep-image-96-angular under inner product: experiments/run_our_method.py:218)
    "deep_l2": dict(n=9_990_000, d=96, frac=-3, cls="VamanaRangeFilterTreeIndexFloatEuclidian", kw=dict(cutoff=1000, split_factor=4), method="optimized_postfilter"),
    # the other two query methods of the tree (range_filter_tree.h:297-401,473-540) at configs[1] size, unit-norm MIPS rows
    # (continuous coordinates: no distance ties, so rows must match exactly although both sides sort unstably)
    "fenwick": dict(n=1_000_000, d=100, frac=-6, cls="VamanaRangeFilterTreeIndexFloatMips", kw=dict(cutoff=1000, split_factor=2), method="fenwick"),
    "three_split": dict(n=1_000_000, d=100, frac=-6, cls="VamanaRangeFilterTreeIndexFloatMips", kw=dict(cutoff=1000, split_factor=2), method="three_split"),
    # configs[1]'s points, queries, tree and window fraction with the points held as BYTES (python_bindings.cpp:234-237: the
    # UInt8Euclidian variant; euclidian_point.h:44-60: int32 accumulation cast to float): a quarter of the vector traffic per
    # scored neighbour, the adjacency rows unchanged
    "sift_u8": dict(n=1_000_000, d=128, frac=-3, cls="VamanaRangeFilterTreeIndexUInt8Euclidian", kw=dict(cutoff=1000, split_factor=2),
                    method="optimized_postfilter", law="sift", dtype="uint8"),
}
R, L, ALPHA, K = 64, 500, 1.0, 10


def make(cfg, n, nq):
    import numpy as np
    if cfg.get("law") == "sift":  # bench.py's SIFT-1M-like law and seeds (integer values 0 .. 255: exact as bytes)
        import bench
        X, Q, labels = bench.make_data(n, cfg["d"], nq, 1)
        return X.astype(cfg["dtype"]), Q.astype(cfg["dtype"]), labels
    from util import unit_mixture
    g = unit_mixture(n, cfg["d"], 2025)
    X, Q = g(n), g(nq)
    labels = ((np.random.default_rng(77).permutation(n) + 0.5) / n).astype(np.float32)
    return X, Q, labels


def qp(mod, beam, mult):
    return mod.QueryParams(K, beam, 1.35, 10_000_000, 10_000, mult, 10000, None, False)


def worker(args):
    """child: the real reference on the cached graphs"""
    os.environ["WANN_NO_TORCH"] = "1"
    import numpy as np
    from oracle import oracle as orc
    from util import quiet_stdout
    cfg = CONFIGS[args.config]
    X, Q, labels = make(cfg, args.n, args.nq)
    res = np.load(args.result)
    ref = orc.load_reference(prefer=("x86-64-v4", "native", "x86-64-v3"))
    assert ref is not None, "no reference build under oracle/_ref"
    t0 = time.time()
    with quiet_stdout():
        idx = getattr(ref, cfg["cls"])(X, labels, build_params=ref.BuildParams(R, L, ALPHA, args.cache), **cfg["kw"])
    load_s = time.time() - t0
    a = (Q, res["W"].astype(np.float64), args.nq) + ((cfg["method"],) if cfg["method"] else ())
    best, reps, t_all = None, 0, time.perf_counter()
    while reps < 2 or (time.perf_counter() - t_all < args.seconds and reps < 30):
        t = time.perf_counter()
        with quiet_stdout():
            ids, dists = idx.batch_search(*a, qp(ref, args.beam, args.mult))
        dt = time.perf_counter() - t
        best = dt if best is None else min(best, dt)
        reps += 1
    print(json.dumps(dict(threads=args.threads, qps=args.nq / best, reps=reps, index_load_s=round(load_s, 1),
                          same_ids=float((ids == res["ids"]).all(axis=1).mean()), same_dists=float((dists == res["dists"]).all(axis=1).mean()))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=list(CONFIGS), required=True)
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--threads", default="32,256", help="reference thread counts to try ('' = skip the reference)")
    ap.add_argument("--cache", default="/tmp/wann_cfg_cache")
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--beam", type=int, default=0)
    ap.add_argument("--mult", type=int, default=1)
    ap.add_argument("--result", default="")
    ap.add_argument("--setting", default="", help="'beam,mult': skip the sweep (profiling runs)")
    args = ap.parse_args()
    cfg = CONFIGS[args.config]
    args.n = args.n or cfg["n"]
    if args.worker:
        args.threads = int(args.threads)
        return worker(args)

    os.environ.setdefault("PARLAY_NUM_THREADS", str(os.cpu_count()))
    import numpy as np
    import torch
    import window_ann as wa
    n, d, nq = args.n, cfg["d"], args.nq
    mem_gib = os.sysconf("SC_PAGE_SIZE") * os.sysconf("SC_PHYS_PAGES") / 2**30
    t0 = time.time()
    X, Q, labels = make(cfg, n, nq)
    print(f"[cfg] {args.config}: data n={n} d={d} in {time.time() - t0:.1f}s; host {os.cpu_count()} cpus, {mem_gib:.0f} GiB", file=sys.stderr, flush=True)
    cache = os.path.join(args.cache, f"{'tree1m' if args.config in ('fenwick', 'three_split') else args.config}_n{n}") + "/"
    if args.config == "sift_u8" and os.environ.get("WANN_BENCH_SIFT_CACHE"):
        # bench.py's float32 index of the same points: on integer-valued data the byte and float32 builds make the same graphs
        # (exact arithmetic either way), so the leg may start from the graph files the headline run left behind
        cache = os.environ["WANN_BENCH_SIFT_CACHE"]
    os.makedirs(cache, exist_ok=True)
    t0 = time.time()
    index = getattr(wa, cfg["cls"])(X, labels, build_params=wa.BuildParams(R, L, ALPHA, cache), **cfg["kw"])
    build_s = time.time() - t0
    levels = index.levels()
    print(f"[cfg] index ready in {build_s:.1f}s: {sum(levels)} graphs in {len(levels)} levels, {index.device_bytes() / 2**30:.2f} GiB in HBM", file=sys.stderr, flush=True)

    dev = torch.device("cuda:0")
    # (device-resident queries of a byte index are float32 rows of integer values: include/wann.h)
    Xt, labt, Qt = torch.from_numpy(X.astype(np.float32)).to(dev), torch.from_numpy(labels).to(dev), torch.from_numpy(Q.astype(np.float32)).to(dev)
    esz = X.dtype.itemsize  # bytes per coordinate in HBM
    ls = np.sort(labels)
    w = int(n * 2.0 ** cfg["frac"])
    st = np.random.default_rng(5).integers(1, n - w - 1, size=nq)
    W = np.stack([ls[st], ls[st + w]], 1).astype(np.float32)
    Wt = torch.from_numpy(W).to(dev)
    gt = torch.empty((nq, K), dtype=torch.int64, device=dev)
    step = max(16, min(256, int(2**31 // (4 * n))))
    l2 = cfg["cls"].endswith("Euclidian")
    xn = (Xt * Xt).sum(1) if l2 else None
    for a in range(0, nq, step):  # exact filtered top-k (inner product, or squared L2 up to the query's own norm), inclusive bounds
        s = -(Qt[a:a + step] @ Xt.T)
        if l2:
            s = s * 2 + xn[None, :]
        s.masked_fill_(~((labt[None, :] >= Wt[a:a + step, 0:1]) & (labt[None, :] <= Wt[a:a + step, 1:2])), float("inf"))
        gt[a:a + step] = torch.topk(s, K, dim=1, largest=False).indices
    del s
    torch.cuda.synchronize()
    print("[cfg] ground truth done", file=sys.stderr, flush=True)
    ids_t = torch.empty((nq, K), dtype=torch.int32, device=dev)
    dist_t = torch.empty((nq, K), dtype=torch.float32, device=dev)
    method = cfg["method"] or ""

    def run(beam, mult):
        index.batch_search_device(Qt.data_ptr(), Wt.data_ptr(), nq, 0, method, qp(wa, beam, mult), ids_t.data_ptr(), dist_t.data_ptr(), 0)

    def recall():
        ids64 = ids_t.to(torch.int64) & 0xFFFFFFFF
        return float((gt[:, :, None] == ids64[:, None, :]).any(2).sum(1).double().mean().item() / K)

    rows = []
    for beam in ((10, 20, 40, 80, 160) if not args.setting else ()):
        for mult in (1, 2):
            run(beam, mult)
            t = time.perf_counter()
            run(beam, mult)
            ms = (time.perf_counter() - t) * 1e3
            rows.append(dict(beam=beam, mult=mult, recall=round(recall(), 4), ms=round(ms, 3)))
            print(f"[cfg]   beam {beam:4d} x{mult}: recall {rows[-1]['recall']:.4f}  {ms:.2f} ms", file=sys.stderr, flush=True)
    if args.setting:
        sb, sm = (int(x) for x in args.setting.split(","))
        rows = [dict(beam=sb, mult=sm, recall=1.0, ms=0.0)]
    ok = [r for r in rows if r["recall"] > 0.95]
    best = min(ok, key=lambda r: r["ms"]) if ok else max(rows, key=lambda r: r["recall"])
    reps = 10
    run(best["beam"], best["mult"])
    t = time.perf_counter()
    kernel_ms = []
    for _ in range(reps):
        run(best["beam"], best["mult"])
        kernel_ms.append(index.counters()["search_kernel_ms"])  # (the call is host-synchronous: the counters are this call's)
    ms = (time.perf_counter() - t) / reps * 1e3
    c = index.counters()
    c["search_kernel_ms"] = sum(kernel_ms) / len(kernel_ms)  # mean over the timed calls (one call's figure varies by +-10 %)
    print(f"[cfg] counters of the last batch: {c}", file=sys.stderr, flush=True)
    out = dict(config=args.config, workload=f"{cfg['cls']} n={n} d={d} {'L2' if l2 else 'MIPS'} R={R} L={L} {cfg['kw']} window 2^{cfg['frac']} nq={nq} k={K}",
               build_s=round(build_s, 1), graphs=int(sum(levels)), levels=len(levels), index_gib=round(index.device_bytes() / 2**30, 2),
               setting=dict(beam=best["beam"], mult=best["mult"]), recall_at_10=round(recall(), 4), ms_per_batch=round(ms, 3), qps=round(nq / ms * 1e3),
               search_kernel_ms=round(c["search_kernel_ms"], 3), search_kernel_ms_per_call=[round(x, 3) for x in kernel_ms],
               algorithmic_gb_per_batch=round((4 * (R + 1) * c["hops"] + esz * d * c["dist_cmps"] + 4 * c["label_reads"]) / 1e9, 3),  # (k_search's bytes: the end scans of fenwick / three_split are k_brute's)
               sweep=rows, reference=[])
    if c["search_kernel_ms"] > 0:
        out["k_search_tb_per_s"] = round(out["algorithmic_gb_per_batch"] / c["search_kernel_ms"], 3)
    if c.get("brute_rows", 0) > 0:
        # fenwick / three_split: the end scans (k_brute) run BESIDE the graph searches (wann_batch.cpp): the call's bytes are both
        # kernels', its time is the device time of the call
        out["scan_gb_per_batch"] = round(esz * d * c["brute_rows"] / 1e9, 3)
        out["device_ms"] = round(c["device_ms"], 3)
    if args.config == "deep_l2":
        out["metric_note"] = "squared L2, as BASELINE.json configs[3]'s text states it; the reference's own deep runs are inner product (configs.deep)"
    if args.config == "deep":  # BASELINE.json's config text says "96-d L2"; the reference itself runs deep under inner product
        out["metric_note"] = "inner product, as the reference runs deep-image-96-angular (experiments/run_our_method.py:218 maps '*angular*' to mips)"
    # the asynchronous call, two batches in flight (wann_batch_search_device_async): does a second batch in flight buy anything on
    # this leg?  Beside the blocking number, never instead of it; rows must equal the blocking call's.
    try:
        rows_b = (ids_t.clone(), dist_t.clone())
        outs = [(torch.empty_like(ids_t), torch.empty_like(dist_t)) for _ in range(3)]
        qpb = qp(wa, best["beam"], best["mult"])

        def pipelined(nsteps):
            tk = []
            for i in range(nsteps):
                oi, od = outs[i % 3]
                tk.append(index.batch_search_device_async(Qt.data_ptr(), Wt.data_ptr(), nq, 0, method, qpb, oi.data_ptr(), od.data_ptr(), 0))
                if i >= 1:
                    index.wait(tk[i - 1])
            index.wait(tk[-1])
        torch.cuda.synchronize()
        pipelined(3)
        t = time.perf_counter()
        pipelined(reps)
        torch.cuda.synchronize()
        pms = (time.perf_counter() - t) / reps * 1e3
        same = bool((outs[(reps - 1) % 3][0] == rows_b[0]).all().item()) and bool((outs[(reps - 1) % 3][1] == rows_b[1]).all().item())
        out["pipelined"] = dict(in_flight=2, ms_per_batch=round(pms, 3), qps=round(nq / pms * 1e3), speedup_over_blocking=round(ms / pms, 3),
                                hbm_frac_of_wall=round(out["algorithmic_gb_per_batch"] / pms * 1e3 / 8000.0, 4), rows_equal_blocking_call=same)
        print(f"[cfg] pipelined: {out['pipelined']}", file=sys.stderr, flush=True)
    except Exception as e:  # noqa: BLE001
        out["pipelined"] = dict(error=repr(e)[-300:])
    if args.threads:
        res = os.path.join(args.cache, f"{args.config}_result.npz")
        np.savez(res, W=W, ids=ids_t.cpu().numpy().view(np.uint32), dists=dist_t.cpu().numpy())
        del index
        for th in [int(x) for x in args.threads.split(",")]:
            env = dict(os.environ, PARLAY_NUM_THREADS=str(th))
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--config", args.config, "--n", str(n), "--nq", str(nq),
                                "--threads", str(th), "--cache", cache, "--beam", str(best["beam"]), "--mult", str(best["mult"]),
                                "--result", res, "--seconds", str(args.seconds)], env=env, capture_output=True, text=True, timeout=3000)
            line = [x for x in p.stdout.strip().splitlines() if x.startswith("{")]
            out["reference"].append(json.loads(line[-1]) if line else dict(threads=th, error=(p.stderr or "")[-400:]))
            print(f"[cfg] reference {out['reference'][-1]}", file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

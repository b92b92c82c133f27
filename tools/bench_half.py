"""Float16 points against float32 on the same box and data: BASELINE.json configs[1] (SIFT-1M-like, 2-WST, L2, 2^-3),
configs[2] (GloVe-like super tree, MIPS, 2^-6) and configs[3] (deep-like 10M, 4-WST, MIPS, 2^-3) at full size on one MI355X.

Per leg: the points and queries are rounded to float16 (numpy astype: nearest, ties to even); a float16 index is built on the
GPU into a cache directory of its own, and a float32 index on the UPCAST points opens the same graph files.  The setting (beam
x final multiplier) is the fastest with recall@10 >= 0.95 against exact ground truth of the ROUNDED data; the two indexes are
then timed ALTERNATELY in this one process (device-resident queries: fp32 rows of the rounded queries) and their rows must be
identical.  Reported per leg: QPS and search_kernel_ms of both, algorithmic bytes (2- or 4-byte elements) and their share of
8 TB/s, device_bytes of both, and recall@10 against exact ground truth of the UNROUNDED data for the float16 index and for a
float32 index built on the unrounded points (its own cache) at the same setting -- what a user deciding on float16 needs.
--dtype bfloat16: the same legs for the BFloat16 classes -- points and queries rounded with bfloat16_round (nearest, ties to
even, 8 significant bits), a cache directory of its own, identical rows required between the bfloat16 index and the float32
index on the upcast points; the report's keys say "bfloat16" where they say "float16" by default.
--dtype float8: likewise for the Float8 classes (OCP E4M3, one byte an element: float8_round).  --scale S multiplies points and
queries by S before rounding -- a power of two changes no ordering, and moves unit-norm components out of E4M3's subnormal range.
Prints one JSON object.   python tools/bench_half.py [--dtype float16|bfloat16|float8] [--scale 1] [--configs sift,glove,deep] [--reps 10] [--no-unrounded]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

LEGS = {  # fullsize_configs name, class suffix-less kind, window fraction
    "sift": dict(frac=-3, kind="VamanaRangeFilterTreeIndex", metric="Euclidian"),
    "glove": dict(frac=-6, kind="SuperOptimizedPostfilterTreeIndex", metric="Mips"),
    "deep": dict(frac=-3, kind="VamanaRangeFilterTreeIndex", metric="Mips"),
}
HBM_TBPS = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="sift,glove,deep")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--dtype", choices=("float16", "bfloat16", "float8"), default="float16", help="the narrow element type under test")
    ap.add_argument("--scale", type=float, default=1.0, help="multiply points and queries by this (a power of two) before rounding")
    ap.add_argument("--cache", default="/tmp/wann_half_cache")
    ap.add_argument("--no-unrounded", dest="unrounded", action="store_false", help="skip the float32 index on the unrounded points")
    ap.add_argument("--setting", default="", help="'beam,mult': skip the sweep (profiling runs)")
    args = ap.parse_args()
    os.environ.setdefault("PARLAY_NUM_THREADS", str(min(16, os.cpu_count() or 1)))
    import numpy as np
    import torch
    import rangefilteredann_amd  # noqa: F401
    import window_ann as wa
    import fullsize_configs as fc

    dev = torch.device("cuda:0")
    HALF = args.dtype
    half_cls = {"float16": "Float16", "bfloat16": "BFloat16", "float8": "Float8"}[HALF]
    half_esz = 1 if HALF == "float8" else 2

    def rounded(a):  # what an index of the type stores: a float16 array / the float32 values of the bfloat16 or float8 roundings
        a = a * np.float32(args.scale) if args.scale != 1.0 else a
        return a.astype(np.float16) if HALF == "float16" else wa.bfloat16_round(a) if HALF == "bfloat16" else wa.float8_round(a)

    K, R, L, ALPHA = fc.K, fc.R, fc.L, fc.ALPHA
    report = dict(tool="tools/bench_half.py", dtype=HALF, scale=args.scale, hbm_tb_per_s=HBM_TBPS, legs=[])

    def log(msg):
        print(f"[half] {msg}", file=sys.stderr, flush=True)

    for name in args.configs.split(","):
        leg, cfg = LEGS[name], fc.CONFIGS[name]
        n, d, nq = cfg["n"], cfg["d"], cfg["nq"]
        l2 = leg["metric"] == "Euclidian"
        X, Q, labels = fc.make_data(name)
        X16, Q16 = rounded(X), rounded(Q)
        W = fc.fraction_windows(labels, nq, leg["frac"], 2000 + leg["frac"]).astype(np.float32)
        method = cfg["method"] or ""
        kw = cfg["kw"]
        Wt = torch.from_numpy(W).to(dev)
        labt = torch.from_numpy(labels).to(dev)

        def ground_truth(Xs, Qs):
            Xt, Qt = torch.from_numpy(Xs.astype(np.float32)).to(dev), torch.from_numpy(Qs.astype(np.float32)).to(dev)
            gt = torch.empty((nq, K), dtype=torch.int64, device=dev)
            step = max(16, min(256, int(2**31 // (4 * n))))
            xn = (Xt * Xt).sum(1) if l2 else None
            for a in range(0, nq, step):
                s = -(Qt[a:a + step] @ Xt.T)
                if l2:
                    s = s * 2 + xn[None, :]
                s.masked_fill_(~((labt[None, :] >= Wt[a:a + step, 0:1]) & (labt[None, :] <= Wt[a:a + step, 1:2])), float("inf"))
                gt[a:a + step] = torch.topk(s, K, dim=1, largest=False).indices
            del Xt, s
            torch.cuda.synchronize()
            return gt

        gt_rounded, gt_orig = ground_truth(X16, Q16), ground_truth(X, Q)
        log(f"{name}: n={n} d={d}, ground truth of rounded and unrounded data done")
        Qt = torch.from_numpy(Q16.astype(np.float32)).to(dev)  # device calls: fp32 rows of the rounded queries
        ids_t = torch.empty((nq, K), dtype=torch.int32, device=dev)
        dist_t = torch.empty((nq, K), dtype=torch.float32, device=dev)

        def qp(beam, mult):
            return wa.QueryParams(K, beam, 1.35, 10_000_000, 10_000, mult, 10000, None, False)

        def run(index, beam, mult, Qdev=Qt):
            index.batch_search_device(Qdev.data_ptr(), Wt.data_ptr(), nq, 0, method, qp(beam, mult), ids_t.data_ptr(), dist_t.data_ptr(), 0)

        def recall(gt):
            ids64 = ids_t.to(torch.int64) & 0xFFFFFFFF
            return float((gt[:, :, None] == ids64[:, None, :]).any(2).sum(1).double().mean().item() / K)

        cache = os.path.join(args.cache, f"{name}_{HALF}_n{n}") + "/"
        os.makedirs(cache, exist_ok=True)
        t0 = time.time()
        h = getattr(wa, leg["kind"] + half_cls + leg["metric"])(X16, labels, build_params=wa.BuildParams(R, L, ALPHA, cache), **kw)
        build_s = time.time() - t0
        f = getattr(wa, leg["kind"] + "Float" + leg["metric"])(X16.astype(np.float32), labels, build_params=wa.BuildParams(R, L, ALPHA, cache), **kw)
        log(f"{name}: {HALF} index built in {build_s:.1f}s ({h.device_bytes() / 2**30:.2f} GiB); float32 index on the upcast points "
            f"opened the same graphs ({f.device_bytes() / 2**30:.2f} GiB)")

        sweep = []
        if args.setting:
            best = tuple(int(x) for x in args.setting.split(","))
        else:
            for beam in (10, 20, 40, 80, 160):
                for mult in (1, 2):
                    run(h, beam, mult)
                    t = time.perf_counter()
                    run(h, beam, mult)
                    ms = (time.perf_counter() - t) * 1e3
                    sweep.append(dict(beam=beam, mult=mult, recall_rounded_gt=round(recall(gt_rounded), 4), ms=round(ms, 3)))
            ok = [r for r in sweep if r["recall_rounded_gt"] >= 0.95]
            b = min(ok, key=lambda r: r["ms"]) if ok else max(sweep, key=lambda r: r["recall_rounded_gt"])
            best = (b["beam"], b["mult"])
        log(f"{name}: setting beam {best[0]} x{best[1]}")

        # rows: identical, and the same operation counts
        run(f, *best)
        fi, fd, fc_ = ids_t.clone(), dist_t.clone(), f.counters()
        run(h, *best)
        hc = h.counters()
        rows_identical = bool((ids_t == fi).all().item()) and bool((dist_t.view(torch.int32) == fd.view(torch.int32)).all().item())
        counters_equal = all(hc[k] == fc_[k] for k in ("beam_searches", "hops", "dist_cmps", "brute_rows"))
        rec16 = recall(gt_orig)
        rec16_rounded = recall(gt_rounded)

        # alternate: f32, f16, f32, f16, ... (each call host-synchronous: its counters are its own)
        times = {"float32": [], HALF: []}
        kms = {"float32": [], HALF: []}
        for _ in range(args.reps):
            for tag, index in (("float32", f), (HALF, h)):
                t = time.perf_counter()
                run(index, *best)
                times[tag].append((time.perf_counter() - t) * 1e3)
                kms[tag].append(index.counters()["search_kernel_ms"])
        res = dict(config=name, workload=f"{cfg['cls']} n={n} d={d} {'L2' if l2 else 'MIPS'} R={R} L={L} {kw} window 2^{leg['frac']} nq={nq} k={K}",
                   **{HALF + "_build_s": round(build_s, 1)}, setting=dict(beam=best[0], mult=best[1]), sweep=sweep,
                   rows_identical=rows_identical, counters_equal=counters_equal,
                   counters=dict((k, hc[k]) for k in ("beam_searches", "hops", "dist_cmps", "brute_rows", "label_reads", "spec_searches")))
        for tag, index, esz in (("float32", f, 4), (HALF, h, half_esz)):
            ms = float(np.median(times[tag]))
            km = float(np.mean(kms[tag]))
            gb = (4 * (R + 1) * hc["hops"] + esz * d * hc["dist_cmps"] + 4 * hc["label_reads"]) / 1e9
            res[tag] = dict(qps=round(nq / ms * 1e3), ms_per_batch=round(ms, 3), search_kernel_ms=round(km, 3),
                            search_kernel_ms_per_call=[round(x, 3) for x in kms[tag]], algorithmic_gb_per_batch=round(gb, 3),
                            hbm_share=round(gb / km / HBM_TBPS, 4) if km > 0 else None, device_bytes=int(index.device_bytes()))
        res[HALF]["recall_at_10_unrounded_gt"] = round(rec16, 4)
        res[HALF]["recall_at_10_rounded_gt"] = round(rec16_rounded, 4)
        res["speedup_qps"] = round(res[HALF]["qps"] / res["float32"]["qps"], 3)
        res["speedup_search_kernel"] = round(res["float32"]["search_kernel_ms"] / res[HALF]["search_kernel_ms"], 3)
        del f, h
        torch.cuda.empty_cache()
        if args.unrounded:  # the float32 index a user would otherwise run: unrounded points, its own graphs
            ucache = os.path.join(args.cache, f"{name}_float32_n{n}") + "/"
            os.makedirs(ucache, exist_ok=True)
            u = getattr(wa, leg["kind"] + "Float" + leg["metric"])(X, labels, build_params=wa.BuildParams(R, L, ALPHA, ucache), **kw)
            Qu = torch.from_numpy(Q).to(dev)
            run(u, *best, Qdev=Qu)
            res["float32_unrounded"] = dict(recall_at_10_unrounded_gt=round(recall(gt_orig), 4), device_bytes=int(u.device_bytes()))
            del u, Qu
        log(f"{name}: {json.dumps({k: res[k] for k in ('rows_identical', 'counters_equal', 'speedup_qps', 'speedup_search_kernel')})}")
        report["legs"].append(res)
        del X, Q, X16, Q16
        torch.cuda.empty_cache()
    report["all_rows_identical"] = all(r["rows_identical"] and r["counters_equal"] for r in report["legs"])
    print(json.dumps(report))
    return 0 if report["all_rows_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())

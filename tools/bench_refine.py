"""Refined search (wann_batch_search_device_refined) against the float32 index, on REAL-VALUED data: does a compact
index (float16 / bfloat16 / float8 rows: a half or a quarter of the float32 bytes per scored row) that re-ranks refine_k candidates
against the full-precision rows reach the float32 index's recall, and what does it cost?

Data: a GloVe-like synthetic set -- a Gaussian mixture with unit-scale elements, scaled by a power of two (2^5) into float8's
range (bench.py's own points are integers: they round to themselves and would show nothing).  Index: VamanaRangeFilterTreeIndex,
optimized_postfilter, window fraction 2^-3, k = 10.  Legs: the float32 index; then the Float16 / BFloat16 / Float8 index of the
rounded points unrefined and refined at refine_k = k, 2k, 4k.  The equal-recall legs ("stop as at k"): the
compact indexes refined at refine_k = 2k, 4k, 8k with stop_k = k -- the search of the unrefined leg, up to refine_k entries of its
last frontier re-ranked (wann_batch_search_device_refined_stop) -- and the float32 index at wider beams (`--float32-beams`), so that
a refined leg can be compared with a float32 leg of no higher recall.  All four indexes are resident and all legs ALTERNATE within
one job, `--reps` repetitions each.  Per repetition: device ms from HIP events (the
search's device_ms plus, for a refined leg, the re-rank launch's refine_ms), wall ms of the blocking device-buffer call; per leg
QPS from the median wall ms and recall@10 against the exact ground truth of the UNROUNDED points (float64, on the GPU).
A refined leg "wins" only if its recall is no lower than the float32 leg's at the same beam and every one of its repetitions
beats every float32 repetition (device ms); recalls are compared UNROUNDED (`recall_exact`; `neighbours_found` of
`neighbours_total` are the integers behind it -- four decimals cannot separate legs a few neighbours apart); `beats` lists every float32 leg (any beam) a refined leg wins against by that same
rule.  Prints one JSON object (profiles/refine_bench.json; with the equal-recall legs profiles/refine_stop_bench.json).
   python tools/bench_refine.py [--n 1000000] [--d 100] [--nq 10000] [--reps 3] [--setting 80,1] [--metric Euclidian]
                                [--float32-beams 100,120,160] [--stop-refine 2,4,8]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

K = 10
SCALE = 32.0  # 2^5: unit-scale elements reach about +-6 sigma = 192, inside float8's 448


def make_data(np, n, d, nq, seed=2026, latent=24, clusters=64):
    """rows of a Gaussian mixture in a `latent`-dimensional subspace plus isotropic noise, every element of about unit variance"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((latent, d)) / np.sqrt(latent)
    cent = rng.standard_normal((clusters, latent))

    def gen(m):
        z = cent[rng.integers(0, clusters, m)] * 0.8 + rng.standard_normal((m, latent)) * 0.6
        return ((z @ A + 0.3 * rng.standard_normal((m, d))) * SCALE).astype(np.float32)

    X, Q = gen(n), gen(nq)
    labels = ((rng.permutation(n) + 0.5) / n).astype(np.float32)
    return X, Q, labels


def ground_truth(torch, Xt, labt, Qt, Wt, k, mips):
    """exact filtered top-k of the unrounded points, float64 on the GPU: (ids, count of in-window points capped at k)"""
    nq = Qt.shape[0]
    X64 = Xt.double()
    x2 = None if mips else (X64 * X64).sum(1)
    out = torch.empty((nq, k), dtype=torch.int64, device=Xt.device)
    cnt = torch.empty((nq,), dtype=torch.int64, device=Xt.device)
    step = max(16, min(128, int(2**30 // (8 * Xt.shape[0]))))
    for a in range(0, nq, step):
        q = Qt[a:a + step].double()
        dmat = -(q @ X64.T) if mips else x2[None, :] - 2.0 * (q @ X64.T) + (q * q).sum(1, keepdim=True)
        mask = (labt[None, :] >= Wt[a:a + step, 0:1]) & (labt[None, :] <= Wt[a:a + step, 1:2])
        dmat.masked_fill_(~mask, float("inf"))
        vals, idx = torch.topk(dmat, k, dim=1, largest=False)
        idx[torch.isinf(vals)] = -1
        out[a:a + step] = idx
        cnt[a:a + step] = mask.sum(1).clamp(max=k)
    return out, cnt


def recall_hits(torch, gt, gcnt, ids):
    """(true neighbours found, true neighbours there are) over the batch: integers, so that two legs compare exactly"""
    ids64 = ids.to(torch.int64) & 0xFFFFFFFF
    hit = ((gt[:, :, None] == ids64[:, None, :]) & (gt[:, :, None] >= 0)).any(2).sum(1)
    return int(hit.sum().item()), int(gcnt.sum().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=100)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--fraction", type=int, default=-3)
    ap.add_argument("--setting", default="80,1", help="'beam,mult'")
    ap.add_argument("--metric", default="Euclidian", choices=("Euclidian", "Mips"))
    ap.add_argument("--types", default="Float16,BFloat16,Float8")
    ap.add_argument("--float32-beams", default="100,120,160", help="further float32 legs at these beams ('' = none)")
    ap.add_argument("--stop-refine", default="2,4,8", help="refined legs at stop_k = k and refine_k = these multiples of k ('' = none)")
    ap.add_argument("--out", default="", help="also write the JSON object to this file")
    args = ap.parse_args()
    reps = max(1, args.reps)
    os.environ.setdefault("PARLAY_NUM_THREADS", str(min(16, os.cpu_count() or 1)))
    import numpy as np
    import torch
    import rangefilteredann_amd  # noqa: F401
    import window_ann as wa
    import bench

    n, d, nq = args.n, args.d, args.nq
    beam, mult = (int(x) for x in args.setting.split(","))
    X, Q, labels = make_data(np, n, d, nq)
    W = bench.make_windows(np.sort(labels), nq, args.fraction, 2000 + args.fraction)
    dev = torch.device("cuda:0")
    Qt, Wt = torch.from_numpy(Q).to(dev), torch.from_numpy(W).to(dev)
    gt, gcnt = ground_truth(torch, torch.from_numpy(X).to(dev), torch.from_numpy(labels).to(dev), Qt, Wt, K, args.metric == "Mips")
    ids_t = torch.empty((nq, K), dtype=torch.int32, device=dev)
    dist_t = torch.empty((nq, K), dtype=torch.float32, device=dev)
    qps = {}

    def qp_at(b):
        if b not in qps:
            qps[b] = wa.QueryParams(K, b, 1.35, 10_000_000, 10_000, mult, 10_000, None, False)
        return qps[b]

    wide_beams = [int(x) for x in args.float32_beams.split(",") if x]
    stop_mults = [int(x) for x in args.stop_refine.split(",") if x]
    rounders = {"Float": lambda x: x, "Float16": lambda x: x.astype(np.float16).astype(np.float32), "BFloat16": wa.bfloat16_round,
                "Float8": wa.float8_round}
    legs, plans, build_s = {}, [], {}
    indexes = {}
    for typ in ["Float"] + [t for t in args.types.split(",") if t]:  # every index resident, so that all legs alternate
        t0 = time.time()
        idx = getattr(wa, "VamanaRangeFilterTreeIndex" + typ + args.metric)(rounders[typ](X), labels, cutoff=1000, split_factor=2,
                                                                           build_params=wa.BuildParams(64, 500, 1.0, ""))
        build_s[typ] = round(time.time() - t0, 1)
        indexes[typ] = idx
        # a plan: (tag, index, refine_k or 0, stop_k or None = the search at k = refine_k, beam)
        plans.append((typ if typ != "Float" else "Float32", typ, 0, None, beam))
        if typ != "Float":
            idx.set_refine_rows(X)
            plans += [(f"{typ}+refine{r}", typ, r, None, beam) for r in (K, 2 * K, 4 * K)]
            plans += [(f"{typ}+refine{m * K}@stop{K}", typ, m * K, K, beam) for m in stop_mults]
        else:
            plans += [(f"Float32@beam{b}", typ, 0, None, b) for b in wide_beams]

    def run(typ, refine_k, stop_k, b):
        idx = indexes[typ]
        if refine_k:
            idx.batch_search_device_refined(Qt.data_ptr(), Wt.data_ptr(), nq, 0, "optimized_postfilter", qp_at(b), refine_k, ids_t.data_ptr(),
                                            dist_t.data_ptr(), 0, stop_k=stop_k)
        else:
            idx.batch_search_device(Qt.data_ptr(), Wt.data_ptr(), nq, 0, "optimized_postfilter", qp_at(b), ids_t.data_ptr(), dist_t.data_ptr(), 0)

    for tag, typ, r, stop_k, b in plans:  # warm-up, recall, counters
        run(typ, r, stop_k, b)
        run(typ, r, stop_k, b)
        torch.cuda.synchronize()
        idx = indexes[typ]
        c = idx.counters()
        recall = bench.recall_of(torch, gt, gcnt, ids_t)  # (the mean over queries; recall_exact is compared, recall_at_10 is for reading)
        hits, slots = recall_hits(torch, gt, gcnt, ids_t)
        legs[tag] = dict(refine_k=r, stop_k=(stop_k if stop_k else r) if r else 0, beam=b, recall_at_10=round(recall, 4), recall_exact=recall,
                         neighbours_found=hits, neighbours_total=slots, hops=c["hops"], dist_cmps=c["dist_cmps"],
                         beam_searches=c["beam_searches"], device_bytes=int(idx.device_bytes()), refine_rows_bytes=int(idx.refine_rows_bytes()),
                         build_s=build_s[typ], device_ms=[], search_ms=[], refine_ms=[], wall_ms=[])
    for _ in range(reps):
        for tag, typ, r, stop_k, b in plans:
            torch.cuda.synchronize()
            t = time.perf_counter()
            run(typ, r, stop_k, b)
            wall = (time.perf_counter() - t) * 1e3
            search = indexes[typ].counters()["device_ms"]
            refine = indexes[typ].refine_counters()["refine_ms"] if r else 0.0
            leg = legs[tag]
            leg["wall_ms"].append(round(wall, 3))
            leg["search_ms"].append(round(search, 3))
            leg["refine_ms"].append(round(refine, 4))
            leg["device_ms"].append(round(search + refine, 3))
    f32 = legs["Float32"]
    for tag, leg in legs.items():
        leg["qps"] = round(nq / float(np.median(leg["wall_ms"])) * 1e3)
        leg["device_ms_median"] = round(float(np.median(leg["device_ms"])), 3)
        if not tag.startswith("Float32"):
            leg["recall_not_lower_than_float32"] = bool(leg["recall_exact"] >= f32["recall_exact"])
            leg["every_rep_beats_every_float32_rep"] = bool(max(leg["device_ms"]) < min(f32["device_ms"]))
            leg["wins"] = bool(leg["refine_k"] > 0 and leg["recall_not_lower_than_float32"] and leg["every_rep_beats_every_float32_rep"])
            # the same rule against every float32 leg: the one at the same beam and the ones at wider beams
            leg["beats"] = [t for t, o in legs.items() if t.startswith("Float32") and leg["refine_k"] > 0 and
                            leg["recall_exact"] >= o["recall_exact"] and max(leg["device_ms"]) < min(o["device_ms"])]
    res = dict(tool="tools/bench_refine.py",
               workload=f"VamanaRangeFilterTreeIndex*{args.metric} n={n} d={d} R=64 L=500 cutoff=1000 split=2 optimized_postfilter window 2^{args.fraction} "
                        f"nq={nq} k={K}; Gaussian mixture x {SCALE:g}",
               setting=dict(beam=beam, mult=mult), reps=reps, legs=legs)
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

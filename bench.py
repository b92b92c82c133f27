#!/usr/bin/env python3
"""bench.py -- the reference's headline benchmark on MI355X: window-filtered batch_search QPS at
recall@10 >= 0.95 (BASELINE.json metric), on BASELINE.json configs[1]: SIFT-1M-like (n = 10^6,
d = 128, squared L2), 2-ary window search tree (cutoff 1000, R = 64, L = 500, alpha = 1),
query method "optimized_postfilter", 10 000 queries per GPU, k = 10.

  python bench.py --gpus N --steps K --warmup W [--scaling weak|strong] [--full]

N > 1: one process per GPU.  Either the caller starts the ranks (python -m torch.distributed.run
--nproc-per-node N ... bench.py --gpus N: RANK / LOCAL_RANK / WORLD_SIZE in the environment), or --
when WORLD_SIZE is unset -- this script starts them itself as a torch.distributed.run CHILD process
before anything here has touched the GPU and relays the child's JSON line.

A "step" is one sharded batch_search (rangefilteredann_amd.distributed.sharded_batch_search) over
the job's query batch -- queries, windows and outputs resident in HBM -- at the fastest sweep
setting whose recall@10 exceeds 0.95 at window fraction 2^-3 (experiments/create_table.py:23-28:
QPS@recall = max qps over settings with recall > tau).  The index is replicated on every GPU, the
batch is cut into contiguous per-rank shards that keep their global query numbers, and the per-shard
top-k are exchanged with ONE RCCL all-gather inside the timed region.
  --scaling weak   (default) 10 000 queries PER GPU: the job's batch is N x 10 000 queries
  --scaling strong ONE 10 000-query batch cut N ways (1 250 queries per GPU at N = 8)

Rank 0 prints ONE JSON line.  Besides the contract's keys it carries `config` (the setting, recall@10 of
the timed setting, index size) and
  roofline      algorithmic bytes of the beam-search kernel / its HIP-event time vs 8 TB/s HBM
A plain run does only what that line needs: data, index, the headline sweep, the warm-up and timed steps,
--dump-outputs and the line.  Its index is built in memory, without graph files (N > 1 --workload deep
excepted: rank 0 builds into --cache, the other ranks load its files).  Everything else runs with --full
(N = 1 only):
  cpu_baseline  the REAL reference (oracle/_ref build) -- or the oracle port -- timed on this
                box's host cores on the same batch and setting, same graphs (--no-cpu-baseline: skip)
  per_fraction  QPS@recall>=0.95 for all 17 window fractions 2^-16..2^0 (device time; --fractions)
  configs       the other BASELINE.json configurations (--configs)
  config.same_batch_*, config.pipelined (--pipeline), config.host_buffer_*: the same-batch replay, the
                asynchronous call with batches in flight, the reference's numpy-in / numpy-out boundary
With --full the index's graph files go to --cache, where the reference legs load them.  --fractions,
--configs and --pipeline choose among these legs; asking for one without --full is an error.
per_fraction and configs are summarised on stdout (the line stays below LINE_BUDGET characters);
the full record goes to stderr as `[bench] full: {...}`.

  --dump-outputs DIR  after the timed steps, rank 0 writes the rows the LAST timed step returned:
                      DIR/ids.npy (float64; the uint32 ids) and DIR/dists.npy (float32), (rows, k).
                      Above DUMP_BUDGET bytes a fixed, seeded sample of rows is written, with its
                      row numbers in DIR/rows.npy.  Same arguments = same inputs, run after run.
Data are synthetic (no network): seeds and laws in SURVEY.md 8(d).
"""
import argparse
import contextlib
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

K = 10
# experiments/run_our_method.py:32-33: beam x final_beam_multiply grid of the reference's sweep
BEAM_SIZES = [10, 20, 40, 80, 160, 320, 640, 1280]
FINAL_MULTIPLIES = [1, 2, 3, 4, 8, 16, 32]
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
LINE_BUDGET = 6000     # characters of the stdout JSON line (readers keep the last 8 000 characters of stdout)
DUMP_BUDGET = 64 << 20  # bytes of --dump-outputs


def log(*a):
    if int(os.environ.get("RANK", "0")) == 0:
        print("[bench]", *a, file=sys.stderr, flush=True)


@contextlib.contextmanager
def quiet_stdout():
    sys.stdout.flush()
    saved = os.dup(1)
    dn = os.open(os.devnull, os.O_WRONLY)
    os.dup2(dn, 1)
    try:
        yield
    finally:
        sys.stdout.flush()
        os.dup2(saved, 1)
        os.close(saved)
        os.close(dn)


def make_data(n, d, nq, draws=1):
    """Points, `draws` consecutive query batches of nq rows (concatenated) and labels: the same on every rank."""
    import numpy as np
    from util import sift_like
    g = sift_like(n, d, 1234)
    X = g(n)
    Q = np.concatenate([g(nq) for _ in range(max(1, draws))])
    rng = np.random.default_rng(4321)
    labels = ((rng.permutation(n) + 0.5) / n).astype(np.float32)
    return X, Q, labels


def make_data_deep(n, d, nq, draws=1):
    """BASELINE.json configs[3] ("deep-10M-like": unit-norm mixture rows, inner product) -- the law and seeds of
    tools/bench_configs.py --config deep."""
    import numpy as np
    from util import unit_mixture
    g = unit_mixture(n, d, 2025)
    X = g(n)
    Q = np.concatenate([g(nq) for _ in range(max(1, draws))])
    labels = ((np.random.default_rng(77).permutation(n) + 0.5) / n).astype(np.float32)
    return X, Q, labels


# --workload: what a step searches.  "sift" = BASELINE.json configs[1] (the metric's configuration); "deep" = configs[3], the
# workload the baseline names for the 8-GPU run (the same launcher, sharding and all-gather).
WORKLOADS = {
    "sift": dict(make=make_data, n=1_000_000, d=128, metric="l2", cls="VamanaRangeFilterTreeIndexFloatEuclidian", cutoff=1000, split=2,
                 R=64, L=500, alpha=1.0, method="optimized_postfilter", label="SIFT-1M-like", dist="L2", cache="siftlike", shared_cache=False),
    "deep": dict(make=make_data_deep, n=9_990_000, d=96, metric="mips", cls="VamanaRangeFilterTreeIndexFloatMips", cutoff=1000, split=4,
                 R=64, L=500, alpha=1.0, method="optimized_postfilter", label="deep-10M-like", dist="MIPS", cache="deeplike", shared_cache=True),
}


def make_windows(labels_sorted, nq, p, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    n = len(labels_sorted)
    w = int(n * 2.0 ** p)
    out = np.zeros((nq, 2), dtype=np.float32)
    if w >= n - 2:
        out[:, 0] = labels_sorted[0] - 1
        out[:, 1] = labels_sorted[-1] + 1
        return out
    w = max(w, 1)
    st = rng.integers(1, n - w - 1, size=nq)
    out[:, 0] = labels_sorted[st]
    out[:, 1] = labels_sorted[st + w]
    return out


def ground_truth(torch, Xt, x2, labt, Qt, Wt, k):
    """Exact filtered top-k on the GPU (integer-valued data: fp32 arithmetic is exact).  x2 = None: inner-product distance."""
    nq = Qt.shape[0]
    out = torch.empty((nq, k), dtype=torch.int64, device=Xt.device)
    cnt = torch.empty((nq,), dtype=torch.int64, device=Xt.device)
    step = max(16, min(256, int(2**31 // (4 * Xt.shape[0]))))
    for a in range(0, nq, step):
        q = Qt[a:a + step]
        dmat = -(q @ Xt.T) if x2 is None else x2[None, :] - 2.0 * (q @ Xt.T) + (q * q).sum(1, keepdim=True)
        mask = (labt[None, :] >= Wt[a:a + step, 0:1]) & (labt[None, :] <= Wt[a:a + step, 1:2])
        dmat.masked_fill_(~mask, float("inf"))
        vals, idx = torch.topk(dmat, k, dim=1, largest=False)
        idx[torch.isinf(vals)] = -1
        out[a:a + step] = idx
        cnt[a:a + step] = mask.sum(1).clamp(max=k)
    return out, cnt


def recall_of(torch, gt, gcnt, ids):
    """mean over queries of |gt ∩ res[:k]| / |gt|  (experiments/run_our_method.py:174-180)"""
    ids64 = ids.to(torch.int64) & 0xFFFFFFFF
    hit = ((gt[:, :, None] == ids64[:, None, :]) & (gt[:, :, None] >= 0)).any(2).sum(1)
    valid = gcnt > 0
    return float((hit[valid].double() / gcnt[valid].double()).mean().item())


def dump_outputs(out_dir, ids, dists, budget=DUMP_BUDGET):
    """--dump-outputs: the (rows, k) result of one step as DIR/ids.npy (float64 of the uint32 ids: exact) and DIR/dists.npy
    (float32); a batch above `budget` bytes is cut to a sample of rows drawn with a fixed seed, listed in DIR/rows.npy."""
    import numpy as np
    ids = np.ascontiguousarray(ids).view(np.uint32).astype(np.float64)
    dists = np.ascontiguousarray(dists, dtype=np.float32)
    nrows, k = ids.shape
    per_row = 12 * k + 8  # ids + dists + the row number when sampled
    files = {}
    if nrows * 12 * k > budget:
        rows = np.sort(np.random.default_rng(0).choice(nrows, budget // per_row, replace=False))
        files["rows"] = rows.astype(np.float64)
        ids, dists = ids[rows], dists[rows]
    files["ids"], files["dists"] = ids, dists
    os.makedirs(out_dir, exist_ok=True)
    for name, a in files.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return {name: a.shape for name, a in files.items()}


def stdout_line(result):
    """The JSON line for stdout: the contract's keys, `config`, `roofline` and `cpu_baseline` as they are; `per_fraction` and
    `configs` cut to a few numbers each (the full record goes to stderr)."""
    line = {k: v for k, v in result.items() if k not in ("per_fraction", "configs")}
    if result.get("per_fraction") is not None:
        keys = ("qps", "recall", "beam", "mult", "roofline_frac", "reference_qps", "rows_identical_ids")
        line["per_fraction"] = {p: {k: r[k] for k in keys if k in r} for p, r in result["per_fraction"].items()}
    if result.get("configs") is not None:
        cfgs = {}
        for name, r in result["configs"].items():
            if "error" in r:
                cfgs[name] = {"error": r["error"][-120:]}
                continue
            c = {k: r[k] for k in ("qps", "mfma_qps", "recall_at_10", "setting") if k in r}
            if isinstance(r.get("roofline"), dict):
                c["frac"] = r["roofline"].get("frac")
            refs = r.get("reference") or []
            if refs:
                c["same_ids"] = min(x.get("same_ids", 0.0) for x in refs)
            elif isinstance(r.get("cpu_reference"), dict):
                c["dists_identical"] = r["cpu_reference"].get("dists_identical")
            cfgs[name] = c
        line["configs"] = cfgs
    s = json.dumps(line)
    if len(s) > LINE_BUDGET and "per_fraction" in line:  # (never expected: drop the per-fraction table before the line overflows)
        line["per_fraction"] = {p: {k: r[k] for k in ("qps", "recall") if k in r} for p, r in line["per_fraction"].items()}
        s = json.dumps(line)
    return s


def free_port():
    import socket
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    return port


def launcher_cmd(n_ranks, argv, port):
    """The command this script runs as a child for --gpus N > 1 (the driver's own launch line)."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_ranks}",
            "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def spawn_ranks(n_ranks, argv):
    """Start the ranks as a CHILD process (this process has not imported torch or made a HIP call, and never
    replaces itself: exec from a GPU-initialised process is forbidden on the pool) and relay its output."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 1) // n_ranks)))
    proc = subprocess.run(launcher_cmd(n_ranks, argv, free_port()), env=env)
    return proc.returncode


def launch_check(args):
    """Self-test of the launch path without a GPU (tests/test_bench_launch.py): rendezvous on gloo, then one STEP of the job as the
    real run would cut it -- the workload's batch shape, weak / strong scaling, count- or cost-balanced shards -- through
    sharded_batch_search with a stand-in search function (row i = f(global query number)), the all-gather included; every rank
    checks every row.  Rank 0 prints a JSON line."""
    import torch
    import torch.distributed as dist
    from rangefilteredann_amd.distributed import shard_bounds, sharded_batch_search, weighted_bounds
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    got = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(got, torch.tensor([rank], dtype=torch.int64))
    wl = WORKLOADS[args.workload]
    gnq = (args.nq if args.nq != 10_000 else 1003) * (world if args.scaling == "weak" else 1)  # (an odd size: uneven shards)
    q = torch.arange(gnq * 4, dtype=torch.float32).reshape(gnq, 4)
    r = torch.zeros((gnq, 2), dtype=torch.float32)
    bounds = None
    if args.balance == "cost" and world > 1:
        bounds = weighted_bounds([1.0 + (i % 7 == 0) * 50.0 for i in range(gnq)], world)

    def fake(qs, rs, base):
        m = qs.shape[0]
        ids = (torch.arange(base, base + m, dtype=torch.int32)[:, None] * K + torch.arange(K, dtype=torch.int32)[None, :])
        return ids, ids.to(torch.float32) * 0.5
    if args.balance == "levels":
        # a stand-in ENGINE with the doubling loop's semantics (postfilter_vamana.h:161-181): query q finds its k entries from beam
        # 5 << (q % 4) on; a row says which query and which beam produced it
        fmax = float(torch.finfo(torch.float32).max)

        def row_of(qi, b):
            found = b >= (5 << (qi % 4))
            ids = torch.full((K,), 0, dtype=torch.int32)
            ds = torch.full((K,), fmax, dtype=torch.float32)
            m = K if found else 3
            ids[:m] = torch.arange(m, dtype=torch.int32) + qi * 100000 + b
            ds[:m] = torch.arange(m, dtype=torch.float32) + b
            return ids, ds, found

        def engine(qi, b, mb, m):
            ids, ds, found = torch.zeros(K, dtype=torch.int32), torch.full((K,), fmax), False
            while not found and b < mb:
                ids, ds, found = row_of(qi, b)
                if not found:
                    b *= 2
            fb = min(b * m, mb)
            if fb > b:
                ids, ds, _ = row_of(qi, fb)
            return ids, ds

        def run_group(qn, b, mb, m):
            rows_ = [engine(int(x), b, mb, m) for x in qn.tolist()]
            return torch.stack([a for a, _ in rows_]), torch.stack([d_ for _, d_ in rows_])
        from rangefilteredann_amd.distributed import level_dealt_batch_search
        levels = [1 + (i * 7) % 5 for i in range(gnq)]
        ids, dists = level_dealt_batch_search(run_group, gnq, K, 5, 10000, 2, levels)
        want_rows = [engine(i, 5, 10000, 2) for i in range(gnq)]
        ok = torch.tensor([int(all(bool((ids[i] == a).all()) and bool((dists[i] == d_).all()) for i, (a, d_) in enumerate(want_rows)))])
    else:
        ids, dists = sharded_batch_search(fake, q, r, K, bounds=bounds)
        want = torch.arange(gnq, dtype=torch.int32)[:, None] * K + torch.arange(K, dtype=torch.int32)[None, :]
        ok = torch.tensor([int(bool((ids == want).all()) and bool((dists == want.to(torch.float32) * 0.5).all()))])
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    if rank == 0:
        print(json.dumps({"launch_check": world, "ranks": [int(t.item()) for t in got], "workload": wl["label"], "scaling": args.scaling,
                          "shard_cut": args.balance, "batch": gnq, "shards": [b - a for a, b in (bounds or [shard_bounds(gnq, world, x) for x in range(world)])],
                          "rows_ok_on_every_rank": bool(ok.item())}), flush=True)
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                    help="weak: --nq queries per GPU; strong: ONE --nq-query batch cut across the GPUs")
    ap.add_argument("--workload", choices=tuple(WORKLOADS), default="sift",
                    help="sift = BASELINE.json configs[1] (the metric's configuration); deep = configs[3] (deep-10M-like, 4-ary tree, inner product)")
    ap.add_argument("--n", "--points", dest="n", type=int, default=0)  # (--points: "--n" is an ambiguous prefix for torch.distributed.run)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--dim", type=int, default=0)
    ap.add_argument("--fraction", type=int, default=-3, help="headline window fraction exponent")
    ap.add_argument("--full", action="store_true",
                    help="N=1: also the CPU baseline, the other window fractions and configurations, the same-batch replay, batches in flight "
                         "and the host-buffer call (a plain run does only what the headline needs)")
    ap.add_argument("--fractions", default=None, help="with --full: 'all' = also sweep 2^-16..2^0 (N=1; default for sift), 'headline' = skip, "
                    "or a list of exponents '-9,-6'")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--setting", default="", help="'beam,mult': skip the sweep and time this setting (profiling runs)")
    ap.add_argument("--balance", choices=("count", "cost", "levels"), default="count",
                    help="shard cut of a step's batch: equal query counts; equal predicted work (wann_predict_costs + weighted_bounds; what "
                         "--scaling strong wants: the step takes as long as its slowest shard); or `levels`: no query shards at all -- the "
                         "single doubling levels of every chain are dealt to the ranks (level_dealt_batch_search, wann_batch_search_device_ids)")
    ap.add_argument("--pipeline", type=int, default=None, help="with --full, N = 1: also time the rotating batches through the ASYNCHRONOUS call, this "
                    "many in flight (wann_batch_search_device_async; reported as config.pipelined, never as `value`); default 2; 0 / 1 = skip")
    ap.add_argument("--rotate", type=int, default=4, help="distinct query / window draws the timed steps rotate through (1 = the same batch every step)")
    ap.add_argument("--cache", default=os.environ.get("WANN_BENCH_CACHE", "/tmp/wann_bench_cache"))
    ap.add_argument("--configs", default=None, help="with --full, N=1: the other BASELINE.json configurations as extra legs of the line: 'all' = glove "
                    "(configs[2]), deep (configs[3] on this one GPU), adverse (configs[4]), sift_u8 / fenwick / three_split (SURVEY.md 8(f)-4 / 8(f)-2 at "
                    "configs[1] size); 'none'; or a comma list (also: deep_l2 = configs[3] under squared L2)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the rows the last timed step returned to DIR/ids.npy (float64) and DIR/dists.npy (float32)")
    ap.add_argument("--launch-check", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    wl = WORKLOADS[args.workload]
    args.n = args.n or wl["n"]
    args.dim = args.dim or wl["d"]
    if not args.full:  # a plain run: the headline alone; the legs beyond it need --full
        extra = []
        if args.fractions not in (None, "headline"):
            extra.append("--fractions " + args.fractions)
        if args.configs not in (None, "none"):
            extra.append("--configs " + args.configs)
        if args.pipeline is not None and args.pipeline >= 2:
            extra.append(f"--pipeline {args.pipeline}")
        if extra:
            ap.error(f"{', '.join(extra)}: legs beyond the headline run with --full only")
        args.fractions, args.configs, args.pipeline = "headline", "none", 0
    if args.fractions is None:
        args.fractions = "all" if args.workload == "sift" else "headline"
    if args.configs is None:
        args.configs = "all" if args.workload == "sift" else "none"
    if args.pipeline is None:
        args.pipeline = 2

    # ---- N > 1 without a launcher: start the ranks ourselves, BEFORE torch / HIP are touched in this process
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(spawn_ranks(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    if args.launch_check:
        return launch_check(args)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    ncpu = os.cpu_count() or 1
    os.environ.setdefault("PARLAY_NUM_THREADS", str(max(1, ncpu // world)))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ["WANN_DEVICE"] = str(local_rank)
    if args.pipeline > 2:  # (the asynchronous call's lanes are created at its first use: a lane per batch in flight)
        os.environ["WANN_ASYNC_LANES"] = str(min(4, args.pipeline))

    import numpy as np
    import torch
    import torch.distributed as dist
    import rangefilteredann_amd  # noqa: F401  (fails loudly when the HIP extension is missing)
    import window_ann as wa
    from rangefilteredann_amd.distributed import level_dealt_batch_search, levels_from_costs, shard_bounds, sharded_batch_search, weighted_bounds

    assert torch.cuda.is_available() and wa.device_count() > local_rank, "bench.py needs MI355X GPUs"
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    distributed = "WORLD_SIZE" in os.environ  # started by a launcher (also at N = 1): the RCCL path runs
    if distributed:
        dist.init_process_group("nccl", device_id=dev)

    n, d = args.n, args.dim
    draws = world if args.scaling == "weak" else 1
    rot = max(1, args.rotate)
    gnq = args.nq * draws                      # the job's batch
    lo, hi = shard_bounds(gnq, world, rank)    # this rank's shard (global query numbers)
    nq = hi - lo
    R, L, alpha, cutoff, split = wl["R"], wl["L"], wl["alpha"], wl["cutoff"], wl["split"]
    method = wl["method"]
    t0 = time.time()
    X, Qall, labels = wl["make"](n, d, args.nq, draws * rot)   # `rot` batches: the timed steps rotate through them
    Qg = Qall[:gnq]
    log(f"data n={n} d={d} batch={gnq} ({args.scaling} scaling, {world} rank(s)) in {time.time() - t0:.1f}s; host cpus={ncpu}")

    # graph files only where something reads them: the reference legs of --full, the other ranks of a shared build.  A plain
    # single-GPU run builds its graphs in memory -- the same graphs, byte for byte -- and reads nothing an earlier run wrote.
    cache = os.path.join(args.cache, f"{wl['cache']}_n{n}_d{d}_R{R}_L{L}_c{cutoff}_s{split}") + "/"
    if args.full or (world > 1 and wl["shared_cache"]):
        os.makedirs(cache, exist_ok=True)
    bp = wa.BuildParams(R, L, alpha, cache if args.full or world > 1 else "")
    t0 = time.time()
    make_index = lambda params: getattr(wa, wl["cls"])(X, labels, cutoff=cutoff, split_factor=split, build_params=params)  # noqa: E731
    if world > 1 and wl["shared_cache"]:
        # a big index (deep: 21 845 graphs, two minutes on one GPU): rank 0 builds it once into the shared graph cache
        # (the reference's file format), the other ranks load the files -- not N concurrent builds
        index = make_index(bp) if rank == 0 else None
        dist.barrier()
        if rank != 0:
            index = make_index(bp)
    elif world > 1:  # every rank builds its replica on its own GPU (seconds); no shared cache files
        index = make_index(wa.BuildParams(R, L, alpha, ""))
    else:
        index = make_index(bp)
    build_s = time.time() - t0
    log(f"index ready in {build_s:.1f}s: levels {index.levels()}, {index.device_bytes() / 2**30:.2f} GiB in HBM")

    Xt = torch.from_numpy(X).to(dev)
    x2 = (Xt * Xt).sum(1) if wl["metric"] == "l2" else None
    labt = torch.from_numpy(labels).to(dev)
    Qgt = torch.from_numpy(Qg).to(dev)         # the whole batch on every rank (sharded_batch_search's contract)
    Q, Qt = Qg[lo:hi], Qgt[lo:hi]
    ls = np.sort(labels)
    ids_t = torch.empty((nq, K), dtype=torch.int32, device=dev)
    dist_t = torch.empty((nq, K), dtype=torch.float32, device=dev)

    def qparams(mod, beam, mult):
        return mod.QueryParams(K, beam, 1.35, 10_000_000, 10_000, mult, 10000, None, False)

    def global_windows(p, seed, rotation=0):
        """windows of the whole batch: draw r uses seed + r (a weak-scaling rank's shard is one draw); rotation j > 0 = another draw"""
        return np.concatenate([make_windows(ls, args.nq, p, seed + r + 7919 * rotation) for r in range(draws)])

    def run(Wt, beam, mult):
        """this rank's shard through the device-pointer C-ABI entry point"""
        index.batch_search_device(Qt.data_ptr(), Wt.data_ptr(), nq, lo, method, qparams(wa, beam, mult),
                                  ids_t.data_ptr(), dist_t.data_ptr(), 0)

    def sweep(p, seed):
        Wg = global_windows(p, seed)
        Wgt = torch.from_numpy(Wg).to(dev)
        Wt = Wgt[lo:hi]
        gt, gcnt = ground_truth(torch, Xt, x2, labt, Qt, Wt, K)
        # the reference's whole grid, walked like its driver walks it: for each beam the multipliers in increasing order
        # until should_break (run_our_method.py:186-203: recall > 0.999, or no better than the previous multiplier).
        # One pruning on top: once a setting has recall > 0.95, a beam whose x1 run is 3x slower than the best such
        # setting ends the walk (larger beams only get slower: QPS@recall is a maximum of QPS).
        rows = []
        best_ok = None
        for beam in BEAM_SIZES:
            prev = None
            for mult in FINAL_MULTIPLIES:
                run(Wt, beam, mult)  # warm
                t = time.perf_counter()
                run(Wt, beam, mult)
                wall = time.perf_counter() - t
                c = index.counters()
                rec = recall_of(torch, gt, gcnt, ids_t)
                rows.append(dict(beam=beam, mult=mult, recall=rec, wall_ms=wall * 1e3, device_ms=c["device_ms"], kernel_ms=c["search_kernel_ms"],
                                 alg_bytes=4 * (R + 1) * c["hops"] + 4 * d * (c["dist_cmps"] + c["brute_rows"]) + 4 * c["label_reads"]))
                if rec > 0.95 and (best_ok is None or wall * 1e3 < best_ok):
                    best_ok = wall * 1e3
                scans_only = c["beam_searches"] == 0 and c["brute_rows"] > 0
                if scans_only or rec > 0.999 or (prev is not None and rec <= prev and mult != 1):
                    break
                prev = rec
            if scans_only:  # every window of this fraction takes the exact scan: beam and multiplier change nothing -- one setting
                break
            first = next(r for r in rows if r["beam"] == beam and r["mult"] == 1)
            if best_ok is not None and first["wall_ms"] > 3 * best_ok:
                break
        ok = [r for r in rows if r["recall"] > 0.95]
        # one timed run per setting is noisy where two settings are within a few per cent of each other (2^-8: (40, x1),
        # (80, x1), (160, x1)): the three fastest are timed three more times each before one is picked
        for r in sorted(ok, key=lambda r: r["wall_ms"])[:3]:
            for _ in range(3):
                t = time.perf_counter()
                run(Wt, r["beam"], r["mult"])
                r["wall_ms"] = min(r["wall_ms"], (time.perf_counter() - t) * 1e3)
                r["device_ms"] = min(r["device_ms"], index.counters()["device_ms"])
        best = min(ok, key=lambda r: r["wall_ms"]) if ok else None
        return Wg, Wgt, rows, best

    # ---- headline fraction: pick the setting, then time K steps
    t0 = time.time()
    if args.setting:
        sb, sm = (int(x) for x in args.setting.split(","))
        Wg = global_windows(args.fraction, 1000)
        Wgt = torch.from_numpy(Wg).to(dev)
        rows, best = [], dict(beam=sb, mult=sm, recall=float("nan"), wall_ms=0.0, device_ms=0.0)
    else:
        Wg, Wgt, rows, best = sweep(args.fraction, 1000)
    W, Wt = Wg[lo:hi], Wgt[lo:hi]
    for r in rows:
        log(f"  2^{args.fraction}: beam {r['beam']:4d} x{r['mult']}  recall {r['recall']:.4f}  {r['wall_ms']:.2f} ms  -> {nq / r['wall_ms'] * 1e3:,.0f} QPS")
    if best is None:
        best = max(rows, key=lambda r: r["recall"])
        log("WARNING: no sweep setting reached recall 0.95; timing the most accurate one")
    beam, mult = best["beam"], best["mult"]
    log(f"setting ({beam}, x{mult}) picked in {time.time() - t0:.1f}s")
    if distributed:  # every rank must time the same setting: take rank 0's choice
        bm = torch.tensor([beam, mult], device=dev)
        dist.broadcast(bm, 0)
        beam, mult = int(bm[0]), int(bm[1])

    agg = dict(beam_searches=0, hops=0, dist_cmps=0, label_reads=0, brute_rows=0, search_kernel_ms=0.0, device_ms=0.0, rounds=0,
               poll_timeouts=0, recovered_continuations=0)
    qp_run = qparams(wa, beam, mult)
    # the batches the timed steps rotate through: rotation 0 is the batch the sweep ran on; the others are fresh query AND window
    # draws (a step that replays one batch finds the upper tree levels' nodes cache-warm from the step before)
    rot_q = [Qgt] + [torch.from_numpy(Qall[j * gnq:(j + 1) * gnq]).to(dev) for j in range(1, rot)]
    rot_w = [Wgt] + [torch.from_numpy(global_windows(args.fraction, 1000, j)).to(dev) for j in range(1, rot)]
    # the shard cut of every rotation: equal counts, or equal predicted work (the same cut on every rank: same windows, same index)
    rot_bounds = [None] * rot
    if args.balance == "cost" and world > 1:
        rot_bounds = [weighted_bounds(index.predict_costs(w.cpu().numpy(), method, qp_run), world) for w in rot_w]
        log("cost-balanced shards (rotation 0):", [b - a for a, b in rot_bounds[0]])

    def search_fn(q, r, base, out_ids=None, out_dists=None):
        """local search of one shard: (nq_shard, d) / (nq_shard, 2) device tensors, global number of its first query; the rows
        go straight into the buffers the caller hands over (the all-gather's send planes)"""
        m = q.shape[0]
        oi = ids_t[:m] if out_ids is None else out_ids
        od = dist_t[:m] if out_dists is None else out_dists
        index.batch_search_device(q.data_ptr(), r.data_ptr(), m, base, method, qp_run, oi.data_ptr(), od.data_ptr(), 0)
        c = index.counters()
        for kk in agg:
            agg[kk] += c[kk]
        return oi, od

    rot_levels = None
    if args.balance == "levels":  # predicted doubling levels per query (the same on every rank); any prediction gives the same rows
        rot_levels = [levels_from_costs(index.predict_costs(w.cpu().numpy(), method, qp_run), beam) for w in rot_w]

    def run_group(qn, b, mb, m, j):
        """the queries numbered qn of rotation j's batch, each under its own global number, one post-filter chain started at beam b"""
        qs, ws = rot_q[j][qn].contiguous(), rot_w[j][qn].contiguous()
        ri = torch.empty((qn.shape[0], K), dtype=torch.int32, device=dev)
        rd = torch.empty((qn.shape[0], K), dtype=torch.float32, device=dev)
        index.batch_search_device_ids(qs.data_ptr(), ws.data_ptr(), qn.shape[0], qn.contiguous().data_ptr(), method,
                                      wa.QueryParams(K, b, 1.35, 10_000_000, 10_000, m, mb, None, False), ri.data_ptr(), rd.data_ptr(), 0)
        c = index.counters()
        for kk in agg:
            agg[kk] += c[kk]
        return ri, rd

    def step(j=0):
        if rot_levels is not None:  # strong scaling below the query: single doubling levels dealt to the ranks, two all-gathers
            return level_dealt_batch_search(lambda qn, b, mb, m: run_group(qn, b, mb, m, j), gnq, K, beam, 10000, mult, rot_levels[j], device=dev)
        # query shards -> HIP batch_search on this rank's GPU -> ONE all-gather of the per-shard top-k over RCCL/xGMI
        return sharded_batch_search(search_fn, rot_q[j], rot_w[j], K, bounds=rot_bounds[j])

    def timed(rotating):
        """exactly args.steps steps between barrier + synchronize on both sides; MAX over the ranks"""
        for i in range(args.warmup):
            step(i % rot if rotating else 0)
        if distributed:
            dist.barrier()
        torch.cuda.synchronize()
        for kk in agg:
            agg[kk] = 0
        t0 = time.perf_counter()
        for i in range(args.steps):
            out = step(i % rot if rotating else 0)
        torch.cuda.synchronize()
        if distributed:
            dist.barrier()
        el = time.perf_counter() - t0
        if distributed:
            te = torch.tensor([el], dtype=torch.float64, device=dev)
            dist.all_reduce(te, op=dist.ReduceOp.MAX)
            el = float(te.item())
        return el, out, dict(agg)

    # --full: the same batch every step (rounds 1-3 timed this) -- reported beside `value`; then THE timed region: rotating batches
    same_elapsed, _, same_agg = timed(False) if args.full and rot > 1 else (None, None, None)
    elapsed, last_out, _ = timed(True)
    if args.dump_outputs and rank == 0:  # (every rank holds every row of the step)
        shapes = dump_outputs(args.dump_outputs, last_out[0].cpu().numpy(), last_out[1].cpu().numpy())
        log(f"outputs of timed step {args.steps} (rotation {(args.steps - 1) % rot}, beam {beam} x{mult}) -> {args.dump_outputs}: {shapes}")
    del last_out
    ms_per_step = elapsed / args.steps * 1e3
    qps = gnq * args.steps / elapsed
    timed_agg = dict(agg)
    all_ids, all_d = step(0)  # rows of rotation 0 for the recall / reference comparison below
    for kk in agg:
        agg[kk] = timed_agg[kk]
    # recall of the gathered result rows of this rank's shard (every rank holds every row), averaged over the ranks
    gt_l, gcnt_l = ground_truth(torch, Xt, x2, labt, Qt, Wt, K)
    final_recall = recall_of(torch, gt_l, gcnt_l, all_ids[lo:hi])
    if distributed:
        fr = torch.tensor([final_recall * nq, float(nq)], dtype=torch.float64, device=dev)
        dist.all_reduce(fr)
        final_recall = float(fr[0] / fr[1])
        sums = torch.tensor([float(agg[kk]) for kk in ("beam_searches", "hops", "dist_cmps", "label_reads", "rounds")] +
                            [agg["search_kernel_ms"], agg["device_ms"]], dtype=torch.float64, device=dev)
        mx = sums[5:].clone()
        dist.all_reduce(sums)                         # work counters: summed over the ranks
        dist.all_reduce(mx, op=dist.ReduceOp.MAX)     # kernel time: the slowest rank's
    # the asynchronous call (two batches in flight: batch i + 1 is routed and ramps up under batch i's tail) over the same rotating
    # batches -- beside `value` (the reference's protocol is one blocking call per batch), never as `value`
    pipe = None
    pouts = None

    def pipelined_rate(qs, ws, qp_, nsteps, warm, ref_rows=None):
        """`nsteps` batches (rotating through qs / ws) through the asynchronous call, two in flight; optionally the rows of one more
        qs[0] / ws[0] batch against `ref_rows` (the blocking call's)."""
        depth = max(2, min(4, args.pipeline))

        def go(ns):
            tickets, ctrs = [], []
            for i in range(ns):
                oi, od = pouts[i % len(pouts)]
                tickets.append(index.batch_search_device_async(qs[i % len(qs)].data_ptr(), ws[i % len(ws)].data_ptr(), nq, lo, method, qp_,
                                                               oi.data_ptr(), od.data_ptr(), 0))
                if i >= depth - 1:
                    ctrs.append(index.wait(tickets[i - (depth - 1)]))
            for t in tickets[len(ctrs):]:
                ctrs.append(index.wait(t))
            return ctrs
        torch.cuda.synchronize()
        go(max(2, warm))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        pc = go(nsteps)
        torch.cuda.synchronize()
        pel = time.perf_counter() - t1
        p_bytes = sum(4 * (R + 1) * c["hops"] + d * 4 * (c["dist_cmps"] + c["brute_rows"]) + 4 * c["label_reads"] for c in pc)
        rec = dict(in_flight=depth, qps=round(nq * nsteps / pel, 1), ms_per_step=round(pel / nsteps * 1e3, 4),
                   hbm_frac_of_wall=round(p_bytes / pel / 1e9 / HBM_PEAK_GBS, 4))
        if ref_rows is not None:
            index.wait(index.batch_search_device_async(qs[0].data_ptr(), ws[0].data_ptr(), nq, lo, method, qp_, pouts[0][0].data_ptr(), pouts[0][1].data_ptr(), 0))
            rec["rows_equal_blocking_call"] = bool((pouts[0][0] == ref_rows[0]).all().item()) and bool((pouts[0][1] == ref_rows[1]).all().item())
        return rec

    if rank == 0 and world == 1 and args.pipeline >= 2:
        pouts = [(torch.empty((nq, K), dtype=torch.int32, device=dev), torch.empty((nq, K), dtype=torch.float32, device=dev)) for _ in range(max(3, args.pipeline + 1))]
        pipe = pipelined_rate([q[lo:hi] for q in rot_q], [w[lo:hi] for w in rot_w], qp_run, args.steps, args.warmup, (all_ids[lo:hi], all_d[lo:hi]))
        log(f"pipelined: {pipe}")

    # the reference's own boundary (numpy in, numpy out): the same batch through the host-buffer entry point,
    # PCIe copies included -- reported beside `value`, never as `value` (--full)
    host_ms = None
    if args.full and rank == 0 and world == 1:
        Wn = W.astype(np.float32)
        index.batch_search(Q, Wn, nq, method, qparams(wa, beam, mult))
        t1 = time.perf_counter()
        for _ in range(5):
            index.batch_search(Q, Wn, nq, method, qparams(wa, beam, mult))
        host_ms = (time.perf_counter() - t1) / 5 * 1e3

    # B = 4(R+1)*hops + d*sizeof(T)*dist_cmps + 4*|beam_out|  per search.  N > 1: bytes of ALL ranks over
    # the slowest rank's kernel time = the job's aggregate rate, against N x the per-GPU peak.
    if distributed:
        hops_all, cmps_all, labs_all = float(sums[1]), float(sums[2]), float(sums[3])
        searches_all, rounds_all = float(sums[0]), float(sums[4]) / world
        kern_ms, dev_ms = float(mx[0]), float(mx[1])
    else:
        hops_all, cmps_all, labs_all = agg["hops"], agg["dist_cmps"], agg["label_reads"]
        searches_all, rounds_all = agg["beam_searches"], agg["rounds"]
        kern_ms, dev_ms = agg["search_kernel_ms"], agg["device_ms"]
    alg_bytes = 4 * (R + 1) * hops_all + d * 4 * cmps_all + 4 * labs_all
    kern_s = kern_ms / 1e3
    achieved = alg_bytes / kern_s / 1e9 if kern_s > 0 else 0.0
    traffic, traffic_source = measured_traffic(beam, mult, n, gnq // world, args.fraction)
    roofline = dict(bound="hbm", kernel="k_search", achieved=round(achieved, 1), peak=HBM_PEAK_GBS * world, unit="GB/s",
                    frac=round(achieved / (HBM_PEAK_GBS * world), 4), traffic=traffic, traffic_source=traffic_source,
                    algorithmic_bytes_per_step=int(alg_bytes / args.steps),
                    launches_per_step=rounds_all / args.steps,
                    kernel_ms_per_step=round(kern_ms / args.steps, 4),
                    device_ms_per_step=round(dev_ms / args.steps, 4),
                    searches_per_step=searches_all / args.steps, hops_per_step=hops_all / args.steps,
                    dist_cmps_per_step=cmps_all / args.steps)

    result = {
        "metric": "QPS @ recall@10>=0.95, window fraction 2^%d" % args.fraction, "value": round(qps, 1), "unit": "queries/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4),
        "higher_is_better": True, "scaling": args.scaling, "shard_cut": args.balance, "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"{wl['label']} n={n} d={d} {wl['dist']}, {split}-WST (cutoff {cutoff}, R={R}, L={L}, alpha={alpha}) {method}, "
                               f"window 2^{args.fraction}, {gnq} queries per step ({nq} on rank 0), k={K}",
                   "beam": beam, "final_beam_multiply": mult, "recall_at_10": round(final_recall, 4),
                   "build_s": round(build_s, 1), "index_gib": round(index.device_bytes() / 2**30, 2),
                   "rotating_batches": rot, "pipelined": pipe,
                   "same_batch_qps": None if same_elapsed is None else round(gnq * args.steps / same_elapsed, 1),
                   "same_batch_kernel_ms_per_step": None if same_agg is None else round(same_agg["search_kernel_ms"] / args.steps, 4),
                   "poll_timeouts": int(agg["poll_timeouts"]), "recovered_continuations": int(agg["recovered_continuations"]),
                   "host_buffer_call_ms": None if host_ms is None else round(host_ms, 3),
                   "host_buffer_qps": None if host_ms is None else round(nq / host_ms * 1e3, 1),
                   "parallelism": (f"replicated index x{world}, contiguous query shards, one RCCL all-gather of the per-shard top-k per step"
                                   if distributed else "1 GPU")},
        "roofline": roofline,
    }

    # ---- legs for the REAL reference (same graph files, same batches): the headline fraction at the GPU's setting and at the
    #      cheapest settings that reach recall 0.95 (the reference's own best setting need not be the GPU's), then every
    #      window fraction at its best setting.  GPU rows are kept per leg: the reference's must be identical.
    legs = {}

    def add_leg(name, Wn, b_, m_, ids_np, d_np):
        legs["W|" + name] = np.asarray(Wn, dtype=np.float32)
        legs["set|" + name] = np.array([b_, m_], dtype=np.int64)
        legs["ids|" + name] = ids_np
        legs["dists|" + name] = d_np

    want_ref = args.full and rank == 0 and world == 1 and not args.no_cpu_baseline
    head_names = []
    if want_ref:
        add_leg(f"h:{beam},{mult}", W, beam, mult, all_ids.cpu().numpy().view(np.uint32), all_d.cpu().numpy())
        head_names.append(f"h:{beam},{mult}")
        ok_rows = sorted((r for r in rows if r["recall"] > 0.95), key=lambda r: (r["beam"] * (1 + (r["mult"] if r["mult"] > 1 else 0)), r["beam"]))
        for r in ok_rows[:3]:
            nm = f"h:{r['beam']},{r['mult']}"
            if nm not in head_names:
                run(Wt, r["beam"], r["mult"])
                add_leg(nm, W, r["beam"], r["mult"], ids_t.cpu().numpy().view(np.uint32).copy(), dist_t.cpu().numpy().copy())
                head_names.append(nm)

    # ---- all 17 window fractions (configs[1]), device-resident, best setting per fraction
    per = None
    if rank == 0 and world == 1 and args.fractions != "headline":
        per = {}
        for p in (range(-16, 1) if args.fractions == "all" else [int(x) for x in args.fractions.split(",")]):
            Wp, Wpt, rws, b = sweep(p, 2000 + p)
            meets = b is not None
            if b is None:  # no setting of the sweep reaches recall 0.95 here (the reference does not either: same rows)
                b = max(rws, key=lambda r: r["recall"])
            per[f"2^{p}"] = dict(qps=round(nq / b["wall_ms"] * 1e3, 1), recall=round(b["recall"], 4), beam=b["beam"], mult=b["mult"],
                                 device_ms=round(b["device_ms"], 3), meets_recall=meets, settings_swept=len(rws),
                                 # algorithmic bytes of the call (graph rows + scored vectors, exact scans included)
                                 # over the WHOLE call's device time, against the 8 TB/s HBM peak
                                 algorithmic_gb=round(b["alg_bytes"] / 1e9, 3),
                                 roofline_frac=round(b["alg_bytes"] / (b["device_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if b["device_ms"] > 0 else None)
            # HBM bytes of the batch from the committed counter pass of this very leg (profiles/*_pmc_traffic.json), if there is one
            tr_p, src_p = measured_traffic(b["beam"], b["mult"], n, nq, p)
            per[f"2^{p}"]["traffic"] = tr_p
            if tr_p is not None:
                per[f"2^{p}"]["traffic_source"] = src_p
                per[f"2^{p}"]["traffic_over_algorithmic"] = round(tr_p / b["alg_bytes"], 3) if b["alg_bytes"] else None
            if pouts is not None and p in (-9, -6):
                # do two batches in flight buy anything where a batch ends with a few long chains?  (rows against the blocking call's)
                run(Wpt[lo:hi], b["beam"], b["mult"])
                blocking = (ids_t.clone(), dist_t.clone())
                pr = pipelined_rate([Qt], [Wpt[lo:hi]], qparams(wa, b["beam"], b["mult"]), 6 if args.pipeline <= 2 else 4 * args.pipeline, 2, blocking)
                pr["speedup_over_blocking"] = round(b["wall_ms"] / pr["ms_per_step"], 3)
                per[f"2^{p}"]["pipelined"] = pr
            log(f"  2^{p}: {per[f'2^{p}']}")
            if want_ref:
                run(Wpt[lo:hi], b["beam"], b["mult"])
                add_leg(f"f:{p}", Wp[lo:hi], b["beam"], b["mult"], ids_t.cpu().numpy().view(np.uint32).copy(), dist_t.cpu().numpy().copy())
        result["per_fraction"] = per

    # ---- CPU baseline: the REAL reference on this box's host cores
    if want_ref:
        try:
            result["cpu_baseline"] = cpu_baseline(np, args.workload, n, d, nq, cache, legs, head_names, f"h:{beam},{mult}", per)
        except Exception as e:  # never lose the GPU number to a baseline problem
            log("cpu baseline failed:", repr(e))
            result["cpu_baseline"] = None

    # ---- the other BASELINE.json configurations (parity cases at full size; each in a child process with its own index)
    if rank == 0 and world == 1 and args.configs != "none":
        want = ["glove", "deep", "adverse", "sift_u8", "fenwick", "three_split"] if args.configs == "all" else [c for c in args.configs.split(",") if c]
        del index, Xt, x2, labt  # HBM and host memory for the children's own data (deep: 24.6 GB of index)
        torch.cuda.empty_cache()
        result["configs"] = other_configs(want, args.cache, ncpu, cache if args.workload == "sift" and n == 1_000_000 and d == 128 else None)

    if rank == 0:
        log("full:", json.dumps(result))
        print(stdout_line(result), flush=True)
    if distributed:
        dist.destroy_process_group()


def other_configs(want, cache, ncpu, sift_cache=None):
    """BASELINE.json configs[2] (GloVe-like super tree, 2^-6), configs[3] (deep-10M-like 4-WST, 2^-3, here on ONE GPU) and
    configs[4] (adversarial data, PrefilterIndex on the dense MFMA path) as child processes (tools/bench_configs.py,
    tools/bench_prefilter.py): each builds its index on the GPU, sweeps against exact ground truth, times the best setting
    and -- glove / adverse -- times the REAL reference on the same graphs and batch (rows must be identical)."""
    import subprocess
    out = {}
    threads = str(min(32, ncpu))
    # (sift_u8 starts from the graph files the headline run left in its cache: the same graphs, see tools/bench_configs.py)
    child_env = dict(os.environ, WANN_BENCH_SIFT_CACHE=sift_cache) if sift_cache else None
    legs = {
        "glove": ("configs[2]", [os.path.join(REPO, "tools", "bench_configs.py"), "--config", "glove", "--threads", threads, "--seconds", "8",
                                 "--cache", os.path.join(cache, "cfg")]),
        "deep": ("configs[3] (one GPU)", [os.path.join(REPO, "tools", "bench_configs.py"), "--config", "deep", "--threads", threads, "--seconds", "8",
                                          "--cache", os.path.join(cache, "cfg")]),
        "adverse": ("configs[4]", [os.path.join(REPO, "tools", "bench_prefilter.py")]),
        # SURVEY.md 8(f)-2 / 8(f)-4, at configs[1] size: the tree's other two query methods and the byte variant of the headline workload
        "fenwick": ("8(f)-2: fenwick query method (range_filter_tree.h:297-401), 2-WST n=10^6", [os.path.join(REPO, "tools", "bench_configs.py"), "--config", "fenwick",
                    "--threads", threads, "--seconds", "6", "--cache", os.path.join(cache, "cfg")]),
        "three_split": ("8(f)-2: three_split query method (range_filter_tree.h:473-540), 2-WST n=10^6", [os.path.join(REPO, "tools", "bench_configs.py"), "--config",
                        "three_split", "--threads", threads, "--seconds", "6", "--cache", os.path.join(cache, "cfg")]),
        "sift_u8": ("8(f)-4: configs[1] with uint8 points (python_bindings.cpp:234-237)", [os.path.join(REPO, "tools", "bench_configs.py"), "--config", "sift_u8",
                    "--threads", threads, "--seconds", "6", "--cache", os.path.join(cache, "cfg")]),
        # not part of "all" (two and a half more minutes): configs[3] under squared L2, as BASELINE.json's text states it
        "deep_l2": ("configs[3] as its text states it (96-d L2; one GPU)", [os.path.join(REPO, "tools", "bench_configs.py"), "--config", "deep_l2", "--threads", threads,
                                                                            "--seconds", "8", "--cache", os.path.join(cache, "cfg")]),
    }
    for name in want:
        if name not in legs:
            continue
        label, cmd = legs[name]
        t0 = time.time()
        try:
            p = subprocess.run([sys.executable] + cmd, capture_output=True, text=True, timeout=1500, env=child_env)
            line = [l for l in p.stdout.splitlines() if l.startswith("{")]
            if p.returncode != 0 or not line:
                raise RuntimeError((p.stderr or "")[-600:])
            rec = json.loads(line[-1])
            rec.pop("sweep", None)
            rec["baseline_config"] = label
            rec["leg_wall_s"] = round(time.time() - t0, 1)
            if "algorithmic_gb_per_batch" in rec and rec.get("search_kernel_ms"):
                tr, src = config_traffic(name, rec.get("setting"))
                if rec.get("scan_gb_per_batch") and rec.get("device_ms"):
                    # fenwick / three_split: k_brute (the end scans) and k_search run side by side: both kernels' algorithmic bytes
                    # over the call's device time (the search launch's own event time covers the scans it shares the chip with)
                    gb = rec["algorithmic_gb_per_batch"] + rec["scan_gb_per_batch"]
                    ach = gb / rec["device_ms"] * 1e3
                    rec["roofline"] = dict(bound="hbm", kernel="k_search + k_brute (concurrent)", achieved=round(ach, 1), peak=HBM_PEAK_GBS, unit="GB/s",
                                           frac=round(ach / HBM_PEAK_GBS, 4), traffic=tr, traffic_source=src, algorithmic_gb=round(gb, 3),
                                           k_search_alone_gb_per_s=round(rec["algorithmic_gb_per_batch"] / rec["search_kernel_ms"] * 1e3, 1))
                else:
                    ach = rec["algorithmic_gb_per_batch"] / rec["search_kernel_ms"] * 1e3
                    rec["roofline"] = dict(bound="hbm", kernel="k_search", achieved=round(ach, 1), peak=HBM_PEAK_GBS, unit="GB/s",
                                           frac=round(ach / HBM_PEAK_GBS, 4), traffic=tr, traffic_source=src)
            elif name == "adverse" and isinstance(rec.get("roofline"), dict) and rec["roofline"].get("traffic") is None:
                tr, src = config_traffic(name, None)
                rec["roofline"]["traffic"], rec["roofline"]["traffic_source"] = tr, src
            out[name] = rec
            log(f"config {name}: {rec}")
        except Exception as e:  # noqa: BLE001  (a failed leg must not lose the headline number)
            out[name] = dict(baseline_config=label, error=repr(e)[-800:])
            log(f"config {name} failed: {e!r}")
    return out


def config_traffic(name, setting):
    """HBM bytes per launch of a configs[2..4] leg's dominant kernel from the committed PMC pass of that leg
    (profiles/*_config_<name>_pmc_traffic.json: separate rocprofv3 --pmc FETCH_SIZE run of the same command), when its setting matches."""
    prof = os.path.join(REPO, "profiles")
    best = (None, None)
    for fn in sorted(os.listdir(prof)) if os.path.isdir(prof) else []:
        if not fn.endswith(f"_config_{name}_pmc_traffic.json"):
            continue
        try:
            pj = json.load(open(os.path.join(prof, fn)))
        except Exception:
            continue
        if setting is None or (pj.get("beam") == setting.get("beam") and pj.get("mult") == setting.get("mult")):
            best = (pj.get("hbm_bytes_per_launch"), f"profiles/{fn} (kernel {pj.get('kernel')}; separate rocprofv3 --pmc FETCH_SIZE pass of this leg, not this run; dispatches serialised under --pmc)")
    return best


def host_cpu():
    """(logical cpus, model name) of this box"""
    model = None
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return os.cpu_count() or 1, model


def measured_traffic(beam, mult, n, nq_per_gpu, fraction=-3):
    """HBM bytes per launch of the dominant kernel from the committed PMC pass (rocprofv3 --pmc cannot run inside this
    process); returned only when that pass measured this very configuration, with its source named."""
    best = None
    prof = os.path.join(REPO, "profiles")
    for name in sorted(os.listdir(prof)) if os.path.isdir(prof) else []:
        if not (name.endswith("_pmc_traffic.json")):
            continue
        try:
            pj = json.load(open(os.path.join(prof, name)))
        except Exception:
            continue
        # (a fraction whose windows all take the exact scan moves the same bytes at every setting)
        if (((pj.get("beam") == beam and pj.get("mult") == mult) or pj.get("scan_only")) and pj.get("n") == n and pj.get("nq", 10_000) == nq_per_gpu
                and pj.get("fraction", -3) == fraction):
            best = (pj.get("hbm_bytes_per_launch"), f"profiles/{name} (separate rocprofv3 --pmc FETCH_SIZE pass of this configuration, not this run; --pmc serialises dispatches: the batch's bytes, not the concurrent launches' timing)")
    return best if best else (None, None)


def cpu_baseline(np, workload, n, d, nq, cache, legs, head_names, gpu_leg, per):
    """The REAL reference on this box's host cores, on the graph files this run left in the cache.  The reference fixes its
    thread count at first use, so every thread count is its own process (tools/ref_legs.py): first the GPU's own setting at
    several thread counts, then -- at the best count, in ONE process that loads the index once -- the other candidate
    settings of the headline fraction and every window fraction's leg.  `value` = the reference's best QPS over the headline
    settings with recall@10 > 0.95 (its own best setting, not necessarily the GPU's)."""
    import subprocess
    import tempfile
    ncpu = os.cpu_count() or 1
    tmp = tempfile.mkdtemp(prefix="wann_bench_")

    def run_legs(names, threads, seconds):
        path = os.path.join(tmp, f"legs_{threads}_{len(names)}.npz")
        np.savez(path, **{k: v for k, v in legs.items() if k.split("|", 1)[1] in names})
        cmd = [sys.executable, os.path.join(REPO, "tools", "ref_legs.py"), "--workload", workload, "--threads", str(threads), "--n", str(n),
               "--nq", str(nq), "--dim", str(d), "--cache", cache, "--legs", path, "--seconds", str(seconds)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
        line = [l for l in out.stdout.splitlines() if l.startswith("{")]
        if not line:
            raise RuntimeError((out.stderr or "")[-500:])
        return json.loads(line[-1])

    tried = []
    for threads in sorted({ncpu, max(1, ncpu // 2), max(1, ncpu // 4), max(1, ncpu // 8), max(1, ncpu // 16)}, reverse=True):
        try:
            r = run_legs([gpu_leg], threads, 4.0)
            tried.append(dict(threads=threads, kind=r["_kind"], **r[gpu_leg]))
            log(f"cpu baseline: {tried[-1]}")
        except Exception as e:  # noqa: BLE001
            log(f"cpu baseline with {threads} threads failed: {e!r}")
    if not tried:
        return None
    best_t = max(tried, key=lambda r: r["qps"])
    others = [nm for nm in legs_names(legs) if nm != gpu_leg]
    rest = run_legs(others, best_t["threads"], 2.5) if others else {}
    heads = {gpu_leg: dict(best_t)}
    heads.update({nm: rest[nm] for nm in head_names if nm in rest})
    top = max(heads.items(), key=lambda kv: kv[1]["qps"])
    if per is not None:  # the reference beside every window fraction
        for key, rec in per.items():
            r = rest.get("f:" + key[2:])
            if r:
                rec.update(reference_qps=round(r["qps"], 1), reference_threads=best_t["threads"], rows_identical_dists=r["same_dists"],
                           rows_identical_ids=r["same_ids"], rows_identical_id_sets=r["same_id_sets"])
    host_cores, cpu_model = host_cpu()
    return dict(value=round(top[1]["qps"], 1), unit="queries/s", cores=best_t["threads"], host_cores=host_cores, cpu_model=cpu_model, kind=best_t["kind"],
                sample=f"the same {nq}-query batch, same graph files; best over the settings with recall@10 > 0.95 "
                       f"({', '.join(nm[2:] + ' -> ' + format(v['qps'], '.0f') + ' QPS' for nm, v in heads.items())}; beam,multiplier) at the best of "
                       f"{', '.join(str(r['threads']) + ' -> ' + format(r['qps'], '.0f') for r in tried)} threads (GPU's setting)",
                setting=top[0][2:], gpu_setting=gpu_leg[2:], value_at_gpu_setting=round(best_t["qps"], 1),
                gpu_rows_identical_ids=min(v["same_ids"] for v in heads.values()), gpu_rows_identical_dists=min(v["same_dists"] for v in heads.values()))


def legs_names(legs):
    return sorted({k.split("|", 1)[1] for k in legs if k.startswith("W|")})


if __name__ == "__main__":
    main()

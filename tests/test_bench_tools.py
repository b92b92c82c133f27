"""CPU: the plumbing of bench.py's reference legs (tools/ref_legs.py) on a tiny workload -- the rows a leg carries (here: the
oracle's, standing in for the GPU's) must come back as identical to the real reference's, for a graph-search leg and an
exact-scan leg (without a reference build: the worker's oracle port, and the rows against the digests of the reference's in
tests/golden/oracle_vs_reference.json) -- and the workload table must describe what BASELINE.json names; the stdout line and
--dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np

from util import REPO


def test_workload_table():
    sys.path.insert(0, REPO)
    import bench
    assert set(bench.WORKLOADS) == {"sift", "deep"}
    s, d = bench.WORKLOADS["sift"], bench.WORKLOADS["deep"]
    assert (s["n"], s["d"], s["split"], s["metric"]) == (1_000_000, 128, 2, "l2")          # BASELINE.json configs[1]
    assert (d["n"], d["d"], d["split"], d["metric"]) == (9_990_000, 96, 4, "mips")         # configs[3]
    assert s["cls"].startswith("VamanaRangeFilterTreeIndex") and d["cls"].endswith("Mips")


LEGS = (("h:20,2", -3, 20, 2), ("f:-9", -9, 10, 1))


def legs_rows(mod, cache):
    """the legs' windows and `mod`'s rows on the sift workload at n = 3000, d = 32 (graphs under `cache`, built there when absent)"""
    sys.path.insert(0, REPO)
    import bench
    n, d, nq = 3000, 32, 200
    wl = bench.WORKLOADS["sift"]
    X, Q, labels = wl["make"](n, d, nq, 0)
    idx = getattr(mod, wl["cls"])(X, labels, cutoff=wl["cutoff"], split_factor=wl["split"], build_params=mod.BuildParams(wl["R"], wl["L"], wl["alpha"], cache))
    ls = np.sort(labels)
    rows = {}
    for name, p, beam, mult in LEGS:
        W = bench.make_windows(ls, nq, p, 7)
        rows[name] = (W, beam, mult) + tuple(idx.batch_search(Q, W, nq, wl["method"], mod.QueryParams(10, beam, 1.35, 10_000_000, 10_000, mult, 10000, None, False)))
    return rows


def leg_digests(ids, dists):
    from test_oracle_vs_reference import digest
    return {"ids": digest(ids, np.int64), "id_sets": digest(np.sort(np.asarray(ids).astype(np.int64), axis=1), np.int64), "dists": digest(dists, np.float32)}


def test_reference_legs_worker(oracle, tmp_path):
    from oracle import oracle as orc
    ref = orc.load_reference()
    n, d, nq = 3000, 32, 200
    cache = str(tmp_path / "cache") + "/"
    os.makedirs(cache)
    legs = {}
    golden = json.load(open(os.path.join(REPO, "tests", "golden", "oracle_vs_reference.json")))
    for name, (W, beam, mult, ids, dists) in legs_rows(orc, cache).items():
        legs["W|" + name], legs["set|" + name] = W, np.array([beam, mult])
        legs["ids|" + name], legs["dists|" + name] = ids, dists
        if ref is None:  # the rows the legs carry against the reference's (what the worker checks below when it runs the reference)
            got, want = leg_digests(ids, dists), golden["legs|" + name]
            assert got["dists"] == want["dists"] and got["id_sets"] == want["id_sets"], name
            if name.startswith("h:"):
                assert got["ids"] == want["ids"], name
    path = str(tmp_path / "legs.npz")
    np.savez(path, **legs)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "ref_legs.py"), "--workload", "sift", "--threads", "2", "--n", str(n), "--nq", str(nq),
                        "--dim", str(d), "--cache", cache, "--legs", path, "--seconds", "0.2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["_kind"] == ("reference" if ref is not None else "port") and out["_threads"] == 2
    for name in ("h:20,2", "f:-9"):
        assert out[name]["same_dists"] == 1.0 and out[name]["same_id_sets"] == 1.0 and out[name]["qps"] > 0, out[name]
    assert out["h:20,2"]["same_ids"] == 1.0


def test_stdout_line_fits_and_keeps_the_contract():
    """the stdout line of the longest recorded run (all 17 fractions, six config legs) and of one whose legs all failed stays below
    LINE_BUDGET characters and carries the contract's keys, `config`, `roofline` and `cpu_baseline` unchanged"""
    sys.path.insert(0, REPO)
    import bench
    full = json.load(open(os.path.join(REPO, "profiles", "r06_bench_n1.json")))
    failed = dict(full, configs={name: dict(baseline_config="x" * 200, error="RuntimeError('" + "y" * 900 + "')") for name in full["configs"]})
    for rec in (full, failed):
        s = bench.stdout_line(rec)
        assert len(s) < bench.LINE_BUDGET and "\n" not in s
        line = json.loads(s)
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "config", "roofline", "cpu_baseline"):
            assert line[k] == rec[k], k
        assert set(line["per_fraction"]) == set(rec["per_fraction"]) and set(line["configs"]) == set(rec["configs"])
        assert all(line["per_fraction"][p]["qps"] == r["qps"] for p, r in rec["per_fraction"].items())


def test_dump_outputs(tmp_path):
    """--dump-outputs: float arrays of the step's rows (ids exact as float64); a batch above the budget is cut to the same seeded
    sample of rows every time"""
    sys.path.insert(0, REPO)
    import bench
    rng = np.random.default_rng(5)
    ids = rng.integers(0, 2**31, size=(3000, 10)).astype(np.int32)
    ids[7, 3] = -1  # (an empty slot: uint32 0xFFFFFFFF)
    dists = rng.standard_normal((3000, 10)).astype(np.float32)
    assert bench.dump_outputs(str(tmp_path / "all"), ids, dists) == {"ids": (3000, 10), "dists": (3000, 10)}
    a_ids, a_d = np.load(tmp_path / "all" / "ids.npy"), np.load(tmp_path / "all" / "dists.npy")
    assert a_ids.dtype == np.float64 and a_d.dtype == np.float32 and not (tmp_path / "all" / "rows.npy").exists()
    assert np.array_equal(a_ids, ids.view(np.uint32)) and np.array_equal(a_d, dists) and a_ids[7, 3] == 2.0**32 - 1
    budget = 128 * 1000
    for sub in ("s1", "s2"):
        assert bench.dump_outputs(str(tmp_path / sub), ids, dists, budget=budget)["ids"] == (1000, 10)
        assert sum(os.path.getsize(tmp_path / sub / f) - 128 for f in os.listdir(tmp_path / sub)) <= budget  # (128-byte .npy headers)
    rows = np.load(tmp_path / "s1" / "rows.npy").astype(np.int64)
    assert np.array_equal(rows, np.load(tmp_path / "s2" / "rows.npy")) and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "s1" / "ids.npy"), ids.view(np.uint32)[rows])
    assert np.array_equal(np.load(tmp_path / "s1" / "dists.npy"), dists[rows])


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr


def test_plain_run_refuses_legs_of_full():
    """the legs beyond the headline run with --full only: asking a plain run for one is an error, not a silent no-op"""
    for extra in (["--fractions", "all"], ["--configs", "glove"], ["--pipeline", "2"]):
        r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "1"] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--full" in r.stderr and extra[0] in r.stderr, (extra, r.stderr[-500:])

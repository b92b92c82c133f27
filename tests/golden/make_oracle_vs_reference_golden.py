"""Writes tests/golden/oracle_vs_reference.json: SHA-256 digests of what the REAL reference (oracle/_ref, `make -C oracle ref`)
writes and returns on the inputs of tests/test_oracle_vs_reference.py and of tests/test_bench_tools.py's reference-legs test --
the graph files of every index it builds and the ids / distances of every batch.  Those tests replay the digests wherever no
reference build is present.

    python tests/golden/make_oracle_vs_reference_golden.py"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
os.environ.setdefault("PARLAY_NUM_THREADS", "4")

import test_bench_tools as tb  # noqa: E402
import test_oracle_vs_reference as tv  # noqa: E402
from oracle import oracle as orc  # noqa: E402

orc.build()
ref = orc.load_reference()
assert ref is not None, "no reference build under oracle/_ref (make -C oracle ref)"
out = {}


def rows_digests(rows):
    return {case: tv.row_digests(ids, dists) for case, (ids, dists) in rows.items()}


for metric, gen, d in tv.EQUALS_CASES:
    for kind in tv.KINDS:
        cache = tempfile.mkdtemp() + "/"
        rows = tv.equals_rows(ref, cache, kind, metric, gen, d)
        out[tv.equals_key(kind, metric, gen, d)] = {"graphs": tv.file_digests(cache), "rows": rows_digests(rows)}
for metric, gen, d in tv.RATIO_CASES:
    cache = tempfile.mkdtemp() + "/"
    rows = tv.ratio_rows(ref, cache, metric, gen, d)
    out[tv.ratio_key(metric, gen, d)] = {"graphs": tv.file_digests(cache), "rows": rows_digests(rows)}
for kind, sfx, labs in tv.TIE_CASES:
    cache = tempfile.mkdtemp() + "/"
    X, labels, Q, rows = tv.ties_rows(ref, cache, kind, sfx, labs)
    out[tv.ties_key(kind, sfx, labs)] = {
        "graphs": tv.file_digests(cache),
        "rows": {case: tv.row_digests(*tv.canonical_rows(kind, ids, dists, labels, W, method))
                 for case, (ids, dists, W, method) in rows.items()}}
for case in tv.BUILDER_CASES:
    out[tv.builder_key(*case)] = tv.builder_files(ref, os.path.join(tempfile.mkdtemp(), "g") + "/", *case)
# the reference-legs test: the oracle writes the graphs (standing in for the GPU build), the reference answers on them
cache = tempfile.mkdtemp() + "/"
tb.legs_rows(orc, cache)
for name, (_, _, _, ids, dists) in tb.legs_rows(ref, cache).items():
    out["legs|" + name] = tb.leg_digests(ids, dists)

with open(os.path.join(HERE, "oracle_vs_reference.json"), "w") as f:
    json.dump(out, f, indent=0, sort_keys=True)
print(len(out), "entries")

"""Generate build_alpha_golden.npz from the REAL reference (authoring container only, like make_build_golden.py).

Pins the graph BUILDER where build_golden.npz does not reach: alpha != 1 (the prune's `alpha * d(p*, c) <= d(p, c)`,
vamana/index.h:93-103), the uint8 / int8 point types (int32 distances cast to float: full of exact ties, so these cases rely on
the builders' reference-tie-order mode, ORC_REF_TIES / WANN_REF_TIES, like int_l2) and a hub input (util.star_hub) in which
every insertion batch is one reverse-edge group of a single node.  Every case is a PostfilterVamanaIndex*; stored per case:
X, labels, meta = (R, L, metric, alpha), sfx (the class-name suffix), file_name, file.  star_mips stores no X and no labels
(12 000 x 32 floats would not fit the size limit for a committed file): the test regenerates them with util.star_hub and
ascending labels, and X_sha256 pins the generator's output.

The reference's builds of float rows whose length is no multiple of 8 are not deterministic: PointRange (point_range.h:99-107)
copies d floats into rows it got from aligned_alloc and leaves the padding as it is, and the AVX distance routines
(NSGDist.h:49-66) read (d + 7) & ~7 floats of both rows.  With d = 12 four floats of whatever the allocator returned enter
every distance.  Where that memory is zero -- fresh pages, typically after a few builds of the same sizes -- the graph is the
one of zero-padded rows, which the oracle and the product restate; otherwise it is another, arbitrary one (seen here: 1 to
12 different files in 12 builds, depending on thread count and on what the process built before).  So this script makes the
padding zero by force: every case is built in a process of its own that starts with MALLOC_PERTURB_=255, with which glibc
fills every block it hands out with zero bytes.  On top of that it keeps the plain precautions: WARMUP throw-away builds of
the case, then RUNS builds, of which at least AGREE must have written the stored file -- otherwise it stops with an error that
names the case.  It prints the agreement count per case and never looks at the oracle's or the product's builder.  Only data
is written.  Usage:  python tests/golden/make_build_alpha_golden.py
"""
import collections
import hashlib
import multiprocessing
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from golden_util import STAR  # noqa: E402
from util import REPO, quiet_stdout, star_hub  # noqa: E402

sys.path.insert(0, REPO)
from oracle import oracle as orc  # noqa: E402

WARMUP, RUNS, AGREE = 3, 5, 4


def ref_build(ref, sfx, X, labels, R, L, alpha):
    """(file name, file bytes) of one build by the reference"""
    tmp = tempfile.mkdtemp(prefix="bagold_") + "/"
    with quiet_stdout():
        getattr(ref, "PostfilterVamanaIndex" + sfx)(X, labels, ref.BuildParams(R, L, alpha, tmp))
    (f,) = os.listdir(tmp)
    blob = open(tmp + f, "rb").read()
    shutil.rmtree(tmp)
    return f, blob


def vote(job):
    """in a process of its own: WARMUP throw-away builds of the case, then RUNS builds -> (file name, bytes, how many agree)"""
    sfx, X, labels, R, L, alpha = job
    ref = orc.load_reference()
    for _ in range(WARMUP):
        ref_build(ref, sfx, X, labels, R, L, alpha)
    votes = collections.Counter(ref_build(ref, sfx, X, labels, R, L, alpha) for _ in range(RUNS))
    (f, blob), cnt = votes.most_common(1)[0]
    return f, blob, cnt


def build_case(out, name, sfx, X, labels, R, L, alpha, store_input=True):
    os.environ["MALLOC_PERTURB_"] = "255"  # read by glibc when the child starts: allocated blocks are zero filled
    with multiprocessing.get_context("spawn").Pool(1) as pool:  # (no build of another case has run in that process)
        f, blob, cnt = pool.apply(vote, ((sfx, X, labels, R, L, alpha),))
    print(f"{name}: {cnt} of {RUNS} builds agree, {f}, {len(blob)} bytes")
    if cnt < AGREE:
        raise SystemExit(f"{name}: only {cnt} of {RUNS} builds of the reference agree")
    if store_input:
        out[f"{name}|X"] = X
        out[f"{name}|labels"] = labels
    else:
        out[f"{name}|X_sha256"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(X).tobytes()).digest(), dtype=np.uint8)
    out[f"{name}|meta"] = np.array([R, L, 1 if sfx.endswith("Mips") else 0, alpha], dtype=np.float64)
    out[f"{name}|sfx"] = np.frombuffer(sfx.encode(), dtype=np.uint8)
    out[f"{name}|file_name"] = np.frombuffer(f.encode(), dtype=np.uint8)
    out[f"{name}|file"] = np.frombuffer(blob, dtype=np.uint8)


def perm_labels(rng, n):
    return ((rng.permutation(n) + 0.5) / n).astype(np.float32)


if __name__ == "__main__":
    assert orc.reference_so(), "build the reference first: make -C oracle ref"
    old = np.load(os.path.join(HERE, "build_golden.npz"))
    gX, glab = old["gauss_l2|X"], old["gauss_l2|labels"]
    out = {}
    build_case(out, "gauss_l2_a120", "FloatEuclidian", gX, glab, 12, 30, 1.2)
    build_case(out, "gauss_l2_a1175", "FloatEuclidian", gX, glab, 12, 30, 1.175)
    rng = np.random.default_rng(21)
    U = rng.standard_normal((700, 12)).astype(np.float32)
    U /= np.linalg.norm(U, axis=1, keepdims=True)
    build_case(out, "unit_mips_a120", "FloatMips", U, perm_labels(rng, 700), 12, 30, 1.2)
    rng = np.random.default_rng(22)
    n, d = 900, 24
    U8, I8 = rng.integers(0, 256, (n, d)).astype(np.uint8), rng.integers(-128, 128, (n, d)).astype(np.int8)
    lab8 = perm_labels(rng, n)
    build_case(out, "u8_l2", "UInt8Euclidian", U8, lab8, 12, 30, 1.0)
    build_case(out, "u8_mips", "UInt8Mips", U8, lab8, 12, 30, 1.0)
    build_case(out, "i8_l2", "Int8Euclidian", I8, lab8, 12, 30, 1.0)
    build_case(out, "i8_mips", "Int8Mips", I8, lab8, 12, 30, 1.0)
    build_case(out, "i8_mips_a120", "Int8Mips", I8, lab8, 12, 30, 1.2)
    n = STAR["n"]
    S = star_hub(n, STAR["d"], "mips", [int(orc.random_permutation(n)[0])])  # the hub is the builder's start point
    build_case(out, "star_mips", "FloatMips", S, np.arange(n, dtype=np.float32), STAR["R"], STAR["L"], 1.0, store_input=False)
    path = os.path.join(HERE, "build_alpha_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote build_alpha_golden.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")

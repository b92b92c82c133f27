"""Full-size parity of a float16 index against the REAL reference: configs[2] (GloVe-1.18M-like super tree, n = 1 183 514,
d = 100, inner product) with the points and queries rounded to float16.  The product builds the float16 index on the GPU into a
cache directory of its own (its graphs are those of the ROUNDED points, under the float32 file names: never a cache of the
unrounded points); the real reference's float variant (oracle/_ref) loads THE SAME graph files in a child process
(tools/ref_rows_half.py) on the points and queries upcast to float32 and answers the same 10 000-query batch at window fraction
2^-6 (companion launch, speculated levels).  Every row must be identical: ids and fp32 distance bits.

Without a reference build the test is SKIPPED, loudly."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import fullsize_configs as fc
from util import REPO

pytestmark = pytest.mark.gpu


def test_glove_super_tree_float16_rows_equal_the_reference(wa, gpu, tmp_path):
    from oracle import oracle as orc
    if orc.reference_so(("x86-64-v4", "native", "x86-64-v3")) is None:
        pytest.skip("NO REFERENCE BUILD under oracle/_ref (make -C oracle ref needs the reference checkout): full-size float16 "
                    "parity against the real reference cannot run on this box")
    name = "glove"
    cfg = fc.CONFIGS[name]
    X, Q, labels = fc.make_data(name)
    X16, Q16 = X.astype(np.float16), Q.astype(np.float16)
    del X, Q
    cache = f"/tmp/wann_fullsize_cache/{name}_float16_n{cfg['n']}/"
    os.makedirs(cache, exist_ok=True)
    t0 = time.time()
    idx = wa.SuperOptimizedPostfilterTreeIndexFloat16Mips(X16, labels, build_params=wa.BuildParams(fc.R, fc.L, fc.ALPHA, cache), **cfg["kw"])
    print(f"[fullsize f16] {name}: index ready in {time.time() - t0:.1f}s, {idx.device_bytes() / 2**30:.2f} GiB in HBM")
    p, (beam, mult) = -6, (40, 1)
    W = fc.fraction_windows(labels, cfg["nq"], p, 2000 + p)
    ids, dists = idx.batch_search(Q16, W.astype(np.float32), cfg["nq"], fc.query_params(wa, beam, mult))
    c = idx.counters()
    del idx
    leg = f"2^{p}"
    lp, op = str(tmp_path / "legs.npz"), str(tmp_path / "ref_rows.npz")
    np.savez(lp, **{"W|" + leg: W, "set|" + leg: np.array([beam, mult], dtype=np.int64)})
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "ref_rows_half.py"), "--config", name, "--cache", cache,
                        "--legs", lp, "--out", op], capture_output=True, text=True, timeout=900)
    if r.returncode == 3:
        pytest.skip("NO REFERENCE BUILD under oracle/_ref: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    ref = np.load(op)
    rids, rdists = ref["ids|" + leg], ref["dists|" + leg]
    assert ids.shape == rids.shape == (cfg["nq"], fc.K)
    bad_d = np.flatnonzero(~(dists.view(np.uint32) == rdists.view(np.uint32)).all(axis=1))
    assert bad_d.size == 0, f"{bad_d.size} rows differ in distance bits, first {bad_d[:5]}; counters {c}"
    same = (ids == rids).all(axis=1)
    assert same.all(), f"{int((~same).sum())} rows differ in ids, first {np.flatnonzero(~same)[:5]}"
    print(f"[fullsize f16] {name} {leg}: {cfg['nq']} rows identical to the reference's (beam {beam} x{mult}); searches "
          f"{c['beam_searches']} hops {c['hops']} look-aheads used {c.get('lookaheads_used', 0)} spec searches {c['spec_searches']}")

"""Dev tool: wall time of one index build, for comparing the GPU builder with the host builder on wide rows.
  python tools/build_wide_bench.py N D R L [host]   ->  one JSON line (the GPU builder's summary line included)
A SIFT-like 2-ary tree (cutoff 1000), alpha 1.2, empty graph cache.  Run each build in a process of its own."""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

if __name__ == "__main__":
    n, d, R, L = (int(x) for x in sys.argv[1:5])
    host = len(sys.argv) > 5
    if len(sys.argv) > 6:  # the measured child: stderr goes to the parent, which keeps the summary line
        import rangefilteredann_amd  # noqa: F401
        import window_ann as wa
        from util import distinct_labels, sift_like
        X = sift_like(n, d, 7)(n)
        t = time.time()
        wa.VamanaRangeFilterTreeIndexFloatEuclidian(X, distinct_labels(n, 8), cutoff=1000, split_factor=2,
                                                    build_params=wa.BuildParams(R, L, 1.2, sys.argv[6]))
        print(time.time() - t)
        sys.exit(0)
    cache = tempfile.mkdtemp() + "/"
    env = dict(os.environ, WANN_VERBOSE="1", PARLAY_NUM_THREADS="16")
    env.pop("WANN_HOST_BUILD", None)
    if host:
        env["WANN_HOST_BUILD"] = "1"
    p = subprocess.run([sys.executable, __file__, *sys.argv[1:5], "host" if host else "gpu", cache], env=env, capture_output=True, text=True)
    shutil.rmtree(cache)
    if p.returncode:
        sys.exit(p.stderr[-2000:])
    summary = [ln for ln in p.stderr.splitlines() if "partitions" in ln]
    print(json.dumps({"n": n, "d": d, "R": R, "L": L, "builder": "host, 16 threads" if host else "gpu",
                      "wall_s": round(float(p.stdout.split()[-1]), 2), "summary": summary}))

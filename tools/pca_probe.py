"""Times of the PCA estimator (pct_pca_curvatures) on the seed-1234 torus: sweep, PCA kernels, download, and the float64
rows the certificate sent to the exhaustive pass; the quadric fit of the same cloud and k for comparison.

    python tools/pca_probe.py [N=1000000] [k=50] [repeats=5]

One JSON line per cloud (float32; float64; float64 x 0.2 + 40, whose float32 rounding is coarse).  Medians of `repeats`
calls after one warm-up call."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    ge.build()
    from point_cloud_toolbox_amd import _capi, shapes
    base = shapes.torus_random(n, seed=1234, dtype=np.float64)
    clouds = {"f32": base.astype(np.float32), "f64": base, "f64_coarse": base * 0.2 + 40.0}
    h = _capi.Handle(0)
    try:
        for name, pts in clouds.items():
            h.set_points(pts)
            rec = {"cloud": name, "n": n, "k": k}
            t = []
            for r in range(reps + 1):
                t0 = time.perf_counter()
                exact = h.pca_curvatures(k)
                t1 = time.perf_counter()
                h.get_pca(0, n)
                t2 = time.perf_counter()
                tm = h.timings()
                t.append((tm["grid_ms"] + tm["knn_ms"], tm["fit_ms"], tm["export_ms"], (t1 - t0) * 1e3, (t2 - t1) * 1e3))
            t = np.median(np.array(t[1:]), axis=0)
            rec.update(sweep_ms=round(t[0], 3), pca_kernel_ms=round(t[1], 3), download_ms=round(t[2], 3),
                       call_ms=round(t[3], 3), get_ms=round(t[4], 3), uncertified_rows=int(exact), algo=tm["algo"])
            fit = []
            for r in range(reps + 1):
                h.knn(k)
                h.fit()
                fit.append(h.timings()["fit_ms"])
            rec["quadric_fit_ms_same_k"] = round(float(np.median(fit[1:])), 3)
            print(json.dumps(rec), flush=True)
    finally:
        h.close()


if __name__ == "__main__":
    main()

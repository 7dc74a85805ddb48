"""Times of the per-point tangent-plane Voronoi areas (pct_point_areas) beside the quadric fit of the same resident table.

    python tools/area_probe.py [N=1000000] [k=50] [repeats=11]

The bench's cloud (random torus, seed 1234, float32), the table planted once and left resident.  Three warm-up calls of
each, then `repeats` rounds of one pct_point_areas and one pct_fit, alternating.  Timed: the device time between the
hipEvents around each call's kernels (k_area + k_area_wide; k_fit + k_fit_svd) and the host's wall clock around the
blocking call (launches, one stream wait, the statistics words).  One JSON line: medians with their ranges, the ratio of
the device medians, rows that overflowed the fast kernel's vertex capacity, cuts examined per row behind the rejection
test, closed rows, and the energies of the cloud (device, all rows)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def spread(v):
    v = np.asarray(v, np.float64)
    return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4)}


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 11
    ge.build()
    from point_cloud_toolbox_amd import _capi, shapes
    pts = shapes.torus_random(n, seed=1234)
    h = _capi.Handle(0)
    try:
        h.set_points(pts)
        h.knn(k)
        for _ in range(3):
            h.point_areas()
            h.fit()
        area_dev, area_wall, fit_dev, fit_wall = [], [], [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            h.point_areas()
            t1 = time.perf_counter()
            h.fit()
            t2 = time.perf_counter()
            area_dev.append(h.point_area_stats()["ms"])
            fit_dev.append(h.timings()["fit_ms"])
            area_wall.append((t1 - t0) * 1e3)
            fit_wall.append((t2 - t1) * 1e3)
        st = h.point_area_stats()
        bend, stretch, area, used = h.point_energies()
        rec = {"n": n, "k": k, "repeats": reps,
               "area_device_ms": spread(area_dev), "fit_device_ms": spread(fit_dev),
               "area_call_ms": spread(area_wall), "fit_call_ms": spread(fit_wall),
               "area_over_fit": round(float(np.median(area_dev) / np.median(fit_dev)), 3),
               "overflow_rows": st["overflow"], "closed_rows": st["closed"], "nan_rows": st["nan"],
               "cuts_examined_per_row": round(st["survivors"] / max(st["rows"], 1), 2),
               "bending": bend, "stretching": stretch, "area": area, "rows_used": used}
        print(json.dumps(rec), flush=True)
    finally:
        h.close()


if __name__ == "__main__":
    main()

"""Times of the faces from the tangent-plane Voronoi cells (pct_point_triangles) beside the areas of the same resident table.

    python tools/fan_probe.py [N=1000000] [k=50] [repeats=11]

The bench's cloud (random torus, seed 1234, float32), the table planted once and left resident.  Three warm-up calls of
each, then `repeats` rounds of one pct_point_areas and one pct_point_triangles, alternating, in one process.  The fan kernels
make the cuts of the area kernels and carry the labels, so the areas are the yardstick.  Timed: the device time between
the hipEvents around each call's work (for the triangles also its two parts: the fan kernels, agreement and emission -- the
call's total includes the two host waits that size the wide buffer and the output) and the host's wall clock around the
blocking call.  One JSON line: medians with their ranges, the ratios of the device medians, and the statistics of the
call."""
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
            h.point_triangles()
        area_dev, area_wall, tri_dev, tri_wall, fan_dev, agree_dev = [], [], [], [], [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            h.point_areas()
            t1 = time.perf_counter()
            h.point_triangles()
            t2 = time.perf_counter()
            st = h.point_triangle_stats()
            area_dev.append(h.point_area_stats()["ms"])
            tri_dev.append(st["ms"])
            fan_dev.append(st["fan_ms"])
            agree_dev.append(st["agree_ms"])
            area_wall.append((t1 - t0) * 1e3)
            tri_wall.append((t2 - t1) * 1e3)
        rec = {"n": n, "k": k, "repeats": reps,
               "area_device_ms": spread(area_dev), "triangles_device_ms": spread(tri_dev),
               "fan_kernels_ms": spread(fan_dev), "agreement_emission_ms": spread(agree_dev),
               "area_call_ms": spread(area_wall), "triangles_call_ms": spread(tri_wall),
               "triangles_over_area": round(float(np.median(tri_dev) / np.median(area_dev)), 3),
               "fan_kernels_over_area": round(float(np.median(fan_dev) / np.median(area_dev)), 3),
               **{key: st[key] for key in ("rows", "rows_with_corner", "corners", "triangles", "wide_rows", "largest_fan", "boundary_edges")},
               "area_overflow_rows": h.point_area_stats()["overflow"]}
        print(json.dumps(rec), flush=True)
    finally:
        h.close()


if __name__ == "__main__":
    main()

"""Times of the boundary loops and the hole filling (pct_fill_holes) beside the faces they close (pct_point_triangles).

    python tools/hole_probe.py [N=1000000] [k=50] [repeats=11] [max_vertices=32] [max_perimeter=inf]

The bench's cloud (random torus, seed 1234, float32), the table planted once and left resident.  Three warm-up calls of
each, then `repeats` rounds of one pct_point_triangles and one pct_fill_holes, alternating, in one process (a new
pct_point_triangles drops the hole results, so every pct_fill_holes starts from fresh triangles).  Timed: the device time
between the hipEvents around each call's work -- for pct_fill_holes it includes the three host waits that size the gap, loop
and patch arrays -- and the host's wall clock around the blocking call.  One JSON line: medians with their ranges, the
ratio of the device medians, the statistics of the call and the boundary edges the filled array still has (counted on the
host).  Per-kernel times: run this under a kernel trace of its own."""
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


def boundary_edges(tri, n):
    """Edges with exactly one face."""
    t = np.asarray(tri, np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [0, 2]]])
    key = e.min(1) * n + e.max(1)
    _, counts = np.unique(key, return_counts=True)
    return int((counts == 1).sum()), int(counts.max()) if len(counts) else 0


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 11
    max_vertices = int(sys.argv[4]) if len(sys.argv) > 4 else 32
    max_perimeter = float(sys.argv[5]) if len(sys.argv) > 5 else float("inf")
    ge.build()
    from point_cloud_toolbox_amd import _capi, shapes
    pts = shapes.torus_random(n, seed=1234)
    h = _capi.Handle(0)
    try:
        h.set_points(pts)
        h.knn(k)
        for _ in range(3):
            h.point_triangles()
            h.fill_holes(max_vertices, max_perimeter)
        tri_dev, tri_wall, hole_dev, hole_wall = [], [], [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            h.point_triangles()
            t1 = time.perf_counter()
            h.fill_holes(max_vertices, max_perimeter)
            t2 = time.perf_counter()
            tri_dev.append(h.point_triangle_stats()["ms"])
            hole_dev.append(h.fill_hole_stats()["ms"])
            tri_wall.append((t1 - t0) * 1e3)
            hole_wall.append((t2 - t1) * 1e3)
        st = h.fill_hole_stats()
        after, most = boundary_edges(h.get_filled_triangles(), n)
        rec = {"n": n, "k": k, "repeats": reps, "max_vertices": max_vertices, "max_perimeter": max_perimeter,
               "triangles_device_ms": spread(tri_dev), "fill_holes_device_ms": spread(hole_dev),
               "triangles_call_ms": spread(tri_wall), "fill_holes_call_ms": spread(hole_wall),
               "fill_holes_over_triangles": round(float(np.median(hole_dev) / np.median(tri_dev)), 3),
               "triangles": h.point_triangle_stats()["triangles"],
               **{key: st[key] for key in ("boundary_edges", "gaps", "odd_gaps", "loops", "filled", "perimeter", "blocked", "patch_triangles")},
               "boundary_edges_after": after, "most_faces_on_an_edge": most}
        print(json.dumps(rec), flush=True)
    finally:
        h.close()


if __name__ == "__main__":
    main()

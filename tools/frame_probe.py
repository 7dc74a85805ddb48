"""Times of the per-point surface frames (pct_point_frames) beside the quadric fit of the same resident table.

    python tools/frame_probe.py [N=1000000] [k=50] [repeats=11]

The bench's cloud (random torus, seed 1234, float32), the table planted once and left resident, the fit resident.  Three
warm-up calls of each, then `repeats` rounds of one pct_point_frames and one pct_fit, alternating (the frames of a round
read the coefficients the fit of the round before left: the same values every time).  Timed: the device time between
the hipEvents around each call's kernels (k_frame; k_fit + k_fit_svd) and the host's wall clock around the blocking call
(launches, one stream wait, the statistics words).  One JSON line: medians with their ranges, the ratio of the device
medians, and the counts of the last call (with a viewpoint far above the torus: about half of the rows flipped)."""
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
        view = (0.0, 0.0, 1e3)
        h.fit()
        for _ in range(3):
            h.point_frames(view)
            h.fit()
        frame_dev, frame_wall, fit_dev, fit_wall = [], [], [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            h.point_frames(view)
            t1 = time.perf_counter()
            st = h.point_frame_stats()
            t2 = time.perf_counter()
            h.fit()
            t3 = time.perf_counter()
            frame_dev.append(st["ms"])
            fit_dev.append(h.timings()["fit_ms"])
            frame_wall.append((t1 - t0) * 1e3)
            fit_wall.append((t3 - t2) * 1e3)
        rec = {"n": n, "k": k, "repeats": reps,
               "frame_device_ms": spread(frame_dev), "fit_device_ms": spread(fit_dev),
               "frame_call_ms": spread(frame_wall), "fit_call_ms": spread(fit_wall),
               "frame_over_fit": round(float(np.median(frame_dev) / np.median(fit_dev)), 3),
               "nan_rows": st["nan"], "flipped_rows": st["flipped"], "umbilic_rows": st["umbilic"]}
        print(json.dumps(rec), flush=True)
    finally:
        h.close()


if __name__ == "__main__":
    main()

"""Times of the consistent orientation (pct_orient_frames) on the bench's cloud, and what its kernels need.

    python tools/orient_probe.py [N=1000000] [k=50] [repeats=11]
    python tools/orient_probe.py --resources

The bench's cloud (random torus, seed 1234, float32), the table planted once and left resident, the fit resident.  Every
round computes the frames again (pct_point_frames without a viewpoint: the fit's own sides, the same input every time) and
orients them under the `top` anchor.  Three warm-up rounds, then `repeats` timed ones.  Timed: the device time between the
two hipEvents around the call's work (every launch and every host wait of the flood lies between them) and the host's
wall clock around the blocking call.  One JSON line: medians with their ranges, and the levels, launches and host waits
of the last call.  PCT_ORIENT_LEVELS (push levels per group, default 8) and PCT_ORIENT_GROUPS (groups per host wait,
default 4) are read per call: run it under several settings to see what a host wait costs.

--resources compiles csrc/pct_orient.hip with -Rpass-analysis=kernel-resource-usage (no GPU needed) and prints, per kernel,
the VGPRs, SGPRs, scratch and LDS bytes and the occupancy the compiler reports."""
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def spread(v):
    v = np.asarray(v, np.float64)
    return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4)}


def resources():
    src = os.path.join(ge.CSRC, "pct_orient.hip")
    cmd = [ge.HIPCC] + [f for f in ge.COMPILE_FLAGS if f != "-fPIC"] + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                                                                         "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, check=True).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s*(VGPRs|SGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+))", line)
        if not m:
            continue
        if m.group(1):
            name = m.group(1)
            out[name] = {}
        elif name:
            out[name][m.group(2).split(" [")[0]] = int(m.group(3))
    for name, r in out.items():
        print(json.dumps({"kernel": name, **r}))


def main():
    if "--resources" in sys.argv:
        return resources()
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
        h.fit()
        dev, wall, frame = [], [], []
        for r in range(3 + reps):
            h.point_frames()
            t0 = time.perf_counter()
            h.orient_frames("top")
            t1 = time.perf_counter()
            if r >= 3:
                st = h.orient_stats()
                dev.append(st["ms"])
                wall.append((t1 - t0) * 1e3)
                frame.append(h.point_frame_stats()["ms"])
        rec = {"n": n, "k": k, "repeats": reps,
               "levels_per_group": int(os.environ.get("PCT_ORIENT_LEVELS", 8)), "groups_per_wait": int(os.environ.get("PCT_ORIENT_GROUPS", 4)),
               "orient_device_ms": spread(dev), "orient_call_ms": spread(wall), "frame_device_ms": spread(frame),
               **{key: st[key] for key in ("valid", "components", "unlabelled", "toggled", "levels", "pulls", "launches", "waits")}}
        print(json.dumps(rec), flush=True)
    finally:
        h.close()


if __name__ == "__main__":
    main()

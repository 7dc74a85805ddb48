"""Developer tool: pct_fit_ball on a 1 M-point random torus with 262 144 centres.

    python tools/ball_fit_probe.py [short] [long] [--out FILE]

    short   the radius of the README's radius-search case: rows of ~17 entries
    long    a radius giving ~200 members

Per case, one JSON line each:
    device      pct_fit_ball on the resident rows: hipEvent time of the fit (pct_timings.fit_ms) and host wall time of the
                call, for the default rule, PCT_FIT_BALL_ROUTE=wave and =table, and the default rule at
                PCT_FIT_BALL_SHORT = 32 | 64 | 128 (kBallFitShortMax's candidates)
    compose     what a caller had before: get_ball -> ranking by (d2, index) and padding on the host -> pct_fit_indices, host
                wall time with the transfers (rows longer than 511 members cannot go this way at all)
    knn_fit     pct_fit at the nearest k of the same cloud (the same work per member), hipEvent time, scaled to the centres

Every configuration is warmed up once; then the median of REPS runs (default 11; the host composition 3) with min .. max.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import __graft_entry__ as ge
ge.build()
from point_cloud_toolbox_amd import _capi, shapes

REPS = int(os.environ.get("BALL_FIT_PROBE_REPS", "11"))
N, M = 1 << 20, 1 << 18
TORUS_AREA = 4.0 * np.pi ** 2 * 1.0 * (1.0 / 3.0)          # shapes.torus_random: R = 1, r = 1/3
CASES = {"short": 17, "long": 201}                         # entries per row aimed for (the centre is one of them)


def stats(ts):
    return {"median": round(float(np.median(ts)), 4), "min": round(float(min(ts)), 4), "max": round(float(max(ts)), 4), "runs": len(ts)}


def device(h, centres, env):
    old = {k: os.environ.get(k) for k in ("PCT_FIT_BALL_ROUTE", "PCT_FIT_BALL_SHORT")}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        h.fit_ball(centres)                                 # warm-up of this configuration
        ev, wall = [], []
        for _ in range(REPS):
            t = time.perf_counter()
            h.fit_ball(centres)
            wall.append((time.perf_counter() - t) * 1e3)
            tm = h.timings()
            ev.append(tm["fit_ms"])
        return {"event_ms": stats(ev), "wall_ms": stats(wall), "svd_rows": int(tm["fit_svd_rows"])}
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def compose(h, pts, centres, offsets, reps=3):
    """get_ball -> host ranking and padding -> pct_fit_indices."""
    cand = pts.astype(np.float64)

    def once():
        idx = h.get_ball(0, len(centres))
        row = np.repeat(np.arange(len(centres)), np.diff(offsets))
        keep = idx != centres[row]
        idx, row = idx[keep], row[keep]
        d = cand[idx] - cand[centres[row]]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        order = np.lexsort((idx, d2, row))
        idx, row = idx[order], row[order]
        count = np.bincount(row, minlength=len(centres)).astype(np.int32)
        if count.max() > 511:
            return None
        start = np.zeros(len(centres) + 1, np.int64)
        np.cumsum(count, out=start[1:])
        table = np.zeros((len(centres), int(count.max())), np.int32)
        table[row, np.arange(len(idx)) - start[row]] = idx
        h.fit_indices(table, count, centres)
        return h.get_fit(0, len(centres), coefs=False)

    if once() is None:
        return {"refused": "a row exceeds 511 members"}
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        once()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"wall_ms": stats(ts)}


def knn_fit(h, pts, k):
    h.set_points(pts)
    h.knn(k)
    h.fit()
    ev = []
    for _ in range(REPS):
        h.fit()
        ev.append(h.timings()["fit_ms"])
    s = stats(ev)
    return {"k": k, "event_ms_all_points": s, "event_ms_scaled_to_centres": round(s["median"] * M / N, 4)}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    names = [a for a in args if a in CASES] or list(CASES)
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        if out:
            with open(out, "w") as f:
                f.write("\n".join(lines) + "\n")

    pts = shapes.torus_random(N, seed=11)
    centres = np.sort(np.random.default_rng(12).choice(N, M, replace=False)).astype(np.int64)
    q = pts[centres].astype(np.float64)
    h = _capi.Handle(0)
    for name in names:
        r = float(np.sqrt(CASES[name] * TORUS_AREA / (np.pi * N)))
        h.set_points(pts)
        h.knn(30)                                           # a resident whole-cloud cell list, as in the README's case
        st, offsets = h.query_ball(q, r, 0, _capi.QUERY_GRID)
        assert st == _capi.PCT_OK
        members = np.diff(offsets) - 1
        emit({"case": name, "radius": r, "rows": M, "members_mean": float(members.mean()), "members_min": int(members.min()),
              "members_max": int(members.max()), "share_over_64": float((members > 64).mean())})
        for label, env in (("default", {}), ("wave", {"PCT_FIT_BALL_ROUTE": "wave"}), ("table", {"PCT_FIT_BALL_ROUTE": "table"}),
                           ("short_max=32", {"PCT_FIT_BALL_SHORT": "32"}), ("short_max=64", {"PCT_FIT_BALL_SHORT": "64"}),
                           ("short_max=128", {"PCT_FIT_BALL_SHORT": "128"}), ("short_max=255, table forced", {"PCT_FIT_BALL_SHORT": "255", "PCT_FIT_BALL_ROUTE": "table"})):
            emit({"case": name, "device": label, **device(h, centres, env)})
        emit({"case": name, "compose": compose(h, pts, centres, offsets)})
        emit({"case": name, "knn_fit": knn_fit(h, pts, int(round(members.mean())))})
    h.close()


if __name__ == "__main__":
    main()

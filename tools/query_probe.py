"""Developer tool: caller-supplied queries through the cell list against the exhaustive sweep.

    python tools/query_probe.py crossover      QUERY_SWEEP | QUERY_GRID (resident list) | QUERY_GRID (list built by the call)
                                               on a random torus, n in {4096 .. 1 M} x m in {1024 .. 1 M}, k = 16
    python tools/query_probe.py gain           n = m = 65 536, k = 16: the three paths, and pct_query_points itself
    python tools/query_probe.py big            n = m = 1 M, k = 16 and 50, QUERY_GRID only; the share of queries redone
                                               by the exact sweep on the torus and on tests/wide_exact.py's clump
    python tools/query_probe.py ball           radius search: random torus, n in {65 536, 1 M} x m in {1024 .. 1 M}, r for
                                               rows of ~16, ~50 and ~500 points; QUERY_SWEEP | QUERY_GRID (resident) | QUERY_GRID (built by
                                               the call), sorted rows, the download of the rows included; beside them SciPy's
                                               cKDTree.query_ball_point(..., workers=-1, return_sorted=True) on the same host (tree build
                                               apart).  BALL_PROBE_SECONDS (default 540) bounds the run: what is left then is not measured.

Times are host wall time of the whole call -- upload of the queries, kernels, download of the rows -- around a call that
ends in a stream synchronisation: what a caller of PointCloud.kdtree.query waits for.  Every shape is warmed up once, then
the median of REPS runs is printed (and the spread: min .. max).  Queries: half cloud points jittered by N(0, 0.01), half
uniform in the bounding box scaled 1.5x.  Pairs whose exhaustive sweep would form more than 2^36 pairs are not swept.
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

REPS = int(os.environ.get("QUERY_PROBE_REPS", "7"))
SWEEP_PAIRS_MAX = 1 << 36


def queries(pts, m, seed):
    rng = np.random.default_rng(seed)
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    centre, half = (lo + hi) / 2, (hi - lo) / 2 * 1.5
    a = pts[rng.integers(0, len(pts), m // 2)].astype(np.float64) + rng.normal(0, 0.01, (m // 2, 3))
    return np.vstack([a, rng.uniform(centre - half, centre + half, (m - m // 2, 3))])


def timed(fn, reps=REPS):
    fn()                                                    # warm-up of this shape
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def paths(h, pts, q, k, sweep=True):
    """ms (median, min, max) per path and the stats of the grid calls."""
    out = {}
    h.set_points(pts)
    h.knn(k)                                                # a resident whole-cloud list
    if sweep:
        out["sweep"] = timed(lambda: h.query_points(q, k, 0.0, _capi.QUERY_SWEEP), reps=3 if len(q) * len(pts) > (1 << 32) else REPS)
    out["grid_resident"] = timed(lambda: h.query_points(q, k, 0.0, _capi.QUERY_GRID))
    st = h.query_stats()
    assert st["route"] == 1, st
    out["stats"] = st

    def build():
        h.set_points(pts)                                   # (a fresh cloud: the call builds the list; the upload is timed apart)
        t = time.perf_counter()
        h.query_points(q, k, 0.0, _capi.QUERY_GRID)
        return (time.perf_counter() - t) * 1e3
    build()
    assert h.query_stats()["route"] == 2
    ts = [build() for _ in range(REPS)]
    out["grid_build"] = (float(np.median(ts)), float(min(ts)), float(max(ts)))
    return out


TORUS_AREA = 4.0 * np.pi ** 2 * 1.0 * (1.0 / 3.0)          # shapes.torus_random: R = 1, r = 1/3


def ball_probe(h):
    from scipy.spatial import cKDTree                        # the reference's engine, for the column beside ours
    t_end = time.perf_counter() + float(os.environ.get("BALL_PROBE_SECONDS", "540"))
    flags = _capi.BALL_SORTED

    def ball(q, r, algo):
        st, off = h.query_ball(q, r, flags, algo)
        assert st == _capi.PCT_OK
        return off, h.get_ball(0, len(q))

    for n in (65536, 1 << 20):
        pts = shapes.torus_random(n, seed=1234)
        t = time.perf_counter()
        tree = cKDTree(pts)
        tree_ms = (time.perf_counter() - t) * 1e3
        for want_rows in (16, 50, 500):
            r = float(np.sqrt(want_rows * TORUS_AREA / (np.pi * n)))
            for m in (1024, 16384, 262144, 1 << 20):
                if time.perf_counter() > t_end:
                    print(json.dumps({"n": n, "m": m, "rows_wanted": want_rows, "skipped": "time"}), flush=True)
                    continue
                q = queries(pts, m, 5)
                rec = {"n": n, "m": m, "mn_log2": float(np.log2(n * m)), "r": r, "rows_wanted": want_rows, "scipy_tree_build": tree_ms}
                if m * want_rows > (1 << 28):
                    rec["skipped"] = "entries"
                    print(json.dumps(rec), flush=True)
                    continue
                h.set_points(pts)
                h.knn(30)                                   # a resident whole-cloud list, as a planted cloud has
                off, idx = ball(q, r, _capi.QUERY_GRID)
                st = h.ball_stats()
                assert st["route"] == 1, st
                rec.update(entries=int(off[-1]), mean_row=float(off[-1] / m), longest_row=int(np.diff(off).max()), stats=st)
                sweep = n * m <= (1 << 40)
                if sweep:                                    # the same rows on both paths, at the size that is timed
                    off2, idx2 = ball(q, r, _capi.QUERY_SWEEP)
                    rec["same_rows"] = bool(np.array_equal(off, off2) and np.array_equal(idx, idx2))
                reps = 3 if n * m > (1 << 30) else REPS
                tg, ts = [], []
                for _ in range(reps):                        # the two paths alternate inside one loop
                    t = time.perf_counter(); ball(q, r, _capi.QUERY_GRID); tg.append((time.perf_counter() - t) * 1e3)
                    if sweep:
                        t = time.perf_counter(); ball(q, r, _capi.QUERY_SWEEP); ts.append((time.perf_counter() - t) * 1e3)
                rec["grid_resident"] = (float(np.median(tg)), float(min(tg)), float(max(tg)))
                if sweep:
                    rec["sweep"] = (float(np.median(ts)), float(min(ts)), float(max(ts)))
                tb = []
                for _ in range(3):
                    h.set_points(pts)                       # (a fresh cloud: the call builds the list; the upload is timed apart)
                    t = time.perf_counter(); ball(q, r, _capi.QUERY_GRID); tb.append((time.perf_counter() - t) * 1e3)
                    assert h.ball_stats()["route"] == 2
                rec["grid_build"] = (float(np.median(tb[1:])), float(min(tb[1:])), float(max(tb[1:])))
                if m * want_rows <= (1 << 24):
                    tsp = []
                    for _ in range(3):
                        t = time.perf_counter(); tree.query_ball_point(q, r, workers=-1, return_sorted=True); tsp.append((time.perf_counter() - t) * 1e3)
                    rec["scipy"] = (float(np.median(tsp[1:])), float(min(tsp[1:])), float(max(tsp[1:])))
                print(json.dumps(rec), flush=True)


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "gain"
    h = _capi.Handle(0)
    if what == "ball":
        ball_probe(h)
        h.close()
        return
    if what == "crossover":
        sizes = [4096, 16384, 65536, 262144, 1 << 20]
        ms = [1024, 4096, 16384, 65536, 262144, 1 << 20]
        for n in sizes:
            pts = shapes.torus_random(n, seed=1234)
            for m in ms:
                q = queries(pts, m, 5)
                r = paths(h, pts, q, 16, sweep=n * m <= SWEEP_PAIRS_MAX)
                print(json.dumps({"n": n, "m": m, "mn_log2": float(np.log2(n * m)), **{k: v for k, v in r.items()}}), flush=True)
    elif what == "gain":
        n = m = 65536
        pts = shapes.torus_random(n, seed=1234)
        q = queries(pts, m, 5)
        r = paths(h, pts, q, 16)
        got = h.query_points(q, 16, 0.0, _capi.QUERY_GRID)
        want = h.query_points(q, 16, 0.0, _capi.QUERY_SWEEP)
        r["same_rows"] = bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64)))
        lib = _capi.load()                                  # pct_query_points itself: the kernel QUERY_SWEEP launches
        idx = np.empty((m, 16), np.int32)
        dist = np.empty((m, 16), np.float64)
        r["pct_query_points"] = timed(lambda: h._check(lib.pct_query_points(h._h, _capi._ptr(q, _capi._f64p), m, 16, 0.0, _capi._ptr(idx, _capi._i32p),
                                                                            _capi._ptr(dist, _capi._f64p))))
        r["gain_resident"] = r["sweep"][0] / r["grid_resident"][0]
        r["gain_build"] = r["sweep"][0] / r["grid_build"][0]
        print(json.dumps({"n": n, "m": m, "k": 16, **r}), flush=True)
    elif what == "big":
        n = m = 1 << 20
        pts = shapes.torus_random(n, seed=1234)
        q = queries(pts, m, 5)
        for k in (16, 50):
            r = paths(h, pts, q, k, sweep=False)
            r["redone_share"] = r["stats"]["redone"] / m
            print(json.dumps({"n": n, "m": m, "k": k, **r}), flush=True)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import wide_exact as we
        pts = we.clump()
        q = queries(pts[np.abs(pts).max(1) <= 1.0], 65536, 6)
        for k in (16, 50):
            r = paths(h, pts, q, k, sweep=True)
            r["redone_share"] = r["stats"]["redone"] / len(q)
            print(json.dumps({"cloud": "clump", "n": len(pts), "m": len(q), "k": k, **r}), flush=True)
    else:
        raise SystemExit(__doc__)
    h.close()


if __name__ == "__main__":
    main()

"""Exact radius-search rows  --  TEST INFRASTRUCTURE ONLY (CPU, no GPU, no import of the package).

``rows`` restates what the comment of ``pct_query_ball`` (include/pct_hip.h) promises, with nothing left open:

* candidates are the float32-rounded coordinates of the cloud, widened to float64 (pct:74);
* the query is the caller's float64 point;
* ``d2 = (dx*dx + dy*dy) + dz*dz`` in NumPy float64: three separate operations, nothing fused;
* a point is a member when ``d2 <= r*r``, the product taken in float64: INCLUSIVE (the hybrid k-NN query's ``eps`` is
  strict).  ``r = 0`` keeps coinciding points, ``r = inf`` every point, a NaN ``r`` nothing, a negative ``r`` is ``|r|``
  -- none of them is a case of its own, the comparison decides;
* row i holds the public indices that pass, ascending.

SciPy's tree gives the same rows (tests/test_ball_exact.py asserts it on every case the device tests use).
"""
import numpy as np


def rows(points, queries, r, chunk=256):
    """(offsets (m + 1) int64, indices int32 ascending per row, d2 float64 beside every index).  ``r``: a scalar, or one
    radius per query."""
    cand = np.asarray(points).astype(np.float32).astype(np.float64)
    q = np.asarray(queries, np.float64).reshape(-1, 3)
    rr = np.broadcast_to(np.asarray(r, np.float64), (len(q),))
    with np.errstate(over="ignore"):
        r2 = rr * rr
    counts = np.zeros(len(q), np.int64)
    idx, d2s = [], []
    for s in range(0, len(q), chunk):
        e = min(s + chunk, len(q))
        with np.errstate(over="ignore", invalid="ignore"):
            dx = cand[None, :, 0] - q[s:e, None, 0]
            dy = cand[None, :, 1] - q[s:e, None, 1]
            dz = cand[None, :, 2] - q[s:e, None, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            keep = d2 <= r2[s:e, None]
        counts[s:e] = keep.sum(1)
        row, col = np.nonzero(keep)                   # row-major: ascending index within every row
        idx.append(col.astype(np.int32))
        d2s.append(d2[row, col])
    offsets = np.zeros(len(q) + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    return offsets, (np.concatenate(idx) if idx else np.empty(0, np.int32)), (np.concatenate(d2s) if d2s else np.empty(0, np.float64))


def at_radius(reference, r, m):
    """Entries whose d2 equals r*r exactly."""
    offsets, _, d2 = reference
    rr = np.broadcast_to(np.asarray(r, np.float64), (m,))
    return int((d2 == np.repeat(rr * rr, np.diff(offsets))).sum())


# ======================================================================================================================
# the cases shared by tests/test_ball_exact.py (SciPy against ``rows``) and tests/test_gpu_ball.py (the device against it)
# ======================================================================================================================
LATTICE_OWN_RADII = (1 / 16, 1 / 8, 1 / 4, 5 / 16, 3 / 8, 1 / 2, 2.0)
LATTICE_QUERY_RADII = (1 / 16, 1 / 4, 5 / 16, 1 / 2, 3.0)
PER_QUERY_CHOICES = (0.0, 1 / 16, 1 / 8, 1 / 4, 5 / 16, 3 / 8, 1.0)
SEED_PER_QUERY = 1501
CLUMP_RADII = (0.005, 0.02, 0.5, 100.0)
SORT_CAP = 1024                                       # kBallSortCap (csrc/pct_ball.hip): the longest row its own sort kernel takes
LADDER = tuple(range(0, 131)) + (255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049)
LADDER_ROWS = 40
SEED_LADDER = 1502


def per_query_radii(m):
    return np.random.default_rng(SEED_PER_QUERY).choice(PER_QUERY_CHOICES, m)


def ladder(we, exact_radius):
    """The per-query-radius length ladder on ``wide_exact.torus()``: 40 rows of the cloud, every target length L of
    LADDER on each.  The ranking of a cloud point starts with the point itself (d2 = 0), so a row of length L >= 1 ends
    between ranked entries L - 1 and L.  ``exact_radius=False``: r is the midpoint of those two distances; ``True``:
    r = sqrt(d2) of entry L - 1 exactly -- whatever the rounding of r*r decides, ``rows`` decides the same way.  A query
    at a cloud point has no row of length 0: for L = 0 the query is moved 10 units off the torus and r = 0.5.
    Returns (points, queries (40 len(LADDER), 3), radii)."""
    pts = we.torus()
    sample = np.random.default_rng(SEED_LADDER).choice(len(pts), LADDER_ROWS, replace=False)
    _, d2 = we.ranked(pts, rows=sample, width=2050)
    dist = np.sqrt(d2)
    q, r = [], []
    for i, row in enumerate(sample):
        for L in LADDER:
            p = pts[row].astype(np.float64)
            if L == 0:
                q.append(p + [10.0, 0.0, 0.0])
                r.append(0.5)
            else:
                q.append(p)
                r.append(dist[i, L - 1] if exact_radius else 0.5 * (dist[i, L - 1] + dist[i, L]))
    return pts, np.array(q), np.array(r)


def cases(we):
    """name -> (cloud, queries, radius or radii): the cases SciPy's tree is compared with ``rows`` on, and the device
    with ``rows``; clouds and queries are those of tests/wide_exact.py."""
    out = {}
    lat = we.lattice()
    lq = we.lattice_queries()
    for r in LATTICE_OWN_RADII:
        out[f"lattice own r={r}"] = (lat, lat.astype(np.float64), r)
    for r in LATTICE_QUERY_RADII:
        out[f"lattice queries r={r}"] = (lat, lq, r)
    out["lattice queries per-query r"] = (lat, lq, per_query_radii(len(lq)))
    tw = we.twins()
    for r in (0.0, 0.1):
        out[f"twins own r={r}"] = (tw, tw.astype(np.float64), r)
    cl = we.clump()
    for r in CLUMP_RADII:
        out[f"clump own r={r}"] = (cl, cl.astype(np.float64), r)
    for name in ("flat", "line"):
        p = getattr(we, name)()
        out[f"{name} own r=0.05"] = (p, p.astype(np.float64), 0.05)
    f = we.f64()
    out["f64 native r=0.02"] = (f, f, 0.02)
    to = we.torus()
    for r in (0.05, 0.1):
        out[f"torus own r={r}"] = (to, to.astype(np.float64), r)
    return out

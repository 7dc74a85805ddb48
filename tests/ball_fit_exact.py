"""Curvature over radius neighbourhoods, the reference  --  TEST INFRASTRUCTURE ONLY (CPU, no GPU, no import of the package).

``pct_fit_ball`` (include/pct_hip.h) fits row i of a radius query about the cloud point ``c``: the members are the row's
entries other than ``c`` itself, and the result is the reference's three per-neighbourhood steps on
``points[ranked] - points[c]``, ``ranked`` the members ascending by ``(d2, index)`` with ``pct_query_ball``'s d2.

* ``ranked_rows``: ``ball_exact.rows`` with the centres' own native-dtype coordinates as queries, self dropped, ordered.
* ``reference``: ``pct_oracle.curvature_loop`` on those rows; fewer than two members give NaN (np.cov of one point).
* the cases shared by tests/test_ball_fit_exact.py (the two restatements of the oracle against each other) and
  tests/test_gpu_fit_ball.py (the device against ``reference``).
"""
import numpy as np

import ball_exact as be
import pct_oracle as oracle

LADDER_SAMPLE_ROWS = 16            # of ball_exact.LADDER_ROWS: members 0 ... 129, 254/255/256 ... 2046/2047/2048 on each
CENTRES = 600
SEED_CENTRES = 1601
MIN_MEMBERS = 4                    # rows below it are left out of VALUE comparisons: a covariance of rank <= 2 whose normal
                                   # is decided by LAPACK's rounding

# name -> (K floor scale, H floor scale): the contract's floor is 1e-2 x the curvature scale of the surface
SCALES = {"torus": (9.0, 3.0), "f64": (225.0, 15.0), "flat": (1.0, 1.0), "line": (1.0, 1.0), "twins": (1.0, 1.0), "clump": (1.0, 1.0)}


def ranked_rows(points, centres, r, queries=None):
    """One int32 array per centre: the members of its ball, ascending by (d2, index).  ``queries``: where the rows were
    asked for, if not at the centres themselves (the ladder's empty rows; a non-empty row is always asked at its centre,
    so that the query's d2 is the key's)."""
    points = np.asarray(points)
    centres = np.asarray(centres, np.int64)
    offsets, idx, d2 = be.rows(points, points[centres].astype(np.float64) if queries is None else queries, r)
    out = []
    for i, c in enumerate(centres):
        e, d = idx[offsets[i]:offsets[i + 1]], d2[offsets[i]:offsets[i + 1]]
        keep = e != c
        e, d = e[keep], d[keep]
        out.append(e[np.lexsort((e, d))].astype(np.int32))
    return out


def reference(points, centres, r=None, ranked=None, queries=None):
    """(coefs (m,6), K, H, H2 float32, used int32): the reference-faithful loop on the ranked members of every ball."""
    points = np.asarray(points)
    centres = np.asarray(centres, np.int64)
    ranked = ranked_rows(points, centres, r, queries) if ranked is None else ranked
    m = len(centres)
    used = np.array([len(x) for x in ranked], np.int32)
    coefs = np.full((m, 6), np.nan, np.float32)
    K, H, H2 = (np.full(m, np.nan, np.float32) for _ in range(3))
    fit = np.flatnonzero(used >= 2)
    if len(fit):
        with np.errstate(invalid="ignore", divide="ignore"):
            coefs[fit], K[fit], H[fit], H2[fit] = oracle.curvature_loop(points, [ranked[i] for i in fit], centres[fit])
    return coefs, K, H, H2, used


def padded(ranked):
    """(idx (m, longest) int32 padded with 0, count int32): the rows as pct_fit_indices and curvature_batched take them."""
    count = np.array([len(x) for x in ranked], np.int32)
    idx = np.zeros((len(ranked), max(1, int(count.max()) if len(count) else 1)), np.int32)
    for i, x in enumerate(ranked):
        idx[i, :len(x)] = x
    return idx, count


def ladder_case(we):
    """(points, centres, queries, radii): the length ladder of ball_exact restricted to its first LADDER_SAMPLE_ROWS sample rows.
    A row of target length L holds L - 1 members (the centre is one of its L entries); L = 0 is the empty row of a
    query moved off the torus, whose `centre` is still the sample row."""
    pts, q, r = be.ladder(we, False)
    per = len(be.LADDER)
    sample = np.random.default_rng(be.SEED_LADDER).choice(len(pts), be.LADDER_ROWS, replace=False)
    keep = LADDER_SAMPLE_ROWS * per
    return pts, np.repeat(sample, per)[:keep].astype(np.int64), q[:keep], r[:keep]


def ladder_members():
    return np.tile(np.maximum(np.array(be.LADDER) - 1, 0), LADDER_SAMPLE_ROWS)


def seeded_centres(n, seed_offset=0):
    return np.sort(np.random.default_rng(SEED_CENTRES + seed_offset).choice(n, min(CENTRES, n), replace=False)).astype(np.int64)


def cloud_cases(we):
    """name -> (scale key, points, centres, radius): the other clouds, 600 seeded centres each."""
    out = {}
    f = we.f64()
    for r in (0.02, 0.05):
        out[f"f64 r={r}"] = ("f64", f, seeded_centres(len(f), 1), r)
    for name in ("flat", "line"):
        p = getattr(we, name)()
        out[f"{name} r=0.05"] = (name, p, seeded_centres(len(p), 2), 0.05)
    tw = we.twins()
    out["twins r=0.1"] = ("twins", tw, seeded_centres(len(tw), 3), 0.1)
    cl = we.clump()
    out["clump r=0.02"] = ("clump", cl, seeded_centres(len(cl), 4), 0.02)
    return out


def knn_radii(we, points, k, ranking):
    """Per-centre radii midway between the k-th and (k+1)-th float64 neighbour distance (element 0 of the ranking is
    the point itself), for every point of the cloud: the ball then holds exactly the k-NN row."""
    d = np.sqrt(ranking[1])
    return 0.5 * (d[:, k] + d[:, k + 1])

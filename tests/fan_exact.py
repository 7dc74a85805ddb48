"""Fans, corners and triangles from the tangent-plane Voronoi cells, the reference  --  TEST INFRASTRUCTURE ONLY (CPU, NumPy,
no import of the package).

``pct_point_triangles`` (include/pct_hip_surface.h) cuts, for every row of the resident table, the cell ``pct_point_areas``
cuts -- ``voronoi_exact`` has the block, the frame, the bound and the cuts -- with one label per polygon vertex, and keeps
the triangles that all three of their corners propose.  This module states it again:

  labels    of the edge from vertex v to vertex v + 1: the square's four edges carry -1; a cut by the neighbour of row slot j
            that removes the run s .. e and inserts I1, I2 leaves the labels of the vertices that stay, gives I1 the label j
            and I2 the label vertex e had -- the wrapped and the unwrapped run alike (``clip``: voronoi_exact.clip, the same
            arithmetic, with the labels)
  fan       the cloud records of the labels >= 0, in polygon order
  corner    vertex v with both its arriving edge (label of v - 1, cyclic) and its leaving edge carrying a neighbour, and
            x^2 + y^2 < L^2; the pair (a, b) = (record of the arriving label, of the leaving label); a == b is dropped
  NaN rows  (count < 2, a frame that is not finite): no fan, no corners
  agreed    the triangle {i, a, b} of a corner (a, b) of row i, when row a has a corner whose unordered pair is {b, i} and
            row b one whose pair is {i, a}
  emitted   once, by its corner of lowest index v0, as (v0, a, b) -- counter-clockwise about +z of v0's rotation -- or
            (v0, b, a) where ``flipped[v0]``; the array ascending by (v0, v1, v2)

What a row's combinatorics hang on is reported as in voronoi_exact.cell: ``short`` (the shortest edge in place, or the distance
by which a cut missed or took a vertex) and, new here, ``disc`` -- the smallest |x^2 + y^2 - L^2| over the vertices whose
leaving edge carries a neighbour.  A row is *decided* when both lie beyond the bar voronoi_exact.compare uses for nverts
(C_AREA x the row's unit, relative to L and to L^2) and the row's unit is finite (the gap rule; on open rows also the rules
under which the rotation is no function of the block).  Undecided rows are compared by nobody.
"""
import math

import numpy as np

import voronoi_exact as ve


def clip(X, Y, Lb, a, b, h, j):
    """voronoi_exact.clip with the labels: (X, Y, Lb, miss)."""
    n = len(X)
    d = [(a * X[i] + b * Y[i]) - h for i in range(n)]
    out = [v > 0.0 for v in d]
    miss = min(abs(v) for v in d)
    r = sum(out)
    if r == 0:
        return X, Y, Lb, miss
    if r == n:
        return [], [], [], miss
    s = e = -1
    for i in range(n):
        prev = out[i - 1]
        if out[i] and not prev:
            s = i
        if not out[i] and prev:
            e = (i - 1) % n
    sp, en = (s - 1) % n, (e + 1) % n

    def cross(p, q):
        t = d[p] / (d[p] - d[q])
        return X[p] + t * (X[q] - X[p]), Y[p] + t * (Y[q] - Y[p])

    i1, i2 = cross(sp, s), cross(en, e)
    if s <= e:
        return (X[:s] + [i1[0], i2[0]] + X[e + 1:], Y[:s] + [i1[1], i2[1]] + Y[e + 1:], Lb[:s] + [j, Lb[e]] + Lb[e + 1:], miss)
    return X[e + 1:s] + [i1[0], i2[0]], Y[e + 1:s] + [i1[1], i2[1]], Lb[e + 1:s] + [j, Lb[e]], miss


def cell(ab, L2):
    """The labelled cell of one row from its in-plane coordinates ab (m, 2) float64 and L^2: dict(labels, inside, X, Y,
    short, disc, closed).  short as voronoi_exact.cell; disc relative to L^2."""
    L = math.sqrt(L2)
    X, Y, Lb = [-L, L, L, -L], [-L, -L, L, L], [-1, -1, -1, -1]
    short = math.inf
    for j, (a, b) in enumerate(ab.tolist()):
        rho2 = a * a + b * b
        if not rho2 > 0.0:
            continue
        X, Y, Lb, miss = clip(X, Y, Lb, a, b, 0.5 * rho2, j)
        short = min(short, miss / math.sqrt(rho2))
        if not X:
            break
    n = len(X)
    r2 = [X[i] * X[i] + Y[i] * Y[i] for i in range(n)]
    disc = math.inf
    for i in range(n):
        j = (i + 1) % n
        short = min(short, math.hypot(X[j] - X[i], Y[j] - Y[i]))
        if Lb[i] >= 0:
            disc = min(disc, abs(r2[i] - L2) / L2)
    inside = [v < L2 for v in r2]
    return dict(labels=Lb, inside=inside, X=X, Y=Y, short=short, disc=disc, closed=bool(n >= 3 and max(r2) < L2))


def corners_of(labels, inside, rec):
    """[(a, b)] over the proper corners in polygon order; rec: the cloud record of every row slot."""
    out = []
    n = len(labels)
    for v in range(n):
        la, lb = labels[v - 1], labels[v]
        if la >= 0 and lb >= 0 and inside[v]:
            a, b = int(rec[la]), int(rec[lb])
            if a != b:
                out.append((a, b))
    return out


def rows(points, idx, count=None, frame=ve.frame_oracle, turn=0.0):
    """Every row of ``idx`` (n, k) about its own point: dict(fan: list of lists, corners: list of lists of pairs, nan, closed,
    short, disc, L2, unit -- the row's bar unit (closed or open, inf where no assertion covers the row) --, decided).
    ``turn``: the in-plane basis turned by this angle (the basis-independence check)."""
    points = np.asarray(points)
    idx = np.asarray(idx)
    n, k = idx.shape
    count = np.full(n, k) if count is None else np.asarray(count)
    fan, corners = [[] for _ in range(n)], [[] for _ in range(n)]
    nan, closed = np.ones(n, bool), np.zeros(n, bool)
    short, disc, L2s, unit = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.inf)
    c, s = math.cos(turn), math.sin(turn)
    for i in range(n):
        m = int(count[i])
        if m < 2:
            continue
        block = points[idx[i, :m]] - points[i]
        try:
            with np.errstate(all="ignore"):
                ab = np.asarray(frame(block), np.float64)
        except (ValueError, np.linalg.LinAlgError):
            continue
        q = block.astype(np.float64)
        L2 = float(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]).max())
        if not (np.isfinite(ab).all() and math.isfinite(L2)):
            continue
        if turn:
            ab = np.stack([c * ab[:, 0] + s * ab[:, 1], -s * ab[:, 0] + c * ab[:, 1]], 1)
        g = cell(ab, L2)
        nan[i] = False
        closed[i] = g["closed"]
        fan[i] = [int(idx[i, l]) for l in g["labels"] if l >= 0]
        corners[i] = corners_of(g["labels"], g["inside"], idx[i])
        short[i], disc[i], L2s[i] = g["short"], g["disc"], L2
        with np.errstate(all="ignore"):
            uc, uo = ve.bar_units(ve.facts(block))
        unit[i] = uc if g["closed"] else uo
    rel = ve.C_AREA * np.where(np.isfinite(unit), unit, 0.0)
    with np.errstate(all="ignore"):
        undecided = ~nan & ((disc <= rel) | (short <= rel * np.sqrt(L2s)))
    decided = ~nan & np.isfinite(unit) & ~undecided
    return dict(fan=fan, corners=corners, nan=nan, closed=closed, short=short, disc=disc, L2=L2s, unit=unit,
                undecided=undecided, decided=decided | nan)          # (a NaN row is decided: it has nothing)


def triangles(corners, flipped=None):
    """(T, 3) int32: the agreed triangles, wound and ordered as the header says."""
    n = len(corners)
    pairs = [{frozenset(p) for p in row} for row in corners]
    out = []
    for i in range(n):
        for a, b in corners[i]:
            if i < a and i < b and frozenset((b, i)) in pairs[a] and frozenset((i, a)) in pairs[b]:
                out.append((i, b, a) if flipped is not None and flipped[i] else (i, a, b))
    out.sort()
    return np.asarray(out, np.int32).reshape(-1, 3)


def edge_faces(tri):
    """{(u, v) with u < v: [the directed traversals (p, q) of the faces on the edge]}."""
    edges = {}
    for a, b, c in np.asarray(tri).tolist():
        for p, q in ((a, b), (b, c), (c, a)):
            edges.setdefault((min(p, q), max(p, q)), []).append((p, q))
    return edges


def cyclic(seq):
    """A cyclic sequence from its smallest element on (fans and corners of one row under another in-plane basis start
    at another vertex of the same polygon)."""
    if not seq:
        return []
    at = seq.index(min(seq))
    return seq[at:] + seq[:at]


# the clouds the device test compares exactly (tests/test_gpu_triangles.py); tests/test_fan_exact.py measures their
# undecided share.  name -> (cloud, k, eps)
def n_equals_k_plus_1():
    return ve.random_sphere(13, seed=3)


CASES = {
    "sphere-k20": (lambda: ve.random_sphere(1500, seed=1), 20, None),
    "sphere-k8": (lambda: ve.random_sphere(1500, seed=1), 8, None),
    "torus-k20": (lambda: ve.table_clouds(2000)[0], 20, None),
    "egg-k20": (lambda: ve.table_clouds(1500)[1], 20, None),
    "offset64-k20": (lambda: ve.random_sphere(1500, seed=1, dtype=np.float64) + ve.F64_OFFSET, 20, None),
    "hybrid-k8": (ve.random_sphere, ve.HYBRID_K, ve.HYBRID_EPS),
    "doubled-k16": (ve.doubled_sphere, 16, None),
    "fib400-k200": (lambda: ve.fibonacci_sphere(400), 200, None),
    "n13-k12": (n_equals_k_plus_1, 12, None),
}
# coinciding twins cut along the same line twice: which of them counts as a cut is decided by the last bit there (as
# voronoi_exact.CONCURRENT); the 1 % cap on undecided rows does not apply and little of the case is compared
CONCURRENT = ("doubled-k16",)
UNDECIDED_CAP = 0.01

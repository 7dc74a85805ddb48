"""Exact neighbour rows for the wide sweeps  --  TEST INFRASTRUCTURE ONLY (CPU, no GPU, no import of the package).

Rows of 128 ... 511 neighbours come from the wave-per-query sweeps with a running list of 256 or 512 entries
(csrc/pct_knn_wide.hip, bodies in csrc/pct_knn_sweep.h), and ``pct_query_points`` keeps the same list for caller-supplied
points.  SciPy orders equal distances arbitrarily, so it cannot be the bar where ties decide a row.  ``rows`` restates
what the header of csrc/pct_knn.hip and DESIGN promise, with nothing left open:

* candidates are the float32-rounded coordinates, widened to float64 (pct:74);
* the query is the point in the cloud's native dtype (pct:83), or a caller's float64 point;
* ``d2 = (dx*dx + dy*dy) + dz*dz`` in NumPy float64: three separate operations, nothing fused;
* the order is by ``(d2, public index)`` over ALL n points, the query's own included;
  - cloud rows: element 0 is dropped (pct:84-85 -- not "the point itself": among coinciding points it is the one with the
    smallest index), the next k are kept, distances are ``float32(sqrt(d2))`` (pct:78);
  - ``queries=``: nothing is dropped, distances are the float64 ``sqrt(d2)``;
* with ``eps > 0`` only entries with ``d2 < eps*eps`` are kept (strict, the product taken in float64); the rest read
  index n / ``inf`` and ``count`` is the number kept.

``ranked`` orders every point once per row; the row for k is a prefix of the row for 511, so one ranking serves every k
of a cloud (all 2 744 rows of the lattice: about a second; 40 sampled rows: 0.05 s).

The clouds (each seeded and built here; at most 6 000 points):

    lattice   arange(14)^3 / 16, shuffled, float32: 2 744 points, every coordinate and every d2 exact.  The first
              512 entries of a row hold 23 ... 74 distinct distances in runs of up to 52 equal keys: nine of ten
              adjacent entries tie exactly, across list registers too, and almost every row has an exact tie at
              its cut (tests/test_wide_exact.py asserts the shares the device cases rely on).
    twins     600 copies of one point among 1 800 uniform ones: more than 512 entries with d2 = 0, the rows of the
              copies are decided by index alone.
    exact     the first 256, 257 and 512 points of the lattice: n = k + 1, the first flush is the last.
    clump     2 500 points in a ball of radius 0.02, 300 uniform in [-1, 1]^3, four outliers 70 ... 200 away: a sparse
              query's 511 neighbours lie many rings of cells away, outliers are clamped into boundary cells.
    flat, line   z = 0 (nz = 1) and y = z = 0 (ny = nz = 1): the thin grids of test_gpu_sweep_prologue.make_clouds.
    f64       a float64 torus scaled by 0.2 and moved to 40: the float32 rounding of a coordinate (up to 1.9e-6) is a
              visible share of a neighbour distance.
    torus     the random torus of the package's shapes.torus_random(6000, seed=21), restated (test_gpu_wide_rows.py
              asserts that the two agree bit for bit), float32 and float64: the fit's cloud.
"""
import numpy as np

WIDTH = 513                   # entries of a ranking: element 0, the 511 neighbours of the longest row, the entry behind its cut

LATTICE_SIDE = 14
SEED_LATTICE, SEED_TWINS, SEED_CLUMP, SEED_THIN, SEED_F64, SEED_TORUS = 1401, 1402, 1403, 1404, 1405, 21
EPS_CASES = ((200, 0.25), (256, 0.3125), (511, 0.375))       # (k, eps) on the lattice: eps and eps*eps exact


# ======================================================================================================================
# the reference
# ======================================================================================================================
def _queries(points, rows, queries):
    if queries is not None:
        q = np.asarray(queries, np.float64).reshape(-1, 3)
        return q
    points = np.asarray(points)
    r = np.arange(len(points)) if rows is None else np.asarray(rows, np.int64)
    return points[r].astype(np.float64)               # the native dtype, widened: float32 exactly, float64 as it is


def ranked(points, rows=None, queries=None, width=WIDTH, chunk=256):
    """Every point of the cloud ordered by (d2, public index), per query: (idx (m, w) int32, d2 (m, w) float64), the
    first ``w = min(width, n)`` entries.  ``rows`` (default: every point) or ``queries`` (float64 points) name the m queries."""
    cand = np.asarray(points).astype(np.float32).astype(np.float64)
    q = _queries(points, rows, queries)
    n, w = len(cand), min(width, len(cand))
    idx = np.empty((len(q), w), np.int32)
    d2s = np.empty((len(q), w), np.float64)
    public = np.arange(n)
    for s in range(0, len(q), chunk):
        e = min(s + chunk, len(q))
        dx = cand[None, :, 0] - q[s:e, None, 0]
        dy = cand[None, :, 1] - q[s:e, None, 1]
        dz = cand[None, :, 2] - q[s:e, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        # the w-th smallest d2 of every row: whatever is larger cannot be among the first w of the order, everything
        # else (ties with it included) is ordered in full
        cut = np.partition(d2, w - 1, axis=1)[:, w - 1]
        for r in range(e - s):
            near = public[d2[r] <= cut[r]]
            order = near[np.lexsort((near, d2[r, near]))][:w]      # last key first: d2, then the public index
            idx[s + r] = order
            d2s[s + r] = d2[r, order]
    return idx, d2s


def rows(points, k, eps=0.0, rows=None, queries=None, ranking=None):
    """(idx (m, k) int32, dist (m, k), count (m,) int32) -- see the module docstring.  ``ranking``: what ``ranked`` gave
    for the same points / rows / queries (any k and eps are prefixes of it)."""
    n = len(points)
    cloud_rows = queries is None
    need = k + 1 if cloud_rows else k
    if ranking is None:
        ranking = ranked(points, rows, queries, width=need)
    order, d2 = ranking
    assert order.shape[1] >= min(need, n), "the ranking is shorter than the row"
    m = len(order)
    idx = np.full((m, need), n, np.int32)
    dd = np.full((m, need), np.inf, np.float64)
    w = min(need, order.shape[1])
    idx[:, :w] = order[:, :w]
    dd[:, :w] = d2[:, :w]
    if eps and eps > 0:
        out = ~(dd < float(eps) * float(eps))         # strict; a sorted row: what is cut is a suffix
        idx[out] = n
        dd[out] = np.inf
    if cloud_rows:
        idx, dd = idx[:, 1:], dd[:, 1:]               # element 0 is dropped, whatever it is
    count = (idx < n).sum(1).astype(np.int32)
    dist = np.sqrt(dd)
    return np.ascontiguousarray(idx), np.ascontiguousarray(dist.astype(np.float32) if cloud_rows else dist), count


def tie_at(ranking, i):
    """Rows whose entries i and i + 1 of the full order (element 0 included) have the same d2."""
    d2 = ranking[1]
    return d2[:, i] == d2[:, i + 1]


# ======================================================================================================================
# the clouds
# ======================================================================================================================
def lattice():
    a = np.arange(LATTICE_SIDE, dtype=np.float64) / 16.0
    g = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    return g[np.random.default_rng(SEED_LATTICE).permutation(len(g))].astype(np.float32)


def exact(n):
    """n = k + 1: the first n points of the lattice."""
    return lattice()[:n].copy()


def twins():
    rng = np.random.default_rng(SEED_TWINS)
    one = rng.random(3)
    pts = np.vstack([np.repeat(one[None, :], 600, 0), rng.random((1800, 3))])
    return pts[rng.permutation(len(pts))].astype(np.float32)


def twin_rows(points):
    """Rows of the 600 coinciding points."""
    p, counts = np.unique(points, axis=0, return_counts=True)
    return np.flatnonzero((points == p[counts.argmax()]).all(1))


CLUMP_CENTRE = np.array([0.3, -0.2, 0.1])


def clump():
    rng = np.random.default_rng(SEED_CLUMP)
    v = rng.standard_normal((2500, 3))
    ball = CLUMP_CENTRE + 0.02 * v / np.linalg.norm(v, axis=1, keepdims=True) * np.cbrt(rng.random((2500, 1)))
    wide = rng.uniform(-1.0, 1.0, (300, 3))
    far = np.array([[70.0, 3.0, -2.0], [-110.0, 40.0, 5.0], [8.0, -150.0, 60.0], [-20.0, 30.0, 200.0]])
    pts = np.vstack([ball, wide, far])
    return pts[rng.permutation(len(pts))].astype(np.float32)


def flat():
    rng = np.random.default_rng(SEED_THIN)
    p = np.zeros((3000, 3))
    p[:, :2] = rng.random((3000, 2))
    return p.astype(np.float32)


def line():
    rng = np.random.default_rng(SEED_THIN + 1000)
    p = np.zeros((2000, 3))
    p[:, 0] = rng.random(2000)
    return p.astype(np.float32)


def torus_random(n, seed, dtype=np.float32, R=1.0, r=1.0 / 3.0):
    """The package's shapes.torus_random for n <= 2^20 (one block of its stream), restated."""
    ang = np.random.default_rng([seed, 0]).uniform(0.0, 2.0 * np.pi, size=(n, 2))
    w = R + r * np.cos(ang[:, 1])
    return np.stack([w * np.cos(ang[:, 0]), w * np.sin(ang[:, 0]), r * np.sin(ang[:, 1])], 1).astype(dtype)


def f64():
    return torus_random(3000, SEED_F64, np.float64) * 0.2 + 40.0


def torus(dtype=np.float32):
    return torus_random(6000, SEED_TORUS, dtype)


def lattice_queries():
    """Caller-supplied queries on the lattice: 40 lattice points (d2 = 0 first, six-fold ties behind it), 40 cell centres
    (eight corners at one distance) and 12 points far outside the box (whole faces of the lattice tie)."""
    rng = np.random.default_rng(SEED_LATTICE + 1)
    pts = lattice().astype(np.float64)
    on = pts[rng.choice(len(pts), 40, replace=False)]
    centre = (rng.integers(0, LATTICE_SIDE - 1, (40, 3)) + 0.5) / 16.0
    far = np.array([[5.0, 0.25, 0.25], [-3.0, 0.40625, 0.40625], [0.375, 9.0, 0.375], [0.125, 0.125, -7.0], [4.0, 4.0, 4.0], [-2.0, -2.0, -2.0],
                    [100.0, 0.0, 0.0], [0.40625, 0.40625, 33.0], [-6.0, 6.0, 0.5], [0.5, -12.0, 12.0], [1e3, 1e3, 1e3], [-64.0, 0.8125, 0.0]])
    return np.vstack([on, centre, far])

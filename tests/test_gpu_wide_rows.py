"""Rows of 128 ... 511 neighbours, their fit, and pct_query_points, against an exact reference.

Every algorithm except the exhaustive sweep becomes GRID_EXACT once k > 127 (csrc/pct_auto_route.h); the rows come from
k_knn_exact<4|8> and k_knn_brute<4|8> (csrc/pct_knn_wide.hip: a running list of 256 or 512 entries, a 512-wide bitonic
network with exact (d2, public index) tie-breaks, shell-by-shell widening under ShellIter's pruning bound), and from
k = 256 on the fit reads the resident table without staging it (k_fit<..., STAGED = false>).  pct_query_points keeps the
same list for caller-supplied points.  tests/wide_exact.py is the bar (tests/test_wide_exact.py checks it on the CPU):
indices, float32 distances and counts with np.array_equal, no tolerance, never the library's own exhaustive sweep.

  (a) the list at its widths     lattice, k = 128 ... 511 on both sides of the R = 4 | 8 switch, GRID and BRUTE; TREE and AUTO
  (b) ties decided by index      600 coinciding points, k = 128, 256, 511
  (c) n = k + 1                  256, 257 and 512 points; k = n refused
  (d) eps on wide rows           points exactly at eps, rows cut short and full rows in one call
  (e) widening and pruning       a sparse point whose 511 neighbours lie many rings away; grids one cell thick
  (f) float64 clouds             native query, rounded candidates
  (g) owned ranges               set_query_range, get_neighbor_rows
  (h) the fit of wide rows       fused call at k = 255 (staged), 256 ... 511 (unstaged, resident table), BRUTE + fit
  (i) pct_query_points           k = 1 ... 128 under ties, clouds of 1 ... 65 points, a strict bound, m = 1 and 5

The fit's bars are the ones of test_gpu_fit_conditioning.test_row_lengths_with_garbage_behind_the_count: fit_exact.RTOL
and fit_exact.FLOOR * max|ref| for K and H, rtol = 1e-5 / atol = 2e-6 * scale for the coefficients, against
oracle.curvature_loop of the reference rows.

Measured on an MI355X (one --durations=0 run of this module: 77 tests, 3.8 s together; the host part -- the rankings of
wide_exact, once per cloud, charged to the first test that asks -- is most of it):
  (a) list widths, 18 cases         0.67 s together, 0.14 s the first (the lattice's ranking), 0.03 s the others;
      TREE / LEVELS / EXACT / AUTO  0.03 s each; AUTO on the torus 0.40 s (the torus' ranking)
  (b) coinciding points             0.11 s the first (ranking), 0.01 ... 0.03 s the others
  (c) n = k + 1                     0.02 ... 0.03 s
  (d) eps                           0.01 ... 0.05 s
  (e) clump                         0.12 s (k = 200, with the ranking), 0.04 s (k = 511); observed with set_stats:
                                    k = 200: ring_fallbacks 327 of 2 804 rows, 9 699 248 cells, 486 occupied
                                    k = 511: ring_fallbacks 312, 3 259 872 cells, 472 occupied
      flat / line                   0.13 / 0.07 s (GRID, with the rankings), 0.04 s (BRUTE)
  (f) float64 cloud                 0.12 s the first, 0.02 ... 0.04 s the others
  (g) owned range, scattered rows   0.01 s each
  (h) fused fit, 10 cases           0.02 ... 0.03 s each, 0.39 s the first float64 case (ranking); BRUTE + fit 0.03 s;
                                    K, H and all six coefficients of the 40 sampled rows equal the reference loop's
                                    bit for bit at every width, float32 and float64 (|dK| = |dH| = |dcoef| = 0)
  (i) point queries                 0.02 s on the lattice, below 0.005 s each otherwise
  module set-up (the handle)        0.23 s
No case failed on the kernels as they are.  Four defects planted one at a time in a scratch build (memory-safe ones:
comparisons and in-bounds reads) were each noticed -- the index tie-break left out of bitonic_level's STRIDE >= 64 branch:
46 of the 65 row cases, the lattice, coinciding-point, n = k + 1, eps and owned-range cases among them, none of the tie-free
ones; refresh_tau's register clamped to 6: the 14 cases at k = 448 and 511; ShellIter::fetch's x_hi without the
query's offset in its cell: 23 GRID cases; the unstaged fit walking rows by k instead of the table's pitch: every k = 511
fit here and test_row_lengths_with_garbage_behind_the_count[511].
"""
import numpy as np
import pytest

import fit_exact as fe
import pct_oracle as oracle
import wide_exact as we

pytestmark = pytest.mark.gpu

ALGOS = ("GRID", "BRUTE")
LIST_WIDTHS = (128, 191, 192, 255, 256, 257, 320, 448, 511)      # refresh_tau's slot / source 2*0, 2*63, 3*0, 3*63, 4*0, 4*1, 5*0, 7*0, 7*63
QUERY_KS = (1, 63, 64, 65, 127, 128)
K_MAX = 511                                                      # PCT_K_MAX (csrc/pct_internal.h)

CLOUDS = {"lattice": we.lattice, "twins": we.twins, "clump": we.clump, "flat": we.flat, "line": we.line, "f64": we.f64,
          "torus32": we.torus, "torus64": lambda: we.torus(np.float64),
          "exact256": lambda: we.exact(256), "exact257": lambda: we.exact(257), "exact512": lambda: we.exact(512)}


@pytest.fixture(scope="module")
def bench(gpu):
    """One handle for the module, and every cloud with its ranking: computed once, on first use, never written to."""
    h = gpu["capi"].Handle(0)
    made = {}

    def cloud(name):
        if name not in made:
            pts = CLOUDS[name]()
            ranking = we.ranked(pts)
            for a in (pts,) + ranking:
                a.setflags(write=False)
            made[name] = (pts, ranking)
        return made[name]
    yield {"h": h, "capi": gpu["capi"], "cloud": cloud}
    h.close()


def _algo(capi, name):
    return getattr(capi, "KNN_" + name)


def _assert_rows(got, want, where):
    """(idx, dist, count) of the device against the reference: exact equality, the first differing row in the message."""
    for name, g, w in zip(("indices", "distances", "counts"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (where, name, g.dtype, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.flatnonzero((g != w).reshape(len(g), -1).any(1))
            r = bad[0]
            col = np.flatnonzero(np.atleast_1d(g[r] != w[r]))
            raise AssertionError(f"{where}: {name} differ on {len(bad)} of {len(g)} rows; row {r}, columns {col[:8]} ...: "
                                 f"got {np.atleast_1d(g[r])[col[:8]]}, want {np.atleast_1d(w[r])[col[:8]]}")


def _sweep(bench, cloud, k, algo, eps=0.0, load=True):
    """pct_knn on a whole cloud -> (idx, dist, count), timings."""
    h, capi = bench["h"], bench["capi"]
    pts, _ = bench["cloud"](cloud)
    if load:
        h.set_points(pts)
    h.knn(k, eps, _algo(capi, algo))
    return h.get_neighbors(0, len(pts), want_count=True), h.timings()


def _check_sweep(bench, cloud, k, algo, eps=0.0, takes=None):
    """takes: the algorithm the request resolves to (default: BRUTE stays, everything else becomes GRID_EXACT)."""
    pts, ranking = bench["cloud"](cloud)
    got, t = _sweep(bench, cloud, k, algo, eps)
    capi = bench["capi"]
    assert t["sweep_variant"] == 0, (cloud, k, algo, t["sweep_variant"])              # no fast sweep beyond k = 127
    assert t["algo"] == _algo(capi, takes or ("BRUTE" if algo == "BRUTE" else "GRID_EXACT")), (cloud, k, algo, t["algo"])
    want = we.rows(pts, k, eps=eps, ranking=ranking)
    if not eps:
        assert (got[2] == k).all()
    _assert_rows(got, want, (cloud, k, algo, eps))
    return got, want, t


# ------------------------------------------------------------------------------------------ (a) the list at its widths
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("k", LIST_WIDTHS)
def test_list_widths_on_a_lattice_of_ties(bench, k, algo):
    """Nine of ten adjacent entries of a lattice row are an exact fp64 tie, across list registers (63 | 64, 255 | 256) and
    at the cut of every k here (test_wide_exact.py): a compare-exchange of the 512-wide network that looks at d2 alone, or
    a (k+1)-th distance read from the wrong register or lane, changes indices."""
    _check_sweep(bench, "lattice", k, algo)


@pytest.mark.parametrize("cloud,algo,takes", [("lattice", "TREE", "GRID_EXACT"), ("lattice", "GRID_LEVELS", "GRID_EXACT"),
                                              ("lattice", "GRID_EXACT", "GRID_EXACT"), ("lattice", "AUTO", "BRUTE"),
                                              ("torus32", "AUTO", "GRID_EXACT")])
def test_every_other_algorithm_takes_a_wide_sweep_at_k_256(bench, cloud, algo, takes):
    """resolve_request (csrc/pct_auto_route.h): AUTO is the exhaustive sweep below 4 096 points and the cell list from
    there on; whatever is not the exhaustive sweep becomes GRID_EXACT once k > 127."""
    assert (len(bench["cloud"](cloud)[0]) >= 4096) == (takes == "GRID_EXACT") or algo != "AUTO"
    _check_sweep(bench, cloud, 256, algo, takes=takes)


# ----------------------------------------------------------------------------------- (b) ties decided by index alone
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("k", (128, 256, 511))
def test_coinciding_points_are_ordered_by_index(bench, k, algo):
    """600 points coincide: their rows hold nothing but d2 = 0, element 0 is the copy with the smallest index (NOT the
    query itself), the other 1 800 rows meet a block of 600 equal distances."""
    got, want, _ = _check_sweep(bench, "twins", k, algo)
    pts, _ = bench["cloud"]("twins")
    copies = we.twin_rows(pts)
    assert np.array_equal(got[0][copies[7]], copies[1:k + 1]) and (got[1][copies] == 0).all()


# ---------------------------------------------------------------------------------------------------- (c) n = k + 1
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("n", (256, 257, 512))
def test_rows_that_take_the_whole_cloud(bench, n, algo):
    """n = k + 1: every row holds every other point; the first flush is the last (and, at n = 257, half of the
    512-entry list is padding); the (k+1)-th distance is the last real element.  One more neighbour is refused."""
    h, capi = bench["h"], bench["capi"]
    got, _, _ = _check_sweep(bench, f"exact{n}", n - 1, algo)
    assert np.array_equal(np.sort(got[0], axis=1), np.array([np.delete(np.arange(n), r) for r in range(n)]))
    if n <= K_MAX:
        with pytest.raises(IndexError):                            # PCT_ERR_K_TOO_LARGE (the reference's IndexError, pct:640)
            h.knn(n, 0.0, _algo(capi, algo))
    else:
        with pytest.raises(ValueError, match="outside"):           # k = 512 is past the longest row before it is past the cloud
            h.knn(n, 0.0, _algo(capi, algo))


# ------------------------------------------------------------------------------------------------ (d) eps on wide rows
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("k,eps", we.EPS_CASES)
def test_eps_ball_on_wide_rows(bench, k, eps, algo):
    """eps * eps is exact and thousands of lattice points lie exactly at eps: the bound is strict.  36 %, 71 % and 47 %
    of the rows are full, the others are cut to as few as 50, 89 and 156 entries; what is behind the count reads n / inf."""
    got, want, _ = _check_sweep(bench, "lattice", k, algo, eps)
    n = len(bench["cloud"]("lattice")[0])
    behind = np.arange(k)[None, :] >= got[2][:, None]
    assert (got[0][behind] == n).all() and np.isinf(got[1][behind]).all()
    assert (got[2] == k).any() and (got[2] < k).any()


# --------------------------------------------------------------------------------------------- (e) widening and pruning
@pytest.mark.parametrize("k", (200, 511))
def test_sparse_points_widen_shell_by_shell_and_prune(bench, k):
    """2 500 of 2 804 points sit in a ball of radius 0.02: the 300 sparse points and the four outliers (clamped into
    boundary cells of the grid) find their k neighbours many rings of cells away -- widening by ring + (ring + 1) / 2,
    pruning against a full list.  ring_fallbacks is the precondition that the path ran (observed counters: the module docstring)."""
    h = bench["h"]
    h.set_stats(True)
    try:
        _, _, t = _check_sweep(bench, "clump", k, "GRID")
    finally:
        h.set_stats(False)
    print(f"clump k={k}: ring_fallbacks {t['ring_fallbacks']}, cells {t['cells']}, occupied {t['occupied_cells']}")
    assert t["ring_fallbacks"] > 0
    _check_sweep(bench, "clump", k, "BRUTE")


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("cloud", ("flat", "line"))
def test_thin_grids(bench, cloud, algo):
    """nz = 1, and ny = nz = 1: most stencil rows of a shell lie outside the grid, at every ring."""
    _check_sweep(bench, cloud, 300, algo)


# --------------------------------------------------------------------------------------------------- (f) float64 clouds
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("k", (128, 256, 511))
def test_float64_cloud(bench, k, algo):
    """The query is the native float64 point, the candidates are rounded to float32 (the query's own rounded copy is
    2e-6 away, a visible share of the spacing), the cell comes from the rounded coordinate."""
    pts, ranking = bench["cloud"]("f64")
    assert pts.dtype == np.float64 and (ranking[1][:, 0] > 0).any()
    _check_sweep(bench, "f64", k, algo)


# ----------------------------------------------------------------------------------------------------- (g) owned ranges
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("k", (256, 511))
def test_owned_range_of_the_lattice(bench, k, algo):
    h, capi = bench["h"], bench["capi"]
    pts, ranking = bench["cloud"]("lattice")
    want = we.rows(pts, k, ranking=ranking)
    h.set_points(pts)
    h.set_query_range(700, 1900)
    h.knn(k, 0.0, _algo(capi, algo))
    got = h.get_neighbors(700, 1900, want_count=True)
    _assert_rows(got, tuple(w[700:1900] for w in want), ("range", k, algo))
    with pytest.raises(ValueError):
        h.get_neighbors(699, 1900)
    some = np.array([700, 1899, 1234, 701, 1898], np.int64)
    _assert_rows(h.get_neighbor_rows(some), tuple(w[some] for w in want), ("range rows", k, algo))
    h.set_query_range(0, len(pts))


@pytest.mark.parametrize("algo", ALGOS)
def test_scattered_rows_of_a_wide_table(bench, algo):
    """k_export_rows strides 128 threads over 511 columns (three full trips and one of 127)."""
    pts, ranking = bench["cloud"]("lattice")
    _sweep(bench, "lattice", 511, algo)
    some = np.random.default_rng(5).choice(len(pts), 50, replace=False).astype(np.int64)
    want = we.rows(pts, 511, ranking=ranking)
    _assert_rows(bench["h"].get_neighbor_rows(some), tuple(w[some] for w in want), ("rows", algo))


# ------------------------------------------------------------------------------------------- (h) the fit of wide rows
def _bits(*arrays):
    return [np.ascontiguousarray(a, np.float32).view(np.uint32) for a in arrays]


def _assert_fit(pts, idx, sample, co, K, H, where):
    """Sampled rows against oracle.curvature_loop of the reference rows; the bars of
    test_row_lengths_with_garbage_behind_the_count, nothing new."""
    rc, rK, rH, _ = oracle.curvature_loop(pts, idx[sample], sample)
    assert np.isfinite(rc).all() and np.isfinite(rK).all() and np.isfinite(rH).all(), where
    okK = oracle.curvature_tolerance_ok(K[sample], rK, fe.FLOOR * np.abs(rK).max(), fe.RTOL)
    okH = oracle.curvature_tolerance_ok(H[sample], rH, fe.FLOOR * np.abs(rH).max(), fe.RTOL)
    assert okK.all() and okH.all(), (where, sample[~(okK & okH)], K[sample][~okK], rK[~okK], H[sample][~okH], rH[~okH])
    scale = max(1.0, float(np.abs(rc[:, :3]).max()))
    close = np.isclose(co[sample], rc, rtol=1e-5, atol=2e-6 * scale).all(1)
    assert close.all(), (where, sample[~close], co[sample][~close], rc[~close])
    print(f"{where}: worst |dK| {np.abs(K[sample] - rK).max():.3e} (max|K| {np.abs(rK).max():.3f}), |dH| {np.abs(H[sample] - rH).max():.3e} "
          f"(max|H| {np.abs(rH).max():.3f}), |dcoef| {np.abs(co[sample] - rc).max():.3e}")


@pytest.mark.parametrize("cloud", ("torus32", "torus64"))
@pytest.mark.parametrize("k", (255, 256, 300, 448, 511))
def test_fused_fit_of_wide_rows(bench, gpu, k, cloud):
    """pct_curvature: k = 255 is the last width staged in LDS; from 256 on k_fit walks the RESIDENT table in global
    memory -- sorted-space positions, the table's pitch, float64 query coordinates.  The same rows handed to
    pct_fit_indices (public indices, the caller's pitch) give the same bits."""
    h, capi = bench["h"], bench["capi"]
    pts, ranking = bench["cloud"](cloud)
    if k == 255:
        assert np.array_equal(pts, gpu["shapes"].torus_random(6000, seed=we.SEED_TORUS, dtype=pts.dtype))
    n = len(pts)
    h.set_points(pts)
    h.curvature(k, 0.0, capi.KNN_GRID)
    t = h.timings()
    assert t["sweep_variant"] == 0 and t["algo"] == capi.KNN_GRID_EXACT
    got = h.get_neighbors(0, n, want_count=True)
    want = we.rows(pts, k, ranking=ranking)
    _assert_rows(got, want, (cloud, k, "fused"))
    co, K, H, H2 = h.get_fit(0, n)
    assert np.isfinite(co).all() and np.isfinite(K).all() and np.isfinite(H).all()
    assert np.array_equal(*_bits(H2, H * H))
    sample = np.sort(np.random.default_rng(k).choice(n, 40, replace=False)).astype(np.int64)
    _assert_fit(pts, want[0], sample, co, K, H, (cloud, k, "fused"))
    h.fit_indices(want[0][sample], query=sample)
    again = h.get_fit(0, len(sample))
    for a, b in zip(_bits(*again), _bits(co[sample], K[sample], H[sample], H2[sample])):
        assert np.array_equal(a, b), (cloud, k, "fit_indices against the fused call")


@pytest.mark.parametrize("cloud", ("torus32", "torus64"))
def test_stepwise_fit_of_a_table_in_public_order(bench, cloud):
    """KNN_BRUTE leaves public indices in the table and pct_fit reads them unstaged: k = 511."""
    h, capi = bench["h"], bench["capi"]
    pts, ranking = bench["cloud"](cloud)
    n, k = len(pts), 511
    h.set_points(pts)
    h.knn(k, 0.0, capi.KNN_BRUTE)
    h.fit()
    want = we.rows(pts, k, ranking=ranking)
    _assert_rows(h.get_neighbors(0, n, want_count=True), want, (cloud, k, "brute"))
    co, K, H, _ = h.get_fit(0, n)
    sample = np.sort(np.random.default_rng(k).choice(n, 40, replace=False)).astype(np.int64)
    _assert_fit(pts, want[0], sample, co, K, H, (cloud, k, "brute + fit"))
    h.curvature(k, 0.0, capi.KNN_GRID)                             # ... and the two tables give the same bits
    for a, b in zip(_bits(*h.get_fit(0, n)[:3]), _bits(co, K, H)):
        assert np.array_equal(a, b)


# -------------------------------------------------------------------------------------------------- (i) pct_query_points
def _check_queries(h, pts, q, k, eps=0.0, where=None):
    idx, dist = h.query_points(q, k, eps)
    want = we.rows(pts, k, eps=eps, queries=q)
    assert idx.dtype == np.int32 and dist.dtype == np.float64
    _assert_rows((idx, dist), want[:2], where)
    return want


def test_point_queries_on_the_lattice(bench):
    """Queries AT lattice points (d2 = 0 first, nothing dropped, six-fold ties behind it), at cell centres (eight corners at
    one distance) and far outside the box (whole faces of the lattice tie): indices compared under ties."""
    h = bench["h"]
    pts, _ = bench["cloud"]("lattice")
    q = we.lattice_queries()
    h.set_points(pts)
    for k in QUERY_KS:
        _check_queries(h, pts, q, k, where=("lattice", k))
    for m in (1, 5):                                               # one wave, and one wave into a second block (kWavesPerBlock + 1)
        for k in QUERY_KS:
            _check_queries(h, pts, q[38:38 + m], k, where=("lattice", k, m))
    for k in QUERY_KS:                                             # distance_upper_bound: strict, points exactly at it
        want = _check_queries(h, pts, q, k, eps=0.25, where=("lattice", k, "eps"))
    assert want[2].min() == 0 and (want[2] == 128).any() and ((want[2] > 0) & (want[2] < 128)).any()
    with pytest.raises(ValueError):
        h.query_points(q, 129)
    with pytest.raises(ValueError):
        h.query_points(q, 0)


def test_point_queries_among_coinciding_points(bench):
    h = bench["h"]
    pts, _ = bench["cloud"]("twins")
    copies = we.twin_rows(pts)
    rng = np.random.default_rng(9)
    q = np.vstack([pts[copies[:2]].astype(np.float64), pts[copies[0]].astype(np.float64) + [[1e-3, 0, 0], [0, -0.3, 0.2]], rng.random((20, 3))])
    h.set_points(pts)
    for k in QUERY_KS:
        want = _check_queries(h, pts, q, k, where=("twins", k))
        assert np.array_equal(want[0][0], copies[:k])              # the copies themselves, in index order


@pytest.mark.parametrize("n", (1, 63, 64, 65))
def test_point_queries_on_clouds_smaller_than_a_batch(bench, n):
    """The only batch is mostly padding; k > n pads with n / inf."""
    h = bench["h"]
    pts = we.lattice()[:n]
    q = np.vstack([we.lattice_queries()[36:48], pts[:1].astype(np.float64)])
    h.set_points(pts)
    for k in QUERY_KS:
        want = _check_queries(h, pts, q, k, where=("small", n, k))
        assert (want[2] == min(k, n)).all()
        want = _check_queries(h, pts, q, k, eps=0.5, where=("small", n, k, "eps"))

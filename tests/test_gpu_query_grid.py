"""Caller-supplied query points through the cell list (pct_query_points_algo, PCT_QUERY_GRID; csrc/pct_query.hip) against
the exact (d2, public index) ranking of tests/wide_exact.py: indices and the uint64 view of the float64 distances, bit
for bit, as test_gpu_wide_rows.py section (i) compares the exhaustive path.

QUERY_GRID is forced unless a test says otherwise, and every case says which route it must have taken
(``Handle.query_stats()``): 2 -- a cell list built by the call (a fresh cloud), 1 -- the resident list (after ``knn(20)``:
a cell edge chosen for another k), 0 -- the exhaustive sweep (the fall-backs).  The three stages are told apart by the
same getter: rows answered from the staged 27-cell stencil, rows redone by the exact sweep, the largest ring reached.

The class-surface case draws its 2 048 queries with seed 77: 1 024 cloud points of the torus jittered by N(0, 0.01) and
1 024 uniform in the bounding box scaled 1.5x about its centre, 728 of which lie outside the box (the issue's text names
793 for a generator it does not spell out; this one is written down in _seed77_queries and its count is asserted).
SciPy's tree and the ranking agree on it in every index and distance bit (asserted first: the input is tie-free).
"""
import numpy as np
import pytest

import wide_exact as we

pytestmark = pytest.mark.gpu

KS = (1, 5, 64, 65, 128)                  # one list register up to 64, two above
CROSSOVER = 1 << 34                       # kQueryAutoCrossover (csrc/pct_query_plan.h), the measured constant
SWEEP, RESIDENT, BUILD = 0, 1, 2


@pytest.fixture(scope="module")
def bench(gpu):
    h = gpu["capi"].Handle(0)
    made = {}

    def cloud(name):
        if name not in made:
            made[name] = getattr(we, name)()
            made[name].setflags(write=False)
        return made[name]
    yield {"h": h, "capi": gpu["capi"], "cloud": cloud, "PointCloud": gpu["PointCloud"]}
    h.close()


def _assert_rows(got, want, where):
    for name, g, w in zip(("indices", "distances"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (where, name, g.dtype, g.shape, w.shape)
        gb, wb = (g, w) if name == "indices" else (g.view(np.uint64), w.view(np.uint64))
        if not np.array_equal(gb, wb):
            bad = np.flatnonzero((gb != wb).reshape(len(g), -1).any(1))
            r = bad[0]
            col = np.flatnonzero(np.atleast_1d(gb[r] != wb[r]))
            raise AssertionError(f"{where}: {name} differ on {len(bad)} of {len(g)} rows; row {r}, columns {col[:8]} ...: "
                                 f"got {np.atleast_1d(g[r])[col[:8]]}, want {np.atleast_1d(w[r])[col[:8]]}")


def _check(bench, pts, q, k, eps=0.0, route=None, algo=None, where=None):
    """One query call against the ranking; returns (reference rows, stats)."""
    h, capi = bench["h"], bench["capi"]
    idx, dist = h.query_points(q, k, eps, capi.QUERY_GRID if algo is None else algo)
    st = h.query_stats()
    want = we.rows(pts, k, eps=eps, queries=q)
    assert idx.dtype == np.int32 and dist.dtype == np.float64
    _assert_rows((idx, dist), want[:2], (where, k, eps, st))
    if route is not None:
        assert st["route"] == route, (where, k, st)
    if st["route"] != SWEEP:
        assert st["stencil"] + st["redone"] == len(q) and st["max_ring"] >= 1, (where, st)
    else:
        assert (st["stencil"], st["redone"], st["max_ring"]) == (0, 0, 0), (where, st)
    return want, st


def _both_ways(bench, pts, q, ks=KS, eps=0.0, where=None):
    """Every k on a fresh cloud (the call builds the list) and on the list a knn(20) left."""
    h, capi = bench["h"], bench["capi"]
    stats = []
    for k in ks:
        h.set_points(pts)
        stats.append(_check(bench, pts, q, k, eps, BUILD, where=(where, "build"))[1])
    h.set_points(pts)
    h.knn(20, 0.0, capi.KNN_GRID)                                  # (AUTO would take the exhaustive sweep below 4096 points: no list)
    for k in ks:
        stats.append(_check(bench, pts, q, k, eps, RESIDENT, where=(where, "resident"))[1])
    return stats


# ------------------------------------------------------------------------------------------------------------ the lattice
def test_lattice_queries_under_ties(bench):
    """On lattice points, at cell centres, far outside the box: ties decide every row."""
    pts, q = bench["cloud"]("lattice"), we.lattice_queries()
    _both_ways(bench, pts, q, where="lattice")


def test_lattice_queries_with_a_strict_bound(bench):
    pts, q = bench["cloud"]("lattice"), we.lattice_queries()
    _both_ways(bench, pts, q, eps=0.25, where="lattice eps")
    want = we.rows(pts, 128, eps=0.25, queries=q)
    assert want[2].min() == 0 and (want[2] == 128).any() and ((want[2] > 0) & (want[2] < 128)).any()     # points exactly at eps


@pytest.mark.parametrize("m", (1, 5))
def test_lattice_slices(bench, m):
    """One wave, and one wave into a second block (kWavesPerBlock + 1)."""
    pts, q = bench["cloud"]("lattice"), we.lattice_queries()
    _both_ways(bench, pts, q[38:38 + m], where=("lattice slice", m))


def test_no_queries(bench):
    h, capi = bench["h"], bench["capi"]
    h.set_points(bench["cloud"]("lattice"))
    for algo in (capi.QUERY_GRID, capi.QUERY_AUTO, capi.QUERY_SWEEP):
        idx, dist = h.query_points(np.empty((0, 3)), 5, 0.0, algo)
        assert idx.shape == (0, 5) and dist.shape == (0, 5) and idx.dtype == np.int32 and dist.dtype == np.float64


def test_arguments(bench):
    h, capi = bench["h"], bench["capi"]
    h.set_points(bench["cloud"]("lattice"))
    q = we.lattice_queries()
    for bad in (3, -1):
        with pytest.raises(ValueError):
            h.query_points(q, 5, 0.0, bad)
        with pytest.raises(ValueError):
            h.query_points(np.empty((0, 3)), 5, 0.0, bad)
    for k in (0, 129):
        with pytest.raises(ValueError):
            h.query_points(q, k, 0.0, capi.QUERY_GRID)
    q = q.copy()
    q[7, 1] = np.nan
    with pytest.raises(ValueError):
        h.query_points(q, 5, 0.0, capi.QUERY_GRID)


def test_many_queries_in_one_cell(bench):
    """300 jittered copies of one lattice point and 40 spread queries: chunks of one cell's queries, the item-to-query map."""
    pts = bench["cloud"]("lattice")
    rng = np.random.default_rng(31)
    one = pts[rng.integers(len(pts))].astype(np.float64)
    q = np.vstack([one + rng.normal(0.0, 1e-3, (300, 3)), rng.uniform(-0.2, 1.0, (40, 3))])
    q = q[rng.permutation(len(q))]
    stats = _both_ways(bench, pts, q, ks=(5, 65), where="one cell")
    assert all(s["stencil"] > 0 for s in stats)


# ------------------------------------------------------------------------------------------- the other clouds of wide_exact
def test_queries_among_coinciding_points(bench):
    pts = bench["cloud"]("twins")
    copies = we.twin_rows(pts)
    rng = np.random.default_rng(9)
    q = np.vstack([pts[copies[:2]].astype(np.float64), pts[copies[0]].astype(np.float64) + [[1e-3, 0, 0], [0, -0.3, 0.2]], rng.random((20, 3))])
    h, capi = bench["h"], bench["capi"]
    for k in KS:
        h.set_points(pts)
        want, _ = _check(bench, pts, q, k, route=BUILD, where="twins")
        assert np.array_equal(want[0][0], copies[:k])              # the copies themselves, in index order
    h.set_points(pts)
    h.knn(20, 0.0, capi.KNN_GRID)                                  # (AUTO would take the exhaustive sweep below 4096 points: no list)
    for k in KS:
        _check(bench, pts, q, k, route=RESIDENT, where="twins resident")


def _clump_queries(pts):
    rng = np.random.default_rng(41)
    inside = we.CLUMP_CENTRE + rng.normal(0.0, 0.008, (40, 3))
    shell = rng.uniform(-1.0, 1.0, (40, 3))
    sparse = np.flatnonzero((np.abs(pts.astype(np.float64) - we.CLUMP_CENTRE).max(1) > 0.1) & (np.abs(pts).max(1) <= 1.0))
    on = pts[sparse[:12]].astype(np.float64)                       # AT sparse cloud points: the nearest neighbour is known at once
    far = pts[np.abs(pts).max(1) > 50.0].astype(np.float64)
    assert len(far) == 4 and len(on) == 12
    beside = np.vstack([far + [0.5, -0.25, 0.125], far - [3.0, 0.0, 1.0]])
    axis = np.array([[1e30, 0.0, 0.0], [-1e30, 0.0, 0.0], [0.3, 1e30, 0.1], [0.3, -0.2, -1e30]])
    return np.vstack([inside, shell, on, beside, axis])


def test_clump_runs_every_stage(bench):
    """Inside the clump (stencils that overflow the staging area), in the sparse shell (rows many rings wide), next to
    every outlier (clamped into boundary cells) and at +-1e30 on an axis.  Every call must redo rows and widen rings; the
    27 cells alone must have answered rows at k = 1 (the queries at sparse cloud points) and under the bound.  Stage 2 is
    not asked for rows at k >= 5 without a bound: the list is sized for the clump, whose 27 cells then hold more than
    the 768 staged slots (every clump item overflows), and no sparse query has k neighbours within one cell edge -- a
    stage-2 count of zero is the right answer there, and a failure on every call where the 27 cells can answer."""
    pts = bench["cloud"]("clump")
    q = _clump_queries(pts)
    for stats in (_both_ways(bench, pts, q, where="clump"), _both_ways(bench, pts, q, eps=0.05, where="clump eps")):
        for s in stats:
            assert s["redone"] >= 1 and s["max_ring"] > 1, s
    plain = _both_ways(bench, pts, q, ks=(1,), where="clump k=1")
    bounded = _both_ways(bench, pts, q, ks=(5, 128), eps=0.05, where="clump eps")
    for s in plain + bounded:
        assert s["stencil"] >= 1 and s["redone"] >= 1 and s["max_ring"] > 1, s


@pytest.mark.parametrize("name", ("flat", "line"))
def test_thin_grids(bench, name):
    """nz = 1 and ny = nz = 1; queries in, on and off the plane / the line."""
    pts = bench["cloud"](name)
    rng = np.random.default_rng(51)
    q = np.vstack([pts[rng.choice(len(pts), 30, replace=False)].astype(np.float64), rng.uniform(-0.5, 1.5, (40, 3)),
                   np.c_[rng.random((20, 2)), np.zeros(20)], [[0.5, 0.5, 40.0], [-30.0, 0.0, 0.0], [0.5, 1e30, 0.0]]])
    _both_ways(bench, pts, q, where=name)


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65))
def test_tiny_clouds(bench, n):
    """k > n pads with n / inf; the only batch is mostly padding."""
    pts = we.lattice()[:n]
    q = np.vstack([we.lattice_queries()[36:48], pts[:1].astype(np.float64)])
    h = bench["h"]
    for k in (1, 64, 128):
        h.set_points(pts)
        want, _ = _check(bench, pts, q, k, route=BUILD, where=("tiny", n))
        assert (want[2] == min(k, n)).all()
        _check(bench, pts, q, k, eps=0.5, route=RESIDENT, where=("tiny eps", n))


def test_float64_cloud(bench):
    """Candidates are the float32 roundings, queries float64, at offset 40."""
    pts = bench["cloud"]("f64")
    assert pts.dtype == np.float64
    rng = np.random.default_rng(61)
    lo, hi = pts.min(0), pts.max(0)
    q = np.vstack([pts[rng.choice(len(pts), 60, replace=False)], pts[rng.choice(len(pts), 60, replace=False)] + rng.normal(0, 1e-5, (60, 3)),
                   rng.uniform(lo - 0.1, hi + 0.1, (60, 3))])
    _both_ways(bench, pts, q, where="f64")


# ------------------------------------------------------------------------------------------------------------------ state
def _snapshot(h, n):
    idx, dist, cnt = h.get_neighbors(0, n, want_count=True)
    return [idx, dist, cnt, *h.get_fit(0, n)]


def _same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize("planted", ("GRID", "BRUTE"))
def test_resident_table_and_fit_are_untouched(bench, planted):
    h, capi = bench["h"], bench["capi"]
    pts, q = bench["cloud"]("lattice"), we.lattice_queries()
    h.set_points(pts)
    h.knn(20, 0.0, getattr(capi, "KNN_" + planted))
    h.fit()
    before = _snapshot(h, len(pts))
    timings = h.timings()                                          # (of the call that produced the table: a query is no sweep of the cloud)
    # the list of the cloud's own sweep; under the exhaustive sweep's table (public order) the first call builds one
    routes = (RESIDENT, RESIDENT) if planted == "GRID" else (BUILD, RESIDENT)
    for k, route in zip((5, 128), routes):
        _check(bench, pts, q, k, route=route, where=("state", planted))
    assert h.timings() == timings
    assert _same(before, _snapshot(h, len(pts)))


def test_plain_entry_leaves_the_stats_alone(bench):
    """pct_query_points shares its body with pct_query_points_algo: it still answers from the sweep, builds nothing and
    leaves query_stats those of the last pct_query_points_algo call."""
    h, capi = bench["h"], bench["capi"]
    pts, q = bench["cloud"]("lattice"), np.ascontiguousarray(we.lattice_queries()[38:43])
    h.set_points(pts)
    _check(bench, pts, q, 5, route=BUILD, where="before the plain entry")
    before = h.query_stats()
    lib = capi.load()
    idx = np.empty((len(q), 5), np.int32)
    dist = np.empty((len(q), 5), np.float64)
    h._check(lib.pct_query_points(h._h, capi._ptr(q, capi._f64p), len(q), 5, 0.0, capi._ptr(idx, capi._i32p), capi._ptr(dist, capi._f64p)))
    _assert_rows((idx, dist), we.rows(pts, 5, queries=q)[:2], "plain entry")
    assert h.query_stats() == before


def test_curvature_after_a_grid_query_equals_a_fresh_handle(bench):
    h, capi = bench["h"], bench["capi"]
    pts = bench["cloud"]("torus")
    q = pts[:200].astype(np.float64) + 1e-3
    h.set_points(pts)
    _check(bench, pts, q, 16, route=BUILD, where="before curvature")
    h.curvature(30)
    got = _snapshot(h, len(pts))
    fresh = capi.Handle(0)
    try:
        fresh.set_points(pts)
        fresh.curvature(30)
        assert _same(got, _snapshot(fresh, len(pts)))
    finally:
        fresh.close()


# -------------------------------------------------------------------------------------------------------------- fall-backs
def test_hierarchical_list_falls_back_to_the_sweep(bench):
    h, capi = bench["h"], bench["capi"]
    pts = bench["cloud"]("torus")
    q = np.vstack([pts[:50].astype(np.float64) + 1e-3, [[3.0, 0.0, 0.0]]])
    h.set_points(pts)
    h.knn(20, 0.0, capi.KNN_TREE)
    assert h.timings()["algo"] in (capi.KNN_TREE, capi.KNN_GRID_LEVELS)          # (what a request for the tree may resolve to)
    before = h.get_neighbors(0, len(pts))
    for k in (5, 128):
        _check(bench, pts, q, k, route=SWEEP, where="tree planted")
    assert _same(before[:2], h.get_neighbors(0, len(pts))[:2])


def test_owned_range_falls_back_to_the_sweep(bench):
    h = bench["h"]
    pts, q = bench["cloud"]("lattice"), we.lattice_queries()
    h.set_points(pts)
    h.set_query_range(0, len(pts) // 2)
    _check(bench, pts, q, 5, route=SWEEP, where="owned half, no list")
    h.knn(20)
    for k in (5, 128):
        _check(bench, pts, q, k, route=SWEEP, where="owned half")
    h.set_query_range(0, len(pts))


# -------------------------------------------------------------------------------------------------------------------- AUTO
def test_auto_keeps_small_query_sets_on_the_sweep(bench):
    h, capi = bench["h"], bench["capi"]
    pts, q = bench["cloud"]("lattice"), we.lattice_queries()
    assert len(q) == 92
    h.set_points(pts)
    _check(bench, pts, q, 16, route=SWEEP, algo=capi.QUERY_AUTO, where="auto m=92")
    big = bench["cloud"]("torus")
    h.set_points(big)
    _check(bench, big, big[:1023].astype(np.float64) + 1e-3, 16, route=SWEEP, algo=capi.QUERY_AUTO, where="auto m=1023")


def test_auto_takes_the_grid_past_the_crossover(bench):
    """The measured constant is 2^34 pairs: with m = n the smallest pair past it is 2^17 x 2^17 points of the random torus.
    No host ranking of 2^34 pairs fits a test, so every row is compared, bit for bit, with QUERY_SWEEP on the same handle
    -- pct_query_points' own kernel, pinned to the ranking by test_gpu_wide_rows.py -- and 64 sampled rows with the
    ranking itself.  On a fresh cloud (the call builds the list), on the resident list, and one query short of the constant."""
    h, capi = bench["h"], bench["capi"]
    n = m = 1 << 17
    assert n * m == CROSSOVER
    pts = we.torus_random(n, 88)
    rng = np.random.default_rng(89)
    q = np.vstack([pts[rng.choice(n, m // 2, replace=False)].astype(np.float64) + rng.normal(0, 0.01, (m // 2, 3)), rng.uniform(-2.0, 2.0, (m // 2, 3))])
    h.set_points(pts)
    got = h.query_points(q, 16, 0.0, capi.QUERY_AUTO)
    st = h.query_stats()
    assert st["route"] == BUILD and st["stencil"] > 0 and st["stencil"] + st["redone"] == m, st
    again = h.query_points(q, 16, 0.0, capi.QUERY_AUTO)
    assert h.query_stats()["route"] == RESIDENT
    short = h.query_points(q[:-1], 16, 0.0, capi.QUERY_AUTO)
    assert h.query_stats()["route"] == SWEEP                         # (2^17 - 1) 2^17 pairs: below the constant
    want = h.query_points(q, 16, 0.0, capi.QUERY_SWEEP)
    assert h.query_stats()["route"] == SWEEP
    _assert_rows(got, want, "auto build")
    _assert_rows(again, want, "auto resident")
    _assert_rows(short, (want[0][:-1], want[1][:-1]), "auto short")
    sample = rng.choice(m, 64, replace=False)
    ref = we.rows(pts, 16, queries=q[sample])
    _assert_rows((got[0][sample], got[1][sample]), ref[:2], "auto sample")


# ----------------------------------------------------------------------------------------------------------- class surface
def _seed77_queries(pts):
    rng = np.random.default_rng(77)
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    centre, half = (lo + hi) / 2, (hi - lo) / 2 * 1.5
    near = pts[rng.choice(len(pts), 1024, replace=False)].astype(np.float64) + rng.normal(0, 0.01, (1024, 3))
    box = rng.uniform(centre - half, centre + half, (1024, 3))
    assert int(((box < lo) | (box > hi)).any(1).sum()) == 728
    return np.vstack([near, box])


def test_class_surface_equals_scipy(bench):
    from scipy.spatial import cKDTree
    pts = bench["cloud"]("torus")
    q = _seed77_queries(pts)
    want = we.rows(pts, 16, queries=q)
    d_ref, i_ref = cKDTree(pts.astype(np.float32)).query(q, 16)
    # the two references first: a SciPy that breaks a tie differently shows up here, not as a product failure
    assert np.array_equal(i_ref.astype(np.int32), want[0]) and np.array_equal(d_ref.view(np.uint64), want[1].view(np.uint64))
    pc = bench["PointCloud"](points=pts, normals=np.zeros((len(pts), 0)))
    pc.plant_kdtree(20, algorithm="grid")                             # (the reference builds its tree here, pct:74)
    dist, idx = pc.kdtree.query(q, 16)
    assert idx.dtype == i_ref.dtype and dist.dtype == np.float64 and idx.shape == i_ref.shape
    assert np.array_equal(idx, i_ref) and np.array_equal(dist.view(np.uint64), d_ref.view(np.uint64))
    assert pc._ctx().query_stats()["route"] == SWEEP                  # 2 048 x 6 000 pairs: AUTO stays below the measured crossover
    # the same surface with the list forced: the planted list answers
    idx2, dist2 = pc._ctx().query_points(q, 16, 0.0, bench["capi"].QUERY_GRID)
    assert pc._ctx().query_stats()["route"] == RESIDENT
    assert np.array_equal(idx2, want[0]) and np.array_equal(dist2.view(np.uint64), want[1].view(np.uint64))


# -------------------------------------------------------------------------------------------------------------------- fuzz
def test_fixed_seed_fuzz_against_the_sweep(bench):
    """200 random cases, QUERY_GRID against QUERY_SWEEP (the exhaustive kernel, untouched) on the same handle."""
    h, capi = bench["h"], bench["capi"]
    rng = np.random.default_rng(20240611)
    routes = set()
    for case in range(200):
        n = int(rng.integers(1, 3001))
        kind = int(rng.integers(3))
        if kind == 0:
            pts = rng.uniform(-1.0, 1.0, (n, 3)) * rng.choice([1.0, 1e-3, 50.0])
        elif kind == 1:
            pts = np.vstack([rng.normal(0.0, 0.01, (n - n // 4, 3)), rng.uniform(-1.0, 1.0, (n // 4, 3))])
        else:
            pts = rng.integers(0, 12, (n, 3)) / 16.0
        pts = pts.astype(np.float32)
        m = int(rng.integers(1, 401))
        k = int(rng.integers(1, 129))
        lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
        span = np.maximum(hi - lo, 1e-3)
        q = np.where(rng.random((m, 1)) < 0.5, pts[rng.integers(0, n, m)].astype(np.float64) + rng.normal(0, 0.01, (m, 3)) * span,
                     rng.uniform(lo - 0.5 * span, hi + 0.5 * span, (m, 3)))
        far = rng.random(m) < 0.05
        q[far] += rng.choice([-1.0, 1.0], (int(far.sum()), 3)) * 10.0 ** rng.uniform(1, 12, (int(far.sum()), 1))
        eps = 0.0 if rng.random() < 0.5 else float(rng.uniform(0.02, 1.0) * span.max())
        h.set_points(pts)
        planted = rng.random()
        if planted < 0.6 and n > 21:                               # a resident list | the exhaustive sweep's table (public order: the call builds)
            h.knn(20, 0.0, capi.KNN_GRID if planted < 0.4 else capi.KNN_BRUTE)
        got = h.query_points(q, k, eps, capi.QUERY_GRID)
        st = h.query_stats()
        routes.add(st["route"])
        assert st["route"] in (RESIDENT, BUILD) and st["stencil"] + st["redone"] == m, (case, st)
        want = h.query_points(q, k, eps, capi.QUERY_SWEEP)
        assert h.query_stats()["route"] == SWEEP
        _assert_rows(got, want, ("fuzz", case, n, m, k, eps, kind, st))
    assert routes == {RESIDENT, BUILD}

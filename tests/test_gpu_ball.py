"""Radius search on the device (pct_query_ball; csrc/pct_ball.hip) against the brute-force statement of
tests/ball_exact.py: offsets and indices exactly, distances by their uint64 view.  No tolerance anywhere, no row left out.

Every case runs three ways -- on a fresh cloud (QUERY_GRID: the call builds the cell list, route 2), after
``knn(20, KNN_GRID)`` (the resident list, sized for something else, route 1) and with QUERY_SWEEP (all n points per query,
route 0) -- and asserts the route through ``Handle.ball_stats()``.  Sorted rows are compared as they come; unsorted rows
after a host sort, and a repeat of the call must give the same bytes.  tests/test_ball_exact.py asserts on the CPU that
SciPy's tree gives the reference's rows on every case used here, and that the cases hold what they are here for."""
import numpy as np
import pytest

import ball_exact as be
import wide_exact as we

pytestmark = pytest.mark.gpu

SWEEP, RESIDENT, BUILD = 0, 1, 2
WAYS = ("build", "resident", "sweep")


@pytest.fixture(scope="module")
def bench(gpu):
    capi = gpu["capi"]
    h = capi.Handle(0)
    cases = be.cases(we)
    refs = {}

    def ref(name):
        if name not in refs:
            pts, q, r = cases[name]
            refs[name] = be.rows(pts, q, r)
            for a in refs[name]:
                a.setflags(write=False)
        return cases[name] + (refs[name],)
    yield {"h": h, "capi": capi, "ref": ref, "PointCloud": gpu["PointCloud"]}
    h.close()


def _prepare(bench, pts, way):
    """The handle in the state of ``way``; returns (algo, the route the next ball query must take)."""
    h, capi = bench["h"], bench["capi"]
    h.set_points(pts)
    if way == "resident":
        h.knn(min(20, len(pts) - 1), 0.0, capi.KNN_GRID)
        return capi.QUERY_GRID, RESIDENT
    return (capi.QUERY_GRID, BUILD) if way == "build" else (capi.QUERY_SWEEP, SWEEP)


def _stats(bench, m, route, where):
    st = bench["h"].ball_stats()
    assert st["route"] == route, (where, st)
    if route == SWEEP:
        assert (st["staged"], st["streamed"], st["max_ring"]) == (0, 0, 0), (where, st)
    elif m:
        assert st["staged"] + st["streamed"] == m and st["max_ring"] >= 1, (where, st)
    return st


def _same_rows(got, ref, where):
    offsets, idx, dist = got
    assert offsets.dtype == np.int64 and idx.dtype == np.int32
    assert np.array_equal(offsets, ref[0]), (where, "offsets", int((offsets != ref[0]).sum()))
    if not np.array_equal(idx, ref[1]):
        e = int(np.flatnonzero(idx != ref[1])[0])
        row = int(np.searchsorted(ref[0], e, side="right")) - 1
        raise AssertionError(f"{where}: indices differ from entry {e} (row {row}): got {idx[ref[0][row]:ref[0][row + 1]][:12]}, "
                             f"want {ref[1][ref[0][row]:ref[0][row + 1]][:12]}")
    if dist is not None:
        assert dist.dtype == np.float64
        assert np.array_equal(dist.view(np.uint64), np.sqrt(ref[2]).view(np.uint64)), (where, "distances")


def _host_sorted(offsets, idx, dist, n):
    row = np.repeat(np.arange(len(offsets) - 1, dtype=np.int64), np.diff(offsets))
    order = np.argsort(row * (n + 1) + idx, kind="stable")
    return idx[order], None if dist is None else dist[order]


def _check(bench, pts, q, r, ref, algo, route, where, earlier=0, distances=True, unsorted=True):
    """Sorted rows as they come; unsorted rows after a host sort, twice the same bytes.  Returns the stats of the first
    call.  ``earlier``: ball queries the handle has answered since ``_prepare`` -- only the first one of a fresh cloud
    builds the list, the later ones find it resident."""
    h, capi = bench["h"], bench["capi"]
    dflag = capi.BALL_DISTANCES if distances else 0
    st, offsets = h.query_ball(q, r, capi.BALL_SORTED | dflag, algo)
    assert st == capi.PCT_OK
    stats = _stats(bench, len(q), RESIDENT if route == BUILD and earlier else route, where)
    got = h.get_ball(0, len(q), want_dist=distances)
    _same_rows((offsets,) + (got if distances else (got, None)), ref, (where, "sorted"))
    if unsorted:
        raw = []
        for _ in range(2):
            st, off2 = h.query_ball(q, r, dflag, algo)
            assert st == capi.PCT_OK and np.array_equal(off2, ref[0]), (where, "unsorted offsets")
            got = h.get_ball(0, len(q), want_dist=distances)
            raw.append(got if distances else (got, None))
        assert all(a is b or np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(raw[0], raw[1])), (where, "a repeat call differs")
        _same_rows((off2,) + _host_sorted(off2, raw[0][0], raw[0][1], len(pts)), ref, (where, "unsorted"))
    return stats


def _run_cases(bench, names, way, **kw):
    """Cases that share a cloud, in the state of ``way``: the first call of "build" builds the list (route 2), the list
    then stays resident (route 1)."""
    stats = {}
    pts0 = None
    for i, name in enumerate(names):
        pts, q, r, ref = bench["ref"](name)
        if pts0 is None:
            pts0 = pts
            algo, route = _prepare(bench, pts, way)
        assert pts is pts0
        stats[name] = _check(bench, pts, q, r, ref, algo, route, (name, way), earlier=i, **kw)
    return stats


# ------------------------------------------------------------------------------------------------------------ the lattice
@pytest.mark.parametrize("way", WAYS)
def test_lattice_own_points(bench, way):
    """Up to 47 544 entries exactly at r; at r = 2 every row is the whole cloud."""
    _run_cases(bench, [f"lattice own r={r}" for r in be.LATTICE_OWN_RADII], way)


@pytest.mark.parametrize("way", WAYS)
def test_lattice_queries(bench, way):
    """On lattice points, at cell centres and far outside the box (rows that reach nothing), one radius and one per query."""
    _run_cases(bench, [f"lattice queries r={r}" for r in be.LATTICE_QUERY_RADII] + ["lattice queries per-query r"], way)
    # exactly one point exactly at r, from outside the box
    pts = we.lattice()
    q = np.array([[5.0, 0.25, 0.25]])
    ref = be.rows(pts, q, 4.1875)
    assert ref[0].tolist() == [0, 1]
    algo, route = _prepare(bench, pts, way)
    _check(bench, pts, q, 4.1875, ref, algo, route, ("one at r", way))


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("m", (0, 1, 5))
def test_lattice_slices(bench, way, m):
    """No query, one wave, one wave into a second block."""
    pts = we.lattice()
    q = we.lattice_queries()[38:38 + m]
    r = be.per_query_radii(92)[38:38 + m] if m else 0.25
    ref = be.rows(pts, q, r)
    algo, route = _prepare(bench, pts, way)
    if m == 0:
        st, offsets = bench["h"].query_ball(q, r, bench["capi"].BALL_SORTED, algo)
        assert st == 0 and offsets.tolist() == [0]
        assert len(bench["h"].get_ball(0, 0)) == 0                  # zero rows are resident
        return
    _check(bench, pts, q, r, ref, algo, route, ("slice", m, way))


# ------------------------------------------------------------------------------------------- the other clouds of wide_exact
@pytest.mark.parametrize("way", WAYS)
def test_coinciding_points(bench, way):
    """600 queries in one cell (items of 16 and a remainder); at r = 0 coincidence alone decides."""
    _run_cases(bench, ["twins own r=0.0", "twins own r=0.1"], way)


@pytest.mark.parametrize("way", WAYS)
def test_clump(bench, way):
    """Cubes that overflow the staging area, cubes of many rings, the cube covering the grid, outliers in clamped
    boundary cells.  At r = 100 every cube covers the grid (every query streams); at r = 0.005 the queries of the sparse
    shell have a few points in their cube (staged)."""
    stats = _run_cases(bench, [f"clump own r={r}" for r in be.CLUMP_RADII], way)
    if way != "sweep":
        assert stats["clump own r=100.0"]["streamed"] == 2804 and stats["clump own r=100.0"]["staged"] == 0
        assert stats["clump own r=0.005"]["staged"] > 0
        assert max(s["max_ring"] for s in stats.values()) > 3
        assert any(s["staged"] for s in stats.values()) and any(s["streamed"] for s in stats.values())


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("name", ("flat own r=0.05", "line own r=0.05", "f64 native r=0.02", "torus own r=0.05", "torus own r=0.1"))
def test_thin_grids_float64_and_the_torus(bench, way, name):
    _run_cases(bench, [name], way)


@pytest.mark.parametrize("way", WAYS)
def test_special_radii(bench, way):
    """r = 0, inf, NaN, negative, huge: the comparison decides, nothing is a case of its own."""
    pts = we.lattice()
    q = we.lattice_queries()
    r = np.resize(np.array([0.0, np.inf, np.nan, -0.25, 1e200, -np.inf, 5e-324, 0.25]), len(q))
    ref = be.rows(pts, q, r)
    lengths = np.diff(ref[0])
    assert lengths[1] == len(pts) and lengths[2] == 0 and lengths[4] == len(pts) and lengths[3] > 1
    again = be.rows(pts, q, np.abs(r))
    assert np.array_equal(again[0], ref[0]) and np.array_equal(again[1], ref[1])
    algo, route = _prepare(bench, pts, way)
    _check(bench, pts, q, r, ref, algo, route, ("special radii", way))


# ----------------------------------------------------------------------------------------------- the ladder of row lengths
@pytest.fixture(scope="module")
def ladders():
    out = {}
    for exact in (False, True):
        pts, q, r = be.ladder(we, exact)
        out[exact] = (pts, q, r, be.rows(pts, q, r))
    return out


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("exact_radius", (False, True))
def test_ladder_of_row_lengths(bench, ladders, way, exact_radius):
    """Rows of 0 ... 130, 255 ... 257, 511 ... 513, 1023 ... 1025 (the cap of the sort kernel), 2047 ... 2049 entries in one
    call, with and without distances, sorted and unsorted; and the rows up to the cap alone, where the sort kernel -- not
    the library's segmented sort -- orders every row."""
    pts, q, r, ref = ladders[exact_radius]
    algo, route = _prepare(bench, pts, way)
    _check(bench, pts, q, r, ref, algo, route, ("ladder", exact_radius, way), distances=True)
    _check(bench, pts, q, r, ref, algo, route, ("ladder, no distances", exact_radius, way), earlier=3, distances=False)
    short = np.flatnonzero(np.diff(ref[0]) <= be.SORT_CAP)
    assert np.diff(ref[0])[short].max() == be.SORT_CAP
    ref_short = be.rows(pts, q[short], r[short])
    _check(bench, pts, q[short], r[short], ref_short, algo, route, ("ladder to the cap", exact_radius, way), earlier=6, unsorted=False)


# -------------------------------------------------------------------------------------------------------- result protocol
@pytest.mark.parametrize("way", WAYS)
def test_result_protocol(bench, way):
    h, capi = bench["h"], bench["capi"]
    pts, q, r, ref = bench["ref"]("lattice queries per-query r")
    algo, route = _prepare(bench, pts, way)
    total = int(ref[0][-1])
    st, offsets = h.query_ball(q, r, capi.BALL_COUNT_ONLY, algo)
    assert st == capi.PCT_OK and np.array_equal(offsets, ref[0])
    with pytest.raises(ValueError):
        h.get_ball(0, 1)                                           # COUNT_ONLY leaves nothing resident
    st, offsets = h.query_ball(q, r, capi.BALL_SORTED, algo, max_entries=total - 1)
    assert st == capi.PCT_ERR_LIMIT and np.array_equal(offsets, ref[0])
    with pytest.raises(ValueError):
        h.get_ball(0, 1)
    assert h._lib.pct_get_ball(h._h, 0, 1, None, None) == capi.PCT_ERR_INVALID
    st, offsets = h.query_ball(q, r, capi.BALL_SORTED | capi.BALL_DISTANCES, algo, max_entries=total)
    assert st == capi.PCT_OK
    empty = np.flatnonzero(np.diff(ref[0]) == 0)
    first, last = int(empty[0]), int(empty[-1])
    for b, e in ((0, len(q)), (first, first + 1), (first, last + 1), (first, min(first + 7, len(q))), (3, 3), (len(q) - 1, len(q)), (0, 1)):
        idx, dist = h.get_ball(b, e, want_dist=True)
        assert np.array_equal(idx, ref[1][ref[0][b]:ref[0][e]]), (b, e)
        assert np.array_equal(dist.view(np.uint64), np.sqrt(ref[2][ref[0][b]:ref[0][e]]).view(np.uint64)), (b, e)
    st, _ = h.query_ball(q, r, capi.BALL_SORTED, algo)
    with pytest.raises(ValueError):
        h.get_ball(0, 1, want_dist=True)                           # no distances were asked for
    bad = q.copy()
    bad[7, 1] = np.nan
    assert h._lib.pct_query_ball(h._h, capi._ptr(bad, capi._f64p), len(bad), capi._ptr(np.array([0.25]), capi._f64p), 1, 0, algo, 0,
                                 capi._ptr(np.zeros(len(bad) + 1, np.int64), capi._i64p)) == capi.PCT_ERR_NONFINITE
    for kw in (dict(flags=8), dict(algo=3), dict(algo=-1)):
        with pytest.raises(ValueError):
            h.query_ball(q, 0.25, **kw)
    with pytest.raises(ValueError):
        h.query_ball(q, np.full(len(q) - 1, 0.25), capi.BALL_SORTED, algo)
    h.set_points(pts)
    with pytest.raises(ValueError):
        h.get_ball(0, 1)                                           # a new cloud: the rows are gone


# ------------------------------------------------------------------------------------------------------------------ state
def _snapshot(h, n):
    idx, dist, cnt = h.get_neighbors(0, n, want_count=True)
    return [idx, dist, cnt, *h.get_fit(0, n)]


def _same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize("planted", ("GRID", "BRUTE", "TREE"))
def test_resident_table_and_fit_are_untouched(bench, planted):
    h, capi = bench["h"], bench["capi"]
    pts = we.torus()
    q = np.vstack([pts[:300].astype(np.float64) + 1e-3, [[3.0, 0.0, 0.0]]])
    ref = be.rows(pts, q, 0.1)
    h.set_points(pts)
    h.knn(20, 0.0, getattr(capi, "KNN_" + planted))
    h.fit()
    before = _snapshot(h, len(pts))
    timings = h.timings()
    routes = {"GRID": (RESIDENT, RESIDENT), "BRUTE": (BUILD, RESIDENT), "TREE": (SWEEP, SWEEP)}[planted]
    for route in routes:
        st, offsets = h.query_ball(q, 0.1, capi.BALL_SORTED | capi.BALL_DISTANCES, capi.QUERY_GRID)
        _stats(bench, len(q), route, ("state", planted))
        _same_rows((offsets,) + h.get_ball(0, len(q), want_dist=True), ref, ("state", planted))
    assert h.timings() == timings
    assert _same(before, _snapshot(h, len(pts)))


# ----------------------------------------------------------------------------------------------------------- class surface
def _as_lists(result):
    return [list(x) for x in np.asarray(result, dtype=object).ravel()]


def test_class_surface_equals_scipy(bench):
    from scipy.spatial import cKDTree
    pts = we.torus()
    tree = cKDTree(pts.astype(np.float32))
    rng = np.random.default_rng(177)
    q = np.vstack([pts[rng.choice(len(pts), 150, replace=False)].astype(np.float64) + rng.normal(0, 0.01, (150, 3)), rng.uniform(-1.6, 1.6, (90, 3))])
    grid = q.reshape(6, 40, 3)
    radii = rng.uniform(0.02, 0.3, (6, 40))
    pc = bench["PointCloud"](points=pts, normals=np.zeros((len(pts), 0)))
    pc.plant_kdtree(20, algorithm="grid")
    for budget in (1 << 28, 4096):
        kw = dict(max_entries=budget)
        one = pc.kdtree.query_ball_point(q[3], 0.2, **kw)
        assert type(one) is list and all(type(i) is int for i in one) and one == tree.query_ball_point(q[3], 0.2, return_sorted=True)
        assert len(one) > 10
        n_one = pc.kdtree.query_ball_point(q[3], 0.2, return_length=True, **kw)
        assert isinstance(n_one, int) and n_one == len(one)
        many = pc.kdtree.query_ball_point(q, 0.2, return_sorted=True, **kw)
        assert many.dtype == object and many.shape == (len(q),) and type(many[0]) is list
        assert _as_lists(many) == _as_lists(tree.query_ball_point(q, 0.2, return_sorted=True))
        assert sum(len(x) for x in many) > 4096                   # the small budget chunks the queries
        default = pc.kdtree.query_ball_point(q, 0.2, **kw)        # return_sorted=None: arrays come unsorted
        assert [sorted(x) for x in default] == _as_lists(many)
        cube = pc.kdtree.query_ball_point(grid, radii, return_sorted=True, **kw)
        want = tree.query_ball_point(grid, radii, return_sorted=True)
        assert cube.shape == (6, 40) and _as_lists(cube) == _as_lists(want)
        lengths = pc.kdtree.query_ball_point(grid, radii, return_length=True, **kw)
        assert lengths.dtype == np.int64 and np.array_equal(lengths, tree.query_ball_point(grid, radii, return_length=True))
        offsets, idx, dist = pc.kdtree.query_ball_point_csr(grid, radii, sorted=True, distances=True, **kw)
        ref = be.rows(pts, grid.reshape(-1, 3), radii.reshape(-1))
        _same_rows((offsets, idx, dist), ref, ("csr", budget))
        assert [idx[offsets[i]:offsets[i + 1]].tolist() for i in range(240)] == _as_lists(cube)
        offsets, idx = pc.kdtree.query_ball_point_csr(q, 0.2, sorted=False, **kw)
        assert [sorted(idx[offsets[i]:offsets[i + 1]].tolist()) for i in range(len(q))] == _as_lists(many)
    with pytest.raises(NotImplementedError):
        pc.kdtree.query_ball_point(q, 0.1, p=1)
    with pytest.raises(NotImplementedError):
        pc.kdtree.query_ball_point(q, 0.1, eps=0.5)
    with pytest.raises(ValueError):
        pc.kdtree.query_ball_point(q, 0.1, return_sorted=True, return_length=True)
    with pytest.raises(ValueError, match="'x' must be finite, check for nan or inf values"):
        pc.kdtree.query_ball_point([0.0, np.nan, 0.0], 0.1)
    with pytest.raises(ValueError, match="vectors of length 3"):
        pc.kdtree.query_ball_point(np.zeros((4, 2)), 0.1)
    with pytest.raises(ValueError):
        pc.kdtree.query_ball_point(np.zeros((2, 3)), np.ones(3))

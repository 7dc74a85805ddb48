"""Random call sequences over every modelled entry point on the device (tests/call_driver.py on `_capi.Handle`), and the
regressions of what those sequences and the reading of include/pct_hip.h for them turned up.

Every case is one committed (seed, profile, steps) of call_driver.CASES: tests/test_call_model.py shows without a GPU
that those seeds reach every entry point and catch every seeded violation of the header's state rules.  No timing is
asserted."""
import numpy as np
import pytest

import call_driver as D

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed,profile,steps", D.CASES, ids=[f"{p}-{s}" for s, p, _ in D.CASES])
def test_call_sequence_matches_fresh_handles(gpu, seed, profile, steps):
    capi = gpu["capi"]
    assert D.run(lambda: capi.Handle(0), seed, profile, steps) == steps


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=x.dtype.kind == "f") for x, y in zip(a, b))


def test_refused_orient_frames_keeps_the_orientation(gpu):
    """pct_orient_frames cleared the orientation before it had checked anything: a call refused for its anchor, its
    viewpoint or the state of the handle dropped what an earlier call had left, while the frames stayed turned.  The
    header: a refused call changes nothing."""
    capi = gpu["capi"]
    pts = gpu["shapes"].torus_random(2500, seed=3)
    h = capi.Handle(0)
    try:
        h.set_points(pts); h.curvature(12); h.point_frames(); h.orient_frames("top")
        labels, frames, stats = h.get_orientation(0, len(pts)), h.get_point_frames(0, len(pts)), h.orient_stats()
        assert stats["toggled"] > 0 and stats["components"] >= 1
        for anchor, view in ((7, None), ("view", None), ("view", (np.nan, 0.0, 0.0))):
            with pytest.raises(ValueError):
                h.orient_frames(anchor, view)
            assert _same(h.get_orientation(0, len(pts)), labels) and _same(h.get_point_frames(0, len(pts)), frames)
            assert h.orient_stats() == stats
        h.voxel_downsample(pts, 0.05)                       # the table is gone: the flood has nothing to read
        with pytest.raises(ValueError):
            h.orient_frames("top")
        assert _same(h.get_orientation(0, len(pts)), labels) and _same(h.get_point_frames(0, len(pts)), frames)
    finally:
        h.close()


@pytest.mark.parametrize("algo", ["KNN_BRUTE", "KNN_GRID", "KNN_GRID_LEVELS", "KNN_TREE"])
def test_results_stay_readable_after_voxel_downsample_whichever_sweep(gpu, algo):
    """After pct_voxel_downsample the areas, the frames and the orientation refused where the uniform or the hierarchical
    list had planted the table and answered where the exhaustive sweep or the chain had -- pct_get_fit answered always.
    The header: fit results, areas, frames and the orientation computed before stay readable, whichever sweep planted."""
    capi = gpu["capi"]
    pts = gpu["shapes"].torus_random(5000, seed=8)
    n = len(pts)
    h = capi.Handle(0)
    try:
        h.set_points(pts); h.curvature(10, 0.0, getattr(capi, algo)); h.point_areas(); h.point_frames((0.0, 0.0, 9.0)); h.orient_frames("seed")
        read = lambda: (h.get_fit(0, n) + h.get_point_areas(0, n) + h.get_point_frames(0, n) + h.get_orientation(0, n),
                        h.point_energies(False), h.point_energies(True))
        before = read()
        kept = h.voxel_downsample(pts, 0.1)
        assert 0 < len(kept) < n
        with pytest.raises(AttributeError):
            h.get_neighbors(0, 1)
        after = read()
        assert _same(after[0], before[0]) and after[1:] == before[1:]
        # a query through the cell list must not rebuild it under results that are indexed by its order
        q = pts[::50].astype(np.float64) + 1e-3
        assert _same(h.query_points(q, 5, 0.0, capi.QUERY_GRID), h.query_points(q, 5, 0.0, capi.QUERY_SWEEP))
        assert _same(read()[0], before[0])
    finally:
        h.close()


def test_areas_outlive_a_cell_list_query_after_voxel_downsample(gpu):
    """Areas of a pct_knn table (no fit on the handle) live in the table's row order; with the table dropped by
    pct_voxel_downsample nothing but the areas refers to that order, and a pct_query_points_algo(PCT_QUERY_GRID) must
    not build a new cell list over it."""
    capi = gpu["capi"]
    pts = gpu["shapes"].torus_random(5000, seed=9)
    n = len(pts)
    h = capi.Handle(0)
    try:
        h.set_points(pts); h.knn(10, 0.0, capi.KNN_GRID); h.point_areas()
        before = h.get_point_areas(0, n)
        h.voxel_downsample(pts, 0.1)
        q = pts[::40].astype(np.float64)
        got = h.query_points(q, 3, 0.0, capi.QUERY_GRID)
        assert h.query_stats()["route"] == 0                # the exhaustive sweep: same rows, nothing rebuilt
        assert _same(got, h.query_points(q, 3, 0.0, capi.QUERY_SWEEP))
        assert _same(h.get_point_areas(0, n), before)
    finally:
        h.close()


def test_ball_rows_stay_readable_after_a_refused_query_ball(gpu):
    """Found by tools/fuzz_calls.py (seed 1003, profile core, step 76): a pct_query_ball refused for the state of the
    handle left the rows of the query before it resident in the library, but the binding had already forgotten their
    offsets and get_ball answered "null output"; a non-finite query was refused only after the rows had been dropped.
    The header: a query refused for its arguments or for the state of the handle leaves them."""
    capi = gpu["capi"]
    pts = gpu["shapes"].torus_random(5000, seed=11)
    q = pts[:40].astype(np.float64)
    h = capi.Handle(0)
    try:
        h.set_points(pts)
        st, off = h.query_ball(q, 0.1, capi.BALL_SORTED | capi.BALL_DISTANCES)
        assert st == 0 and off[-1] >= 40
        rows = h.get_ball(0, 40, want_dist=True)
        bad = q.copy(); bad[3, 1] = np.nan
        for refused in (lambda: h.query_ball(q, 0.1, 64), lambda: h.query_ball(q, [0.1, 0.2]), lambda: h.query_ball(bad, 0.1)):
            with pytest.raises(ValueError):
                refused()
            assert _same(h.get_ball(0, 40, want_dist=True), rows)
        h.set_query_slab(0, 1)                                # the state of the handle: a slab handle refuses the query
        with pytest.raises(ValueError, match="slab"):
            h.query_ball(q, 0.1)
        assert _same(h.get_ball(0, 40, want_dist=True), rows)
        assert np.array_equal(h.get_ball(7, 19), rows[0][off[7]:off[19]])
        h.set_query_slab(0, 0)
        st, _ = h.query_ball(q, 0.1, capi.BALL_SORTED, capi.QUERY_AUTO, 1)      # accepted, then capped: no rows are resident
        assert st == capi.PCT_ERR_LIMIT
        with pytest.raises(ValueError, match="no ball rows"):
            h.get_ball(0, 1)
    finally:
        h.close()


def test_fit_indices_is_refused_on_a_slab_handle(gpu):
    """pct_fit_indices went through on a slab handle and replaced the slab pass's results row by row: pct_slab_records
    then refused while pct_slab_counts answered.  It refuses like pct_fit; the records of the pass stay."""
    capi = gpu["capi"]
    pts = gpu["shapes"].torus_random(5000, seed=10)
    n = len(pts)
    h = capi.Handle(0)
    try:
        h.set_points(pts); h.set_query_slab(0, 1); h.curvature(10)
        with pytest.raises(ValueError, match="slab"):
            h.fit_indices(np.zeros((4, 10), np.int32))
        assert h.slab_counts(1) == [n]
        rec = h.device_alloc(n * 12)
        try:
            assert h.slab_records(rec, n) == n
        finally:
            h.device_free(rec)
    finally:
        h.close()


# ---- fans and triangles: the header's sentences a drawn sequence meets only by luck ----------------------------------------
_TRI_CLOUDS = [(300, 8), (300, 30), (5000, 8), (5000, 30)]       # (the driver's small and large size classes: 5000 points take the cell-list path)


def _triangles(h, n):
    stats = {k: v for k, v in h.point_triangle_stats().items() if not k.endswith("ms")}
    return (h.get_triangles(0, stats["triangles"]),) + h.get_point_fans(0, n), stats


def _no_triangles(h):
    for read in (lambda: h.get_triangles(0, 1), lambda: h.get_point_fans(0, 1)):
        with pytest.raises(ValueError, match="no triangles"):
            read()
    assert not any(v for k, v in h.point_triangle_stats().items())


@pytest.mark.parametrize("n,k", _TRI_CLOUDS)
def test_triangles_outlive_a_fit_new_frames_an_orientation_and_voxel_downsample(gpu, n, k):
    """The header: a fit, pct_point_frames, pct_orient_frames and pct_voxel_downsample do not drop the triangles -- they
    are kept by public index, and the winding is a snapshot of the flipped bits at the call."""
    capi = gpu["capi"]
    pts = gpu["shapes"].torus_random(n, seed=21)
    h = capi.Handle(0)
    try:
        h.set_points(pts); h.curvature(k); h.point_frames(); h.point_triangles(True)
        before, stats = _triangles(h, n)
        assert stats["rows"] == n and len(before[0]) == stats["triangles"] > 0 and before[1][-1] == len(before[2]) > 0
        for change in (h.fit, lambda: h.point_frames((0.0, 0.0, 9.0)), lambda: h.orient_frames("top"), lambda: h.voxel_downsample(pts, 0.1)):
            change()
            after = _triangles(h, n)
            assert _same(after[0], before) and after[1] == stats
        with pytest.raises(AttributeError):
            h.get_neighbors(0, 1)                             # (the table went with pct_voxel_downsample, the triangles did not)
    finally:
        h.close()


@pytest.mark.parametrize("n,k", _TRI_CLOUDS)
def test_triangles_go_with_every_planting_and_with_the_range_set_again(gpu, n, k):
    """The header: a new cloud, a change of ownership and every planting drop the triangles -- all four plantings, and
    pct_set_query_range also where the range is the one already set."""
    capi = gpu["capi"]
    pts = gpu["shapes"].torus_random(n, seed=22)
    h = capi.Handle(0)
    try:
        h.set_points(pts)
        for drop in (lambda: h.knn(k), lambda: h.curvature(k), lambda: h.surface_variation(k + 1), lambda: h.pca_curvatures(k), lambda: h.set_query_range(0, n)):
            h.knn(k); h.point_triangles()
            assert h.point_triangle_stats()["triangles"] > 0 and len(h.get_triangles(0, 1)) == 1
            drop()
            _no_triangles(h)
    finally:
        h.close()


@pytest.mark.parametrize("n,k", _TRI_CLOUDS)
def test_refused_point_triangles_keeps_the_triangles(gpu, n, k):
    """The header: a refused call changes nothing -- pct_point_triangles drops the triangles of an earlier call behind
    its last refusal, so an unknown flag bit or PCT_TRI_WIND_FRAMES without frames leaves them."""
    capi = gpu["capi"]
    pts = gpu["shapes"].torus_random(n, seed=23)
    h = capi.Handle(0)
    try:
        h.set_points(pts); h.knn(k); h.point_triangles()
        before, stats = _triangles(h, n)
        for refused, why in ((lambda: h.point_triangles(False, flags=64), "unknown flags"), (lambda: h.point_triangles(True), "no point frames")):
            with pytest.raises(ValueError, match=why):
                refused()
            after = _triangles(h, n)
            assert _same(after[0], before) and after[1] == stats
    finally:
        h.close()

"""The cell-list build of the whole-cloud paths: the two-level LDS counting sort (k_bin_*) against the per-point-atomics
build it replaces (PCT_GRID_ATOMIC=1, read per call).

The order of the points inside a cell is arbitrary in both builds, the sweep breaks exact distance ties by public index
and the fit walks the rows in table order: every case asserts EQUAL neighbour indices, distances, K and H, bit for bit,
and checks a sample against the oracle where the cloud has no exact distance ties (distances only where it has).
"""
import numpy as np
import pytest

import pct_oracle as oracle

pytestmark = pytest.mark.gpu


def _set_build(monkeypatch, atomic):
    if atomic:
        monkeypatch.setenv("PCT_GRID_ATOMIC", "1")
    else:
        monkeypatch.delenv("PCT_GRID_ATOMIC", raising=False)


def _result(h, lo, hi):
    i, d, _ = h.get_neighbors(lo, hi)
    _, K, H, _ = h.get_fit(lo, hi, coefs=False, H2=False)
    return i, d, K, H


def _assert_same(a, b, what=""):
    for x, y, name in zip(a, b, ("indices", "distances", "K", "H")):
        assert np.array_equal(x, y, equal_nan=True), f"{what}: {name} differ between the two builds"


def _run(capi, monkeypatch, pts, k, atomic, qrange=None, eps=0.0):
    """One call on a fresh handle (the packed first-call build)."""
    _set_build(monkeypatch, atomic)
    h = capi.Handle(0)
    h.set_points(pts)
    lo, hi = qrange if qrange else (0, len(pts))
    if qrange:
        h.set_query_range(lo, hi)
    h.curvature(k, eps, capi.KNN_GRID)
    out = _result(h, lo, hi)
    t = h.timings()
    h.close()
    return out, t


def _both(capi, monkeypatch, pts, k, qrange=None):
    new, t_new = _run(capi, monkeypatch, pts, k, False, qrange)
    old, t_old = _run(capi, monkeypatch, pts, k, True, qrange)
    _assert_same(new, old, f"n={len(pts)} k={k} range={qrange}")
    assert t_new["cells"] == t_old["cells"] and t_new["grid_iters"] == t_old["grid_iters"]
    assert t_new["grid_points"] == t_old["grid_points"]
    return new, t_new


def _oracle_sample(pts, k, result, lo=0, rows=2000, seed=0, indices=True):
    """Sampled rows of result (table rows lo..) against cKDTree on the float32-rounded cloud."""
    i, d = result[0], result[1]
    rng = np.random.default_rng(seed)
    pick = np.unique(rng.integers(0, len(i), size=min(rows, len(i))))
    ri, rd = oracle.knn(pts, k, query_rows=pick + lo)
    assert np.array_equal(d[pick], rd)
    if indices:
        assert np.array_equal(i[pick], ri)


@pytest.mark.parametrize("n", [1_000_000, 100_000, 5_000, 700, 51])
def test_random_torus_sizes(gpu, monkeypatch, n):
    """1 M, 100 k, 5 k points, fewer points than one input tile, n = k + 1."""
    pts = gpu["shapes"].torus_random(n, seed=1234 if n == 1_000_000 else 21)
    new, _ = _both(gpu["capi"], monkeypatch, pts, 50)
    _oracle_sample(pts, 50, new)


def test_the_new_build_is_the_one_that_runs(gpu, monkeypatch, capfd):
    """PCT_GRID_DEBUG names the build: the counting sort by default, none of it under PCT_GRID_ATOMIC=1."""
    capi = gpu["capi"]
    pts = gpu["shapes"].torus_random(100_000, seed=3)
    monkeypatch.setenv("PCT_GRID_DEBUG", "1")
    capfd.readouterr()
    _run(capi, monkeypatch, pts, 50, False)
    assert "[grid] bin build:" in capfd.readouterr().err
    _run(capi, monkeypatch, pts, 50, True)
    assert "[grid] bin build:" not in capfd.readouterr().err


def _dense_theta_torus(n, seed, like):
    """The box of the torus `like` with another density: 90 % of the points on a quarter of the major circle."""
    rng = np.random.default_rng(seed)
    theta = np.where(rng.uniform(size=n) < 0.9, rng.uniform(0, np.pi / 2, size=n), rng.uniform(0, 2 * np.pi, size=n))
    phi = rng.uniform(0, 2 * np.pi, size=n)
    ref = np.abs(like).max(0)                                         # (R + r, R + r, r)
    r = ref[2]
    R = ref[0] - r
    return np.stack([(R + r * np.cos(phi)) * np.cos(theta), (R + r * np.cos(phi)) * np.sin(theta), r * np.sin(phi)], 1).astype(np.float32)


def test_stream_of_clouds_on_one_handle(gpu, monkeypatch):
    """Cloud A, A again (speculative box: one pass, the caller's rows are binned directly), a cloud with another box
    (restart the regular way), a cloud with the same box and another density (a second pass with another cell size --
    scratch sized per pass).  Two handles take the same stream, one per build."""
    capi, shapes = gpu["capi"], gpu["shapes"]
    n, k = 150_000, 50
    A = shapes.torus_random(n, seed=8)
    A2 = shapes.torus_random(n, seed=9)
    B = (2.5 * shapes.torus_random(n, seed=10) + np.float32(4.0)).astype(np.float32)
    C = _dense_theta_torus(n, seed=11, like=A)
    h_new, h_old = capi.Handle(0), capi.Handle(0)
    iters = []
    for step, pts in enumerate((A, A, A2, B, B, C, A)):
        res = []
        for h, atomic in ((h_new, False), (h_old, True)):
            _set_build(monkeypatch, atomic)
            h.set_points(pts)
            h.curvature(k, 0.0, capi.KNN_GRID)
            res.append((_result(h, 0, n), h.timings()))
        _assert_same(res[0][0], res[1][0], f"stream step {step}")
        assert res[0][1]["grid_iters"] == res[1][1]["grid_iters"] and res[0][1]["cells"] == res[1][1]["cells"]
        iters.append(res[0][1]["grid_iters"])
        _oracle_sample(pts, k, res[0][0], rows=500, seed=step)
    assert iters[1] == 1 and iters[2] == 1, iters        # the speculative path: one pass
    assert iters[5] >= 2, iters                          # the other density: the first cell size was rejected
    h_new.close()
    h_old.close()


@pytest.mark.parametrize("cull", [True, False])
def test_index_range_shards(gpu, monkeypatch, cull):
    """q_begin > 0 and q_end < n, with the range-culled pack (scan order) and without it (PCT_NO_CULL)."""
    capi = gpu["capi"]
    pts = gpu["shapes"].torus_random(120_000, seed=16)
    theta = np.arctan2(pts[:, 1], pts[:, 0])
    pts = np.ascontiguousarray(pts[np.argsort(theta, kind="stable")])
    n = len(pts)
    if not cull:
        monkeypatch.setenv("PCT_NO_CULL", "1")
    whole, _ = _both(capi, monkeypatch, pts, 50)
    for lo, hi in ((n // 4, n // 2), (n // 2 + 17, n - 5)):
        part, t = _both(capi, monkeypatch, pts, 50, qrange=(lo, hi))
        assert (t["grid_points"] < n) == cull, t
        _assert_same(part, tuple(x[lo:hi] for x in whole), f"shard [{lo}, {hi})")
    # the steady state of a sharded handle that is not culled: the speculative build with two classes
    if not cull:
        lo, hi = n // 4, n // 2
        res = []
        for atomic in (False, True):
            _set_build(monkeypatch, atomic)
            h = capi.Handle(0)
            for _ in range(2):
                h.set_points(pts)
                h.set_query_range(lo, hi)
                h.curvature(50, 0.0, capi.KNN_GRID)
            res.append(_result(h, lo, hi))
            h.close()
        _assert_same(res[0], res[1], "sharded, second call")
        _assert_same(res[0], tuple(x[lo:hi] for x in whole), "sharded, second call against the whole cloud")


def test_float64_cloud(gpu, monkeypatch):
    """Native float64 records ride along (sorted4d); first call and steady state, whole cloud and a shard."""
    capi = gpu["capi"]
    pts = gpu["shapes"].torus_random(80_000, seed=5, dtype=np.float64)
    new, _ = _both(capi, monkeypatch, pts, 50)
    _oracle_sample(pts, 50, new)
    _both(capi, monkeypatch, pts, 50, qrange=(10_000, 70_001))
    res = []
    for atomic in (False, True):
        _set_build(monkeypatch, atomic)
        h = capi.Handle(0)
        for _ in range(3):
            h.set_points(pts)
            h.curvature(50, 0.0, capi.KNN_GRID)
        res.append(_result(h, 0, len(pts)))
        h.close()
    _assert_same(res[0], res[1], "float64 steady state")
    _assert_same(res[0], new, "float64 steady state against the first call")


def test_all_points_in_one_cell_and_on_one_line(gpu, monkeypatch):
    capi = gpu["capi"]
    same = np.tile(np.array([[0.25, -1.0, 3.0]], np.float32), (3000, 1))
    new, _ = _both(capi, monkeypatch, same, 20)
    assert (new[1] == 0).all()
    t = np.random.default_rng(4).uniform(-1, 1, size=20_000).astype(np.float32)
    line = np.stack([t, 2 * t, -0.5 * t], 1).astype(np.float32)
    new, _ = _both(capi, monkeypatch, line, 20)
    _oracle_sample(line, 20, new, indices=False)


def test_far_outliers_share_the_boundary_cells(gpu, monkeypatch):
    """1 % of the points far outside: the grid box is trimmed, the outliers are clamped into boundary cells."""
    capi = gpu["capi"]
    rng = np.random.default_rng(12)
    pts = gpu["shapes"].torus_random(100_000, seed=4)
    far = (rng.normal(size=(1000, 3)) * 60.0).astype(np.float32)
    both = np.ascontiguousarray(np.vstack([pts, far])[rng.permutation(len(pts) + len(far))])
    new, t = _both(capi, monkeypatch, both, 30)
    assert t["cell_size"] < 1.5 * _run(capi, monkeypatch, pts, 30, False)[1]["cell_size"]
    _oracle_sample(both, 30, new)
    # steady state on the trimmed (speculative) box
    res = []
    for atomic in (False, True):
        _set_build(monkeypatch, atomic)
        h = capi.Handle(0)
        for _ in range(2):
            h.set_points(both)
            h.curvature(30, 0.0, capi.KNN_GRID)
        res.append(_result(h, 0, len(both)))
        h.close()
    _assert_same(res[0], res[1], "outliers, steady state")
    _assert_same(res[0], new, "outliers, steady state against the first call")


def test_dense_minority_takes_the_shared_bucket_path(gpu, monkeypatch, capfd):
    """90 % of the points in 1 % of the box (a thin slab at its floor): whole buckets of cells are full, a bucket holds
    several work items' worth of records and its items share the bucket's cells."""
    capi = gpu["capi"]
    rng = np.random.default_rng(31)
    n = 300_000
    pts = rng.uniform(0, 1, size=(n, 3))
    pts[: 9 * n // 10, 2] *= 0.01
    pts = np.ascontiguousarray(pts[rng.permutation(n)].astype(np.float32))
    monkeypatch.setenv("PCT_GRID_DEBUG", "1")
    capfd.readouterr()
    new, _ = _run(capi, monkeypatch, pts, 30, False)
    err = capfd.readouterr().err
    lines = [ln for ln in err.splitlines() if ln.startswith("[grid] bin build:")]
    assert lines, err
    shared = [int(ln.split(" of them in ")[1].split()[0]) for ln in lines]
    assert max(shared) >= 1, lines                         # the multi-block path ran
    monkeypatch.delenv("PCT_GRID_DEBUG")
    old, _ = _run(capi, monkeypatch, pts, 30, True)
    _assert_same(new, old, "dense minority")
    _oracle_sample(pts, 30, new)
    # the same through the caller's rows (steady state)
    res = []
    for atomic in (False, True):
        _set_build(monkeypatch, atomic)
        h = capi.Handle(0)
        for _ in range(2):
            h.set_points(pts)
            h.curvature(30, 0.0, capi.KNN_GRID)
        res.append(_result(h, 0, n))
        h.close()
    _assert_same(res[0], res[1], "dense minority, steady state")
    _assert_same(res[0], new, "dense minority, steady state against the first call")


def test_non_finite_row_is_still_refused(gpu, monkeypatch):
    """On the first call by the pack, in the steady state by the binning pass's own record."""
    capi = gpu["capi"]
    pts = gpu["shapes"].torus_random(50_000, seed=2)
    bad = pts.copy()
    bad[31_337, 1] = np.nan
    for atomic in (False, True):
        _set_build(monkeypatch, atomic)
        h = capi.Handle(0)
        h.set_points(bad)
        with pytest.raises(ValueError, match="Non-finite values in input points"):
            h.curvature(50, 0.0, capi.KNN_GRID)
        h.set_points(pts)
        h.curvature(50, 0.0, capi.KNN_GRID)
        h.set_points(bad)                                   # same size, the previous cloud's box: the speculative build
        with pytest.raises(ValueError, match="Non-finite values in input points"):
            h.curvature(50, 0.0, capi.KNN_GRID)
        h.set_points(pts)
        h.curvature(50, 0.0, capi.KNN_GRID)                 # the handle goes on
        good = _result(h, 0, 1000)
        h.close()
        ref, _ = _run(capi, monkeypatch, pts, 50, atomic)
        _assert_same(good, tuple(x[:1000] for x in ref), "after a refused cloud")


def test_async_stream_over_alternating_clouds_equals_the_blocking_run(gpu, monkeypatch):
    capi, shapes = gpu["capi"], gpu["shapes"]
    n, k = 120_000, 50
    clouds = [shapes.torus_random(n, seed=41), shapes.torus_random(n, seed=42),
              (1.7 * shapes.torus_random(n, seed=43) - np.float32(2.0)).astype(np.float32)]
    order = [0, 1, 0, 2, 2, 1, 0]
    blocking = {}
    _set_build(monkeypatch, False)
    for j in set(order):
        blocking[j], _ = _run(capi, monkeypatch, clouds[j], k, False)
    for atomic in (False, True):
        _set_build(monkeypatch, atomic)
        h = capi.Handle(0)
        h.set_async(True)
        for step, j in enumerate(order):
            h.set_points(clouds[j])
            h.curvature(k, 0.0, capi.KNN_GRID)
            if step % 2:                                    # (every other result is read back: that waits for the call)
                _assert_same(_result(h, 0, n), blocking[j], f"async step {step} atomic={atomic}")
        _assert_same(_result(h, 0, n), blocking[order[-1]], f"async last step atomic={atomic}")
        h.close()


def test_row_table_is_built_on_first_need(gpu, monkeypatch):
    """The counting sort leaves row_of to the first call that gathers through it: listed rows, the fit's download, ranges
    that do not start at the handle's first row, and a second build on the same handle in between."""
    capi = gpu["capi"]
    pts = gpu["shapes"].torus_random(60_000, seed=13)
    rows = np.array([0, 1, 777, 31_337, 59_999], dtype=np.int64)
    out = []
    for atomic in (False, True):
        _set_build(monkeypatch, atomic)
        h = capi.Handle(0)
        h.set_points(pts)
        h.curvature(30, 0.0, capi.KNN_GRID)
        first = h.get_neighbor_rows(rows)[:2]                 # (the first reader of the row table)
        h.set_points(pts)
        h.curvature(30, 0.0, capi.KNN_GRID)                   # steady state: another list, the table is stale again
        again = h.get_neighbor_rows(rows)[:2]
        part = _result(h, 20_000, 20_500)
        h.set_query_range(10_000, 50_000)
        h.curvature(30, 0.0, capi.KNN_GRID)
        shard = h.get_neighbor_rows(rows[3:4])[:2] + _result(h, 30_000, 30_100)
        h.close()
        out.append((first, again, part, shard))
    for a, b in zip(out[0], out[1]):
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True)
    ri, rd = oracle.knn(pts, 30, query_rows=rows)
    for got in (out[0][0], out[0][1]):
        assert np.array_equal(got[0], ri) and np.array_equal(got[1], rd)

"""The counting sort's bucket-local cell scan: k_bin_cells leaves one scan record per bucket, k_scan_tiles scans those,
k_bin_place scans inside its bucket and writes cell_start / own_start / occ -- against the builds that keep the three-kernel
scan over the cells (PCT_GRID_ATOMIC=1, read per call).

The shapes are the smallest at which the bucket-local scan can go wrong: a bucket shared by several work items (the ticket
and the read-back of the final counts), a ragged last bucket, whole empty buckets, two classes (cell_oth and the row
offsets), float64 records, the caller's rows in the steady state (blocking and asynchronous) and one cell that holds
everything.  Every case asserts EQUAL neighbour indices, distances, K and H, bit for bit (the helpers' pattern of
test_gpu_grid_build.py).
"""
import numpy as np
import pytest

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


def _run(capi, monkeypatch, pts, k, atomic, qrange=None, calls=1, use_async=False):
    """`calls` consecutive set_points + curvature on one handle (the second and later ones bin the caller's rows on the
    previous call's box); the results of the last one."""
    _set_build(monkeypatch, atomic)
    h = capi.Handle(0)
    if use_async:
        h.set_async(True)
    lo, hi = qrange if qrange else (0, len(pts))
    for _ in range(calls):
        h.set_points(pts)
        if qrange:
            h.set_query_range(lo, hi)
        h.curvature(k, 0.0, capi.KNN_GRID)
    if use_async:
        h.synchronize()
    out = _result(h, lo, hi)
    t = h.timings()
    h.close()
    return out, t


def _both(capi, monkeypatch, pts, k, **kw):
    new, t_new = _run(capi, monkeypatch, pts, k, False, **kw)
    old, t_old = _run(capi, monkeypatch, pts, k, True, **kw)
    _assert_same(new, old, f"n={len(pts)} k={k} {kw}")
    assert t_new["cells"] == t_old["cells"] and t_new["grid_iters"] == t_old["grid_iters"]
    assert t_new["grid_points"] == t_old["grid_points"]
    return new, t_new


def _bin_lines(err):
    """(buckets, cells per bucket, items in shared buckets, shared buckets) of every '[grid] bin build:' line."""
    out = []
    for ln in err.splitlines():
        if ln.startswith("[grid] bin build:"):
            w = ln.split()
            out.append((int(w[3]), int(w[6]), int(ln.split(" of them in ")[0].split()[-1]), int(ln.split(" of them in ")[1].split()[0])))
    return out


def _debug_run(capi, monkeypatch, capfd, pts, k, **kw):
    """The default build with PCT_GRID_DEBUG=1: its results, its timings and its bin-build lines."""
    monkeypatch.setenv("PCT_GRID_DEBUG", "1")
    capfd.readouterr()
    new, t = _run(capi, monkeypatch, pts, k, False, **kw)
    err = capfd.readouterr().err
    monkeypatch.delenv("PCT_GRID_DEBUG")
    lines = _bin_lines(err)
    assert lines, err
    return new, t, lines


@pytest.fixture(scope="module")
def dense_slab():
    """20 000 uniform points, 12 000 of them squeezed into 1 % of the z axis (the slowest cell coordinate): the cells of
    the bottom layer fill one bucket of 256 cells with more than chunk = 4096 records."""
    rng = np.random.default_rng(77)
    n = 20_000
    pts = rng.uniform(0, 1, size=(n, 3))
    pts[:12_000, 2] *= 0.01
    pts = np.ascontiguousarray(pts[rng.permutation(n)].astype(np.float32))
    pts.setflags(write=False)
    return pts


def test_shared_bucket(gpu, monkeypatch, capfd, dense_slab):
    capi = gpu["capi"]
    new, _, lines = _debug_run(capi, monkeypatch, capfd, dense_slab, 10)
    assert max(ln[3] for ln in lines) >= 1, lines             # a bucket with several items: the ticket path ran
    assert max(ln[2] for ln in lines) >= 3, lines
    old, _ = _run(capi, monkeypatch, dense_slab, 10, True)
    _assert_same(new, old, "shared bucket")


def test_two_classes_on_the_shared_bucket(gpu, monkeypatch, capfd, dense_slab):
    """An index-range handle over the middle third: cell_oth, the other class's cursors and the s_row offsets."""
    capi = gpu["capi"]
    n = len(dense_slab)
    q = (n // 3, 2 * n // 3)
    new, _, lines = _debug_run(capi, monkeypatch, capfd, dense_slab, 10, qrange=q)
    assert max(ln[3] for ln in lines) >= 1, lines
    old, _ = _run(capi, monkeypatch, dense_slab, 10, True, qrange=q)
    _assert_same(new, old, "two classes")
    whole, _ = _run(capi, monkeypatch, dense_slab, 10, False)
    _assert_same(new, tuple(x[q[0]:q[1]] for x in whole), "two classes against the whole cloud")


def test_ragged_last_bucket(gpu, monkeypatch, capfd):
    """ncell is no multiple of the bucket size: the last bucket holds fewer cells than the others (and the two end
    entries of cell_start / own_start)."""
    capi = gpu["capi"]
    pts = gpu["shapes"].torus_random(5_000, seed=6)
    new, t, lines = _debug_run(capi, monkeypatch, capfd, pts, 10)
    nb, cpb = lines[-1][0], lines[-1][1]
    assert t["cells"] % cpb != 0 and nb == -(-t["cells"] // cpb), (t["cells"], lines)
    old, _ = _run(capi, monkeypatch, pts, 10, True)
    _assert_same(new, old, "ragged last bucket")


def test_whole_empty_buckets(gpu, monkeypatch, capfd):
    """Two clusters of 5 000 points far apart along z: the buckets between them hold no record at all, and their one item
    still writes their cells' starts."""
    capi = gpu["capi"]
    rng = np.random.default_rng(5)
    pts = rng.uniform(0, 1, size=(10_000, 3))
    pts[5_000:, 2] += 20.0
    pts = np.ascontiguousarray(pts[rng.permutation(len(pts))].astype(np.float32))
    new, t, lines = _debug_run(capi, monkeypatch, capfd, pts, 10)
    nb, cpb = lines[-1][0], lines[-1][1]
    # the buckets that lie wholly inside the gap: z layers above the first cluster and below the second
    a = t["cell_size"]
    nx, ny = int((pts[:, 0].max() - pts[:, 0].min()) / a) + 1, int((pts[:, 1].max() - pts[:, 1].min()) / a) + 1
    first_empty_cell = (int(1.0 / a) + 2) * nx * ny
    last_empty_cell = (int(20.0 / a) - 2) * nx * ny
    assert last_empty_cell // cpb - (first_empty_cell + cpb - 1) // cpb >= 1, (t, lines)
    assert nb > 2
    old, _ = _run(capi, monkeypatch, pts, 10, True)
    _assert_same(new, old, "empty buckets")


def test_float64_cloud(gpu, monkeypatch):
    """The sorted4d path: float64 records ride along."""
    pts = gpu["shapes"].torus_random(10_000, seed=15, dtype=np.float64)
    _both(gpu["capi"], monkeypatch, pts, 10)


@pytest.mark.parametrize("use_async", [False, True])
def test_steady_state_over_the_callers_rows(gpu, monkeypatch, dense_slab, use_async):
    """Two consecutive set_points + curvature on one handle: the second builds on the first's box from the caller's
    rows; blocking, and asynchronous ended by synchronize."""
    capi = gpu["capi"]
    twice, t = _both(capi, monkeypatch, dense_slab, 10, calls=2, use_async=use_async)
    assert t["grid_iters"] == 1, t
    once, _ = _run(capi, monkeypatch, dense_slab, 10, False)
    _assert_same(twice, once, "second call against a fresh handle's first")


def test_all_points_in_one_cell(gpu, monkeypatch):
    """One bucket holds everything and there is one rank chain."""
    same = np.tile(np.array([[0.25, -1.0, 3.0]], np.float32), (3000, 1))
    new, t = _both(gpu["capi"], monkeypatch, same, 20)
    assert t["cells"] == 1
    assert (new[1] == 0).all()

"""k_fit's register stash (KEEP, pct_fit.hip): the first min(m, KEEP) neighbours of a row stay in registers from pass 1
to pass 2.  Only where an operand comes from changes, so every built depth must give the BITS of depth 0.

PCT_FIT_KEEP=<depth> is read per call, so the reference of every case is the same handle with PCT_FIT_KEEP=0.  Equality
is on the raw float32 words of the coefficients, K, H and H^2 (NaNs in the same places, with the same payload), and on
the number of rows handed to k_fit_svd.

  rows       64 * 3 + 5 rows (a partial last block) through pct_fit_indices at k = 6 .. 63: below, at and above every
             depth and the eight-wide unroll
  short      eps-bounded fused calls: rows of m < k neighbours, m < KEEP and m < 6 (k_fit_svd's rows) among them
  caller     pct_fit_indices with counts, a foreign query and one entry outside the cloud (the row reads NaN)
  sick       collinear and duplicate-point neighbourhoods: the same rows go to k_fit_svd
  bench      a 20 000-point torus through the fused call at k = 50, the default depth against 0
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEPTHS = [8, 10, 16, 25, 50]
KS = [6, 7, 8, 9, 10, 11, 15, 16, 17, 24, 25, 26, 49, 50, 51, 63]
ROWS = 64 * 3 + 5


@pytest.fixture
def handle(gpu):
    h = gpu["capi"].Handle(0)
    yield h
    h.close()


def _depth(monkeypatch, depth):
    if depth is None:
        monkeypatch.delenv("PCT_FIT_KEEP", raising=False)
    else:
        monkeypatch.setenv("PCT_FIT_KEEP", str(depth))


def _words(handle, rows):
    co, K, H, H2 = handle.get_fit(0, rows)
    return [np.ascontiguousarray(a).view(np.uint32).copy() for a in (co, K, H, H2)] + [int(handle.timings()["fit_svd_rows"])]


def _same(got, ref, what):
    for name, a, b in zip(("coefs", "K", "H", "H2"), got, ref):
        assert np.array_equal(a, b), (what, name, np.flatnonzero((a != b).reshape(len(b), -1).any(1))[:8])
    assert got[4] == ref[4], (what, "rows to k_fit_svd", got[4], ref[4])


def _brute_rows(pts, k):
    """(n, k) nearest rows by brute force, self first: any fixed rows would do, these are neighbourhoods."""
    p = pts.astype(np.float64)
    d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    return np.argsort(d, axis=1, kind="stable")[:, :k].astype(np.int32)


@pytest.fixture(scope="module")
def small(built):
    pts = built["shapes"].torus_random(ROWS, seed=77)
    return pts, _brute_rows(pts, max(KS))


# ------------------------------------------------------------------------------------------------ rows
def test_every_depth_at_every_row_length(handle, monkeypatch, small):
    pts, idx = small
    handle.set_points(pts)
    finite = 0
    for k in KS:
        rows = np.ascontiguousarray(idx[:, :k])
        _depth(monkeypatch, 0)
        handle.fit_indices(rows)
        ref = _words(handle, ROWS)
        finite += int(np.isfinite(ref[1].view(np.float32)).sum())
        for depth in DEPTHS:
            _depth(monkeypatch, depth)
            handle.fit_indices(rows)
            _same(_words(handle, ROWS), ref, (k, depth))
    assert finite > 0.9 * ROWS * len(KS)                     # fits, not rows of NaN


# ------------------------------------------------------------------------------------------------ short
@pytest.mark.parametrize("k,mean", [(30, 9), (63, 30)])
def test_eps_bounded_rows(handle, gpu, monkeypatch, k, mean):
    pts = gpu["shapes"].torus_random(2000, seed=78)
    p = pts.astype(np.float64)
    d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))
    eps = float(np.median(np.sort(d, axis=1)[:, mean]))       # about `mean` neighbours inside the bound, self included
    handle.set_points(pts)
    ref = cnt = None
    for depth in [0] + DEPTHS:
        _depth(monkeypatch, depth)
        handle.curvature(k, eps=eps, algo=gpu["capi"].KNN_GRID)
        got = _words(handle, len(pts))
        if depth == 0:
            ref = got
            cnt = handle.get_neighbors(0, len(pts), want_idx=False, want_dist=False, want_count=True)[2]
            assert (cnt < k).any() and (cnt >= 6).any()
            edges = [6, 8, 10] if mean == 9 else [16, 25, 50]
            assert cnt.min() < edges[0] and all((cnt < e).any() and (cnt >= e).any() for e in edges), (cnt.min(), cnt.max())
            assert not (mean == 9 and ref[4] == 0)            # m in [2, 6): rows handed to k_fit_svd
        else:
            _same(got, ref, (k, depth))


# ------------------------------------------------------------------------------------------------ caller
def test_caller_rows_with_an_entry_outside_the_cloud(handle, monkeypatch, small):
    pts, idx = small
    k = 26
    rows = np.ascontiguousarray(idx[:, :k]).copy()
    rng = np.random.default_rng(79)
    count = rng.integers(0, k + 1, ROWS).astype(np.int32)
    count[:8] = [0, 1, 2, 5, 6, 8, 25, 26]
    query = rng.permutation(ROWS).astype(np.int64)           # foreign queries: rows centred on another point
    handle.set_points(pts)
    bad = [20, 70, 130, ROWS - 1]                            # rows with an entry outside the cloud, at four places of a row
    count[bad] = [26, 26, 12, 26]
    rows[20, 0] = 2_000_000_000
    rows[70, 9] = -3
    rows[130, 11] = ROWS
    rows[ROWS - 1, 25] = ROWS + 5
    monkeypatch.setenv("PCT_TRUST_ROWS", "1")                # the host's validation off: the kernel's own clamp answers
    ref = None
    for depth in [0] + DEPTHS:
        _depth(monkeypatch, depth)
        handle.fit_indices(rows, count=count, query=query)
        got = _words(handle, ROWS)
        if depth == 0:
            ref = got
            K = ref[1].view(np.float32)
            assert np.isnan(K[bad]).all() and np.isfinite(K[count >= 6]).mean() > 0.8
        else:
            _same(got, ref, depth)


# ------------------------------------------------------------------------------------------------ sick
def test_ill_conditioned_rows_are_handed_over_alike(handle, monkeypatch, small):
    pts, _ = small
    t = np.linspace(0.0, 1.0, 70, dtype=np.float32)
    line = np.stack([2.0 + 0.3 * t, 2.0 - 0.2 * t, 0.5 * t], 1).astype(np.float32)     # collinear neighbourhoods
    dup = np.repeat(np.array([[-2.0, 1.5, 0.25]], np.float32), 70, 0)                  # 70 copies of one point
    cloud = np.concatenate([pts, line, dup])
    idx = _brute_rows(cloud, 26)
    handle.set_points(cloud)
    ref = None
    for k in (10, 26):
        rows = np.ascontiguousarray(idx[:, :k])
        for depth in [0] + DEPTHS:
            _depth(monkeypatch, depth)
            handle.fit_indices(rows)
            got = _words(handle, len(cloud))
            if depth == 0:
                ref = got
                assert ref[4] >= 140, ref[4]                  # the line's and the duplicates' rows, at least
            else:
                _same(got, ref, (k, depth))


# ------------------------------------------------------------------------------------------------ bench
def test_bench_kernel_default_depth_against_none(handle, gpu, monkeypatch):
    pts = gpu["shapes"].torus_random(20000, seed=1234)
    handle.set_points(pts)
    out = {}
    for depth in (0, None):
        _depth(monkeypatch, depth)
        handle.curvature(50)
        out[depth] = _words(handle, len(pts))
    assert np.isfinite(out[0][1].view(np.float32)).all()
    _same(out[None], out[0], "default")

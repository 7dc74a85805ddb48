"""The reference of the wide-row tests checked on the CPU: tests/wide_exact.py against SciPy where SciPy's answer is
defined (no exact ties), and the properties of its clouds that tests/test_gpu_wide_rows.py relies on -- asserted on the
reference alone, no device involved."""
import numpy as np
import pytest

import pct_oracle as oracle
import wide_exact as we

KS = (128, 256, 511)


@pytest.fixture(scope="module")
def ranking():
    made = {}

    def get(name):
        if name not in made:
            pts = {"lattice": we.lattice, "twins": we.twins, "clump": we.clump, "f64": we.f64, "torus32": we.torus,
                   "torus64": lambda: we.torus(np.float64)}[name]()
            made[name] = (pts, we.ranked(pts))
        return made[name]
    return get


def test_one_ranking_serves_every_row_length():
    """``ranked`` pre-selects by the 513th smallest d2 before it sorts: the plain lexsort of every point gives the same
    order, and a row computed on its own is the prefix of the ranking."""
    pts = we.lattice()
    rows = np.arange(0, len(pts), 137)
    full = we.ranked(pts, rows=rows)
    cand = pts.astype(np.float64)
    for o, r in enumerate(rows):
        d = cand - cand[r]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        order = np.lexsort((np.arange(len(pts)), d2))[:we.WIDTH]
        assert np.array_equal(order, full[0][o]) and np.array_equal(d2[order], full[1][o])
    for k in (128, 300, 511):
        alone = we.rows(pts, k, rows=rows)
        prefix = we.rows(pts, k, rows=rows, ranking=full)
        assert all(np.array_equal(a, b) for a, b in zip(alone, prefix))
        assert alone[0].dtype == np.int32 and alone[1].dtype == np.float32 and (alone[2] == k).all()


def test_the_restated_torus_is_the_packages(built):
    sh = built["shapes"]
    for dtype in (np.float32, np.float64):
        assert np.array_equal(sh.torus_random(6000, seed=we.SEED_TORUS, dtype=dtype), we.torus(dtype))
    assert np.array_equal(sh.torus_random(3000, seed=we.SEED_F64, dtype=np.float64) * 0.2 + 40.0, we.f64())


@pytest.mark.parametrize("name", ["torus32", "torus64", "f64", "clump"])
def test_tie_free_clouds_equal_scipy_bit_for_bit(ranking, name):
    pts, rk = ranking(name)
    assert not (np.diff(rk[1], axis=1) == 0).any()                   # no exact tie anywhere in the first 513 entries
    for k in KS:
        idx, dist, count = we.rows(pts, k, ranking=rk)
        ref_idx, ref_dist = oracle.knn(pts, k)
        assert np.array_equal(idx, ref_idx) and np.array_equal(dist, ref_dist) and (count == k).all()


@pytest.mark.parametrize("name", ["lattice", "twins"])
def test_clouds_with_ties_equal_scipy_where_it_is_defined(ranking, name):
    """Distances everywhere; index sets on every row without a tie at the cut (a tie between elements 0 and 1 -- which
    coinciding point is dropped -- only occurs on rows that have one at the cut as well)."""
    pts, rk = ranking(name)
    for k in KS:
        idx, dist, _ = we.rows(pts, k, ranking=rk)
        ref_idx, ref_dist = oracle.knn(pts, k)
        assert np.array_equal(dist, ref_dist)
        cut = we.tie_at(rk, k)
        assert not (we.tie_at(rk, 0) & ~cut).any()
        assert 0 < (~cut).sum()
        assert np.array_equal(np.sort(idx[~cut], axis=1), np.sort(ref_idx[~cut], axis=1))
        assert (np.sort(idx[cut], axis=1) != np.sort(ref_idx[cut], axis=1)).any()        # ... and SciPy is no bar beyond


def test_eps_rows_of_the_lattice(ranking):
    """Counts and distances are SciPy's (``distance_upper_bound`` is strict as well); some rows are cut short, others
    full, and points lie exactly at distance eps -- the strictness decides entries."""
    pts, rk = ranking("lattice")
    for k, eps in we.EPS_CASES:
        assert float(np.float64(eps) * np.float64(eps)) == eps ** 2 and (eps * 16) ** 2 == int((eps * 16) ** 2)
        idx, dist, count = we.rows(pts, k, eps=eps, ranking=rk)
        _, ref_dist, ref_count = oracle.knn(pts, k, eps=eps)
        assert np.array_equal(count, ref_count) and np.array_equal(dist, ref_dist)
        full = (count == k).mean()
        assert 0.3 < full < 0.75 and 6 <= count.min() < k // 2, (k, eps, full, count.min())
        assert (rk[1] == eps * eps).sum() > 1000
        at_eps = (rk[1][:, 1:k + 1] == eps * eps)                   # entries the strict bound drops from within a row
        assert at_eps.any() and not np.isfinite(dist[at_eps]).any() and (idx[at_eps] == len(pts)).all()
        behind = np.arange(k)[None, :] >= count[:, None]
        assert (idx[behind] == len(pts)).all() and np.isinf(dist[behind]).all() and np.isfinite(dist[~behind]).all()


def test_ties_of_the_lattice_straddle_list_registers_and_cuts(ranking):
    """Element i of the running list sits in lane i % 64 of list register i // 64: equal keys in entries 63 | 64 and
    255 | 256 are compared across registers (and, for 255 | 256, only exist in the 512-wide list); a tie at k | k + 1
    is decided at the cut.  Measured: 100 % of the rows tie at 63 | 64, 89.5 % at 255 | 256, 99.1 % / 89.5 % / 89.5 % /
    87.5 % at the cut of k = 128 / 255 / 256 / 511; the first 512 entries of a row hold 23 ... 74 distinct distances,
    the longest run of equal keys in a row is 18 ... 52 entries (median 37)."""
    pts, rk = ranking("lattice")
    assert we.tie_at(rk, 63).mean() > 0.9 and we.tie_at(rk, 255).mean() > 0.8
    for k in (128, 191, 192, 255, 256, 257, 320, 448, 511):
        assert we.tie_at(rk, k).mean() > 0.8, k
    distinct = np.array([len(np.unique(r)) for r in rk[1][:, :512]])
    assert distinct.max() < 128                                     # runs of equal keys, four entries long at the very least
    assert (np.diff(rk[1][:, :512], axis=1) == 0).mean() > 0.9      # ... nine of ten adjacent entries are an exact tie


def test_twin_rows_are_decided_by_index_alone(ranking):
    pts, rk = ranking("twins")
    copies = we.twin_rows(pts)
    assert len(copies) == 600
    assert (rk[1][copies] == 0).all()                               # more than 512 entries at d2 = 0
    assert np.array_equal(rk[0][copies], np.tile(copies[:we.WIDTH], (600, 1)))
    idx, dist, _ = we.rows(pts, 511, ranking=rk)
    # element 0 is the smallest-index copy, for every copy: the first copy's own row starts behind itself, every other
    # copy's row does NOT hold the first copy and DOES hold the point itself if it is among the next 511
    assert np.array_equal(idx[copies[0]], copies[1:512]) and np.array_equal(idx[copies[5]], copies[1:512])
    assert copies[5] in idx[copies[5]] and (dist[copies] == 0).all()


def test_a_sparse_point_of_the_clump_cloud_reaches_across_the_cloud(ranking):
    """The four outliers and the sparse points need the dense ball to fill 511 entries: their 511th neighbour is farther
    than 10 times the median spacing of the sparse part."""
    pts, rk = ranking("clump")
    far = np.flatnonzero(np.abs(pts).max(1) > 50)
    assert len(far) == 4
    kth = np.sqrt(rk[1][:, 511])
    assert kth[far].min() > 60 and np.median(kth) < 0.05


def test_queries_restate_the_tree_query(ranking):
    """``queries=``: nothing dropped, float64 distances, k > n padded with n / inf, the bound strict -- SciPy's
    ``query`` bit for bit in distances, and in indices where no tie decides."""
    from scipy.spatial import cKDTree
    pts, _ = ranking("lattice")
    q = we.lattice_queries()
    tree = cKDTree(pts)
    for k in (1, 64, 128):
        idx, dist, count = we.rows(pts, k, queries=q)
        d, i = tree.query(q, k)
        assert dist.dtype == np.float64 and np.array_equal(dist, d.reshape(len(q), k)) and (count == k).all()
    idx, dist, count = we.rows(pts, 128, eps=0.25, queries=q)
    d, i = tree.query(q, 128, distance_upper_bound=0.25)
    assert np.array_equal(dist, d) and np.array_equal(count, (i < len(pts)).sum(1)) and count.min() == 0 and (count == 128).any()
    assert ((count > 0) & (count < 128)).any()
    small = pts[:63]
    idx, dist, count = we.rows(small, 65, queries=q[:5])
    d, i = cKDTree(small).query(q[:5], 65)
    assert np.array_equal(dist, d) and (idx[:, 63:] == 63).all() and (count == 63).all()
    tie_free = we.torus()
    tq = tie_free[:30].astype(np.float64) + 1e-3
    idx, dist, _ = we.rows(tie_free, 100, queries=tq)
    d, i = cKDTree(tie_free).query(tq, 100)
    assert np.array_equal(dist, d) and np.array_equal(idx, i)

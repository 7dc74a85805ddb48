"""The argument behind the exact sweep's starting bound (csrc/pct_knn_sweep.h, Sweep::seed), as a NumPy property test.

A redo row holds k claimed neighbours of its query.  If they are k distinct points of the cloud, none of them the query's
own record, then they and that record are k+1 distinct points, and the largest of their squared distances B cannot be
smaller than the (k+1)-th smallest squared distance over the whole cloud -- whichever k points they are, in whatever
order.  A sweep that starts with the bound B and lets a candidate pass when d2 < B or d2 == B therefore meets every one of
the true k+1 nearest, and the list it keeps -- the k+1 smallest by (d2, index) -- is the list of the sweep that starts at
+inf.  With a strict test at the seed (d2 < B only) the farthest of them is lost whenever B is tight, which the last
test shows on a lattice of exact ties."""
import numpy as np
import pytest


def d2_from(pts, q):
    """fp64 ((dx^2 + dy^2) + dz^2) from the float32 records: the sweep's arithmetic."""
    d = pts.astype(np.float64) - pts[q].astype(np.float64)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def nearest(d2, k1, keep=None):
    """The k1 smallest by (d2, index) among the candidates `keep` lets through."""
    idx = np.arange(len(d2)) if keep is None else np.flatnonzero(keep)
    order = np.lexsort((idx, d2[idx]))
    return idx[order[:k1]]


def clouds():
    rng = np.random.default_rng(11)
    out = {"random": rng.normal(size=(400, 3)).astype(np.float32)}
    dup = rng.normal(size=(300, 3)).astype(np.float32)
    dup[:120] = dup[7]                                     # 120 copies of one point
    dup[200:230] = dup[250]
    out["duplicates"] = dup
    g = np.stack(np.meshgrid(*[np.arange(7.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    out["lattice"] = g.astype(np.float32)                  # shells of exactly equal distances
    out["tiny"] = rng.normal(size=(7, 3)).astype(np.float32)
    return out


CLOUDS = clouds()


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_any_k_distinct_points_bound_the_kth_distance(name):
    pts = CLOUDS[name]
    n = len(pts)
    rng = np.random.default_rng(5)
    for k in (1, 5, min(50, n - 2), n - 2):
        for _ in range(40):
            q = int(rng.integers(n))
            d2 = d2_from(pts, q)
            true = nearest(d2, k + 1)
            tau = d2[true[-1]]
            others = np.delete(np.arange(n), q)
            picks = [rng.choice(others, k, replace=False),                       # any k of them
                     others[np.argsort(d2[others], kind="stable")[:k]],         # the nearest k: the tightest bound
                     others[np.argsort(d2[others], kind="stable")[:k]][::-1]]   # ... in another order
            for S in picks:
                B = max(d2[S].max(), d2[q])
                assert B >= tau, (name, k, q)
                # the seeded sweep: d2 <= B passes; what it keeps is what the unseeded sweep keeps
                got = nearest(d2, k + 1, keep=d2 <= B)
                assert np.array_equal(got, true), (name, k, q)


def test_a_candidate_at_the_bound_must_pass():
    """Lattice, query in the middle: the six face neighbours are at d2 = 1 exactly.  The row holds five of them (k = 5); the
    bound is 1 and the (k+1)-th nearest -- self first, then the six by index -- is at 1 as well."""
    pts = CLOUDS["lattice"]
    q = int(np.flatnonzero((pts == 3).all(axis=1))[0])
    d2 = d2_from(pts, q)
    k = 5
    S = np.flatnonzero(d2 == 1.0)[1:]                      # five of the six, not the one with the smallest index
    assert len(S) == k
    B = d2[S].max()
    true = nearest(d2, k + 1)
    assert B == d2[true[-1]] == 1.0
    assert np.array_equal(nearest(d2, k + 1, keep=d2 <= B), true)
    strict = nearest(d2, k + 1, keep=d2 < B)
    assert len(strict) < k + 1                             # only the query itself is strictly inside


def test_the_querys_own_record_is_not_one_of_the_k():
    """Why the seed refuses a row that names the query itself: with duplicates the row [self] (k = 1) would give B = 0 while
    the second nearest of a query without a twin is farther."""
    pts = CLOUDS["random"]
    d2 = d2_from(pts, 3)
    tau = d2[nearest(d2, 2)[-1]]
    assert d2[3] == 0.0 and tau > 0.0                      # k distinct points including self bound nothing

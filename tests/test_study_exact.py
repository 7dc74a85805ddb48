"""tests/study_exact.py on the CPU: the restatement against the oracle, the cases of tests/test_gpu_study.py against the
cap, and planted table defects against the two checks.  No GPU, no import of the package.

Measured here (one run; figures in the assertions' messages):
  restatement    400 (sample, n) entries of the golden's torus and 160 of the torus with twins: K equals the oracle's
                 inner K(n) (tree query, plane_align, quadric_fit, quadric_curvatures) bit for bit; the bisection of the
                 table equals oracle.neighbor_study's counts on all 64 samples at three tolerances
  spread         0 on every entry of every torus case (3 ... 511 neighbours); up to 1.1e-12 on the lattice
  left out       kinds 0 / 0 / 2 of 64; wide 0 of 6; pairs 0 of 16; golden float32 0 / 0 / 0 of 48, float64 see
                 tests/test_oracle_goldens.py
  flat rows      the reference's noise is at most 9.1e-9 of special_bar's bound, the bound at most 5.2e-15
  planted        each of the five table defects fails the value check on 16 samples x 39 counts (worst entry 7e5 ... 7e6
                 bars) AND changes the converged count of comparable samples (two samples for the swap, six or more otherwise)
"""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import pct_oracle as oracle
import study_exact as se
import wide_exact as we


def _inner_K(points, tree, i, n):
    """oracle.neighbor_study's k_gauss (pct:756-770)."""
    nb = points[tree.query(points[i], n + 1)[1]]
    try:
        cf = oracle.quadric_fit(oracle.plane_align(nb - points[i]))
    except Exception:
        cf = (0, 0, 0, 0, 0, 0)
    return np.float32(oracle.quadric_curvatures(cf)[0])


@pytest.mark.parametrize("cloud", ("torus32", "torus64", "pairs"))
def test_the_restatement_is_the_oracles_inner_K(cloud):
    """Tie-free clouds: the tree's n + 1 nearest ARE [i] + the first n of the ranking, in this order.  With twins the tree
    may return the twin before the sample; the coordinates, and therefore the bits, are the same."""
    if cloud == "pairs":
        pts, later = se.torus_pairs()
        rows = later[:8]
        assert len(later) >= 16 and (we.ranked(pts, rows, width=2)[0][:, 0] < rows).all()       # the twin comes first
    else:
        pts = se.torus32() if cloud == "torus32" else se.torus64()
        rows = np.random.default_rng(3).integers(0, len(pts), 20)
    ns = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 31, 32, 50, 63, 64, 65, 99, 100, 101])
    K = se.table(pts, rows, 1, 101)
    tree = cKDTree(np.array(pts, dtype=np.float32))
    with np.errstate(invalid="ignore"):
        want = np.array([[_inner_K(pts, tree, i, n) for n in ns] for i in rows], np.float32)
    cols = ns - 1
    solid = ns >= 2                                      # two points: the normal is LAPACK's pick, K is 0 either way
    assert K.dtype == np.float32
    assert np.array_equal(K[:, cols][:, solid].view(np.uint32), want[:, solid].view(np.uint32))
    assert np.isfinite(K).all()


def test_the_bisection_is_the_oracles():
    pts = se.torus32()
    rows = np.random.default_rng(4).integers(0, 3000, 64)
    rows[40:44] = rows[[3, 3, 17, 0]]
    assert len(np.unique(rows)) < 64                     # repeated samples, as np.random.randint draws them
    K = se.table(pts, rows, 3, 100)
    for tol, lo, hi in se.GOLDEN_CASES:
        res, conv = oracle.neighbor_study(pts, rows, tol, lo, hi)
        got, seen = se.counts(K, tol, lo, hi, 3)
        assert np.array_equal(got, conv) and se.result(got) == res, (tol, lo, hi)
        assert all(lo <= mid <= hi and d.dtype == np.float32 for dec in seen for mid, d in dec)
    # no candidate found: the count is the upper bound of the LAST interval (pct:787-788), below the lower bound if need be
    assert se.bisect(np.arange(9, dtype=np.float32), 0.5, 3, 9)[0] == 9
    assert se.bisect(np.zeros(8, np.float32), 0.5, 3, 9)[0] == 3
    assert se.bisect(np.array([0, 1], np.float32), 0.5, 5, 5)[0] == 5 and se.bisect(np.array([0, 0], np.float32), 0.5, 5, 5)[0] == 5
    # tol is compared in float32 (NumPy's weak Python scalar): a difference equal to float32(tol) is NOT below it
    t32 = np.float32(0.03)
    assert float(t32) < 0.03 and se.bisect(np.array([0, t32], np.float32), 0.03, 1, 1)[1][0][1] == t32
    assert se.bisect(np.array([0, t32, 7], np.float32), 0.03, 1, 1) == (1, [(1, t32)])          # not converged: upper stays


@pytest.mark.parametrize("name", sorted(se.CASES))
def test_every_case_stays_under_the_cap_for_the_reference_alone(name):
    """The cap is a property of (cloud, samples, tol, bounds), decided by the reference and its bars alone."""
    with np.errstate(invalid="ignore"):
        st, decisions = se.case(name, full=False)
    assert np.isfinite(st.K).all()
    for tol, lo, hi in decisions:
        c, comparable, _ = st.decide(tol, lo, hi)
        print(f"{name} tol {tol} [{lo}, {hi}]: counts {c.min()} ... {c.max()}, {len(set(c.tolist()))} distinct, "
              f"left out {(~comparable).sum()} of {len(c)}, largest measured spread {np.nanmax(st.spread):.2e}")
        assert se.under_cap(comparable), (name, tol, lo, hi, np.flatnonzero(~comparable))
        assert len(set(c[comparable].tolist())) >= min(5, len(c) - 1), "the bisection decides nothing on this case"
    ordinary = np.isnan(st.special)
    if name in ("kinds", "wide", "pairs"):
        # a torus: a row is special only where it is three distinct points
        three = np.arange(st.n_lo, st.n_hi + 1)[None, :] + 1 - (name == "pairs") == 3
        assert np.array_equal(~ordinary, np.broadcast_to(three, ordinary.shape)) and not st.zero.any()
    if name == "twins":
        assert st.zero[:4].all() and not st.zero[4:].any() and np.isinf(st.special[:4]).all() and (st.K[st.zero] == 0).all()
    if name == "lattice":
        ranking = we.ranked(st.points, st.samples, width=st.n_hi + 2)
        ties = np.array([we.tie_at(ranking, n) for n in range(st.n_lo, st.n_hi + 1)]).T      # entry n ties with entry n + 1
        print(f"lattice: {ties.mean():.2f} of the prefixes are cut inside a run of equal distances")
        assert ties.mean() > 0.8 and ties.any(0).all()


def test_flat_rows_the_references_noise_is_below_the_bound():
    pts = se.torus32()
    rows = np.arange(0, 3000, 23)
    st = se.Study(pts, rows, 1, 3, full=False)
    assert np.isinf(st.special[:, 0]).all() and np.isfinite(st.special[:, 1]).all() and np.isnan(st.special[:, 2]).all()
    frac = np.abs(st.K[:, 1]) / st.special[:, 1]
    print(f"three points: |K| of the reference up to {np.abs(st.K[:, 1]).max():.2e}, {frac.max():.2e} of the bound; "
          f"bounds {st.special[:, 1].min():.1e} ... {st.special[:, 1].max():.1e}")
    assert frac.max() < 1.0 / 16
    assert st.special[:, 1].max() < 1e-9                 # ... and the bound stays far below any tolerance of a study
    bar = se.bars(st.K, np.zeros(st.K.shape), 1, st.special)
    assert np.isinf(bar[:, 0]).all() and np.array_equal(bar[:, 1], np.maximum(st.special[:, 1], bar[:, 1]))
    k3 = np.abs(st.K[:, 2].astype(np.float64))
    assert np.array_equal(bar[:, 2], 1e-5 * np.maximum(k3, 1e-2 * k3.max()))                   # the contract, nothing else


# ---------------------------------------------------------------------------------------------------- planted defects
@pytest.fixture(scope="module")
def small():
    pts = se.torus32()
    rows = np.random.default_rng(8).choice(3000, 16, replace=False)
    st = se.Study(pts, rows, 3, 41)
    nbr = se.neighbour_rows(pts, rows, 43)
    return pts, rows, st, nbr


def _table_of(pts, rows, nbr, make_row, query=None):
    K = np.empty((len(rows), 39), np.float32)
    q = rows if query is None else query
    for j, n in enumerate(range(3, 42)):
        K[:, j] = oracle.curvature_loop(pts, np.array([make_row(s, n) for s in range(len(rows))]), q)[1]
    return K


PLANTS = ("prefix shifted by one neighbour", "count n instead of n + 1", "columns shifted by one",
          "query replaced by its nearest neighbour", "two samples' rows swapped")


@pytest.mark.parametrize("plant", PLANTS)
def test_planted_table_defects_are_caught(small, plant):
    pts, rows, st, nbr = small
    tol, lo, hi = 0.03, 3, 40
    if plant == PLANTS[0]:
        K = _table_of(pts, rows, nbr, lambda s, n: np.concatenate([[rows[s]], nbr[s, 1:n + 1]]))
    elif plant == PLANTS[1]:
        K = _table_of(pts, rows, nbr, lambda s, n: np.concatenate([[rows[s]], nbr[s, :n - 1]]))
    elif plant == PLANTS[2]:
        K = np.concatenate([st.K[:, 1:], se.table(pts, rows, 42, 42)], 1)
    elif plant == PLANTS[3]:
        K = _table_of(pts, rows, nbr, lambda s, n: np.concatenate([[nbr[s, 0]], nbr[s, :n]]), query=nbr[:, 0])
    else:
        K = st.K.copy()
        K[[2, 9]] = K[[9, 2]]
    clean = st.compare(st.K.copy(), tol, lo, hi)
    assert clean["ok"] and clean["worst"] == 0.0 and clean["left_out"] <= se.CAP
    found = st.compare(K, tol, lo, hi)
    print(f"{plant}: values {'miss' if not found['values_ok'] else 'pass'} (worst {found['worst']:.3g} bars, {len(found['bad'])}+ entries), "
          f"counts {'differ on samples ' + str(found['wrong']) if not found['counts_ok'] else 'agree'}")
    assert not found["values_ok"] and found["worst"] > 100.0
    assert not found["ok"]
    assert not found["counts_ok"], "the decision check alone would have let this through"

"""SciPy's ``query_ball_point`` equals the brute-force statement of tests/ball_exact.py on every case the device tests
(tests/test_gpu_ball.py) compare against it, and the cases hold what those tests rely on: masses of entries exactly at
the radius, empty rows, rows longer than every sort path, and a ladder of row lengths around every threshold of the
kernels (64 lanes, the 1 024-entry cap of the LDS sort)."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import ball_exact as be
import wide_exact as we


@pytest.fixture(scope="module")
def table():
    out = {}
    for name, (pts, q, r) in be.cases(we).items():
        ref = be.rows(pts, q, r)
        out[name] = (pts, q, r, ref)
    return out


def _scipy_rows(pts, q, r):
    got = cKDTree(np.asarray(pts).astype(np.float32)).query_ball_point(q, r, return_sorted=True)
    counts = np.array([len(x) for x in got], np.int64)
    offsets = np.zeros(len(q) + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    return offsets, np.fromiter((i for x in got for i in x), np.int32, int(counts.sum()))


def test_scipy_equals_the_statement_on_every_case(table):
    for name, (pts, q, r, ref) in table.items():
        offsets, idx = _scipy_rows(pts, q, r)
        assert np.array_equal(offsets, ref[0]) and np.array_equal(idx, ref[1]), name


def test_negative_radius_is_its_absolute_value():
    pts = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], np.float32)
    assert cKDTree(pts).query_ball_point([0, 0, 0], -1.0, return_sorted=True) == [0, 1]
    assert be.rows(pts, [[0, 0, 0]], -1.0)[1].tolist() == [0, 1]
    assert be.rows(pts, [[0, 0, 0]], np.nan)[0].tolist() == [0, 0] and be.rows(pts, [[0, 0, 0]], np.inf)[0].tolist() == [0, 3]


def test_lattice_holds_masses_of_entries_exactly_at_the_radius(table):
    want = (15288, 14112, 11760, 47544, 38208, 7056, 0)
    for r, n_at in zip(be.LATTICE_OWN_RADII, want):
        pts, q, _, ref = table[f"lattice own r={r}"]
        assert len(q) == 2744 and be.at_radius(ref, r, len(q)) == n_at, r
    assert np.diff(table["lattice own r=2.0"][3][0]).max() == 2744      # the whole cloud in a row


def test_lattice_queries_have_empty_rows_and_entries_at_the_radius(table):
    """Entries exactly at r: 100 ... 744 at the radii within the lattice, none at r = 3 (which takes the whole lattice
    for every query near it); the 12 far queries reach nothing at any of them.  The per-query draw (seed 1501) uses
    every radius of its set and leaves 15 rows empty."""
    for r, n_at in zip(be.LATTICE_QUERY_RADII, (220, 181, 744, 100, 0)):
        pts, q, _, ref = table[f"lattice queries r={r}"]
        assert len(q) == 92
        assert be.at_radius(ref, r, len(q)) == n_at, r
        assert int((np.diff(ref[0]) == 0).sum()) == 12, r
    pts, q, r, ref = table["lattice queries per-query r"]
    assert set(r) == set(be.PER_QUERY_CHOICES)
    assert be.at_radius(ref, r, len(q)) == 226 and int((np.diff(ref[0]) == 0).sum()) == 15


def test_one_point_exactly_at_the_radius_from_outside_the_box():
    ref = be.rows(we.lattice(), [[5.0, 0.25, 0.25]], 4.1875)
    assert ref[0].tolist() == [0, 1] and ref[2][0] == 4.1875 ** 2


def test_twins_and_clump_rows(table):
    pts, q, _, ref = table["twins own r=0.0"]
    assert len(q) == 2400 and be.at_radius(ref, 0.0, len(q)) == 361800 and np.diff(ref[0]).max() == 600
    pts, q, _, ref = table["twins own r=0.1"]
    assert be.at_radius(ref, 0.1, len(q)) == 0 and np.diff(ref[0]).max() >= 600
    for r, longest in zip(be.CLUMP_RADII, (59, 2330, 2526, 2801)):
        pts, q, _, ref = table[f"clump own r={r}"]
        assert len(q) == 2804 and np.diff(ref[0]).max() == longest and be.at_radius(ref, r, len(q)) == 0, r


def test_other_cases_have_no_entry_at_the_radius(table):
    for name, m in (("flat own r=0.05", 3000), ("line own r=0.05", 2000), ("f64 native r=0.02", 3000), ("torus own r=0.05", 6000),
                    ("torus own r=0.1", 6000)):
        pts, q, r, ref = table[name]
        assert len(q) == m and be.at_radius(ref, r, m) == 0, name
    assert table["f64 native r=0.02"][1].dtype == np.float64 and not np.array_equal(table["f64 native r=0.02"][1], table["f64 native r=0.02"][0].astype(np.float32))


@pytest.mark.parametrize("exact_radius", (False, True))
def test_ladder_reaches_every_length(exact_radius):
    pts, q, r = be.ladder(we, exact_radius)
    ref = be.rows(pts, q, r)
    lengths = np.diff(ref[0]).reshape(be.LADDER_ROWS, len(be.LADDER))
    if not exact_radius:
        assert (lengths == np.array(be.LADDER)).all()          # the torus is tie-free over these rows: every target is met
    have = set(lengths.ravel().tolist())
    need = set(range(0, 131)) | {255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049} | {be.SORT_CAP - 1, be.SORT_CAP, be.SORT_CAP + 1}
    assert need <= have, sorted(need - have)
    offsets, idx = _scipy_rows(pts, q, r)
    assert np.array_equal(offsets, ref[0]) and np.array_equal(idx, ref[1])

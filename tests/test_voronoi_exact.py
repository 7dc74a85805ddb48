"""The CPU restatement of the tangent-plane Voronoi areas (tests/voronoi_exact.py): pinned against SciPy's Voronoi diagram
and closed forms, its bar re-measured, the table of DESIGN 4.3h reproduced.  No GPU, no import of the package."""
import functools
import math

import numpy as np
import pytest

import pct_oracle as oracle
import voronoi_exact as ve


@functools.lru_cache(maxsize=None)
def case(name):
    """(points, idx, count, reference with detail) of one case, on the oracle's rows; computed once per session."""
    make, k, eps = ve.CASES[name]
    pts = make()
    idx, count = (ve.knn_rows(pts, k), None) if eps is None else ve.knn_rows(pts, k, eps)
    return pts, idx, count, ve.reference(pts, idx, count, detail=True)


# ---- the restatement is the Voronoi cell --------------------------------------------------------------------------------
def test_flat_cloud_equals_scipy_voronoi():
    from scipy.spatial import Voronoi
    pts = ve.flat_cloud(400)
    idx = ve.knn_rows(pts, 12)
    ref = ve.reference(pts, idx)
    xy = pts[:, :2].astype(np.float64)
    vor = Voronoi(xy)
    closed = np.flatnonzero(ref["closed"])
    assert len(closed) > 300
    # A row sees 12 neighbours, the diagram all 400 points.  "Closed" keeps the vertices inside the farthest neighbour's
    # distance L, and a point outside the row has its bisector at L / 2 or beyond: near the rim of the cloud, where cells
    # are long, such a point can still cut.  Whether one does is decided here from the row's own polygon; the rows no
    # outside point reaches must be SciPy's regions to 1e-12, the others must be strictly larger than them.
    worst, reached = 0.0, 0
    for i in closed:
        block = pts[idx[i]] - pts[i]
        ab = ve.frame_oracle(block)
        assert np.array_equal(ab, block[:, :2].astype(np.float64))            # a flat cloud at z = 0: the frame is the identity
        q = block.astype(np.float64)
        c = ve.cell(ab, float(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]).max()))
        assert c["area"] == ref["area"][i]
        V = np.stack([c["X"], c["Y"]], 1)
        others = np.setdiff1d(np.arange(len(pts)), np.append(idx[i], i))
        d = xy[others] - xy[i]
        cuts = ((V @ d.T).max(0) - 0.5 * (d * d).sum(1) > 0).any()
        region = vor.regions[vor.point_region[i]]
        assert -1 not in region and len(region) >= 3, f"row {i} is closed but SciPy's region is unbounded"
        v = vor.vertices[region] - xy[i]
        v = v[np.argsort(np.arctan2(v[:, 1], v[:, 0]))]
        x, y = v[:, 0], v[:, 1]
        area = 0.5 * abs(float(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1))))
        if cuts:
            reached += 1
            assert ref["area"][i] > area * (1 + 1e-12), i
            continue
        worst = max(worst, abs(ref["area"][i] - area) / area)
        assert ref["nverts"][i] == len(region), i
    print(f"flat cloud: {len(closed)} closed rows, {reached} reached by a point outside their row; the others differ from "
          f"scipy.spatial.Voronoi by at most {worst:.2e} relative")
    assert worst <= 1e-12 and len(closed) - reached >= 250


def test_lattice_interior_cells_are_unit_squares():
    _, _, _, ref = case("lattice-k8")
    inner = ve.lattice_interior()
    assert inner.sum() == 25 and ref["closed"][inner].all() and not ref["closed"][~inner].any()
    assert np.abs(ref["area"][inner] - 1.0).max() <= 1e-14


def test_ring_cell_is_the_40_gon():
    _, _, _, ref = case("ring-k80")
    assert ref["nverts"][0] == ve.RING_M and ref["closed"][0] == 1
    assert abs(ref["area"][0] - ve.RING_AREA) <= 1e-7          # float32 coordinates
    assert abs(ref["area"][0] - 0.78701708) <= 0.5e-8


def test_degenerate_rows_are_nan():
    pts, _, _, _ = case("sphere-k8")
    idx = np.zeros((3, 4), np.int32)
    idx[2] = [5, 6, 7, 8]
    ref = ve.reference(pts, idx, np.array([0, 1, 4]), rows=np.array([1, 2, 3]))
    assert np.isnan(ref["area"][:2]).all() and not ref["closed"][:2].any() and not ref["nverts"][:2].any()
    assert ref["area"][2] > 0
    pts = pts.copy()
    pts[5, 0] = np.inf                                           # a frame that is not finite
    assert np.isnan(ve.reference(pts, idx[2:], rows=np.array([3]))["area"][0])


def test_twin_neighbours_cut_nothing():
    """rho^2 == 0 is skipped: a point and its twin keep the same full cell."""
    pts, idx, _, ref = case("doubled-k16")
    half = len(pts) // 2
    assert np.array_equal(pts[:half], pts[half:])
    assert np.allclose(ref["area"][:half], ref["area"][half:], rtol=1e-9, atol=0)
    assert ref["closed"].all()
    s = ve.fibonacci_sphere(1000)
    single = ve.reference(s, ve.knn_rows(s, 8))
    assert abs(ref["area"].sum() - 2.0 * single["area"].sum()) <= 1e-3 * single["area"].sum()


# ---- the bar, measured again on every run --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ve.CASES))
def test_area_bar_is_four_times_the_need(name):
    pts, idx, count, ref = case(name)
    stride = 1 if len(pts) <= 100 else 4
    need_c, need_o, left, _ = ve.measure_need(pts, idx, count, ref=ref, stride=stride)
    live = int((~np.isnan(ref["area"])).sum())
    print(f"{name}: need {need_c:.2f} closed, {need_o:.2f} open (every {stride}th row); {left} of {live} rows left out; bar {ve.C_AREA:g}")
    assert max(need_c, need_o) <= ve.C_AREA / 4
    assert ve.C_AREA == 4 * ve.C_AREA_NEEDED
    if name in ve.NOTHING_LEFT_OUT:
        assert left == 0
    else:
        assert left <= ve.LEFT_OUT_CAP * len(pts)
    # the reference against itself passes its own comparison, whatever it leaves undecided
    c = ve.compare(ref["area"], ref["closed"], ref["nverts"], ref)
    assert not (c["bad_area"].any() or c["bad_closed"].any() or c["bad_nverts"].any() or c["nan_differs"].any())
    if name not in ve.CONCURRENT:
        assert c["undecided"].sum() <= ve.LEFT_OUT_CAP * len(pts)


def test_hybrid_case_has_rows_of_every_length():
    _, _, count, ref = case("hybrid-k8")
    hist = np.bincount(count, minlength=ve.HYBRID_K + 1)
    print("eps-hybrid rows by count:", hist.tolist())
    assert hist[0] > 0 and hist[1] > 0 and (hist[2:] > 0).all()
    assert np.array_equal(np.isnan(ref["area"]), count < 2)


def test_bar_has_teeth():
    """A normal off by 1e-9 rad -- a million eps -- moves the areas of a curved cloud far past the bar."""
    pts, idx, _, ref = case("torus-k30")
    rows = np.arange(0, len(pts), 40)

    def tilted(block):
        r = oracle.plane_align(block)
        t = 1e-9
        rot = np.array([[1.0, 0.0, t], [0.0, 1.0, 0.0], [-t, 0.0, 1.0]])
        return (r @ rot.T)[:, :2]

    other = ve.reference(pts, idx[rows], rows=rows, frame=tilted)
    sub = {k: v[rows] for k, v in ref.items()}
    c = ve.compare(other["area"], other["closed"], other["nverts"], sub)
    assert c["need"] > 100 * ve.C_AREA and c["bad_area"].sum() > 0.5 * len(rows)


# ---- energies: the table of the issue, and the closed forms ----------------------------------------------------------------
def table_row(name, mask_closed=False):
    pts, idx, count, ref = case(name)
    _, K, H, _ = oracle.curvature_batched(pts, idx)
    (bend, stretch, area, used), _ = ve.energies(ref["area"], K, H, ref["closed"].astype(bool) if mask_closed else None)
    return bend, stretch, area, int((ref["closed"] == 0).sum()), int(ref["nverts"].max())


def digits(x, shown, places):
    return abs(x - shown) <= 0.5 * 10.0 ** -places


def test_energy_table_sphere():
    make, _, _ = ve.CASES["sphere-k8"]
    s = make()
    idx = ve.knn_rows(s, 6)
    ref = ve.reference(s, idx)
    _, K, H, _ = oracle.curvature_batched(s, idx)
    (bend, stretch, area, _), _ = ve.energies(ref["area"], K, H)
    assert digits(area, 12.5423, 4) and digits(bend, 12.633, 3) and digits(stretch, 12.633, 3)
    assert ref["closed"].all() and ref["nverts"].max() == 6
    assert abs(bend - 4 * math.pi) <= 0.02 * 4 * math.pi and abs(stretch - 4 * math.pi) <= 0.02 * 4 * math.pi
    bend, stretch, area, opened, nv = table_row("sphere-k8")
    assert digits(area, 12.5413, 4) and opened == 0 and nv == 7
    bend, stretch, area, opened, nv = table_row("sphere-k30")
    assert digits(area, 12.5412, 4) and digits(bend, 12.958, 3) and digits(stretch, 12.958, 3) and opened == 0 and nv == 7
    assert abs(area - 4 * math.pi) <= 0.005 * 4 * math.pi


def test_energy_table_torus_and_egg_carton():
    bend, stretch, area, opened, nv = table_row("torus-k30")
    assert digits(area, 13.0449, 4) and digits(bend, 34.71, 2) and digits(stretch, 0.216, 3) and opened == 0 and nv == 12
    true_area = 4 * math.pi ** 2 / 3.0                            # (2 pi R)(2 pi r), R = 1, r = 1/3
    assert abs(true_area - 13.1595) < 1e-4 and abs(area - true_area) <= 0.015 * true_area
    assert table_row("torus-k16")[3] == 38
    bend, stretch, area, opened, nv = table_row("egg-k30", mask_closed=True)
    assert digits(area, 4.0003, 4) and opened == 149


def test_energies_restate_the_reference_loop():
    """pct:652-653 as written -- Python's sum over zip, float32 h -- against the exactly rounded sums of ``energies``."""
    pts, idx, _, ref = case("sphere-k8")
    _, K, H, _ = oracle.curvature_batched(pts, idx)
    bending = sum((h ** 2) * area for h, area in zip(H, ref["area"]))
    stretching = sum(k * area for k, area in zip(K, ref["area"]))
    (bend, stretch, _, used), (tb, ts, _) = ve.energies(ref["area"], K, H)
    assert used == len(pts)
    n = len(pts)
    assert abs(bending - bend) <= n * ve.EPS64 * np.abs(tb).sum() and abs(stretching - stretch) <= n * ve.EPS64 * np.abs(ts).sum()

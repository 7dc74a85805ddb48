"""A redo row whose list the fast sweep proved to be the set of its 27 cells is taken over by the exact sweep, which then
starts at the guarantee test of ring 1 instead of walking the first cube again (csrc/pct_knn_sweep.h, Sweep::adopt; the mark:
`trusted` in csrc/pct_knn_pair.hip and csrc/pct_knn_duo.hip; tests/test_redo_adopt_set.py is the argument in NumPy).

Every case runs one cloud four ways -- PCT_KNN_GRID, the same under PCT_REDO_ADOPT=0 (no marks), the same under
PCT_REDO_SEED=0 (no lists left at all) and PCT_KNN_GRID_EXACT (no fast sweep) -- as fused calls, and compares indices,
distances, counts, K and H bit for bit.  Each case asserts from the sweep's statistics the path it names; redone_queries
is printed, not compared (it moves by a row between runs: tests/test_gpu_redo_seed.py)."""
import os

import numpy as np
import pytest

import test_gpu_redo_seed as rs          # the clouds, the fused call and the comparison of the seed's own test

pytestmark = pytest.mark.gpu

PAIR, DUO, Q64_BIT = rs.PAIR, rs.DUO, rs.Q64_BIT
SWITCHES = ("PCT_REDO_SEED", "PCT_REDO_ADOPT")


class switches:
    """the two A/B variables for the length of a block, whatever the caller's environment holds"""

    def __init__(self, **values):
        self.values = values

    def __enter__(self):
        self.saved = {name: os.environ.pop(name, None) for name in SWITCHES}
        for name, v in self.values.items():
            os.environ[name] = v

    def __exit__(self, *exc):
        for name in SWITCHES:
            os.environ.pop(name, None)
            if self.saved[name] is not None:
                os.environ[name] = self.saved[name]


def one(capi, pts, k, eps, algo, rows=None, **env):
    with switches(**env):
        h = capi.Handle(0)
        try:
            h.set_stats(True)
            return rs.fused(capi, h, pts, k, eps, algo, rows)
        finally:
            h.close()


def four_ways(capi, pts, k, eps=0.0, rows=None, what=""):
    got, t = one(capi, pts, k, eps, capi.KNN_GRID, rows)
    plain, t_plain = one(capi, pts, k, eps, capi.KNN_GRID, rows, PCT_REDO_ADOPT="0")
    bare, t_bare = one(capi, pts, k, eps, capi.KNN_GRID, rows, PCT_REDO_SEED="0")
    ref, t_ref = one(capi, pts, k, eps, capi.KNN_GRID_EXACT, rows)
    print(what, {f: t[f] for f in ("sweep_variant", "redone_queries", "redo_adopted", "ring_fallbacks", "lds_overflows", "grid_points")},
          "| redone with PCT_REDO_ADOPT=0", t_plain["redone_queries"], "with PCT_REDO_SEED=0", t_bare["redone_queries"])
    rs.same(got, ref, what + " against the exact sweep alone")
    rs.same(got, plain, what + " against PCT_REDO_ADOPT=0")
    rs.same(got, bare, what + " against PCT_REDO_SEED=0")
    # an adopted row ends in the ring the walked one ends in, and only the adopting run adopts
    for other in (t_plain, t_bare):
        for f in ("lds_overflows", "ring_fallbacks"):
            assert t[f] == other[f], (what, f, t[f], other[f])
    assert t_plain["redo_adopted"] == 0 and t_bare["redo_adopted"] == 0 and t_ref["redo_adopted"] == 0
    assert 0 <= t["redo_adopted"] <= t["redone_queries"]
    return got, t


@pytest.fixture(scope="module")
def seam(gpu):
    return rs.two_density_torus(gpu["shapes"], 12_000, seed=3)


def test_seam_through_the_pair_kernel(gpu, seam):
    _, t = four_ways(gpu["capi"], seam, 50, what="seam k=50")
    assert t["sweep_variant"] & 3 == PAIR
    assert 1 <= t["redo_adopted"] <= t["ring_fallbacks"]


@pytest.mark.parametrize("k", [80, 100])
def test_seam_through_the_duo_kernel(gpu, seam, k):
    _, t = four_ways(gpu["capi"], seam, k, what=f"seam k={k}")
    assert t["sweep_variant"] & 3 == DUO
    assert 1 <= t["redo_adopted"] <= t["ring_fallbacks"]


def test_overflowing_item_is_not_adopted(gpu):
    """700 points in one cell: the items of that cell run on the first 512 staged slots, their lists are the set of no
    stencil.  All 700 rows are redone and none of them is adopted: what is adopted lies among the other redone rows."""
    capi = gpu["capi"]
    pts = rs.coincident(gpu["shapes"])
    _, t = four_ways(capi, pts, 50, what="overflow")
    assert t["sweep_variant"] & 3 == PAIR and t["lds_overflows"] >= 1 and t["redone_queries"] >= 700
    assert t["redo_adopted"] <= t["redone_queries"] - 700


def test_eps_rows_with_padding_are_not_adopted(gpu, seam):
    """eps just above one cell edge (tests/test_gpu_redo_seed.py): rows whose eps ball holds fewer than k+1 points are redone
    with -1 in their tail.  A row with padding has no (k+1)-th entry and is never marked: what is adopted lies among the
    full rows."""
    capi = gpu["capi"]
    _, t0 = one(capi, seam, 50, 0.0, capi.KNN_GRID)
    eps = 1.05 * t0["cell_size"]
    (_, _, cnt, _, _), t = four_ways(capi, seam, 50, eps=eps, what=f"seam eps={eps:.4f}")
    full = int((cnt == 50).sum())
    print("rows with padding", int((cnt < 50).sum()), "full rows", full)
    assert t["redone_queries"] >= 1 and (cnt < 50).any() and full >= 1
    assert t["redo_adopted"] <= full


def test_boundary_ties_on_a_lattice(gpu):
    """shapes.torus_grid(110): every point has symmetric partners at equal distances, so the k-th and the (k+1)-th
    neighbour tie for many rows -- the case in which an adopted list with the wrong one of the two would show."""
    capi, k = gpu["capi"], 50
    pts = gpu["shapes"].torus_grid(110)
    (idx, dist, _, _, _), t = four_ways(capi, pts, k, what="lattice 110")
    # the tie, from the distances all four ways agree on: the (k+1)-th neighbour as brute force over the float32 records
    # gives it, against the row's last column (every eighth row: the lattice repeats itself)
    p = pts.astype(np.float64)
    rows = np.arange(0, len(p), 8)
    d = p[rows, None, :] - p[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    part = np.partition(d2, (k, k + 1), axis=1)
    assert np.array_equal(np.sqrt(part[:, k]).astype(np.float32), dist[rows, k - 1])
    # a tie as the fast sweep sees it: equal keys, floor(d2 2^26 / (2.3 cell^2)) (csrc/pct_knn_item.h); equal distances are
    # equal keys, and the float32 rounding of the lattice leaves many partners a few ulp apart
    scale = 2.0 ** 26 / (2.3 * t["cell_size"] ** 2)
    ties = int((np.floor(part[:, k] * scale) == np.floor(part[:, k + 1] * scale)).sum())
    print("rows whose k-th and (k+1)-th neighbour share a key:", ties, "a distance:", int((part[:, k] == part[:, k + 1]).sum()), "of", len(rows))
    assert ties >= 1


@pytest.mark.parametrize("k", [50, 49])
def test_duplicates(gpu, seam, k):
    """Every point stored twice: the list of a query is pairs of twins with equal keys, itself and its own twin first.
    k = 50: entries 50 and 51 are twins -- a tie at the boundary, no row is marked.  k = 49: entries 48 and 49 are twins
    and entry 50 belongs to the next pair, so the rows the cube cannot vouch for are marked; the staging order decides who
    leads a list, so of a query and its twin one finds its own record in column 0 and Sweep::adopt's validation (seed()'s)
    refuses it: a row counts as adopted only behind that validation, and some marked rows must fail it."""
    capi = gpu["capi"]
    pts = np.ascontiguousarray(np.concatenate([seam[:6000], seam[:6000]])[np.random.default_rng(5).permutation(12_000)])
    _, t = four_ways(capi, pts, k, what=f"doubled k={k}")
    assert t["sweep_variant"] & 3 == PAIR and t["ring_fallbacks"] >= 2
    if k == 50:
        assert t["redo_adopted"] == 0
    else:
        assert 1 <= t["redo_adopted"] < t["ring_fallbacks"]


def test_float64_cloud(gpu, seam):
    _, t = four_ways(gpu["capi"], seam.astype(np.float64) * (1.0 + 1e-9), 50, what="seam float64")
    assert t["sweep_variant"] & 3 == PAIR and t["sweep_variant"] & Q64_BIT and t["redone_queries"] >= 1


def test_index_range_whose_grid_left_points_out(gpu, seam):
    pts = np.ascontiguousarray(seam[np.argsort(seam[:, 0], kind="stable")])      # the owned quarter is one end of the cloud
    _, t = four_ways(gpu["capi"], pts, 50, rows=(0, len(pts) // 4), what="owned quarter")
    assert t["grid_points"] < len(pts) and t["redone_queries"] >= 1


@pytest.mark.parametrize("async_mode", [False, True], ids=["blocking", "async"])
def test_one_handle_cloud_after_cloud(gpu, async_mode):
    """One handle alternating two clouds and k = 50 / 30: the table's rows hold an earlier call's lists when a sweep starts,
    and a mark must never meet a list it was not given for."""
    capi, shapes = gpu["capi"], gpu["shapes"]
    a, b = rs.two_density_torus(shapes, 12_000, seed=3), rs.two_density_torus(shapes, 12_000, seed=4)
    want = {}
    for name, pts, k in (("a50", a, 50), ("b50", b, 50), ("b30", b, 30)):
        want[name] = [one(capi, pts, k, 0.0, capi.KNN_GRID_EXACT)[0], one(capi, pts, k, 0.0, capi.KNN_GRID, PCT_REDO_ADOPT="0")[0],
                      one(capi, pts, k, 0.0, capi.KNN_GRID, PCT_REDO_SEED="0")[0]]
    steps = [("a50", a, 50), ("b50", b, 50), ("a50", a, 50), ("b30", b, 30), ("a50", a, 50)]
    with switches():
        h = capi.Handle(0)
        try:
            if async_mode:
                h.set_async(True)
            else:
                h.set_stats(True)
            adopted = 0
            for i, (name, pts, k) in enumerate(steps):
                got, t = rs.fused(capi, h, pts, k, 0.0, capi.KNN_GRID, wait=async_mode)
                for other, how in zip(want[name], ("the exact sweep alone", "PCT_REDO_ADOPT=0", "PCT_REDO_SEED=0")):
                    rs.same(got, other, f"step {i} {name} async={async_mode} against {how}")
                adopted += t["redo_adopted"]
            print("adopted over the five steps:", adopted)
            if not async_mode:
                assert adopted >= 1
        finally:
            h.close()


@pytest.mark.parametrize("make,n,k", [(rs.uneven_line, 52, 50), (rs.tight_pairs, 7, 5)], ids=["n=k+2", "n=7"])
def test_smallest_clouds(gpu, make, n, k):
    four_ways(gpu["capi"], make(n), k, what=f"{make.__name__} n={n} k={k}")

"""The exact sweep behind k_knn_pair / k_knn_duo starts from what the fast sweep found (csrc/pct_knn_sweep.h, Sweep::seed;
overflowing items run on a truncated stencil to have something to leave): the rows it answers are the rows of the sweep
that starts at +inf.

Every case runs one cloud three ways -- PCT_KNN_GRID, PCT_KNN_GRID under PCT_REDO_SEED=0 (no truncated items, no seed read)
and PCT_KNN_GRID_EXACT (no fast sweep, never seeded) -- as fused calls, and compares indices, distances, counts, K and H
bit for bit.  Each case asserts from the sweep's statistics that it sent rows to the exact sweep in the way it names."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAIR, DUO, Q64_BIT = 2, 3, 64          # pct_timings.sweep_variant: the family in the low two bits, bit 6 = float64 queries


def two_density_torus(shapes, n, seed):
    """A torus whose x > 0 half holds four times the points per area of the other: the cell edge suits neither, and the
    rows along the seam fail the 27-cell guarantee."""
    pts = shapes.torus_random(4 * n, seed=seed)
    dense = pts[pts[:, 0] > 0]
    sparse = pts[pts[:, 0] <= 0][::4]
    out = np.concatenate([dense, sparse])[:n]
    return np.ascontiguousarray(out[np.random.default_rng(seed).permutation(len(out))], dtype=np.float32)


def coincident(shapes, spread=0.0):
    """tests/test_gpu_stage_stamps.py's _coincident: 700 copies of the corner of the cloud's box among 4 000 points (the
    first work item overflows the staging area); spread > 0: the 700 scattered over a cube of that edge instead."""
    pts = shapes.torus_random(4000, seed=9)
    pts[:700] = pts.min(axis=0)
    if spread > 0:
        pts[:700] += np.random.default_rng(2).uniform(0, spread, (700, 3)).astype(np.float32)
    return pts


def uneven_line(n):
    """n points at x = 1, 2, 4, 8, ... (wrapping every 20 doublings, shifted in y): no cell edge suits both ends."""
    i = np.arange(n)
    return np.ascontiguousarray(np.stack([2.0 ** (i % 20), 0.37 * (i // 20), 0.0 * i], 1), dtype=np.float32)


class seed_switch:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.saved = os.environ.pop("PCT_REDO_SEED", None)
        if self.value is not None:
            os.environ["PCT_REDO_SEED"] = self.value

    def __exit__(self, *exc):
        os.environ.pop("PCT_REDO_SEED", None)
        if self.saved is not None:
            os.environ["PCT_REDO_SEED"] = self.saved


def fused(capi, h, pts, k, eps, algo, rows=None, wait=False):
    """One fused call on handle h; (idx, dist, cnt, K, H) of the owned rows and the call's record."""
    h.set_points(pts)
    begin, end = rows or (0, len(pts))
    if rows:
        h.set_query_range(begin, end)
    h.curvature(k, eps, algo)
    if wait:
        h.synchronize()
    t = h.timings()
    idx, dist, cnt = h.get_neighbors(begin, end, want_count=eps > 0)
    _, K, H, _ = h.get_fit(begin, end, coefs=False, H2=False)
    return (idx, dist, cnt, K, H), t


def one(capi, pts, k, eps, algo, seed=None, rows=None):
    with seed_switch(seed):
        h = capi.Handle(0)
        try:
            h.set_stats(True)
            return fused(capi, h, pts, k, eps, algo, rows)
        finally:
            h.close()


def same(got, want, what):
    for name, x, y in zip(("idx", "dist", "cnt", "K", "H"), got, want):
        if x is None and y is None:
            continue
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), (what, name, int((x != y).sum()))


def three_ways(capi, pts, k, eps=0.0, rows=None, what=""):
    got, t = one(capi, pts, k, eps, capi.KNN_GRID, rows=rows)
    off, t_off = one(capi, pts, k, eps, capi.KNN_GRID, seed="0", rows=rows)
    ref, _ = one(capi, pts, k, eps, capi.KNN_GRID_EXACT, rows=rows)
    print(what, {f: t[f] for f in ("sweep_variant", "redone_queries", "lds_overflows", "ring_fallbacks", "grid_points")})
    same(got, ref, what + " against the exact sweep alone")
    same(got, off, what + " against PCT_REDO_SEED=0")
    # truncated items and handed-over items count alike, and a seeded row ends in the ring the unseeded one ends in.
    # (redone_queries is printed, not compared: the build places the points of a cell with returning LDS atomics, their
    # order inside the cell decides which queries share a work item and with it a threshold search's starting value,
    # and a row at the edge of its proof can fall either way from run to run: 284 against 283 was seen once.)
    print(what, "redone", t["redone_queries"], "with PCT_REDO_SEED=0", t_off["redone_queries"])
    for f in ("lds_overflows", "ring_fallbacks"):
        assert t[f] == t_off[f], (what, f, t[f], t_off[f])
    return got, t


@pytest.fixture(scope="module")
def seam(gpu):
    return two_density_torus(gpu["shapes"], 12_000, seed=3)


def test_ring_fallbacks_through_the_pair_kernel(gpu, seam):
    _, t = three_ways(gpu["capi"], seam, 50, what="seam k=50")
    assert t["sweep_variant"] & 3 == PAIR and t["ring_fallbacks"] >= 1 and t["redone_queries"] >= t["ring_fallbacks"]


@pytest.mark.parametrize("cells", [0.0, 0.1], ids=["coincident", "tenth_of_a_cell"])
def test_overflowing_item(gpu, cells):
    """700 points in one cell: the item runs on its first 512 staged slots.  Coincident: the bound is 0 and every candidate
    at it ties on the index; spread over a tenth of a cell edge: a bound above 0."""
    capi, shapes = gpu["capi"], gpu["shapes"]
    pts = coincident(shapes)
    if cells > 0:
        _, t0 = one(capi, pts, 50, 0.0, capi.KNN_GRID)
        pts = coincident(shapes, cells * t0["cell_size"])
    _, t = three_ways(capi, pts, 50, what=f"overflow spread={cells} cells")
    assert t["sweep_variant"] & 3 == PAIR and t["lds_overflows"] >= 1 and t["redone_queries"] >= 700


@pytest.mark.parametrize("k", [80, 100])
def test_ring_fallbacks_through_the_duo_kernel(gpu, seam, k):
    _, t = three_ways(gpu["capi"], seam, k, what=f"seam k={k}")
    assert t["sweep_variant"] & 3 == DUO and t["ring_fallbacks"] >= 1 and t["redone_queries"] >= t["ring_fallbacks"]


def test_eps_rows_with_padding_take_no_seed(gpu, seam):
    """eps just above one cell edge: the 27 cells vouch for 1 .. 1.5 edges around a query, so a query near a face of its
    cell whose eps ball holds fewer than k+1 points cannot prove that and is redone -- with -1 in its row's tail."""
    capi = gpu["capi"]
    _, t0 = one(capi, seam, 50, 0.0, capi.KNN_GRID)
    eps = 1.05 * t0["cell_size"]
    (_, _, cnt, _, _), t = three_ways(capi, seam, 50, eps=eps, what=f"seam eps={eps:.4f}")
    print("rows with padding", int((cnt < 50).sum()))
    assert t["redone_queries"] >= 1
    assert (cnt < 50).any() and (cnt == 50).any()


def test_float64_cloud(gpu, seam):
    _, t = three_ways(gpu["capi"], seam.astype(np.float64) * (1.0 + 1e-9), 50, what="seam float64")
    assert t["sweep_variant"] & 3 == PAIR and t["sweep_variant"] & Q64_BIT and t["redone_queries"] >= 1


def tight_pairs(n):
    """Pairs 0.001 apart every 10 units along x: cells of about two points, so a row of five neighbours reaches far
    beyond its 27 cells."""
    i = np.arange(n)
    return np.ascontiguousarray(np.stack([10.0 * (i // 2) + 0.001 * (i % 2), 0.0 * i, 0.0 * i], 1), dtype=np.float32)


@pytest.mark.parametrize("make,n,k", [(uneven_line, 52, 50), (uneven_line, 70, 5), (tight_pairs, 7, 5)], ids=["n=k+2", "n=70", "n=7"])
def test_smallest_clouds(gpu, make, n, k):
    """(Seven points: one stencil covers whatever grid the build gives them -- neither this cloud nor the line produced a
    redo, 0 redone rows on an MI355X -- so that size checks the three ways against each other and nothing else.)"""
    _, t = three_ways(gpu["capi"], make(n), k, what=f"{make.__name__} n={n} k={k}")
    if n > 7:
        assert t["redone_queries"] >= 1 and t["ring_fallbacks"] >= 1


def alternation(capi, shapes, async_mode):
    """One handle: cloud A, another cloud B of the same size, then k = 50 followed by k = 30 -- the table's rows hold an
    earlier call's lists (and, at another pitch, anything at all) when each sweep starts."""
    a, b = two_density_torus(shapes, 12_000, seed=3), two_density_torus(shapes, 12_000, seed=4)
    steps = [(a, 50), (b, 50), (a, 50), (b, 30), (a, 50)]
    h = capi.Handle(0)
    try:
        if async_mode:
            h.set_async(True)
        else:
            h.set_stats(True)
        for i, (pts, k) in enumerate(steps):
            got, t = fused(capi, h, pts, k, 0.0, capi.KNN_GRID, wait=async_mode)
            want, t_ref = one(capi, pts, k, 0.0, capi.KNN_GRID_EXACT)
            same(got, want, f"step {i} k={k} async={async_mode}")
            fresh, t_fresh = one(capi, pts, k, 0.0, capi.KNN_GRID)
            same(got, fresh, f"step {i} k={k} async={async_mode} against a fresh handle")
            assert t_fresh["redone_queries"] >= 1 and t_fresh["ring_fallbacks"] >= 1
            if not async_mode:      # (its cell edge starts from the previous build's: not the fresh handle's redo set)
                assert t["redone_queries"] >= 1 and t["ring_fallbacks"] >= 1
    finally:
        h.close()


def test_one_handle_cloud_after_cloud(gpu):
    alternation(gpu["capi"], gpu["shapes"], False)


def test_one_handle_cloud_after_cloud_async(gpu):
    with seed_switch(None):
        alternation(gpu["capi"], gpu["shapes"], True)


def test_index_range_whose_grid_left_points_out(gpu, seam):
    pts = np.ascontiguousarray(seam[np.argsort(seam[:, 0], kind="stable")])      # the owned quarter is one end of the cloud
    _, t = three_ways(gpu["capi"], pts, 50, rows=(0, len(pts) // 4), what="owned quarter")
    assert t["grid_points"] < len(pts) and t["redone_queries"] >= 1

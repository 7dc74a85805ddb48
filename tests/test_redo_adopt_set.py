"""The argument the exact sweep's adoption of a redo row rests on (csrc/pct_knn_sweep.h, Sweep::adopt), in NumPy.

A row the fast sweep marks brings S, the k+1 nearest candidates of the query's 27 cells (the query's own record among them),
and the exact sweep does not walk those cells again: it tests the guarantee of ring 1 and, where that fails, merges S with
the candidates of the rings beyond, widening as k_knn_exact always does.  Claim: the list that leaves is brute force's.
The mark needs the SET to be right, and the fast sweep's keys are quantised distances: where entries k and k+1 share a key,
either of the two may stand at k.  Second claim: with the wrong one of the two inside, the list that leaves is not brute
force's whenever the right one belongs to the answer -- ring 1 is never looked at again, so nothing mends it.  That is why
a row with equal keys at the boundary is not marked."""
import numpy as np
import pytest


def guaranteed_r2(dims, cell, c, g, ring):
    """query_guaranteed_r2 (csrc/pct_query_plan.h): the squared radius the cube of `ring` cells around cell c vouches for,
    for a query at fraction g of its cell; a side where the cube reaches the grid's rim vouches for everything."""
    gmin = np.inf
    for a in range(3):
        if c[a] - ring > 0:
            gmin = min(gmin, g[a] + ring)
        if c[a] + ring < dims[a] - 1:
            gmin = min(gmin, (1.0 - g[a]) + ring)
    rr = gmin * cell * (1.0 - 1e-6)
    return rr * rr


def widen(ring):
    """k_knn_exact's next radius: one ring at a time near the query, then by half the radius"""
    return ring + 1 if ring < 4 else ring + (ring + 1) // 2


def nearest(d2, ids, count):
    """the `count` smallest of ids under the sweep's order (d2, index)"""
    order = np.lexsort((ids, d2[ids]))
    return ids[order[:count]]


def cloud_with_grid(rng, n, cells_per_axis, clumped):
    pts = rng.random((n, 3))
    if clumped:         # half of the points in one corner: sparse queries reach far beyond their 27 cells
        pts[: n // 2] *= 0.25
    pts = pts.astype(np.float32).astype(np.float64)
    dims = np.array(cells_per_axis)
    origin = pts.min(axis=0)
    cell = float((pts.max(axis=0) - origin).max() / dims.max()) * (1.0 + 1e-9) + 1e-12
    coords = np.minimum(np.floor((pts - origin) / cell).astype(np.int64), dims - 1)
    return pts, dims, origin, cell, coords


def continue_from(start, q, k, d2, cheb, dims, cell, c, g):
    """k_knn_exact from an adopted list `start` (k+1 ids): the guarantee test of ring 1, then shell after shell merged in.
    Returns the k+1 ids of the final list and the ring it ended in."""
    best = np.array(start)
    ring = 1
    while True:
        tau = d2[best].max()
        if tau <= guaranteed_r2(dims, cell, c, g, ring):
            return best, ring
        nxt = widen(ring)
        shell = np.flatnonzero((cheb > ring) & (cheb <= nxt))
        best = nearest(d2, np.concatenate([best, shell]), k + 1)
        ring = nxt


CASES = [(0, 400, (6, 6, 6), False, 8), (1, 600, (9, 7, 5), True, 12), (2, 500, (12, 3, 1), True, 20), (3, 300, (5, 5, 5), True, 30)]


@pytest.fixture(scope="module", params=CASES, ids=lambda p: f"seed{p[0]}-n{p[1]}-k{p[4]}")
def walked(request):
    seed, n, grid, clumped, k = request.param
    rng = np.random.default_rng(seed)
    pts, dims, origin, cell, coords = cloud_with_grid(rng, n, grid, clumped)
    rows = []
    for q in range(n):
        d = pts - pts[q]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        cheb = np.abs(coords - coords[q]).max(axis=1)
        inside = np.flatnonzero(cheb <= 1)
        if len(inside) < k + 2:
            continue                                    # fewer than k+1 candidates: the list has padding, the row is never marked
        order = np.lexsort((inside, d2[inside]))
        g = (pts[q] - origin) / cell - coords[q]
        rows.append(dict(q=q, k=k, d2=d2, cheb=cheb, dims=dims, cell=cell, c=coords[q], g=g, inside=inside[order],
                         brute=nearest(d2, np.arange(n), k + 1)))
    assert len(rows) > n // 4
    return rows


def test_adopted_set_widened_equals_brute_force(walked):
    beyond = 0
    for r in walked:
        k = r["k"]
        got, ring = continue_from(r["inside"][: k + 1], r["q"], k, r["d2"], r["cheb"], r["dims"], r["cell"], r["c"], r["g"])
        assert r["inside"][0] == r["q"]                 # (distinct points: the own record leads its list)
        assert np.array_equal(np.sort(got), np.sort(r["brute"])), r["q"]
        assert np.array_equal(got, r["brute"]), r["q"]
        beyond += ring > 1
    print("rows", len(walked), "of which answered beyond ring 1:", beyond)
    assert beyond >= 1                                  # the case is about the rows that widen


def test_wrong_entry_at_the_boundary_is_not_mended(walked):
    hit = 0
    for r in walked:
        k = r["k"]
        right, other = r["inside"][k], r["inside"][k + 1]
        wrong = np.concatenate([r["inside"][:k], [other]])          # entry k+1 in entry k's place
        got, ring = continue_from(wrong, r["q"], k, r["d2"], r["cheb"], r["dims"], r["cell"], r["c"], r["g"])
        if right in r["brute"]:
            assert right not in got and not np.array_equal(np.sort(got), np.sort(r["brute"])), r["q"]
            hit += 1
    print("rows whose boundary entry belongs to the answer:", hit, "of", len(walked))
    assert hit >= 1

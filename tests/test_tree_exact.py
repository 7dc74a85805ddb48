"""tests/tree_exact.py against itself, on the CPU: the level against a brute-force count, the live pieces against what a
build must leave, the recorded row of test_gpu_grid_plan, and -- for every case of tests/test_gpu_tree_build.py -- the
share of rows whose exact-sweep walk the restatement cannot decide (printed; at most 1 % per case, which is a condition
on the choice of the clouds, not a tolerance)."""
import numpy as np
import pytest

import tree_exact as te
import test_gpu_tree_build as T
from test_gpu_grid_plan import EXPECTED


def _codes_of(pts):
    cb = te.cube(pts)
    q = np.clip(np.floor((pts.astype(np.float32).astype(np.float64) - cb["o"]) * cb["inv"]), 0, te.TOP).astype(np.int64)
    return np.sort(te.morton(q[:, 0], q[:, 1], q[:, 2]))


def _small_clouds():
    rng = np.random.default_rng(8)
    blob = rng.normal(size=(300, 3)).astype(np.float32)
    piles = np.concatenate([np.repeat(blob[:3], 40, 0), blob[:200], np.repeat(blob[5:6], 77, 0)])
    frac = (rng.integers(0, 9, (400, 3)) / 8.0).astype(np.float32)                     # on the faces of the cells of levels <= 18
    frac2 = np.concatenate([(rng.integers(0, 1025, (300, 3)) / 1024.0), [[0, 0, 0], [1, 1, 1]]]).astype(np.float32)
    return {"blob": blob, "piles": piles, "few": blob[:9], "one_pile": np.ones((50, 3), np.float32), "eighths": frac, "1024ths": frac2,
            "pair": blob[:2]}


@pytest.mark.parametrize("name", sorted(_small_clouds()))
@pytest.mark.parametrize("n_min", [2, 3, 14, 28, 124])
def test_level_is_the_brute_force_count(name, n_min):
    codes = _codes_of(_small_clouds()[name])
    n = len(codes)
    want = np.full(n, te.BITS)
    for j in range(n):
        for l in range(te.BITS + 1):
            if int(((codes >> np.uint64(3 * l)) == (codes[j] >> np.uint64(3 * l))).sum()) >= n_min:
                want[j] = l
                break
    assert np.array_equal(te.level_by_count(codes, n_min), want)
    assert np.array_equal(te.level_by_count(codes, n_min, 5), np.minimum(want, 5))
    if n < n_min:
        assert (want == te.BITS).all()


def test_codes_round_trip_and_order():
    rng = np.random.default_rng(3)
    q = rng.integers(0, te.TOP + 1, (1000, 3))
    q[:3] = [[0, 0, 0], [te.TOP] * 3, [1, 2, 4]]
    c = te.morton(q[:, 0], q[:, 1], q[:, 2])
    assert int(c[1]) == (1 << 63) - 1 and int(c[2]) == 1 | 2 << 3 | 4 << 6          # x lowest
    for a in range(3):
        assert np.array_equal(te.compact3(c >> np.uint64(a)), q[:, a])


def test_knobs_and_max_level():
    assert te.knobs(30)["n_min"] == 14 and te.knobs(1)["n_min"] == 2 and te.knobs(30, f_min=4.0)["n_min"] == 124
    assert te.knobs(30, f_min=9.0)["n_min"] == 14 and te.knobs(30, items_q=65)["items_q"] == 12
    assert te.knobs(59)["cap"] == 768 and te.knobs(60)["cap"] == 768 and te.knobs(61)["cap"] == 1024
    assert te.knobs(30, split=63)["cap"] == 768 and te.knobs(30, split=64)["cap"] == 64 and te.knobs(30, split=64)["kernel_cap"] == 768
    assert te.max_level(0.0, 1.0) == 21 and te.max_level(0.5, 1.0) == 0 and te.max_level(2.0 ** 21, 1.0) == 21
    assert te.max_level(4.0, 1.0) == 3 and te.max_level(4.0 * (1 - 2e-6), 1.0) == 2 and te.max_level(5.0, 1.0) == 3


def test_recorded_row_of_the_scan(built):
    """test_gpu_grid_plan.EXPECTED["auto_scan"], recorded from a run, is what the restatement derives."""
    b = T.restate(next(c for c in T.CASES if c[0] == "scan_k30"), built["shapes"])[3]
    assert (b["segments0"], b["items0"], b["over_segments"], b["over_points"]) == (1026, 2174, 33, 356)
    row = EXPECTED["auto_scan"]
    assert (b["segments"], float(b["cell"]).hex(), b["n"], b["items"], (b["n"] / b["segments"]).hex()) == row[1:]
    assert (b["segments"], b["items"], float(b["cell"]).hex()) == (1068, 2220, "0x1.530afdc2aa400p-20")


@pytest.mark.parametrize("case", T.CASES, ids=[c[0] for c in T.CASES])
def test_live_pieces_and_undecided_share(built, case):
    name = case[0]
    pts, k, eps, b, w, want = T.restate(case, built["shapes"])
    n, codes, cap = b["n"], b["codes"], b["cap"]
    pieces = b["pieces"]
    # the live pieces partition [0, n), each inside one cell of its level, each within the cap or at level 0
    assert pieces[0][4] == 0 and sum(p[5] for p in pieces) == n
    for p, nxt in zip(pieces, pieces[1:]):
        assert p[4] + p[5] == nxt[4]
    for l, cx, cy, cz, first, rows, pop, ranges in pieces:
        run = codes[first:first + rows]
        assert (b["level"][first:first + rows] == l).all()
        assert (te.compact3(run) >> l == cx).all() and (te.compact3(run >> np.uint64(1)) >> l == cy).all() and (te.compact3(run >> np.uint64(2)) >> l == cz).all()
        assert rows <= pop and 1 <= ranges <= 27
        if b["refine"]:
            assert pop <= cap or l == 0
    assert b["segments0"] <= b["items0"] <= n and b["segments"] <= b["items"]
    assert b["items"] - b["items0"] <= b["over_points"] and sum(i[1] for i in b["live_items"]) == n
    assert (b["level"] <= b["level0"]).all() and (b["level"] <= b["max_level"]).all()
    share = want["undecided"] / n
    print(f"{name}: n {n} k {k} eps {eps:g}: segments {b['segments0']} -> {b['segments']}, items {b['items0']} -> {b['items']}, over {b['over_segments']} "
          f"({b['over_points']} points), cap {cap}, levels {b['level'].min()}..{b['level'].max()}, overflow items {want['lds_overflows']}, "
          f"rows redone at least {want['redone_min']}, climbing rows {want['fallbacks']}, steps {want['steps']}, undecided {want['undecided']} ({100 * share:.3f} %)")
    assert share <= 0.01

    # what each case is there for
    if name in T.EXPECTED_MAX_LEVEL:
        assert b["max_level"] == T.EXPECTED_MAX_LEVEL[name]
    if name in ("tiny7", "tiny13"):
        assert b["n_min"] < n
    if name in ("tiny7_below_nmin", "tiny13_below_nmin"):
        assert n < b["n_min"] and b["segments"] == 1 and (b["level"] == 21).all() and pieces[0][:4] == (21, 0, 0, 0)
    if name == "segments_not_by_8":
        assert b["segments0"] % 8 != 0
    if name == "identical":
        assert (b["level"] == 0).all() and b["segments"] == 1 and b["over_segments"] == 0 and pieces[0][6] == n > cap
        assert want["lds_overflows"] == b["items"] == 250 and want["redone_min"] == n and want["fallbacks"] == (0, 0)
    if name == "twins":
        assert any(p[0] == 0 and p[5] >= 900 for p in pieces) and b["over_segments"] > 0
    if name == "line":
        assert max(p[7] for p in pieces) <= 3
    if name == "lattice":
        assert want["lds_overflows"] > 0 and max(p[7] for p in pieces) == 27
    if name in ("two", "scan_k30"):
        assert b["over_segments"] > 0 and b["segments"] > b["segments0"]
    if name in ("scan_no_refine", "no_refine"):
        assert b["segments"] == b["segments0"] and b["items"] == b["items0"] and (b["level"] == b["level0"]).all()
    if name == "scan_no_refine":
        assert b["over_segments"] == 33
    if name == "split64":
        assert b["over_points"] > n // 8 + 64 and b["over_segments"] > 0.9 * b["segments0"]
    if name == "items_q1":
        assert b["items0"] == n
    if name == "far64":
        assert pts.dtype == np.float64 and not np.array_equal(pts.astype(np.float32).astype(np.float64), pts)


def _walk_one_row(pts, k, eps, b, j):
    """k_knn_exact_tree for sorted row j, one cell and one candidate at a time in Python integers"""
    codes = [int(c) for c in b["codes"]]
    rec = pts.astype(np.float32).astype(np.float64)[b["order"]]
    q = pts.astype(np.float64)[b["order"]][j] if pts.dtype == np.float64 else rec[j]
    f = [sum(((codes[j] >> (3 * i + a)) & 1) << i for i in range(te.BITS)) for a in range(3)]
    level, rounds, steps = int(b["level"][j]), 0, 0
    while True:
        dim, c = 1 << (te.BITS - level), [v >> level for v in f]
        d2 = []
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    x, y, z = c[0] + dx, c[1] + dy, c[2] + dz
                    if not (0 <= x < dim and 0 <= y < dim and 0 <= z < dim):
                        continue
                    inside = [i for i, code in enumerate(codes) if [sum(((code >> (3 * (i2 + level) + a)) & 1) << i2 for i2 in range(te.BITS - level))
                                                                     for a in range(3)] == [x, y, z]]
                    steps += (len(inside) + 63) // 64
                    d2 += [float(((rec[i][0] - q[0]) ** 2 + (rec[i][1] - q[1]) ** 2) + (rec[i][2] - q[2]) ** 2) for i in inside]
        tau = sorted(d2)[k] if len(d2) >= k + 1 else np.inf
        cell, inv = b["cell"] * 2.0 ** level, b["inv"] * 2.0 ** -level
        g = [(q[a] - b["o"][a]) * inv - c[a] for a in range(3)]
        r2 = float(te.guaranteed_r2(dim, cell, c[0], c[1], c[2], np.float64(g[0]), np.float64(g[1]), np.float64(g[2])))
        if min(tau, eps * eps if eps > 0 else np.inf) <= r2 or level >= te.BITS:
            return rounds, steps
        level += 1
        rounds += 1


@pytest.mark.parametrize("name,k,eps", [("n255", 10, 0.0), ("n255", 30, 0.3), ("tiny13", 12, 0.0)])
def test_walk_is_the_row_by_row_walk(built, name, k, eps):
    """exact_walk groups the rows of a cell and takes a round per pass; a row alone, cell by cell, walks the same way"""
    pts = T.cloud(name, built["shapes"])
    b = te.build(pts, k, eps)
    w = te.exact_walk(pts, k, eps, b)
    assert w["decided"].all() and (w["rounds"] > 0).any() == ((name, k) == ("n255", 10))
    for j in range(0, len(pts), 3):
        assert (int(w["rounds"][j]), int(w["steps"][j])) == _walk_one_row(pts, k, eps, b, j), j
    assert np.array_equal(w["rounds"], w["rounds_hi"]) and np.array_equal(w["steps"], w["steps_hi"])


def test_every_stencil_cell_counts(built, monkeypatch):
    """A stencil population summed over 26 cells must show, whichever cell is left out: over the two turned scans, the loss
    of any one of the 27 changes the segments (or their points) over the cap, which the GPU test compares."""
    orig = te.stencil_ranges
    seen = set()
    for name in T.TILTS:
        pts = T.cloud(name, built["shapes"])
        full = te.build(pts, 30, refine=False)
        for t in range(27):
            def without(codes, l, cx, cy, cz, t=t):
                first, rows = orig(codes, l, cx, cy, cz)
                rows = rows.copy()
                rows[:, t] = 0
                return first, rows
            monkeypatch.setattr(te, "stencil_ranges", without)
            less = te.build(pts, 30, refine=False)
            monkeypatch.setattr(te, "stencil_ranges", orig)
            if (less["over_segments"], less["over_points"]) != (full["over_segments"], full["over_points"]):
                seen.add(t)
    assert seen == set(range(27)), sorted(set(range(27)) - seen)


def test_refused_cube(built):
    pts = T.cloud("refused", built["shapes"])
    assert not te.build(pts, 30)["built"] and te.build(T.cloud("torus", built["shapes"]), 30)["built"]
    assert not te.build(T.cloud("torus", built["shapes"]), 30, eps=1e-19)["built"]

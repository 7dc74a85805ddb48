"""tests/grid_exact.py against the project's own records and against itself, on the CPU: the rows of
test_gpu_grid_plan.EXPECTED that were recorded from runs are DERIVED here, so is the census line quoted in
tests/test_gpu_step_route.py; the filing of points, the census and the final ring are checked against brute force; and
for every case of tests/test_gpu_grid_exact.py the rows the restatement cannot decide are at most 0.1 % of the owned rows
(a condition on the choice of the clouds, not a tolerance)."""
import numpy as np
import pytest

import grid_exact as ge
import test_gpu_grid_exact as T
import test_gpu_grid_plan as plan
import test_gpu_step_route as route
from test_gpu_tree_build import TILTS
from test_gpu_tree_build import cloud as tree_cloud


@pytest.fixture(scope="module")
def clouds(built):
    return plan.make_clouds(built["shapes"])


def _derive_scenario(scenario, clouds):
    """the steps of one scenario of test_gpu_grid_plan on one restated handle: {name: row}"""
    h, out = ge.Handle(), {}
    for name, cname, k, eps, algo, shard, knobs in scenario:
        assert algo in ("GRID", "AUTO")
        lo, hi = shard[1:] if shard else (0, len(clouds[cname]))
        b = h.build(clouds[cname], k, eps, begin=lo, end=hi, no_spec="PCT_NO_SPEC" in knobs, may_give_up=algo == "AUTO")
        out[name] = b
    return out


# Left out, because their box is not the cloud's: `range` (culled: the owned rows' box and a margin, ownership_exact.py),
# `slab` (culled by slab), `levels` (the first pass of a chained sweep: level_mode, another cell budget and two passes),
# `auto_scan` (the hierarchical list: tests/test_tree_exact.py derives it).  PCT_GRID_ATOMIC changes the kernels, not a rule.
DERIVED = ("plain", "plain_B", "atomic", "f64", "eps", "k80", "range_no_cull", "stream_A", "stream_A_again", "stream_A2_atomic", "stream_B",
           "stream_A_last", "warm_A", "warm_A_no_spec", "auto_scan_grid", "auto_torus")


def test_recorded_rows_are_derived(clouds):
    seen = {}
    for scenario in plan.SCENARIOS:
        names = [st[0] for st in scenario]
        if not set(names) & set(DERIVED):
            continue
        if names[0] == "auto_scan_grid":
            # the scan's uniform list, then PCT_KNN_AUTO on the handle: the warm-started edge asks for more than 16 cells per
            # point, the scan's own first guess replaces it and the search gives up on a later pass; the torus behind it
            # drops the inherited edge as well and is built
            h = ge.Handle()
            seen["auto_scan_grid"] = h.build(clouds["scan"], plan.K)
            gave_up = h.build(clouds["scan"], plan.K, may_give_up=True)
            assert gave_up["verdict"] == "gave_up" and gave_up["lines"][0][0] == 0
            seen["auto_torus"] = h.build(clouds["T"], plan.K, may_give_up=True)
            assert seen["auto_torus"]["give_up_test"] and seen["auto_torus"]["hinted"]          # (inherited, then dropped)
            continue
        seen.update(_derive_scenario(scenario, clouds))
    for name in DERIVED:
        print(name, ge.row_of(seen[name]), seen[name]["lines"])
        assert seen[name]["verdict"] == "built" and not seen[name]["trimmed"]
        assert ge.row_of(seen[name]) == plan.EXPECTED[name], name
    # what the stream is there for: speculative builds on the remembered box, and a dropped attempt in front of another box
    assert seen["stream_A_again"]["speculative"] and seen["stream_A_again"]["hinted"] and seen["stream_A2_atomic"]["speculative"]
    assert len(seen["stream_B"]["lines"]) == 2 and not seen["stream_B"]["speculative"]
    assert not seen["warm_A_no_spec"]["speculative"] and seen["warm_A_no_spec"]["hinted"]
    assert seen["k80"]["grid_iters"] == 2 and seen["auto_scan_grid"]["grid_iters"] == 4 and seen["auto_scan_grid"]["d_last"] < 2.0


def test_census_line_of_the_step_route(built):
    """the line quoted in the docstring of tests/test_gpu_step_route.py, PCT_GRID_DEBUG=1 on its census cloud:
        [auto] occupancy 27.1, 9998 non-empty cells, skew 4.13
        [auto] census: 65536 queries, 11065 overflow, 30459 short, 9.2 non-empty stencil cells"""
    pts = T.cloud("census", built["shapes"])
    b = ge.build(pts, T.CENSUS_K, may_give_up=True)
    words, cells = ge.census(b, T.CENSUS_K)
    print(ge.row_of(b), b["nonempty"], words, cells)
    assert b["verdict"] == "built"
    assert ("%.1f" % b["occupancy"], b["nonempty"], "%.2f" % (b["occupancy"] * b["nonempty"] / len(pts))) == ("27.1", 9998, "4.13")
    assert words[:3] == (65536, 11065, 30459) and "%.1f" % cells == "9.2"
    assert T.CENSUS_K == 40 and route.N_CENSUS == 65536


# ---- own properties -----------------------------------------------------------------------------------------------------------
def _built_cases(shapes):
    for case in T.CASES:
        for w in T.restate(case, shapes):
            if not w["grid"]["trimmed"]:
                yield case[0], w


def test_every_point_lies_in_its_cell_and_the_counts_add_up(built):
    for name, w in _built_cases(built["shapes"]):
        for b in (w["grid"], w["exact"]):
            c = b["cells_obj"]
            p = np.asarray(w["pts"]).astype(np.float32).astype(np.float64)
            a, lo = b["cell_size"], b["lo"].astype(np.float64)
            dims = np.asarray(b["dims"])
            # geometrically, within one rounding of the product; a point outside a remembered box sits in the rim cell
            slack = 4 * np.finfo(np.float64).eps * (np.abs(p - lo) / a + 1.0)
            t = (p - lo) / a
            inside_lo = (t >= c.coord - slack) | (c.coord == 0)
            inside_hi = (t <= c.coord + 1 + slack) | (c.coord == dims - 1)
            assert inside_lo.all() and inside_hi.all(), name
            assert (c.coord >= 0).all() and (c.coord < dims).all()
            assert int(c.total.sum()) == len(p) and int(c.owned.sum()) == w["rows"][1] - w["rows"][0], name
            assert (c.owned <= c.total).all() and b["nonempty"] == len(c.ids) and b["cells"] == int(np.prod(dims.astype(object)))
            assert ge.census(b, w["k"])[0][0] == w["rows"][1] - w["rows"][0]
            q = b["items_q"]
            assert b["occupied_cells"] == sum(-(-int(o) // q) for o in c.owned)


def test_every_stencil_cell_counts(built):
    """A stencil summed over 26 cells must show, whichever cell is left out: over the two turned scans the loss of any one
    of the 27 changes the census."""
    seen = set()
    for name in TILTS:
        pts = tree_cloud(name, built["shapes"])
        b = ge.build(pts, 30)
        full = ge.census(b, 30)[0]
        for t in range(27):
            if ge.census(b, 30, drop=t)[0] != full:
                seen.add(t)
    assert seen == set(range(27)), sorted(set(range(27)) - seen)


def test_census_against_a_loop_over_the_items(built):
    """k_item_census item by item in Python integers, on a range-owned scan (owned != total; overflowing, short and other
    stencils) under PCT_ITEMS_Q = 5"""
    pts = T.cloud("scan", built["shapes"])
    k, q = 30, 5
    b = ge.build(pts, k, begin=5000, end=15000, items_q=q)
    c = b["cells_obj"]
    nx, ny, nz = b["dims"]
    total = {int(i): int(t) for i, t in zip(c.ids, c.total)}
    v = [0, 0, 0, 0]
    n_items = 0
    for cell, own in zip(c.ids, c.owned):
        cell, own = int(cell), int(own)
        cx, cy, cz = cell % nx, (cell // nx) % ny, cell // (nx * ny)
        for chunk in range(-(-own // q)):
            nq = min(q, own - chunk * q)
            n_items += 1
            m = occupied = 0
            for dz in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    z, y = cz + dz, cy + dy
                    if z < 0 or z >= nz or y < 0 or y >= ny:
                        continue
                    for x in range(max(cx - 1, 0), min(cx + 1, nx - 1) + 1):
                        t = total.get((z * ny + y) * nx + x, 0)
                        occupied += t > 0
                        m += t
            v[0] += nq
            if m > ge.stage_cap(k):
                v[1] += nq
            elif 2 * m < 5 * (k + 1):
                v[2] += nq
            else:
                v[3] += nq * occupied
    assert tuple(v) == ge.census(b, k)[0] and n_items == b["occupied_cells"] and v[0] == 10000 and min(v) > 0


def test_final_ring_is_one_exactly_where_the_stencil_vouches():
    """500 points, O(n^2): the final ring is 1 exactly where the k + 1 nearest records all lie in the 27 cells around the
    row's cell and the (k+1)-th lies within the guaranteed radius of ring 1"""
    rng = np.random.default_rng(19)
    pts = rng.normal(size=(500, 3)).astype(np.float32)
    k = 8
    b = ge.build(pts, k)
    p = pts.astype(np.float64)
    d2 = ((p[None, :, 0] - p[:, None, 0]) ** 2 + (p[None, :, 1] - p[:, None, 1]) ** 2) + (p[None, :, 2] - p[:, None, 2]) ** 2
    order = np.argsort(d2, axis=1, kind="stable")[:, :k + 1]
    tau = np.take_along_axis(d2, order, 1)[:, k]
    assert np.array_equal(tau, ge.tau_of(pts, k, np.arange(500)))
    ring, decided = ge.final_rings(pts, b, tau)
    assert decided.all() and (ring == 1).any() and (ring > 1).any()
    c = b["cells_obj"].coord
    g = (p - b["lo"].astype(np.float64)) * b["inv"] - c
    r2 = ge.guaranteed_r2(b, c, g, 1)
    in_stencil = (np.abs(c[order] - c[:, None, :]).max(2) <= 1).all(1)
    assert np.array_equal(ring == 1, tau <= r2)
    assert np.array_equal(ring == 1, in_stencil & (tau <= r2))
    # the ring sequence: 1, 2, 3, 4, then by half the radius
    seq = ge.ring_sequence()
    assert [next(seq) for _ in range(8)] == [1, 2, 3, 4, 6, 9, 14, 21]
    assert set(np.unique(ring)) <= {1, 2, 3, 4, 6, 9, 14, 21}


@pytest.mark.parametrize("case", T.CASES, ids=[c[0] for c in T.CASES])
def test_undecided_rows_of_the_gpu_cases(built, case):
    for i, w in enumerate(T.restate(case, built["shapes"])):
        n_owned = w["rows"][1] - w["rows"][0]
        if w["grid"]["trimmed"]:
            print(case[0], i, "trimmed in", w["grid"]["trim_passes"], "passes")
            assert not w["grid"]["trim_undecided"] and case[0] == "outlier"
            continue
        g, x = w["grid"], w["exact"]
        print(f"{case[0]}[{i}]: k {w['k']} eps {w['eps']:g}: GRID {ge.row_of(g)} {g['lines']} spec {g['speculative']} hinted {g['hinted']} | "
              f"GRID_EXACT {ge.row_of(x)} {x['lines']} | overflow items {w['want_grid']['lds_overflows']} ({w['want_grid']['overflow_queries']} "
              f"queries), redone at least {w['want_grid']['redone_min']}, ring > 1 {w['want_grid']['fallbacks']} | {w['want_exact']['fallbacks']}, "
              f"max ring {w['want_grid']['max_ring']}, undecided {w['want_grid']['undecided']} | {w['want_exact']['undecided']}")
        assert g["verdict"] == "built" and x["verdict"] == "built" and not g["trim_undecided"] and not x["trim_undecided"]
        assert w["want_grid"]["undecided"] <= 0.001 * n_owned and w["want_exact"]["undecided"] <= 0.001 * n_owned
        # what each case is there for
        name = case[0]
        if name == "torus4k_k80":
            assert g["grid_iters"] == 2
        if name == "n_eq_k1":
            assert len(w["pts"]) == w["k"] + 1
        if name == "identical":
            assert g["dims"] == (1, 1, 1) and g["grid_iters"] == (1 if ge.NO_EXTENT_STOPS else 8) and w["want_grid"]["overflow_queries"] == n_owned
        if name == "line":
            assert g["dims"][1:] == (1, 1) and g["d_last"] < 2.0
        if name == "flat":
            assert g["dims"][2] == 1 and g["dims"][0] > 1 and g["dims"][1] > 1
        if name == "eps_clamp_02":
            assert g["cell_size"] == 0.2 * 1.000001
        if name == "eps_clamp_half_edge":
            assert g["cell_size"] == w["eps"] * 1.000001 and g["grid_iters"] == 1
        if name == "eps_tiny":
            assert g["give_up_test"] and g["cells"] <= 1 << 27 and g["cells"] * 2 > 1 << 27
        if name == "scan20k":
            assert g["grid_iters"] == 4 and g["cells"] == 1156896 and w["want_grid"]["lds_overflows"] > 0 and w["want_grid"]["max_ring"] > 1
        if name == "two_density":
            assert w["want_grid"]["max_ring"] > 4
        if name == "range_no_cull":
            c = g["cells_obj"]
            assert (c.owned < c.total).any() and n_owned == 1000
        if name == "items_q1":
            assert g["occupied_cells"] == n_owned
        if name == "warm":
            assert (g["speculative"], g["hinted"]) == ((False, False), (True, True), (False, True))[i]

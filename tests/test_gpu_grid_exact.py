"""The build of the uniform cell list (pct_build_grid, csrc/pct_grid.hip) against its restatement (tests/grid_exact.py).

Every edge, every source and both builds return the same rows bit for bit: a wrong first edge, a pass too many, a point
filed one cell over, a miscounted occupancy or census show in the timings only.  A case is a list of steps on ONE fresh
handle with the statistics on; every step sets its cloud (and its range) and then calls pct_knn three times: PCT_KNN_GRID,
PCT_KNN_GRID_EXACT, PCT_KNN_BRUTE.  The first two build a cell list each -- the second one warm-started and on the
remembered box, like any later build of a handle --, and the restatement follows the handle through all of them.  Per step,
with no tolerance anywhere:

  a. the build of both calls: the six words of pct_timings (grid_iters, cells, cell_size, grid_points, occupied_cells,
     occupancy) EQUAL the restatement's, and so do pass number, edge (as %g prints it), dims and cells of every
     "[grid] pass i:" line of PCT_GRID_DEBUG, the passes of an attempt the deferred-box check dropped included;
  b. PCT_KNN_GRID: lds_overflows EQUALS the work items whose stencil holds more points than the staging area;
     redone_queries is at least their queries plus the other decided rows whose final ring lies above 1;
  c. ring_fallbacks.  Only k_knn_exact adds to it (the three fast kernels never do), once per row it answered beyond ring
     1.  PCT_KNN_GRID_EXACT runs it over every owned row: the word lies between the decided rows with a final ring above 1
     and that plus the undecided rows, so it is EQUAL where no row is undecided.  PCT_KNN_GRID runs it over the redo list
     only, and the same bounds hold there: a fast kernel keeps a row only where key(tau) + 1 <= floor(guaranteed_r2 *
     scale) and ceil(eps^2 * scale) <= the same, which implies min(tau, eps^2) < guaranteed_r2(ring 1) -- so every row
     whose final ring lies above 1 is on the list, and the rows on it whose ring is 1 add nothing;
  d. indices, distances and counts of both calls equal the PCT_KNN_BRUTE run of the same handle; tau of the restatement
     is formed from that run's indices.

A trimmed cloud (`outlier`) is held to the trim decision and the number of trim passes only (grid_iters minus the pass
lines), and to (d).  The two census cases call pct_curvature with PCT_KNN_AUTO on the census cloud of
test_gpu_step_route.py: the "[auto] occupancy" and "[auto] census:" lines EQUAL the restatement's as printed.

Measured on the MI355X, per step: redone_queries of PCT_KNN_GRID = its lower bound + excess, then ring_fallbacks of the two
calls (each EQUAL to the restatement's); no row of any case was undecided, under either build (what was seen, not
thresholds):
  torus4k_k30 307 = 307 + 0, 0 | 0; k50 547 = 547 + 0, 0 | 7; k60 813 = 813 + 0, 13 | 36; k61 7 = 7 + 0, 7 | 10;
  k80 105 = 105 + 0, 45 | 18; k127 1868 = 1865 + 3, 282 | 351; n_eq_k1 0 = 0 + 0, 0 | 0; identical 3000 = 3000 + 0, 0 | 0;
  line 0 = 0 + 0, 0 | 0; flat 0 = 0 + 0, 0 | 0; lattice17 1701 = 1701 + 0, 0 | 0; far32 307 = 307 + 0, 0 | 0;
  f64 307 = 307 + 0, 0 | 0; eps_clamp_02, eps_clamp_half_edge, eps_tiny 0 = 0 + 0, 0 | 0; scan20k 15920 = 15920 + 0,
  12228 | 12228 (rings up to 32); two_density 1838 = 1838 + 0, 1838 | 1846 (rings up to 32); range_no_cull 87 = 87 + 0, 0 | 0;
  items_q1, items_q64 307 = 307 + 0, 0 | 0; warm 307 = 307 + 0, 83 = 83 + 0, 64 = 64 + 0, 0 | 0 each.
lds_overflows, the six words and every pass line equalled the restatement's in every step, and both census lines did.
The cloud of identical points took EIGHT passes on the commit before this test (the same one-cell grid each time, the edge
shrinking sixteenfold per pass, as the restatement predicted); EdgeSearch::accept now ends the search of a box without
extent at its first pass, and the case holds it to one.

What the cases turned out to be.  `n_eq_k1` (51 points, k = 50) is not one cell and one item: the search wants 28.5 of
the 51 points in a point's cell and settles on 2 x 2 x 1 cells in three passes, five work items.  `eps_tiny`
(eps = 1e-30) is built, not refused: eight turns of the cell-budget loop lead from the 2^62 sentinel to 130 901 050 cells,
accepted at once (more than half the budget, occupancy 1.0); the warm-started build behind it meets the sentinel on pass 0,
takes the cloud's own first guess -- which clamp_eps does not see again -- and is accepted there.
"""
import os
import re

import numpy as np
import pytest

import grid_exact as ge
import test_gpu_step_route as route
from test_gpu_grid_plan import KNOBS, make_clouds
from test_gpu_tree_build import _two

pytestmark = pytest.mark.gpu

N_TORUS = 4000


# ---- the clouds -----------------------------------------------------------------------------------------------------------
def _cloud(name, shapes):
    if name == "torus":
        return shapes.torus_random(N_TORUS, seed=11)
    if name == "torus12":
        return shapes.torus_random(N_TORUS, seed=12)
    if name == "torus64":
        return shapes.torus_random(N_TORUS, seed=11, dtype=np.float64)
    if name == "n51":
        return shapes.torus_random(51, seed=11)
    if name == "identical":
        return np.ones((3000, 3), np.float32)
    if name == "line":
        return np.stack([np.linspace(0, 1, 5000), np.zeros(5000), np.zeros(5000)], 1).astype(np.float32)
    if name == "flat":
        xy = np.random.default_rng(41).uniform(0, 1, (5000, 2))
        return np.stack([xy[:, 0], xy[:, 1], np.zeros(5000)], 1).astype(np.float32)
    if name == "lattice17":        # every coordinate a multiple of 1/16: points on cell faces wherever the edge is a multiple too
        g = np.arange(17, dtype=np.float32) / np.float32(16)
        return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    if name == "far32":
        return (shapes.torus_random(N_TORUS, seed=11).astype(np.float64) * 3.0 + 4000.0).astype(np.float32)
    if name == "scan":
        return make_clouds(shapes)["scan"]
    if name == "two":
        return _two()
    if name == "outlier":
        return np.concatenate([shapes.torus_random(N_TORUS, seed=11), np.full((1, 3), 1e4, np.float32)])
    if name == "census":
        return route.scan_cloud(route.N_CENSUS, route.CENSUS_DECADES, 5)
    raise KeyError(name)


_clouds = {}


def cloud(name, shapes):
    if name not in _clouds:
        _clouds[name] = _cloud(name, shapes)
        _clouds[name].setflags(write=False)
    return _clouds[name]


# A step: (cloud, k, eps, (begin, end) or None, {switch: value}); eps: a number, or ("first", f) = f times the first edge
# of a fresh handle's search.  A case: (id, [steps on one handle]).
def one(cloud_name, k, eps=0.0, rows=None, env=None):
    return [(cloud_name, k, eps, rows, env or {})]


CASES = [(f"torus4k_k{k}", one("torus", k)) for k in (30, 50, 60, 61, 80, 127)] + [
    ("n_eq_k1", one("n51", 50)),
    ("identical", one("identical", 20)),
    ("line", one("line", 30)),
    ("flat", one("flat", 30)),
    ("lattice17", one("lattice17", 26)),
    ("far32", one("far32", 30)),
    ("f64", one("torus64", 30)),
    ("eps_clamp_02", one("torus", 30, 0.2)),
    ("eps_clamp_half_edge", one("torus", 30, ("first", 0.5))),
    ("eps_tiny", one("torus", 10, 1e-30)),
    ("scan20k", one("scan", 30)),
    ("two_density", one("two", 50)),
    ("range_no_cull", one("torus", 30, rows=(1000, 2000), env={"PCT_NO_CULL": "1"})),
    ("items_q1", one("torus", 30, env={"PCT_ITEMS_Q": "1"})),
    ("items_q64", one("torus", 30, env={"PCT_ITEMS_Q": "64"})),
    ("warm", one("torus", 30) + one("torus12", 30) + one("torus12", 30, env={"PCT_NO_SPEC": "1"})),
    ("outlier", one("outlier", 30)),
]
CENSUS_K = 40
CENSUS_CASES = [("census", {}), ("census_no_tree", {"PCT_NO_TREE": "1"})]


def eps_of(spec, pts, k):
    if not isinstance(spec, tuple):
        return float(spec)
    lo, hi = ge.oe.box_of(pts)
    return spec[1] * ge.EdgeSearch(ge.oe.target_of(k), len(pts), [float(hi[a]) - float(lo[a]) for a in range(3)]).first()


_restated = {}


def restate(case, shapes, taus=None):
    """Per step of a case: dict(pts, k, eps, rows, env, grid (the PCT_KNN_GRID build), exact (the PCT_KNN_GRID_EXACT build),
    want_grid, want_exact (grid_exact.expected_counters; None for a trimmed build)).  taus: per step the squared distance to
    the (k+1)-th nearest of the owned rows (from the device's exhaustive sweep); computed here by default.  Cached per case
    when computed here."""
    name, steps = case
    if taus is None and name in _restated:
        return _restated[name]
    h, out = ge.Handle(), []
    for i, (cname, k, eps_spec, rows, env) in enumerate(steps):
        pts = cloud(cname, shapes)
        eps = eps_of(eps_spec, pts, k)
        lo, hi = rows or (0, len(pts))
        kw = dict(begin=lo, end=hi, items_q=ge.items_q_of(env.get("PCT_ITEMS_Q")), no_spec="PCT_NO_SPEC" in env)
        grid = h.build(pts, k, eps, **kw)
        if grid["trimmed"]:                  # (of a trimmed build only the decision is restated: the case ends here)
            out.append(dict(pts=pts, k=k, eps=eps, rows=(lo, hi), env=env, grid=grid, exact=None, want_grid=None, want_exact=None))
            break
        exact = h.build(pts, k, eps, **kw)
        tau = taus[i] if taus is not None else ge.tau_of(pts, k, np.arange(lo, hi), eps)
        out.append(dict(pts=pts, k=k, eps=eps, rows=(lo, hi), env=env, grid=grid, exact=exact,
                        want_grid=ge.expected_counters(pts, grid, k, tau, eps), want_exact=ge.expected_counters(pts, exact, k, tau, eps)))
    if taus is None:
        _restated[name] = out
    return out


# ---- the device -----------------------------------------------------------------------------------------------------------------
_PASS = re.compile(r"\[grid\] pass (\d+): n (\d+) owned (\d+) edge (\S+) dims (\d+) x (\d+) x (\d+) = (\d+) cells")
_AUTO = re.compile(r"\[auto\] occupancy (\S+), (\d+) non-empty cells, skew (\S+)")
_CENSUS = re.compile(r"\[auto\] census: (\d+) queries, (\d+) overflow, (\d+) short, (\S+) non-empty stencil cells")


def _set_env(env):
    for v in KNOBS:
        os.environ.pop(v, None)
    os.environ.update(env)


@pytest.fixture
def grid_env():
    saved = {v: os.environ.get(v) for v in KNOBS}
    yield _set_env
    for v, val in saved.items():
        os.environ.pop(v, None)
        if val is not None:
            os.environ[v] = val


def _pass_lines(err):
    return [(int(m[0]), m[3], (int(m[4]), int(m[5]), int(m[6])), int(m[7])) for m in _PASS.findall(err)]


def _six(t):
    return (t["grid_iters"], t["cells"], float(t["cell_size"]).hex(), t["grid_points"], t["occupied_cells"], float(t["occupancy"]).hex())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_grid_build_equals_restatement(gpu, grid_env, capfd, case):
    capi, shapes = gpu["capi"], gpu["shapes"]
    name, steps = case
    got = []
    h = capi.Handle(0)
    try:
        h.set_stats(True)
        for cname, k, eps_spec, rows, env in steps:
            pts = cloud(cname, shapes)
            eps = eps_of(eps_spec, pts, k)
            lo, hi = rows or (0, len(pts))
            grid_env(dict(env, PCT_GRID_DEBUG="1"))
            h.set_points(pts)
            if rows:
                h.set_query_range(lo, hi)
            res = {}
            for algo in ("GRID", "GRID_EXACT", "BRUTE"):
                capfd.readouterr()
                h.knn(k, eps, getattr(capi, "KNN_" + algo))
                res[algo] = (h.timings(), _pass_lines(capfd.readouterr().err), h.get_neighbors(lo, hi, want_count=True))
            got.append(res)
    finally:
        h.close()
        grid_env({})

    taus = [ge.tau_from_rows(cloud(st[0], shapes), np.arange(*(st[3] or (0, len(cloud(st[0], shapes))))), r["BRUTE"][2][0],
                             r["BRUTE"][2][2] if eps_of(st[2], cloud(st[0], shapes), st[1]) > 0 else None) for st, r in zip(steps, got)]
    want = restate(case, shapes, taus)
    for i, (w, r) in enumerate(zip(want, got)):
        step = f"{name}[{i}]"
        n_owned = w["rows"][1] - w["rows"][0]
        ib, db, cb = r["BRUTE"][2]
        # d. the rows
        for algo in ("GRID", "GRID_EXACT"):
            ia, da, ca = r[algo][2]
            assert np.array_equal(ia, ib) and np.array_equal(da, db) and np.array_equal(ca, cb), (step, algo)
        t, tx = r["GRID"][0], r["GRID_EXACT"][0]
        if w["grid"]["trimmed"]:
            print(step, "trimmed: grid_iters", t["grid_iters"], "pass lines", len(r["GRID"][1]), "restated trim passes", w["grid"]["trim_passes"])
            assert not w["grid"]["trim_undecided"] and w["grid"]["trim_passes"] > 0
            assert t["grid_iters"] - len(r["GRID"][1]) == w["grid"]["trim_passes"]
            continue
        wg, wx = w["want_grid"], w["want_exact"]
        print(step, "GRID", _six(t), r["GRID"][1], "restated", ge.row_of(w["grid"]), w["grid"]["lines"],
              "| lds_overflows", t["lds_overflows"], "restated", wg["lds_overflows"], "| redone_queries", t["redone_queries"], "lower bound",
              wg["redone_min"], "| ring_fallbacks", t["ring_fallbacks"], "restated", wg["fallbacks"], "undecided", wg["undecided"], "max ring", wg["max_ring"],
              "| GRID_EXACT", _six(tx), r["GRID_EXACT"][1], "restated", ge.row_of(w["exact"]), w["exact"]["lines"], "ring_fallbacks", tx["ring_fallbacks"],
              "restated", wx["fallbacks"], "undecided", wx["undecided"])
        assert not w["grid"]["trim_undecided"] and not w["exact"]["trim_undecided"]
        assert wg["undecided"] <= 0.001 * n_owned and wx["undecided"] <= 0.001 * n_owned
        # a. the build, of both calls
        assert w["grid"]["verdict"] == "built" and w["exact"]["verdict"] == "built"
        assert _six(t) == ge.row_of(w["grid"]), step
        assert _six(tx) == ge.row_of(w["exact"]), step
        # (the lines of a step are those of its own builds: the restatement's list runs over one build's attempts)
        assert r["GRID"][1] == w["grid"]["lines"], step
        assert r["GRID_EXACT"][1] == w["exact"]["lines"], step
        # b. the hand-overs of the fast sweep
        assert t["lds_overflows"] == wg["lds_overflows"], step
        assert t["redone_queries"] >= wg["redone_min"], step
        # c. the rows answered beyond ring 1
        assert tx["sweep_variant"] == 0 and tx["lds_overflows"] == 0 and tx["redone_queries"] == 0
        assert wx["fallbacks"][0] <= tx["ring_fallbacks"] <= wx["fallbacks"][1], step
        assert wg["fallbacks"][0] <= t["ring_fallbacks"] <= wg["fallbacks"][1], step
        if wx["undecided"] == 0:
            assert wx["fallbacks"][0] == wx["fallbacks"][1]


@pytest.mark.parametrize("name,env", CENSUS_CASES, ids=[c[0] for c in CENSUS_CASES])
def test_census_equals_restatement(gpu, grid_env, capfd, name, env):
    capi = gpu["capi"]
    pts = cloud("census", gpu["shapes"])
    b = ge.build(pts, CENSUS_K, may_give_up="PCT_NO_TREE" not in env)
    words, cells = ge.census(b, CENSUS_K)
    h = capi.Handle(0)
    try:
        h.set_points(pts)
        grid_env(dict(env, PCT_GRID_DEBUG="1"))
        capfd.readouterr()
        h.curvature(CENSUS_K, 0.0, capi.KNN_AUTO)
        err = capfd.readouterr().err
        algo = h.timings()["algo"]
    finally:
        h.close()
        grid_env({})
    auto, census = _AUTO.findall(err), _CENSUS.findall(err)
    print(name, auto, census, "restated", ge.row_of(b), b["nonempty"], words, cells, "algo", algo)
    assert b["verdict"] == "built" and _pass_lines(err)[:len(b["lines"])] == b["lines"]
    assert len(auto) == 1 and len(census) == 1, err
    assert auto[0] == ("%.1f" % b["occupancy"], str(b["nonempty"]), "%.2f" % (b["occupancy"] * b["nonempty"] / len(pts)))
    assert census[0] == (str(words[0]), str(words[1]), str(words[2]), "%.1f" % cells)
    assert algo == (capi.KNN_GRID_LEVELS if "PCT_NO_TREE" in env else capi.KNN_TREE)

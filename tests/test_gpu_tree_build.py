"""The build of the hierarchical cell list (PCT_KNN_TREE, csrc/pct_tree.hip) against its restatement (tests/tree_exact.py).

The tree's exact sweep climbs a level whenever the cube cannot vouch for a row, and the root vouches for everything: a
wrong build -- levels an octave off, a refinement that splits nothing or everything, miscounted stencils, a level
histogram that misleads PCT_KNN_AUTO -- still returns the right table, only slowly.  Per case, on a fresh handle with
the statistics on:

  a. the build: algo, cells (segments), occupied_cells (items), cell_size, grid_points, occupancy from pct_timings and,
     from the PCT_TREE_DEBUG line, items, segments, spread, the two-level share as printed, the segments over the cap,
     the cap and their points -- all EQUAL to the restatement's;
  b. the level of every row: under PCT_TREE_EXACT_ONLY the plan's family is kNoSweep (plan_sweep returns before it
     chooses one, csrc/pct_sweep_plan.h), k_knn_exact_tree alone runs over every row and alone adds to candidate_steps
     and ring_fallbacks: the first is then the sum over the rows of the 64-candidate steps of their 27 ranges at the
     level the build left (and of every level they climb), the second the rows that climb.  Equal to the restatement's
     where every row is decided, else held between its sums with the undecided rows at their fewest and most rounds;
  c. the hand-overs of the normal call: lds_overflows EQUALS the live items whose stencil exceeds the kernel's capacity
     or has more than 16 non-empty ranges; redone_queries is at least their rows plus the decided rows whose level cube
     cannot vouch, and at most that plus a budget (below);
  d. the rows: indices and distances of both calls equal the exhaustive sweep's of the same handle.

The budget of (c).  Beyond the lower bound the fast sweep redoes rows for reasons no restatement predicts: equal
float keys, the float32 pre-selection, and the order in which LDS atomics place candidates.  EXCESS is
redone_queries - lower bound per case, measured on the MI355X on the commit before this test existed (the library is
unchanged by it); a case may exceed twice its measured excess by 0.5 % of its points, no more.

Measured (redone_queries = lower bound + excess), two runs that agreed in every figure:
  tiny7 0 + 2, line 0 + 2, scan_k127 3832 + 15; every other case 0 over its lower bound: tiny13 0, tiny7_below_nmin 0,
  tiny13_below_nmin 0, n255 18, n256 18, n257 18, segments_not_by_8 416, identical 3000, twins 2512, lattice 3923,
  two 113, scan_k30 80, scan_k60 553, scan_k61 111, scan_k100 1822, scan_no_refine 435, scan_tilt_a 2918,
  scan_tilt_b 2195, eps_below_finest 0, eps_between_levels 0, eps_on_a_level 0, eps_just_under_a_level 0, eps_root 1613,
  split64 3961, no_refine 1901, items_q1 1613, items_q64 1613, nmin_0.1 3085, nmin_4 1952, far64 1608.
In the same runs lds_overflows, ring_fallbacks, candidate_steps and every word of (a) equalled the restatement's in
every case.

The two turned scans are there for the stencil sum: the scan lies in the xy plane, where the cells above and below a
coarse cell hold nothing, and a population summed over 26 cells passed every other case.

The issue's two smallest clouds (n = 7, k = 5 and n = 13, k = 12) are NOT below n_min: k + 1 <= n is a precondition of
the call and n_min = lrint(0.45 (k + 1)).  They stay as cases; the same clouds under PCT_TREE_NMIN=4 are the ones that
sit at level 21 in one segment.
"""
import os
import re

import numpy as np
import pytest

import tree_exact as te
from test_gpu_grid_plan import make_clouds

pytestmark = pytest.mark.gpu

TREE_KNOBS = ("PCT_TREE_DEBUG", "PCT_TREE_EXACT_ONLY", "PCT_TREE_SPLIT", "PCT_TREE_NO_REFINE", "PCT_ITEMS_Q", "PCT_TREE_NMIN",
              "PCT_NO_PAIR", "PCT_NO_PAIR_KERNEL", "PCT_NO_DUO_KERNEL")
N_TORUS = 4000
# two turns of the scan (angles about z, y, x): between them the loss of ANY one of the 27 stencil cells changes the
# segments over the cap (tests/test_tree_exact.py: test_every_stencil_cell_counts)
TILTS = {"scan_tilt_a": (0.7, 0.5, 0.9), "scan_tilt_b": (-0.4, 0.6, -1.1)}


# ---- the clouds -------------------------------------------------------------------------------------------------------
def _two(n_dense=18_180, n_sparse=1_820):
    """test_hierarchical_cell_list_on_awkward_clouds' two densities (10 : 1) with a loner, at 20 000 points"""
    rng = np.random.default_rng(77)
    plane = np.concatenate([rng.uniform(-1, 0, (n_dense, 2)), rng.uniform(0, 1, (n_sparse, 2))])
    two = np.stack([plane[:, 0], plane[:, 1], 0.05 * np.sin(plane[:, 0]) * np.cos(plane[:, 1])], 1).astype(np.float32)
    two[-1] = (0.9, -0.9, 0.0)
    return two


def _cloud(name, shapes):
    rng = np.random.default_rng(20)
    if name == "tiny7":
        return rng.normal(size=(7, 3)).astype(np.float32)
    if name == "tiny13":
        return rng.normal(size=(13, 3)).astype(np.float32)
    if name in ("n255", "n256", "n257", "n1000"):
        return shapes.torus_random(int(name[1:]), seed=31)
    if name == "identical":
        return np.ones((3000, 3), np.float32)
    if name == "twins":
        t = shapes.torus_random(N_TORUS, seed=33)
        return np.concatenate([t, np.repeat(t[1234:1235], 900, 0)])
    if name == "line":
        return np.stack([np.linspace(0, 1, 5000), np.zeros(5000), np.zeros(5000)], 1).astype(np.float32)
    if name == "lattice":          # every coordinate a multiple of ext / 16: on the faces of the cells of levels <= 17
        g = np.arange(17, dtype=np.float32) / np.float32(16)
        return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    if name == "two":
        return _two()
    if name == "scan":
        return make_clouds(shapes)["scan"]
    if name in TILTS:              # the scan lies in the xy plane, where the cells above and below a coarse cell are empty: turned, all 27 count
        a, b, c = TILTS[name]
        rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
        rx = np.array([[1, 0, 0], [0, np.cos(c), -np.sin(c)], [0, np.sin(c), np.cos(c)]])
        return (make_clouds(shapes)["scan"].astype(np.float64) @ (rz @ ry @ rx).T).astype(np.float32)
    if name == "torus":
        return shapes.torus_random(N_TORUS, seed=11)
    if name == "far64":
        return shapes.torus_random(N_TORUS, seed=5).astype(np.float64) * 3.0 + 4000.0
    if name == "refused":
        return (shapes.torus_random(N_TORUS, seed=11).astype(np.float64) * 1e-20).astype(np.float32)
    raise KeyError(name)


_clouds = {}


def cloud(name, shapes):
    if name not in _clouds:
        _clouds[name] = _cloud(name, shapes)
        _clouds[name].setflags(write=False)
    return _clouds[name]


def _eps_of(spec, pts):
    """eps given in units of the finest cell of the cloud's cube: ("cells", factor) | ("root", factor) | a number"""
    if not isinstance(spec, tuple):
        return float(spec)
    cb = te.cube(pts)
    return spec[1] * (cb["cell"] if spec[0] == "cells" else cb["root"])


# (id, cloud, k, eps, {switch: value})
CASES = [
    ("tiny7", "tiny7", 5, 0.0, {}),
    ("tiny13", "tiny13", 12, 0.0, {}),
    # (k + 1 <= n leaves n_min = lrint(0.45 (k + 1)) below n: a cloud smaller than n_min takes the switch)
    ("tiny7_below_nmin", "tiny7", 5, 0.0, {"PCT_TREE_NMIN": "4"}),
    ("tiny13_below_nmin", "tiny13", 12, 0.0, {"PCT_TREE_NMIN": "4"}),
    ("n255", "n255", 10, 0.0, {}),
    ("n256", "n256", 10, 0.0, {}),
    ("n257", "n257", 10, 0.0, {}),
    ("segments_not_by_8", "n1000", 10, 0.0, {}),
    ("identical", "identical", 20, 0.0, {}),
    ("twins", "twins", 30, 0.0, {}),
    ("line", "line", 30, 0.0, {}),
    ("lattice", "lattice", 26, 0.0, {}),
    ("two", "two", 50, 0.0, {}),
    ("scan_k30", "scan", 30, 0.0, {}),
    ("scan_k60", "scan", 60, 0.0, {}),
    ("scan_k61", "scan", 61, 0.0, {}),
    ("scan_k100", "scan", 100, 0.0, {}),
    ("scan_k127", "scan", 127, 0.0, {}),
    ("scan_no_refine", "scan", 30, 0.0, {"PCT_TREE_NO_REFINE": "1"}),
    ("scan_tilt_a", "scan_tilt_a", 30, 0.0, {}),
    ("scan_tilt_b", "scan_tilt_b", 30, 0.0, {}),
    ("eps_below_finest", "torus", 30, ("cells", 0.5), {}),
    ("eps_between_levels", "torus", 30, ("cells", 1.5 * 2.0 ** 15), {}),
    ("eps_on_a_level", "torus", 30, ("cells", 2.0 ** 15), {}),
    ("eps_just_under_a_level", "torus", 30, ("cells", 2.0 ** 15 * (1 - 2e-6)), {}),
    ("eps_root", "torus", 30, ("root", 1.0), {}),
    ("split64", "torus", 30, 0.0, {"PCT_TREE_SPLIT": "64"}),
    ("no_refine", "torus", 30, 0.0, {"PCT_TREE_NO_REFINE": "1"}),
    ("items_q1", "torus", 30, 0.0, {"PCT_ITEMS_Q": "1"}),
    ("items_q64", "torus", 30, 0.0, {"PCT_ITEMS_Q": "64"}),
    ("nmin_0.1", "torus", 30, 0.0, {"PCT_TREE_NMIN": "0.1"}),
    ("nmin_4", "torus", 30, 0.0, {"PCT_TREE_NMIN": "4"}),
    ("far64", "far64", 30, 0.0, {}),
]
EXPECTED_MAX_LEVEL = {"eps_below_finest": 0, "eps_between_levels": 16, "eps_on_a_level": 16, "eps_just_under_a_level": 15, "eps_root": 21}

# redone_queries - lower bound, measured per case (module docstring); the cases not named measured 0
EXCESS = dict({c[0]: 0 for c in CASES}, tiny7=2, line=2, scan_k127=15)


def restate(case, shapes):
    """(points, k, eps, build, walk, expected counters) of a case, computed once"""
    name, cname, k, eps_spec, env = case
    if name not in _restated:
        pts = cloud(cname, shapes)
        eps = _eps_of(eps_spec, pts)
        b = te.build(pts, k, eps, f_min=float(env["PCT_TREE_NMIN"]) if "PCT_TREE_NMIN" in env else None,
                     items_q=int(env["PCT_ITEMS_Q"]) if "PCT_ITEMS_Q" in env else None,
                     split=int(env["PCT_TREE_SPLIT"]) if "PCT_TREE_SPLIT" in env else None,
                     refine="PCT_TREE_NO_REFINE" not in env)
        w = te.exact_walk(pts, k, eps, b)
        _restated[name] = (pts, k, eps, b, w, te.expected_counters(b, w))
    return _restated[name]


_restated = {}

_LINE = re.compile(r"\[tree\] (\d+) points: (\d+) items in (\d+) segments \(levels spread (\d+), (\d+) % of the points on two adjacent levels\); "
                   r"(\d+) segments over (\d+) stencil points \((\d+) points\) split")


def _set_env(env):
    for v in TREE_KNOBS:
        os.environ.pop(v, None)
    os.environ.update(env)


@pytest.fixture
def tree_env():
    saved = {v: os.environ.get(v) for v in TREE_KNOBS}
    yield _set_env
    for v, val in saved.items():
        os.environ.pop(v, None)
        if val is not None:
            os.environ[v] = val


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_tree_build_equals_restatement(gpu, tree_env, capfd, case):
    capi = gpu["capi"]
    name, _, _, _, env = case
    pts, k, eps, b, w, want = restate(case, gpu["shapes"])
    n = len(pts)
    assert b["built"] and want["undecided"] <= 0.01 * n
    h = capi.Handle(0)
    try:
        h.set_stats(True)
        h.set_points(pts)
        tree_env(dict(env, PCT_TREE_DEBUG="1"))
        capfd.readouterr()
        h.curvature(k, eps, capi.KNN_TREE)
        err = capfd.readouterr().err
        t = h.timings()
        it, dt, ct = h.get_neighbors(0, n, want_count=True)
        tree_env(dict(env, PCT_TREE_EXACT_ONLY="1"))
        h.curvature(k, eps, capi.KNN_TREE)
        tx = h.timings()
        ix, dx, cx = h.get_neighbors(0, n, want_count=True)
        tree_env({})
        h.curvature(k, eps, capi.KNN_BRUTE)
        ib, db, cb = h.get_neighbors(0, n, want_count=True)
    finally:
        h.close()
    lines = _LINE.findall(err)
    print(name, "debug line", lines, "timings", {f: t[f] for f in ("algo", "cells", "occupied_cells", "grid_points", "lds_overflows", "redone_queries")},
          "exact only", {f: tx[f] for f in ("candidate_steps", "ring_fallbacks", "sweep_variant")}, "restated", want,
          "excess", t["redone_queries"] - want["redone_min"])

    # d. the rows
    for got in ((it, dt, ct), (ix, dx, cx)):
        assert np.array_equal(got[0], ib) and np.array_equal(got[1], db) and np.array_equal(got[2], cb), name

    # a. the build
    assert t["algo"] == capi.KNN_TREE and tx["algo"] == capi.KNN_TREE
    assert (t["cells"], t["occupied_cells"], t["grid_points"]) == (b["segments"], b["items"], n)
    assert float(t["cell_size"]).hex() == float(b["cell"]).hex()
    assert t["occupancy"] == n / b["segments"]
    assert len(lines) == 1, err
    assert tuple(int(v) for v in lines[0]) == (n, b["items"], b["segments"], b["spread"], int("%.0f" % (100.0 * b["share"])),
                                               b["over_segments"], b["cap"], b["over_points"])
    if name == "split64":          # the "larger table, contents kept" branch: the range table's first room is n / 8 + 64 new segments
        assert int(lines[0][7]) > n // 8 + 64

    # b. the level of every row, through the exact sweep alone
    assert tx["sweep_variant"] == 0 and tx["lds_overflows"] == 0 and tx["redone_queries"] == 0
    assert want["steps"][0] <= tx["candidate_steps"] <= want["steps"][1]
    assert want["fallbacks"][0] <= tx["ring_fallbacks"] <= want["fallbacks"][1]
    if want["undecided"] == 0:
        assert want["steps"][0] == want["steps"][1] and want["fallbacks"][0] == want["fallbacks"][1]

    # c. the hand-overs of the fast sweep
    assert t["sweep_variant"] & 3 == (2 if k + 1 <= te.R1_MAX else 3) and t["sweep_variant"] & 128
    assert t["lds_overflows"] == want["lds_overflows"]
    assert t["redone_queries"] >= want["redone_min"]
    assert t["redone_queries"] - want["redone_min"] <= 2 * EXCESS[name] + 0.005 * n


def test_refused_cube_goes_down_the_chain_of_cell_lists(gpu, tree_env):
    """A cube whose finest cell squared underflows the float32 pre-selection is not built: PCT_KNN_TREE then takes the
    chain of cell lists (include/pct_hip.h, sweep_tree), reports that, and returns the exhaustive sweep's rows."""
    capi = gpu["capi"]
    pts = cloud("refused", gpu["shapes"])
    assert not te.build(pts, 30)["built"]
    tree_env({})
    h = capi.Handle(0)
    try:
        h.set_points(pts)
        h.curvature(30, 0.0, capi.KNN_TREE)
        assert h.timings()["algo"] == capi.KNN_GRID_LEVELS
        it, dt, _ = h.get_neighbors(0, len(pts))
        h.curvature(30, 0.0, capi.KNN_BRUTE)
        ib, db, _ = h.get_neighbors(0, len(pts))
    finally:
        h.close()
    assert np.array_equal(it, ib) and np.array_equal(dt, db)

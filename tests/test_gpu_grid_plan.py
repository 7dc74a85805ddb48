"""The host decisions of the cell-list build (pct_build_grid): where the grid's points come from, the cell-size search,
the restarts, the give-up of PCT_KNN_AUTO.

Both builds and every source return the same rows bit for bit, so a slip of the host half -- another first edge, a pass
more, a stale box that was kept -- shows in the timings only.  The words below were recorded on the MI355X from the
commit BEFORE the build was split into select_source / EdgeSearch / launch_count / launch_place / commit_grid (twice;
every field agreed between the two runs); nothing here recomputes them.  A row is
(grid_iters, cells, cell_size.hex(), grid_points, occupied_cells, occupancy.hex()).  Every case also compares indices,
distances, K and H with a fresh handle's PCT_GRID_ATOMIC=1 run of the same call."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the switches that steer the build: unset unless a step sets one
KNOBS = ("PCT_GRID_ATOMIC", "PCT_NO_CULL", "PCT_NO_SPEC", "PCT_GRID_DEBUG", "PCT_SLAB_MARGIN", "PCT_ITEMS_Q", "PCT_NO_TREE",
         "PCT_NO_AUTO_LEVELS")

ALGOS = ("AUTO", "BRUTE", "GRID", "GRID_EXACT", "GRID_LEVELS", "TREE")          # pct_timings.algo
N, K = 4000, 30
N_SLAB = 5000            # (slab ownership serves clouds of at least 4096 points)
N_AUTO = 20_000          # (PCT_KNN_AUTO probes clouds of at least 16384 points)
SKEW_DECADES = 2.0       # density ~ 1/r^2 over this many decades of r: the parent commit gives the uniform list up on it


def make_clouds(shapes):
    A = shapes.torus_random(N, seed=11)
    rng = np.random.default_rng(5)
    r, a = (4.0 / 3.0) * 10.0 ** (-SKEW_DECADES * rng.uniform(0, 1, N_AUTO)), rng.uniform(0, 2 * np.pi, N_AUTO)
    x, y = r * np.cos(a), r * np.sin(a)
    return {
        "A": A,
        "A2": shapes.torus_random(N, seed=12),
        "B": (2.5 * A + np.float32(4.0)).astype(np.float32),
        "A64": shapes.torus_random(N, seed=11, dtype=np.float64),
        "S": shapes.torus_random(N_SLAB, seed=11),
        "scan": np.stack([x, y, 0.05 * np.sin(x) * np.cos(y)], 1).astype(np.float32),     # the torus' box, another density
        "T": shapes.torus_random(N_AUTO, seed=11),
    }


# A step: (name, cloud, k, eps, algo, shard, knobs); shard = None | ("range", lo, hi) | ("slab", part, parts).
# A scenario: steps that share one handle, in order.
def step(name, cloud="A", k=K, eps=0.0, algo="GRID", shard=None, knobs=()):
    return (name, cloud, k, eps, algo, shard, tuple(knobs))


SCENARIOS = [
    [step("plain")],
    [step("plain_B", cloud="B")],
    [step("atomic", knobs=["PCT_GRID_ATOMIC"])],
    [step("f64", cloud="A64")],
    [step("eps", eps=0.2)],
    [step("k80", k=80)],
    [step("range", shard=("range", 1000, 2000))],
    [step("range_no_cull", shard=("range", 1000, 2000), knobs=["PCT_NO_CULL"])],
    [step("slab", cloud="S", shard=("slab", 1, 3))],
    [step("levels", algo="GRID_LEVELS")],
    # a stream on one handle: packed, speculative, speculative through k_hist_raw / k_scatter_raw, another box
    # (the deferred check restarts the build), the first cloud again
    [step("stream_A"), step("stream_A_again"), step("stream_A2_atomic", cloud="A2", knobs=["PCT_GRID_ATOMIC"]),
     step("stream_B", cloud="B"), step("stream_A_last")],
    [step("warm_A"), step("warm_A_no_spec", knobs=["PCT_NO_SPEC"])],
    # the uniform list of the scan leaves its edge on the handle; AUTO then drops that edge for the scan's own first
    # guess, sees where the search goes and gives up (hierarchical list); the torus that follows drops it as well and
    # gets the uniform list
    [step("auto_scan_grid", cloud="scan"), step("auto_scan", cloud="scan", algo="AUTO"), step("auto_torus", cloud="T", algo="AUTO")],
]

# recorded on the parent commit (see the module docstring); algo of pct_timings where the case is about it
EXPECTED = {
    "plain": (1, 300, "0x1.2cb9435ffee0ap-2", 4000, 352, "0x1.d4a5e353f7ceep+4"),
    "plain_B": (1, 300, "0x1.77e7949f79c90p-1", 4000, 352, "0x1.d4a5e353f7ceep+4"),
    "atomic": (1, 300, "0x1.2cb9435ffee0ap-2", 4000, 352, "0x1.d4a5e353f7ceep+4"),
    "f64": (1, 300, "0x1.2cb9435ffee0ap-2", 4000, 352, "0x1.d4a5e353f7ceep+4"),
    "eps": (1, 784, "0x1.9999b4718c345p-3", 4000, 458, "0x1.af810624dd2f2p+3"),
    "k80": (2, 243, "0x1.544f09c47e3fep-2", 4000, 323, "0x1.4a1999999999ap+5"),
    "range": (1, 300, "0x1.2cb9435ffee0ap-2", 4000, 174, "0x1.d5e76c8b43958p+4"),
    "range_no_cull": (1, 300, "0x1.2cb9435ffee0ap-2", 4000, 174, "0x1.d5e76c8b43958p+4"),
    "slab": (1, 363, "0x1.0cf9b6735a19cp-2", 5000, 141, "0x1.d42b06742b067p+4"),
    "levels": (1, 784, "0x1.85fd88b0d5647p-3", 4000, 68, "0x1.0eda79bef528ep+4"),
    "stream_A": (1, 300, "0x1.2cb9435ffee0ap-2", 4000, 352, "0x1.d4a5e353f7ceep+4"),
    "stream_A_again": (1, 300, "0x1.20b9e519d607bp-2", 4000, 360, "0x1.b326e978d4fdfp+4"),
    "stream_A2_atomic": (1, 300, "0x1.1fadb676c8485p-2", 4000, 354, "0x1.b21cac083126fp+4"),
    "stream_B": (1, 300, "0x1.77e7949f79c90p-1", 4000, 352, "0x1.d4a5e353f7ceep+4"),
    "stream_A_last": (1, 300, "0x1.2cb9435ffee0ap-2", 4000, 352, "0x1.d4a5e353f7ceep+4"),
    "warm_A": (1, 300, "0x1.2cb9435ffee0ap-2", 4000, 352, "0x1.d4a5e353f7ceep+4"),
    "warm_A_no_spec": (1, 300, "0x1.20b9e519d607bp-2", 4000, 360, "0x1.b326e978d4fdfp+4"),
    "auto_scan_grid": (4, 1156896, "0x1.1694cf3ace62fp-7", 20000, 9120, "0x1.b3c63f141205cp+4"),
    # (the one row of the hierarchical list: also DERIVED, by tests/tree_exact.py -- test_tree_exact.py: test_recorded_row_of_the_scan)
    "auto_scan": (1, 1068, "0x1.530afdc2aa400p-20", 20000, 2220, "0x1.2ba01eae807acp+4"),
    "auto_torus": (1, 2646, "0x1.0d2759bd94b65p-3", 20000, 1776, "0x1.b396bb98c7e28p+4"),
}
EXPECTED_ALGO = {"auto_scan": "TREE", "auto_torus": "GRID", "levels": "GRID_LEVELS"}


def _set_env(knobs):
    for v in KNOBS:
        os.environ.pop(v, None)
    for v in knobs:
        os.environ[v] = "1"


def _call(h, capi, clouds, st):
    """One step on handle h; returns (timings, result arrays)."""
    _, cloud, k, eps, algo, shard, _ = st
    pts = clouds[cloud]
    h.set_points(pts)
    lo, hi = 0, len(pts)
    if shard and shard[0] == "range":
        lo, hi = shard[1:]
        h.set_query_range(lo, hi)
    if shard and shard[0] == "slab":
        h.set_query_slab(*shard[1:])
    h.curvature(k, eps, getattr(capi, "KNN_" + algo))
    t = h.timings()
    if shard and shard[0] == "slab":          # (public index, K, H) records in table order: by public index here
        rows = h.slab_counts(shard[2])[shard[1]]
        dev = h.device_alloc(rows * 12)
        try:
            assert h.slab_records(dev, rows) == rows
            rec = np.empty((rows, 3), np.float32)
            h.device_download(dev, rec)
        finally:
            h.device_free(dev)
        rec = rec[np.argsort(rec[:, 0].view(np.int32), kind="stable")]
        return t, (rec[:, 0].view(np.int32), rec[:, 1], rec[:, 2])
    i, d, _ = h.get_neighbors(lo, hi)
    _, Kc, Hc, _ = h.get_fit(lo, hi, coefs=False, H2=False)
    return t, (i, d, Kc, Hc)


def row_of(t):
    return (t["grid_iters"], t["cells"], float(t["cell_size"]).hex(), t["grid_points"], t["occupied_cells"], float(t["occupancy"]).hex())


def run_all(capi, shapes):
    """Every scenario once: {step name: (row, algo, result arrays, the atomic build's arrays)}."""
    saved = {v: os.environ.get(v) for v in KNOBS}
    clouds, out = make_clouds(shapes), {}
    try:
        for scenario in SCENARIOS:
            h = capi.Handle(0)
            try:
                for st in scenario:
                    _set_env(st[6])
                    t, res = _call(h, capi, clouds, st)
                    _set_env(["PCT_GRID_ATOMIC"])
                    ref_h = capi.Handle(0)
                    try:
                        ref = _call(ref_h, capi, clouds, st)[1]
                    finally:
                        ref_h.close()
                    algo = ALGOS[t["algo"]]
                    out[st[0]] = (row_of(t), algo, res, ref)
            finally:
                h.close()
    finally:
        for v, val in saved.items():
            os.environ.pop(v, None)
            if val is not None:
                os.environ[v] = val
    return out


@pytest.fixture(scope="module")
def plans(gpu):
    return run_all(gpu["capi"], gpu["shapes"])


STEPS = [st[0] for scenario in SCENARIOS for st in scenario]


@pytest.mark.parametrize("name", STEPS)
def test_grid_plan(plans, name):
    row, algo, res, ref = plans[name]
    print(name, row, algo)
    assert row == EXPECTED[name], (name, row, EXPECTED[name])
    if name in EXPECTED_ALGO:
        assert algo == EXPECTED_ALGO[name], (name, algo)
    for x, y in zip(res, ref):
        assert np.array_equal(x, y, equal_nan=True), name


def test_rejected_box_leaves_a_plain_build(plans):
    """The restart after the deferred-box check is the packed build of a fresh handle, apart from the first edge (the
    handle's warm start): same box, same points; and the handle goes on speculating afterwards."""
    assert plans["stream_A_again"][0][0] == 1 and plans["stream_A2_atomic"][0][0] == 1      # speculative: one pass
    assert plans["stream_A_last"][2][0].shape == plans["plain"][2][0].shape
    for x, y in zip(plans["stream_A_last"][2], plans["plain"][2]):
        assert np.array_equal(x, y, equal_nan=True)
    for x, y in zip(plans["stream_B"][2], plans["plain_B"][2]):
        assert np.array_equal(x, y, equal_nan=True)
    assert plans["stream_B"][0][3] == plans["plain_B"][0][3] == N

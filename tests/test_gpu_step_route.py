"""The host decisions of a step (run_knn and the fused tail in pct_api.hip, the rules of csrc/pct_auto_route.h): which
algorithm a request resolves to, what PCT_KNN_AUTO remembers from call to call, which sweep serves it, who fits the rows.

Every route returns the same rows bit for bit, so a slip of the host half -- a verdict remembered for the wrong cloud, a
re-examination a call early, a fit launched twice -- shows in the timings only.  Each scenario runs its steps on ONE
handle, in order, and a step leaves a row
(algo, levels, sweep_variant, knn_launches, grid_iters, cells, limit_retries).
The rows below were recorded on the MI355X from the commit BEFORE a call's requests became arguments (the eleven request
and answer flags were still fields of the handle), twice; the two recordings agree in every field of every step, so
every field is compared.  Nothing here recomputes them.  Every step also compares indices, distances, K and H bit for
bit with a fresh handle's PCT_KNN_BRUTE run of the same request; the census clouds (N_CENSUS points) compare 2000
sampled rows, K and H with a fresh handle's PCT_KNN_GRID run.

The census scenario needs a cloud that the uniform list is BUILT for (at most 16 cells per point, or 2^20 cells) and
whose skew then passes its gate: a 1/r^2 scan of 65 536 points over ONE decade of r, k = 40 (over two decades the build
gives up; over half a decade the census says stay).  PCT_GRID_DEBUG=1 on the parent commit:
    [auto] occupancy 27.1, 9998 non-empty cells, skew 4.13
    [auto] census: 65536 queries, 11065 overflow, 30459 short, 9.2 non-empty stencil cells
63 % of the queries would fail, more than max(8 %, 37 500 / N) = 57 %: the hierarchical list; with PCT_NO_TREE more than
30 %: the chain."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KNOBS = ("PCT_NO_TREE", "PCT_NO_AUTO_LEVELS", "PCT_GRID_DEBUG", "PCT_KEEP_DIST", "PCT_NO_PAIR", "PCT_NO_SPEC", "PCT_GRID_ATOMIC",
         "PCT_TREE_EXACT_ONLY", "PCT_NO_CULL")
ALGOS = ("AUTO", "BRUTE", "GRID", "GRID_EXACT", "GRID_LEVELS", "TREE")          # pct_timings.algo
N, K = 4000, 30
N_GRID = 5000            # PCT_KNN_AUTO resolves to the cell list from 4096 points on
N_AUTO = 20_000          # ... and may give the uniform list up from 16384 on
SKEW_DECADES = 2.0       # the scan of test_gpu_grid_plan.py: density ~ 1/r^2 over two decades of r
N_CENSUS = 65_536        # the skew gate opens here
CENSUS_DECADES = 1.0
N_SAMPLE = 2000


def scan_cloud(n, decades, seed):
    """A 1/r^2 scan; its first four points are the corners of one box for every seed (the remembered verdict of
    PCT_KNN_AUTO holds for clouds of the same size whose bounding box agrees within 2 % per face)."""
    rng = np.random.default_rng(seed)
    r, a = (4.0 / 3.0) * 10.0 ** (-decades * rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
    x, y = r * np.cos(a), r * np.sin(a)
    pts = np.stack([x, y, 0.05 * np.sin(x) * np.cos(y)], 1).astype(np.float32)
    e = np.float32(4.0 / 3.0)
    pts[:4] = [(-e, -e, -0.05), (e, e, 0.05), (-e, e, 0.05), (e, -e, -0.05)]
    return pts


def make_clouds(shapes):
    A = shapes.torus_random(N, seed=11)
    nan_row = A.copy()
    nan_row[1234, 1] = np.nan
    return {
        "A": A,
        "A_tiny": A * np.float32(1e-20),            # f32_tiny of test_gpu_sweep_dispatch.py: no cloud for the float32 pre-selection
        "A_nan": nan_row,
        "G": shapes.torus_random(N_GRID, seed=11),
        "scan": scan_cloud(N_AUTO, SKEW_DECADES, 5),
        "scan2": scan_cloud(N_AUTO, SKEW_DECADES, 2),
        "T": shapes.torus_random(N_AUTO, seed=11),
        "census": scan_cloud(N_CENSUS, CENSUS_DECADES, 5),
        "census_T": shapes.torus_random(N_CENSUS, seed=11),
    }


# A step: (name, cloud, k, algo, fused, query range or None, knobs).  A scenario: steps that share one handle, in order.
def step(name, cloud="A", k=K, algo="GRID", fused=True, shard=None, knobs=()):
    return (name, cloud, k, algo, fused, shard, tuple(knobs))


SCENARIOS = (
    [[step(f"fused_{a}", algo=a)] for a in ALGOS] + [[step(f"stepwise_{a}", algo=a, fused=False)] for a in ALGOS] + [
        [step("auto_5000", cloud="G", algo="AUTO")],
        [step("auto_k128", cloud="G", k=128, algo="AUTO")],
        [step("auto_small_k128", k=128, algo="AUTO")],          # (below 4096 points AUTO is the exhaustive sweep, which takes any k)
        [step("brute_k200", k=200, algo="BRUTE")],
        [step("tree_range", algo="TREE", shard=(1000, 2000))],
        [step("tree_tiny", cloud="A_tiny", algo="TREE")],
        # the uniform list given up, the hierarchical one taken and remembered; a cloud of the same box goes there directly;
        # another box is examined afresh (and forgotten), twice; the scan again
        [step("seq_scan", cloud="scan", algo="AUTO"), step("seq_scan2", cloud="scan2", algo="AUTO"), step("seq_T", cloud="T", algo="AUTO"),
         step("seq_T_again", cloud="T", algo="AUTO"), step("seq_scan_last", cloud="scan", algo="AUTO")],
        # the remembered verdict is re-examined on every 16th call
        [step(f"cadence_{i:02d}", cloud="scan", algo="AUTO") for i in range(1, 19)],
        # a uniform list built, its skew past the gate, the census: hierarchical list | chain of cell lists | stay
        [step("census_tree", cloud="census", k=40, algo="AUTO")],
        [step("census_levels", cloud="census", k=40, algo="AUTO", knobs=["PCT_NO_TREE"])],
        [step("census_torus", cloud="census_T", k=40, algo="AUTO")],
    ])
ASYNC_ALGOS = ("GRID", "GRID_LEVELS", "GRID", "GRID_LEVELS", "GRID", "GRID_LEVELS")

# recorded on the parent commit (see the module docstring)
EXPECTED = {'fused_AUTO': ('BRUTE', 0, 0, 1, 0, 0, 0),
 'fused_BRUTE': ('BRUTE', 0, 0, 1, 0, 0, 0),
 'fused_GRID': ('GRID', 0, 50, 1, 1, 300, 0),
 'fused_GRID_EXACT': ('GRID_EXACT', 0, 0, 1, 1, 300, 0),
 'fused_GRID_LEVELS': ('GRID_LEVELS', 2, 305, 2, 1, 784, 0),
 'fused_TREE': ('TREE', 0, 178, 1, 1, 236, 0),
 'stepwise_AUTO': ('BRUTE', 0, 0, 1, 0, 0, 0),
 'stepwise_BRUTE': ('BRUTE', 0, 0, 1, 0, 0, 0),
 'stepwise_GRID': ('GRID', 0, 306, 1, 1, 300, 0),
 'stepwise_GRID_EXACT': ('GRID_EXACT', 0, 0, 1, 1, 300, 0),
 'stepwise_GRID_LEVELS': ('GRID_LEVELS', 2, 305, 2, 1, 784, 0),
 'stepwise_TREE': ('TREE', 0, 434, 1, 1, 236, 0),
 'auto_5000': ('GRID', 0, 50, 1, 1, 363, 0),
 'auto_k128': ('GRID_EXACT', 0, 0, 1, 2, 243, 0),
 'auto_small_k128': ('BRUTE', 0, 0, 1, 0, 0, 0),
 'brute_k200': ('BRUTE', 0, 0, 1, 0, 0, 0),
 'tree_range': ('GRID_LEVELS', 2, 305, 2, 1, 784, 0),
 'tree_tiny': ('GRID_LEVELS', 2, 257, 2, 1, 784, 0),
 'seq_scan': ('TREE', 0, 178, 1, 1, 1053, 0),
 'seq_scan2': ('TREE', 0, 178, 1, 1, 1040, 0),
 'seq_T': ('GRID', 0, 50, 1, 1, 2646, 0),
 'seq_T_again': ('GRID', 0, 50, 1, 1, 2646, 0),
 'seq_scan_last': ('TREE', 0, 178, 1, 1, 1053, 0),
 'cadence_01': ('TREE', 0, 178, 1, 1, 1053, 0),
 'cadence_02': ('TREE', 0, 178, 1, 1, 1053, 0),
 'cadence_03': ('TREE', 0, 178, 1, 1, 1053, 0),
 'cadence_04': ('TREE', 0, 178, 1, 1, 1053, 0),
 'cadence_05': ('TREE', 0, 178, 1, 1, 1053, 0),
 'cadence_06': ('TREE', 0, 178, 1, 1, 1053, 0),
 'cadence_07': ('TREE', 0, 178, 1, 1, 1053, 0),
 'cadence_08': ('TREE', 0, 178, 1, 1, 1053, 0),
 'cadence_09': ('TREE', 0, 178, 1, 1, 1053, 0),
 'cadence_10': ('TREE', 0, 178, 1, 1, 1053, 0),
 'cadence_11': ('TREE', 0, 178, 1, 1, 1053, 0),
 'cadence_12': ('TREE', 0, 178, 1, 1, 1053, 0),
 'cadence_13': ('TREE', 0, 178, 1, 1, 1053, 0),
 'cadence_14': ('TREE', 0, 178, 1, 1, 1053, 0),
 'cadence_15': ('TREE', 0, 178, 1, 1, 1053, 0),
 'cadence_16': ('TREE', 0, 178, 1, 1, 1053, 0),
 'cadence_17': ('TREE', 0, 178, 1, 1, 1053, 0),
 'cadence_18': ('TREE', 0, 178, 1, 1, 1053, 0),
 'census_tree': ('TREE', 0, 178, 1, 1, 2643, 0),
 'census_levels': ('GRID_LEVELS', 7, 305, 7, 1, 17787, 0),
 'census_torus': ('GRID', 0, 50, 1, 1, 13690, 0)}


def _set_env(knobs):
    for v in KNOBS:
        os.environ.pop(v, None)
    for v in knobs:
        os.environ[v] = "1"


def row_of(t):
    return (ALGOS[t["algo"]], t["levels"], t["sweep_variant"], t["knn_launches"], t["grid_iters"], t["cells"], t["limit_retries"])


def _sampled(cloud):
    return cloud.startswith("census")


def _results(h, cloud, n, shard):
    lo, hi = shard or (0, n)
    if _sampled(cloud):
        i, d, _ = h.get_neighbor_rows(np.random.default_rng(3).choice(n, N_SAMPLE, replace=False))
    else:
        i, d, _ = h.get_neighbors(lo, hi)
    _, Kc, Hc, _ = h.get_fit(lo, hi, coefs=False, H2=False)
    return i, d, Kc, Hc


def _call(h, capi, clouds, st, algo=None):
    """One step on handle h; returns (timings, result arrays)."""
    _, cloud, k, requested, fused, shard, _ = st
    pts = clouds[cloud]
    h.set_points(pts)
    if shard:
        h.set_query_range(*shard)
    which = getattr(capi, "KNN_" + (algo or requested))
    if fused:
        h.curvature(k, 0.0, which)
    else:
        h.knn(k, 0.0, which)
        h.fit()
    return h.timings(), _results(h, cloud, len(pts), shard)


def run_all(capi, shapes):
    """Every scenario once: {step name: (row, fit_svd_rows, result arrays, the reference's arrays)}."""
    saved = {v: os.environ.get(v) for v in KNOBS}
    clouds, out, refs = make_clouds(shapes), {}, {}
    try:
        for scenario in SCENARIOS:
            h = capi.Handle(0)
            try:
                for st in scenario:
                    _set_env(st[6])
                    t, res = _call(h, capi, clouds, st)
                    key = (st[1], st[2], st[5])
                    if key not in refs:                  # computed once, shared by the steps of the same request
                        _set_env(())
                        ref_h = capi.Handle(0)
                        try:
                            refs[key] = _call(ref_h, capi, clouds, st[:4] + (True,) + st[5:], algo="GRID" if _sampled(st[1]) else "BRUTE")[1]
                        finally:
                            ref_h.close()
                    out[st[0]] = (row_of(t), t["fit_svd_rows"], res, refs[key])
            finally:
                h.close()
    finally:
        for v, val in saved.items():
            os.environ.pop(v, None)
            if val is not None:
                os.environ[v] = val
    return out


def run_stream(capi, shapes, asynchronous):
    """ASYNC_ALGOS back to back on one handle and one cloud: (the row and fit_svd_rows of every call, K and H of the last)."""
    saved = {v: os.environ.get(v) for v in KNOBS}
    _set_env(())
    h = capi.Handle(0)
    try:
        h.set_points(shapes.torus_random(N, seed=11))
        h.set_async(asynchronous)
        rows = []
        for i, a in enumerate(ASYNC_ALGOS):
            h.curvature(K, 0.0, getattr(capi, "KNN_" + a))
            if not asynchronous or i >= 1:               # asynchronous: the call before the pending one
                t = h.stage_times_done().as_dict()
                rows.append((row_of(t), t["fit_svd_rows"]))
        if asynchronous:
            h.synchronize()
            t = h.timings()
            rows.append((row_of(t), t["fit_svd_rows"]))
        _, Kc, Hc, _ = h.get_fit(0, N, coefs=False, H2=False)
        i, d, _ = h.get_neighbors(0, N)
        return rows, (i, d, Kc, Hc)
    finally:
        h.close()
        for v, val in saved.items():
            os.environ.pop(v, None)
            if val is not None:
                os.environ[v] = val


@pytest.fixture(scope="module")
def routes(gpu):
    return run_all(gpu["capi"], gpu["shapes"])


STEPS = [st[0] for scenario in SCENARIOS for st in scenario]


@pytest.mark.parametrize("name", STEPS)
def test_step_route(routes, name):
    row, _, res, ref = routes[name]
    print(name, row)
    assert row == EXPECTED[name], (name, row, EXPECTED[name])
    for x, y in zip(res, ref):
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), name


def test_requests_resolve_as_documented(routes):
    """What the recorded rows say, in words (include/pct_hip.h)."""
    algo = lambda name: routes[name][0][0]
    for a in ALGOS:
        for mode in ("fused", "stepwise"):
            assert algo(f"{mode}_{a}") == ("BRUTE" if a == "AUTO" else a), (mode, a)
    assert algo("auto_5000") == "GRID" and algo("auto_k128") == "GRID_EXACT" and algo("auto_small_k128") == "BRUTE" and algo("brute_k200") == "BRUTE"
    assert algo("tree_range") == "GRID_LEVELS" and algo("tree_tiny") == "GRID_LEVELS"
    assert [algo(s) for s in ("seq_scan", "seq_scan2", "seq_T", "seq_T_again", "seq_scan_last")] == ["TREE", "TREE", "GRID", "GRID", "TREE"]
    assert all(algo(f"cadence_{i:02d}") == "TREE" for i in range(1, 19))
    assert algo("census_tree") == "TREE" and routes["census_tree"][0][4] >= 1          # (a uniform list was built first)
    assert algo("census_levels") == "GRID_LEVELS" and algo("census_torus") == "GRID"


def test_passes_of_a_fused_chained_sweep_fit_their_rows(routes):
    """The fused call's passes fit the rows they answer; the stepwise call fits the merged table: the same rows go to the
    SVD either way (and K and H are the exhaustive sweep's, test_step_route)."""
    assert routes["fused_GRID_LEVELS"][1] == routes["stepwise_GRID_LEVELS"][1]
    assert routes["fused_GRID_LEVELS"][0][1] >= 1


def test_asynchronous_steps_take_the_blocking_routes(gpu):
    """pct_set_async, uniform list and chained sweep in turn: both parities of the pinned slots, statistics words mirrored
    by the fit kernel (uniform list) and copied (the passes fitted the rows: no fit kernel behind the sweep)."""
    blocking, res0 = run_stream(gpu["capi"], gpu["shapes"], False)
    streamed, res1 = run_stream(gpu["capi"], gpu["shapes"], True)
    print(blocking, streamed)
    assert len(blocking) == len(streamed) == len(ASYNC_ALGOS)
    assert streamed == blocking
    assert [r[0][0] for r in blocking] == list(ASYNC_ALGOS)
    for x, y in zip(res1, res0):
        assert np.array_equal(x, y, equal_nan=True)


def test_failed_call_leaves_nothing_behind(gpu):
    """A fused call that fails (a non-finite coordinate) leaves no request behind: the sweep and the fit that follow on
    the handle report the timings, statistics and values of a fresh handle's."""
    capi, clouds = gpu["capi"], make_clouds(gpu["shapes"])
    saved = {v: os.environ.get(v) for v in KNOBS}
    _set_env(())
    h, fresh = capi.Handle(0), capi.Handle(0)
    try:
        h.set_stats(True)
        fresh.set_stats(True)
        h.set_points(clouds["A_nan"])
        with pytest.raises(ValueError, match="Non-finite"):
            h.curvature(K, 0.0, capi.KNN_AUTO)
        got = []
        for x in (h, fresh):
            x.set_points(clouds["A"])
            x.knn(K, 0.0, capi.KNN_GRID)
            x.fit()
            t = x.timings()
            got.append(({f: v for f, v in t.items() if not f.endswith("_ms")}, _results(x, "A", N, None)))
        print(got[0][0], got[1][0])
        assert got[0][0] == got[1][0]
        assert got[0][0]["redone_queries"] > 0                    # (statistics were collected)
        for x, y in zip(got[0][1], got[1][1]):
            assert np.array_equal(x, y, equal_nan=True)
    finally:
        h.close()
        fresh.close()
        for v, val in saved.items():
            os.environ.pop(v, None)
            if val is not None:
                os.environ[v] = val

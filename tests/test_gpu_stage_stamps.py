"""Stage times from device clock stamps (csrc/pct_stamp.h): an explicit PCT_KNN_GRID / PCT_KNN_GRID_EXACT call records no
timing event; the first kernel of every stage stamps the device's wall clock and the step's last kernel stamps its end.

What a wrong clock rate, counters that differ between the dies, a stamp missed behind an early return or a stamp block
read for the wrong call would break is the BRACKET: every stage time is positive, the stages add up to the total, and the
total -- device time between the first kernel's entry and the last kernel's end -- cannot exceed the host's wall time
around the call that enqueued those kernels and waited for them.  Nothing here compares against a recorded time.

The first call on a fresh handle packs the cloud first (k_pack takes the begin stamp); the second call on the same cloud
builds from the caller's rows (k_bin_count takes it).  Every bracket below is checked on both."""
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 50
REL = 2.0 ** -22    # the stages add up exactly in ticks; each of the four float32 values is within 2^-24 of its own


def _without_event_switch():
    saved = os.environ.pop("PCT_TIME_EVENTS", None)
    return saved


def _restore(saved):
    os.environ.pop("PCT_TIME_EVENTS", None)
    if saved is not None:
        os.environ["PCT_TIME_EVENTS"] = saved


def bracket(t, wall_ms, what, fast=True):
    print(what, {f: t[f] for f in ("grid_ms", "knn_ms", "knn_fast_ms", "fit_ms", "total_ms")}, "wall %.4f" % wall_ms)
    assert t["grid_ms"] > 0 and t["knn_ms"] > 0 and t["fit_ms"] > 0, what
    if fast:
        assert 0 < t["knn_fast_ms"] <= t["knn_ms"], what
    else:
        assert t["knn_fast_ms"] == 0, what
    s = t["grid_ms"] + t["knn_ms"] + t["fit_ms"]
    assert abs(s - t["total_ms"]) <= REL * t["total_ms"], what
    assert t["total_ms"] <= wall_ms, what


def stages(t, what):
    """The part of the bracket that needs no wall time of the single call: every stage positive, the stages add up."""
    assert t["grid_ms"] > 0 and t["knn_ms"] > 0 and t["fit_ms"] > 0 and 0 < t["knn_fast_ms"] <= t["knn_ms"], what
    assert abs(t["grid_ms"] + t["knn_ms"] + t["fit_ms"] - t["total_ms"]) <= REL * t["total_ms"], what


def fused_twice(capi, pts, k, algo=None, fast=True, what=""):
    """Two blocking fused calls on one handle (pack pass first | caller's rows), each inside its bracket; the last timings."""
    h = capi.Handle(0)
    try:
        h.set_points(pts)
        t = None
        for call in ("first", "second"):
            t0 = time.perf_counter()
            h.curvature(k, 0.0, capi.KNN_GRID if algo is None else algo)
            wall = 1e3 * (time.perf_counter() - t0)
            t = h.timings()
            bracket(t, wall, f"{what} {call}", fast)
        return t
    finally:
        h.close()


@pytest.fixture(scope="module")
def torus(gpu):
    return gpu["shapes"].torus_random(20_000, seed=3)


def stepwise_twice(capi, pts, k, algo, fast=True):
    """Two sweeps on their own, each followed by its fit, on one handle: the sweep's call ends where the sweep does."""
    h = capi.Handle(0)
    try:
        h.set_points(pts)
        for call in ("first", "second"):
            t0 = time.perf_counter()
            h.knn(k, 0.0, algo)
            t = h.timings()
            h.fit()
            wall = 1e3 * (time.perf_counter() - t0)
            f = h.timings()
            print("stepwise", call, t["grid_ms"], t["knn_ms"], t["knn_fast_ms"], t["total_ms"], f["fit_ms"], "wall %.4f" % wall)
            assert t["grid_ms"] > 0 and t["knn_ms"] > 0 and f["fit_ms"] > 0
            if fast:
                assert 0 < t["knn_fast_ms"] <= t["knn_ms"]
            else:
                assert t["knn_fast_ms"] == 0
            assert t["fit_ms"] == 0
            assert abs(t["grid_ms"] + t["knn_ms"] - t["total_ms"]) <= REL * t["total_ms"]
            assert t["total_ms"] + f["fit_ms"] <= wall
    finally:
        h.close()


def test_bracket_fused_and_stepwise(gpu, torus):
    capi = gpu["capi"]
    saved = _without_event_switch()
    try:
        fused_twice(capi, torus, K, what="fused")
        stepwise_twice(capi, torus, K, capi.KNN_GRID)
    finally:
        _restore(saved)


@pytest.mark.parametrize("route", ["grid", "brute"])
def test_sweep_on_its_own_under_events(gpu, torus, route):
    """PCT_TIME_EVENTS=1: the sweep's call ends at its sweep-end event -- fit_ms = 0, grid + knn = total; the exhaustive
    sweep (2 000 points) has no fast sweep."""
    capi = gpu["capi"]
    saved = _without_event_switch()
    os.environ["PCT_TIME_EVENTS"] = "1"
    try:
        if route == "grid":
            stepwise_twice(capi, torus, K, capi.KNN_GRID)
        else:
            stepwise_twice(capi, gpu["shapes"].torus_random(2000, seed=6), K, capi.KNN_BRUTE, fast=False)
    finally:
        _restore(saved)


def test_same_bits_under_both_sources(gpu, torus):
    capi = gpu["capi"]
    saved = _without_event_switch()
    got = []
    try:
        for events in (False, True):
            if events:
                os.environ["PCT_TIME_EVENTS"] = "1"
            h = capi.Handle(0)
            try:
                h.set_points(torus)
                for _ in range(2):
                    t0 = time.perf_counter()
                    h.curvature(K, 0.0, capi.KNN_GRID)
                    wall = 1e3 * (time.perf_counter() - t0)
                    bracket(h.timings(), wall, "events" if events else "stamps")
                idx, dist, _ = h.get_neighbors(0, len(torus))
                _, Kc, Hc, _ = h.get_fit(0, len(torus), coefs=False, H2=False)
                got.append((idx, dist, Kc, Hc))
            finally:
                h.close()
    finally:
        _restore(saved)
    for x, y in zip(*got):
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True)


def _coincident(shapes):
    """700 copies of the corner of the cloud's box -- cell 0 of any grid over it, the first work item of the sweep -- among
    4 000 points: the item's stencil overflows the 512 staged slots and the item leaves through the hand-over to the exact
    sweep, in front of the sweep's loop."""
    pts = shapes.torus_random(4000, seed=9)
    pts[:700] = pts.min(axis=0)
    return pts


EDGES = {
    # name: (cloud, k, a fast sweep runs)
    "single_block": (lambda s: s.torus_random(70, seed=4), 5, True),
    "duo_k80": (lambda s: s.torus_random(20_000, seed=3), 80, True),
    "float64": (lambda s: s.torus_random(20_000, seed=3).astype(np.float64) * (1.0 + 1e-9), K, True),
    "no_fast_k130": (lambda s: s.torus_random(2000, seed=6), 130, False),
    "overflow_item0": (_coincident, K, True),
}


@pytest.mark.parametrize("name", sorted(EDGES))
def test_edges_of_the_stamp_writers(gpu, name):
    capi = gpu["capi"]
    make, k, fast = EDGES[name]
    saved = _without_event_switch()
    try:
        t = fused_twice(capi, make(gpu["shapes"]), k, fast=fast, what=name)
        if name == "duo_k80":
            assert t["sweep_variant"] & 3 == 3              # pct_timings.sweep_variant: the family in the low bits, 3 = k_knn_duo
        if name == "float64":
            assert t["sweep_variant"] & 64                   # ... bit 6: float64 queries
        if name == "no_fast_k130":
            assert t["algo"] == capi.KNN_GRID_EXACT and t["sweep_variant"] == 0
    finally:
        _restore(saved)


def test_overflowing_first_item_is_handed_over(gpu):
    """The cloud of "overflow_item0" does what its docstring says (statistics on: same kernels, counted)."""
    capi = gpu["capi"]
    h = capi.Handle(0)
    try:
        h.set_points(_coincident(gpu["shapes"]))
        h.set_stats(True)
        h.curvature(K, 0.0, capi.KNN_GRID)
        t = h.timings()
        print(t["lds_overflows"], t["redone_queries"])
        assert t["lds_overflows"] >= 1 and t["redone_queries"] >= 700
    finally:
        h.close()


def test_every_row_through_the_svd_kernel(gpu):
    """3 000 collinear points: k_fit hands every row to k_fit_svd, whose last block out stamps the end: fit_ms covers it."""
    capi = gpu["capi"]
    rng = np.random.default_rng(8)
    pts = np.zeros((3000, 3), np.float32)
    pts[:, 0] = np.sort(rng.uniform(0, 1, 3000)).astype(np.float32)
    saved = _without_event_switch()
    try:
        t = fused_twice(capi, pts, 10, what="collinear")
        assert t["fit_svd_rows"] == 3000
    finally:
        _restore(saved)


def test_async_parity(gpu):
    capi, shapes = gpu["capi"], gpu["shapes"]
    clouds = [shapes.torus_random(4096, seed=1), shapes.torus_random(500_000, seed=2)]
    saved = _without_event_switch()
    h = capi.Handle(0)
    try:
        h.set_async(True)
        totals, sizes = [], []
        t0 = time.perf_counter()
        for i in range(8):
            pts = clouds[i & 1]
            h.set_points(pts)
            h.curvature(K, 0.0, capi.KNN_GRID)
            if i >= 1:
                t = h.stage_times_done().as_dict()
                assert t["grid_points"] == len(clouds[(i - 1) & 1]), i
                stages(t, i - 1)
                totals.append(t["total_ms"])
                sizes.append(t["grid_points"])
        h.synchronize()
        wall = 1e3 * (time.perf_counter() - t0)
        t = h.timings()
        assert t["grid_points"] == len(clouds[1])
        stages(t, 7)
        totals.append(t["total_ms"])
        sizes.append(t["grid_points"])
        print(totals, "wall %.3f" % wall)
        assert all(x > 0 for x in totals)
        for j in range(8):
            if sizes[j] == len(clouds[1]):
                for nb in (j - 1, j + 1):
                    if 0 <= nb < 8:
                        assert totals[j] > totals[nb], (j, nb)
        assert sum(totals) <= wall

        # one cloud, call after call with nothing in between: the calls alternate between the two stamp blocks
        h.set_points(clouds[1])
        h.synchronize()
        t0 = time.perf_counter()
        seen = []
        for i in range(6):
            h.curvature(K, 0.0, capi.KNN_GRID)
            if i >= 1:
                seen.append(h.stage_times_done().as_dict())
        h.synchronize()
        wall = 1e3 * (time.perf_counter() - t0)
        seen.append(h.timings())
        print([s["total_ms"] for s in seen], "wall %.3f" % wall)
        for j, s in enumerate(seen):
            stages(s, j)
        assert sum(s["total_ms"] for s in seen) <= wall
    finally:
        h.close()
        _restore(saved)


def test_other_routes_keep_their_events(gpu):
    """PCT_KNN_AUTO on a 1/r^2 scan (the cloud of bench.py's secondary_uneven, 50 000 points): the route is open until the
    uniform list has been examined, so the call is timed by events as before."""
    capi = gpu["capi"]
    rng = np.random.default_rng(5)
    n = 1_000_000
    r, a = 0.01 * 100 ** rng.uniform(0, 1, n), rng.uniform(0, 2 * np.pi, n)
    x, y = r * np.cos(a), r * np.sin(a)
    pts = np.ascontiguousarray(np.stack([x, y, 0.05 * np.sin(x) * np.cos(y)], 1), dtype=np.float32)[:50_000]
    h = capi.Handle(0)
    try:
        h.set_points(pts)
        for _ in range(2):
            h.curvature(K, 0.0, capi.KNN_AUTO)
            t = h.timings()
            print(t["algo"], t["grid_ms"], t["knn_ms"], t["fit_ms"], t["total_ms"])
            assert t["grid_ms"] > 0 and t["knn_ms"] > 0 and t["fit_ms"] > 0
    finally:
        h.close()


def _owned_fit_bits(capi, pts, begin, end, events, what, env=None):
    """Two fused PCT_KNN_GRID calls on a handle that owns rows [begin, end), each inside its bracket, with the stamps or
    (events) with PCT_TIME_EVENTS=1; the fit of the owned rows."""
    saved = _without_event_switch()
    saved_env = {name: os.environ.pop(name, None) for name in (env or {})}
    try:
        os.environ.update(env or {})
        if events:
            os.environ["PCT_TIME_EVENTS"] = "1"
        h = capi.Handle(0)
        try:
            h.set_points(pts)
            if (begin, end) != (0, len(pts)):
                h.set_query_range(begin, end)
            for call in ("first", "second"):
                t0 = time.perf_counter()
                h.curvature(K, 0.0, capi.KNN_GRID)
                wall = 1e3 * (time.perf_counter() - t0)
                bracket(h.timings(), wall, f"{what} {'events' if events else 'stamps'} {call}")
            return h.get_fit(begin, end)
        finally:
            h.close()
    finally:
        for name, value in saved_env.items():
            os.environ.pop(name, None)
            if value is not None:
                os.environ[name] = value
        _restore(saved)


def test_begin_falls_back_behind_a_cull_pass(gpu, torus):
    """A handle that owns the first quarter of a float32 cloud: its build starts with the cull pass, which takes no stamp,
    so the call that opened on stamps marks its begin with an event and goes on with events."""
    capi = gpu["capi"]
    got = [_owned_fit_bits(capi, torus, 0, len(torus) // 4, events, "cull") for events in (False, True)]
    for x, y in zip(*got):
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True)


def test_begin_falls_back_behind_a_clearing_fill(gpu, torus):
    """PCT_GRID_ATOMIC=1: the second call builds from the caller's rows with per-point atomics, so its first launch is a
    clearing fill (the first call's is k_pack, which takes the begin stamp)."""
    _owned_fit_bits(gpu["capi"], torus, 0, len(torus), False, "atomic build", env={"PCT_GRID_ATOMIC": "1"})


@pytest.mark.parametrize("route", ["tree", "levels", "brute"])
def test_routes_that_never_take_stamps(gpu, torus, route):
    """The hierarchical list, the chained sweep (which fits inside its passes: its fit stage may be empty) and the
    exhaustive sweep (2 000 points, no fast sweep) are timed by events whatever was asked."""
    capi = gpu["capi"]
    algo = {"tree": capi.KNN_TREE, "levels": capi.KNN_GRID_LEVELS, "brute": capi.KNN_BRUTE}[route]
    pts = gpu["shapes"].torus_random(2000, seed=6) if route == "brute" else torus
    saved = _without_event_switch()
    h = capi.Handle(0)
    try:
        h.set_points(pts)
        for call in ("first", "second"):
            t0 = time.perf_counter()
            h.curvature(K, 0.0, algo)
            wall = 1e3 * (time.perf_counter() - t0)
            t = h.timings()
            print(route, call, {f: t[f] for f in ("algo", "grid_ms", "knn_ms", "knn_fast_ms", "fit_ms", "total_ms")}, "wall %.4f" % wall)
            assert t["grid_ms"] > 0 and t["knn_ms"] > 0 and t["fit_ms"] >= 0
            assert abs(t["grid_ms"] + t["knn_ms"] + t["fit_ms"] - t["total_ms"]) <= REL * t["total_ms"]
            assert t["total_ms"] <= wall
            if route == "brute":
                assert t["knn_fast_ms"] == 0
            elif route == "tree":       # (the chained sweep's table is in public space: no knn_fast_ms is reported for it)
                assert 0 < t["knn_fast_ms"] <= t["knn_ms"]
    finally:
        h.close()
        _restore(saved)


K_MAX = 511     # PCT_K_MAX (csrc/pct_internal.h)


def test_refused_call_behind_a_pending_one(gpu, torus):
    """Async mode: a call the library refuses before it enqueues anything (k out of range) finds nothing to undo: the
    record on the handle is still the good call's and the handle goes on as a blocking one's would.  (The stage fields of
    that record are not checked: after a refusal the handle reports its current record, whose times are the last drained
    call's -- none on this handle.)"""
    capi = gpu["capi"]
    saved = _without_event_switch()
    h, ref = capi.Handle(0), capi.Handle(0)
    try:
        ref.set_points(torus)
        ref.curvature(K, 0.0, capi.KNN_GRID)
        want = ref.get_fit(0, len(torus))
        h.set_async(True)
        h.set_points(torus)
        h.curvature(K, 0.0, capi.KNN_GRID)
        with pytest.raises(ValueError):
            h.curvature(K_MAX + 1, 0.0, capi.KNN_GRID)
        t = h.stage_times_done().as_dict()
        print({f: t[f] for f in ("grid_points", "grid_ms", "knn_ms", "knn_fast_ms", "fit_ms", "total_ms")})
        assert t["grid_points"] == len(torus)
        h.curvature(K, 0.0, capi.KNN_GRID)
        h.synchronize()
        for x, y in zip(h.get_fit(0, len(torus)), want):
            assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True)
    finally:
        h.close()
        ref.close()
        _restore(saved)

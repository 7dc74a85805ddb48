"""The passes of the chained sweep (pct_knn_levels), one by one.

The routes of test_gpu_step_route.py and the `levels` row of test_gpu_grid_plan.py see the LAST build of a chained call
and the number of its passes.  What one pass asks of the cell-list build and of the sweep -- the band of wanted edges it
owns, the sub-box of its points, the edge it is given, the base records of the first pass and that pass's box -- shows
only in the passes in between.  Here they are pinned: with PCT_GRID_DEBUG=1 and PCT_LEVELS_DEBUG=1 every call writes

    [grid] pass i: n .. owned .. edge .. dims .. = .. cells (.. scan tiles), box [..]-[..]      every pass of every build
    [grid] box [..]-[..] edge .. dims .. = .. cells, .. passes, occupancy .., items ..          every accepted build
    [levels] after pass p (edge .., .. cells): pending .. (exact-only ..), best octave ..       between the chain's passes

to stderr.  These lines, whole and in order, were recorded on the MI355X from the commit BEFORE the passes' requests
became an argument (LevelPass) -- twice, in two processes; the two recordings agreed in every character, so no field is
left out -- and are kept in tests/golden/levels_passes.json.  Nothing here recomputes them; they are compared as text.
The `[levels] pass p: .. ms` lines carry wall times and the `[grid] bin build` lines are not about the passes: dropped.

Every call also compares indices, distances, counts, K and H bit for bit with a fresh handle's PCT_KNN_BRUTE run of the
same request; the census scan compares 2000 sampled rows (and K and H of every row) with a fresh handle's PCT_KNN_GRID
run, as test_gpu_step_route.py does."""
import json
import os

import numpy as np
import pytest

from test_gpu_step_route import CENSUS_DECADES, N_CENSUS, N_SAMPLE, scan_cloud

pytestmark = pytest.mark.gpu

RECORDED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "levels_passes.json")
KNOBS = ("PCT_GRID_DEBUG", "PCT_LEVELS_DEBUG", "PCT_GRID_ATOMIC", "PCT_NO_CULL", "PCT_NO_SPEC", "PCT_NO_TREE", "PCT_NO_AUTO_LEVELS",
         "PCT_ITEMS_Q", "PCT_KEEP_DIST", "PCT_NO_PAIR")
KEPT = ("[grid] pass ", "[grid] box ", "[levels] after pass ")
N, K = 4000, 30


def make_cloud(name, shapes):
    if name == "A":
        return shapes.torus_random(N, seed=11)
    if name == "A64":
        return shapes.torus_random(N, seed=11, dtype=np.float64)
    assert name == "census"
    return scan_cloud(N_CENSUS, CENSUS_DECADES, 5)


# A call: (cloud, k, eps, algo, query range or None).  A case: calls that share one handle, in order.
def call(cloud="A", k=K, eps=0.0, algo="GRID_LEVELS", shard=None):
    return (cloud, k, eps, algo, shard)


CASES = {
    "torus": [call()],                                      # two passes, the leftovers to the exact sweep
    "census": [call(cloud="census", k=40)],                 # banded passes on a sub-box, built from the base records (k_hist_agg)
    "range": [call(shard=(1000, 2000))],                    # a sharded first pass, no_cull
    "f64": [call(cloud="A64")],                             # sorted4d rides along
    "eps": [call(eps=0.2)],                                 # counts merged through pub_cnt
    # what the plain build after a chained call finds on the handle: warm start, no speculation record from the chain
    "grid_levels_grid": [call(algo="GRID"), call(), call(algo="GRID")],
}


def kept_lines(err):
    return [ln for ln in err.splitlines() if ln.startswith(KEPT)]


def _results(h, c, n):
    cloud, _, _, _, shard = c
    lo, hi = shard or (0, n)
    if cloud == "census":
        i, d, cnt = h.get_neighbor_rows(np.random.default_rng(3).choice(n, N_SAMPLE, replace=False))
    else:
        i, d, cnt = h.get_neighbors(lo, hi, want_count=True)
    _, Kc, Hc, _ = h.get_fit(lo, hi, coefs=False, H2=False)
    return i, d, cnt, Kc, Hc


def _run(h, capi, pts, c, algo):
    _, k, eps, _, shard = c
    h.set_points(pts)
    if shard:
        h.set_query_range(*shard)
    h.curvature(k, eps, getattr(capi, "KNN_" + algo))
    return _results(h, c, len(pts))


def run_case(capi, shapes, name, read_err):
    """The calls of one case on one handle: [(kept lines, result arrays, the reference's arrays)].  read_err() returns
    what the process has written to stderr since it was last called."""
    saved = {v: os.environ.get(v) for v in KNOBS}
    out, refs = [], {}
    h = capi.Handle(0)
    try:
        for c in CASES[name]:
            pts = make_cloud(c[0], shapes)
            for v in KNOBS:
                os.environ.pop(v, None)
            os.environ["PCT_GRID_DEBUG"] = os.environ["PCT_LEVELS_DEBUG"] = "1"
            read_err()
            res = _run(h, capi, pts, c, c[3])
            lines = kept_lines(read_err())
            key = c[:3] + c[4:]
            if key not in refs:                              # computed once, shared by the calls of the same request
                del os.environ["PCT_GRID_DEBUG"], os.environ["PCT_LEVELS_DEBUG"]
                ref_h = capi.Handle(0)
                try:
                    refs[key] = _run(ref_h, capi, pts, c, "GRID" if c[0] == "census" else "BRUTE")
                finally:
                    ref_h.close()
            out.append((lines, res, refs[key]))
    finally:
        h.close()
        for v, val in saved.items():
            os.environ.pop(v, None)
            if val is not None:
                os.environ[v] = val
    return out


@pytest.fixture(scope="module")
def recorded():
    with open(RECORDED) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_passes_of_the_chain(gpu, capfd, recorded, name):
    got = run_case(gpu["capi"], gpu["shapes"], name, lambda: capfd.readouterr().err)
    assert len(got) == len(recorded[name])
    for c, (lines, res, ref), want in zip(CASES[name], got, recorded[name]):
        print(name, c, *lines, sep="\n")
        assert lines == want, (name, c)
        for x, y in zip(res, ref):
            assert np.array_equal(x, y, equal_nan=True), (name, c)


def test_recorded_cases_reach_their_branches(recorded):
    """The recording itself: the pass counts the cases were chosen for."""
    after = lambda name, i=0: sum(ln.startswith("[levels] after pass") for ln in recorded[name][i])
    builds = lambda name, i=0: sum(ln.startswith("[grid] box") for ln in recorded[name][i])
    assert builds("torus") == builds("range") == builds("f64") == 2 and builds("eps") == 1
    assert builds("census") == 8 and after("census") == 7    # the first pass, six banded ones on their sub-boxes, the exact sweep
    assert [builds("grid_levels_grid", i) for i in range(3)] == [1, 2, 1]
    assert after("grid_levels_grid", 0) == after("grid_levels_grid", 2) == 0

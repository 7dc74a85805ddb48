"""Which fast sweep kernel a call takes (pct_timings.sweep_variant).

Every instantiation of k_knn_fast / k_knn_pair / k_knn_duo returns the same rows bit for bit, so nothing else in the
suite can see a slip of the dispatch (a float64 cloud on the all-float64 variant, say): only the timings would.  The
expected words below are written out from the rule in DESIGN 4.2, case by case; nothing here recomputes the rule."""
import re

import numpy as np
import pytest

# pct_timings.sweep_variant (include/pct_hip.h): family in bits 0-1, then one bit per template argument
FAST, PAIR_KERNEL, DUO_KERNEL = 1, 2, 3
R2, EPS, PRE, PAIR, Q64, TREE, DIST = 4, 8, 16, 32, 64, 128, 256

# the switches that steer the dispatch: unset unless a case sets one
KNOBS = ("PCT_NO_PAIR", "PCT_NO_PAIR_KERNEL", "PCT_NO_DUO_KERNEL", "PCT_KEEP_DIST", "PCT_TREE_EXACT_ONLY", "PCT_NO_XCD_MAP",
         "PCT_FAST_R1_MAX", "PCT_NO_TREE", "PCT_NO_AUTO_LEVELS")

N = 4000
FAR_SHIFT = 1.0e6        # float32 resolves 2^-4 there: far beyond "small against a cell edge" for this cloud (asserted below)

# (name, cloud, k, eps, algo, fused, knob, expected word, the case it differs from by the knob only)
CASES = [
    # uniform cell list
    ("f32", "f32", 30, 0.0, "GRID", False, None, PAIR_KERNEL | PRE | PAIR | DIST, None),
    ("f32_fused", "f32", 30, 0.0, "GRID", True, None, PAIR_KERNEL | PRE | PAIR, None),
    ("f32_fused_keep_dist", "f32", 30, 0.0, "GRID", True, "PCT_KEEP_DIST", PAIR_KERNEL | PRE | PAIR | DIST, "f32_fused"),
    ("f32_eps", "f32", 30, 0.2, "GRID", False, None, PAIR_KERNEL | EPS | PRE | PAIR | DIST, None),
    ("f32_k80", "f32", 80, 0.0, "GRID", False, None, DUO_KERNEL | R2 | PRE | PAIR | DIST, None),
    ("f64", "f64", 30, 0.0, "GRID", False, None, PAIR_KERNEL | PRE | PAIR | Q64 | DIST, None),
    ("f64_far", "f64_far", 30, 0.0, "GRID", False, None, FAST | DIST, None),
    ("f32_tiny", "f32_tiny", 30, 0.0, "GRID", False, None, FAST | DIST, None),
    ("f32_no_pair", "f32", 30, 0.0, "GRID", False, "PCT_NO_PAIR", FAST | PRE | DIST, "f32"),
    ("f32_no_pair_kernel", "f32", 30, 0.0, "GRID", False, "PCT_NO_PAIR_KERNEL", FAST | PRE | PAIR | DIST, "f32"),
    ("f64_no_pair_kernel", "f64", 30, 0.0, "GRID", False, "PCT_NO_PAIR_KERNEL", FAST | PRE | PAIR | Q64 | DIST, "f64"),
    ("f32_k80_no_duo_kernel", "f32", 80, 0.0, "GRID", False, "PCT_NO_DUO_KERNEL", FAST | R2 | PRE | PAIR | DIST, "f32_k80"),
    ("f32_levels", "f32", 30, 0.0, "GRID_LEVELS", False, None, FAST | PRE | PAIR | DIST, None),
    ("f64_levels", "f64", 30, 0.0, "GRID_LEVELS", False, None, FAST | DIST, None),
    ("f32_exact", "f32", 30, 0.0, "GRID_EXACT", False, None, 0, None),
    ("f32_k200", "f32", 200, 0.0, "GRID", False, None, 0, None),
    # hierarchical cell list
    ("tree_f32", "f32", 30, 0.0, "TREE", False, None, PAIR_KERNEL | PRE | PAIR | TREE | DIST, None),
    ("tree_f32_k80", "f32", 80, 0.0, "TREE", False, None, DUO_KERNEL | R2 | PRE | PAIR | TREE | DIST, None),
    ("tree_f64", "f64", 30, 0.0, "TREE", False, None, PAIR_KERNEL | PRE | PAIR | Q64 | TREE | DIST, None),
    ("tree_f32_no_pair_kernel", "f32", 30, 0.0, "TREE", False, "PCT_NO_PAIR_KERNEL", FAST | PRE | PAIR | TREE | DIST, "tree_f32"),
    ("tree_f64_no_pair_kernel", "f64", 30, 0.0, "TREE", False, "PCT_NO_PAIR_KERNEL", FAST | PRE | PAIR | Q64 | TREE | DIST, "tree_f64"),
    ("tree_f32_exact_only", "f32", 30, 0.0, "TREE", False, "PCT_TREE_EXACT_ONLY", 0, "tree_f32"),
]


def make_clouds(shapes):
    f32 = shapes.torus_random(N, seed=11)
    f64 = shapes.torus_random(N, seed=11, dtype=np.float64)
    return {"f32": f32, "f64": f64, "f64_far": f64 + FAR_SHIFT, "f32_tiny": f32 * np.float32(1e-20)}


def run_case(h, capi, clouds, case):
    """One call; returns (timings, indices, distances)."""
    _, cloud, k, eps, algo, fused, _, _, _ = case
    h.set_points(clouds[cloud])
    (h.curvature if fused else h.knn)(k, eps, getattr(capi, "KNN_" + algo))
    t = h.timings()
    idx, dist, _ = h.get_neighbors(0, N)
    return t, idx, dist


@pytest.fixture(scope="module")
def bench(gpu):
    h = gpu["capi"].Handle(0)
    yield {"h": h, "capi": gpu["capi"], "clouds": make_clouds(gpu["shapes"]), "rows": {}}
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_sweep_variant(bench, case, monkeypatch):
    name, cloud, k, eps, algo, fused, knob, expected, same_as = case
    h, capi, clouds, rows = bench["h"], bench["capi"], bench["clouds"], bench["rows"]
    for v in KNOBS:
        monkeypatch.delenv(v, raising=False)
    if same_as is not None and same_as not in rows:       # the rows without the knob, computed once
        rows[same_as] = run_case(h, capi, clouds, next(c for c in CASES if c[0] == same_as))[1:]
    if knob:
        monkeypatch.setenv(knob, "1")
    t, idx, dist = run_case(h, capi, clouds, case)
    rows.setdefault(name, (idx, dist))
    if algo in ("TREE", "GRID_LEVELS"):                     # (the tree build took this cloud and did not fall back)
        assert t["algo"] == getattr(capi, "KNN_" + algo), (name, t["algo"])
    if cloud == "f64_far":
        # the precondition of the case: the float32 rounding distance out there, far 2^-23, is not small against a
        # cell edge (cell 2^-7), with a factor of four to spare
        assert t["cell_size"] > 0 and FAR_SHIFT * 2.0 ** -23 >= 4.0 * t["cell_size"] * 2.0 ** -7, t["cell_size"]
    if cloud == "f32_tiny":
        assert 0 < t["cell_size"] ** 2 < 1e-30 / 4, t["cell_size"]
    assert t["sweep_variant"] == expected, (name, bin(t["sweep_variant"]), bin(expected))
    if same_as is not None:                                 # the knob changed the kernel and not one bit of the answer
        assert np.array_equal(idx, rows[same_as][0]) and np.array_equal(dist, rows[same_as][1]), name


@pytest.mark.gpu
def test_sweep_variant_travels_with_its_asynchronous_call(bench, monkeypatch):
    """pct_set_async: pct_get_timings_done describes the call before the pending one -- its kernel, not the pending one's."""
    for v in KNOBS:
        monkeypatch.delenv(v, raising=False)
    h, capi = bench["h"], bench["capi"]
    h.set_points(bench["clouds"]["f32"])
    h.set_async(True)
    try:
        h.curvature(30, 0.0, capi.KNN_GRID)
        h.curvature(80, 0.0, capi.KNN_GRID)               # finishes the bookkeeping of the first, stays pending itself
        assert h.stage_times_done().sweep_variant == PAIR_KERNEL | PRE | PAIR
        assert h.timings()["sweep_variant"] == DUO_KERNEL | R2 | PRE | PAIR      # (waits for the pending call)
    finally:
        h.set_async(False)


def test_launchers_instantiate_the_supported_kernels_only(built):
    """The abort trace names a sweep's launch by the launcher's instantiation, template arguments by value: one such name
    per kernel the library can launch -- k_knn_fast in its six (PRE, PAIR, Q64, TREE) forms x R x EPS, every
    (EPS, DIST, Q64, TREE) of k_knn_pair and k_knn_duo -- and no other."""
    blob = open(built["capi"].LIB_PATH, "rb").read().decode("latin-1")
    names = set(re.findall(r"launch_(?:fast|pair|duo)\([^\[\0]*\[[^\]\0]*\]", blob))
    fast = sorted(re.findall(r"\[R = (\d), EPS = (\w+), PRE = (\w+), PAIR = (\w+), Q64 = (\w+), TREE = (\w+)\]", "\n".join(n for n in names if "launch_fast" in n)))
    t, f = "true", "false"
    forms = [(f, f, f, f), (t, f, f, f), (t, t, f, f), (t, t, t, f), (t, t, f, t), (t, t, t, t)]
    assert fast == sorted((r, e) + form for r in "12" for e in (t, f) for form in forms)
    for kernel in ("pair", "duo"):
        assert len([n for n in names if "launch_" + kernel in n]) == 16, kernel

"""The start of a work item of the fast sweeps (csrc/pct_knn_item.h), on clouds that reach its corners.

k_knn_fast, k_knn_pair and k_knn_duo start a work item the same way: the item's decode, its stencil runs, the prefix of
the run lengths, the overflow test, the hand-off to the redo list, the staging of the runs and the key set-up (shared
helpers, or the kernel's own copy where the header says so).  The clouds here are small and aimed at what a torus never shows it: stencil rows outside the grid (empty runs, the ballot numbering of the
non-empty ones), a grid one cell thick in two axes, stencils beyond the staging capacity next to stencils within it,
tree items that meet more than 16 of their 27 cells, and an owned range that ends inside cells.  Every case must return the
rows of the exhaustive sweep of a fresh handle bit for bit -- indices, distances and, with eps, counts -- and take the
kernel it is aimed at (pct_timings.sweep_variant)."""
import numpy as np
import pytest

FAST, PAIR_KERNEL, DUO_KERNEL = 1, 2, 3          # pct_timings.sweep_variant, bits 0-1 (include/pct_hip.h)
Q64, TREE = 64, 128

KNOBS = ("PCT_NO_PAIR", "PCT_NO_PAIR_KERNEL", "PCT_NO_DUO_KERNEL", "PCT_KEEP_DIST", "PCT_TREE_EXACT_ONLY", "PCT_NO_XCD_MAP",
         "PCT_FAST_R1_MAX", "PCT_NO_TREE", "PCT_NO_AUTO_LEVELS")

DISC_RADIUS = 0.03                                 # clump: radius of the dense disc (see make_clouds)


def make_clouds():
    rng = np.random.default_rng(20240611)
    flat = np.zeros((3000, 3))
    flat[:, :2] = rng.random((3000, 2))          # z exactly 0: nz = 1, six of the nine stencil rows lie outside the grid
    line = np.zeros((2000, 3))
    line[:, 0] = rng.random(2000)                # y = z = 0: ny = nz = 1, one stencil row
    clouds = {"flat": flat, "line": line, "range": flat}
    # 2000 points on the unit square and 2000 in a disc so dense that stencils at its rim, whose cells the square sized,
    # exceed the staging capacity (512 | 768 slots) while those of the square stay well within it: both sides of m > CAP in
    # one launch, at k = 30 and at k = 80 (a few dozen overflowing items each, about 2500 of the 4000 rows redone)
    square = np.zeros((2000, 3))
    square[:, :2] = rng.random((2000, 2))
    r = DISC_RADIUS * np.sqrt(rng.random(2000))
    phi = 2.0 * np.pi * rng.random(2000)
    disc = np.stack([0.5 + r * np.cos(phi), 0.5 + r * np.sin(phi), np.zeros(2000)], axis=1)
    clouds["clump"] = np.concatenate([square, disc])[rng.permutation(4000)]
    # a volume: an item of the hierarchical cell list meets more than 16 of its 27 stencil cells (the crowded rule)
    v = rng.standard_normal((4000, 3))
    clouds["ball"] = v / np.linalg.norm(v, axis=1, keepdims=True) * np.cbrt(rng.random((4000, 1)))
    return clouds


RANGE = (1000, 2000)                               # "range": the middle third of the flat cloud is owned
# eps about the radius that holds k neighbours in the thin part of the cloud: rows on both sides of the bound
EPS = {("flat", 30): 0.05, ("flat", 80): 0.09, ("line", 30): 0.007, ("range", 30): 0.05, ("clump", 30): 0.06, ("ball", 30): 0.18}


def cases():
    out = []

    def add(cloud, dtype, k, algo, family, eps=False):
        out.append((f"{cloud}-{dtype}-k{k}-{algo.lower()}" + ("-eps" if eps else ""), cloud, dtype, k, eps, algo, family))

    for cloud in ("flat", "line", "range"):
        for dtype in ("f32", "f64"):
            add(cloud, dtype, 30, "GRID", PAIR_KERNEL)
            add(cloud, dtype, 80, "GRID", DUO_KERNEL)
            if cloud != "range":                   # (a level pass owns by flag, not by range)
                add(cloud, dtype, 30, "GRID_LEVELS", FAST)
        add(cloud, "f32", 30, "GRID", PAIR_KERNEL, eps=True)
    add("flat", "f32", 80, "GRID", DUO_KERNEL, eps=True)
    add("flat", "f32", 30, "GRID_LEVELS", FAST, eps=True)
    for dtype in ("f32", "f64"):
        add("clump", dtype, 30, "GRID", PAIR_KERNEL)
        add("clump", dtype, 80, "GRID", DUO_KERNEL)
        add("clump", dtype, 30, "GRID_LEVELS", FAST)
    add("clump", "f32", 30, "GRID", PAIR_KERNEL, eps=True)
    for cloud, k in (("flat", 30), ("flat", 80), ("clump", 30), ("clump", 80), ("ball", 30), ("ball", 80)):
        add(cloud, "f32", k, "TREE", PAIR_KERNEL if k == 30 else DUO_KERNEL)
    add("flat", "f64", 30, "TREE", PAIR_KERNEL)
    add("ball", "f64", 30, "TREE", PAIR_KERNEL)
    add("ball", "f32", 30, "TREE", PAIR_KERNEL, eps=True)
    return out


CASES = cases()


@pytest.fixture(scope="module")
def bench(gpu):
    h, ref = gpu["capi"].Handle(0), gpu["capi"].Handle(0)
    yield {"h": h, "ref": ref, "capi": gpu["capi"], "clouds": make_clouds(), "oracle": {}}
    h.close()
    ref.close()


def points(bench, cloud, dtype):
    return bench["clouds"][cloud].astype(np.float32 if dtype == "f32" else np.float64)


def oracle_rows(bench, cloud, dtype, k, eps):
    """The exhaustive sweep of a handle of its own, once per (cloud, dtype, k, eps): whole-cloud rows."""
    key = ("flat" if cloud == "range" else cloud, dtype, k, eps)
    if key not in bench["oracle"]:
        ref, capi = bench["ref"], bench["capi"]
        pts = points(bench, cloud, dtype)
        ref.set_points(pts)
        ref.knn(k, eps, capi.KNN_BRUTE)
        idx, dist, cnt = ref.get_neighbors(0, len(pts), want_count=True)
        assert ref.timings()["sweep_variant"] == 0
        if not eps:                                # the k-th neighbour exists: the rows are full
            assert (cnt == k).all() and (idx < len(pts)).all() and np.isfinite(dist).all()
        bench["oracle"][key] = (idx, dist, cnt)
    return bench["oracle"][key]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_rows_equal_the_exhaustive_sweep(bench, case, monkeypatch):
    name, cloud, dtype, k, with_eps, algo, family = case
    for v in KNOBS:
        monkeypatch.delenv(v, raising=False)
    h, capi = bench["h"], bench["capi"]
    eps = EPS[(cloud, k)] if with_eps else 0.0
    pts = points(bench, cloud, dtype)
    n = len(pts)
    begin, end = RANGE if cloud == "range" else (0, n)
    want_idx, want_dist, want_cnt = (a[begin:end] for a in oracle_rows(bench, cloud, dtype, k, eps))
    if with_eps:                                   # the bound cuts some rows short and leaves others whole
        assert (want_cnt < k).any() and (want_cnt == k).any(), name

    stats = cloud in ("clump", "ball")
    h.set_stats(stats)
    try:
        h.set_points(pts)
        if cloud == "range":
            h.set_query_range(begin, end)
        h.knn(k, eps, getattr(capi, "KNN_" + algo))
        t = h.timings()
        idx, dist, cnt = h.get_neighbors(begin, end, want_count=True)
    finally:
        h.set_stats(False)
    print(name, "variant", bin(t["sweep_variant"]), "algo", t["algo"], "cell", t["cell_size"], "lds_overflows", t["lds_overflows"], "redone", t["redone_queries"])

    assert t["algo"] == getattr(capi, "KNN_" + algo), (name, t["algo"])
    assert t["sweep_variant"] & 3 == family, (name, bin(t["sweep_variant"]))
    assert bool(t["sweep_variant"] & TREE) == (algo == "TREE"), (name, bin(t["sweep_variant"]))
    if family != FAST or algo == "TREE":           # (a float64 level pass keys every candidate in float64: no Q64 form)
        assert bool(t["sweep_variant"] & Q64) == (dtype == "f64"), (name, bin(t["sweep_variant"]))
    assert np.array_equal(idx, want_idx), name
    assert np.array_equal(dist, want_dist), name
    assert np.array_equal(cnt, want_cnt), name

    if cloud == "clump" and algo == "GRID":
        # both sides of m > CAP ran: items of the disc went to the exact sweep whole, items of the square did not
        assert t["lds_overflows"] > 0 and t["redone_queries"] < n, (name, t["lds_overflows"], t["redone_queries"])
    if cloud == "ball":
        assert t["redone_queries"] > 0, name

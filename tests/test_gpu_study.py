"""pct_neighbor_study_curvatures and PointCloud.explicit_quadratic_neighbor_study against the contract of tests/study_exact.py.

The study is how the reference chooses k for everything downstream (pct:732-800, validate_shape calls it before the
curvature pass).  Here k_prefix_rows builds "the point itself + its n nearest" rows from the resident neighbour table,
the fit kernel solves them with per-row counts, and the class bisects columns of the K(n) table on the host.  Every
K(n) entry is held to study_exact's bar -- the larger of the project's contract 1e-5 max(|ref|, 1e-2 max|ref| of the
column) and 4 x the reference's own spread -- and every comparable sample (all decisions further than 4 bars from tol)
to the reference's converged count, at tolerances where the bisection stops anywhere between its bounds.

  (a) table kinds    one 6 000-point torus, k = 100: BRUTE (public order), GRID, GRID_EXACT, GRID_LEVELS (sorted space),
                     TREE (Morton order) and the fused call (no distances kept): same bits from all six
  (b) wide tables    k = 127 ... 511 with n_hi = k: the staged | unstaged fit (n_hi + 1 = 255 | 256), pitch 128 ... 512
  (c) float64        native centring on the x 0.2 + 40 cloud of g13, GRID and TREE
  (d) owned range    set_query_range with lo > 0: the whole-cloud handle's bits; a sample outside is refused
  (e) ties, twins    a lattice whose prefixes are cut inside runs of equal distances; 600 coinciding points; a torus
                     with 60 doubled points, sampled where the twin has the smaller index
  (f) sample lists   repeats, any order, one sample, one column, n_lo = 1 and 2, 513 rows
  (g) refusals
  (h) state          the planted table and an earlier fit keep their bits; a pending asynchronous call is waited for
  (i) the class      g13 per seed and per whole sample, float32 and float64, own table | second handle | eps | one count

The reference tables cost a fit per entry and six more for its spread on the host: they are made once per module, by
the first test that needs them, and never written to.

Measured on an MI355X (one --durations=0 run of this module: 37 tests, 15.9 s together).  The first test of a group pays
for its reference: kinds 3.2 s, wide 2.0 s, float64 2.4 s, the whole samples 2.5 s each, the per-seed counts 1.0 s; every
other test takes 0.5 s or less.  Worst |dK| as a fraction of its bar: kinds 0.015 (all six tables, identical bits), wide
0.013 at every width, float64 0.070, lattice 0.24, pairs 1.8e-9, coinciding points exactly 0, n = 2: 3.9e-10; n = 1:
|K| <= 1.3e-35, finite.  Samples left out: kinds 0 / 0 / 2 of 64, wide 0 of 6, float64 2 / 0 / 2 / 0 / 0 / 0 of 48, float32
0 of 48, whole samples 1 / 0 / 0 of 60 on both clouds.  No case failed on the library as it is.  Five defects planted one at
a time in a scratch build (in-bounds reads only) were each noticed: k_prefix_rows reading nbr_pos[... + j] for j - 1, and
cnt[row] = n: 30 of the 37 tests each; q = trow + q_begin on a sorted-space table: test_owned_range[GRID] (on a whole cloud
owned_pos[trow] == trow, the defect cannot show there); nbr_pitch replaced by k: test_wide_tables[127], [254], [255], [511]
(k no multiple of four); row[mid - lower_bound] for both columns of the class's bisection: the four class tests against g13.
"""
import numpy as np
import pytest

import study_exact as se

pytestmark = pytest.mark.gpu

K_KINDS = 100
KINDS = ("BRUTE", "GRID", "GRID_EXACT", "GRID_LEVELS", "TREE", "FUSED")
WIDE_KS = (127, 128, 254, 255, 256, 511)          # n_hi + 1 = 255 is the last row staged in LDS (csrc/pct_fit.hip: launch)


@pytest.fixture(scope="module")
def bench(gpu, golden):
    """One handle for the module; reference studies and device tables made once, on first use, never written to."""
    h = gpu["capi"].Handle(0)
    made = {}

    def study(name):
        if name not in made:
            with np.errstate(invalid="ignore"):
                if name in se.CASES:
                    made[name] = se.case(name)
                else:                                          # "g13/32", "g13/64": the golden's clouds and per-seed draws
                    g, tag = golden("g13_neighbor_study.npz"), name[-2:]
                    cases = [(float(t), int(lo), int(hi)) for t, lo, hi in g["cases" + tag]]
                    made[name] = (se.Study(g["points" + tag], g["draw" + tag], 3, 100, full=tag == "64"), cases)
        return made[name]
    yield {"h": h, "capi": gpu["capi"], "study": study, "bits": {}, "golden": golden("g13_neighbor_study.npz")}
    h.close()


def _plant(bench, pts, k, kind, load=True):
    """The neighbour table of one kind on the module's handle; asserts the algorithm that ran."""
    h, capi = bench["h"], bench["capi"]
    if load:
        h.set_points(pts)
    algo = getattr(capi, "KNN_" + ("GRID" if kind == "FUSED" else kind))
    (h.curvature if kind == "FUSED" else h.knn)(k, 0.0, algo)
    took = h.timings()["algo"]
    want = algo if k <= 127 or kind == "BRUTE" else capi.KNN_GRID_EXACT       # csrc/pct_auto_route.h: resolve_request
    assert took == want, (kind, k, took, want)
    return h


def _bits(K):
    return np.ascontiguousarray(K, np.float32).view(np.uint32)


def _check(st, K, decisions, where, cols=None):
    """Every entry against its bar; every comparable sample against the reference's count.  Prints the measured figures."""
    ref = st if cols is None else None
    if cols is not None:                                       # a prefix of the study's columns (bars are per column)
        ok, worst = se.check_values(K, st.K[:, :cols], st.bar[:, :cols])
        bad = np.argwhere(~ok)
        assert ok.all(), (where, "values", worst, bad[:6].tolist(), K[~ok][:6], st.K[:, :cols][~ok][:6])
        out = dict(worst=worst, left_out=0.0)
        for tol, lo, hi in decisions:
            want, comparable, _ = st.decide(tol, lo, hi)
            have, _ = se.counts(K, tol, lo, hi, st.n_lo)
            assert se.under_cap(comparable) and (have[comparable] == want[comparable]).all(), (where, tol, lo, hi, have, want, comparable)
            out["left_out"] = max(out["left_out"], float((~comparable).mean()))
    else:
        out = ref.compare(K)
        assert out["values_ok"], (where, "values", out["worst"], out["bad"], [(K[i, j], st.K[i, j], st.bar[i, j]) for i, j in out["bad"]])
        for tol, lo, hi in decisions:
            r = st.compare(K, tol, lo, hi)
            assert r["ok"], (where, tol, lo, hi, r)
            out["left_out"] = max(out["left_out"], r["left_out"])
    print(f"{where}: worst |dK| / bar {out['worst']:.3g}, left out at most {out['left_out']:.3f} of the samples")
    return out


# --------------------------------------------------------------------------------------------------- (a) table kinds
@pytest.mark.parametrize("kind", KINDS)
def test_every_kind_of_table_gives_the_reference_table(bench, kind):
    """BRUTE leaves public indices in the table, the cell lists sorted-space positions (row_of maps a sample to its row),
    TREE Morton order; the fused call keeps no distances.  The rows are the same, so are the bits
    (test_a_neighbourhood_gives_the_same_bits_in_every_row: position must not show)."""
    st, decisions = bench["study"]("kinds")
    h = _plant(bench, st.points, K_KINDS, kind)
    K = h.neighbor_study_curvatures(st.samples, 3, K_KINDS)
    assert K.dtype == np.float32 and K.shape == (64, 98) and np.isfinite(K).all()
    _check(st, K, decisions, ("kinds", kind))
    first = bench["bits"].setdefault("kinds", (kind, _bits(K)))
    assert np.array_equal(_bits(K), first[1]), (kind, "differs from", first[0], np.argwhere(_bits(K) != first[1])[:6].tolist())


# --------------------------------------------------------------------------------------------------- (b) wide tables
@pytest.mark.parametrize("k", WIDE_KS)
def test_wide_tables(bench, k):
    """n_hi = k: rows of up to 512 entries, pitch (n_hi + 4) & ~3 = 128, 132, 256, 256, 260, 512; n_hi + 1 = 255 is the last
    row the fit stages in LDS, from 256 on it walks the prefix table in global memory.  GRID (sorted space) and BRUTE."""
    st, decisions = bench["study"]("wide")
    tables = []
    for kind in ("GRID", "BRUTE"):
        h = _plant(bench, st.points, k, kind, load=kind == "GRID")
        K = h.neighbor_study_curvatures(st.samples, 3, k)
        assert K.shape == (6, k - 2) and np.isfinite(K).all()
        _check(st, K, [d for d in decisions if d[2] + 1 <= k], ("wide", k, kind), cols=k - 2)
        tables.append(_bits(K))
    assert np.array_equal(*tables)
    if k == 511:                                               # a shorter study of the same table: the same columns
        assert np.array_equal(_bits(h.neighbor_study_curvatures(st.samples, 3, 254)), tables[0][:, :252])


# -------------------------------------------------------------------------------------------------------- (c) float64
@pytest.mark.parametrize("kind", ("GRID", "TREE"))
def test_float64_cloud(bench, kind):
    """pct:761 centres in the cloud's dtype: the sample is the native float64 point, its own float32-rounded copy is not
    at distance zero, and 40 + 0.2 x needs the float64 coordinates of the neighbours (float32: 1.9e-6 of 0.01 spacings)."""
    st, decisions = bench["study"]("g13/64")
    assert st.points.dtype == np.float64
    h = _plant(bench, st.points, 100, kind)
    K = h.neighbor_study_curvatures(st.samples, 3, 100)
    _check(st, K, decisions, ("float64", kind))
    first = bench["bits"].setdefault("f64", _bits(K))
    assert np.array_equal(_bits(K), first)
    h.set_points(st.points.astype(np.float32))                 # the precondition: the float32 copy is another cloud
    h.knn(100, 0.0, bench["capi"].KNN_GRID)
    ok, worst = se.check_values(h.neighbor_study_curvatures(st.samples, 3, 100), st.K, st.bar)
    assert worst > 100.0, "float32 rounding does not show on this cloud"


# ---------------------------------------------------------------------------------------------------- (d) owned range
@pytest.mark.parametrize("kind", ("GRID", "BRUTE", "TREE"))
def test_owned_range(bench, kind):
    """q_begin > 0: the table's row of a sample is sample - q_begin (BRUTE) or row_of[sample - q_begin] (sorted space)."""
    st, _ = bench["study"]("kinds")
    h, capi = bench["h"], bench["capi"]
    lo, hi = 1500, 4300
    inside = (st.samples >= lo) & (st.samples < hi)
    assert 20 <= inside.sum() <= 44
    h.set_points(st.points)
    h.knn(K_KINDS, 0.0, getattr(capi, "KNN_" + kind))
    whole = h.neighbor_study_curvatures(st.samples[inside], 3, K_KINDS)
    ok, worst = se.check_values(whole, st.K[inside], st.bar[inside])
    assert ok.all(), (kind, worst)
    h.set_query_range(lo, hi)
    try:
        with pytest.raises(AttributeError):                    # the range dropped the table
            h.neighbor_study_curvatures(st.samples[inside], 3, K_KINDS)
        h.knn(K_KINDS, 0.0, getattr(capi, "KNN_" + kind))
        part = h.neighbor_study_curvatures(st.samples[inside], 3, K_KINDS)
        assert np.array_equal(_bits(part), _bits(whole)), kind
        edge = np.array([lo, hi - 1], np.int64)
        edge_ref = se.table(st.points, edge, 3, 12)
        got = h.neighbor_study_curvatures(edge, 3, 12)
        assert (np.abs(got - edge_ref) <= se.bars(edge_ref, np.zeros(edge_ref.shape), 3)).all()   # (spread 0 on this torus)
        for outside in (lo - 1, hi, 0, 5999):
            with pytest.raises(ValueError, match=f"sample row {outside} outside the owned range"):
                h.neighbor_study_curvatures(np.array([lo, outside]), 3, K_KINDS)
    finally:
        h.set_query_range(0, len(st.points))


# -------------------------------------------------------------------------------------------------- (e) ties and twins
@pytest.mark.parametrize("kind", ("GRID", "BRUTE"))
@pytest.mark.parametrize("name", ("lattice", "twins", "pairs"))
def test_ties_and_twins(bench, name, kind):
    """lattice: nine of ten prefixes are cut inside a run of equal distances -- which points belong to K(n) is decided by
    the public index alone.  twins: a copy's row holds nothing but copies, K is an exact 0; element 0 of the order is the
    copy with the smallest index, not the sample.  pairs: the sample's twin has the smaller index, the neighbour row
    therefore holds the sample itself in the twin's place: coordinates decide, not indices."""
    st, decisions = bench["study"](name)
    h = _plant(bench, st.points, st.n_hi, kind)
    K = h.neighbor_study_curvatures(st.samples, st.n_lo, st.n_hi)
    assert np.isfinite(K).all(), (name, kind, np.argwhere(~np.isfinite(K))[:6].tolist())
    _check(st, K, decisions, (name, kind))
    assert (K[st.zero] == 0).all()
    print(f"{name}: {np.isinf(st.special).sum()} entries without a bar, {np.isfinite(st.special).sum()} flat, {st.zero.sum()} exact zeros of {K.size}")
    first = bench["bits"].setdefault(name, _bits(K))
    assert np.array_equal(_bits(K), first)


# ------------------------------------------------------------------------------------------------------ (f) sample lists
def test_sample_lists(bench):
    st, _ = bench["study"]("kinds")
    h = _plant(bench, st.points, K_KINDS, "GRID")
    full = _bits(h.neighbor_study_curvatures(st.samples, 3, K_KINDS))
    order = np.array([5, 63, 5, 0, 17, 17, 17, 62, 1, 0])     # repeated and unsorted, as np.random.randint draws
    got = _bits(h.neighbor_study_curvatures(st.samples[order], 3, K_KINDS))
    assert np.array_equal(got, full[order])
    for s in (0, 31, 63):                                     # one sample: 98 rows, two blocks of the fit
        assert np.array_equal(_bits(h.neighbor_study_curvatures(st.samples[s:s + 1], 3, K_KINDS)), full[s:s + 1])
    for n in (3, 5, 6, 64, 99, 100):                          # one column
        assert np.array_equal(_bits(h.neighbor_study_curvatures(st.samples, n, n)), full[:, n - 3:n - 2]), n
    assert np.array_equal(_bits(h.neighbor_study_curvatures(st.samples[:9], 40, 100)), full[:9, 37:])
    # 27 samples x 19 counts = 513 rows: one more than 8 x 64, the fit's rows of eight blocks
    assert np.array_equal(_bits(h.neighbor_study_curvatures(st.samples[:27], 3, 21)), full[:27, :19])


@pytest.mark.parametrize("kind", ("GRID", "BRUTE"))
def test_counts_of_one_and_two(bench, kind):
    """n + 1 = 2: no bar (the reference's normal is LAPACK's pick), but whatever normal is picked both points lie in its
    plane: K is 0 up to noise there as well, and finite.  n + 1 = 3: study_exact.special_bar.  From n = 3 on: the contract."""
    kinds, _ = bench["study"]("kinds")
    rows = kinds.samples[:16]
    with np.errstate(invalid="ignore"):
        st = se.Study(kinds.points, rows, 1, 8)
    assert np.isinf(st.bar[:, 0]).all() and np.isfinite(st.bar[:, 1:]).all()
    h = _plant(bench, st.points, K_KINDS, kind)
    K = h.neighbor_study_curvatures(rows, 1, 8)
    print(f"n = 1: |K| up to {np.abs(K[:, 0]).max():.3g} (reference {np.abs(st.K[:, 0]).max():.3g}); n = 2: {np.abs(K[:, 1]).max():.3g} "
          f"(reference {np.abs(st.K[:, 1]).max():.3g}, bars {st.bar[:, 1].min():.3g} ... {st.bar[:, 1].max():.3g})")
    assert np.isfinite(K).all()
    _check(st, K, (), ("n_lo = 1", kind))
    assert np.array_equal(_bits(h.neighbor_study_curvatures(rows, 2, 8)), _bits(K[:, 1:]))


# ----------------------------------------------------------------------------------------------------------- (g) refusals
def test_refusals(bench, gpu):
    st, _ = bench["study"]("kinds")
    capi = bench["capi"]
    h = capi.Handle(0)
    try:
        rows = st.samples[:4]
        h.set_points(st.points)
        with pytest.raises(AttributeError, match="plant the neighbour table first"):       # no table
            h.neighbor_study_curvatures(rows, 3, 20)
        h.knn(40, 0.25, capi.KNN_GRID)
        with pytest.raises(ValueError, match="plain k-NN table"):                           # planted with eps > 0
            h.neighbor_study_curvatures(rows, 3, 20)
        h.knn(40, 0.0, capi.KNN_GRID)
        with pytest.raises(ValueError, match="needs 41 neighbours per point, the table holds 40"):
            h.neighbor_study_curvatures(rows, 3, 41)
        for n_lo, n_hi in ((0, 10), (-1, 10), (11, 10)):
            with pytest.raises(ValueError, match="bad study arguments"):
                h.neighbor_study_curvatures(rows, n_lo, n_hi)
        with pytest.raises(ValueError, match="bad study arguments"):
            h.neighbor_study_curvatures(rows[:0], 3, 10)
        for bad in (-1, 6000):
            with pytest.raises(ValueError, match="outside the owned range"):
                h.neighbor_study_curvatures(np.array([bad]), 3, 10)
        good = h.neighbor_study_curvatures(rows, 3, 40)                                     # ... none of which cost the table
        assert se.check_values(good, st.K[:4, :38], st.bar[:4, :38])[0].all()
        h.voxel_downsample(st.points, 0.05)                                                 # reuses the cell list's buffers
        with pytest.raises(AttributeError, match="plant the neighbour table first"):
            h.neighbor_study_curvatures(rows, 3, 20)
        h.set_query_slab(0, 2)
        h.curvature(40, 0.0, capi.KNN_GRID)
        with pytest.raises(ValueError, match="pct_neighbor_study_curvatures: this handle owns a slab"):
            h.neighbor_study_curvatures(rows, 3, 20)
    finally:
        h.close()


# -------------------------------------------------------------------------------------------------------------- (h) state
@pytest.mark.parametrize("kind", ("GRID", "BRUTE", "TREE", "FUSED"))
def test_a_study_leaves_the_table_and_the_fit_alone(bench, kind):
    """PointCloud studies its own planted table when it is long enough: neighbours and an earlier fit must come back
    bit for bit afterwards (the study's rows, counts and results live in the staging buffers)."""
    st, _ = bench["study"]("kinds")
    n = len(st.points)
    h = _plant(bench, st.points, K_KINDS, kind)
    if kind != "FUSED":
        h.fit()
    keeps_dist = kind != "FUSED"
    before = h.get_neighbors(0, n, want_dist=keeps_dist, want_count=True) + h.get_fit(0, n)
    K = h.neighbor_study_curvatures(st.samples, 3, K_KINDS)
    K2 = h.neighbor_study_curvatures(st.samples[:5], 1, 7)
    after = h.get_neighbors(0, n, want_dist=keeps_dist, want_count=True) + h.get_fit(0, n)
    for name, a, b in zip(("idx", "dist", "count", "coefs", "K", "H", "H2"), before, after):
        assert (a is None and b is None) or np.array_equal(a.view(np.uint32), b.view(np.uint32)), (kind, name)
    h.fit()                                                   # ... and the table still fits to the same bits
    for a, b in zip(before[3:], h.get_fit(0, n)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), kind
    assert np.array_equal(_bits(h.neighbor_study_curvatures(st.samples, 3, K_KINDS)), _bits(K))


def test_a_pending_call_is_waited_for(bench):
    st, _ = bench["study"]("kinds")
    h, capi = bench["h"], bench["capi"]
    h.set_points(st.points)
    h.knn(K_KINDS, 0.0, capi.KNN_GRID)
    want = _bits(h.neighbor_study_curvatures(st.samples, 3, K_KINDS))
    h.set_async(True)
    try:
        h.curvature(40, 0.0, capi.KNN_GRID)
        h.curvature(K_KINDS, 0.0, capi.KNN_GRID)              # pending when the study is asked
        got = _bits(h.neighbor_study_curvatures(st.samples, 3, K_KINDS))
    finally:
        h.set_async(False)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------------- (i) the class
def _cloud(gpu, pts):
    return gpu["PointCloud"](points=pts, normals=np.zeros((len(pts), 0)))


@pytest.mark.parametrize("tag", ("32", "64"))
def test_class_per_seed_counts(bench, gpu, tag):
    """sample_size = 1 under np.random.seed(s): one sample's converged count + 1 per call, as g13 records it from the
    unmodified reference -- on the planted k = 100 table (studied in place) for every seed and case, and through the second
    handle (planted with k = 30) for a dozen seeds.  The planted table and the fit stay what they were."""
    st, cases = bench["study"]("g13/" + tag)
    g = bench["golden"]
    pc = _cloud(gpu, st.points)
    pc.plant_kdtree(100, algorithm="grid")
    pc.fit_explicit_quadratic_surfaces_to_neighborhoods()
    idx, coefs = pc.neighbor_indices.copy(), pc.quadratic_coefficients.copy()
    left = []
    for c, (tol, lo, hi) in enumerate(cases):
        want, comparable, _ = st.decide(tol, lo, hi)
        assert np.array_equal(want + 1, g["plus1_" + tag][:, c])
        assert se.under_cap(comparable)
        left.append(int((~comparable).sum()))
        got = []
        for s in g["seeds"]:
            np.random.seed(int(s))
            got.append(pc.explicit_quadratic_neighbor_study(tol=tol, sample_size=1, lower_bound=lo, upper_bound=hi))
        got = np.array(got)
        assert np.array_equal(got[comparable], want[comparable] + 1), (tag, tol, lo, hi, got, want + 1, comparable)
    print(f"g13 float{tag}: seeds left out per case {left} of 48")
    assert pc._handle.k == 100 and np.array_equal(pc.neighbor_indices, idx)
    assert np.array_equal(pc._handle.get_neighbors(0, 3000)[0], idx) and np.array_equal(pc._handle.get_fit(0, 3000)[0], coefs)
    # the second handle: a table too short for the study stays as it is
    pc.plant_kdtree(30, algorithm="grid")
    pc.fit_explicit_quadratic_surfaces_to_neighborhoods()
    idx, coefs = pc.neighbor_indices.copy(), pc.quadratic_coefficients.copy()
    tol, lo, hi = cases[se.WHOLE_CASES[tag]]
    want, comparable, _ = st.decide(tol, lo, hi)
    for s in g["seeds"][:12]:
        np.random.seed(int(s))
        got = pc.explicit_quadratic_neighbor_study(tol=tol, sample_size=1, lower_bound=lo, upper_bound=hi)
        assert not comparable[s] or got == want[s] + 1, (tag, s, got, want[s] + 1)
    assert pc._handle.k == 30 and np.array_equal(pc._handle.get_neighbors(0, 3000)[0], idx)
    assert np.array_equal(pc._handle.get_fit(0, 3000)[0], coefs) and np.array_equal(pc.quadratic_coefficients, coefs)


@pytest.mark.parametrize("tag", ("32", "64"))
def test_class_whole_samples(bench, gpu, tag):
    """sample_size = 60: the reference returns int(mean) + 1 alone.  The expected value is computed from the reference's
    per-sample counts, with the device's own count substituted for the samples ``stable`` leaves out -- on both sides
    the same -- so that one undecidable sample cannot move the mean across an integer unnoticed.  Own table, second
    handle and a table planted with eps give the same result."""
    g, capi = bench["golden"], bench["capi"]
    pts = g["points" + tag]
    c = se.WHOLE_CASES[tag]
    tol, lo, hi = (float(v) if i == 0 else int(v) for i, v in enumerate(g["cases" + tag][c]))
    draws = g["whole_draw" + tag]
    with np.errstate(invalid="ignore"):
        st = se.Study(pts, draws.ravel(), 3, 100, full=False)
    want, comparable, _ = st.decide(tol, lo, hi)
    h = _plant(bench, pts, 100, "GRID")
    have, _ = se.counts(h.neighbor_study_curvatures(draws.ravel(), lo, hi + 1), tol, lo, hi)
    pc = _cloud(gpu, pts)
    for w, seed in enumerate(g["whole_seeds"]):
        part = slice(60 * w, 60 * w + 60)
        assert se.under_cap(comparable[part]) and se.result(want[part]) == g["whole" + tag][w, c]
        assert (have[part][comparable[part]] == want[part][comparable[part]]).all()
        expected = se.result(np.where(comparable[part], want[part], have[part]))
        print(f"g13 float{tag} whole sample {seed}: {(~comparable[part]).sum()} of 60 left out, reference {g['whole' + tag][w, c]}, expected {expected}")
        results = []
        for planting in (dict(k_neighbors=100), dict(k_neighbors=30), dict(k_neighbors=100, eps=0.5 if tag == "32" else 40.0)):
            pc.plant_kdtree(algorithm="grid", **planting)
            np.random.seed(int(seed))
            results.append(pc.explicit_quadratic_neighbor_study(tol=tol, sample_size=60, lower_bound=lo, upper_bound=hi))
        assert results == [expected] * 3, (tag, seed, results, expected)
        assert pc.eps == planting["eps"] and pc.k_neighbors == 100


def test_class_bounds(bench, gpu):
    """lower_bound == upper_bound: one decision per sample, and the count is the bound whichever way it goes (converged:
    best = mid; not converged: upper is still the bound, pct:787-788).  upper_bound + 1 neighbours must exist: the
    reference's tree returns index N for a missing one and pct:760 raises IndexError, as plant_kdtree does for k > N - 1."""
    st, _ = bench["study"]("g13/32")
    pc = _cloud(gpu, st.points)
    pc.plant_kdtree(100, algorithm="grid")
    for bound in (3, 17, 99):
        np.random.seed(2)
        rows = np.random.randint(0, 3000, 20)
        K = se.table(st.points, rows, bound, bound + 1)
        want, _ = se.counts(K, 0.03, bound, bound)
        assert set(want.tolist()) == {bound}
        np.random.seed(2)
        got = pc.explicit_quadratic_neighbor_study(tol=0.03, sample_size=20, lower_bound=bound, upper_bound=bound)
        d = np.abs(K[:, 1] - K[:, 0])
        bar = se.bars(K, np.zeros(K.shape), bound)             # (spread 0 on this torus: tests/test_study_exact.py)
        if (np.abs(d - np.float32(0.03)) > se.MARGIN * bar.max(1)).all():
            assert got == se.result(want), (bound, got, want)
    assert pc.explicit_quadratic_neighbor_study(sample_size=0) == 0                        # pct:797-798
    small = _cloud(gpu, st.points[:50].copy())
    with pytest.raises(IndexError) as planted:
        small.plant_kdtree(50)
    with pytest.raises(IndexError) as studied:
        small.explicit_quadratic_neighbor_study(tol=0.03, sample_size=5, lower_bound=3, upper_bound=49)
    assert type(planted.value) is type(studied.value)
    np.random.seed(5)
    assert isinstance(small.explicit_quadratic_neighbor_study(tol=0.03, sample_size=5, lower_bound=3, upper_bound=48), int)

"""The quadric fit on the device against an exact solve, across its conditioning range, and at the edges of its launch.

tests/fit_exact.py builds the cases and the bars (and says where every constant comes from); tests/test_fit_exact.py
checks on the CPU that the reference itself meets them.  Here the kernels do:

  (a) k_quadric_rows (always the SVD)           -- Handle.fit_quadric on every rung, m = 6, 7, 8, 50, 300
  (b) k_fit and its hand-over to k_fit_svd      -- the paired blocks as clouds through Handle.fit_indices, float32 / float64
  (c) the unrounded variant                     -- Handle.fit_indices_f64, against the conditioning term alone
  (d) row lengths 0 ... 512, staged and unstaged, garbage behind the count
  (e) row position: XCD block map, partial last block, SVD list spanning waves -- identical bits wherever a row sits
  (f) queries 0 ... 1 000 radii outside their neighbourhood
  (g) the float32 curvature formulas over coefficient space

Every bar is the exact solution or the reference; only (e) compares the device with itself, and (e) is an invariance.
"""
import numpy as np
import pytest

import fit_exact as fe
import pct_oracle as oracle

pytestmark = pytest.mark.gpu


@pytest.fixture
def handle(gpu):
    h = gpu["capi"].Handle(0)
    yield h
    h.close()


def _bits(*arrays):
    return [np.ascontiguousarray(a, np.float32).view(np.uint32) for a in arrays]


def _assert_curvatures_of_rung(K, H, c32, where):
    """K, H against oracle.quadric_curvatures of the correctly rounded exact coefficients: the 1e-5 contract, its floor
    taken over the rung."""
    rK, rH, _ = oracle._curv_f32(c32)
    for name, got, ref in (("K", K, rK), ("H", H, rH)):
        ok = oracle.curvature_tolerance_ok(got, ref, fe.FLOOR * np.abs(ref).max(), fe.RTOL)
        assert ok.all(), (where, name, got[~ok], ref[~ok])


def _assert_coefficients(co, facts, where, rounded=True):
    worst = 0.0
    for c, f in zip(co, facts):
        ok, err, bar = fe.within_bar(c, f, rounded)
        assert ok.all(), (where, f["pivot"], f["kappa"], err / bar)
        worst = max(worst, float((err / bar).max()))
    return worst


# ------------------------------------------------------------------------------------------------ (a) the solver alone
@pytest.mark.parametrize("m,paired", fe.SOLVER_CASES)
def test_solver_alone_on_every_rung(handle, m, paired):
    for kind, cond, facts in fe.ladder_facts(m, paired):
        blocks = np.array([f["block"] for f in facts], np.float32)
        co = handle.fit_quadric(blocks)
        assert co.dtype == np.float32 and co.shape == (len(facts), 6)
        worst = _assert_coefficients(co, facts, (m, paired, kind, cond))
        K, H, _ = handle.curvatures_from_coefficients(co)
        _assert_curvatures_of_rung(K, H, np.array([f["c32"] for f in facts]), (m, paired, kind, cond))
        print(f"m={m} paired={paired} {kind} {cond:g}: worst error {worst:.3f} of the bar")


# ----------------------------------------------------------------------------- (b), (c) the fused fit and its hand-over
def _ladder_cloud(m, dtype):
    """Every paired block of one m as ONE cloud: the query at the origin (record 0), then the blocks' points; one table
    row per block.  Returns (cloud, idx, query, [(kind, cond, facts, row slice)])."""
    rungs, pts, at = [], [np.zeros((1, 3), np.float32)], 0
    for kind, cond, facts in fe.ladder_facts(m, True):
        rungs.append((kind, cond, facts, slice(at, at + len(facts))))
        pts += [f["block"] for f in facts]
        at += len(facts)
    idx = 1 + np.arange(at * m, dtype=np.int32).reshape(at, m)
    return np.vstack(pts).astype(dtype), idx, np.zeros(at, np.int64), rungs


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("m", fe.FUSED_M)
def test_fused_fit_and_its_switch_on_every_rung(handle, m, dtype):
    cloud, idx, query, rungs = _ladder_cloud(m, dtype)
    handle.set_points(cloud)
    handle.fit_indices(idx, query=query)
    co, K, H, H2 = handle.get_fit(0, len(idx))
    svd_rows = handle.timings()["fit_svd_rows"]
    pivots = np.concatenate([[f["pivot"] for f in facts] for _, _, facts, _ in rungs])
    # the design's invariants, not the constant: hopeless normal equations are handed over, comfortable ones are not
    assert (pivots <= 1e-10).sum() <= svd_rows <= len(idx) - (pivots >= 1e-3).sum(), (svd_rows, len(idx))
    for kind, cond, facts, rows in rungs:
        worst = _assert_coefficients(co[rows], facts, (m, dtype.__name__, kind, cond))
        _assert_curvatures_of_rung(K[rows], H[rows], np.array([f["c32"] for f in facts]), (m, dtype.__name__, kind, cond))
        assert np.array_equal(*_bits(H2[rows], H[rows] * H[rows]))
        # ... and rung by rung, where a rung lies on one side altogether
        handle.fit_indices(idx[rows], query=query[rows])
        n_svd = handle.timings()["fit_svd_rows"]
        piv = np.array([f["pivot"] for f in facts])
        if (piv <= 1e-10).all():
            assert n_svd == len(facts), (kind, cond, n_svd)
        if (piv >= 1e-3).all():
            assert n_svd == 0, (kind, cond, n_svd)
        print(f"m={m} {dtype.__name__} {kind} {cond:g}: pivot ratio {piv.min():.1e}..{piv.max():.1e}, {n_svd}/{len(facts)} rows handed over, "
              f"worst error {worst:.3f} of the bar")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("m", fe.FUSED_M)
def test_unrounded_fit_against_the_conditioning_term_alone(handle, m, dtype):
    """The only place where an fp64-level error of the Cholesky path is visible at all."""
    cloud, idx, query, rungs = _ladder_cloud(m, dtype)
    handle.set_points(cloud)
    c64, K64, H64 = handle.fit_indices_f64(idx, query=query)
    assert c64.dtype == np.float64
    for kind, cond, facts, rows in rungs:
        worst = _assert_coefficients(c64[rows], facts, (m, dtype.__name__, kind, cond), rounded=False)
        print(f"m={m} {dtype.__name__} {kind} {cond:g}: worst unrounded error {worst:.3f} of C eps kappa S")


# ---------------------------------------------------------------------------------------------------- (d) row lengths
LENGTHS = tuple(range(0, 41)) + (63, 64, 65, 127, 128, 255, 256, 300, 448, 511, 512)


@pytest.mark.parametrize("width", [40, 64, 65, 128, 255, 256, 300, 448, 511, 512])
def test_row_lengths_with_garbage_behind_the_count(handle, gpu, width):
    """Rows of every length in one table (count array), the unused entries holding -1 and indices far outside the cloud.
    width <= 255 is staged in LDS, 256 ... 512 are walked in global memory (512: one past the longest row a sweep writes).  Each row against the reference loop on its
    valid prefix; 2 ... 5 neighbours against lstsq's minimum-norm answer; 0 and 1 read NaN."""
    pts = gpu["shapes"].torus_random(3000, seed=21)
    full, _ = oracle.knn(pts, 512)                  # (a tie-free cloud: the row for a width is a prefix of this one)
    lengths = [n for n in LENGTHS if n <= width]
    rng = np.random.default_rng(width)
    query = rng.choice(len(pts), 3 * len(lengths), replace=False).astype(np.int64)
    count = np.repeat(lengths, 3).astype(np.int32)
    idx = full[query][:, :width].copy()
    junk = rng.choice(np.array([-1, -7, len(pts), 2_000_000_000, -2_147_483_648], np.int64), idx.shape).astype(np.int32)
    behind = np.arange(width)[None, :] >= count[:, None]
    idx[behind] = junk[behind]
    handle.set_points(pts)
    handle.fit_indices(idx, count=count, query=query)
    co, K, H, H2 = handle.get_fit(0, len(idx))
    c64, K64, H64 = handle.fit_indices_f64(idx, count=count, query=query)

    none = count < 2
    assert np.isnan(co[none]).all() and np.isnan(K[none]).all() and np.isnan(H[none]).all() and np.isnan(H2[none]).all()
    assert np.isnan(c64[none]).all() and np.isnan(K64[none]).all()
    assert np.isfinite(co[~none]).all() and np.isfinite(K[~none]).all() and np.isfinite(c64[~none]).all()

    def reference(r, order=None):
        nb = idx[r, :count[r]] if order is None else idx[r, :count[r]][order]
        c, k, h, _ = oracle.curvature_loop(pts, nb[None, :], [query[r]])
        return c[0], k[0], h[0]

    full_rows = np.flatnonzero(count >= 6)
    ref = [reference(r) for r in full_rows]
    rc, rK, rH = (np.array(x) for x in zip(*ref))
    okK = oracle.curvature_tolerance_ok(K[full_rows], rK, fe.FLOOR * np.abs(rK).max(), fe.RTOL)
    okH = oracle.curvature_tolerance_ok(H[full_rows], rH, fe.FLOOR * np.abs(rH).max(), fe.RTOL)
    assert okK.all() and okH.all(), (width, count[full_rows][~(okK & okH)])
    scale = max(1.0, float(np.abs(rc[:, :3]).max()))
    for got in (co[full_rows], c64[full_rows]):
        close = np.isclose(got, rc, rtol=1e-5, atol=2e-6 * scale).all(1)
        assert close.all(), (width, count[full_rows][~close])
    for r in np.flatnonzero((count >= 2) & (count < 6)):
        n = count[r]
        # three points lie IN their plane and two on a line: the orientation test's dot product (pct:293) is rounding
        # noise (n = 3) and the normal LAPACK's pick in a null space (n = 2) -- the reference's answer is defined up to
        # the orientation (either order of first and last neighbour) for n = 3 and not at all for n = 2
        if n == 2:
            continue
        cands = [reference(r)[0]] + ([reference(r, np.arange(n)[::-1])[0]] if n == 3 else [])
        assert any(np.allclose(co[r], c, rtol=1e-5, atol=1e-6 * np.abs(c).max()) for c in cands), (width, n, co[r], cands)


# --------------------------------------------------------------------------------------------------- (e) row position
def _position_case(gpu):
    """64 distinct neighbourhoods (k = 30) of one cloud: 56 on a torus, 8 on straight lines (collinear: the normal
    equations have no pivot, the rows go to k_fit_svd)."""
    pts = gpu["shapes"].torus_random(2000, seed=13)
    rng = np.random.default_rng(13)
    lines = []
    for _ in range(8):
        p0, d = rng.uniform(-1, 1, 3) + 5.0, rng.standard_normal(3)
        lines.append(p0 + np.outer(np.linspace(-0.1, 0.1, 31), d / np.linalg.norm(d)))
    cloud = np.vstack([pts] + lines).astype(np.float32)
    idx, _ = oracle.knn(cloud, 30)
    smooth = rng.choice(2000, 56, replace=False)
    degenerate = 2000 + 31 * np.arange(8) + 15                     # the middle point of every line
    query = np.empty(64, np.int64)
    slots = np.array([3, 12, 21, 30, 39, 48, 57, 63])
    query[slots] = degenerate
    query[np.setdiff1d(np.arange(64), slots)] = smooth
    return cloud, idx[query], query


@pytest.mark.parametrize("xcd_map", [True, False])
def test_a_neighbourhood_gives_the_same_bits_in_every_row(handle, gpu, monkeypatch, xcd_map):
    """The grid is rounded up to a multiple of 8 blocks (blocks past the rows return early), the last block is partial,
    the SVD list is filled by several waves: none of it may show in a row's result."""
    cloud, idx64, query64 = _position_case(gpu)
    if not xcd_map:
        monkeypatch.setenv("PCT_NO_XCD_MAP", "1")
    handle.set_points(cloud)
    handle.fit_indices(idx64, query=query64)
    base = _bits(*handle.get_fit(0, 64))
    assert handle.timings()["fit_svd_rows"] == 8
    assert all(np.isfinite(b.view(np.float32)).all() for b in base)
    for rows in (1, 63, 64, 65, 511, 512, 513, 8 * 64 * 3 + 1):
        tile = np.arange(rows) % 64
        handle.fit_indices(idx64[tile], query=query64[tile])
        got = _bits(*handle.get_fit(0, rows))
        assert handle.timings()["fit_svd_rows"] == np.isin(tile, [3, 12, 21, 30, 39, 48, 57, 63]).sum(), rows
        for g, b in zip(got, base):
            assert np.array_equal(g, b[tile]), (rows, xcd_map)
        c64 = handle.fit_indices_f64(idx64[tile], query=query64[tile])[0]
        assert np.array_equal(c64.astype(np.float32).view(np.uint32), base[0][tile]), (rows, xcd_map)


# ------------------------------------------------------------------------------- (f) queries outside their neighbourhood
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_queries_outside_their_neighbourhood(handle, dtype):
    """query= 0, 1, 3, 10, 100 and 1 000 neighbourhood radii from the centroid, along the normal and in the tangent plane,
    against oracle.curvature_loop: per row the larger of the 1e-5 contract and R x the reference's own spread over
    permuted rows (fit_exact.foreign_bars).  Also what far outliers look like to their own fit
    (test_far_outliers_do_not_coarsen_the_cell_list masks those rows)."""
    P, idx, query, offset = fe.foreign_query_cloud(11, dtype)
    K_ref, H_ref, sK, sH = fe.reference_with_spread(P, idx, query)
    handle.set_points(P)
    handle.fit_indices(idx, query=query)
    _, K, H, _ = handle.get_fit(0, len(idx))
    for name, got, ref, spread in (("K", K, K_ref, sK), ("H", H, H_ref, sH)):
        contract, term, drop = fe.foreign_bars(ref, spread, offset)
        for t in fe.FOREIGN_OFFSETS:
            r = offset == t
            assert drop[r].sum() <= 0.1 * r.sum(), (name, t)
            if t <= 10:
                assert (term[r] <= contract[r]).all(), (name, t)
            err = np.abs(got - ref)[r & ~drop] / np.maximum(contract, term)[r & ~drop]
            print(f"{dtype.__name__} {name} at {t:g} radii: worst error {err.max():.3f} of the bar")
        keep = ~drop
        assert (np.abs(got - ref)[keep] <= np.maximum(contract, term)[keep]).all(), (name, offset[keep][np.abs(got - ref)[keep] > np.maximum(contract, term)[keep]])


# ------------------------------------------------------------------------------------------- (g) the curvature formulas
def test_curvature_formulas_over_coefficient_space(handle):
    """calculate_explicit_quadratic_curvatures (pct:398-431) in float32, operation for operation: K bit for bit; H within
    one ulp (the reference's ** 1.5 is powf, the kernel's a correctly rounded w * sqrt(w)); same inf / NaN pattern."""
    co = fe.coefficient_space()
    K, H, H2 = handle.curvatures_from_coefficients(co)
    with np.errstate(all="ignore"):
        rK, rH, rH2 = oracle._curv_f32(co, scalar_pow=True)
    assert len(co) > 2000 and np.isinf(rK).any() + np.isnan(rK).any() + np.isnan(rH).any() > 0
    assert np.array_equal(np.isnan(K), np.isnan(rK)) and np.array_equal(np.isnan(H), np.isnan(rH))
    assert np.array_equal(np.isinf(K), np.isinf(rK)) and np.array_equal(np.isinf(H), np.isinf(rH))
    num = ~np.isnan(rK)
    same = K[num].view(np.uint32) == rK[num].view(np.uint32)
    assert same.all(), (co[num][~same][:5], K[num][~same][:5], rK[num][~same][:5])
    fin = np.isfinite(rH)
    inf = np.isinf(rH)
    assert np.array_equal(H[inf], rH[inf])
    off = np.abs(H[fin].astype(np.float64) - rH[fin].astype(np.float64)) / np.spacing(np.abs(rH[fin])).astype(np.float64)
    assert (off <= 1.0).all(), (off.max(), co[fin][off > 1.0][:5])
    assert np.array_equal(*_bits(H2[fin], H[fin] * H[fin]))
    print(f"{len(co)} coefficient rows: K identical, H identical on {(off == 0).mean():.4f}, off by one ulp on the rest")

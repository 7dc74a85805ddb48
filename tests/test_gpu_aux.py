"""The kernels around the path on the device, at their launch edges: voxel down-sampling and surface variation
(pct_aux.hip), mesh energies (pct_mesh.hip).

tests/aux_exact.py builds the cases and the bars (and says where every constant comes from); tests/test_aux_exact.py
checks on the CPU that the reference meets them and that planted defects do not.  Here the kernels do:

  (a) voxel down-sampling, float32 / float64, indices compared exactly with the vectorised first-occurrence reference:
      n = 1, 255, 256, 257; 524 545 points (three passes of k_scan_int, the carry passing 2^18) half kept, one voxel, every
      point its own voxel; 2^21 - 1 voxels along an axis (accepted) and 2^21 (refused); points ON voxel boundaries, both
      signs, -0.0; a float32 cloud 1e5 from the origin; one handle for large, small, large
  (b) surface variation under a query range (k_surface_variation's row_offset / out_base; brute-force, uniform and
      hierarchical cell list): the rows of the whole-cloud call bit for bit, sampled rows within eig_exact's bar
  (c) mesh energies: every golden of the reference run, T = 0, 1, 255, 256, 257, 262 144, 262 145, 524 588 (the
      grid-stride loop's second and third pass), slivers, mixed curvature dtypes, handle reuse

Every bar is the exact reference or the reference run; the device is compared with itself only for the stated
invariances: range against whole cloud, and handle reuse.

Measured on an MI355X (worst error as a share of its bar, per group; every test prints its own):
  voxel down-sampling     identical indices in every case; 524 545 points: 262 869 (float32) / 262 870 (float64) kept of
                          the uniform cloud, 1 of the one-voxel cloud, all 524 545 of the lattice
  surface variation       range == whole cloud bit for bit on the exhaustive sweep (n = 3 000), the uniform list (5 000) and
                          the hierarchical list (200 000); sampled rows at 0.42 ... 0.49 of eig_exact's bar
  energies, goldens       0.061 (live_inf's area), 0.053 ... 0.056 on the others, 0 on zero_area; mixed dtypes bit-equal to
                          the pure case of each array's dtype
  energies, launch edges  T = 1 ... 257: 0.051;  262 144: 0.011;  262 145: 0.019;  524 588: 0.016
  energies, slivers       0.023 whole mesh, 0.076 rung by rung (0.061 at the georeferenced offset)
The three suspicions of the code reading: no triangles -- pct_mesh_energies already returned zeros before any launch
(test_energies_of_no_triangles is the evidence); mixed curvature dtypes and the surface-variation output under a query
range were wrong as read (float64 K rounded to float32 beside a float32 H; N outputs allocated, end - begin written)
and are fixed -- test_energies_mixed_dtypes_keep_each_array_in_its_own, test_surface_variation_under_a_query_range.
"""
import math

import numpy as np
import pytest

import aux_exact as ax
import eig_exact as ee
import pct_oracle as oracle

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


@pytest.fixture
def handle(gpu):
    h = gpu["capi"].Handle(0)
    yield h
    h.close()


# ======================================================================================================================
# (a) voxel down-sampling
# ======================================================================================================================
def _check_voxel(h, pts, voxel, where):
    got = h.voxel_downsample(pts, voxel)
    want = ax.first_occurrence(pts, voxel)
    assert got.dtype == np.int64 and got.ndim == 1, where
    assert (np.diff(got) > 0).all(), where                             # strictly increasing = order of first occurrence
    assert len(got) == len(want) and np.array_equal(got, want), (where, len(got), len(want))
    return want


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_voxel_block_edges(handle, n, dtype):
    rng = np.random.default_rng(n)
    pts = (rng.normal(size=(n, 3)) * 0.3).astype(dtype)
    for voxel in (0.05, 0.3, 10.0):
        _check_voxel(handle, pts, voxel, (n, dtype.__name__, voxel))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["half", "one_voxel", "lattice"])
def test_voxel_three_scan_passes(handle, form, dtype):
    """2 050 block counts: k_scan_int runs three passes and carries twice."""
    pts, voxel = {"half": ax.half_kept_cloud, "one_voxel": ax.one_voxel_cloud, "lattice": ax.lattice_cloud}[form](dtype)
    n = len(pts)
    assert n == ax.N_THREE_PASSES == 524_545 and pts.dtype == dtype
    want = ax.first_occurrence(pts, voxel)
    if form == "half":
        assert 0.3 * n < len(want) < 0.7 * n, len(want)
    elif form == "one_voxel":
        assert want.tolist() == [0]
    else:
        assert np.array_equal(want, np.arange(n))                     # the scan's total is n, its carry 2^18 after one pass
    got = _check_voxel(handle, pts, voxel, (form, dtype.__name__))
    print(f"voxel {form} {dtype.__name__}: {len(got)} of {n} kept, identical")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_voxel_span_limit(handle, axis, dtype):
    """21 bits per axis in the packed key: a span of 2^21 - 1 voxels is the last one accepted."""
    pts, voxel = ax.span_cloud(dtype, axis, ax.VOXEL_SPAN_MAX - 1)
    assert _check_voxel(handle, pts, voxel, ("span", axis)).tolist() == [0, 1]
    pts, voxel = ax.span_cloud(dtype, axis, ax.VOXEL_SPAN_MAX)
    with pytest.raises(ValueError, match=r"voxel grid spans more than 2\^21 voxels along an axis"):
        handle.voxel_downsample(pts, voxel)
    pts, voxel = ax.span_cloud(dtype, axis, ax.VOXEL_SPAN_MAX - 1)     # ... and the handle is none the worse for refusing
    assert handle.voxel_downsample(pts, voxel).tolist() == [0, 1]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("voxel", [0.05, 0.1])
def test_voxel_boundaries_signs_and_negative_zero(handle, voxel, dtype):
    _check_voxel(handle, ax.multiples_cloud(dtype, voxel), voxel, ("multiples", voxel, dtype.__name__))


def test_voxel_float32_quotient_decides(handle):
    pts, voxel = ax.offset_cloud()
    _check_voxel(handle, pts, voxel, "offset 1e5 float32")
    _check_voxel(handle, pts.astype(np.float64), voxel, "offset 1e5, the same coordinates in float64")


def test_voxel_one_handle_large_small_large(handle):
    big, vb = ax.half_kept_cloud(np.float32, n=300_001, seed=41)
    small, vs = ax.half_kept_cloud(np.float64, n=700, seed=42)
    big2, vb2 = ax.lattice_cloud(np.float32, n=300_001, seed=43)
    for pts, voxel, where in ((big, vb, "large"), (small, vs, "small"), (big2, vb2, "large again"), (small, vs, "small again")):
        _check_voxel(handle, pts, voxel, where)


# ======================================================================================================================
# (b) surface variation under a query range
# ======================================================================================================================
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _range_against_whole(handle, capi, pts, k_total, begin, end, algo_whole, algo_range, sample):
    handle.set_points(pts)
    whole = handle.surface_variation(k_total)
    assert handle.timings()["algo"] == algo_whole, handle.timings()["algo"]
    assert whole.shape == (len(pts),) and whole.dtype == np.float32 and np.isfinite(whole).all()
    handle.set_query_range(begin, end)
    part = handle.surface_variation(k_total)
    assert handle.timings()["algo"] == algo_range, handle.timings()["algo"]
    assert part.shape == (end - begin,) and part.dtype == np.float32
    assert np.array_equal(_bits(part), _bits(whole[begin:end]))
    handle.set_query_range(0, len(pts))
    again = handle.surface_variation(k_total)
    assert again.shape == (len(pts),) and np.array_equal(_bits(again), _bits(whole))
    # sampled rows of the range against the exact value of their neighbourhood (the point itself + k_total - 1 neighbours)
    rows = begin + np.sort(np.random.default_rng(k_total).choice(end - begin, sample, replace=False))
    idx, _ = oracle.knn(pts, k_total - 1, query_rows=rows)
    worst = 0.0
    for r, nb in zip(rows, idx):
        ok, share = ee.sv_within_bar(part[r - begin], pts[np.concatenate([[r], nb])])
        assert ok, (k_total, r, share)
        worst = max(worst, share)
    return worst


@pytest.mark.parametrize("k_total", [11, 100])
@pytest.mark.parametrize("n", [3000, 5000])
def test_surface_variation_under_a_query_range(handle, gpu, n, k_total):
    """n = 5 000: the uniform cell list (rows in sorted space, owned_pos); n = 3 000: the exhaustive sweep (row_offset)."""
    capi = gpu["capi"]
    pts = gpu["shapes"].torus_random(n, seed=29)
    algo = capi.KNN_GRID if n >= 4096 else capi.KNN_BRUTE
    begin, end = (1234, 3001) if n == 5000 else (1234, 2999)
    worst = _range_against_whole(handle, capi, pts, k_total, begin, end, algo, algo, sample=12)
    assert end - begin == (1767 if n == 5000 else 1765)
    print(f"surface variation n={n} k={k_total} rows [{begin}, {end}): bits of the whole-cloud call; worst sampled error {worst:.3f} of the bar")


def test_surface_variation_range_on_the_hierarchical_list(handle, gpu):
    """The scan of test_pointcloud_flow_on_a_lidar_like_scan (density ~ 1/r^2, k = 100: AUTO takes the hierarchical cell
    list for the whole cloud; a range of it is answered by the uniform list): the same bits either way."""
    capi = gpu["capi"]
    rng = np.random.default_rng(18)
    n = 200_000
    r, a = 0.02 * 50 ** rng.uniform(0, 1, n), rng.uniform(0, 2 * np.pi, n)
    x, y = r * np.cos(a), r * np.sin(a)
    pts = np.stack([x, y, 0.1 * np.sin(2 * x) * np.cos(2 * y)], 1).astype(np.float32)
    worst = _range_against_whole(handle, capi, pts, 101, 123_456, 125_223, capi.KNN_TREE, capi.KNN_GRID, sample=6)
    print(f"surface variation on the hierarchical list, rows [123456, 125223): bits of the whole-cloud call; worst sampled error {worst:.3f} of the bar")


# ======================================================================================================================
# (c) mesh energies
# ======================================================================================================================
def _check_energies(got, want, bar, where):
    assert all(isinstance(g, float) for g in got) and len(got) == 3
    assert ax.same_values(got, want), (where, got, want)
    sh = ax.shares(got, want, bar)
    fin = [s for s, w in zip(sh, want) if math.isfinite(w)]
    assert all(s <= 1 for s in fin), (where, dict(zip(ax.NAMES, sh)), got, want)
    return max(fin)


@pytest.mark.parametrize("case", ax.GOLDEN_CASES)
def test_energies_on_the_goldens(handle, golden, case):
    """Against the exact reference within the bars AND against the reference run: the non-finite sums as values, the
    finite ones within the same bars (the run's own error included: its loop meets them, tests/test_aux_exact.py)."""
    v, t, K, H, out = ax.golden_case(golden(ax.GOLDEN), case)
    K, H = ax.curvatures_or_zeros(v, K, H)
    want, facts = ax.exact_energies(v, t, K, H)
    got = handle.mesh_energies(v, t, K, H)
    worst = _check_energies(got, want, ax.bars(facts), case)
    assert ax.same_values(got, out), (case, got, out)
    if case == "zero_area":
        assert got == (0.0, 0.0, 0.0)
    print(f"energies {case} (K {K.dtype.name}, H {H.dtype.name}): worst error {worst:.3f} of the bar")


def test_energies_mixed_dtypes_keep_each_array_in_its_own(handle, golden):
    """np.mean takes each array in its own dtype: K float64 with H float32 gives the float64 case's stretching and the
    float32 case's bending, bit for bit on the device too -- and the pure cases are what they were."""
    g = golden(ax.GOLDEN)
    got = {}
    for case in ("random_f32", "random_f64", "mixed_K64_H32", "mixed_K32_H64"):
        v, t, K, H, _ = ax.golden_case(g, case)
        got[case] = handle.mesh_energies(v, t, K, H)
    assert got["mixed_K64_H32"] == (got["random_f32"][0], got["random_f64"][1], got["random_f64"][2])
    assert got["mixed_K32_H64"] == (got["random_f64"][0], got["random_f32"][1], got["random_f64"][2])
    assert got["random_f32"][0] != got["random_f64"][0] and got["random_f32"][1] != got["random_f64"][1]


def test_energies_of_no_triangles(handle, gpu):
    """utils.py:719-721: zeros, without a launch of no blocks -- and bad arguments are still refused."""
    from point_cloud_toolbox_amd.energies import mesh_energies
    v, t, K, H = ax.random_mesh(3, 50, 10, np.float32)
    for empty in (np.zeros((0, 3), np.int32), np.zeros((0, 3), np.int64), []):
        assert mesh_energies(v, empty, K, H) == (0.0, 0.0, 0.0)
        assert handle.mesh_energies(v, empty, K.astype(np.float64), H) == (0.0, 0.0, 0.0)
    bad = t.copy()
    bad[3, 2] = -1
    with pytest.raises(ValueError, match="outside"):
        handle.mesh_energies(v, bad, K, H)
    with pytest.raises(ValueError, match="one curvature value per vertex"):
        handle.mesh_energies(v, t, K[:-1], H)
    want, facts = ax.exact_energies(v, t, K, H)                       # ... and the handle answers the next mesh
    _check_energies(handle.mesh_energies(v, t, K, H), want, ax.bars(facts), "after the refusals")


_EDGE = {}


def _edge(T, dtype):
    key = (T, np.dtype(dtype).name)
    if key not in _EDGE:
        m = ax.edge_mesh(T, dtype)
        _EDGE[key] = (m, ax.reference_energies(*m))
    return _EDGE[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", ax.EDGE_T)
def test_energies_at_the_launch_edges(handle, T, dtype):
    """One thread ... the cap of 1024 blocks exactly, one triangle into the second pass of the grid-stride loop, two passes
    and a partial third.  Rational areas up to 2 000 triangles, the float64 area with math.fsum (and both sides' area
    error in the bar) above."""
    (v, t, K, H), (want, facts, sides) = _edge(T, dtype)
    got = handle.mesh_energies(v, t, K, H)
    worst = _check_energies(got, want, ax.bars(facts, sides), (T, dtype.__name__))
    print(f"energies T={T} {dtype.__name__}: depth {ax.kernel_depth(T)}, worst error {worst:.3f} of the bar")


@pytest.mark.parametrize("offset", [(0.0, 0.0, 0.0), (4.2e5, 5.1e6, 250.0)])
def test_energies_on_slivers(handle, offset):
    """Aspect ratios 1 ... 1e12, at the origin and at a georeferenced offset (the edge subtractions then round)."""
    v, t, K, H = ax.sliver_mesh(seed=15, offset=offset)
    want, facts = ax.exact_energies(v, t, K, H)
    worst = _check_energies(handle.mesh_energies(v, t, K, H), want, ax.bars(facts), ("slivers", offset))
    one = 0.0                                                          # ... and each rung alone: the large ones cannot hide the small
    per = len(t) // len(ax.SLIVER_ASPECTS)
    for j, aspect in enumerate(ax.SLIVER_ASPECTS):
        tj = t[j * per:(j + 1) * per]
        wj, fj = ax.exact_energies(v, tj, K, H)
        one = max(one, _check_energies(handle.mesh_energies(v, tj, K, H), wj, ax.bars(fj), ("sliver rung", aspect, offset)))
    print(f"energies slivers at {offset}: worst error {worst:.3f} of the bar, rung by rung {one:.3f}")


def test_energies_handle_reuse_gives_the_same_bits(handle):
    (small, _), (large, _) = _edge(257, np.float32), _edge(ax.MESH_STRIDE + 1, np.float64)
    first = handle.mesh_energies(*small)
    assert handle.mesh_energies(*small) == first
    big = handle.mesh_energies(*large)
    assert handle.mesh_energies(*small) == first                       # stale partials of 1024 blocks behind the 2 in use
    assert handle.mesh_energies(*large) == big
    sl = ax.sliver_mesh()
    s1 = handle.mesh_energies(*sl)
    assert handle.mesh_energies(*small) == first and handle.mesh_energies(*sl) == s1

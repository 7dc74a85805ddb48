"""PCA principal curvatures on the device (pct_pca_curvatures, PointCloud.principal_curvatures_via_principal_component_analysis)
against goldens of the unmodified reference (pct:901-950) and the CPU restatement in tests/pca_restatement.py."""
import glob
import os
import sys

import numpy as np
import pytest
from scipy.spatial import cKDTree

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pca_restatement as pr  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[len("g12_pca_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "g12_pca_*.npz")))
NAN_MSG = "array must not contain infs or NaNs"


def assert_sign_rule(dirs):
    """Documented sign of every eigenvector: its component of largest magnitude (the first of equal ones) is positive."""
    first_max = np.take_along_axis(dirs, np.abs(dirs).argmax(axis=1)[:, None, :], 1)[:, 0, :]
    assert (first_max >= 0).all()


def run_class(PointCloud, pts, k, **kw):
    pc = PointCloud(points=pts, normals=np.zeros((len(pts), 0)))
    assert pc.principal_curvatures_via_principal_component_analysis(k, **kw) is None
    assert_sign_rule(pc.principal_curvature_directions)
    return pc, dict(l1=pc.pca_principal_curvature_values_1, l2=pc.pca_principal_curvature_values_2,
                    dirs=pc.principal_curvature_directions, K=pc.pca_K_values, H=pc.pca_H_values)


def run_handle(capi, pts, k, algo=0):
    h = capi.Handle(0)
    try:
        h.set_points(pts)
        exact = h.pca_curvatures(k, algo, keep_neighbors=True)
        l1, l2, dirs, K, H, idx = h.get_pca(0, len(pts), want_idx=True)
    finally:
        h.close()
    assert_sign_rule(dirs)
    return dict(l1=l1, l2=l2, dirs=dirs, K=K, H=H), idx, exact


def check_against_restatement(pts, k, got, idx, rows=None):
    """Rows whose k-th place is no near-tie: the restatement's values; the others: a valid k-nearest set and the
    restatement's values on that set."""
    rows = np.arange(len(pts)) if rows is None else rows
    ref = pr.restate(pts, k, rows)
    sub = {key: v[rows] for key, v in got.items()}
    ok = pr.compare(sub, ref, ref["l3"], rows_mask=~ref["ambiguous"])
    assert ok.all(), f"{(~ok).sum()} of {len(rows)} rows outside the bars"
    amb = np.flatnonzero(ref["ambiguous"])[:200]
    if len(amb):
        kk = idx.shape[1]
        for r in amb:
            assert pr.valid_set(pts, rows[r], idx[rows[r]], kk), f"row {rows[r]}: not a k-nearest set"
        own = pr.frame(pts, idx[rows[amb]])
        ok = pr.compare({key: v[rows[amb]] for key, v in got.items()}, own, own["l3"])
        assert ok.all()
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_goldens_through_the_class(gpu, golden, case):
    g = golden(f"g12_pca_{case}.npz")
    pts, k = g["points"], int(g["k"])
    if "error" in g:
        pc = gpu["PointCloud"](points=pts, normals=np.zeros((len(pts), 0)))
        with pytest.raises(ValueError, match=NAN_MSG):
            pc.principal_curvatures_via_principal_component_analysis(k)
        return
    _, got = run_class(gpu["PointCloud"], pts, k)
    ref = dict(l1=g["pca_principal_curvature_values_1"], l2=g["pca_principal_curvature_values_2"],
               dirs=g["principal_curvature_directions"], K=g["pca_K_values"], H=g["pca_H_values"])
    for key in ref:
        assert got[key].shape == ref[key].shape and got[key].dtype == np.float64
    res = pr.restate(pts, k)                                            # (lambda_3 for the projector bar)
    ok = pr.compare(got, ref, res["l3"], rows_mask=~g["ambiguous"])
    assert ok.all(), f"{(~ok).sum()} rows outside the bars"
    hgot, idx, _ = run_handle(gpu["capi"], pts, k)
    for key in got:
        assert np.array_equal(hgot[key], got[key])
    amb = np.flatnonzero(g["ambiguous"])
    kk = min(k, len(pts) - 1)
    for r in amb:
        assert pr.valid_set(pts, r, idx[r], kk)
    if len(amb):
        own = pr.frame(pts, idx[amb])
        assert pr.compare({key: v[amb] for key, v in got.items()}, own, own["l3"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [20, 50, 100])
def test_float64_cloud_takes_float64_neighbours(gpu, k):
    """Coarse float32 rounding (x 0.2 + 40): the float32-rounded ranking differs at the k-th place on many rows; the
    neighbour set of every row must be the float64 k-d tree's."""
    pts = gpu["shapes"].torus_random(60_000, seed=3, dtype=np.float64) * 0.2 + 40.0
    got, idx, exact = run_handle(gpu["capi"], pts, k)
    _, want = cKDTree(pts).query(pts, k + 1)
    assert np.array_equal(np.sort(idx, 1), np.sort(want[:, 1:], 1))
    _, want32 = cKDTree(pts.astype(np.float32).astype(np.float64)).query(pts, k + 1)
    assert (np.sort(want32[:, 1:], 1) != np.sort(want[:, 1:], 1)).any(axis=1).sum() > 0    # the test has teeth
    ref = pr.frame(pts, want[:, 1:])
    assert pr.compare(got, ref, ref["l3"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("algorithm", ["brute", "grid", "tree"])
def test_float64_lattice_goes_through_the_exact_pass(gpu, algorithm):
    """A cubic lattice, exact in float64 and float32: at k = 100 the k-th distance of an interior point lies in the shell
    of 30 points at distance 3, which also holds the 16 extra candidates -- no certificate, the exhaustive float64 pass
    answers the row (in the sweep's cell order under grid and tree, in public order under brute)."""
    g = np.arange(14, dtype=np.float64)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + 0.5
    algo = {"brute": 1, "grid": 2, "tree": 5}[algorithm]
    got, idx, exact = run_handle(gpu["capi"], pts, 100, algo)
    assert exact > 0
    for r in range(0, len(pts), 29):
        assert pr.valid_set(pts, r, idx[r], 100)
    ref = pr.frame(pts, idx)
    assert pr.compare(got, ref, ref["l3"]).all()
    base, _, _ = run_handle(gpu["capi"], pts, 100, 1)
    for key in got:
        assert np.array_equal(got[key], base[key]), key


@pytest.mark.gpu
def test_float64_k511_every_row_exact(gpu):
    """k = 511 leaves no room for candidates beyond k: every row of a float64 cloud takes the exhaustive pass (in the
    sweep's cell order: k > 127 sweeps the cell list), within its limit of point visits at 20 000 points ..."""
    pts = gpu["shapes"].torus_random(20_000, seed=9, dtype=np.float64)
    got, idx, exact = run_handle(gpu["capi"], pts, 511)
    assert exact == len(pts)
    check_against_restatement(pts, 511, got, idx, np.arange(0, len(pts), 7))


@pytest.mark.gpu
def test_float64_k511_beyond_the_limit_is_refused(gpu):
    """... and is refused, with the reason, where that pass would exceed the limit (2^30 point visits)."""
    pts = gpu["shapes"].torus_random(40_000, seed=9, dtype=np.float64)
    pc = gpu["PointCloud"](points=pts, normals=np.zeros((len(pts), 0)))
    with pytest.raises(ValueError, match="no room for candidates beyond k"):
        pc.principal_curvatures_via_principal_component_analysis(511)
    pc.principal_curvatures_via_principal_component_analysis(495)           # 16 candidates beyond k: certified
    assert pc.pca_exact_rows < 100


@pytest.mark.gpu
@pytest.mark.parametrize("k", [20, 50])
def test_float64_georeferenced_offset(gpu, k):
    """A scan at a UTM-like offset (float32 steps of 0.5 m near a 5e6 m northing, point spacing ~0.7 m): the sweep
    ranks the cloud recentred on its first point, so the float64 neighbour sets are certified without the exhaustive
    pass, and equal a float64 k-d tree's."""
    pts = gpu["shapes"].torus_random(60_000, seed=15, dtype=np.float64) * 50.0 + np.array([4.2e5, 5.1e6, 250.0])
    got, idx, exact = run_handle(gpu["capi"], pts, k)
    assert exact < 60
    _, want = cKDTree(pts).query(pts, k + 1)
    assert np.array_equal(np.sort(idx, 1), np.sort(want[:, 1:], 1))
    ref = pr.frame(pts, want[:, 1:])
    assert pr.compare(got, ref, ref["l3"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("shape,k", [("sphere", 20), ("sphere", 50), ("torus", 20), ("torus", 50)])
def test_100k_clouds(gpu, shape, k):
    sh = gpu["shapes"]
    pts = sh.fibonacci_sphere(100_000) if shape == "sphere" else sh.torus_random(100_000, seed=21)
    got, idx, _ = run_handle(gpu["capi"], pts, k)
    check_against_restatement(pts, k, got, idx)


@pytest.mark.gpu
def test_1m_torus_sampled_rows(gpu):
    pts = gpu["shapes"].torus_random(1_000_000, seed=1234)
    got, idx, _ = run_handle(gpu["capi"], pts, 50)
    rows = np.sort(np.random.default_rng(5).choice(len(pts), 2000, replace=False))
    check_against_restatement(pts, 50, got, idx, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 3, 30, 63, 64, 127, 128, 300, 511])
def test_k_range(gpu, k):
    pts = gpu["shapes"].torus_random(20_000, seed=9)
    got, idx, _ = run_handle(gpu["capi"], pts, k)
    rows = np.arange(len(pts)) if k <= 128 else np.arange(0, len(pts), 7)
    check_against_restatement(pts, k, got, idx, rows)


@pytest.mark.gpu
def test_edges(gpu):
    PointCloud = gpu["PointCloud"]
    pts = gpu["shapes"].torus_random(50, seed=2)
    _, got = run_class(PointCloud, pts, 100)                           # k >= N: N - 1 neighbours
    ref = pr.restate(pts, 100)
    assert pr.compare(got, ref, ref["l3"], rows_mask=~ref["ambiguous"]).all()
    pc = PointCloud(points=pts, normals=np.zeros((50, 0)))
    for k in (0, 1):
        with pytest.raises(ValueError, match=NAN_MSG):
            pc.principal_curvatures_via_principal_component_analysis(k)
    for dtype in (np.float32, np.float64):
        pc = PointCloud(points=pts.astype(dtype), normals=np.zeros((50, 0)))
        bad = pts.astype(dtype)
        bad[7, 1] = np.nan
        pc.points = bad                                                 # after construction (the constructor refuses NaN)
        with pytest.raises(ValueError, match=NAN_MSG):
            pc.principal_curvatures_via_principal_component_analysis(10)
    big = gpu["shapes"].torus_random(20_000, seed=9)
    pc = PointCloud(points=big, normals=np.zeros((len(big), 0)))
    with pytest.raises(ValueError, match="at most 511"):
        pc.principal_curvatures_via_principal_component_analysis(512)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_algorithms_bit_identical(gpu, dtype):
    pts = gpu["shapes"].torus_random(20_000, seed=4, dtype=dtype)
    if dtype == np.float64:
        pts = pts * 0.2 + 40.0
    outs = [run_class(gpu["PointCloud"], pts, 30, algorithm=a)[1] for a in ("brute", "grid", "tree")]
    for o in outs[1:]:
        for key in o:
            assert np.array_equal(o[key], outs[0][key]), key


@pytest.mark.gpu
def test_state_is_preserved(gpu):
    pts = gpu["shapes"].torus_random(30_000, seed=8)
    pc = gpu["PointCloud"](points=pts, normals=np.zeros((len(pts), 0)))
    pc.plant_kdtree(30)
    pc.fit_explicit_quadratic_surfaces_to_neighborhoods()
    K0, H0 = (np.array(a) for a in pc.calculate_curvatures_of_explicit_quadratic_surfaces_for_all_points())
    before = dict(idx=pc.neighbor_indices.copy(), dists=pc.dists.copy(), coefs=np.array(pc.quadratic_coefficients),
                  K=np.array(pc.K_quadratic), q=pc.kdtree.query(pts[:100].astype(np.float64), 5))
    pc.principal_curvatures_via_principal_component_analysis(50)
    assert pc.k_neighbors == 30
    assert np.array_equal(pc.neighbor_indices, before["idx"]) and np.array_equal(pc.dists, before["dists"])
    assert np.array_equal(np.array(pc.quadratic_coefficients), before["coefs"])
    assert np.array_equal(np.array(pc.K_quadratic), before["K"])
    K1, H1 = pc.calculate_curvatures_of_explicit_quadratic_surfaces_for_all_points()
    assert np.array_equal(np.array(K1), K0) and np.array_equal(np.array(H1), H0)
    q = pc.kdtree.query(pts[:100].astype(np.float64), 5)
    assert np.array_equal(q[0], before["q"][0]) and np.array_equal(q[1], before["q"][1])


@pytest.mark.gpu
def test_exact_duplicates(gpu):
    base = gpu["shapes"].torus_random(5000, seed=6)
    rng = np.random.default_rng(6)
    pts = np.concatenate([base, base[rng.choice(5000, 1500, replace=False)]])[rng.permutation(6500)]
    got, idx, _ = run_handle(gpu["capi"], pts, 20)
    check_against_restatement(pts, 20, got, idx)

"""Per-point surface frames on the device (pct_point_frames; csrc/pct_frame.hip) against ``frame_exact.reference`` on the rows
the device's own k-NN returns and the coefficients the device's own fit left.

Per case (voronoi_exact.CASES; the bars and their exclusions are measured and pinned on the CPU in tests/test_frame_exact.py):
  NaN rows, flipped           exactly the reference's (flipped: where the dot product clears the normal's own bar)
  k1, k2                      C_K eps max|k|, every row
  normal                      C_N u, the rows whose rotation is a function of the block
  d1, d2                      up to sign, C_D (u + eps max|k| / (k1 - k2)), where k1 - k2 >= 1e-6 max|k|
  invariants                  unit length and orthogonality within 16 eps on EVERY row that is no NaN
  rows left out               counted: at most 10 % of a case, 1 % on the spheres, the tori, the egg carton, the doubled sphere
"""
import numpy as np
import pytest

import frame_exact as fe
import voronoi_exact as ve

pytestmark = pytest.mark.gpu

TIGHT = ("sphere-k8", "sphere-k30", "sphere-k200", "torus-k30", "torus-k16", "egg-k30", "doubled-k16")
FLAT = ("ring-k80", "lattice-k8")


@pytest.fixture(scope="module")
def dev(gpu):
    h = gpu["capi"].Handle(0)
    yield {"h": h, "capi": gpu["capi"], "PointCloud": gpu["PointCloud"]}
    h.close()


def frames(h, n, begin=0, end=None, viewpoint=None):
    """Frames of the resident table and fit; the device's rows, coefficients and results for [begin, end)."""
    end = n if end is None else end
    h.point_frames(viewpoint)
    idx, _, cnt = h.get_neighbors(begin, end, True, False, True)
    coefs = h.get_fit(begin, end, K=False, H=False, H2=False)[0]
    normal, k, dirs, flipped = h.get_point_frames(begin, end)
    assert normal.dtype == k.dtype == dirs.dtype == np.float64 and flipped.dtype == np.uint8
    assert normal.shape == (end - begin, 3) and k.shape == (end - begin, 2) and dirs.shape == (end - begin, 3, 2)
    return np.where((idx >= 0) & (idx < n), idx, 0), cnt, coefs, (normal, k, dirs, flipped), h.point_frame_stats()


def plant(h, pts, k, eps=None, algo=None, begin=None, end=None, viewpoint=None, fused=False):
    h.set_points(pts)
    if begin is not None:
        h.set_query_range(begin, end)
    args = (k, eps or 0.0) if algo is None else (k, eps or 0.0, algo)
    if fused:
        h.curvature(*args)
    else:
        h.knn(*args)
        h.fit()
    idx, cnt, coefs, got, stats = frames(h, len(pts), begin or 0, end, viewpoint)
    return idx, (cnt if eps else None), coefs, got, stats


def hold(name, pts, idx, cnt, coefs, got, stats, rows=None, viewpoint=None):
    ref = fe.reference(pts, idx, cnt, coefs, viewpoint=viewpoint, rows=rows)
    c = fe.compare(*got, ref)
    m = len(idx)
    print(f"{name}: {m} rows, {stats['nan']} NaN, {stats['flipped']} flipped, {stats['umbilic']} umbilic, {stats['ms']:.3f} ms; share of the bar: "
          f"k {c['share_k']:.3f}, normal {c['share_normal']:.3f}, directions {c['share_dirs']:.3f}, invariants {c['share_invariant']:.3f}; "
          f"left out {int(c['left_out'].sum())}, by the k-gap {int(c['gap_out'].sum())} more")
    fe.assert_frames(name, c)
    normal, k, dirs, flipped = got
    nan = np.isnan(k[:, 0])
    assert stats["rows"] == m and stats["nan"] == int(nan.sum()) and stats["flipped"] == int(flipped.sum()), (name, stats)
    assert stats["umbilic"] <= int((k[:, 0] == k[:, 1]).sum()) and (viewpoint is not None or stats["flipped"] == 0)
    assert (k[~nan, 0] >= k[~nan, 1]).all()
    assert c["left_out"].sum() <= ve.LEFT_OUT_CAP * m, (name, "rows left out", int(c["left_out"].sum()))
    if name in TIGHT:
        assert c["left_out"].sum() <= 0.01 * m and c["gap_out"].sum() <= 0.01 * m, (name, int(c["left_out"].sum()), int(c["gap_out"].sum()))
    return ref, c


def run(dev, name, **kw):
    make, k, eps = ve.CASES[name]
    pts = make()
    idx, cnt, coefs, got, stats = plant(dev["h"], pts, k, eps, **kw)
    ref, c = hold(name, pts, idx, cnt, coefs, got, stats)
    return pts, idx, cnt, coefs, got, stats, ref, c


@pytest.mark.parametrize("name", ["sphere-k8", "sphere-k30", "sphere-k200", "torus-k30", "torus-k16", "egg-k30", "doubled-k16",
                                  "offset64-k30"])
def test_curved_cases(dev, name):
    pts, idx, cnt, coefs, got, stats, ref, c = run(dev, name)
    assert stats["nan"] == 0
    if name == "sphere-k200":
        assert idx.shape[1] == 200


@pytest.mark.parametrize("name", FLAT)
def test_flat_cases(dev, name):
    """k1 = k2 = 0 exactly, every direction left out by construction, the normal (0, 0, +-1) exactly."""
    pts, idx, cnt, coefs, (normal, k, dirs, flipped), stats, ref, c = run(dev, name)
    assert not k.any() and stats["umbilic"] == len(pts) and c["gap_out"].all()
    assert np.array_equal(np.abs(normal), np.tile([0.0, 0.0, 1.0], (len(pts), 1)))


def test_eps_hybrid_rows(dev):
    pts, idx, cnt, coefs, (normal, k, dirs, flipped), stats, ref, c = run(dev, "hybrid-k8")
    hist = np.bincount(cnt, minlength=ve.HYBRID_K + 1)
    assert hist[0] > 0 and hist[1] > 0 and (hist[2:] > 0).all()
    assert np.array_equal(np.isnan(k[:, 0]), cnt < 2) and stats["nan"] == int((cnt < 2).sum())
    assert c["left_out"][cnt == 3].all()                   # three neighbours: no orientation, rule (2)


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_block_edges(dev, n):
    """One block and a lane short of it, one lane into the next, two blocks and a lane: fewer blocks than XCDs."""
    pts = ve.fibonacci_sphere(n)
    capi = dev["capi"]
    got = {}
    for algo in (capi.KNN_BRUTE, capi.KNN_GRID):
        idx, cnt, coefs, got[algo], stats = plant(dev["h"], pts, 8, algo=algo)
        hold(f"sphere-{n}", pts, idx, cnt, coefs, got[algo], stats)
    for a, b in zip(got[capi.KNN_BRUTE], got[capi.KNN_GRID]):
        assert np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("k", [5, 8, 9])
def test_one_and_two_index_quads(dev, k):
    pts = ve.table_clouds(n=1000)[0]
    idx, cnt, coefs, got, stats = plant(dev["h"], pts, k)
    hold(f"torus-1000-k{k}", pts, idx, cnt, coefs, got, stats)


def test_query_range_owns_the_middle_third(dev):
    h = dev["h"]
    pts = ve.table_clouds()[0]
    b, e = len(pts) // 3, 2 * len(pts) // 3
    idx, cnt, coefs, got, stats = plant(h, pts, 30, begin=b, end=e)
    hold("torus-range", pts, idx, cnt, coefs, got, stats, rows=np.arange(b, e))
    assert stats["rows"] == e - b
    for lo, hi in ((0, 10), (e - 5, e + 5), (b - 1, b + 1)):
        with pytest.raises(ValueError):
            h.get_point_frames(lo, hi)
    part = h.get_point_frames(b + 7, b + 19, k=False, flipped=False)
    assert part[1] is None and part[3] is None and np.array_equal(part[0], got[0][7:19]) and np.array_equal(part[2], got[2][7:19])
    whole = plant(h, pts, 30)[3]                            # the whole cloud on the same handle gives these rows the same bytes
    for a, w in zip(got, whole):
        assert np.array_equal(a, w[b:e])


def test_every_sweep_gives_the_same_frames(dev):
    """Public order (the exhaustive sweep) against table-row order and the gather (the cell list, the hierarchical list)."""
    capi = dev["capi"]
    pts = ve.table_clouds()[0]
    view = (0.3, -0.2, 5.0)
    base = None
    for algo in (capi.KNN_BRUTE, capi.KNN_GRID, capi.KNN_TREE):
        idx, cnt, coefs, got, stats = plant(dev["h"], pts, 30, algo=algo, viewpoint=view)
        if base is None:
            base = (idx, coefs, got)
            hold("torus-brute", pts, idx, cnt, coefs, got, stats, viewpoint=view)
            continue
        assert np.array_equal(idx, base[0]) and np.array_equal(coefs, base[1], equal_nan=True), algo
        for a, w in zip(got, base[2]):
            assert np.array_equal(a, w), algo


def test_fused_and_separate_fits_give_the_same_frames(dev):
    pts = ve.table_clouds()[1]
    capi = dev["capi"]
    one = plant(dev["h"], pts, 30, algo=capi.KNN_GRID, fused=True)
    two = plant(dev["h"], pts, 30, algo=capi.KNN_GRID)
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[2], two[2])
    for a, w in zip(one[3], two[3]):
        assert np.array_equal(a, w)


def test_jacobi_route_within_the_bars(dev, monkeypatch):
    monkeypatch.setenv("PCT_FIT_JACOBI", "1")
    run(dev, "torus-k30")
    monkeypatch.delenv("PCT_FIT_JACOBI")


# ---- the viewpoint -------------------------------------------------------------------------------------------------------
def egg_H(pts, amp=0.1):
    """Mean curvature of z = amp sin(pi x) cos(pi y) against the upward normal (closed form)."""
    x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    s, c, sy, cy = np.sin(np.pi * x), np.cos(np.pi * x), np.sin(np.pi * y), np.cos(np.pi * y)
    fx, fy = amp * np.pi * c * cy, -amp * np.pi * s * sy
    fxx = fyy = -amp * np.pi ** 2 * s * cy
    fxy = -amp * np.pi ** 2 * c * sy
    return ((1 + fx * fx) * fyy - 2 * fx * fy * fxy + (1 + fy * fy) * fxx) / (2 * (1 + fx * fx + fy * fy) ** 1.5)


def test_viewpoint_above_the_egg_carton(dev):
    h = dev["h"]
    pts = ve.table_clouds()[1]
    view = (0.0, 0.0, 1e3)
    idx, cnt, coefs, got, stats = plant(h, pts, 30, viewpoint=view)
    hold("egg-view", pts, idx, cnt, coefs, got, stats, viewpoint=view)
    normal, k, dirs, flipped = got
    assert (normal[flipped.astype(bool)][:, 2] > 0).all() and (normal[:, 2] > 0).all()
    H_fit = h.get_fit(0, len(pts), coefs=False, K=False, H2=False)[2]
    H = egg_H(pts)
    rows = (np.abs(pts[:, 0]) < 0.85) & (np.abs(pts[:, 1]) < 0.85) & (np.abs(H) > 0.05 * np.abs(H).max())
    H_signed = np.where(flipped.astype(bool), -H_fit, H_fit)
    wrong, plain = int((np.sign(H_signed) != np.sign(H))[rows].sum()), int((np.sign(H_fit) != np.sign(H))[rows].sum())
    print(f"egg carton: {int(rows.sum())} interior rows: {wrong} signs of H wrong with the viewpoint, {plain} without")
    assert int(rows.sum()) == 2593 and wrong == 0 and plain > 1000
    # without the viewpoint: the same frames on the fit's own side
    h.point_frames()
    n0, k0, d0, f0 = h.get_point_frames(0, len(pts))
    assert not f0.any()
    back = fe.unflip(normal, k, dirs, flipped.astype(bool))
    assert np.array_equal(back[0], n0) and np.array_equal(back[1], k0) and np.array_equal(back[2], d0)


def test_viewpoint_at_the_centre_of_the_sphere(dev):
    h = dev["h"]
    pts = ve.fibonacci_sphere(ve.SPHERE_N)
    idx, cnt, coefs, got, stats = plant(h, pts, 30, viewpoint=(0.0, 0.0, 0.0))
    hold("sphere-view", pts, idx, cnt, coefs, got, stats, viewpoint=(0.0, 0.0, 0.0))
    normal, k, dirs, flipped = got
    H = h.get_fit(0, len(pts), coefs=False, K=False, H2=False)[2]
    assert (np.where(flipped.astype(bool), -H, H) > 0).all() and (k[:, 1] > 0).all() and ((normal * pts).sum(1) < 0).all()


def test_viewpoint_at_a_cloud_point(dev):
    """(v - p) is zero for that row: the dot product is 0, which is not below 0 -- no flip, whatever the normal."""
    h = dev["h"]
    pts = ve.table_clouds()[0]
    h.set_points(pts)
    h.knn(30)
    h.fit()
    h.point_frames()
    plain = h.get_point_frames(0, len(pts))
    for row in (0, 1234, len(pts) - 1):
        h.point_frames(pts[row].astype(np.float64))
        got = h.get_point_frames(0, len(pts))
        assert got[3][row] == 0 and got[3].any()
        for a, w in zip(got, plain):
            assert np.array_equal(a[row], w[row])
    for bad in ((np.nan, 0.0, 0.0), (0.0, np.inf, 0.0)):
        with pytest.raises(ValueError):
            h.point_frames(bad)


# ---- state and class -------------------------------------------------------------------------------------------------------
def test_state_rules(dev):
    h = dev["h"]
    pts = ve.fibonacci_sphere(500)
    h.set_points(pts)
    with pytest.raises(AttributeError):
        h.point_frames()                                   # no table: as pct_fit
    h.knn(8)
    with pytest.raises(ValueError, match="no fit results"):
        h.point_frames()
    with pytest.raises(ValueError, match="no point frames"):
        h.get_point_frames(0, len(pts))
    assert h.point_frame_stats()["rows"] == 0
    h.fit()
    h.point_frames()
    first = h.get_point_frames(0, len(pts))
    assert h.point_frame_stats()["rows"] == len(pts)
    h.fit()                                                # a fit drops them
    with pytest.raises(ValueError, match="no point frames"):
        h.get_point_frames(0, len(pts))
    h.point_frames()
    for a, w in zip(h.get_point_frames(0, len(pts)), first):
        assert np.array_equal(a, w)
    h.knn(8)                                               # a new planting drops them, as it drops the fit
    with pytest.raises(ValueError):
        h.get_point_frames(0, len(pts))
    assert h.point_frame_stats()["rows"] == 0
    h.fit()
    h.point_frames()
    h.set_query_range(0, 100)                              # so does a new owned range
    with pytest.raises(ValueError):
        h.get_point_frames(0, 100)
    h.set_points(pts)                                      # and a new cloud
    with pytest.raises(ValueError):
        h.get_point_frames(0, len(pts))


def test_class_surface(dev, tmp_path):
    PointCloud = dev["PointCloud"]
    pts = ve.table_clouds()[1]
    pc = PointCloud(points=pts, normals=np.zeros((len(pts), 0)))
    with pytest.raises(AttributeError):
        pc.compute_surface_frames()                        # needs plant_kdtree
    pc.plant_kdtree(30)
    energies = pc.compute_point_energies()
    K, H = pc.compute_pointwise_explicit_quadratic_curvature()
    normals, k1, k2, dirs = pc.compute_surface_frames()
    assert normals.shape == (len(pts), 3) and normals.dtype == np.float64 and pc.normals is normals
    assert pc.k1_quadratic is k1 and pc.k2_quadratic is k2 and pc.principal_directions_quadratic is dirs and dirs.shape == (len(pts), 3, 2)
    assert pc.normals_flipped.dtype == bool and not pc.normals_flipped.any()
    assert pc.H_signed_quadratic.dtype == np.float32 and np.array_equal(pc.H_signed_quadratic, H)
    assert pc.last_frame_stats["rows"] == len(pts) and pc.last_frame_stats["flipped"] == 0
    assert pc.compute_surface_frames()[0] is normals      # cached per planting, fit and viewpoint
    up = pc.compute_surface_frames(viewpoint=(0.0, 0.0, 1e3))
    assert (up[0][:, 2] > 0).all() and pc.normals_flipped.any() and pc.last_frame_stats["flipped"] == int(pc.normals_flipped.sum())
    assert np.array_equal(pc.H_signed_quadratic, np.where(pc.normals_flipped, -H, H))
    assert np.array_equal(up[1][pc.normals_flipped], -k2[pc.normals_flipped])
    # against the handle's own calls
    h = dev["h"]
    _, _, _, got, _ = plant(h, pts, 30)
    assert np.array_equal(got[0], normals) and np.array_equal(got[1][:, 0], k1) and np.array_equal(got[2], dirs)
    # the reference's names
    pc.normals = np.zeros((len(pts), 0))
    assert pc.compute_normals() is None and np.array_equal(pc.normals, normals)
    pc.normals = None
    out = tmp_path / "frames.ply"
    pc.export_ply_with_curvature_and_normals(str(out))
    assert np.array_equal(pc.normals, normals)
    text = out.read_text().split("\n")
    assert text[2] == f"element vertex {len(pts)}" and text[6:9] == ["property float nx", "property float ny", "property float nz"]
    back = np.loadtxt(out, skiprows=text.index("end_header") + 1)
    assert np.array_equal(back.astype(np.float32), np.column_stack([pts, normals.astype(np.float32), K, H]))
    # the object still answers as before
    assert pc.compute_point_energies() == energies
    K2, H2 = pc.compute_pointwise_explicit_quadratic_curvature()
    assert np.array_equal(K2, K) and np.array_equal(H2, H)
    assert np.array_equal(pc.compute_surface_frames()[0], normals)      # a new fit: computed again, the same bits
    pc.plant_kdtree(8)                                     # a second planting invalidates them
    assert not np.array_equal(pc.compute_surface_frames()[0], normals)
    pc.close()

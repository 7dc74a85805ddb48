"""Consistent normal orientation on the device (pct_orient_frames; csrc/pct_orient.hip) against ``orient_exact.orient`` run on the
device's own unoriented normals and the table ``pct_get_neighbors`` returns.  No tolerance anywhere: component, parent, level
and toggle are equal, the turned frames are the flip of the frames before the call byte for byte, and the statistics agree.
On the closed shapes the count of rows against the analytic outward normal is 0 after the ``top`` anchor.
"""
import numpy as np
import pytest

import orient_exact as oe
import voronoi_exact as ve

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(gpu):
    h = gpu["capi"].Handle(0)
    yield {"h": h, "capi": gpu["capi"], "PointCloud": gpu["PointCloud"]}
    h.close()


def torus():
    return ve.table_clouds()[0]


def sphere():
    return ve.fibonacci_sphere(ve.SPHERE_N)


def plant(h, pts, k, eps=None, algo=None, view_first=None):
    """pct_curvature, pct_point_frames: the frames before the call and the table they were made from."""
    n = len(pts)
    h.set_points(pts)
    h.curvature(*((k, eps or 0.0) if algo is None else (k, eps or 0.0, algo)))
    h.point_frames(view_first)
    before = h.get_point_frames(0, n)
    idx, _, cnt = h.get_neighbors(0, n, True, False, True)
    return before, idx, (cnt if eps else None)


def orient(h, pts, before, idx, cnt, anchor="top", viewpoint=None, max_components=None, name=""):
    """pct_orient_frames on what ``plant`` left, held to the restatement.  Returns (frames after, restatement, statistics)."""
    n = len(pts)
    N0, k0, d0, f0 = before
    h.orient_frames(anchor, viewpoint, max_components)
    after = h.get_point_frames(0, n)
    comp, parent, level, toggled = h.get_orientation(0, n)
    stats = h.orient_stats()
    ref = oe.orient(N0, idx, cnt, anchor, points=pts, viewpoint=viewpoint, max_components=max_components)
    print(f"{name}: {stats}")
    assert comp.dtype == parent.dtype == level.dtype == np.int32 and toggled.dtype == np.uint8
    assert np.array_equal(comp, ref["component"]), (name, int((comp != ref["component"]).sum()))
    assert np.array_equal(parent, ref["parent"]), (name, int((parent != ref["parent"]).sum()))
    assert np.array_equal(level, ref["level"]), name
    assert np.array_equal(toggled, ref["toggled"]), (name, int((toggled != ref["toggled"]).sum()))
    t = toggled.astype(bool)
    want = oe.apply(N0, k0, d0, f0, toggled)
    assert after[0].tobytes() == np.where(t[:, None], -N0, N0).tobytes(), name
    for got, exp in zip(after, want):
        assert got.tobytes() == exp.tobytes(), name
    assert np.array_equal(after[3], f0 ^ toggled)
    rs = ref["stats"]
    assert (stats["valid"], stats["components"], stats["unlabelled"], stats["toggled"]) == \
        (rs["valid"], rs["components"], rs["unlabelled"], rs["toggled"]), (name, stats, rs)
    assert (stats["levels"], stats["pulls"]) == (rs["levels"], rs["pulls"]), (name, stats, rs)
    assert stats["valid"] == int((~np.isnan(N0).any(1)).sum()) and stats["toggled"] == int(t.sum())
    assert stats["launches"] > 0 and 0 < stats["waits"] < stats["launches"] and stats["ms"] > 0
    oe.check_tree(ref, N0, idx, cnt)
    return after, ref, stats


def run(dev, pts, k, eps=None, algo=None, view_first=None, name="", **kw):
    before, idx, cnt = plant(dev["h"], pts, k, eps, algo, view_first)
    after, ref, stats = orient(dev["h"], pts, before, idx, cnt, name=name, **kw)
    return before, idx, cnt, after, ref, stats


# ---- the closed-form table: 0 rows against the outward normal, on the device's own normals ----------------------------------
TABLE = {
    "torus-k16": (torus, 16, oe.torus_outward),
    "torus-k30": (torus, 30, oe.torus_outward),
    "torus-k50": (torus, 50, oe.torus_outward),
    "egg-k30": (lambda: ve.table_clouds()[1], 30, lambda p: np.tile([0.0, 0.0, 1.0], (len(p), 1))),
    "sphere-k8": (sphere, 8, lambda p: p.astype(np.float64)),
    "sphere-k30": (sphere, 30, lambda p: p.astype(np.float64)),
    "sphere-k200": (sphere, 200, lambda p: p.astype(np.float64)),
    "two-spheres-k16": (oe.two_spheres, 16, oe.two_spheres_outward),
}


@pytest.mark.parametrize("name", list(TABLE))
def test_closed_form_table(dev, name):
    make, k, outward = TABLE[name]
    pts = make()
    before, idx, cnt, after, ref, stats = run(dev, pts, k, name=name)
    out = outward(pts)
    wrong_before, wrong_after = oe.against(before[0], out), oe.against(after[0], out)
    print(f"{name}: {wrong_before} of {len(pts)} rows against the outward normal before, {wrong_after} after")
    assert stats["valid"] == len(pts) and stats["unlabelled"] == 0 and stats["pulls"] == 0
    assert stats["components"] == (2 if name.startswith("two") else 1)
    assert wrong_after == 0 and wrong_before > 0.2 * len(pts)
    if name == "sphere-k200":
        assert idx.shape[1] == 200


def test_pull_round_reaches_the_outliers(dev):
    pts = oe.sphere_with_outliers()
    n = len(pts) - 2
    before, idx, cnt, after, ref, stats = run(dev, pts, 16, name="outliers-k16")
    assert not (idx[:n] >= n).any()
    assert stats["pulls"] >= 1 and stats["components"] == 1 and stats["unlabelled"] == 0
    assert oe.against(after[0][:n], pts[:n].astype(np.float64)) == 0


def test_eps_rows_nan_rows_and_several_components(dev):
    make, k, eps = ve.CASES["hybrid-k8"]
    pts = make()
    before, idx, cnt, after, ref, stats = run(dev, pts, k, eps, name="hybrid-k8")
    nan = np.isnan(before[0]).any(1)
    assert nan.any() and (cnt < k).any() and stats["components"] > 1 and stats["valid"] == int((~nan).sum())
    comp = dev["h"].get_orientation(0, len(pts))[0]
    assert (comp[nan] == -1).all() and np.isnan(after[0][nan]).all()
    # a cap below the number of components: the rest stays untouched
    cap = stats["components"] // 2
    before, idx, cnt, after, ref, capped = run(dev, pts, k, eps, name="hybrid-k8-capped", max_components=cap)
    assert capped["components"] == cap and capped["unlabelled"] > 0


@pytest.mark.parametrize("name", ["offset64-k30", "doubled-k16"])
def test_float64_cloud_and_coinciding_twins(dev, name):
    make, k, eps = ve.CASES[name]
    pts = make()
    before, idx, cnt, after, ref, stats = run(dev, pts, k, name=name)
    assert stats["unlabelled"] == 0
    if name == "offset64-k30":
        assert pts.dtype == np.float64 and stats["components"] == 1
        assert oe.against(after[0], pts - ve.F64_OFFSET) == 0


def test_nine_points(dev):
    """n = k + 1: every row lists every other point; one level."""
    pts = ve.fibonacci_sphere(9)
    before, idx, cnt, after, ref, stats = run(dev, pts, 8, name="sphere-9-k8")
    assert stats["valid"] == 9 and stats["components"] == 1 and stats["levels"] == 1 and stats["unlabelled"] == 0


def test_max_components_leaves_the_second_sphere(dev):
    pts = oe.two_spheres()
    before, idx, cnt, after, ref, stats = run(dev, pts, 16, name="two-spheres-one-component", max_components=1)
    a = oe.TWO_N[0]
    comp, parent, level, toggled = dev["h"].get_orientation(0, len(pts))
    assert stats["components"] == 1 and stats["unlabelled"] == oe.TWO_N[1]
    assert (comp[:a] == 0).all() and (comp[a:] == -1).all() and (parent[a:] == -1).all() and (level[a:] == -1).all()
    assert not toggled[a:].any()
    for got, was in zip(after, before):
        assert got[a:].tobytes() == was[a:].tobytes()


def test_frames_with_a_viewpoint_first(dev):
    pts = torus()
    view = (0.3, -0.2, 5.0)
    before, idx, cnt, after, ref, stats = run(dev, pts, 30, view_first=view, name="torus-view-first")
    assert before[3].any() and oe.against(after[0], oe.torus_outward(pts)) == 0
    plain = run(dev, pts, 30, name="torus-k30")[3]
    assert np.array_equal(plain[0], after[0]) and np.array_equal(plain[3], after[3])     # the same surface, the same side


def test_all_three_anchors(dev):
    pts = oe.two_spheres()
    h = dev["h"]
    got = {}
    for anchor, view in (("seed", None), ("top", None), ("view", (0.0, 0.0, 0.0)), ("view", (1.5, 40.0, 0.0))):
        before, idx, cnt, after, ref, stats = run(dev, pts, 16, anchor=anchor, viewpoint=view, name=f"two-spheres-{anchor}")
        got[(anchor, view)] = after[0]
    out = oe.two_spheres_outward(pts)
    a = oe.TWO_N[0]
    inside = got[("view", (0.0, 0.0, 0.0))]
    assert oe.against(-inside[:a], out[:a]) == 0           # seen from its centre, the first sphere's normals point inward
    assert oe.against(got[("top", None)], out) == 0
    for key, normal in got.items():                         # every anchor: one side per component
        for rows in (slice(0, a), slice(a, None)):
            assert oe.against(normal[rows], out[rows]) in (0, len(out[rows])), key
    h.orient_frames(dev["capi"].ORIENT_SEED)               # the anchor by its value; a second call on turned frames turns nothing
    assert h.orient_stats()["toggled"] == 0


def test_every_sweep_gives_the_same_orientation(dev):
    """Public order (the exhaustive sweep) against table-row order (the uniform cell list, the hierarchical list)."""
    capi = dev["capi"]
    pts = torus()
    base = None
    for algo in (capi.KNN_BRUTE, capi.KNN_GRID, capi.KNN_TREE):
        before, idx, cnt, after, ref, stats = run(dev, pts, 30, algo=algo, name=f"torus-k30-algo{algo}")
        got = (idx,) + tuple(after) + dev["h"].get_orientation(0, len(pts))
        if base is None:
            base = got
            continue
        for a, w in zip(got, base):
            assert np.array_equal(a, w), algo


# ---- errors and state ------------------------------------------------------------------------------------------------------
def test_error_paths(dev):
    h = dev["h"]
    pts = ve.fibonacci_sphere(500)
    h.set_points(pts)
    h.knn(8)
    h.fit()
    with pytest.raises(ValueError, match="no point frames"):
        h.orient_frames()
    with pytest.raises(ValueError, match="no orientation"):
        h.get_orientation(0, len(pts))
    assert h.orient_stats()["valid"] == 0
    h.point_frames()
    with pytest.raises(ValueError, match="viewpoint"):
        h.orient_frames("view")
    with pytest.raises(ValueError, match="viewpoint"):
        h.orient_frames("view", (0.0, np.nan, 0.0))
    with pytest.raises(ValueError, match="anchor"):
        h.orient_frames(7)
    with pytest.raises(ValueError):
        h.orient_frames("up")
    h.orient_frames("seed")
    first = h.get_orientation(0, len(pts))
    assert h.orient_stats()["valid"] == len(pts)
    with pytest.raises(ValueError):
        h.get_orientation(0, len(pts) + 1)
    part = h.get_orientation(100, 200)
    for a, w in zip(part, first):
        assert np.array_equal(a, w[100:200])
    h.point_frames()                                       # new frames drop it
    with pytest.raises(ValueError, match="no orientation"):
        h.get_orientation(0, len(pts))
    h.orient_frames("seed")
    h.knn(8)                                               # so does a planting
    with pytest.raises(ValueError):
        h.get_orientation(0, len(pts))
    assert h.orient_stats()["valid"] == 0
    # an owned range
    h.set_points(pts)
    h.set_query_range(0, 100)
    h.curvature(8, 0.0)
    h.point_frames()
    with pytest.raises(ValueError, match="whole cloud"):
        h.orient_frames()
    h.set_points(pts)


def test_class_surface(dev, tmp_path):
    PointCloud = dev["PointCloud"]
    pts = torus()
    pc = PointCloud(points=pts, normals=np.zeros((len(pts), 0)))
    with pytest.raises(AttributeError):
        pc.orient_normals_consistently()                   # needs plant_kdtree
    pc.plant_kdtree(30)
    K, H = pc.compute_pointwise_explicit_quadratic_curvature()
    normals = pc.orient_normals_consistently()
    assert normals is pc.normals and oe.against(normals, oe.torus_outward(pts)) == 0
    assert pc.last_orientation_stats["components"] == 1 and pc.last_orientation_stats["unlabelled"] == 0
    assert pc.normal_components.dtype == np.int32 and not pc.normal_components.any()
    assert pc.normals_flipped.dtype == bool and pc.normals_flipped.sum() == pc.last_orientation_stats["toggled"]
    assert np.array_equal(pc.H_signed_quadratic, np.where(pc.normals_flipped, -H, H)) and pc.H_signed_quadratic.dtype == np.float32
    # signed against the outward normal, the mean curvature of this torus is negative on its outer half
    outer = np.hypot(pts[:, 0], pts[:, 1]) > 1.15
    assert (pc.H_signed_quadratic[outer] < 0).all() and not (H[outer] < 0).all()
    # against the handle's own calls
    h = dev["h"]
    h.set_points(pts)
    h.knn(30)
    h.fit()
    h.point_frames()
    h.orient_frames("top")
    hn, hk, hd, hf = h.get_point_frames(0, len(pts))
    Hh = h.get_fit(0, len(pts), coefs=False, K=False, H2=False)[2]
    assert np.array_equal(hn, pc.normals) and np.array_equal(hk[:, 0], pc.k1_quadratic) and np.array_equal(hk[:, 1], pc.k2_quadratic)
    assert np.array_equal(hd, pc.principal_directions_quadratic)
    assert np.array_equal(np.where(hf.astype(bool), -Hh, Hh).astype(np.float32), pc.H_signed_quadratic)
    # the frames and the export serve the oriented values
    assert np.array_equal(pc.compute_surface_frames()[0], normals)
    pc.compute_normals()
    assert np.array_equal(pc.normals, normals)
    out = tmp_path / "oriented.ply"
    pc.export_ply_with_curvature_and_normals(str(out))
    text = out.read_text().split("\n")
    back = np.loadtxt(out, skiprows=text.index("end_header") + 1)
    assert np.array_equal(back.astype(np.float32), np.column_stack([pts, normals.astype(np.float32), K, H]))
    pc.plant_kdtree(16)                                    # a new planting: frames and orientation are computed again
    again = pc.orient_normals_consistently(anchor="view", viewpoint=(0.0, 0.0, 50.0))
    assert again.shape == normals.shape and pc.last_orientation_stats["components"] == 1
    pc.close()

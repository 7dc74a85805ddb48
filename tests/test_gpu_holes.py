"""Boundary loops and hole filling on the device (pct_fill_holes, include/pct_hip_holes.h; csrc/pct_hole.hip) against
``hole_exact`` applied to the device's OWN fans and triangles (pct_get_point_fans, pct_get_triangles): patches, filled array,
loops, status and statistics bit for bit, no tolerance, no row left out -- what a fan row's last bits decided is an input
here, not something compared.  tests/test_hole_exact.py pins the restatement."""
import math

import numpy as np
import pytest

import fan_exact as fe
import hole_exact as he
import voronoi_exact as ve

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(gpu):
    h = gpu["capi"].Handle(0)
    yield {"h": h, "capi": gpu["capi"], "PointCloud": gpu["PointCloud"]}
    h.close()


def fans_of(h, n):
    off, nbr = h.get_point_fans(0, n)
    return [nbr[off[i]:off[i + 1]].tolist() for i in range(n)]


def bundle(h):
    """Everything pct_fill_holes leaves, as bytes."""
    st = h.fill_hole_stats()
    off, verts, status = h.get_boundary_loops()
    return dict(patches=h.get_hole_triangles(), filled=h.get_filled_triangles(), off=off, verts=verts, status=status,
                stats={k: v for k, v in st.items() if k != "ms"}, ms=st["ms"])


def same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("patches", "filled", "off", "verts", "status")) and a["stats"] == b["stats"]


def hold(name, h, pts, fans, tri, max_vertices, max_perimeter):
    """One pct_fill_holes on the state in place, held to the restatement on the device's fans and triangles."""
    h.fill_holes(max_vertices, max_perimeter)
    got = bundle(h)
    want = he.fill(pts, fans, tri, max_vertices, max_perimeter)
    woff, wverts = he.loops_csr(want["loops"])
    print(f"{name} max_vertices={max_vertices} max_perimeter={max_perimeter}: device {got['stats']} {got['ms']:.3f} ms; restatement {want['stats']}, "
          f"{want['rejected']} walks rejected")
    assert got["stats"] == want["stats"], name
    assert got["off"].dtype == np.int64 and got["verts"].dtype == np.int32 and got["status"].dtype == np.uint8
    assert np.array_equal(got["off"], woff) and np.array_equal(got["verts"], wverts) and np.array_equal(got["status"], want["status"]), name
    assert got["patches"].dtype == np.int32 and got["patches"].tobytes() == want["patches"].tobytes(), name
    assert got["filled"].tobytes() == want["filled"].tobytes(), name
    # properties, whatever the restatement says
    filled = got["filled"]
    keys = filled.tolist()
    assert keys == sorted(keys), (name, "ascending")
    assert keys == sorted(tri.tolist() + got["patches"].tolist()), (name, "the sorted union")
    assert len({frozenset(t) for t in keys}) == len(keys), (name, "no duplicate")
    assert max(he.edge_count(filled).values(), default=0) <= 2, (name, "faces per edge")
    assert np.array_equal(h.get_triangles(), tri), (name, "the triangles are untouched")
    assert got["ms"] > 0
    return got, want


def planted(h, capi, name):
    make, k, eps = fe.CASES[name]
    pts = make()
    n = len(pts)
    h.set_points(pts)
    h.knn(k, eps or 0.0, capi.KNN_GRID if n > 64 else capi.KNN_BRUTE)
    h.point_triangles()
    return pts, fans_of(h, n), h.get_triangles()


@pytest.mark.parametrize("name", list(fe.CASES))
def test_exact_equality_with_the_restatement(dev, name):
    """Every cloud of fe.CASES -- the float64, the hybrid-count and the coinciding-point ones too --, without a cap and
    under the default one (finite against infinite max_perimeter)."""
    h, capi = dev["h"], dev["capi"]
    pts, fans, tri = planted(h, capi, name)
    n = len(pts)
    open_, want = hold(name, h, pts, fans, tri, 32, math.inf)
    assert open_["stats"]["perimeter"] == 0
    assert open_["stats"]["boundary_edges"] == h.point_triangle_stats()["boundary_edges"]
    capped, _ = hold(name, h, pts, fans, tri, 32, he.default_max_perimeter(pts))
    assert capped["stats"]["loops"] == open_["stats"]["loops"]
    assert capped["stats"]["filled"] + capped["stats"]["perimeter"] + capped["stats"]["blocked"] == capped["stats"]["loops"]
    closed = {"sphere-k20": 2 * n - 4, "torus-k20": 2 * n, "fib400-k200": 2 * n - 4}
    if name in closed:
        make, k, eps = fe.CASES[name]
        idx, _, _ = h.get_neighbors(0, n, True, False, False)
        ref = fe.rows(pts, idx)
        if np.array_equal(tri, fe.triangles(ref["corners"])):     # the device's triangles are the restatement's
            assert len(open_["filled"]) == closed[name] and he.boundary_edges(open_["filled"]) == 0
        else:
            print(name, "the device's triangles differ from the restatement's: the closed-surface count is not held")
    if name == "n13-k12":
        assert open_["stats"]["filled"] == 0 and len(open_["patches"]) == 0 and np.array_equal(open_["filled"], tri)
    if name == "egg-k20":
        assert he.boundary_edges(open_["filled"]) > 0             # the rim stays open


def test_the_vertex_cap(dev):
    """sphere-k8 has loops of every length up to 32, a blocked loop and many rejected walks: the cap at 3, 4, 31 and 32."""
    h, capi = dev["h"], dev["capi"]
    pts, fans, tri = planted(h, capi, "sphere-k8")
    longest = {}
    for mv in (3, 4, 31, 32):
        got, want = hold("sphere-k8", h, pts, fans, tri, mv, math.inf)
        lens = np.diff(got["off"])
        longest[mv] = int(lens.max())
        assert lens.min() >= 3 and lens.max() <= mv
        assert want["rejected"] > 0
    assert longest[3] == 3 and longest[4] == 4
    if any(len(l) == 32 for l in he.fill(pts, fans, tri, 32, math.inf)["loops"]):
        assert longest[31] == 31 and longest[32] == 32            # the 32-loop flips from rejected to filled
        off, verts, status = h.get_boundary_loops()
        assert (status[np.diff(off) == 32] == he.FILLED).all()
    assert h.fill_hole_stats()["blocked"] >= 1


def test_two_calls_and_two_plantings_give_the_same_bytes(dev):
    h, capi = dev["h"], dev["capi"]
    pts = ve.table_clouds(2000)[0]
    out = []
    for algo in (capi.KNN_BRUTE, capi.KNN_GRID):
        h.set_points(pts)
        h.knn(20, 0.0, algo)
        h.point_triangles()
        h.fill_holes(32, math.inf)
        first = bundle(h)
        h.fill_holes(32, math.inf)
        assert same(first, bundle(h))
        out.append(first)
    assert same(out[0], out[1]) and out[0]["stats"]["filled"] > 0


def snapshot(h, n):
    return [x.tobytes() for x in (*h.get_point_areas(0, n), *h.get_fit(0, n), *h.get_point_frames(0, n), *h.get_orientation(0, n),
                                  *h.get_neighbors(0, n, True, True, True), h.get_triangles(), *h.get_point_fans(0, n))]


def test_state_rules(dev):
    capi, h = dev["capi"], dev["h"]
    lib = h._lib
    INVALID = capi.PCT_ERR_INVALID
    pts = ve.random_sphere(600, seed=4)
    n = len(pts)
    one = np.zeros(3, np.int32)
    off2 = np.zeros(2, np.int64)
    inf = math.inf

    def fill(mv=32, mp=inf, flags=0):
        return lib.pct_fill_holes(h._h, mv, mp, flags)

    def no_results():
        st = h.fill_hole_stats()
        return lib.pct_get_hole_triangles(h._h, 0, 0, one.ctypes.data_as(capi._i32p)) == INVALID and \
            lib.pct_get_filled_triangles(h._h, 0, 0, one.ctypes.data_as(capi._i32p)) == INVALID and \
            lib.pct_get_boundary_loops(h._h, off2.ctypes.data_as(capi._i64p), None, None) == INVALID and \
            all(v == 0 for v in st.values())

    h.set_points(pts)
    assert fill() == INVALID and b"no triangles" in lib.pct_last_error(h._h) and no_results()
    h.set_query_range(0, n // 2)                              # an owned range: refused as an unsupported state
    h.knn(12)
    assert fill() == INVALID and b"owns rows" in lib.pct_last_error(h._h) and no_results()
    h.set_query_range(0, n)
    h.knn(12)
    assert fill() == INVALID and b"no triangles" in lib.pct_last_error(h._h)
    h.point_triangles()
    assert no_results()                                       # triangles, and nothing filled yet
    for bad in ((2, inf, 0), (33, inf, 0), (32, 0.0, 0), (32, -1.0, 0), (32, math.nan, 0), (32, -inf, 0), (32, inf, 1)):
        assert fill(*bad) == INVALID and no_results(), bad
    # the call touches nothing else on the handle
    h.fit()
    h.point_areas()
    h.point_frames()
    h.orient_frames("top")
    before, timed = snapshot(h, n), h.timings()
    h.fill_holes(32, inf)
    first = bundle(h)
    assert first["stats"]["filled"] > 0 and first["stats"]["patch_triangles"] == len(first["patches"])
    assert h.timings() == timed
    assert snapshot(h, n) == before
    # every refusal leaves the residents and the hole results untouched
    for bad in ((2, inf, 0), (33, inf, 0), (32, 0.0, 0), (32, math.nan, 0), (32, inf, 2)):
        assert fill(*bad) == INVALID, bad
    assert lib.pct_get_hole_triangles(h._h, 0, len(first["patches"]) + 1, one.ctypes.data_as(capi._i32p)) == INVALID
    assert lib.pct_get_filled_triangles(h._h, -1, 1, one.ctypes.data_as(capi._i32p)) == INVALID
    assert same(first, bundle(h)) and snapshot(h, n) == before
    # a fit, pct_point_frames, pct_orient_frames and pct_voxel_downsample drop neither the triangles nor the hole results
    h.fit()
    h.point_frames((0.0, 0.0, 0.0))
    h.orient_frames("seed")
    h.voxel_downsample(pts, 0.5)
    assert same(first, bundle(h))
    h.fill_holes(4, inf)                                      # ... and the call still works behind a lost table
    assert h.fill_hole_stats()["filled"] <= first["stats"]["filled"]
    h.fill_holes(32, inf)
    assert same(first, bundle(h))
    # a new pct_point_triangles drops them (the triangles it leaves have not been filled)
    h.knn(12)
    h.point_triangles()
    h.fill_holes(32, inf)
    assert same(first, bundle(h))
    h.point_triangles()
    assert no_results() and len(h.get_triangles()) > 0
    # ... a replanting, a change of ownership and a new cloud too
    h.fill_holes(32, inf)
    h.knn(12)
    assert no_results()
    h.point_triangles()
    h.fill_holes(32, inf)
    h.set_query_range(0, n)
    assert no_results()
    h.knn(12)
    h.point_triangles()
    h.fill_holes(32, inf)
    assert same(first, bundle(h))
    h.set_points(pts)
    assert no_results()
    # a slab handle
    big = ve.random_sphere(4096, seed=2)
    h.set_points(big)
    h.set_query_slab(0, 1)
    assert fill() == INVALID and b"slab" in lib.pct_last_error(h._h)
    h.set_query_slab(0, 0)


def parse_face_count(path):
    with open(path, "rb") as f:
        head = f.read(4096).decode(errors="replace").split("end_header")[0]
    return next(int(l.split()[2]) for l in head.split("\n") if l.startswith("element face"))


def test_class_surface(dev, tmp_path):
    pts = ve.random_sphere(1500, seed=1)
    n = len(pts)
    pc = dev["PointCloud"](points=pts, normals=np.zeros((n, 0)))
    pc.plant_kdtree(20)
    pc.compute_pointwise_explicit_quadratic_curvature()
    open_faces = pc.compute_surface_triangles().copy()
    area_open = pc.compute_mesh_energies()[2]
    filled = pc.fill_surface_holes(max_perimeter=math.inf)
    assert filled is pc.faces and len(pc.faces) == 2 * n - 4
    st = pc.last_hole_stats
    assert st["patch_triangles"] == len(pc.hole_faces) == len(pc.faces) - len(open_faces) and st["filled"] == st["loops"] > 0
    off, verts, status = pc.boundary_loops
    assert len(off) == st["loops"] + 1 and off[-1] == len(verts) and (status == 0).all()
    area_filled = pc.compute_mesh_energies()[2]
    print("area", area_open, "->", area_filled, "of", 4 * math.pi)
    assert area_open < area_filled < 4 * math.pi
    path = tmp_path / "filled.ply"
    pc.export_ply_with_curvature_and_normals(str(path))
    assert parse_face_count(str(path)) == len(pc.faces) == 2 * n - 4
    # update_faces=False leaves ``faces``; the default cap; a later compute_surface_triangles restores the unfilled faces
    assert np.array_equal(pc.compute_surface_triangles(), open_faces)
    kept = pc.fill_surface_holes(update_faces=False)
    assert np.array_equal(pc.faces, open_faces) and len(kept) == len(open_faces) + pc.last_hole_stats["patch_triangles"]
    assert pc.last_hole_stats["filled"] + pc.last_hole_stats["perimeter"] == st["loops"]
    with pytest.raises(ValueError):
        pc.fill_surface_holes(max_vertices=33)
    pc.close()
    # the faces are computed first where they are missing
    pc2 = dev["PointCloud"](points=pts, normals=np.zeros((n, 0)))
    pc2.plant_kdtree(20)
    assert len(pc2.fill_surface_holes(max_perimeter=math.inf)) == 2 * n - 4 and pc2.last_triangle_stats["triangles"] == len(open_faces)
    pc2.close()

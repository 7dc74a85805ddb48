"""The NumPy restatement of the fans, corners and triangles (tests/fan_exact.py) pinned on its own, on the CPU: against
scipy's Delaunay triangulation of the projected block, under a turn of the in-plane basis, and in what it produces --
at most two faces per edge, the winding, the coverage DESIGN 4.3k quotes, the share of undecided rows on every cloud
tests/test_gpu_triangles.py compares exactly."""
import numpy as np
import pytest
from scipy.spatial import Delaunay

import fan_exact as fe
import voronoi_exact as ve


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, (make, k, eps) in fe.CASES.items():
        pts = make()
        r = ve.knn_rows(pts, k, eps)
        idx, cnt = r if eps else (r, None)
        ref = fe.rows(pts, idx, cnt)
        out[name] = (pts, idx, cnt, ref, fe.triangles(ref["corners"]))
    return out


@pytest.mark.parametrize("name", ["sphere-k20", "torus-k20", "egg-k20", "sphere-k8"])
def test_closed_rows_are_the_delaunay_neighbours(cases, name):
    pts, idx, cnt, ref, _ = cases[name]
    checked = 0
    for i in np.flatnonzero(ref["closed"] & ref["decided"])[::3]:
        ab = np.asarray(ve.frame_oracle(pts[idx[i]] - pts[i]), np.float64)
        tri = Delaunay(np.concatenate([np.zeros((1, 2)), ab]))
        ptr, nb = tri.vertex_neighbor_vertices
        want = sorted(int(idx[i, j - 1]) for j in nb[ptr[0]:ptr[1]])
        fan = ref["fan"][i]
        assert sorted(fan) == want, (name, i)
        assert ref["corners"][i] == [(fan[v - 1], fan[v]) for v in range(len(fan))], (name, i)      # taken consecutively
        checked += 1
    assert checked > 100


@pytest.mark.parametrize("name", ["sphere-k20", "sphere-k8", "egg-k20"])
def test_corners_do_not_depend_on_the_basis(cases, name):
    pts, idx, cnt, ref, _ = cases[name]
    turned = fe.rows(pts, idx, cnt, turn=0.7)
    rows = np.flatnonzero(ref["decided"] & turned["decided"] & ~ref["nan"])
    assert (~ref["closed"][rows]).any() or name == "sphere-k20"            # open rows among them
    for i in rows:
        assert fe.cyclic(ref["corners"][i]) == fe.cyclic(turned["corners"][i]), (name, i)


def test_no_edge_has_more_than_two_faces(cases):
    for name, (pts, idx, cnt, ref, tri) in cases.items():
        assert max((len(v) for v in fe.edge_faces(tri).values()), default=0) <= 2, name


def test_winding_on_the_sphere(cases):
    pts, idx, cnt, ref, _ = cases["sphere-k20"]
    p = pts.astype(np.float64)
    flipped = np.zeros(len(pts), bool)                           # all normals outward: flipped where the row's +z points inward
    for i in range(len(pts)):
        rot = np.asarray(ve.oracle.plane_align(pts[idx[i]] - pts[i]))
        # the first two columns are the in-plane coordinates: the rotation's +z is the direction the third column measures
        q = (pts[idx[i]] - pts[i]).astype(np.float64)
        nz = np.linalg.lstsq(q, rot[:, 2], rcond=None)[0]
        flipped[i] = nz @ p[i] < 0
    tri = fe.triangles(ref["corners"], flipped)
    a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    assert ((np.cross(b - a, c - a) * (a + b + c)).sum(1) > 0).all()
    assert all(len(v) < 2 or v[0] == v[1][::-1] for v in fe.edge_faces(tri).values())


def test_coverage(cases):
    """The figures DESIGN 4.3k quotes, measured again: triangles against the 2 n - 4 of a closed surface, boundary edges."""
    shown = {}
    for name in ("sphere-k20", "sphere-k8", "torus-k20", "egg-k20", "fib400-k200"):
        pts, idx, cnt, ref, tri = cases[name]
        boundary = sum(1 for v in fe.edge_faces(tri).values() if len(v) == 1)
        shown[name] = (len(pts), len(tri), boundary, int((~ref["closed"] & ~ref["nan"]).sum()))
        print(name, "points, triangles, boundary edges, open rows:", shown[name])
    assert shown["sphere-k20"] == (1500, 2892, 196, 1)
    assert shown["torus-k20"] == (2000, 3790, 398, 5)
    assert shown["egg-k20"] == (1500, 2842, 210, 82)
    assert shown["fib400-k200"] == (400, 792, 8, 0)
    assert shown["sphere-k8"][1:] == (1746, 1360, 428)


def test_undecided_share(cases):
    for name, (pts, idx, cnt, ref, _) in cases.items():
        share = ref["undecided"].sum() / len(pts)
        print(name, "undecided", int(ref["undecided"].sum()), "of", len(pts), "; no assertion covers", int((~ref["decided"]).sum()))
        if name in fe.CONCURRENT:
            assert share > fe.UNDECIDED_CAP                       # (why the device test holds properties only there)
        else:
            assert share <= fe.UNDECIDED_CAP, (name, share)

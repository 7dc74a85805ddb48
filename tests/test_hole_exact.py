"""The NumPy restatement of the boundary loops and the hole filling (tests/hole_exact.py) pinned on its own, on the CPU, over
the restatement's own fans and triangles (tests/fan_exact.py, the clouds of fe.CASES): the figures DESIGN 4.3l quotes, what
the filled surface is (closed where the cloud is, manifold, wound as its surroundings), the dynamic programme against the
enumeration of every triangulation, and the independence of the fans' direction."""
import math

import numpy as np
import pytest

import fan_exact as fe
import hole_exact as he
import voronoi_exact as ve


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, (make, k, eps) in fe.CASES.items():
        pts = make()
        r = ve.knn_rows(pts, k, eps)
        idx, cnt = r if eps else (r, None)
        ref = fe.rows(pts, idx, cnt)
        tri = fe.triangles(ref["corners"])
        out[name] = dict(pts=pts, idx=idx, fans=ref["fan"], corners=ref["corners"], tri=tri, fill=he.fill(pts, ref["fan"], tri, 32, math.inf))
    return out


# case -> (loops filled, patch triangles, triangles after, boundary edges before, after, area before, after)
TABLE = {
    "sphere-k20": (46, 104, 2996, 196, 0, 11.181, 12.515),
    "torus-k20": (94, 210, 4000, 398, 0, 11.526, 13.090),
    "fib400-k200": (2, 4, 796, 8, 0, None, None),
    "offset64-k20": (219, 578, 2982, 1016, 0, 10.155, 12.517),
    "egg-k20": (27, 65, None, 210, 91, None, None),
}


@pytest.mark.parametrize("name", list(TABLE))
def test_the_table_of_figures(cases, name):
    c = cases[name]
    f, st = c["fill"], c["fill"]["stats"]
    filled, patches, after, b0, b1, a0, a1 = TABLE[name]
    n = len(c["pts"])
    print(name, st, "rejected walks", f["rejected"], "triangles", len(c["tri"]), "->", len(f["filled"]))
    assert (st["filled"], st["patch_triangles"], st["boundary_edges"]) == (filled, patches, b0)
    assert he.boundary_edges(f["filled"]) == b1
    assert len(f["filled"]) == len(c["tri"]) + patches
    if after is not None:
        assert len(f["filled"]) == after
    if a0 is not None:
        assert round(he.mesh_area(c["pts"], c["tri"]), 3) == a0 and round(he.mesh_area(c["pts"], f["filled"]), 3) == a1
        assert a1 < 4 * math.pi or name == "torus-k20"
    # the closed surfaces: 2 n - 4 on the spheres, 2 n on the torus
    closed = {"sphere-k20": 2 * n - 4, "torus-k20": 2 * n, "fib400-k200": 2 * n - 4}
    if name in closed:
        assert len(f["filled"]) == closed[name] and st["blocked"] == 0 and st["odd_gaps"] == 0 and f["rejected"] == 0


def test_the_edge_case_inputs(cases):
    """The sparse clouds: loops of every length up to the cap, a blocked loop on each, rejected walks; the rim of the open
    surface stays open; the cloud of thirteen points has nothing to fill."""
    for name in ("sphere-k8", "hybrid-k8"):
        f = cases[name]["fill"]
        print(name, f["stats"], "rejected", f["rejected"], sorted({len(l) for l in f["loops"]}))
        assert f["stats"]["blocked"] == 1 and f["rejected"] > 12
    assert {len(l) for l in cases["sphere-k8"]["fill"]["loops"]} >= {3, 4, 5, 31, 32}
    egg = cases["egg-k20"]["fill"]
    assert egg["rejected"] > 0 and egg["stats"]["blocked"] == 0
    small = cases["n13-k12"]["fill"]
    assert small["stats"]["filled"] == 0 and small["stats"]["loops"] == 0 and small["rejected"] > 0 and len(small["patches"]) == 0
    assert np.array_equal(small["filled"], cases["n13-k12"]["tri"])


def test_the_filled_surface_stays_manifold(cases):
    for name, c in cases.items():
        f = c["fill"]
        assert max(he.edge_count(f["filled"]).values(), default=0) <= 2, name
        keys = [frozenset(t) for t in f["filled"].tolist()]
        assert len(set(keys)) == len(keys) and all(len(k) == 3 for k in keys), name
        assert f["filled"].tolist() == sorted(f["filled"].tolist()) and f["patches"].tolist() == sorted(f["patches"].tolist()), name
        assert len(f["patches"]) == 0 or (f["patches"][:, 0] < f["patches"][:, 1:].min(1)).all(), name
        # every filled loop is gone from the boundary, every other one is still there
        edges = he.edge_count(f["filled"])
        for loop, status in zip(f["loops"], f["status"]):
            want = 2 if status == he.FILLED else 1
            for x, y in zip(loop, loop[1:] + loop[:1]):
                assert edges[(min(x, y), max(x, y))] == want, (name, loop)
            assert loop[0] == min(loop) and loop[1] < loop[-1], (name, loop)


def test_the_programme_finds_the_least_total(cases):
    """Against every triangulation enumerated as a tree and summed in the tree's order, for every loop of up to 7 vertices
    (42 triangulations); blocked loops have no triangulation of finite total."""
    checked = blocked = 0
    for name, c in cases.items():
        f = c["fill"]
        faces = he.edge_count(c["tri"])
        resident = {frozenset(t) for t in c["tri"].tolist()}
        p = np.asarray(c["pts"], np.float64)
        for loop, status, total in zip(f["loops"], f["status"], f["totals"]):
            if len(loop) > 7:
                continue
            least, count = he.brute_force_minimum(p[loop], he.forbidden(loop, faces, resident))
            assert count == (1, 2, 5, 14, 42)[len(loop) - 3]
            assert total == least, (name, loop, total, least)
            assert (status == he.BLOCKED) == (not math.isfinite(least))
            checked += 1
            blocked += status == he.BLOCKED
    print("loops checked", checked, "of them blocked", blocked)
    assert checked > 400 and blocked > 50


def test_reversed_fans_give_the_same_bytes(cases):
    for name in ("sphere-k20", "sphere-k8", "egg-k20", "hybrid-k8"):
        c = cases[name]
        mirrored = he.fill(c["pts"], [f[::-1] for f in c["fans"]], c["tri"], 32, math.inf)
        assert mirrored["patches"].tobytes() == c["fill"]["patches"].tobytes(), name
        # (the loops are listed by fan position: two loops through one lowest vertex change places, nothing else)
        listed = lambda f: sorted(zip(f["loops"], f["status"].tolist()))
        assert listed(mirrored) == listed(c["fill"]), name
        assert mirrored["stats"] == c["fill"]["stats"], name


def test_patches_are_wound_as_their_surroundings(cases):
    c = cases["sphere-k20"]
    pts, idx = c["pts"], c["idx"]
    p = pts.astype(np.float64)
    flipped = np.zeros(len(pts), bool)                           # all normals outward (test_fan_exact.test_winding_on_the_sphere)
    for i in range(len(pts)):
        rot = np.asarray(ve.oracle.plane_align(pts[idx[i]] - pts[i]))
        q = (pts[idx[i]] - pts[i]).astype(np.float64)
        nz = np.linalg.lstsq(q, rot[:, 2], rcond=None)[0]
        flipped[i] = nz @ p[i] < 0
    tri = fe.triangles(c["corners"], flipped)
    f = he.fill(pts, c["fans"], tri, 32, math.inf)
    assert len(f["patches"]) == 104 and len(f["filled"]) == 2 * len(pts) - 4
    for t in (f["patches"], f["filled"]):
        a, b, cc = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]
        assert ((np.cross(b - a, cc - a) * (a + b + cc)).sum(1) > 0).all()
    ef = fe.edge_faces(f["filled"])
    assert all(len(v) == 2 and v[0] == v[1][::-1] for v in ef.values())
    # the same triangles as sets, whichever way the faces were wound
    assert {frozenset(t) for t in f["patches"].tolist()} == {frozenset(t) for t in c["fill"]["patches"].tolist()}


def test_no_perimeter_sits_on_the_default_cap(cases):
    """A condition on the inputs: the device's square root may differ from NumPy's in the last bit, which must not move a
    loop across the cap the device test compares under."""
    eps = np.finfo(np.float64).eps
    for name, c in cases.items():
        cap = he.default_max_perimeter(c["pts"])
        per = c["fill"]["perimeters"]
        if len(per):
            assert (np.abs(per - cap) > 8 * eps * cap).all(), name
        capped = he.fill(c["pts"], c["fans"], c["tri"], 32, cap)
        print(name, "cap", cap, "left for the perimeter", capped["stats"]["perimeter"], "of", capped["stats"]["loops"])
        assert capped["stats"]["loops"] == c["fill"]["stats"]["loops"]
        assert capped["stats"]["perimeter"] == int((per >= cap).sum())

"""The CPU restatement of the consistent orientation (tests/orient_exact.py): its invariants, its independence of the labelling
and of the input signs, and the closed-form table -- on the patch normals (-D, -E, 1) / w of frame_exact.reference over the
oracle's rows and fit.  No GPU.

Rows against the analytic outward normal, before (the fit's own far-minus-near sides) and after the ``top`` anchor; measured
with the patch normals:

    torus k = 16         3 448 of 4 000 -> 0     1 component, 28 levels
    torus k = 30         3 414 of 4 000 -> 0     1 component, 20 levels
    torus k = 50         3 434 of 4 000 -> 0     1 component, 15 levels
    sphere k = 8         2 000 of 2 000 -> 0     1 component, 30 levels
    sphere k = 30        2 000 of 2 000 -> 0     1 component, 14 levels
    sphere k = 200       2 000 of 2 000 -> 0     1 component,  5 levels
    two spheres k = 16   1 600 of 1 600 -> 0     2 components, 25 levels
    egg carton k = 30    2 027 of 4 000 -> 0     1 component, 22 levels   (against +z; smallest |cos| to +z 0.953)

(levels: push levels that labelled a row, summed over the components.  The spheres' fits all choose the inward side: the
far-minus-near rule of pct:286-297 on a convex surface.)
"""
import functools

import numpy as np
import pytest

import frame_exact as fe
import orient_exact as oe
import pct_oracle as oracle
import voronoi_exact as ve

CLOUDS = {
    "torus-k16": (lambda: ve.table_clouds()[0], 16),
    "torus-k30": (lambda: ve.table_clouds()[0], 30),
    "torus-k50": (lambda: ve.table_clouds()[0], 50),
    "sphere-k8": (lambda: ve.fibonacci_sphere(ve.SPHERE_N), 8),
    "sphere-k30": (lambda: ve.fibonacci_sphere(ve.SPHERE_N), 30),
    "sphere-k200": (lambda: ve.fibonacci_sphere(ve.SPHERE_N), 200),
    "two-spheres-k16": (oe.two_spheres, 16),
    "egg-k30": (lambda: ve.table_clouds()[1], 30),
    "outliers-k16": (oe.sphere_with_outliers, 16),
}
TABLE = ("torus-k16", "torus-k30", "torus-k50", "sphere-k8", "sphere-k30", "sphere-k200", "two-spheres-k16", "egg-k30")


def outward(name, pts):
    if name.startswith("torus"):
        return oe.torus_outward(pts)
    if name.startswith("two"):
        return oe.two_spheres_outward(pts)
    if name.startswith("egg"):
        return np.tile([0.0, 0.0, 1.0], (len(pts), 1))
    return pts.astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(name):
    """(points, idx, unoriented patch normals, the orientation under ``top``), once per session."""
    make, k = CLOUDS[name]
    pts = make()
    idx = ve.knn_rows(pts, k)
    coefs = oracle.curvature_batched(pts, idx)[0]
    N0 = fe.reference(pts, idx, None, coefs, detail=False)["normal"]
    return pts, idx, N0, oe.orient(N0, idx, anchor=oe.TOP, points=pts)


@pytest.mark.parametrize("name", TABLE)
def test_closed_form_table(name):
    pts, idx, N0, res = case(name)
    out = outward(name, pts)
    rows = len(pts)
    N1 = np.where(res["toggled"][:, None].astype(bool), -N0, N0)
    before, after = oe.against(N0, out), oe.against(N1, out)
    with np.errstate(invalid="ignore"):
        cos = np.abs((N0 * out).sum(1)) / np.linalg.norm(out, axis=1)
    s = res["stats"]
    print(f"{name}: {before} of {rows} rows against the outward normal before, {after} after; {s['components']} components, "
          f"{s['levels']} levels, {s['pulls']} pull rounds, {s['unlabelled']} unlabelled; smallest |cos| {np.nanmin(cos):.3f}")
    assert not np.isnan(N0).any() and s["valid"] == rows and s["unlabelled"] == 0
    assert s["components"] == (2 if name.startswith("two") else 1)
    assert after == 0
    assert before > 0.2 * rows                      # the fit's own sides: what the call is for


def test_pull_round_reaches_the_outliers():
    pts, idx, N0, res = case("outliers-k16")
    n = len(pts) - 2
    assert not (idx[:n] >= n).any() and (idx[n:] < n).any()            # nothing points at them, they point at the sphere
    s = res["stats"]
    assert s["components"] == 1 and s["pulls"] == 1 and s["unlabelled"] == 0
    assert (res["parent"][n:] >= 0).all() and (res["parent"][n:] < n).all()
    N1 = np.where(res["toggled"][:, None].astype(bool), -N0, N0)
    assert oe.against(N1[:n], pts[:n].astype(np.float64)) == 0


@pytest.mark.parametrize("name", list(CLOUDS))
def test_tree_invariants(name):
    pts, idx, N0, res = case(name)
    kids = oe.check_tree(res, N0, idx)
    assert kids == res["stats"]["valid"] - res["stats"]["components"] - res["stats"]["unlabelled"]
    assert oe.seed_toggles(res, N0)
    seeded = oe.orient(N0, idx, anchor=oe.SEED)
    for c in range(seeded["stats"]["components"]):
        assert seeded["toggled"][np.flatnonzero(seeded["component"] == c)[0]] == 0         # the seed: the lowest index, toggle 0
    for key in ("component", "parent", "level"):
        assert np.array_equal(seeded[key], res[key])


@pytest.mark.parametrize("name", ["torus-k16", "two-spheres-k16", "outliers-k16"])
def test_relabelling_keeps_the_partition(name):
    """A permutation of the cloud that keeps row 0: the same partition into components (ids follow the lowest index)."""
    pts, idx, N0, res = case(name)
    n = len(pts)
    rng = np.random.default_rng(7)
    perm = np.r_[0, 1 + rng.permutation(n - 1)]               # new row i is old row perm[i]
    inv = np.argsort(perm)
    got = oe.orient(N0[perm], inv[idx[perm]], anchor=oe.TOP, points=pts[perm])
    comp_old = res["component"][perm]
    pairs = set(zip(comp_old.tolist(), got["component"].tolist()))
    assert len(pairs) == res["stats"]["components"] == got["stats"]["components"]
    assert np.array_equal(got["component"] < 0, comp_old < 0)
    oe.check_tree(got, N0[perm], inv[idx[perm]])


@pytest.mark.parametrize("name", ["torus-k30", "two-spheres-k16", "sphere-k8"])
def test_input_signs_do_not_matter(name):
    """Half of the input normals negated: the same oriented normals, up to one sign per component under ``seed``; the
    same normals outright under ``top``."""
    pts, idx, N0, res = case(name)
    neg = np.random.default_rng(11).random(len(pts)) < 0.5
    Nn = np.where(neg[:, None], -N0, N0)
    for anchor in (oe.SEED, oe.TOP):
        a = oe.orient(N0, idx, anchor=anchor, points=pts)
        b = oe.orient(Nn, idx, anchor=anchor, points=pts)
        for key in ("component", "parent", "level"):
            assert np.array_equal(a[key], b[key])
        Na = np.where(a["toggled"][:, None].astype(bool), -N0, N0)
        Nb = np.where(b["toggled"][:, None].astype(bool), -Nn, Nn)
        for c in range(a["stats"]["components"]):
            rows = a["component"] == c
            same, opposite = np.array_equal(Na[rows], Nb[rows]), np.array_equal(Na[rows], -Nb[rows])
            assert same or (anchor == oe.SEED and opposite), (name, anchor, c)


def test_limits_and_invalid_rows():
    pts, idx, N0, res = case("two-spheres-k16")
    one = oe.orient(N0, idx, anchor=oe.TOP, points=pts, max_components=1)
    a = oe.TWO_N[0]
    assert one["stats"]["components"] == 1 and one["stats"]["unlabelled"] == oe.TWO_N[1]
    assert (one["component"][:a] == 0).all() and (one["component"][a:] == -1).all() and not one["toggled"][a:].any()
    assert np.array_equal(one["toggled"][:a], res["toggled"][:a])
    # NaN rows are never labelled and never parents
    Nn = N0.copy()
    dead = np.arange(0, len(pts), 7)
    Nn[dead] = np.nan
    got = oe.orient(Nn, idx, anchor=oe.TOP, points=pts)
    assert (got["component"][dead] == -1).all() and not got["toggled"][dead].any() and got["stats"]["valid"] == len(pts) - len(dead)
    assert not np.isin(got["parent"], dead).any()
    oe.check_tree(got, Nn, idx)
    # the viewpoint anchor: from the centre of the first sphere its normals point inward, the second sphere's to the viewpoint's side
    view = oe.orient(N0, idx, anchor=oe.VIEW, points=pts, viewpoint=(0.0, 0.0, 0.0))
    Nv = np.where(view["toggled"][:, None].astype(bool), -N0, N0)
    out = oe.two_spheres_outward(pts)
    assert oe.against(-Nv[:a], out[:a]) == 0
    with pytest.raises(ValueError):
        oe.orient(N0, idx, anchor=5)


def test_apply_is_the_frames_flip():
    rng = np.random.default_rng(3)
    normal, k12, dirs = rng.normal(size=(6, 3)), rng.normal(size=(6, 2)), rng.normal(size=(6, 3, 2))
    flipped = np.array([0, 1, 0, 1, 0, 1], np.uint8)
    t = np.array([1, 1, 0, 0, 1, 0], np.uint8)
    n1, k1, d1, f1 = oe.apply(normal, k12, dirs, flipped, t)
    for i in range(6):
        if t[i]:
            n, a, b, e1, e2 = fe.flip(list(normal[i]), k12[i, 0], k12[i, 1], list(dirs[i, :, 0]), list(dirs[i, :, 1]))
        else:
            n, a, b, e1, e2 = normal[i], k12[i, 0], k12[i, 1], dirs[i, :, 0], dirs[i, :, 1]
        assert np.array_equal(n1[i], n) and (k1[i, 0], k1[i, 1]) == (a, b)
        assert np.array_equal(d1[i, :, 0], e1) and np.array_equal(d1[i, :, 1], e2)
    assert np.array_equal(f1, flipped ^ t)

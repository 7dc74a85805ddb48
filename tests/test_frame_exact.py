"""The CPU restatement of the surface frames (tests/frame_exact.py): its bars re-measured, its identities with the fit's K and
H, a closed form, the viewpoint's effect on the sign of H, planted defects, and the PLY writer.  No GPU."""
import functools
import math

import numpy as np
import pytest

import frame_exact as fe
import pct_oracle as oracle
import voronoi_exact as ve


def fit_rows(pts, idx, count=None):
    """The oracle's coefficients of the rows: the batched restatement, or -- rows of every length -- pct:644-647 row by row."""
    if count is None:
        return oracle.curvature_batched(pts, idx)[0]
    coefs = np.full((len(idx), 6), np.nan, np.float32)
    for i in range(len(idx)):
        m = int(count[i])
        if m >= 2:
            with np.errstate(all="ignore"):
                coefs[i] = oracle.quadric_fit(oracle.plane_align(pts[idx[i, :m]] - pts[i]))
    return coefs


@functools.lru_cache(maxsize=None)
def case(name):
    """(points, idx, count, coefs, reference) of one case, on the oracle's rows and fit; computed once per session."""
    make, k, eps = ve.CASES[name]
    pts = make()
    idx, count = (ve.knn_rows(pts, k), None) if eps is None else ve.knn_rows(pts, k, eps)
    coefs = fit_rows(pts, idx, count)
    return pts, idx, count, coefs, fe.reference(pts, idx, count, coefs)


def test_rotation_is_plane_align():
    pts, idx, _, _, _ = case("torus-k16")
    for i in range(0, len(pts), 400):
        assert fe.rotation_is_plane_align(pts[idx[i]] - pts[i])


# ---- the bars, measured again on every run ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def needs(name):
    pts, idx, count, coefs, ref = case(name)
    return fe.measure_need(pts, idx, count, coefs, ref=ref)


@pytest.mark.parametrize("name", list(ve.CASES))
def test_needs_per_case(name):
    pts, idx, count, coefs, ref = case(name)
    need_k, need_n, need_d, taken = needs(name)
    c = fe.compare(ref["normal"], ref["k"], ref["dirs"], ref["flipped"], ref)
    live = int((~np.isnan(ref["k"][:, 0])).sum())
    print(f"{name}: {taken} rows taken a second way: k needs {need_k:.2f}, normal {need_n:.2f}, directions {need_d:.2f}; "
          f"{int(c['left_out'].sum())} of {live} rows left out of the normal, {int(c['gap_out'].sum())} more of the directions; "
          f"invariants {c['share_invariant'] * fe.ORTHO_EPS:.1f} eps")
    assert need_k <= fe.C_K_NEEDED and need_n <= fe.C_N_NEEDED and need_d <= fe.C_D_NEEDED
    fe.assert_frames(name, c)                      # the reference against itself: the invariants, on every row
    m = len(pts)
    assert c["left_out"].sum() <= ve.LEFT_OUT_CAP * m
    if name in ("sphere-k8", "sphere-k30", "sphere-k200", "torus-k30", "torus-k16", "egg-k30", "doubled-k16"):
        assert c["left_out"].sum() <= 0.01 * m and c["gap_out"].sum() <= 0.01 * m
    if name in ("ring-k80", "lattice-k8"):          # flat: no curvature, no direction, the normal along z exactly
        assert not ref["k"].any() and ref["umbilic"].all() and c["gap_out"].all()
        assert np.array_equal(ref["normal"], np.tile([0.0, 0.0, 1.0], (m, 1)))


def test_constants_are_the_measured_needs():
    for i, (name, needed) in enumerate((("C_K", fe.C_K_NEEDED), ("C_N", fe.C_N_NEEDED), ("C_D", fe.C_D_NEEDED))):
        measured = max(needs(case_name)[i] for case_name in ve.CASES)
        print(f"{name}_NEEDED = {needed:g}: measured {measured:.2f}")
        assert 0.5 * needed <= measured <= needed
    assert (fe.C_K, fe.C_N, fe.C_D) == (4 * fe.C_K_NEEDED, 4 * fe.C_N_NEEDED, 4 * fe.C_D_NEEDED)


# ---- tr S = 2H, det S = K: the fit's float32 curvatures of the same rows -------------------------------------------------------
# measured 2.73e-7 (sphere-k8) and 3.61e-7 (sphere-k30), rounded up, over the five curved cases: float32 rounding of pct:403-419, not an error of the frames
H_IDENTITY, K_IDENTITY = 4 * 2.7e-7, 4 * 3.7e-7


@pytest.mark.parametrize("name", ["torus-k30", "egg-k30", "sphere-k30", "sphere-k8", "torus-k16"])
def test_identities_with_the_fit(name):
    _, _, _, coefs, ref = case(name)
    K, H, _ = oracle._curv_f32(coefs)
    k1, k2 = ref["k"][:, 0], ref["k"][:, 1]
    kmax = np.maximum(np.abs(k1), np.abs(k2))
    eh = np.abs((k1 + k2) / 2 - H) / np.maximum(np.abs(H), kmax)
    ek = np.abs(k1 * k2 - K) / np.maximum(np.abs(K), kmax * kmax)
    print(f"{name}: |(k1 + k2) / 2 - H| <= {eh.max():.2e}, |k1 k2 - K| <= {ek.max():.2e}")
    assert eh.max() <= H_IDENTITY and ek.max() <= K_IDENTITY


# ---- a closed form ------------------------------------------------------------------------------------------------------
QUADRIC = (0.8, -0.3, 0.4)


def quadric_cloud(dtype):
    """1 500 random points on z = 0.8 a^2 - 0.3 b^2 + 0.4 ab, |a|, |b| < 0.25, the origin as row 0, under a fixed rotation."""
    rng = np.random.default_rng(99)
    ab = rng.uniform(-0.25, 0.25, (1500, 2))
    ab[0] = 0.0
    A, B, C = QUADRIC
    local = np.column_stack([ab, A * ab[:, 0] ** 2 + B * ab[:, 1] ** 2 + C * ab[:, 0] * ab[:, 1]])
    axis, angle = np.array([0.48, -0.6, 0.64]), 1.1
    kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    G = np.eye(3) + math.sin(angle) * kx + (1 - math.cos(angle)) * kx @ kx
    return (local @ G.T).astype(dtype), G


def quadric_truth(G):
    A, B, C = QUADRIC
    k, v = np.linalg.eigh(np.array([[2 * A, C], [C, 2 * B]]))
    return G[:, 2], k[1], k[0], G[:, :2] @ v[:, 1], G[:, :2] @ v[:, 0]


# what the restatement needs on the oracle's rows and fit of this cloud -- the fit's truncation error, not rounding: normal
# 1.45e-5 (k = 100), k1 / k2 7.54e-4 (k = 8), directions 3.40e-5 (k = 8)
CLOSED_N, CLOSED_K, CLOSED_D = 4 * 1.45e-5, 4 * 7.54e-4, 4 * 3.40e-5


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("k", [8, 30, 100])
def test_quadric_patch_at_the_origin(k, dtype):
    pts, G = quadric_cloud(dtype)
    idx = ve.knn_rows(pts, k)[:1]
    coefs = oracle.curvature_batched(pts, idx, rows=np.array([0]))[0]
    n, k1, k2, d1, d2 = quadric_truth(G)
    ref = fe.reference(pts, idx, None, coefs, viewpoint=10.0 * n, rows=np.array([0]))
    en = np.abs(ref["normal"][0] - n).max()
    ek = max(abs(ref["k"][0, 0] - k1), abs(ref["k"][0, 1] - k2))
    ed = max(fe.ee.up_to_sign(ref["dirs"][0, :, 0], d1), fe.ee.up_to_sign(ref["dirs"][0, :, 1], d2))
    print(f"k = {k} {np.dtype(dtype).name}: normal {en:.2e}, k1 / k2 {ek:.2e}, directions {ed:.2e}")
    assert en <= CLOSED_N and ek <= CLOSED_K and ed <= CLOSED_D


# ---- the viewpoint ---------------------------------------------------------------------------------------------------------
def egg_H(pts, amp=0.1):
    """Mean curvature of z = amp sin(pi x) cos(pi y) against the upward normal (closed form)."""
    x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    s, c, sy, cy = np.sin(np.pi * x), np.cos(np.pi * x), np.sin(np.pi * y), np.cos(np.pi * y)
    fx, fy = amp * np.pi * c * cy, -amp * np.pi * s * sy
    fxx = fyy = -amp * np.pi ** 2 * s * cy
    fxy = -amp * np.pi ** 2 * c * sy
    return ((1 + fx * fx) * fyy - 2 * fx * fy * fxy + (1 + fy * fy) * fxx) / (2 * (1 + fx * fx + fy * fy) ** 1.5)


def egg_rows(pts):
    H = egg_H(pts)
    return (np.abs(pts[:, 0]) < 0.85) & (np.abs(pts[:, 1]) < 0.85) & (np.abs(H) > 0.05 * np.abs(H).max()), H


def test_viewpoint_above_the_egg_carton_signs_H():
    pts, idx, _, coefs, plain = case("egg-k30")
    H_fit = oracle._curv_f32(coefs)[1]
    ref = fe.reference(pts, idx, None, coefs, viewpoint=(0.0, 0.0, 1e3))
    flipped = ref["flipped"].astype(bool)
    assert (ref["normal"][:, 2] > 0).all() and (plain["normal"][flipped][:, 2] < 0).all()
    rows, H = egg_rows(pts)
    H_signed = np.where(flipped, -H_fit, H_fit)
    wrong, wrong_plain = int((np.sign(H_signed) != np.sign(H))[rows].sum()), int((np.sign(H_fit) != np.sign(H))[rows].sum())
    print(f"egg carton: {int(rows.sum())} interior rows with |H| above 5 % of its maximum: {wrong} signs wrong with the viewpoint, {wrong_plain} without")
    assert int(rows.sum()) == 2593 and wrong == 0 and wrong_plain == 1279
    # H and k1, k2 are signed against the same normal
    assert (np.sign((ref["k"][:, 0] + ref["k"][:, 1])[rows]) == np.sign(H_signed[rows])).all()
    # the flip is the documented one
    n, k, d = fe.unflip(ref["normal"], ref["k"], ref["dirs"], flipped)
    assert np.array_equal(n, plain["normal"]) and np.array_equal(k, plain["k"]) and np.array_equal(d, plain["dirs"])


def test_viewpoint_inside_the_sphere():
    pts, idx, _, coefs, _ = case("sphere-k30")
    ref = fe.reference(pts, idx, None, coefs, viewpoint=(0.0, 0.0, 0.0))
    H = oracle._curv_f32(coefs)[1]
    assert (np.where(ref["flipped"].astype(bool), -H, H) > 0).all() and (ref["k"][:, 1] > 0).all()
    assert ((ref["normal"] * pts).sum(1) < 0).all()


# ---- the bars have teeth ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", fe.DEFECTS)
def test_planted_defects_fail_a_bar(defect):
    pts, idx, _, coefs, _ = case("egg-k30")
    rows = np.arange(0, len(pts), 10)
    view = (0.0, 0.0, 1e3)
    ref = fe.reference(pts, idx[rows], None, coefs[rows], viewpoint=view, rows=rows)
    bad = fe.reference(pts, idx[rows], None, coefs[rows], viewpoint=view, rows=rows, defect=defect, detail=False)
    c = fe.compare(bad["normal"], bad["k"], bad["dirs"], bad["flipped"], ref)
    failed = {w: int(c[w].sum()) for w in ("bad_k", "bad_normal", "bad_dirs", "bad_flipped", "bad_invariant") if c[w].any()}
    print(defect, failed)
    assert failed, defect
    with pytest.raises(AssertionError):
        fe.assert_frames(defect, c)


def test_degenerate_rows_are_nan():
    pts, idx, _, coefs, _ = case("sphere-k8")
    coefs = coefs.copy()
    coefs[2, 3] = np.inf
    ref = fe.reference(pts, idx[:4], np.array([0, 1, 8, 8]), coefs[:4])
    assert np.isnan(ref["k"][:3]).all() and np.isnan(ref["normal"][:3]).all() and np.isnan(ref["dirs"][:3]).all()
    assert not ref["flipped"].any() and not np.isnan(ref["k"][3]).any()


def test_hybrid_rows():
    _, _, count, _, ref = case("hybrid-k8")
    assert np.array_equal(np.isnan(ref["k"][:, 0]), count < 2)


# ---- the PLY with normals (host code: no device) ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 1000])
def test_ply_with_normals_round_trips(built, tmp_path, n):
    capi = built["capi"]
    rng = np.random.default_rng(n)
    pts = rng.normal(size=(n, 3)).astype(np.float32)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    K, H = (rng.normal(size=n) * 10.0 ** rng.integers(-6, 6, n)).astype(np.float32), rng.normal(size=n).astype(np.float32)
    out = tmp_path / "frames.ply"
    capi.write_ply_ascii_normals(str(out), pts, nrm, K, H)
    lines = out.read_text().split("\n")
    header = ["ply", "format ascii 1.0", f"element vertex {n}", "property float x", "property float y", "property float z",
              "property float nx", "property float ny", "property float nz", "property float gaussian_curvature",
              "property float mean_curvature", "end_header"]
    assert lines[:len(header)] == header and lines[-1] == "" and len(lines) == len(header) + n + 1
    back = np.loadtxt(out, skiprows=len(header), ndmin=2)
    assert back.shape == (n, 8)
    assert np.array_equal(back.astype(np.float32), np.column_stack([pts, nrm, K, H]))
    with pytest.raises(ValueError):
        capi.write_ply_ascii_normals(str(out), pts, nrm[:-1], K, H)

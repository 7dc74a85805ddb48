"""Per-point surface frames from the quadric fit, the reference  --  TEST INFRASTRUCTURE ONLY (CPU, NumPy, no import of the package).

``pct_point_frames`` (include/pct_hip.h) gives every row of the resident neighbour table the unit normal of its fitted patch,
the principal curvatures k1 >= k2 and their directions.  ``reference`` states the definition again in float64, every product
and sum rounded on its own (Python floats: no fused multiply-add) in the order the kernel takes them, with the rotation R
taken from the reference's own route (np.cov + svd, orientation, Rodrigues: pct:270-312 as ``pct_oracle.plane_align``
walks it, ``rotation`` returns the 3 x 3 it builds):

  block   Q_j = points[idx[i, j]] - points[i], in the cloud's dtype (pct:641), j < count_i
  coefs   (A, B, C, D, E) of the row, float32 widened -- GIVEN, not fitted here
  patch   w = sqrt((1 + D D) + E E), m = (-D, -E, 1) / w;  g2 = 1 + D D, g = sqrt(g2), e1 = (1, 0, D) / g,
          e2 = (-D E, g2, E) / (g w)
  shape   II(x, y) = ((2A xa ya + C (xa yb + xb ya)) + 2B xb yb) / w;  s11 = II(e1, e1), s12 = II(e1, e2), s22 = II(e2, e2)
  k1, k2  h = (s11 + s22) / 2, d = (s11 - s22) / 2, r = sqrt(d d + s12 s12): h + r, h - r
  t1, t2  t = s12 / (|d| + r), cj = 1 / sqrt(t t + 1), sj = t cj, (c, s) = (cj, sj) where d > 0 else (sj, cj);
          t1 = c e1 + s e2, t2 = -s e1 + c e2;  r == 0: t1 = e1, t2 = e2 (umbilic)
  world   n = R^T m, d1 = R^T t1, d2 = R^T t2, component i = (R[0][i] v0 + R[1][i] v1) + R[2][i] v2;  d1, d2 under the sign
          rule (largest component positive, the first among equals)
  view    ((vx - px) n0 + (vy - py) n1) + (vz - pz) n2 < 0: n <- -n, (k1, k2) <- (-k2, -k1), (d1, d2) <- (d2, d1), flipped
  NaN     count_i < 2, a rotation or coefficient that is not finite: every output NaN, flipped 0

The bars, in the project's idiom, with u = voronoi_exact.bar_units(voronoi_exact.facts(block))[1] =
eps l1 / gap3 (1 + (1 - c) / s), infinite under rules (1), (2) and (3):

    k1, k2          C_K eps max(|k1|, |k2|)           (they depend on the coefficients alone, not on R)
    normal          C_N u, componentwise
    d1, d2          up to sign, C_D (u + eps max|k| / (k1 - k2)); only where k1 - k2 >= GAP_MIN max|k|
    flipped         only where |(v - p) . n| > C_N u |v - p|
    every row that is no NaN, without exception:  |n| = |d1| = |d2| = 1 and n . d1 = n . d2 = d1 . d2 = 0 within 16 eps

Each C_NEEDED is measured on the CPU, never against the GPU: ``measure_need`` takes the rows a second way -- the exactly
rounded rotation of eig_exact.exact_align, the generalised eigenproblem II x = k I x of the two fundamental forms through
Cholesky and eigh -- over the clouds of voronoi_exact.CASES; the committed bar is 4 x the need.  Measured on every row;
tests/test_frame_exact.py re-measures on every 8th row on every run (4.98, 30.6, 17.4 there) and asserts
0.5 C_NEEDED <= measured <= C_NEEDED:

    C_K_NEEDED = 8     measured 5.39  (Fibonacci sphere, k = 200; every case lies between 3.9 and 5.4)
    C_N_NEEDED = 36    measured 35.1  (egg carton, k = 30; torus k = 30 29.5, sphere k = 200 26.3)
    C_D_NEEDED = 28    measured 25.9  (egg carton, k = 30; torus 19.7; spheres, whose k1 - k2 is small, about 2)

The restatement's own invariants stay within 6 eps on every row of every case.
"""
import math

import numpy as np

import eig_exact as ee
import pct_oracle as oracle
import voronoi_exact as ve

EPS64 = 2.0 ** -52
GAP_MIN = 1e-6
ORTHO_EPS = 16.0
C_K_NEEDED, C_N_NEEDED, C_D_NEEDED = 8.0, 36.0, 28.0
C_K, C_N, C_D = 4 * C_K_NEEDED, 4 * C_N_NEEDED, 4 * C_D_NEEDED
MEASURE_STRIDE = 8

DEFECTS = ("plane_normal", "no_w", "R_not_RT", "no_swap", "no_negate")


def rotation(block):
    """The 3 x 3 of pct:270-312 (np.cov + svd, far-minus-near flip, Rodrigues), operation for operation as
    pct_oracle.plane_align builds it: ``rotation(b) @ b.T`` is plane_align(b).T, bit for bit."""
    nbrs = np.asarray(block)
    cov = np.cov(nbrs, rowvar=False)
    n = np.linalg.svd(cov, full_matrices=True)[2][-1]
    ref = nbrs[-1] - nbrs[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        if np.dot(n / np.linalg.norm(n), ref / np.linalg.norm(ref)) < 0:
            n = -n
    a = n / np.linalg.norm(n)
    z = np.array([0, 0, 1])
    v = np.cross(a, z)
    c = np.dot(a, z)
    s = np.linalg.norm(v)
    if s == 0:
        return np.eye(3)
    kx = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + kx + kx.dot(kx) * ((1 - c) / (s ** 2))


def rotation_is_plane_align(block):
    """``rotation`` against the oracle on one block: the rotated block, bit for bit."""
    return np.array_equal(np.dot(rotation(block), np.asarray(block).T).T, oracle.plane_align(block))


def sign_rule(v):
    big = v[0]
    if abs(v[1]) > abs(big):
        big = v[1]
    if abs(v[2]) > abs(big):
        big = v[2]
    return [-v[0], -v[1], -v[2]] if big < 0.0 else v


def flip(n, k1, k2, d1, d2):
    return [-x for x in n], -k2, -k1, d2, d1


def frame_of(R, coefs, p=None, viewpoint=None, defect=None):
    """One row from its rotation (3 x 3) and coefficients: (n, k1, k2, d1, d2, flipped, umbilic), or None for a NaN row.
    ``defect``: one of DEFECTS, planted (tests only)."""
    R = [[float(x) for x in row] for row in np.asarray(R, np.float64)]
    A, B, C, D, E = (float(x) for x in np.asarray(coefs, np.float32)[:5].astype(np.float64))
    if not all(math.isfinite(x) for row in R for x in row) or not all(math.isfinite(x) for x in (A, B, C, D, E)):
        return None
    g2 = 1.0 + D * D
    w, g = math.sqrt(g2 + E * E), math.sqrt(g2)
    m = [-D / w, -E / w, 1.0 / w]
    if defect == "plane_normal":
        m = [0.0, 0.0, 1.0]
    e1a, e1c = 1.0 / g, D / g
    gw = g * w
    e2a, e2b, e2c = (-(D * E)) / gw, g2 / gw, E / gw
    A2, B2 = 2.0 * A, 2.0 * B
    wd = 1.0 if defect == "no_w" else w

    def II(xa, xb, ya, yb):
        return ((A2 * xa * ya + C * (xa * yb + xb * ya)) + B2 * xb * yb) / wd

    s11, s12, s22 = II(e1a, 0.0, e1a, 0.0), II(e1a, 0.0, e2a, e2b), II(e2a, e2b, e2a, e2b)
    h, d = 0.5 * (s11 + s22), 0.5 * (s11 - s22)
    r = math.sqrt(d * d + s12 * s12)
    k1, k2 = h + r, h - r
    c, s = 1.0, 0.0
    if r != 0.0:
        t = s12 / (abs(d) + r)
        cj = 1.0 / math.sqrt(t * t + 1.0)
        sj = t * cj
        c, s = (cj, sj) if d > 0.0 else (sj, cj)
    t1 = [c * e1a + s * e2a, s * e2b, c * e1c + s * e2c]
    t2 = [(-s) * e1a + c * e2a, c * e2b, (-s) * e1c + c * e2c]

    def world(v):
        if defect == "R_not_RT":
            return [(R[i][0] * v[0] + R[i][1] * v[1]) + R[i][2] * v[2] for i in range(3)]
        return [(R[0][i] * v[0] + R[1][i] * v[1]) + R[2][i] * v[2] for i in range(3)]

    n, d1, d2 = world(m), sign_rule(world(t1)), sign_rule(world(t2))
    flipped = 0
    if viewpoint is not None:
        px, py, pz = (float(x) for x in p)
        vx, vy, vz = (float(x) for x in viewpoint)
        if ((vx - px) * n[0] + (vy - py) * n[1]) + (vz - pz) * n[2] < 0.0:
            flipped = 1
            n, k1, k2, d1, d2 = flip(n, k1, k2, d1, d2)
            if defect == "no_swap":
                d1, d2 = d2, d1
            if defect == "no_negate":
                k1, k2 = -k2, -k1
    return n, k1, k2, d1, d2, flipped, int(r == 0.0)


def second_patch(coefs):
    """The patch another way, for ``measure_need``: (m, k1, k2, t1, t2) in the rotated frame -- the principal curvatures and
    directions as the generalised eigenproblem II x = k I x of the two fundamental forms at the origin (Cholesky of I,
    eigh); directions up to sign."""
    A, B, C, D, E = np.asarray(coefs, np.float32)[:5].astype(np.float64)
    w = math.sqrt(1.0 + D * D + E * E)
    first = np.array([[1.0 + D * D, D * E], [D * E, 1.0 + E * E]])
    second = np.array([[2.0 * A, C], [C, 2.0 * B]]) / w
    Li = np.linalg.inv(np.linalg.cholesky(first))
    k, y = np.linalg.eigh(Li @ second @ Li.T)
    x = Li.T @ y                                            # columns: tangent vectors in (a, b) coordinates, ascending k
    T = np.array([[1.0, 0.0, D], [0.0, 1.0, E]]).T @ x      # ... in the rotated frame
    T /= np.sqrt((T * T).sum(0))
    return np.array([-D, -E, 1.0]) / w, float(k[1]), float(k[0]), T[:, 1], T[:, 0]


def second_route(block, coefs):
    """... and in the cloud's frame, through the exactly rounded rotation (eig_exact.exact_align): (n, k1, k2, d1, d2)
    without a viewpoint."""
    R = ee.exact_align(np.asarray(block))["R"]
    m, k1, k2, t1, t2 = second_patch(coefs)
    return R.T @ m, k1, k2, R.T @ t1, R.T @ t2


# ======================================================================================================================
# the reference
# ======================================================================================================================
def reference(points, idx, count, coefs, viewpoint=None, rows=None, detail=True, defect=None, rot=rotation):
    """Frames of the rows ``idx`` (M, k) about points[rows] (default: row i about point i), ``count`` valid entries each
    (None: k), ``coefs`` (M, >= 5) the rows' fit coefficients.  dict(normal (M, 3), k (M, 2), dirs (M, 3, 2), flipped uint8,
    umbilic uint8) -- with ``detail`` also unit (the bar unit u of every row, inf where the normal is not asserted), kmax,
    dot ((v - p) . n before the flip) and dist (|v - p|)."""
    points = np.asarray(points)
    idx = np.asarray(idx)
    M, k = idx.shape
    rows = np.arange(M) if rows is None else np.asarray(rows)
    count = np.full(M, k) if count is None else np.asarray(count)
    out = dict(normal=np.full((M, 3), np.nan), k=np.full((M, 2), np.nan), dirs=np.full((M, 3, 2), np.nan),
               flipped=np.zeros(M, np.uint8), umbilic=np.zeros(M, np.uint8))
    if detail:
        out.update(unit=np.full(M, np.inf), kmax=np.full(M, np.nan), dot=np.full(M, np.nan), dist=np.full(M, np.nan))
    for o in range(M):
        m = int(count[o])
        if m < 2:
            continue
        p = points[rows[o]]
        block = points[idx[o, :m]] - p                              # pct:641, the cloud's dtype
        try:
            with np.errstate(all="ignore"):
                R = rot(block)
        except (ValueError, np.linalg.LinAlgError):
            continue
        fr = frame_of(R, coefs[o], p, viewpoint, defect)
        if fr is None:
            continue
        n, k1, k2, d1, d2, flipped, umbilic = fr
        out["normal"][o] = n
        out["k"][o] = k1, k2
        out["dirs"][o, :, 0], out["dirs"][o, :, 1] = d1, d2
        out["flipped"][o], out["umbilic"][o] = flipped, umbilic
        if detail:
            with np.errstate(all="ignore"):
                out["unit"][o] = ve.bar_units(ve.facts(block))[1]
            out["kmax"][o] = max(abs(k1), abs(k2))
            if viewpoint is not None:
                dv = np.asarray(viewpoint, np.float64) - p.astype(np.float64)
                n0 = -np.asarray(n) if flipped else np.asarray(n)
                out["dot"][o], out["dist"][o] = float(dv @ n0), float(np.sqrt(dv @ dv))
    return out


def unflip(normal, k, dirs, which):
    """The flip is its own inverse: rows ``which`` of (normal, k, dirs) turned to the other side."""
    normal, k, dirs = normal.copy(), k.copy(), dirs.copy()
    normal[which] = -normal[which]
    k[which] = -k[which][:, ::-1]
    dirs[which] = dirs[which][:, :, ::-1]
    return normal, k, dirs


def invariants(normal, dirs):
    """Per row: the worst of | |n| - 1 |, | |d1| - 1 |, | |d2| - 1 |, |n . d1|, |n . d2|, |d1 . d2| in units of eps."""
    d1, d2 = dirs[:, :, 0], dirs[:, :, 1]
    with np.errstate(invalid="ignore"):
        parts = [np.abs(np.sqrt((v * v).sum(1)) - 1.0) for v in (normal, d1, d2)]
        parts += [np.abs((a * b).sum(1)) for a, b in ((normal, d1), (normal, d2), (d1, d2))]
    return np.max(parts, 0) / EPS64


def compare(got_normal, got_k, got_dirs, got_flipped, ref, c_k=C_K, c_n=C_N, c_d=C_D):
    """The device's (or a second route's) rows against ``reference(..., detail=True)``.  Returns dict of row masks --
    nan_differs, bad_k, bad_normal, bad_dirs, bad_flipped, bad_invariant (asserted and failed), left_out (rows no normal
    assertion covers: u infinite), gap_out (rows whose normal is asserted and whose directions are not: the k-gap) -- and
    the worst share of each bar: share_k, share_normal, share_dirs, share_invariant."""
    nan = np.isnan(ref["k"][:, 0])
    got_nan = np.isnan(got_k[:, 0])
    all_nan = np.isnan(got_normal).all(1) & np.isnan(got_k).all(1) & np.isnan(got_dirs).all((1, 2)) & (got_flipped == 0)
    any_nan = np.isnan(got_normal).any(1) | np.isnan(got_k).any(1) | np.isnan(got_dirs).any((1, 2))
    nan_differs = (nan != got_nan) | (got_nan & ~all_nan) | (~got_nan & any_nan)
    live = ~nan & ~nan_differs
    unit, kmax = ref["unit"], np.where(nan, 0.0, ref["kmax"])
    defined = live & np.isfinite(unit)
    u = np.where(np.isfinite(unit), unit, 0.0)
    # the side: asserted where the dot product clears the normal's own bar; elsewhere the row is taken to the reference's side
    with np.errstate(invalid="ignore"):
        decided = defined & (np.abs(ref["dot"]) > c_n * u * ref["dist"])
    differs = live & (got_flipped != ref["flipped"])
    bad_flipped = decided & differs
    normal, k, dirs = unflip(got_normal, got_k, got_dirs, differs & ~decided)
    with np.errstate(invalid="ignore", divide="ignore"):
        err_k = np.abs(k - ref["k"]).max(1)
        bar_k = c_k * EPS64 * kmax
        err_n = np.abs(normal - ref["normal"]).max(1)
        gap = ref["k"][:, 0] - ref["k"][:, 1]
        gap_ok = defined & (gap >= GAP_MIN * kmax) & (kmax > 0)
        err_d = np.maximum(*[np.minimum(np.abs(dirs[:, :, c] - ref["dirs"][:, :, c]).max(1), np.abs(dirs[:, :, c] + ref["dirs"][:, :, c]).max(1))
                             for c in range(2)])
        bar_d = c_d * (u + EPS64 * kmax / gap)
    bad_k = live & ~(err_k <= bar_k)
    bad_normal = defined & ~(err_n <= c_n * u)
    bad_dirs = gap_ok & ~(err_d <= bar_d)
    inv = invariants(got_normal, got_dirs)
    bad_invariant = ~got_nan & ~(inv <= ORTHO_EPS)

    def worst(err, bar, mask):
        with np.errstate(invalid="ignore", divide="ignore"):
            share = np.where(mask & (bar > 0), err / bar, np.where(mask & (err > 0), np.inf, 0.0))
        return float(share.max()) if len(share) else 0.0

    return dict(nan_differs=nan_differs, bad_k=bad_k, bad_normal=bad_normal, bad_dirs=bad_dirs, bad_flipped=bad_flipped,
                bad_invariant=bad_invariant, left_out=~nan & ~np.isfinite(unit), gap_out=defined & ~gap_ok,
                share_k=worst(err_k, bar_k, live), share_normal=worst(err_n, c_n * u, defined),
                share_dirs=worst(err_d, bar_d, gap_ok), share_invariant=float(np.where(got_nan, 0.0, inv).max()) / ORTHO_EPS if len(inv) else 0.0)


def assert_frames(name, c):
    """The assertions every comparison makes."""
    for what in ("nan_differs", "bad_invariant", "bad_k", "bad_normal", "bad_dirs", "bad_flipped"):
        assert not c[what].any(), (name, what, np.flatnonzero(c[what])[:8], {k: v for k, v in c.items() if k.startswith("share")})


def measure_need(points, idx, count, coefs, ref=None, stride=MEASURE_STRIDE):
    """The smallest (C_K, C_N, C_D) between ``reference`` and ``second_route`` on every stride-th row, 0 where the bar leaves
    the row out.  Returns (need_k, need_n, need_d, rows taken)."""
    ref = reference(points, idx, count, coefs) if ref is None else ref
    points = np.asarray(points)
    need_k = need_n = need_d = 0.0
    taken = 0
    for o in range(0, len(idx), stride):
        if np.isnan(ref["k"][o, 0]):
            continue
        m = idx.shape[1] if count is None else int(count[o])
        block = points[idx[o, :m]] - points[o]
        taken += 1
        u, kmax = ref["unit"][o], ref["kmax"][o]
        k1r, k2r = ref["k"][o]
        # (the curvatures need no rotation: rows the normal's bar leaves out are still held to theirs)
        n, k1, k2, d1, d2 = second_route(block, coefs[o]) if np.isfinite(u) else second_patch(coefs[o])
        if kmax > 0:
            need_k = max(need_k, max(abs(k1 - k1r), abs(k2 - k2r)) / (EPS64 * kmax))
        else:
            assert k1 == 0.0 and k2 == 0.0
        if not np.isfinite(u):
            continue
        need_n = max(need_n, float(np.abs(n - ref["normal"][o]).max()) / u)
        if kmax > 0 and k1r - k2r >= GAP_MIN * kmax:
            bar = u + EPS64 * kmax / (k1r - k2r)
            for got, want in ((d1, ref["dirs"][o, :, 0]), (d2, ref["dirs"][o, :, 1])):
                need_d = max(need_d, ee.up_to_sign(got, want) / bar)
    return need_k, need_n, need_d, taken

"""Exact ground truth for the 3 x 3 eigen stages  --  TEST INFRASTRUCTURE ONLY (CPU, stdlib + NumPy, no import of the package).

Three kernels run a symmetric 3 x 3 eigen-solve on a neighbourhood covariance: plane_rotation() (pct_fit.hip: the
tangent-plane normal, its orientation, the Rodrigues rotation; fed by k_fit's one-pass and k_plane_rotate's two-pass
moments), write_frame() (pct_pca.hip: l1, l2, two directions, K, H) and k_surface_variation (pct_aux.hip).  fit_exact.py
pinned the least-squares solve BEHIND the rotation; this module supplies a reference MORE precise than either side for
the stage in front of it:

* ``exact_cov``      the ddof-1 covariance of float32 / float64 points taken at face value, as ``Fraction``s;
* ``exact_eigen``    eigenvalues as roots of the rational characteristic cubic (monotone Newton steps in ``decimal`` from
                     both ends of the spectrum), eigenvectors from the largest cross product of two rows of A - lambda I;
* ``exact_align``    get_best_fit_plane_and_rotate (pct:270-321) from the stored values: normal, normalised orientation
                     dot (the reference vector subtracted in the input's dtype, pct:286), c, s, R*, and R* p rounded to
                     float64 and float32;
* ``exact_pca``      pct:901-950 on one neighbourhood: l1 >= l2 >= l3, the (3, 2) frame under the device's documented
                     sign rule, K, H;
* ``exact_surface_variation``   lmin / (sum + 1e-10), utils.py:822-828 as oracle.surface_variation restates it;
* seeded builders (``gap_ladder``, ``grading_ladder``, ``tilt_ladder``, ``dot_ladder``, ``shape_rungs``, ``identity_block``)
                     that walk what the stage is sensitive to, every block with its exact facts attached;
* ``emulate_align / emulate_pca``   the kernels' choreography in float64 Python, with switches for planted defects --
                     used to CALIBRATE and to prove that the bars have teeth, never as a bar.

The bars (eps = 2^-52; l1 >= l2 >= l3 the exact eigenvalues; gap3 = l2 - l3):

    eigenvalues, PCA H     C_VAL eps l1                    PCA K   C_VAL eps l1^2
    a direction, up to sign   C_VEC eps l1 / gap (its distance to the nearest other eigenvalue); the projector onto
                           span{v1, v2} and the normal use gap3
    rotated points         C_ROT eps (l1 / gap3) (1 + (1 - c) / s) |p|      -- the last factor is Rodrigues' own
                           sensitivity: near -z the rotation axis (a_y, -a_x, 0) / s turns by (error of the normal) / s
    surface variation      max(1 ulp32, C_VAL eps l1 / (sum + 1e-10))
    orientation            the flip equals the exact sign wherever |dot| > C_DOT (eps l1 / gap3 [+ 2^-23 for float32 input:
                           pct:290 normalises the float32 reference vector in float32])

Where the reference's answer is not a function of its input (rows left out of the respective assertion, COUNTED per rung;
tests assert that a rung not built to sit in such a zone loses at most 10 % of its rows):

    zone "gap"    gap below 1e-6 l1: the direction(s) belonging to it, and for gap3 everything that follows from the normal;
    zone "dot"    |dot| below its margin: the orientation, hence the rotation;
    zone "negz"   oriented normal within C_VEC eps l1 / gap3 of -z: which rotation by ~pi comes out (or the s == 0 identity)
                  is an accident of LAPACK's rounding; so is the sign of the rotated z, and with it the sign of H;
    (float32 rounding boundaries of exactly rotated coordinates: ``boundary_clear``, used by the fused-fit test; cap 1 %).
    The PCA frame has the same "gap" rule per direction (v1, v2, the projector): ``pca_shares(tally=)`` counts what it leaves out on
    the neighbourhoods the assertion really runs on, ``assert_pca_caps`` holds the 10 % on rungs outside the gap zones.

Constants.  Each C_NEEDED is what the REFERENCE'S OWN ROUTE needs against the exact value over the whole ladder
(``calibrate()``: np.cov + np.linalg.svd for the alignment, np.cov + eigh for PCA, the restatement in
oracle.surface_variation); the committed floor is 4 x C_NEEDED, for the same reason as in fit_exact.py: two backward-stable
methods (LAPACK there, cyclic Jacobi on the device) have different constants.  Measured on the CPU, never against the GPU;
tests/test_eig_exact.py re-measures them on every run and asserts 0.5 C_NEEDED <= measured <= C_NEEDED:

    C_VAL_NEEDED = 6     measured 5.0  (float64, tilt ladder 1 rad from -z, m = 300: an eigenvalue of np.cov + eigh)
    C_VEC_NEEDED = 24    measured 19.7 ) all three on ONE block -- float64, tilt ladder 0.1 from -z, m = 50 -- where gesdd's
    C_ROT_NEEDED = 24    measured 19.9 ) normal is 20 eps l1 / gap3 off; typical blocks need 1 to 3
    C_DOT_NEEDED = 24    measured 20.3 ) (the dot term is the error of the route's own dot product in units of its margin)

    The float64 emulation of the kernels needs, over the same 1 308 blocks: one-pass moments about the first neighbour
    (k_fit) val 3.5, vec 7.1, rot 6.4, dot 8.2; two-pass moments (k_plane_rotate, write_frame) val 3.5, vec 3.8, rot 1.4,
    dot 1.4; never more than 4 sweeps.  The exact bars (24 eps l1, 96 eps l1 / gap) are 200 and 50 000 times tighter than
    pca_restatement.compare's 1e-12 l1 and 1e-9 l1 / gap, which stay as they are for the large clouds; the atol = 1e-13
    comparisons with oracle.plane_align are tighter than the rotation bar wherever l1 / gap3 (1 + (1 - c) / s) exceeds 5.
"""
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np

EPS64 = 2.0 ** -52
EPS32 = 2.0 ** -23
GAP_MIN = 1e-6                   # a direction is asserted only where its gap exceeds this share of l1

# -- measured constants (tests/test_eig_exact.py asserts that they still hold) ------------------------------------------
C_VAL_NEEDED, C_VEC_NEEDED, C_ROT_NEEDED, C_DOT_NEEDED = 6.0, 24.0, 24.0, 24.0
C_VAL, C_VEC, C_ROT, C_DOT = 4 * C_VAL_NEEDED, 4 * C_VEC_NEEDED, 4 * C_ROT_NEEDED, 4 * C_DOT_NEEDED


# ======================================================================================================================
# exact covariance and eigen-decomposition
# ======================================================================================================================
def _ints(values):
    """Floats as integers over one power-of-two denominator: values[i] == ints[i] / den, exactly."""
    ratios = [float(v).as_integer_ratio() for v in values]
    den = max(d for _, d in ratios)
    return [n * (den // d) for n, d in ratios], den


def exact_cov(points):
    """np.cov(points, rowvar=False) (ddof 1, pct:277) of the stored values, a 3 x 3 list of ``Fraction``s."""
    p = np.asarray(points)
    m = len(p)
    assert p.ndim == 2 and p.shape[1] == 3 and m >= 2
    flat, den = _ints(p.reshape(-1).tolist())
    cols = [flat[c::3] for c in range(3)]
    s = [sum(col) for col in cols]
    scale = m * (m - 1) * den * den
    cov = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(i, 3):
            cov[i][j] = cov[j][i] = Fraction(m * sum(a * b for a, b in zip(cols[i], cols[j])) - s[i] * s[j], scale)
    return cov


def _dec(fr):
    return Decimal(fr.numerator) / Decimal(fr.denominator)


def _newton(x, t, s, d, tol):
    """Newton on p(x) = x^3 - t x^2 + s x - d from outside the spectrum: monotone for a cubic with three real roots,
    quadratic at a simple root, linear (ratio 1/2) at a double one -- hence the doubled working precision."""
    left = None
    for _ in range(6000):
        f = ((x - t) * x + s) * x - d
        fp = (3 * x - 2 * t) * x + s
        if f == 0 or fp == 0:
            break
        step = f / fp
        x -= step
        if left is None and abs(step) <= tol:
            left = 3
        if left is not None:
            left -= 1
            if left < 0:
                break
    return x


def exact_eigen(cov, digits=60):
    """Eigen-decomposition of a symmetric positive semi-definite 3 x 3 matrix of ``Fraction``s to ``digits`` digits of l1.

    Returns dict(values (3,) float64 descending, vectors (3, 3) float64 unit columns, gaps (3,) float64 -- each
    eigenvalue's distance to the nearest other one --, dvalues / dvectors the ``Decimal`` objects).  The vector of an
    eigenvalue whose gap is zero is whatever unit vector the cross products give: not a function of the input."""
    a = cov
    t = a[0][0] + a[1][1] + a[2][2]
    s = (a[0][0] * a[1][1] - a[0][1] ** 2) + (a[0][0] * a[2][2] - a[0][2] ** 2) + (a[1][1] * a[2][2] - a[1][2] ** 2)
    d = (a[0][0] * (a[1][1] * a[2][2] - a[1][2] ** 2) - a[0][1] * (a[0][1] * a[2][2] - a[1][2] * a[0][2])
         + a[0][2] * (a[0][1] * a[1][2] - a[1][1] * a[0][2]))
    with localcontext() as ctx:
        ctx.prec = 2 * digits + 40
        A = [[_dec(a[i][j]) for j in range(3)] for i in range(3)]
        td, sd, dd = _dec(t), _dec(s), _dec(d)
        zero = Decimal(0)
        if td == 0:
            vals = [zero, zero, zero]
        else:
            tol = td * Decimal(10) ** (-(digits + 15))
            l1 = _newton(td, td, sd, dd, tol)                       # from above: all eigenvalues are <= the trace
            l3 = _newton(zero, td, sd, dd, tol) if dd != 0 else zero  # from below: all are >= 0
            l3 = max(l3, zero)
            l2 = td - l1 - l3
            l2 = min(max(l2, l3), l1)
            vals = [l1, l2, l3]
        vecs = []
        for lam in vals:
            B = [[A[i][j] - (lam if i == j else 0) for j in range(3)] for i in range(3)]
            best, best_n = None, zero
            for p, q in ((0, 1), (0, 2), (1, 2)):
                u, w = B[p], B[q]
                c = [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]
                n2 = c[0] * c[0] + c[1] * c[1] + c[2] * c[2]
                if n2 > best_n:
                    best, best_n = c, n2
            scale4 = max(sum(x * x for x in row) for row in B) ** 2
            if best is None or best_n <= scale4 * Decimal(10) ** (-(ctx.prec - 30)):    # rank <= 1 to the working precision
                best, best_n = None, zero       # (a double eigenvalue): any vector orthogonal to the longest row
                u = max(B, key=lambda row: row[0] * row[0] + row[1] * row[1] + row[2] * row[2])
                for c in ([zero, -u[2], u[1]], [u[2], zero, -u[0]], [-u[1], u[0], zero]):
                    n2 = c[0] * c[0] + c[1] * c[1] + c[2] * c[2]
                    if n2 > best_n:
                        best, best_n = c, n2
                if best is None:                                     # A - lambda I vanishes: a triple eigenvalue
                    best, best_n = [zero, zero, Decimal(1)], Decimal(1)
            nrm = best_n.sqrt()
            vecs.append([x / nrm for x in best])
        gaps = [vals[0] - vals[1], min(vals[0] - vals[1], vals[1] - vals[2]), vals[1] - vals[2]]
        return dict(values=np.array([float(v) for v in vals]), vectors=np.array([[float(x) for x in v] for v in vecs]).T,
                    gaps=np.array([float(g) for g in gaps]), dvalues=vals, dvectors=vecs, prec=ctx.prec)


def residual(cov, eig):
    """max_i |A v_i - l_i v_i| / l1 evaluated in ``decimal`` -- the helper's agreement with itself."""
    with localcontext() as ctx:
        ctx.prec = eig["prec"]
        A = [[_dec(cov[i][j]) for j in range(3)] for i in range(3)]
        worst = Decimal(0)
        for lam, v in zip(eig["dvalues"], eig["dvectors"]):
            for i in range(3):
                worst = max(worst, abs(sum(A[i][j] * v[j] for j in range(3)) - lam * v[i]))
        return float(worst / eig["dvalues"][0]) if eig["dvalues"][0] != 0 else float(worst)


# ======================================================================================================================
# the three stages, exactly
# ======================================================================================================================
def exact_align(points, digits=60):
    """get_best_fit_plane_and_rotate (pct:270-321) of one (m, 3) float32 / float64 block, from the stored values.

    pct:277-283 the normal is the eigenvector of the smallest eigenvalue of the ddof-1 covariance; pct:286-297 it is
    negated when its dot product with points[-1] - points[0] (subtracted IN THE INPUT'S DTYPE), both normalised, is
    negative; pct:300-312 a = the unit normal, v = a x z, c = a . z, s = |v|, R = I + [v]x + [v]x^2 (1 - c) / s^2, the
    identity when s == 0 (which includes a == -z: the block then comes back unrotated); pct:315 R p.
    (1 - c) / s^2 == 1 / (1 + c) exactly, which is how R* is evaluated here.

    Returns a dict of float64 facts: l (3,) descending, gap3, normal (oriented; sign arbitrary when dot == 0), dot >= 0,
    c, s, sens = 1 + (1 - c) / s, R (3, 3), rot64 (m, 3) = R* p correctly rounded, rot32 = rot64 rounded to float32,
    clear32 (m, 3): the distance of R* p from the nearest float32 rounding boundary, pnorm (m,)."""
    p = np.asarray(points)
    eig = exact_eigen(exact_cov(p), digits)
    ref = (p[-1] - p[0]).tolist()                                     # pct:286, in the input's dtype
    with localcontext() as ctx:
        ctx.prec = eig["prec"]
        n = list(eig["dvectors"][2])
        r = [Decimal(x) for x in ref]
        rn = (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]).sqrt()
        # points[-1] == points[0]: pct:290 divides by zero, the comparison with NaN is False and nothing is flipped --
        # dot reads NaN and the orientation (hence the rotation) counts as undefined
        dot = (n[0] * r[0] + n[1] * r[1] + n[2] * r[2]) / rn if rn != 0 else None
        if dot is not None and dot < 0:
            n, dot = [-x for x in n], -dot
        c = n[2]
        s = (n[0] * n[0] + n[1] * n[1]).sqrt()
        one, zero = Decimal(1), Decimal(0)
        if s == 0:
            R = [[one, zero, zero], [zero, one, zero], [zero, zero, one]]
        else:
            f = one / (one + c)
            R = [[one - n[0] * n[0] * f, -n[0] * n[1] * f, -n[0]],
                 [-n[0] * n[1] * f, one - n[1] * n[1] * f, -n[1]],
                 [n[0], n[1], c]]
        rows = [[Decimal(x) for x in row] for row in p.tolist()]
        rot = np.array([[float(R[i][0] * q[0] + R[i][1] * q[1] + R[i][2] * q[2]) for i in range(3)] for q in rows])
        sens = float(one + s / (one + c)) if (s != 0 and c != -1) else (np.inf if c < 0 else 1.0)
        out = dict(l=eig["values"], gaps=eig["gaps"], gap3=float(eig["gaps"][2]), normal=np.array([float(x) for x in n]),
                   dot=float(dot) if dot is not None else float("nan"), c=float(c), s=float(s), sens=sens, R=np.array([[float(x) for x in row] for row in R]))
    rot32 = rot.astype(np.float32)
    # rot64 is within half a float64 ulp of R* p; where that could decide the float32 rounding, clear32 is <= 0
    up = np.nextafter(rot32, np.float32(np.inf)).astype(np.float64)
    dn = np.nextafter(rot32, np.float32(-np.inf)).astype(np.float64)
    mid_up, mid_dn = 0.5 * (rot32 + up), 0.5 * (rot32 + dn)
    out.update(rot64=rot, rot32=rot32, clear32=np.minimum(np.abs(mid_up - rot), np.abs(rot - mid_dn)) - np.spacing(np.abs(rot)),
               pnorm=np.sqrt((p.astype(np.float64) ** 2).sum(1)), block=p, eig=eig)
    return out


def sign_rule(v):
    """The device's documented sign: the component of largest magnitude (the first of equal ones) is positive."""
    v = np.asarray(v, np.float64)
    big = v[np.abs(v).argmax()]
    return -v if big < 0 else v


def exact_pca(points, digits=60):
    """principal_curvatures_via_principal_component_analysis (pct:901-950) of ONE neighbourhood: np.cov of the raw
    coordinates (pct:922), the two largest eigenvalues and their eigenvectors (pct:925-931), K = l1 l2,
    H = (l1 + l2) / 2 (pct:933-934).  Returns dict(l (3,), gaps (3,), dirs (3, 2), K, H), float64, correctly rounded."""
    eig = exact_eigen(exact_cov(points), digits)
    with localcontext() as ctx:
        ctx.prec = eig["prec"]
        l1, l2 = eig["dvalues"][0], eig["dvalues"][1]
        K, H = float(l1 * l2), float((l1 + l2) / 2)
    dirs = np.column_stack([sign_rule(eig["vectors"][:, 0]), sign_rule(eig["vectors"][:, 1])])
    return dict(l=eig["values"], gaps=eig["gaps"], dirs=dirs, K=K, H=H, eig=eig)


SV_EPSILON = 1e-10                # utils.py:828, the float64 literal taken at face value


def exact_surface_variation(points, digits=60):
    """lmin / (l1 + l2 + l3 + 1e-10) of the ddof-1 covariance of the whole block (utils.py:818-828 as restated by
    oracle.surface_variation).  Returns (value float64, l (3,), denominator float64)."""
    cov = exact_cov(points)
    eig = exact_eigen(cov, digits)
    with localcontext() as ctx:
        ctx.prec = eig["prec"]
        den = _dec(cov[0][0] + cov[1][1] + cov[2][2]) + Decimal(SV_EPSILON)
        return float(eig["dvalues"][2] / den), eig["values"], float(den)


# ======================================================================================================================
# bars and exclusions
# ======================================================================================================================
def val_bar(l1, c=None):
    return (C_VAL if c is None else c) * EPS64 * l1


def vec_bar(l1, gap, c=None):
    with np.errstate(divide="ignore"):
        return (C_VEC if c is None else c) * EPS64 * l1 / gap


def rot_unit(f):
    """eps (l1 / gap3) (1 + (1 - c) / s) |p|, (m,): the rotation bar is C_ROT times this."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return EPS64 * (f["l"][0] / f["gap3"]) * f["sens"] * f["pnorm"]


def dot_unit(f):
    """eps l1 / gap3, the error of the normal -- plus, for float32 input, 2^-23: pct:290 normalises the float32 reference
    vector IN FLOAT32, so the reference's own dot product carries a float32 rounding error (the device normalises in
    float64; it is held to the margin the reference needs all the same)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return EPS64 * f["l"][0] / f["gap3"] + (EPS32 if f["block"].dtype == np.float32 else 0.0)


def direction_defined(f):
    return bool(f["gap3"] >= GAP_MIN * f["l"][0]) and f["l"][0] > 0


def orientation_defined(f):
    return direction_defined(f) and bool(f["dot"] > C_DOT * dot_unit(f))


def rotation_defined(f):
    """... and the oriented normal not within its own bar of -z."""
    return orientation_defined(f) and not (f["c"] < 0 and f["s"] <= vec_bar(f["l"][0], f["gap3"]))


def boundary_clear(f):
    """No exactly rotated coordinate within the rotation bar of a float32 rounding boundary: float32(R p) of any
    rotation within the bar is then rot32, bit for bit."""
    return rotation_defined(f) and bool((f["clear32"] > C_ROT * rot_unit(f)[:, None]).all())


def up_to_sign(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(min(np.abs(got - want).max(), np.abs(got + want).max()))


# ======================================================================================================================
# builders
# ======================================================================================================================
def _frame_to(rng, normal):
    """A rotation matrix whose third column is the unit vector along ``normal``."""
    n = np.asarray(normal, np.float64)
    n = n / np.sqrt((n * n).sum())
    t = rng.standard_normal(3)
    t -= (t @ n) * n
    t /= np.sqrt((t * t).sum())
    return np.column_stack([t, np.cross(n, t), n])


def make_block(rng, m, lam, normal, dot=0.3, dtype=np.float64, centre=(0.0, 0.0, 0.0), radius=None):
    """m points whose ddof-1 covariance has eigenvalues ``lam`` (l1 >= l2 >= l3) up to the rounding of the stored
    coordinates, whose ORIENTED normal (pct:286-297) is ``normal`` and whose normalised orientation dot product is |dot|
    (sign: whether the eigen-frame's third axis or its opposite becomes the oriented normal).  Construction: three
    orthonormal, centred columns scaled by sqrt(lam (m - 1)); the third is chosen inside the complement of the first two
    so that last-minus-first has the prescribed component; a rotation onto ``normal``; the cast.  m = 3 is planar, at
    m = 4 the complement is a line and the dot product comes out as it does.  ``radius``: scaled so that the largest
    |coordinate| about the centre is this."""
    l1, l2, l3 = (float(x) for x in lam)
    B = np.linalg.qr(np.column_stack([np.ones(m), rng.standard_normal((m, 2))]))[0]
    u0, v0 = B[:, 1], B[:, 2]
    sig = np.sqrt(np.array([l1, l2, l3]) * (m - 1))
    proj = lambda x: x - B @ (B.T @ x)
    w0 = np.zeros(m)
    if m >= 4:
        e = np.zeros(m)
        e[-1], e[0] = 1.0, -1.0
        pe = proj(e)
        npe = np.sqrt((pe * pe).sum())
        g = proj(rng.standard_normal(m))
        g -= (g @ pe) / (npe * npe) * pe
        ng = np.sqrt((g * g).sum())
        r = np.hypot(sig[0] * (u0[-1] - u0[0]), sig[1] * (v0[-1] - v0[0]))
        d = abs(float(dot))
        alpha = (d * r / np.sqrt(1.0 - d * d)) / (sig[2] * npe) if sig[2] > 0 else 0.0
        if m == 4 or ng < 1e-8 * npe:
            w0 = pe / npe
        else:
            alpha = min(alpha, 0.9)
            w0 = alpha * pe / npe + np.sqrt(1.0 - alpha * alpha) * g / ng
    Q = _frame_to(rng, np.asarray(normal, np.float64) * (1.0 if dot >= 0 else -1.0))
    P = np.column_stack([sig[0] * u0, sig[1] * v0, sig[2] * w0]) @ Q.T
    if radius is not None:
        P *= radius / np.abs(P).max()
    return (P + np.asarray(centre, np.float64)).astype(dtype)


GENERIC_NORMAL = (0.48, -0.6, 0.64)
LADDER_SEED = 20241018
LADDER_M = (8, 50)
GAP_RUNGS = (0.4, 1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8, 1e-9, 1e-10, 1e-11, 1e-12)
GRADING_RUNGS = {np.float64: (1e-2, 1e-4, 1e-8, 1e-12, 1e-16, 1e-20, 1e-24, 1e-28), np.float32: (1e-2, 1e-4, 1e-8, 1e-12)}
TILT_RUNGS = (1.0, 1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-9)     # (1e-9: below any s < 1e-8 shortcut)
DOT_RUNGS = tuple(10.0 ** -j for j in range(1, 13))
SHAPE_M = (3, 4, 6, 8, 50, 300)


def _rng(*key):
    return np.random.default_rng([LADDER_SEED] + [int(k) for k in key])


def _bits(x):
    b = int(np.float64(x).view(np.uint64))
    return b >> 32, b & 0xFFFFFFFF


def _tilted(theta, phi, pole):
    """The unit vector at angle theta from pole * z, azimuth phi."""
    return np.array([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), pole * np.cos(theta)])


def gap_blocks(which, gap, m, dtype, rows):
    """which = 3: l2 - l3 = gap l1 (the normal's gap); which = 1: l1 - l2 = gap l1 (the PCA frame's)."""
    rng = _rng(1, which, m, dtype().itemsize, *_bits(gap))
    lam = (1.0, 0.05 + gap, 0.05) if which == 3 else (1.0, 1.0 - gap, 0.05)
    return [make_block(rng, m, lam, GENERIC_NORMAL, 0.3, dtype) for _ in range(rows)]


def grading_blocks(ratio, m, dtype, rows):
    rng = _rng(2, m, dtype().itemsize, *_bits(ratio))
    return [make_block(rng, m, (1.0, 0.5, ratio), GENERIC_NORMAL, 0.3, dtype) for _ in range(rows)]


def tilt_blocks(theta, pole, m, dtype, rows):
    rng = _rng(3, m, dtype().itemsize, pole + 1, *_bits(theta))
    return [make_block(rng, m, (1.0, 0.6, 0.2), _tilted(theta, rng.uniform(0, 2 * np.pi), pole), 0.3, dtype) for _ in range(rows)]


def dot_blocks(dot, m, dtype, rows):
    rng = _rng(4, m, dtype().itemsize, int(dot > 0), *_bits(abs(dot)))
    return [make_block(rng, m, (1.0, 0.6, 0.3), GENERIC_NORMAL, dot, dtype) for _ in range(rows)]


def shape_blocks(m, dtype, rows):
    """Generic blocks of every row length: m = 300 walks k_fit's unstaged path, m = 3 lies in its own plane (its
    orientation is never asserted), m = 4 ... 8 sit before and after the 8-neighbour unrolled walk."""
    rng = _rng(5, m, dtype().itemsize)
    out = []
    for i in range(rows):
        normal = GENERIC_NORMAL if i % 2 == 0 else _tilted(0.1, rng.uniform(0, 2 * np.pi), -1.0)
        out.append(make_block(rng, m, (1.0, 0.6, 0.2), normal, 0.3, dtype))
    return out


def planar_block(m, dtype):
    """Exactly planar: x, y multiples of 2^-10, z = x + y / 2 (exact in float32): l3 == 0, the normal (1, 1/2, -1) / 1.5."""
    rng = _rng(6, m)
    xy = rng.integers(-1024, 1025, (m, 2)) / 1024.0
    return np.column_stack([xy, xy[:, 0] + 0.5 * xy[:, 1]]).astype(dtype)


def collinear_block(m, dtype):
    """Exactly collinear: t (1, 1/2, -1/4), t a multiple of 2^-10: l2 == l3 == 0, no normal."""
    rng = _rng(7, m)
    t = np.sort(rng.choice(np.arange(-1024, 1025), m, replace=False)) / 1024.0
    return np.outer(t, [1.0, 0.5, -0.25]).astype(dtype)


def identity_block(dtype, h=0.5, reverse=False, tilt=0.0):
    """(0, 0, h) first, the corners (+-1, +-1, 0), (+-2, 0, 0), (0, 0, -h) last: the covariance is exactly
    diag(12, 4, 2 h^2) / 7, the flipped normal exactly -z, s == 0, and the reference returns the input unrotated (checked
    against oracle.plane_align, in both orders, by tests/test_eig_exact.py).  ``tilt``: the block turned about the x axis
    by that angle -- the normal leaves -z and the reference rotates by ~pi instead: the block comes back flipped."""
    P = np.array([[0, 0, h], [1, 1, 0], [1, -1, 0], [-1, 1, 0], [-1, -1, 0], [2, 0, 0], [-2, 0, 0], [0, 0, -h]], np.float64)
    if reverse:
        P = P[::-1].copy()
    if tilt:
        ct, st = np.cos(tilt), np.sin(tilt)
        P = P @ np.array([[1, 0, 0], [0, ct, -st], [0, st, ct]]).T
    return P.astype(dtype)


_RUNGS = {}


def rungs(dtype, ms=LADDER_M, rows=4):
    """Every rung of every ladder for one input dtype: a list of dict(ladder, cond, zones, m, facts), ``facts`` the
    exact_align dicts (block included) of its rows.  ``zones``: the exclusion zones the rung is BUILT to sit in.
    Cached: the CPU and the GPU tests share it."""
    dtype = np.dtype(dtype).type
    key = (dtype, tuple(ms), rows)
    if key in _RUNGS:
        return _RUNGS[key]
    out = []

    def add(ladder, cond, zones, m, blocks):
        out.append(dict(ladder=ladder, cond=cond, zones=frozenset(zones), m=m, facts=[exact_align(b) for b in blocks]))

    f32 = dtype is np.float32
    for m in ms:
        for g in GAP_RUNGS:
            # (float32 inputs: the stored coordinates move the spectrum by 1e-7 l1, the nominal gap is met down to 1e-5)
            undefined = g < (1e-4 if f32 else 3e-6)
            add("gap3", g, ("gap", "dot", "negz") if undefined else (), m, gap_blocks(3, g, m, dtype, rows))
            add("gap1", g, ("gap1",) if undefined else (), m, gap_blocks(1, g, m, dtype, rows))
        for r in GRADING_RUNGS[dtype]:
            # below ~1e-26 (1e-10 in float32) the stored block is flat to rounding: last-minus-first lies in the plane
            add("grading", r, ("dot", "negz") if r < (1e-10 if f32 else 1e-26) else (), m, grading_blocks(r, m, dtype, rows))
        for pole in (-1.0, 1.0):
            for th in TILT_RUNGS:
                add("tilt-z" if pole < 0 else "tilt+z", th, (), m, tilt_blocks(th, pole, m, dtype, rows))
        for d in DOT_RUNGS:
            for sgn in (1.0, -1.0):
                add("dot", sgn * d, ("dot", "negz") if d < (1e-4 if f32 else 1e-13) else (), m, dot_blocks(sgn * d, m, dtype, rows))
    if 300 not in ms:          # the row length of k_fit's unstaged walk: the rungs the fused fit can be held on (fused_rungs)
        for g in (0.4, 0.1):
            add("gap3", g, (), 300, gap_blocks(3, g, 300, dtype, rows))
        add("grading", 1e-2, (), 300, grading_blocks(1e-2, 300, dtype, rows))
        for pole in (-1.0, 1.0):
            for th in (1.0, 0.1):
                add("tilt-z" if pole < 0 else "tilt+z", th, (), 300, tilt_blocks(th, pole, 300, dtype, rows))
    for m in SHAPE_M:
        add("shape", m, ("gap", "dot", "negz") if m == 3 else (("dot", "negz") if m == 4 else ()), m,
            shape_blocks(m, dtype, rows if m < 300 else 2))
        add("planar", m, ("dot", "negz"), m, [planar_block(m, dtype)])
        add("collinear", m, ("gap", "gap1", "dot", "negz"), m, [collinear_block(m, dtype)])
    _RUNGS[key] = out
    return out


def exclusion_counts(rung):
    """(rows, rows without a defined direction, without a defined orientation, without a defined rotation)."""
    fs = rung["facts"]
    return (len(fs), sum(not direction_defined(f) for f in fs), sum(not orientation_defined(f) for f in fs),
            sum(not rotation_defined(f) for f in fs))


def assert_exclusion_caps(rung_list):
    """A rung that is not built to sit in a zone leaves out at most 10 % of its rows from the respective assertion
    (rows of one ladder rung are pooled over m).  Returns the shares for the report."""
    pooled = {}
    for r in rung_list:
        key = (r["ladder"], r["cond"]) if r["ladder"] not in ("shape", "planar", "collinear") else (r["ladder"], r["m"])
        n, nd, no, nr = exclusion_counts(r)
        acc = pooled.setdefault(key, dict(zones=r["zones"], n=0, gap=0, dot=0, negz=0))
        acc["n"] += n; acc["gap"] += nd; acc["dot"] += no; acc["negz"] += nr
    for key, acc in pooled.items():
        for zone in ("gap", "dot", "negz"):
            if zone not in acc["zones"]:
                assert acc[zone] <= 0.1 * acc["n"], (key, zone, acc)
    return pooled


# ======================================================================================================================
# the reference's own routes (float64 NumPy), and what they need from the constants
# ======================================================================================================================
def reference_align(points):
    """pct:270-321 as oracle.plane_align states it, returning (rotated (m, 3) float64, normal as oriented, |dot| as
    pct:293 evaluates it)."""
    p = np.asarray(points)
    cov = np.cov(p, rowvar=False)
    n = np.linalg.svd(cov, full_matrices=True)[2][-1]
    ref = p[-1] - p[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        dot = np.dot(n / np.linalg.norm(n), ref / np.linalg.norm(ref))
    if dot < 0:
        n = -n
    a = n / np.linalg.norm(n)
    v = np.cross(a, np.array([0, 0, 1]))
    c, s = np.dot(a, np.array([0, 0, 1])), np.linalg.norm(v)
    rot = np.eye(3)
    if s != 0:
        kx = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
        rot = np.eye(3) + kx + kx.dot(kx) * ((1 - c) / (s ** 2))
    return np.dot(rot, p.T).T, a, abs(float(dot))


def reference_pca(points):
    """np.cov + eigh: (l (3,) descending, dirs (3, 2) under the sign rule, K, H)."""
    w, v = np.linalg.eigh(np.cov(np.asarray(points, np.float64), rowvar=False))
    return w[::-1].copy(), np.column_stack([sign_rule(v[:, 2]), sign_rule(v[:, 1])]), w[2] * w[1], (w[2] + w[1]) / 2


def reference_surface_variation(points):
    nb = np.asarray(points, np.float64)
    c = nb - nb.mean(0, keepdims=True)
    w = np.linalg.eigh(np.einsum("ki,kj->ij", c, c) / (len(nb) - 1))[0]
    return w[0] / (w.sum() + SV_EPSILON)


def align_needs(f, rotated, normal, dot=None):
    """What one alignment result needs from (C_VEC, C_ROT, C_DOT) on one block -- 0 where the row is excluded.  The
    dot term: the error of the route's own |dot| in units of ``dot_unit`` (a route whose dot product is off by less than
    the margin decides every row outside the margin like the exact sign)."""
    need = dict(vec=0.0, rot=0.0, dot=0.0)
    if not direction_defined(f):
        return need
    need["vec"] = up_to_sign(normal, f["normal"]) / (EPS64 * f["l"][0] / f["gap3"])
    if dot is not None and np.isfinite(f["dot"]):
        need["dot"] = abs(dot - f["dot"]) / dot_unit(f)
    if rotation_defined(f):
        err = np.abs(np.asarray(rotated, np.float64) - f["rot64"]).max(1)
        need["rot"] = float((err / rot_unit(f)).max())
    return need


def pca_needs(points, got, ex=None):
    """What (l (3,)|(2,), dirs, K, H) needs from (C_VAL, C_VEC) against exact_pca; directions only where their gap is
    defined; the projector onto span{v1, v2} by gap3.  ``skipped``: how many of the three direction assertions (v1, v2, the
    projector) the gap rule left out -- callers count them (``pca_shares``)."""
    ex = exact_pca(points) if ex is None else ex
    l, dirs, K, H = got
    l1 = ex["l"][0]
    if not l1 > 0:
        return dict(val=0.0, vec=0.0, skipped=3)
    n = min(len(l), 3)
    val = max(float(np.abs(np.asarray(l[:n]) - ex["l"][:n]).max()) / (EPS64 * l1), abs(H - ex["H"]) / (EPS64 * l1),
              abs(K - ex["K"]) / (EPS64 * l1 * l1))
    vec, skipped = 0.0, 0
    for c in range(2):
        if ex["gaps"][c] >= GAP_MIN * l1:
            vec = max(vec, up_to_sign(dirs[:, c], ex["dirs"][:, c]) / (EPS64 * l1 / ex["gaps"][c]))
        else:
            skipped += 1
    skipped += int(not ex["gaps"][2] >= GAP_MIN * l1)
    if ex["gaps"][2] >= GAP_MIN * l1:
        v3 = ex["eig"]["vectors"][:, 2]                    # span{v1, v2} is the complement of v3, also where l1 == l2
        perr = np.abs(dirs @ dirs.T - (np.eye(3) - np.outer(v3, v3))).max()
        vec = max(vec, float(perr) / (EPS64 * l1 / ex["gaps"][2]))
    return dict(val=val, vec=vec, skipped=skipped)


def sv_within_bar(got, points):
    """|got - exact| <= max(1 ulp32, C_VAL eps l1 / (sum + 1e-10)).  Returns (ok, error / bar)."""
    want, bar, _ = sv_bar(points)
    err = abs(float(got) - want)
    return err <= bar, err / bar


def calibrate(dtypes=(np.float32, np.float64), route=None, pca_route=None):
    """The largest need of a route over the whole ladder, per constant, and the block that sets it.  Default routes: the
    reference's.  ``route(block) -> (rotated, normal, |dot|)``, ``pca_route(block) -> (l, dirs, K, H)``."""
    route = reference_align if route is None else route
    pca_route = reference_pca if pca_route is None else pca_route
    worst = {k: (0.0, None) for k in ("val", "vec", "rot", "dot")}

    def note(kind, value, where):
        if np.isfinite(value) and value > worst[kind][0]:
            worst[kind] = (float(value), where)

    for dtype in dtypes:
        for r in rungs(dtype):
            for f in r["facts"]:
                where = (np.dtype(dtype).name, r["ladder"], r["cond"], r["m"])
                for kind, v in align_needs(f, *route(f["block"])[:3]).items():
                    note(kind, v, where)
                ex = f.setdefault("pca", exact_pca(f["block"]))
                pn = pca_needs(f["block"], pca_route(f["block"]), ex)
                note("val", pn["val"], where)
                note("vec", pn["vec"], where)
    return worst


# ======================================================================================================================
# the kernels' choreography in float64 Python (calibration and teeth only -- never a bar)
# ======================================================================================================================
def _jacobi(a, sweeps, vectors=True):
    """Cyclic Jacobi as JACOBI_ROT / jacobi_rotate: a = [a00, a01, a02, a11, a12, a22].  Returns (diag, V, sweeps used)."""
    a00, a01, a02, a11, a12, a22 = (float(x) for x in a)
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    A = [[a00, a01, a02], [a01, a11, a12], [a02, a12, a22]]
    used = 0
    for _ in range(sweeps):
        off = abs(A[0][1]) + abs(A[0][2]) + abs(A[1][2])
        if off <= 1e-22 * (abs(A[0][0]) + abs(A[1][1]) + abs(A[2][2])):
            break
        used += 1
        for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            apq = A[p][q]
            if apq == 0.0:
                continue
            alpha = 0.5 * (A[q][q] - A[p][p])
            t = (apq if alpha >= 0.0 else -apq) / (abs(alpha) + np.sqrt(alpha * alpha + apq * apq))
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            A[p][p] -= t * apq
            A[q][q] += t * apq
            A[p][q] = A[q][p] = 0.0
            rp, rq = A[r][p], A[r][q]
            A[r][p] = A[p][r] = c * rp - s * rq
            A[r][q] = A[q][r] = s * rp + c * rq
            for i in range(3):
                vp, vq = V[i][p], V[i][q]
                V[i][p], V[i][q] = c * vp - s * vq, s * vp + c * vq
    return [A[0][0], A[1][1], A[2][2]], V, used


def _moments(points, one_pass, origin=None):
    """The six covariance entries as k_fit (one pass about the first neighbour, sxx - sx * mx) or k_plane_rotate (two
    passes) forms them.  ``origin``: the planted defect -- one-pass moments about that point instead."""
    q = np.asarray(points).astype(np.float64)
    m = len(q)
    if one_pass:
        d = q - (q[0] if origin is None else np.asarray(origin, np.float64))
        s1 = [float(np.cumsum(d[:, i])[-1]) for i in range(3)]
        s2 = {(i, j): float(np.cumsum(d[:, i] * d[:, j])[-1]) for i in range(3) for j in range(i, 3)}
        return [(s2[i, j] - s1[i] * (s1[j] / m)) / (m - 1) for i in range(3) for j in range(i, 3)]
    c = q - np.array([float(np.cumsum(q[:, i])[-1]) / m for i in range(3)])
    return [float(np.cumsum(c[:, i] * c[:, j])[-1]) / (m - 1) for i in range(3) for j in range(i, 3)]


def emulate_align(points, one_pass=True, sweeps=8, origin=None, flip=True, c_float32=False, s_zero_below=0.0):
    """plane_rotation() of pct_fit.hip on the CPU.  Returns (rotated (m, 3) float64, oriented unit normal, |dot|, sweeps used).
    Planted defects: sweeps=1, origin=far point, flip=False, c_float32, s_zero_below=1e-8 (the
    tie-order defect lives in ``emulate_pca``)."""
    p = np.asarray(points)
    d, V, used = _jacobi(_moments(p, one_pass, origin), sweeps)
    col = 0 if (d[0] <= d[1] and d[0] <= d[2]) else (1 if d[1] <= d[2] else 2)
    n = np.array([V[0][col], V[1][col], V[2][col]])
    ref = (p[-1] - p[0]).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        dot = np.dot(n / np.sqrt((n * n).sum()), ref / np.sqrt((ref * ref).sum()))
    if flip and dot < 0:
        n = -n
    a = n / np.sqrt((n * n).sum())
    v0, v1 = a[1], -a[0]
    c = float(np.float32(a[2])) if c_float32 else a[2]
    s = np.sqrt(v0 * v0 + v1 * v1)
    R = np.eye(3)
    if s != 0.0 and not s < s_zero_below:
        f = (1.0 - c) / (s * s)
        R = np.array([[1.0 - v1 * v1 * f, v1 * v0 * f, v1], [v0 * v1 * f, 1.0 - v0 * v0 * f, -v0],
                      [-v1, v0, 1.0 + (-(v1 * v1) - v0 * v0) * f]])
    q = p.astype(np.float64)
    return (R[:, 0] * q[:, :1] + R[:, 1] * q[:, 1:2]) + R[:, 2] * q[:, 2:], a, abs(float(dot)), used


def emulate_pca(points, sweeps=16, ties_high_index_first=False):
    """write_frame() of pct_pca.hip on two-pass moments: (l (3,) descending, dirs (3, 2), K, H)."""
    d, V, _ = _jacobi(_moments(points, False), sweeps)
    ge = (lambda x, y: x > y) if ties_high_index_first else (lambda x, y: x >= y)
    if ge(d[0], d[1]) and ge(d[0], d[2]):
        i1, i2 = 0, (1 if ge(d[1], d[2]) else 2)
    elif ge(d[1], d[2]):
        i1, i2 = 1, (0 if ge(d[0], d[2]) else 2)
    else:
        i1, i2 = 2, (0 if ge(d[0], d[1]) else 1)
    i3 = 3 - i1 - i2
    V = np.array(V)
    dirs = np.column_stack([sign_rule(V[:, i1]), sign_rule(V[:, i2])])
    return np.array([d[i1], d[i2], d[i3]]), dirs, d[i1] * d[i2], (d[i1] + d[i2]) / 2


def tie_block(dtype=np.float64):
    """Exactly equal l1 == l2: the corners (+-1, +-1, +-1/4) -- cov == diag(8, 8, 1/2) / 7.  The device documents
    'ties: lower index first': direction 1 is +x, direction 2 is +y."""
    return np.array([[x, y, z] for x in (1, -1) for y in (1, -1) for z in (0.25, -0.25)], dtype)


# ======================================================================================================================
# clusters: neighbourhoods as clouds, for the kernels that find their own neighbours
# ======================================================================================================================
def cluster_cloud(blocks, dtype, spacing=16.0, offset=(0.0, 0.0, 0.0), radius=1.0):
    """Each (m, 3) block becomes a cluster of m + 1 points: the block scaled to ``radius`` (largest |coordinate| about
    its centre), preceded by one point near its mean, placed on a cubic lattice of pitch ``spacing`` (a power of two,
    several cluster diameters).  With k = m every point's neighbour set is the rest of its cluster.  float32: offsets are
    quantised to spacing * 2^-20 with at most 8 clusters per axis, so that centre + offset is exact.
    Returns (cloud (n (m + 1), 3), first row of every cluster)."""
    side = 8
    assert len(blocks) <= side ** 3 and np.log2(spacing) == np.round(np.log2(spacing))
    quantum = spacing * 2.0 ** -20
    pts, first = [], []
    for i, b in enumerate(blocks):
        b = np.asarray(b, np.float64)
        b = b - b.mean(0)
        b = b * (radius / np.abs(b).max())
        extra = 0.37 * b[0] + 0.21 * b[-1]
        c = np.vstack([extra[None], b])
        if np.dtype(dtype) == np.float32:
            c = np.round(c / quantum) * quantum
        centre = spacing * np.array([i % side, (i // side) % side, i // (side * side)], np.float64)
        first.append(i * len(c))
        pts.append(c + centre + np.asarray(offset, np.float64))
    return np.vstack(pts).astype(dtype), np.array(first, np.int64)


# ======================================================================================================================
# the checks the CPU and the GPU tests share
# ======================================================================================================================
NORM_EPS = 16.0     # |R p| against |p|: a (1.5 eps), f = (1 - c) / s^2 (3 eps) and the three-term products (3 eps) leave R
                    # orthogonal to ~8 eps; doubled.  Asserted on EVERY finite row, defined rotation or not.


def align_shares(f, rotated):
    """One block's result against the bars: dict(rot -- worst error as a share of the rotation bar, None where the
    rotation is not defined --, norm -- worst | |R p| - |p| | as a share of NORM_EPS eps |p| --, oriented -- the rotated
    block lies on the exact side of its plane, None where the orientation is not defined)."""
    out = np.asarray(rotated, np.float64)
    res = dict(rot=None, norm=0.0, oriented=None, finite=bool(np.isfinite(out).all()))
    if not res["finite"]:
        return res
    pn = f["pnorm"]
    nz = pn > 0
    if nz.any():
        res["norm"] = float((np.abs(np.sqrt((out * out).sum(1)) - pn)[nz] / (NORM_EPS * EPS64 * pn[nz])).max())
    if rotation_defined(f):
        unit = rot_unit(f)
        res["rot"] = float((np.abs(out - f["rot64"]).max(1)[nz] / (C_ROT * unit[nz])).max())
        res["oriented"] = bool((out[:, 2] * f["rot64"][:, 2]).sum() > 0)
    return res


def check_rung(rung, results, where=""):
    """Asserts one rung's results (a sequence of rotated blocks) and returns (worst rot share, worst norm share,
    rows asserted, rows)."""
    worst_r = worst_n = 0.0
    asserted = 0
    for f, out in zip(rung["facts"], results):
        sh = align_shares(f, out)
        tag = (where, rung["ladder"], rung["cond"], rung["m"])
        assert sh["finite"], tag
        assert sh["norm"] <= 1.0, (tag, "norm", sh["norm"])
        worst_n = max(worst_n, sh["norm"])
        if sh["rot"] is not None:
            asserted += 1
            assert sh["oriented"], (tag, "orientation", f["dot"])
            assert sh["rot"] <= 1.0, (tag, "rotation", sh["rot"], f["l"], f["c"], f["s"])
            worst_r = max(worst_r, sh["rot"])
    return worst_r, worst_n, asserted, len(rung["facts"])


def pca_shares(points, got, ex=None, tally=None, rung=None):
    """(l, dirs, K, H) against exact_pca: worst shares of the value and the direction bars.  ``tally`` (with ``rung``)
    counts the direction assertions the gap rule left out, per (ladder, cond)."""
    n = pca_needs(points, got, ex)
    if tally is not None:
        acc = tally.setdefault((rung["ladder"], rung["cond"]), dict(zones=rung["zones"], n=0, skipped=0))
        acc["n"] += 3
        acc["skipped"] += n["skipped"]
    return n["val"] / C_VAL, n["vec"] / C_VEC


def assert_pca_caps(tally):
    """Of the direction assertions (v1, v2, projector per row) a rung that is built to sit in neither gap zone leaves out
    at most 10 %.  Returns (left out, asserted or left out) over those rungs."""
    out = total = 0
    for key, acc in tally.items():
        if "gap" not in acc["zones"] and "gap1" not in acc["zones"]:
            assert acc["skipped"] <= 0.1 * acc["n"], (key, acc)
            out += acc["skipped"]
            total += acc["n"]
    assert total > 0
    return out, total


TIE_FRAME = np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]])


def tie_frame_ok(l1, l2, dirs):
    """The assertion on ``tie_block``: exactly equal eigenvalues, and 'ties: lower index first' -- +x, then +y."""
    return bool(l1 == l2) and np.array_equal(np.asarray(dirs), TIE_FRAME)


UTM_OFFSET = (4.2e5, 5.1e6, 250.0)
PCA_LADDERS = ("gap1", "gap3", "grading", "planar", "collinear")
TIE_RUNG = dict(ladder="tie", cond=0.0, zones=frozenset(("gap1",)))


def pca_blocks(m, dtype):
    """[(rung, block)] that become the clusters of one (m, dtype): the gap ladders, the grading, the degenerate blocks,
    and at m = 8 the tie block."""
    blocks = [(r, f["block"]) for r in rungs(dtype) if r["m"] == m and r["ladder"] in PCA_LADDERS for f in r["facts"]]
    if m == 8:
        blocks.append((TIE_RUNG, tie_block(dtype)))
    return blocks


def cluster_rows(first, m):
    """The rows of a cluster cloud that are held to the exact value: per cluster the added point's row and the row of the
    block's first point, each with its neighbour set (the rest of its cluster).  Yields (cluster, row, neighbours)."""
    for c, at in enumerate(first):
        members = np.arange(at, at + m + 1)
        for row in (at, at + 1):
            yield c, row, members[members != row]


def sv_bar(points):
    """(exact surface variation, its bar max(1 ulp32, C_VAL eps l1 / (sum + 1e-10)), the denominator)."""
    want, l, den = exact_surface_variation(points)
    return want, max(float(np.spacing(np.float32(want))), val_bar(l[0]) / den), den


FUSED_M = (8, 50, 300)


def fused_rungs(dtype):
    """The rungs the fused fit is walked over (tests 4(b)): the rungs on which the rotation bar stays below ~1e-5 of a
    float32 ulp of every coordinate, so that the boundary rule leaves out at most 1 % of the rows -- gaps of 0.4 and 0.1,
    grading 1e-2, tilts of 1 and 0.1 from either pole, dot products down to 1e-3, the row lengths 8, 50, 300 -- and the
    identity-branch block.  m = 300 (k_fit's unstaged walk) takes gap 0.4, grading 1e-2, tilts of 1 and 0.1 from +z and
    its two shape blocks (one of them 0.1 from -z): 18 rows.  (Beyond them the rule bites by construction: the bar grows with l1 / gap3 and with
    (1 - c) / s, and a block graded to 1e-8 has rotated z coordinates whose float32 ulp lies below eps |p|.)"""
    out = []
    for r in rungs(dtype):
        if r["m"] not in FUSED_M:
            continue
        lad, c = r["ladder"], r["cond"]
        if r["m"] == 300 and ((lad == "gap3" and c < 0.4) or lad == "tilt-z"):
            continue        # 900 coordinates a row: only l1 / gap3 (1 + (1 - c) / s) <= 4 keeps the boundary rule's share at 1 %
        if ((lad == "gap3" and c >= 0.1) or (lad == "grading" and c >= 1e-2) or (lad in ("tilt-z", "tilt+z") and c >= 0.1)
                or (lad == "dot" and abs(c) >= 1e-3) or lad == "shape"):
            out.append(r)
    key = ("identity", np.dtype(dtype).type)
    if key not in _RUNGS:
        _RUNGS[key] = dict(ladder="identity", cond=0.0, zones=frozenset(("negz",)), m=8,
                           facts=[exact_align(identity_block(dtype, reverse=rev)) for rev in (False, True)])
    return out + [_RUNGS[key]]

"""Exact ground truth for the quadric fit  --  TEST INFRASTRUCTURE ONLY (CPU, no GPU, no import of the package).

Everything the suite knew about the fit (pct:331-360: ``lstsq`` of the float32 design rows [a^2, b^2, ab, a, b, 1]) was
a comparison with float64 NumPy.  This module supplies a reference that is MORE precise than either side:

* ``exact_lstsq``         the least-squares solution of a float32 system in exact rational arithmetic;
* diagnostics             the kernel's Cholesky pivot ratios, relative singular values, the conditioning of the
                          column-equilibrated matrix and a natural scale per coefficient;
* ``ring / lines / aspect``  seeded ladders of centred neighbourhoods that walk from a well-conditioned design matrix
                          to within a few decades of gelsd's cut-off, built so that the reference's own rotation
                          (pct:270-321) returns the constructed float32 block bit for bit;
* ``emulated_cholesky``   a float64 normal-equation solve with k_fit's pivot test, written from DESIGN.md 4.3 --
                          used to CALIBRATE (where do normal equations stop being good enough), never as a bar.

The bar every solver is held to (``coef_bar``), per coefficient j:

    |c[j] - c*[j]|  <=  max( 1 ulp32(c*[j]),  C_FLOOR * 2^-52 * kappa * S_j )

c* the exact solution, kappa = sigma_1 / sigma_6 of the column-equilibrated design matrix, S_j = max|z| / max|X[:, j]|.
The first term is what rounding a float64 solution to float32 costs (pct:359's cast, double rounding included); the
second is the error bound of a backward-stable least-squares solve, eps * kappa, in the units of coefficient j.

Constants (measured on the CPU against the exact solution or the reference, never against the GPU;
tests/test_fit_exact.py re-measures them on every run and asserts that they still hold):

    C_NEEDED = 2800   what ``calibrate()`` finds over the whole ladder (ring, lines, aspect; m = 6, 7, 8, 50, 300; 1 248
                      blocks): numpy.linalg.lstsq, rounded to float32 as pct:359 returns it, needs 11.0 where the ulp term
                      does not cover it already; emulated_cholesky with the SVD fallback below its pivot threshold,
                      unrounded, needs 2 791 -- on a block with pivot ratio 5e-6, kappa = 1e3: the error of normal
                      equations is eps * kappa^2, i.e. they need C ~ kappa at the threshold.  (The unrounded lstsq needs
                      1.3e5 on the unpaired 1 : 1000 aspect rung -- gelsd follows the unscaled condition number -- which
                      is 1e-9 relative and far below the ulp term: it is recorded, not used.)
    C_FLOOR  = 4 * C_NEEDED = 11 200.  The factor 4 covers the different constants of two backward-stable
                      factorisations: Householder bidiagonalisation in gelsd, Givens QR + one-sided Jacobi in k_fit_svd.
                      On every block k_fit keeps (pivot ratio >= 1e-6) the ulp term is the larger one for every coefficient
                      whose exact value is not zero (smallest ulp / (eps kappa S) there: 16 820): Cholesky rows are held
                      to pure rounding.

    R_SPREAD = 4      queries outside their neighbourhood (``foreign_bars``): the bar of a row is the larger of the 1e-5
                      contract and R x the reference's own spread over permuted, mathematically equivalent rows.  Measured:
                      the spread is 0 on every one of the 2 x 132 rows, at 1 000 radii too -- np.cov's centred moments
                      move the rotation by 1e-16, and the float32 cast of the rotated block erases that -- and
                      ``emulated_fused`` needs no spread term at all (it stays within 1.4e-2 of the contract).  R is
                      therefore the bare safety factor, the same 4 as above, and the bar is the contract.
                      The same emulation with moments about the QUERY (``shift=False``, what k_fit did before this test
                      existed) misses the contract in H at 1 000 radii: 1 100-fold (float32 cloud), 50-fold (float64).
"""
from fractions import Fraction

import numpy as np

EPS64 = 2.0 ** -52
PIVOT_RATIO_MIN = 1e-6          # k_fit's kPivotRatioMin

# -- measured constants (tests/test_fit_exact.py asserts that they still hold) ------------------------------------------
C_NEEDED = 2800.0
C_FLOOR = 4.0 * C_NEEDED
R_SPREAD = 4.0


# ======================================================================================================================
# exact rational least squares
# ======================================================================================================================
def _int_column(v):
    """A float vector as integers over one power-of-two denominator: v[i] == ints[i] / den, exactly."""
    fr = [Fraction(float(x)) for x in v]
    den = max(f.denominator for f in fr)
    return [f.numerator * (den // f.denominator) for f in fr], den


def exact_lstsq(X, z):
    """The least-squares solution of X c = z as a list of six ``Fraction``s, or None unless X has full column rank.

    X (m, n) and z (m,) are taken at face value (float32 or float64 entries are exact rationals).  Normal equations
    over the integers, Gaussian elimination over ``Fraction``: no rounding anywhere."""
    X = np.asarray(X)
    z = np.asarray(z)
    m, n = X.shape
    if m < n:
        return None
    cols, dens = zip(*(_int_column(X[:, j]) for j in range(n)))
    zi, zden = _int_column(z)
    G = [[Fraction(sum(a * b for a, b in zip(cols[i], cols[j]))) for j in range(n)] for i in range(n)]
    r = [Fraction(sum(a * b for a, b in zip(cols[i], zi))) for i in range(n)]
    # G' c' = r'  with  c_j = c'_j * dens[j] / zden
    for p in range(n):
        piv = next((q for q in range(p, n) if G[q][p] != 0), None)
        if piv is None:
            return None
        if piv != p:
            G[p], G[piv] = G[piv], G[p]
            r[p], r[piv] = r[piv], r[p]
        inv = 1 / G[p][p]
        for q in range(p + 1, n):
            f = G[q][p] * inv
            if f != 0:
                G[q] = [gq - f * gp for gq, gp in zip(G[q], G[p])]
                r[q] -= f * r[p]
    c = [Fraction(0)] * n
    for p in range(n - 1, -1, -1):
        c[p] = (r[p] - sum(G[p][q] * c[q] for q in range(p + 1, n))) / G[p][p]
    return [c[j] * dens[j] / zden for j in range(n)]


def round_f32(fr):
    """A rational correctly rounded to float32 (no double rounding: the float64 neighbours are compared exactly)."""
    c = np.float32(float(fr))
    cands = [c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))]
    cands = [x for x in cands if np.isfinite(x)]
    return min(cands, key=lambda x: abs(Fraction(float(x)) - fr))


def exact_f64(sol):
    return np.array([float(f) for f in sol], np.float64)


def exact_f32(sol):
    return np.array([round_f32(f) for f in sol], np.float32)


def abs_err(c, sol):
    """|c[j] - c*[j]| evaluated exactly, returned as float64."""
    return np.array([float(abs(Fraction(float(x)) - f)) if np.isfinite(x) else np.inf
                     for x, f in zip(np.asarray(c).tolist(), sol)], np.float64)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


# ======================================================================================================================
# diagnostics of one design matrix
# ======================================================================================================================
def design(block):
    """The reference's float32 design matrix and right-hand side of one ROTATED float32 neighbourhood (pct:350-358)."""
    p = np.array(block, dtype=np.float32)
    a, b, c = p[:, 0], p[:, 1], p[:, 2]
    return np.column_stack((a ** 2, b ** 2, a * b, a, b, np.ones_like(a))).astype(np.float32), c


def pivot_ratios(X):
    """k_fit's d_j / g_jj of the float64 Gram matrix, j = 0..5.  After a non-positive pivot the
    remaining ratios read 0."""
    X = np.asarray(X, np.float64)
    G = X.T @ X
    n = G.shape[0]
    L = np.zeros((n, n))
    out = np.zeros(n)
    for j in range(n):
        d = G[j, j] - (L[j, :j] ** 2).sum()
        out[j] = d / G[j, j] if G[j, j] > 0 else 0.0
        if not d > 0:
            out[j:] = np.minimum(out[j:], 0.0)
            break
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (G[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return out


def rel_singular_values(X):
    s = np.linalg.svd(np.asarray(X, np.float64), compute_uv=False)
    return s / s[0]


def kappa_equilibrated(X):
    """sigma_1 / sigma_6 of X with its columns scaled to unit length."""
    X = np.asarray(X, np.float64)
    nrm = np.sqrt((X * X).sum(0))
    s = np.linalg.svd(X / np.where(nrm > 0, nrm, 1.0), compute_uv=False)
    return s[0] / s[-1] if s[-1] > 0 else np.inf


def natural_scale(X, z):
    """S_j = max|z| / max|X[:, j]|: the size coefficient j has when its column alone explains the data."""
    X = np.asarray(X, np.float64)
    return np.abs(np.asarray(z, np.float64)).max() / np.abs(X).max(0)


def gelsd_cut(m):
    return EPS64 * max(m, 6)


def coef_bar(sol, X, z, c_floor=None):
    """(ulp term, conditioning term) of the bar, each (6,) float64."""
    c_floor = C_FLOOR if c_floor is None else c_floor
    return ulp32(exact_f32(sol)), c_floor * EPS64 * kappa_equilibrated(X) * natural_scale(X, z)


# ======================================================================================================================
# ladders
# ======================================================================================================================
def _assemble(rng, ab, m, paired, extent):
    """A centred neighbourhood of m float32 points over the footprint ``ab`` ((m // 2, 2) when paired, else (m, 2)).

    paired: the points come as adjacent pairs (a, b, z), (-a, -b, z), z an even function of (a, b), which leaves the
    covariance without xz / yz entries: the best-fit normal is +z up to rounding noise.  They are ordered by z, lowest
    first and highest last, so that points[-1] - points[0] (pct:286) has a clear +z component.  The reference's
    rotation then returns the float32 block bit for bit (tests/test_fit_exact.py asserts it).  m must be even: an
    antipodally symmetric set of odd size contains the origin, whose zero coordinates the rotation turns into 1e-20.
    unpaired: m generic points and odd terms in z (used where the design matrix is handed over directly).

    The surface is drawn in the footprint's own units -- z = amp (A u^2 + B v^2 + C uv [+ D u + E v] + F), u = a / extent_a,
    v = b / extent_b, every coefficient between 1/2 and 2 in size -- so that every column carries a comparable share of z
    and the exact coefficients are of the order of their natural scale S_j.  The misfit is the float32 rounding of the
    block (a relative 1e-7 is added to z on top): the error of a backward-stable solve is then eps * kappa up to
    kappa ~ 1e7 (its eps * kappa^2 * residual term stays below)."""
    ea, eb = extent
    amp = 0.02 * min(ea, eb)                                  # keeps var(z) the smallest of the three
    A, B, C = rng.uniform(1.0, 2.0, 3) * rng.choice([-1.0, 1.0], 3)
    D, E = rng.uniform(0.5, 1.0, 2) * rng.choice([-1.0, 1.0], 2)
    F = rng.uniform(0.5, 1.0) * rng.choice([-1.0, 1.0])
    ab = np.asarray(ab, np.float64).astype(np.float32).astype(np.float64)
    u, v = ab[:, 0] / ea, ab[:, 1] / eb
    z = A * u * u + B * v * v + C * u * v + F
    if not paired:
        z = z + D * u + E * v
    z = amp * z * (1.0 + 1e-7 * rng.standard_normal(len(z)))
    if paired:
        assert m % 2 == 0 and len(ab) == m // 2
        pts = np.empty((m, 3))
        pts[0::2] = np.column_stack([ab, z])
        pts[1::2] = np.column_stack([-ab, z])
    else:
        pts = np.column_stack([ab, z])
    assert len(pts) == m
    pts = pts.astype(np.float32)
    return pts[np.argsort(pts[:, 2], kind="stable")]


def _footprint(kind, rng, n, cond):
    """n footprint points (a, b) of one ladder and the footprint's two extents."""
    if kind == "ring":           # a, b on the unit circle, relative radial jitter cond: a^2 + b^2 -> 1
        th = rng.uniform(0.0, 2.0 * np.pi, n)
        r = 1.0 + cond * rng.uniform(-1.0, 1.0, n)
        return np.column_stack([r * np.cos(th), r * np.sin(th)]), (1.0, 1.0)
    if kind == "lines":          # two scan lines b = +-1 with relative across-line jitter cond: b^2 -> 1
        a = rng.uniform(-1.0, 1.0, n)
        b = rng.choice([-1.0, 1.0], n) * (1.0 + cond * rng.uniform(-1.0, 1.0, n))
        return np.column_stack([a, b]), (1.0, 1.0)
    if kind == "aspect":         # a jittered lattice patch, spacing 1 : 1 / cond
        side = int(np.ceil(np.sqrt(2.0 * n))) + 1
        ij = np.array([(i, j) for i in range(-side, side + 1) for j in range(0, side + 1) if j > 0 or i > 0], float)
        ij = ij[np.argsort((ij ** 2).sum(1), kind="stable")][:n]
        ij += 0.05 * rng.uniform(-1.0, 1.0, ij.shape)
        ij /= np.abs(ij).max()
        return np.column_stack([ij[:, 0], ij[:, 1] / cond]), (1.0, 1.0 / cond)
    raise ValueError(kind)


def ladder(kind, seed, cond, rows, m, paired=True):
    """Up to ``rows`` float32 centred neighbourhoods (n, m, 3) of ladder ``kind`` at conditioning parameter ``cond``.

    A drawn block is kept only if its design matrix has sigma_6 / sigma_1 >= 100 x gelsd's cut-off eps * max(m, 6): inside
    that band whether LAPACK keeps the singular value is decided by rounding and the reference's answer is not a
    function of its input.  At most 4 * rows draws are made; a rung that lies in the band altogether comes back empty."""
    bits = int(np.float64(cond).view(np.uint64))
    rng = np.random.default_rng([int(seed), {"ring": 1, "lines": 2, "aspect": 3}[kind], int(m), int(paired),
                                 bits >> 32, bits & 0xFFFFFFFF])
    out = []
    for _ in range(4 * rows):
        ab, ext = _footprint(kind, rng, m // 2 if paired else m, cond)
        blk = _assemble(rng, ab, m, paired, ext)
        if rel_singular_values(design(blk)[0])[-1] >= 100.0 * gelsd_cut(m):
            out.append(blk)
            if len(out) == rows:
                break
    return np.array(out, np.float32).reshape(len(out), m, 3)


def ring(seed, delta, rows=8, m=50, paired=True):
    return ladder("ring", seed, delta, rows, m, paired)


def lines(seed, delta, rows=8, m=50, paired=True):
    return ladder("lines", seed, delta, rows, m, paired)


def aspect(seed, ratio, rows=8, m=50, paired=True):
    return ladder("aspect", seed, ratio, rows, m, paired)


# Decades, except around k_fit's threshold: delta = 1e-3 puts the pivot ratio AT 1e-6 (1.1e-6 ... 1.5e-6 measured), where
# which side a block falls on is an accident of the seed; 2e-3 and 5e-4 straddle it by a factor of 3 to 5 instead
# (5e-6 and 3e-7).  3e-6 adds a rung at ratio 1e-11, inside the decades where normal equations visibly fail.
RING_DELTAS = (1.0, 1e-1, 1e-2, 2e-3, 5e-4, 1e-4, 1e-5, 3e-6, 1e-6, 1e-7)
LINES_DELTAS = RING_DELTAS
ASPECT_RATIOS = (1.0, 10.0, 100.0, 1000.0)
LADDER_SEED = 20240607


def all_rungs(m, rows=8, paired=True, seed=LADDER_SEED, kinds=("ring", "lines", "aspect")):
    """Every non-empty rung of the ladders: a list of (kind, cond, blocks (n, m, 3) float32)."""
    conds = {"ring": RING_DELTAS, "lines": LINES_DELTAS, "aspect": ASPECT_RATIOS}
    out = [(kind, c, ladder(kind, seed, c, rows, m, paired)) for kind in kinds for c in conds[kind]]
    return [r for r in out if len(r[2])]


# ======================================================================================================================
# CPU solvers used for calibration only
# ======================================================================================================================
def emulated_cholesky(X, z, ratio_min=PIVOT_RATIO_MIN):
    """k_fit's solve as DESIGN.md 4.3 describes it: float64 Gram matrix of the float32 design rows, unpivoted
    Cholesky with reciprocal pivots, and the pivot test.  Returns (coefficients float64, smallest ratio, well)."""
    X, z = np.asarray(X, np.float64), np.asarray(z, np.float64)
    n = X.shape[1]
    # row by row, as the kernel accumulates (and independent of the BLAS at hand: the constants below are re-measured)
    G = np.array([[np.cumsum(X[:, i] * X[:, j])[-1] for j in range(n)] for i in range(n)])
    b = np.array([np.cumsum(X[:, i] * z)[-1] for i in range(n)])
    L = np.zeros((n, n))
    dinv = np.zeros(n)
    well, rmin = True, np.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(n):
            d = G[j, j] - (L[j, :j] ** 2).sum()
            well = well and bool(d > ratio_min * G[j, j])
            rmin = min(rmin, d / G[j, j]) if G[j, j] > 0 else 0.0
            dinv[j] = 1.0 / np.sqrt(d)
            for i in range(j + 1, n):
                L[i, j] = (G[i, j] - (L[i, :j] * L[j, :j]).sum()) * dinv[j]
        y = np.zeros(n)
        for i in range(n):
            y[i] = (b[i] - (L[i, :i] * y[:i]).sum()) * dinv[i]
        c = np.zeros(n)
        for i in range(n - 1, -1, -1):
            c[i] = (y[i] - (L[i + 1:, i] * c[i + 1:]).sum()) * dinv[i]
    return c, rmin, well


def svd_fallback(X, z):
    """The shape of k_fit_svd on the CPU: QR first (no squaring of the condition number), SVD of the triangular
    factor, singular values below gelsd's cut-off dropped."""
    X, z = np.asarray(X, np.float64), np.asarray(z, np.float64)
    Q, Rm = np.linalg.qr(X)
    U, s, Vt = np.linalg.svd(Rm)
    keep = s > gelsd_cut(len(X)) * s[0]
    w = (U.T @ (Q.T @ z))[keep] / s[keep]
    return Vt[keep].T @ w


def emulated_fit(X, z):
    """emulated_cholesky, handed to svd_fallback below the pivot threshold: the float64 solution k_fit + k_fit_svd aim at."""
    c, _, well = emulated_cholesky(X, z)
    return c if well else svd_fallback(X, z)


def reference_lstsq64(X, z):
    """pct:359 before its cast: numpy.linalg.lstsq(rcond=None) of the float32 rows, in float64."""
    return np.linalg.lstsq(np.asarray(X, np.float64), np.asarray(z, np.float64), rcond=None)[0]


# ======================================================================================================================
# the cases every test walks, with their exact solutions (cached: the GPU tests and the CPU tests share them)
# ======================================================================================================================
# (m, paired).  Paired blocks are the ones the fused path can be fed (its rotation returns them bit for bit); they need an
# even m, and m >= 8 for full column rank (the four even columns see each pair once).  m = 6 and 7 are unpaired and go to
# the solver alone.
SOLVER_CASES = ((6, False), (7, False), (8, True), (50, False), (50, True), (300, False), (300, True))
FUSED_M = (8, 50, 300)
_FACTS = {}


def block_facts(blk):
    X, z = design(blk)
    sol = exact_lstsq(X, z)
    assert sol is not None                        # (a block that passed the band test has full column rank)
    S = natural_scale(X, z)
    kap = kappa_equilibrated(X)
    return dict(block=blk, X=X, z=z, sol=sol, c32=exact_f32(sol), c64=exact_f64(sol), pivot=float(pivot_ratios(X).min()),
                sv6=float(rel_singular_values(X)[-1]), kappa=kap, S=S, unit=EPS64 * kap * S, ulp=ulp32(exact_f32(sol)),
                nonzero=np.array([f != 0 for f in sol]))


def ladder_facts(m, paired):
    """[(kind, cond, [facts of every block])] of one case."""
    key = (int(m), bool(paired))
    if key not in _FACTS:
        _FACTS[key] = [(kind, cond, [block_facts(b) for b in blocks]) for kind, cond, blocks in all_rungs(m, paired=paired)]
    return _FACTS[key]


def in_calibration(kind, paired):
    """Every rung calibrates C but the PAIRED aspect ones.  There D* = E* = 0 exactly, so only the conditioning term
    stands between lstsq and the bar, and gelsd is normwise stable, not columnwise: at 1 : 1000 its absolute error is
    eps * sigma_1 / sigma_6 of the UNSCALED matrix (4e6) times the largest coefficient, 1e5 times the columnwise floor.
    That is a property of the reference, invisible in float32 (1e-9 of the other coefficients), and it would cost the bar
    all its teeth.  tests/test_fit_exact.py pins it on its own; the unpaired aspect rungs (no exact zeros) calibrate."""
    return not (kind == "aspect" and paired)


def calibrate():
    """What the two CPU solvers need from C over the whole ladder, each against the bar it is held to:
      lstsq32   numpy.linalg.lstsq rounded to float32 (what pct:359 returns) against max(ulp, C eps kappa S): the largest
                err / (eps kappa S) over the coefficients the ulp term does not already cover;
      emu64     emulated_cholesky (SVD fallback below the pivot threshold), unrounded, against C eps kappa S alone.
    Also: the worst error in float32 ulps of A, B, C of the bare Cholesky solve by pivot-ratio class, and the smallest
    ulp / (eps kappa S) over the non-zero coefficients of the rows k_fit keeps (pivot ratio >= 1e-6)."""
    out = dict(lstsq32=0.0, emu64=0.0, lstsq64=0.0, chol_ulps_well=0.0, chol_ulps_below_1e10=np.inf, ulp_over_unit_well=np.inf,
               blocks=0)
    for m, paired in SOLVER_CASES:
        for kind, cond, facts in ladder_facts(m, paired):
            if not in_calibration(kind, paired):
                continue
            for f in facts:
                out["blocks"] += 1
                c_ref = reference_lstsq64(f["X"], f["z"])
                e32 = abs_err(c_ref.astype(np.float32), f["sol"])
                out["lstsq32"] = max(out["lstsq32"], float(np.where(e32 > f["ulp"], e32 / f["unit"], 0.0).max()))
                out["lstsq64"] = max(out["lstsq64"], float((abs_err(c_ref, f["sol"]) / f["unit"]).max()))
                out["emu64"] = max(out["emu64"], float((abs_err(emulated_fit(f["X"], f["z"]), f["sol"]) / f["unit"]).max()))
                chol = emulated_cholesky(f["X"], f["z"])[0]
                ulps = float((abs_err(chol.astype(np.float32), f["sol"]) / f["ulp"])[:3].max())
                if f["pivot"] >= PIVOT_RATIO_MIN:
                    out["chol_ulps_well"] = max(out["chol_ulps_well"], ulps)
                    out["ulp_over_unit_well"] = min(out["ulp_over_unit_well"], float((f["ulp"] / f["unit"])[f["nonzero"]].min()))
                elif f["pivot"] < 1e-10:
                    out["chol_ulps_below_1e10"] = min(out["chol_ulps_below_1e10"], ulps)
    return out


def within_bar(c, f, rounded=True):
    """|c - c*| <= max(ulp, C eps kappa S) per coefficient (rounded: a float32 result) or <= C eps kappa S alone."""
    bar = C_FLOOR * f["unit"]
    if rounded:
        bar = np.maximum(f["ulp"], bar)
    err = abs_err(c, f["sol"])
    return err <= bar, err, bar


# ======================================================================================================================
# queries outside their neighbourhood
# ======================================================================================================================
FOREIGN_OFFSETS = (0.0, 1.0, 3.0, 10.0, 100.0, 1000.0)      # neighbourhood radii between the query and the centroid
FOREIGN_PERMUTATIONS = 6
SPREAD_DROP = 1e-2
RTOL, FLOOR = 1e-5, 1e-2                                     # the project's contract (tests/test_gpu_parity.py)


def foreign_query_cloud(seed, dtype, patches=12, m=50, h=0.05):
    """Smooth patches (principal curvatures up to 6, radius h: k h <= 0.3), randomly oriented and placed, each queried
    from points 0 ... 1000 radii away from its centroid, along its normal and in its tangent plane.

    Returns (points, idx (rows, m), query (rows,), offset (rows,)).  The patch points are ordered by height over their
    tangent plane, so that the orientation test's last-minus-first vector (pct:286) has a clear normal component."""
    rng = np.random.default_rng([int(seed), 77])
    pts, idx, query, offset = [], [], [], []
    n = 0
    for _ in range(patches):
        r, th = h * np.sqrt(rng.uniform(0.0, 1.0, m)), rng.uniform(0.0, 2.0 * np.pi, m)
        u, v = r * np.cos(th), r * np.sin(th)
        k1, k2 = rng.uniform(1.0, 6.0, 2) * rng.choice([-1.0, 1.0], 2)
        w = 0.5 * (k1 * u * u + k2 * v * v) + rng.uniform(-20.0, 20.0) * u * u * v
        order = np.argsort(w, kind="stable")
        u, v, w = u[order], v[order], w[order]
        Q = np.linalg.qr(rng.standard_normal((3, 3)))[0]
        c0 = rng.uniform(-1.0, 1.0, 3)
        P = c0 + np.column_stack([u, v, w]) @ Q.T
        ids = np.arange(n, n + m)
        pts.append(P)
        n += m
        cen = P.mean(0)
        for t in FOREIGN_OFFSETS:
            for d in ((Q[:, 2],) if t == 0 else (Q[:, 2], Q[:, 0])):
                pts.append((cen + t * h * d)[None, :])
                idx.append(ids)
                query.append(n)
                offset.append(t)
                n += 1
    return (np.vstack(pts).astype(dtype), np.array(idx, np.int32), np.array(query, np.int64), np.array(offset))


def foreign_permutations(m, n=FOREIGN_PERMUTATIONS, seed=5):
    """n orders of a row of m neighbours (the identity first) that keep its first and last entry where they are: the
    reference reads those two for its orientation test, everything else it does is a sum over the neighbours."""
    rng = np.random.default_rng(seed)
    out = [np.arange(m)]
    for _ in range(n - 1):
        out.append(np.concatenate([[0], 1 + rng.permutation(m - 2), [m - 1]]))
    return out


def reference_with_spread(points, idx, query):
    """oracle.curvature_loop on the rows as given, and the reference's own spread: the largest deviation of its K and H
    over the permuted (mathematically equivalent) rows.  Returns (K, H, spread_K, spread_H), float64."""
    import pct_oracle as oracle
    K = np.empty((FOREIGN_PERMUTATIONS, len(idx)))
    H = np.empty_like(K)
    for p, perm in enumerate(foreign_permutations(idx.shape[1])):
        _, k, hh, _ = oracle.curvature_loop(points, idx[:, perm], query)
        K[p], H[p] = k, hh
    return K[0], H[0], np.abs(K - K[0]).max(0), np.abs(H - H[0]).max(0)


def foreign_bars(ref, spread, offset):
    """Per row: the contract |x - ref| <= 1e-5 max(|ref|, 1e-2 max|ref| of the rung), the spread term R x spread, and
    which rows carry no information (spread above 1e-2 of the contract's own yardstick)."""
    contract, drop = np.empty(len(ref)), np.zeros(len(ref), bool)
    for t in np.unique(offset):
        r = offset == t
        yard = np.maximum(np.abs(ref[r]), FLOOR * np.abs(ref[r]).max())
        contract[r] = RTOL * yard
        drop[r] = spread[r] > SPREAD_DROP * yard
    return contract, R_SPREAD * spread, drop


def emulated_fused(centred, shift=True):
    """The fused kernel's choreography on the CPU, from DESIGN.md 4.3 (calibration only): moments about the first
    neighbour (shift=False: about the query), covariance as sxx - sx * mx, normal, flip, Rodrigues, float32 design
    rows, emulated_fit, float32 coefficients."""
    q = np.asarray(centred).astype(np.float64)
    m = len(q)
    qs = q - q[0] if shift else q
    s1 = np.cumsum(qs, 0)[-1]
    s2 = np.array([[np.cumsum(qs[:, i] * qs[:, j])[-1] for j in range(3)] for i in range(3)])
    cov = (s2 - np.outer(s1, s1 / m)) / (m - 1)
    n = np.linalg.eigh(cov)[1][:, 0]
    ref = (np.asarray(centred)[-1] - np.asarray(centred)[0]).astype(np.float64)
    if np.dot(n / np.linalg.norm(n), ref / np.linalg.norm(ref)) < 0:
        n = -n
    a = n / np.linalg.norm(n)
    v = np.array([a[1], -a[0], 0.0])
    c, s = a[2], np.hypot(a[0], a[1])
    rot = np.eye(3)
    if s != 0:
        kx = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
        rot = np.eye(3) + kx + kx @ kx * ((1 - c) / (s * s))
    X, z = design((rot @ q.T).T.astype(np.float32))
    return emulated_fit(X, z).astype(np.float32)


# ======================================================================================================================
# coefficient space for the float32 curvature formulas
# ======================================================================================================================
def coefficient_space():
    """Coefficient rows (n, 6) float32: slopes D, E from 0 to 1e3, A, B, C over 1e-20 ... 1e18, parabolic points (4AB - C^2
    cancels), and values whose squares or products leave float32 at either end."""
    rng = np.random.default_rng(2)
    slopes = np.array([0.0, 1e-3, 0.3, 1.0, 30.0, 1e3], np.float32)
    mags = np.float32(10.0) ** np.arange(-20, 19, 2, dtype=np.float32)
    rows = []
    for D in slopes:
        for E in slopes:
            for _ in range(40):
                A, B = rng.choice(mags, 2) * rng.uniform(1, 10, 2).astype(np.float32) * rng.choice([-1, 1], 2)
                C = rng.choice(mags) * np.float32(rng.uniform(1, 10)) * rng.choice([-1, 1])
                rows.append([A, B, C, D * rng.choice([-1, 1]), E * rng.choice([-1, 1]), rng.standard_normal()])
            for _ in range(10):                              # parabolic points: 4AB - C^2 cancels
                A = rng.choice(mags[5:15]) * np.float32(rng.uniform(1, 10))
                B = rng.choice(mags[5:15]) * np.float32(rng.uniform(1, 10))
                C = np.float32(2.0) * np.sqrt(np.float32(A) * np.float32(B))
                rows.append([A, B, C * rng.choice([-1, 1]), D, -E, 0.0])
                rows.append([-A, -B, np.nextafter(np.float32(C), np.float32(0)), -D, E, 0.0])
    for big in (1e9, 3e9, 1e10, 1e15, 1.8e19, 1.9e19, 3e19, 3e38):        # wgt * wgt, then Fx * Fx itself, leave float32
        for A, B, C in ((1.0, 2.0, 0.5), (0.0, 0.0, 0.0), (1e30, -1e30, 1e20), (1e-30, 1e-30, 0.0)):
            rows += [[A, B, C, big, 0.0, 0.0], [A, B, C, -big, big, 0.0], [A, B, C, 1.0, big, 0.0]]
    for A, B, C in ((3e38, 3e38, 0.0), (1e19, 1e19, 3e19), (3e38, 1.0, 3e38), (1e-45, 1e-45, 1e-45), (1e-38, 1e-7, 1e-22)):
        rows += [[A, B, C, 0.0, 0.0, 0.0], [A, -B, C, 0.5, -0.25, 0.0]]   # products that overflow / underflow on their own
    return np.array(rows, np.float32)

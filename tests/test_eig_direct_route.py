"""The direct route to the tangent-plane normal (plane_rotation() of pct_fit.hip), emulated in float64 on the CPU.

plane_rotation() no longer runs the cyclic Jacobi on every row.  From the six covariance entries it takes

  1. the matrix scaled by the exact power of two that brings its trace into [1/2, 1)  (frexp / ldexp: no rounding);
  2. l3 as the smallest root of  f(x) = x^3 - c2 x^2 + c1 x - c0  (trace, principal 2 x 2 minors, determinant): Newton
     from x = 0, where f is increasing and concave -- monotone from the left, quadratic at a simple root; NEWTON_CAP steps;
  3. the normal as the largest (squared norm, the first of equal ones) of the three cross products of rows of A - x I;
  4. one refinement: x += n^T (A - x I) n / n^T n (the Rayleigh quotient, as a correction), the cross products again;
  5. one reciprocal square root.

A row is HEALTHY when f' stayed positive, a Newton step s with |s| c2 <= NEWTON_TOL f' came within the cap, and
both rounds' largest cross product has a squared norm of at least (CROSS_FLOOR trace^2)^2.  Every other row -- near-equal
small eigenvalues, lines, points, non-finite input -- takes the cyclic Jacobi, unchanged, behind a branch.  Behind either
route the normal is a unit vector and is normalised no further: the orientation is the sign of n . (last - first) with
the reference vector as subtracted, and Rodrigues' factor is (1 - c) / (v0^2 + v1^2).

``emulate_direct`` states this operation for operation, as eig_exact.emulate_align does for the old choreography
(which stays the yardstick: its needs, measured here again, are what the new route is held to).  The bars are
eig_exact's; nothing here is compared with the device -- tests/test_gpu_fit_direct_normal.py does that.

The rule the constants were chosen by: over the 1 308 ladder blocks the largest need of the combined route may not exceed
1.5 x the need of the Jacobi emulation, per constant (which leaves the 4 x margin under the bars that eig_exact built in).
"""
import math

import numpy as np
import pytest

import eig_exact as ee

NEWTON_CAP = 6                 # steps; bench-like torus rows take 2, the ladder's healthy blocks up to 6 (l3 = l2 / 2)
NEWTON_TOL = 2.0 ** -14        # |step| c2 <= NEWTON_TOL f': see direct_normal
CROSS_FLOOR = 1e-4             # |largest cross product| >= CROSS_FLOOR trace^2, i.e. l1 gap3 >~ 1e-4 trace^2


def _cross_rows(b00, b01, b02, b11, b12, b22, first_only=False):
    """The largest of r0 x r1, r0 x r2, r1 x r2 (rows of the symmetric B), the first of equal ones; its squared norm."""
    rows = ((b00, b01, b02), (b01, b11, b12), (b02, b12, b22))
    best, best_n = None, -1.0
    for p, q in ((0, 1), (0, 2), (1, 2)):
        u, w = rows[p], rows[q]
        c = (u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0])
        n2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
        if best is None or n2 > best_n:
            best, best_n = c, n2
        if first_only:
            break
    return best, best_n


def direct_normal(a, refine=True, scale=True, first_only=False, health=True):
    """Steps 1-5 on a = [a00, a01, a02, a11, a12, a22].  Returns (unit normal or None for 'take the Jacobi', Newton steps).
    Planted defects: refine=False, scale=False, first_only=True, health=False.

    The stopping rule.  After a step s the distance to the root is about s^2 |f''| / (2 f') <= s^2 c2 / f', and f' is
    about l1 gap3, so gap3 is about f' / c2.  The refinement squares the RELATIVE error: a value off by d leaves a normal
    off by d / gap3 and a Rayleigh quotient off by (d / gap3)^2 l1.  (d / gap3)^2 <= eps / 4 asks d <= 7e-9 f' / c2, that
    is |s| c2 <= 8.6e-5 f'; 2^-14 = 6.1e-5."""
    a00, a01, a02, a11, a12, a22 = (float(x) for x in a)
    tr = (a00 + a11) + a22
    if not (tr > 0.0 and tr < math.inf):
        return None, 0
    if scale:
        e = -math.frexp(tr)[1]
        a00, a01, a02, a11, a12, a22 = (math.ldexp(x, e) for x in (a00, a01, a02, a11, a12, a22))
    c2 = (a00 + a11) + a22
    m01, m02, m12 = a00 * a11 - a01 * a01, a00 * a22 - a02 * a02, a11 * a22 - a12 * a12
    c1 = (m01 + m02) + m12
    c0 = (a00 * m12 - a01 * (a01 * a22 - a12 * a02)) + a02 * (a01 * a12 - a11 * a02)
    lam, ok, steps = 0.0, False, 0
    for _ in range(NEWTON_CAP):
        f = ((lam - c2) * lam + c1) * lam - c0
        fp = (3.0 * lam - 2.0 * c2) * lam + c1
        if not fp > 0.0:
            break
        step = f / fp
        lam -= step
        steps += 1
        if abs(step) * c2 <= NEWTON_TOL * fp:
            ok = True
            break
    floor = (CROSS_FLOOR * (c2 * c2)) * (CROSS_FLOOR * (c2 * c2))
    n, n2 = _cross_rows(a00 - lam, a01, a02, a11 - lam, a12, a22 - lam, first_only)
    ok = ok and n2 >= floor
    if health and not ok:
        return None, steps
    if refine:
        b00, b11, b22 = a00 - lam, a11 - lam, a22 - lam
        w0 = (b00 * n[0] + a01 * n[1]) + a02 * n[2]
        w1 = (a01 * n[0] + b11 * n[1]) + a12 * n[2]
        w2 = (a02 * n[0] + a12 * n[1]) + b22 * n[2]
        with np.errstate(all="ignore"):
            lam = float(np.float64(lam) + np.float64((w0 * n[0] + w1 * n[1]) + w2 * n[2]) / np.float64(n2))
        n, n2 = _cross_rows(a00 - lam, a01, a02, a11 - lam, a12, a22 - lam, first_only)
        if health and not n2 >= floor:
            return None, steps
    with np.errstate(all="ignore"):
        inv = float(np.float64(1.0) / np.sqrt(np.float64(n2)))
    return np.array([n[0] * inv, n[1] * inv, n[2] * inv]), steps


def emulate_direct(points, one_pass=True, force_jacobi=False, **defect):
    """plane_rotation() on the CPU.  Returns (rotated (m, 3) float64, oriented unit normal, |dot| normalised -- for the
    measurement only: the route itself takes the sign of the unnormalised product --, fell back to the Jacobi)."""
    p = np.asarray(points)
    a = ee._moments(p, one_pass)
    n = None if force_jacobi else direct_normal(a, **defect)[0]
    fell_back = n is None
    if fell_back:
        d, V, _ = ee._jacobi(a, 8)
        col = 0 if (d[0] <= d[1] and d[0] <= d[2]) else (1 if d[1] <= d[2] else 2)
        n = np.array([V[0][col], V[1][col], V[2][col]])
        n = n / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    ref = (p[-1] - p[0]).astype(np.float64)                       # subtracted in the input's dtype (pct:286)
    with np.errstate(all="ignore"):
        dot = (n[0] * ref[0] + n[1] * ref[1]) + n[2] * ref[2]
        if dot < 0:
            n = -n
        shown = abs(float(dot)) / np.sqrt((ref * ref).sum())
        v0, v1, c = n[1], -n[0], n[2]
        ss = v0 * v0 + v1 * v1
        R = np.eye(3)
        if ss != 0.0:
            f = (1.0 - c) / ss
            R = np.array([[1.0 - v1 * v1 * f, v1 * v0 * f, v1], [v0 * v1 * f, 1.0 - v0 * v0 * f, -v0],
                          [-v1, v0, 1.0 + (-(v1 * v1) - v0 * v0) * f]])
        q = p.astype(np.float64)
        return (R[:, 0] * q[:, :1] + R[:, 1] * q[:, 1:2]) + R[:, 2] * q[:, 2:], n, shown, fell_back


# ------------------------------------------------------------------------------------------------ the 1.5 x rule
def test_combined_route_needs_at_most_one_and_a_half_times_the_jacobi_emulation():
    fell = [0, 0]

    def route(block):
        out = emulate_direct(block)
        fell[0] += int(out[3])
        fell[1] += 1
        return out[:3]

    new = ee.calibrate(route=route, pca_route=ee.emulate_pca)
    old = ee.calibrate(route=lambda b: ee.emulate_align(b)[:3], pca_route=ee.emulate_pca)
    print("direct route with fallback:", {k: (round(v, 2), w) for k, (v, w) in new.items()})
    print("Jacobi emulation:          ", {k: (round(v, 2), w) for k, (v, w) in old.items()})
    print(f"{fell[0]} of {fell[1]} ladder blocks took the fallback")
    assert fell[1] > 1200 and 0 < fell[0] < 0.25 * fell[1], fell
    for kind in ("vec", "rot", "dot", "val"):
        assert new[kind][0] <= 1.5 * old[kind][0], (kind, new[kind], old[kind])
        assert new[kind][0] <= {"val": ee.C_VAL_NEEDED}.get(kind, ee.C_VEC_NEEDED), (kind, new[kind])
    # two-pass moments (k_plane_rotate) and the switch: the same bars, rung by rung
    for dtype in (np.float32, np.float64):
        for r in ee.rungs(dtype):
            if r["ladder"] == "collinear":
                continue
            ee.check_rung(r, [emulate_direct(f["block"], one_pass=False)[0] for f in r["facts"]], "two-pass")
            ee.check_rung(r, [emulate_direct(f["block"], force_jacobi=True)[0] for f in r["facts"]], "switch")


def test_newton_steps_and_the_identity_branch():
    steps = [direct_normal(ee._moments(f["block"], True)) for dt in (np.float32, np.float64) for r in ee.rungs(dt) for f in r["facts"]]
    healthy = [s for n, s in steps if n is not None]
    print(f"Newton steps on the {len(healthy)} healthy ladder blocks: max {max(healthy)}, mean {np.mean(healthy):.2f}")
    assert max(healthy) <= NEWTON_CAP
    for dtype in (np.float32, np.float64):
        for rev in (False, True):
            b = ee.identity_block(dtype, reverse=rev)
            out = emulate_direct(b, one_pass=False)
            assert not out[3] and np.array_equal(out[0], b.astype(np.float64))       # healthy, and bit for bit
            assert np.array_equal(emulate_direct(b)[0], b.astype(np.float64))
    tilted = ee.identity_block(np.float64, tilt=min(ee.TILT_RUNGS))
    f = ee.exact_align(tilted)
    sh = ee.align_shares(f, emulate_direct(tilted, one_pass=False)[0])
    assert sh["rot"] <= 1.0 and sh["norm"] <= 1.0 and sh["oriented"], sh


# ------------------------------------------------------------------------------------------------ teeth
def _misses(facts, **defect):
    """The planted defect misses a bar of check_rung on this block (non-finite output counts: it is check_rung's first bar)."""
    rung = dict(ladder="teeth", cond=0.0, m=len(facts["block"]), facts=[facts])
    for one_pass in (True, False):
        try:
            ee.check_rung(rung, [emulate_direct(facts["block"], one_pass, **defect)[0]])
        except AssertionError:
            return True
    return False


def _sound(facts):
    return ee.rotation_defined(facts) and not _misses(facts)


def test_no_rayleigh_refinement_misses_the_bar_where_l2_is_far_below_l1():
    rng = np.random.default_rng(ee.LADDER_SEED + 11)
    hit = 0
    for i in range(8):
        f = ee.exact_align(ee.make_block(rng, 50, (1.0, 2e-3, 1e-3), ee.GENERIC_NORMAL, 0.3, np.float64))
        assert _sound(f) and not emulate_direct(f["block"])[3]                      # healthy, direct, within the bars
        hit += _misses(f, refine=False)
    print(f"no refinement: {hit} of 8 blocks with l = (1, 2e-3, 1e-3) miss the rotation bar")
    assert hit >= 4


def test_no_power_of_two_scaling_misses_at_radius_2_to_the_minus_200():
    rng = np.random.default_rng(ee.LADDER_SEED + 12)
    b = ee.make_block(rng, 50, (1.0, 0.6, 0.2), ee.GENERIC_NORMAL, 0.3, np.float64)
    small = b * 2.0 ** -200
    f = ee.exact_align(small)
    assert _sound(f) and not emulate_direct(small)[3]
    # unscaled, the cubic's coefficients underflow: the health test (or, with it off, the zero cross product) gives it away
    assert emulate_direct(small, scale=False)[3]
    assert _misses(f, scale=False, health=False)


def test_always_the_first_cross_product_misses_where_it_vanishes():
    # the normal along x: rows 0 and 1 of A - l3 I are (0, 0, 0)-ish and e_y-ish; r0 x r1 vanishes to rounding
    rng = np.random.default_rng(ee.LADDER_SEED + 13)
    f = ee.exact_align(ee.make_block(rng, 50, (1.0, 0.6, 0.2), (1.0, 0.0, 0.0), 0.3, np.float64))
    assert _sound(f) and not emulate_direct(f["block"])[3]
    assert _misses(f, first_only=True, health=False)


def test_health_test_off_misses_on_the_close_gaps():
    """The gap3 ladder, l = (1, 0.05 + g, 0.05): every rung from g = 1e-2 down takes the fallback (Newton from the left
    is slow towards two close roots, then the cross products shrink).  With the health test off the unconverged value
    is used as it is.  Where eig_exact has a bar for the direction (g >= 1e-5) every row misses it, by up to 5e11 of
    its unit.  On the rungs g <= 1e-9 NO row can miss: they lie in eig_exact's zone "gap" (gap3 < 1e-6 l1, the normal
    is not a function of the input), where only finiteness and the row norms are asserted and any unit vector passes --
    measured: 0 of 64 rows.  What holds there instead is asserted: every row takes the Jacobi."""
    missed = rows = 0
    for dtype in (np.float32, np.float64):
        for r in ee.rungs(dtype):
            if r["ladder"] != "gap3" or r["cond"] > 1e-2:
                continue
            for f in r["facts"]:
                assert emulate_direct(f["block"])[3] and emulate_direct(f["block"], one_pass=False)[3]
                assert not _misses(f)                                        # with it on: the Jacobi, within its bars
                if r["cond"] >= 1e-5:
                    assert ee.rotation_defined(f) and _misses(f, health=False), (dtype.__name__, r["cond"], r["m"])
                if r["cond"] <= 1e-9:
                    rows += 1
                    missed += _misses(f, health=False)
                    assert not ee.direction_defined(f)
    print(f"health test off: {missed} of {rows} rows of the gap3 <= 1e-9 rungs miss a bar (none applies to their normal); "
          f"every row of the rungs 1e-2 ... 1e-5 does")
    for dtype in (np.float32, np.float64):                                   # lines: no cross product survives
        f = ee.exact_align(ee.collinear_block(8, dtype))
        assert emulate_direct(f["block"])[3] and _misses(f, health=False)


# ------------------------------------------------------------------------------------------------ scaling
def test_scaled_by_two_to_the_plus_and_minus_200_the_normal_keeps_its_bits():
    rng = np.random.default_rng(ee.LADDER_SEED + 14)
    b = ee.make_block(rng, 50, (1.0, 0.6, 0.2), ee.GENERIC_NORMAL, 0.3, np.float64)
    base = emulate_direct(b)
    assert not base[3]
    for e in (-200, 200):
        out = emulate_direct(b * 2.0 ** e)
        assert not out[3]
        assert np.array_equal(out[1].view(np.uint64), base[1].view(np.uint64)), e
        assert np.array_equal(out[0].view(np.uint64), (base[0] * 2.0 ** e).view(np.uint64)), e

"""The quadric fit's ground truth, checked on the CPU: exact rational least squares, the conditioning ladders, and the
constants the GPU tests (tests/test_gpu_fit_conditioning.py) hold the kernels to.  Nothing here touches the package.

What is pinned, and by what:
  * the helpers themselves (exact_lstsq against hand-made systems);
  * the ladder construction: the reference's rotation returns every constructed block bit for bit (cap: 1 % excluded);
  * the reference (pct:270-360) lies within the bar on every rung -- so the bar is one the reference meets;
  * the claims behind kPivotRatioMin = 1e-6 (formerly the docstring of oracle/calibrate_pivot_ratio.py);
  * C and R, re-measured.
"""
from fractions import Fraction

import numpy as np
import pytest

import fit_exact as fe
import pct_oracle as oracle


def test_exact_lstsq_on_systems_with_known_answers():
    rng = np.random.default_rng(1)
    want = [Fraction(3), Fraction(-7, 4), Fraction(1, 8), Fraction(5), Fraction(-2), Fraction(9, 16)]
    X = rng.integers(-8, 9, (11, 6)).astype(np.float32) / np.float32(4)
    z = np.array([float(sum(Fraction(float(x)) * w for x, w in zip(row, want))) for row in X], np.float32)
    assert fe.exact_lstsq(X, z) == want                                   # a consistent system: the solution itself
    z2 = z.copy()
    z2[3] += np.float32(0.5)                                              # an inconsistent one: the normal equations hold exactly
    sol = fe.exact_lstsq(X, z2)
    res = [Fraction(float(v)) - sum(Fraction(float(x)) * c for x, c in zip(row, sol)) for row, v in zip(X, z2)]
    assert all(sum(Fraction(float(X[i, j])) * res[i] for i in range(len(X))) == 0 for j in range(6))
    assert fe.exact_lstsq(np.column_stack([X[:, :5], X[:, 0] + X[:, 1]]), z) is None      # dependent columns
    assert fe.exact_lstsq(X[:5], z[:5]) is None                                           # fewer rows than columns
    # correct rounding to float32: exactly halfway between two neighbours goes to the even one, a hair above goes up
    one, nxt = np.float32(1), np.nextafter(np.float32(1), np.float32(2))
    half = (Fraction(float(one)) + Fraction(float(nxt))) / 2
    assert fe.round_f32(half + Fraction(1, 1 << 80)) == nxt and fe.round_f32(half - Fraction(1, 1 << 80)) == one
    assert fe.ulp32(np.float32(1.5)) == 2.0 ** -23 and fe.ulp32(np.float32(0)) == 2.0 ** -149


def test_diagnostics_agree_with_their_definitions():
    blk = fe.ring(3, 1e-2, rows=1, m=50)[0]
    X, z = fe.design(blk)
    assert X.dtype == np.float32 and np.array_equal(X[:, 0], blk[:, 0] * blk[:, 0]) and np.array_equal(z, blk[:, 2])
    pr = fe.pivot_ratios(X)
    _, rmin, well = fe.emulated_cholesky(X, z)
    assert np.isclose(pr.min(), rmin, rtol=1e-6) and well == (rmin > fe.PIVOT_RATIO_MIN)
    # d_j / g_jj = sin^2 of the angle between column j and the span of the columns before it
    X64 = X.astype(np.float64)
    for j in (1, 5):
        proj = X64[:, :j] @ np.linalg.lstsq(X64[:, :j], X64[:, j], rcond=None)[0]
        assert np.isclose(pr[j], ((X64[:, j] - proj) ** 2).sum() / (X64[:, j] ** 2).sum(), rtol=1e-6)
    assert np.isclose(fe.kappa_equilibrated(X * np.float32(8)), fe.kappa_equilibrated(X))
    assert np.allclose(fe.natural_scale(X, z) * np.abs(X64).max(0), np.abs(z).max())
    # pivot ratios are invariant under column scaling, relative singular values are not
    D = np.array([1, 1e-6, 1e-3, 1, 1e-3, 1])
    assert np.allclose(fe.pivot_ratios(X64 * D), pr, rtol=1e-6)


def test_ladders_walk_the_conditioning_range_and_stay_out_of_gelsds_band():
    for m, paired in fe.SOLVER_CASES:
        rungs = fe.ladder_facts(m, paired)
        assert {k for k, _, _ in rungs} == {"ring", "lines", "aspect"}
        for kind, cond, facts in rungs:
            assert all(f["sv6"] >= 100 * fe.gelsd_cut(m) for f in facts), (m, kind, cond)
    for m in (50, 300):                 # (at m = 6 ... 8 the conditioning of a block is mostly the luck of its draw)
        for kind in ("ring", "lines"):
            piv = {c: [f["pivot"] for f in fs] for k, c, fs in fe.ladder_facts(m, True) if k == kind}
            assert min(piv[1.0]) > 1e-1 and max(piv[1e-7]) < 1e-13                    # the range of the issue's table
            assert min(piv[2e-3]) > 3e-6 and max(piv[5e-4]) < 5e-7                    # the threshold is straddled, not hit
            assert all(1e-12 < p < 1e-10 for c in (3e-6,) for p in piv[c])            # the decades a lowered threshold would open
        asp = {c: fs for k, c, fs in fe.ladder_facts(m, True) if k == "aspect"}
        assert all(f["pivot"] > 1e-1 for fs in asp.values() for f in fs)              # scale-invariant ...
        assert max(f["sv6"] for f in asp[1000.0]) < 1e-6                              # ... where sigma_6 / sigma_1 is not


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_rotation_returns_the_constructed_block(dtype):
    """What makes the ladder usable on the fused path: oracle.plane_align of a paired, z-ordered block is the block."""
    total = bad = 0
    for m in fe.FUSED_M:
        for kind, cond, facts in fe.ladder_facts(m, True):
            for f in facts:
                total += 1
                rot = np.array(oracle.plane_align(f["block"].astype(dtype)), dtype=np.float32)
                bad += not np.array_equal(rot, f["block"])
    assert total > 500 and bad <= 0.01 * total, (bad, total)
    print(f"{dtype.__name__}: {bad} of {total} blocks differ after the reference's rotation")


def _reference_coefficients(f, paired):
    return oracle.quadric_fit(oracle.plane_align(f["block"])) if paired else oracle.quadric_fit(f["block"])


def test_reference_lies_within_the_bar_on_every_rung():
    """oracle.quadric_fit (through oracle.plane_align for the paired blocks) against the exact solution."""
    worst_ulps = 0.0
    for m, paired in fe.SOLVER_CASES:
        for kind, cond, facts in fe.ladder_facts(m, paired):
            if not fe.in_calibration(kind, paired):
                continue
            for f in facts:
                c = _reference_coefficients(f, paired)
                assert c.dtype == np.float32
                ok, err, bar = fe.within_bar(c, f)
                assert ok.all(), (m, paired, kind, cond, err / bar)
                if (bar[:3] == f["ulp"][:3]).all():
                    worst_ulps = max(worst_ulps, float((err / f["ulp"])[:3].max()))
    # where the ulp term is the bar, lstsq is the correctly rounded exact A, B, C up to double rounding (its float64 error
    # is at most C_NEEDED / C_FLOOR / 250 of an ulp there)
    assert worst_ulps <= 0.51, worst_ulps
    print(f"reference: worst error of A, B, C where one ulp is the bar: {worst_ulps:.4f} ulp32")


def test_reference_on_the_paired_aspect_rungs_is_normwise_stable_only():
    """The one place where lstsq does not meet the columnwise bar: D* = E* = 0 exactly on a badly scaled matrix.  A, B, C
    and F are within half an ulp all the same; D and E within eps * sigma_1 / sigma_6 (unscaled) * max|c*|, the normwise
    bound of a backward-stable solve -- and not within the columnwise bar, which is why these rungs do not calibrate C."""
    beyond = 0
    for m in fe.FUSED_M:
        for kind, cond, facts in fe.ladder_facts(m, True):
            if kind != "aspect":
                continue
            for f in facts:
                c = _reference_coefficients(f, True)
                ok, err, bar = fe.within_bar(c, f)
                assert ok[[0, 1, 2, 5]].all() and (err <= 0.5 * f["ulp"] * (1 + 2.0 ** -20))[[0, 1, 2, 5]].all()
                assert not f["nonzero"][3] and not f["nonzero"][4]
                assert (err[3:5] <= fe.EPS64 / f["sv6"] * np.abs(f["c64"]).max()).all(), (m, cond, err[3:5])
                beyond += int((~ok[3:5]).any())
    assert beyond > 0


def test_calibration_claims_behind_the_pivot_threshold():
    """On the blocks k_fit keeps (pivot ratio >= 1e-6) a float64 Cholesky solve of the normal equations stays within one
    float32 ulp of the exact A, B, C; on the rungs below 1e-10 it does not."""
    cal = fe.calibrate()
    assert cal["chol_ulps_well"] <= 1.0, cal
    rungs_below = 0
    for m, paired in fe.SOLVER_CASES:
        for kind, cond, facts in fe.ladder_facts(m, paired):
            if not all(f["pivot"] < 1e-10 for f in facts) or not fe.in_calibration(kind, paired):
                continue
            rungs_below += 1
            ulps = [float((fe.abs_err(fe.emulated_cholesky(f["X"], f["z"])[0].astype(np.float32), f["sol"]) / f["ulp"])[:3].max())
                    for f in facts]
            assert max(ulps) > 1.0, (m, paired, kind, cond, ulps)
    assert rungs_below >= 20
    print(f"Cholesky, pivot ratio >= 1e-6: worst {cal['chol_ulps_well']:.3f} ulp32 of A, B, C; {rungs_below} rungs below 1e-10 all beyond 1 ulp")


def test_conditioning_floor_constant():
    """C, re-measured against the exact solution (never against the GPU), and what the bar promises with it."""
    cal = fe.calibrate()
    print({k: (round(v, 3) if isinstance(v, float) else v) for k, v in cal.items()})
    need = max(cal["lstsq32"], cal["emu64"])
    assert 0.5 * fe.C_NEEDED <= need <= fe.C_NEEDED, cal                  # (the recorded value is neither short nor stale)
    assert fe.C_FLOOR == 4 * fe.C_NEEDED
    # where k_fit keeps a row, one float32 ulp is the larger term for every coefficient that is not exactly zero
    assert cal["ulp_over_unit_well"] > fe.C_FLOOR, cal
    assert cal["blocks"] >= 1200


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_foreign_queries_reference_spread_and_R(dtype):
    """Queries 0 ... 1 000 radii away from their neighbourhood: the reference's own spread, the caps, and the CPU
    emulation of the fused path against the bar the GPU test uses."""
    P, idx, query, offset = fe.foreign_query_cloud(11, dtype)
    K, H, sK, sH = fe.reference_with_spread(P, idx, query)
    co = np.array([fe.emulated_fused(P[i] - P[q]) for i, q in zip(idx, query)])
    raw = np.array([fe.emulated_fused(P[i] - P[q], shift=False) for i, q in zip(idx, query)])
    eK, eH, _ = oracle._curv_f32(co)
    rK, rH, _ = oracle._curv_f32(raw)
    for name, ref, spread, emu, emu_raw in (("K", K, sK, eK, rK), ("H", H, sH, eH, rH)):
        contract, term, drop = fe.foreign_bars(ref, spread, offset)
        for t in fe.FOREIGN_OFFSETS:
            r = offset == t
            assert drop[r].sum() <= 0.1 * r.sum(), (name, t)                         # the cap on rows without information
            if t <= 10:
                assert (term[r] <= contract[r]).all(), (name, t)                     # near the patch the contract rules
        assert (spread / contract).max() <= 2.5e-3                                   # the recorded largest spread
        keep = ~drop
        assert (np.abs(emu - ref)[keep] <= np.maximum(contract, term)[keep]).all(), name
        assert (np.abs(emu - ref) / contract).max() < 0.05
        far = offset == 1000.0
        print(f"{dtype.__name__} {name}: spread {float((spread / contract).max()):.1e} of the contract at most; moments about the query miss it "
              f"{float((np.abs(emu_raw - ref) / contract)[far].max()):.0f}-fold at 1 000 radii")
    # moments about the query (k_fit before this test): H leaves the contract at 1 000 radii
    contract = fe.foreign_bars(H, sH, offset)[0]
    assert (np.abs(rH - H) / contract)[offset == 1000.0].max() > 10


def test_vectorised_curvature_formulas_against_the_line_by_line_ones():
    """oracle._curv_f32(scalar_pow=True), the reference of the GPU test of the formulas, against oracle.quadric_curvatures
    (pct:398-431 line by line, on float32 scalars) over the whole coefficient space, inf and NaN included: H bit for bit.
    K and H^2 contain ``** 2`` of a float32 scalar, which is powf(x, 2) and not x * x: one ulp apart on a row in a
    thousand (the vectorised restatement and the kernel multiply)."""
    co = fe.coefficient_space()
    assert co.dtype == np.float32 and len(co) > 2000
    with np.errstate(all="ignore"):
        K, H, H2 = oracle._curv_f32(co, scalar_pow=True)
        rows = [oracle.quadric_curvatures(c) for c in co]
    for name, got, col in (("K", K, 0), ("H", H, 1), ("H2", H2, 4)):
        ref = np.array([r[col] for r in rows], np.float32)
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref)), name
        fin = np.isfinite(ref)
        off = np.abs(got[fin].astype(np.float64) - ref[fin]) / np.spacing(np.abs(ref[fin])).astype(np.float64)
        assert off.max() <= (0.0 if name == "H" else 1.0) and (off == 0).mean() >= 0.995, (name, off.max(), (off == 0).mean())
    slopes = np.hypot(co[:, 3].astype(np.float64), co[:, 4])
    assert (slopes == 0).any() and (slopes >= 1e3).any() and np.isinf(K).any() and np.isnan(H).any()

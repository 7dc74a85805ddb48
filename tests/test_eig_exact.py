"""The eigen stages' ground truth, checked on the CPU: the exact helper against itself, the ladders, the exclusion zones,
and the constants the GPU tests (tests/test_gpu_tangent_frame.py) hold the kernels to.  Nothing here touches the package.

What is pinned, and by what:
  * exact_cov / exact_eigen / exact_align against their definitions (A v = l v to the working precision, hand-made blocks,
    mpmath where it is importable);
  * the reference's own routes (np.cov + svd, np.cov + eigh, oracle.surface_variation's restatement) meet every bar on every
    rung, with every excluded row counted and the caps asserted -- so the bars are ones the reference meets;
  * the constants, re-measured;
  * teeth: the float64 emulation of the kernels meets every bar, and misses one with each of six planted defects.
"""
import importlib.util
from fractions import Fraction

import numpy as np
import pytest

import eig_exact as ee
import fit_exact as fe
import pct_oracle as oracle

DTYPES = (np.float32, np.float64)


def _all_facts():
    for dtype in DTYPES:
        for r in ee.rungs(dtype):
            for f in r["facts"]:
                yield dtype, r, f


def test_helper_agrees_with_itself():
    rng = np.random.default_rng(3)
    blk = rng.integers(-8, 9, (7, 3)).astype(np.float32) / np.float32(4)
    cov = ee.exact_cov(blk)
    mean = [sum(Fraction(float(x)) for x in blk[:, c]) / 7 for c in range(3)]
    for i in range(3):
        for j in range(3):
            want = sum((Fraction(float(p[i])) - mean[i]) * (Fraction(float(p[j])) - mean[j]) for p in blk) / 6
            assert cov[i][j] == want
    worst = 0.0
    for dtype, r, f in _all_facts():
        worst = max(worst, ee.residual(ee.exact_cov(f["block"]), f["eig"]))
        v = f["eig"]["vectors"]
        assert np.isfinite(v).all() and np.allclose((v * v).sum(0), 1.0, atol=1e-15)
        l = f["l"]
        assert l[0] >= l[1] >= l[2] >= 0.0
    assert worst <= 1e-58, worst                          # |A v - l v| / l1 (an exactly double root: half the digits, 1e-76)
    # exact structure: the identity block, the tie block, an exactly planar and an exactly collinear block
    f = ee.exact_align(ee.identity_block(np.float32))
    assert f["l"].tolist() == [12 / 7, 4 / 7, 0.5 / 7] and f["c"] == -1.0 and f["s"] == 0.0 and f["sens"] == np.inf
    assert np.array_equal(f["rot64"], ee.identity_block(np.float64)) and f["dot"] == 1.0
    p = ee.exact_pca(ee.tie_block())
    assert p["l"].tolist() == [8 / 7, 8 / 7, 0.5 / 7] and p["gaps"][0] < 1e-60 and p["K"] == float(Fraction(64, 49))
    f = ee.exact_align(ee.planar_block(50, np.float32))
    assert f["l"][2] == 0.0 and ee.up_to_sign(f["normal"], np.array([1, 0.5, -1]) / 1.5) <= 1e-16
    assert np.abs(f["rot64"][:, 2]).max() <= 1e-150                   # (the working precision)
    f = ee.exact_align(ee.collinear_block(50, np.float64))
    assert f["l"][1] == 0.0 and f["l"][2] == 0.0 and not ee.direction_defined(f)
    sv, l, den = ee.exact_surface_variation(ee.identity_block(np.float32))
    assert sv == float(Fraction(1, 14) / (Fraction(33, 14) + Fraction(1e-10)))


@pytest.mark.skipif(importlib.util.find_spec("mpmath") is None, reason="cross-check only; the helper stands on the stdlib")
def test_helper_agrees_with_mpmath():
    import mpmath
    old = mpmath.mp.dps
    mpmath.mp.dps = 70
    try:
        picks = [f for _, r, f in _all_facts() if r["m"] == 8 and r["ladder"] in ("gap3", "grading", "tilt-z")][::5]
        assert len(picks) > 40
        for f in picks:
            cov = ee.exact_cov(f["block"])
            A = mpmath.matrix([[mpmath.mpf(c.numerator) / c.denominator for c in row] for row in cov])
            E, Q = mpmath.eigsy(A)
            want = sorted((E[i] for i in range(3)), reverse=True)
            for got, w in zip(f["eig"]["dvalues"], want):
                assert abs(mpmath.mpf(str(got)) - w) <= mpmath.mpf(10) ** -55 * want[0]
            if ee.direction_defined(f):
                i3 = min(range(3), key=lambda i: E[i])
                n = np.array([float(Q[j, i3]) for j in range(3)])
                assert ee.up_to_sign(n, f["normal"]) <= 4 * 2.0 ** -53
    finally:
        mpmath.mp.dps = old


def test_restatement_is_the_oracle_and_the_identity_branch_is_real():
    """reference_align restates oracle.plane_align (bit for bit); the identity-branch block comes back unrotated from the
    reference in both orders, and flipped once it is tilted by the ladder's smallest angle."""
    for dtype, r, f in list(_all_facts())[::7]:
        if r["ladder"] == "collinear":
            continue
        assert np.array_equal(ee.reference_align(f["block"])[0], oracle.plane_align(f["block"]))
    for dtype in DTYPES:
        for rev in (False, True):
            b = ee.identity_block(dtype, reverse=rev)
            assert np.array_equal(oracle.plane_align(b), b.astype(np.float64))
    b = ee.identity_block(np.float64, tilt=min(ee.TILT_RUNGS))
    out = oracle.plane_align(b)
    assert np.array_equal(np.sign(out[[0, -1], 2]), -np.sign(b[[0, -1], 2]))
    f = ee.exact_align(b)
    assert ee.rotation_defined(f) and ee.align_shares(f, out)["rot"] <= 1.0


def test_ladders_walk_what_they_claim_and_every_exclusion_is_counted():
    for dtype in DTYPES:
        rs = ee.rungs(dtype)
        pooled = ee.assert_exclusion_caps(rs)
        by = {}
        for r in rs:
            by.setdefault(r["ladder"], []).append(r)
        assert set(by) == {"gap3", "gap1", "grading", "tilt-z", "tilt+z", "dot", "shape", "planar", "collinear"}
        assert {r["m"] for r in by["shape"]} == set(ee.SHAPE_M)
        f64 = dtype is np.float64
        # the gaps, the grading, the tilt and the dot product the stored blocks REALLY have follow the nominal rung
        for r in by["gap3"]:
            if r["cond"] >= (1e-12 if f64 else 1e-4):
                assert all(0.3 * r["cond"] <= f["gap3"] / f["l"][0] <= 3 * r["cond"] for f in r["facts"]), (dtype, r["cond"])
        for r in by["gap1"]:
            if r["cond"] >= (1e-12 if f64 else 1e-4):
                assert all(0.3 * r["cond"] <= f["gaps"][0] / f["l"][0] <= 3 * r["cond"] for f in r["facts"]), (dtype, r["cond"])
        for r in by["grading"]:
            assert all(0.3 * r["cond"] <= f["l"][2] / f["l"][0] <= 3 * r["cond"] for f in r["facts"]), (dtype, r["cond"])
        for r in by["tilt-z"] + by["tilt+z"]:
            if r["cond"] < 1.0 and r["cond"] >= (1e-9 if f64 else 1e-5):
                pole = -1.0 if r["ladder"] == "tilt-z" else 1.0
                assert all(f["c"] * pole > 0 and 0.3 * r["cond"] <= f["s"] <= 3 * r["cond"] for f in r["facts"]), (dtype, r["cond"])
        for r in by["dot"]:
            if r["m"] >= 5 and abs(r["cond"]) >= (1e-12 if f64 else 1e-5):
                assert all(0.5 * abs(r["cond"]) <= f["dot"] <= 2 * abs(r["cond"]) for f in r["facts"]), (dtype, r["cond"])
        n = sum(a["n"] for a in pooled.values())
        print(f"{dtype.__name__}: {len(rs)} rungs, {n} blocks; left out: direction {sum(a['gap'] for a in pooled.values())}, "
              f"orientation {sum(a['dot'] for a in pooled.values())}, rotation {sum(a['negz'] for a in pooled.values())}")


def test_reference_meets_every_bar_and_the_constants_hold():
    """The reference's own routes against the exact values, rung by rung; then C_NEEDED, re-measured (never against the
    GPU): neither short nor stale."""
    asserted = total = 0
    for dtype in DTYPES:
        tally = {}
        for r in ee.rungs(dtype):
            if r["ladder"] == "collinear":                            # (np.cov + svd of a line: finite, nothing else is defined)
                assert all(np.isfinite(ee.reference_align(f["block"])[0]).all() for f in r["facts"])
                continue
            _, _, a, n = ee.check_rung(r, [ee.reference_align(f["block"])[0] for f in r["facts"]], dtype.__name__)
            asserted += a
            total += n
            for f in r["facts"]:
                val, vec = ee.pca_shares(f["block"], ee.reference_pca(f["block"]), f.setdefault("pca", ee.exact_pca(f["block"])),
                                         tally, r)
                assert val <= 1.0 and vec <= 1.0, (dtype.__name__, r["ladder"], r["cond"], r["m"], val, vec)
                ok, share = ee.sv_within_bar(np.float32(ee.reference_surface_variation(f["block"])), f["block"])
                assert ok, (dtype.__name__, r["ladder"], r["cond"], r["m"], share)
        out, of = ee.assert_pca_caps(tally)           # the PCA directions the gap rule leaves out: counted per rung, capped
        print(f"{dtype.__name__}: {out} of {of} PCA direction assertions left out on the rungs outside the gap zones")
    assert total > 1200 and asserted >= 0.7 * total, (asserted, total)
    cal = ee.calibrate()
    print({k: (round(v, 2), w) for k, (v, w) in cal.items()})
    for kind, need in (("val", ee.C_VAL_NEEDED), ("vec", ee.C_VEC_NEEDED), ("rot", ee.C_ROT_NEEDED), ("dot", ee.C_DOT_NEEDED)):
        assert 0.5 * need <= cal[kind][0] <= need, (kind, cal[kind])
    assert (ee.C_VAL, ee.C_VEC, ee.C_ROT, ee.C_DOT) == tuple(4 * c for c in (ee.C_VAL_NEEDED, ee.C_VEC_NEEDED, ee.C_ROT_NEEDED, ee.C_DOT_NEEDED))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", ee.LADDER_M)
def test_cluster_neighbourhoods_keep_their_gaps(m, dtype):
    """The neighbourhoods the device's PCA is held on are not the rung blocks: a cluster row's neighbour set swaps one
    block point for the added one, the blocks are rescaled, float32 clouds are quantised.  The same walk as
    tests/test_gpu_tangent_frame.py (c), with the reference route: it meets the bars, and the gap rule leaves out at
    most 10 % of the direction assertions of every rung outside the gap zones -- also at the georeferenced offset."""
    blocks = ee.pca_blocks(m, dtype)
    for offset in ((0.0, 0.0, 0.0),) + ((ee.UTM_OFFSET,) if (m == 8 and dtype is np.float64) else ()):
        cloud, first = ee.cluster_cloud([b for _, b in blocks], dtype, offset=offset)
        tally = {}
        for c, row, nbrs in ee.cluster_rows(first, m):
            nb = cloud[nbrs]
            val, vec = ee.pca_shares(nb, ee.reference_pca(nb), None, tally, blocks[c][0])
            assert val <= 1.0 and vec <= 1.0, (blocks[c][0]["ladder"], blocks[c][0]["cond"], val, vec)
        out, of = ee.assert_pca_caps(tally)
        print(f"m={m} {dtype.__name__} offset {offset}: {out} of {of} direction assertions left out outside the gap zones")


def _reference_fused(block):
    return oracle.quadric_fit(oracle.plane_align(block))


@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_fit_of_the_exactly_rotated_block(dtype):
    """What ties the fused kernel to exact arithmetic (tests/test_gpu_tangent_frame.py (b)): on the rows whose exactly
    rotated coordinates are clear of every float32 rounding boundary, float32(R p) of ANY rotation within the bar is
    float32(R* p) -- and the reference's coefficients lie within fit_exact's bar of the exact least squares of that block.
    The boundary rule leaves out at most 1 % of the rows."""
    rows = clear = 0
    worst = 0.0
    by_ladder = {}
    for r in ee.fused_rungs(dtype):
        for f in r["facts"]:
            rows += 1
            if not (ee.boundary_clear(f) or r["ladder"] == "identity"):
                continue
            clear += 1
            assert np.array_equal(oracle.plane_align(f["block"]).astype(np.float32), f["rot32"]), (r["ladder"], r["cond"], r["m"])
            facts = f.setdefault("fit", fe.block_facts(f["rot32"]))
            co = _reference_fused(f["block"])
            ok, err, bar = fe.within_bar(co, facts)
            assert ok.all(), (r["ladder"], r["cond"], r["m"], err / bar)
            worst = max(worst, float((err / bar).max()))
            by_ladder.setdefault((r["m"], r["ladder"]), []).append((co, facts["c32"]))
    for key, pairs in by_ladder.items():          # K, H of the reference's coefficients: the 1e-5 contract, floor over the ladder
        (gK, gH, _), (rK, rH, _) = oracle._curv_f32(np.array([p[0] for p in pairs])), oracle._curv_f32(np.array([p[1] for p in pairs]))
        for got, ref in ((gK, rK), (gH, rH)):
            if not np.abs(ref).max() > 0:         # (the identity block: K == H == 0 exactly, a relative contract has no yardstick)
                continue
            assert oracle.curvature_tolerance_ok(got, ref, fe.FLOOR * np.abs(ref).max(), fe.RTOL).all(), (key, got, ref)
    assert rows > 100 and rows - clear <= 0.01 * rows, (rows, clear)
    print(f"{dtype.__name__}: {rows - clear} of {rows} rows within the bar of a float32 boundary; reference worst {worst:.3f} of the bar")


def _emulated_ok(dtype, ladders=None, pca=False, **defect):
    """True when the emulation (with the defect) meets every bar on the rungs of ``ladders``."""
    try:
        for r in ee.rungs(dtype):
            if r["ladder"] == "collinear" or (ladders and r["ladder"] not in ladders):
                continue
            for one_pass in ((True,) if "origin" in defect else (True, False)):
                ee.check_rung(r, [ee.emulate_align(f["block"], one_pass, **defect)[0] for f in r["facts"]])
    except AssertionError:
        return False
    return True


def test_teeth_six_planted_defects_each_miss_a_bar():
    worst = dict(val=0.0, vec=0.0)
    for dtype in DTYPES:
        assert _emulated_ok(dtype)                                            # the choreography itself passes everywhere
        for r in ee.rungs(dtype):
            for f in r["facts"]:
                val, vec = ee.pca_shares(f["block"], ee.emulate_pca(f["block"]), f.setdefault("pca", ee.exact_pca(f["block"])))
                assert val <= 1.0 and vec <= 1.0, (r["ladder"], r["cond"], val, vec)
                worst = dict(val=max(worst["val"], val), vec=max(worst["vec"], vec))
    print("emulated write_frame: worst shares", worst)
    sweeps = max(ee.emulate_align(f["block"], one_pass, sweeps=16)[3] for _, _, f in _all_facts() for one_pass in (True, False))
    assert sweeps <= 4, sweeps                                                # both caps (8 and 16) are slack
    far = lambda f: f["block"][0].astype(np.float64) + 1000.0 * np.abs(f["block"] - f["block"][0]).max()
    assert not _emulated_ok(np.float64, ("grading", "tilt-z"), sweeps=1)             # 1. the Jacobi capped at one sweep
    for r in ee.rungs(np.float64):                                                   # 2. moments about a far origin: the rotation
        if r["ladder"] == "grading" and r["cond"] == 1e-2 and r["m"] == 50:          #    bar, on EVERY row of grading 1e-2, m = 50
            shares = [ee.align_shares(f, ee.emulate_align(f["block"], True, origin=far(f))[0])["rot"] for f in r["facts"]]
            assert len(shares) == 4 and all(s is not None and s > 1.0 for s in shares), shares
            break
    else:
        raise AssertionError("rung not found")
    assert not _emulated_ok(np.float64, ("dot",), flip=False)                        # 3. the flip omitted
    assert not _emulated_ok(np.float64, ("tilt-z",), c_float32=True)                 # 4. c computed in float32
    got = ee.emulate_pca(ee.tie_block())                                             # 5. selection swapped on ties: the tie-order
    assert ee.tie_frame_ok(got[0][0], got[0][1], got[1])                             #    assertion of the GPU file's _check_pca
    bad = ee.emulate_pca(ee.tie_block(), ties_high_index_first=True)
    assert not ee.tie_frame_ok(bad[0][0], bad[0][1], bad[1])
    assert not _emulated_ok(np.float64, ("tilt-z",), s_zero_below=1e-8)              # 6. the identity branch taken early ...
    assert not _emulated_ok(np.float64, ("tilt+z",), s_zero_below=1e-8)              #    ... at either pole
    # the emulation also takes the true identity branch, and leaves it after the smallest tilt
    for dtype in DTYPES:
        b = ee.identity_block(dtype)
        assert np.array_equal(ee.emulate_align(b)[0], b.astype(np.float64))

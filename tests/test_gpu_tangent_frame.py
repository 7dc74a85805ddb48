"""The tangent-plane and PCA eigen stages on the device against an exact reference.

tests/eig_exact.py builds the cases and the bars (and says where every constant comes from); tests/test_eig_exact.py checks
on the CPU that the reference's own routes meet them and that six planted defects do not.  Here the kernels do:

  (a) k_plane_rotate (two-pass moments)        -- Handle.plane_rotate on every rung, one batch per (m, dtype); the identity
                                                  branch bit for bit, and left again after the ladder's smallest tilt
  (b) k_fit (one-pass moments) end to end      -- Handle.fit_indices / fit_indices_f64: on the rows clear of every float32
                                                  rounding boundary the design block IS float32(R* p), so the coefficients
                                                  are held to the exact least squares of the exactly rotated block
  (c) write_frame                              -- Handle.pca_curvatures on clusters whose neighbour sets are known
  (d) k_surface_variation                      -- the same clusters, scales 1 ... 1e-3 (the additive 1e-10 shows)
  (e) batch position                           -- identical bits wherever a neighbourhood sits

Every bar is the exact value; only (e) and the three-sweeps comparison in (c) compare the device with itself, and those
are invariances.  Every "worst error as a share of the bar" is printed: they are what the next change to these kernels
will be read against.
"""
import numpy as np
import pytest

import eig_exact as ee
import fit_exact as fe
import pct_oracle as oracle

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]


@pytest.fixture
def handle(gpu):
    h = gpu["capi"].Handle(0)
    yield h
    h.close()


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ (a) Handle.plane_rotate
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", ee.SHAPE_M)
def test_plane_rotate_on_every_rung(handle, m, dtype):
    rungs = [r for r in ee.rungs(dtype) if r["m"] == m]
    ee.assert_exclusion_caps(ee.rungs(dtype))
    blocks = np.array([f["block"] for r in rungs for f in r["facts"]], dtype)
    out = handle.plane_rotate(blocks)
    assert out.dtype == np.float64 and out.shape == blocks.shape
    at, report = 0, {}
    for r in rungs:
        n = len(r["facts"])
        res = out[at:at + n]
        at += n
        if r["ladder"] == "collinear":                 # no normal: finiteness and the row norms are all there is to assert
            assert np.isfinite(res).all()
            assert all(ee.align_shares(f, o)["norm"] <= 1.0 for f, o in zip(r["facts"], res))
            continue
        worst_r, worst_n, asserted, rows = ee.check_rung(r, res, dtype.__name__)
        acc = report.setdefault(r["ladder"], [0.0, 0.0, 0, 0])
        acc[0], acc[1], acc[2], acc[3] = max(acc[0], worst_r), max(acc[1], worst_n), acc[2] + asserted, acc[3] + rows
    for ladder, (wr, wn, asserted, rows) in report.items():
        print(f"plane_rotate m={m} {dtype.__name__} {ladder}: worst rotation error {wr:.3f} of the bar, norms {wn:.3f} of "
              f"{ee.NORM_EPS:g} eps, {rows - asserted} of {rows} rows left out")


@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_branch_bit_for_bit_and_left_after_the_smallest_tilt(handle, dtype):
    blocks = np.array([ee.identity_block(dtype, reverse=rev) for rev in (False, True)], dtype)
    out = handle.plane_rotate(blocks)
    assert np.array_equal(_bits64(out), _bits64(blocks.astype(np.float64)))
    theta = min(ee.TILT_RUNGS)
    tilted = ee.identity_block(np.float64, tilt=theta)                 # (float32 cannot hold a tilt of 1e-9)
    f = ee.exact_align(tilted)
    assert ee.rotation_defined(f) and abs(f["s"] - theta) <= 1e-3 * theta and f["c"] < 0
    got = handle.plane_rotate(tilted[None])[0]
    sh = ee.align_shares(f, got)
    assert sh["rot"] <= 1.0 and sh["norm"] <= 1.0 and sh["oriented"], sh
    assert np.array_equal(np.sign(got[[0, -1], 2]), -np.sign(tilted[[0, -1], 2]))      # flipped: a rotation by ~pi
    print(f"identity block tilted by {theta:g}: rotation error {sh['rot']:.2e} of the bar")


# ------------------------------------------------------------------------------------------------ (b) k_fit, end to end
def _fused_cloud(m, dtype):
    """Every fused-rung block of one m as ONE cloud: the query at the origin (record 0), one table row per block."""
    rungs = [r for r in ee.fused_rungs(dtype) if r["m"] == m]
    facts = [(r, f) for r in rungs for f in r["facts"]]
    pts = np.vstack([np.zeros((1, 3))] + [f["block"].astype(np.float64) for _, f in facts]).astype(dtype)
    idx = 1 + np.arange(len(facts) * m, dtype=np.int32).reshape(len(facts), m)
    return pts, idx, np.zeros(len(facts), np.int64), facts


def _clear_rows(dtype):
    """The boundary rule over ALL fused rows of a dtype: at most 1 % left out."""
    rows = [(r, f) for r in ee.fused_rungs(dtype) for f in r["facts"]]
    out = sum(not (ee.boundary_clear(f) or r["ladder"] == "identity") for r, f in rows)
    assert out <= 0.01 * len(rows), (out, len(rows))
    return out, len(rows)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", ee.FUSED_M)
def test_fused_fit_against_the_exact_fit_of_the_exactly_rotated_block(handle, m, dtype):
    left_out, total = _clear_rows(dtype)
    cloud, idx, query, facts = _fused_cloud(m, dtype)
    handle.set_points(cloud)
    handle.fit_indices(idx, query=query)
    co, K, H, H2 = handle.get_fit(0, len(idx))
    c64, K64, H64 = handle.fit_indices_f64(idx, query=query)
    worst = worst64 = 0.0
    by_ladder = {}
    for row, (r, f) in enumerate(facts):
        if not (ee.boundary_clear(f) or r["ladder"] == "identity"):
            continue
        fit = f.setdefault("fit", fe.block_facts(f["rot32"]))
        where = (m, dtype.__name__, r["ladder"], r["cond"])
        ok, err, bar = fe.within_bar(co[row], fit)
        assert ok.all(), (where, err / bar)
        worst = max(worst, float((err / bar).max()))
        ok, err, bar = fe.within_bar(c64[row], fit, rounded=False)          # the conditioning term alone
        assert ok.all(), (where, "f64", err / bar)
        worst64 = max(worst64, float((err / bar).max()))
        by_ladder.setdefault(r["ladder"], []).append((row, fit["c32"]))
    for ladder, rows in by_ladder.items():                                   # K, H: the 1e-5 contract, floor over the ladder
        sel = np.array([row for row, _ in rows])
        rK, rH, _ = oracle._curv_f32(np.array([c for _, c in rows]))
        for name, got, ref in (("K", K[sel], rK), ("H", H[sel], rH)):
            if not np.abs(ref).max() > 0:     # (the identity block: K == H == 0 exactly, a relative contract has no yardstick;
                continue                      #  its coefficients are held above like any others)
            ok = oracle.curvature_tolerance_ok(got, ref, fe.FLOOR * np.abs(ref).max(), fe.RTOL)
            assert ok.all(), (m, dtype.__name__, ladder, name, got[~ok], ref[~ok])
    print(f"k_fit m={m} {dtype.__name__}: {len(facts)} rows, worst coefficient error {worst:.3f} of the bar, unrounded "
          f"{worst64:.3f} of C eps kappa S; boundary rule leaves out {left_out} of {total} rows of this dtype")


# ------------------------------------------------------------------------------------------------ (c) write_frame
def _algos(gpu):
    capi = gpu["capi"]
    algos = {"brute": capi.KNN_BRUTE, "grid": capi.KNN_GRID, "tree": capi.KNN_TREE}
    assert len({capi.KNN_AUTO, *algos.values()}) == 4                          # three different sweeps, none of them "auto"
    return algos


def _run_pca(handle, cloud, m, algo):
    handle.set_points(cloud)
    handle.pca_curvatures(m, algo, keep_neighbors=True)
    return handle.get_pca(0, len(cloud), want_idx=True)


def _check_pca(cloud, first, blocks, m, got, where):
    l1, l2, dirs, K, H, idx = got
    n = len(cloud)
    cluster = np.arange(n) // (m + 1)
    # keep_neighbors: every row was computed from the rest of its cluster
    want = np.array([[j for j in range(c * (m + 1), (c + 1) * (m + 1)) if j != i] for i, c in enumerate(cluster)])
    assert np.array_equal(np.sort(idx, 1), want), where
    first_max = np.take_along_axis(dirs, np.abs(dirs).argmax(axis=1)[:, None, :], 1)[:, 0, :]
    assert (first_max >= 0).all(), where                                       # the documented sign rule
    worst, tally = {}, {}
    for c, row, nbrs in ee.cluster_rows(first, m):                             # the added point's row and one of the block's own
        r = blocks[c][0]
        assert np.array_equal(nbrs, want[row])
        nb = cloud[nbrs]
        ex = ee.exact_pca(nb)
        val, vec = ee.pca_shares(nb, (np.array([l1[row], l2[row]]), dirs[row], K[row], H[row]), ex, tally, r)
        assert val <= 1.0 and vec <= 1.0, (where, r["ladder"], r["cond"], val, vec, ex["l"])
        w = worst.setdefault(r["ladder"], [0.0, 0.0])
        w[0], w[1] = max(w[0], val), max(w[1], vec)
        if r["ladder"] == "tie" and row == first[c]:                           # exactly equal l1 == l2: lower index first
            assert ee.tie_frame_ok(l1[row], l2[row], dirs[row]), (l1[row], l2[row], dirs[row])
    out, total = ee.assert_pca_caps(tally)      # every direction the gap rule leaves out is counted; cap 10 % outside the gap zones
    for ladder, (val, vec) in worst.items():
        skipped = sum(a["skipped"] for (lad, _), a in tally.items() if lad == ladder)
        asked = sum(a["n"] for (lad, _), a in tally.items() if lad == ladder)
        print(f"pca {where} {ladder}: worst value error {val:.3f}, direction error {vec:.3f} of the bar, "
              f"{skipped} of {asked} direction assertions left out (gap)")
    print(f"pca {where}: {out} of {total} direction assertions left out on the rungs outside the gap zones")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", ee.LADDER_M)
def test_pca_frame_on_clusters(handle, gpu, m, dtype):
    algos = _algos(gpu)
    blocks = ee.pca_blocks(m, dtype)
    cloud, first = ee.cluster_cloud([b for _, b in blocks], dtype)
    base = _run_pca(handle, cloud, m, algos["brute"])
    _check_pca(cloud, first, blocks, m, base, f"m={m} {dtype.__name__}")
    for name in ("grid", "tree"):                                              # all three sweeps: identical bits
        got = _run_pca(handle, cloud, m, algos[name])
        for a, b in zip(got[:5], base[:5]):
            assert np.array_equal(_bits64(a), _bits64(b)), (name, m, dtype.__name__)
        assert np.array_equal(np.sort(got[5], 1), np.sort(base[5], 1))


def test_pca_frame_at_a_georeferenced_offset(handle, gpu):
    """The float64 clusters at a UTM-like offset: the exact values are those of the STORED coordinates."""
    blocks = ee.pca_blocks(8, np.float64)
    cloud, first = ee.cluster_cloud([b for _, b in blocks], np.float64, offset=ee.UTM_OFFSET)
    _check_pca(cloud, first, blocks, 8, _run_pca(handle, cloud, 8, gpu["capi"].KNN_AUTO), "m=8 float64 at (4.2e5, 5.1e6, 250)")


# ------------------------------------------------------------------------------------------------ (d) surface variation
@pytest.mark.parametrize("scale", [1.0, 1e-1, 1e-2, 1e-3])
@pytest.mark.parametrize("m", ee.LADDER_M)
def test_surface_variation_on_clusters(handle, m, scale):
    blocks = [(r, f["block"]) for r in ee.rungs(np.float32) if r["m"] == m and r["ladder"] in ("gap3", "grading", "planar")
              for f in r["facts"]]
    spacing = 2.0 ** np.round(np.log2(16.0 * scale))
    cloud, first = ee.cluster_cloud([b for _, b in blocks], np.float32, spacing=spacing, radius=scale)
    handle.set_points(cloud)
    sv = handle.surface_variation(m + 1)
    assert sv.dtype == np.float32 and sv.shape == (len(cloud),)
    worst, eps_share = 0.0, 0.0
    for (r, _), at in zip(blocks, first):
        want, bar, den = ee.sv_bar(cloud[at:at + m + 1])                       # the whole cluster is every row's neighbourhood
        eps_share = max(eps_share, ee.SV_EPSILON / den)
        share = np.abs(sv[at:at + m + 1].astype(np.float64) - want) / bar
        assert (share <= 1.0).all(), (m, scale, r["ladder"], r["cond"], share.max(), want)
        worst = max(worst, float(share.max()))
    assert (scale > 1e-3) or eps_share > 1e-4                                  # the 1e-10 is visible in float32 at the small end
    print(f"surface variation m={m} scale={scale:g}: worst error {worst:.3f} of the bar; 1e-10 is up to {eps_share:.1e} of the denominator")


# ------------------------------------------------------------------------------------------------ (e) batch position
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_neighbourhood_gives_the_same_bits_in_every_batch_slot(handle, dtype):
    blocks = np.array([f["block"] for r in ee.rungs(dtype) if r["m"] == 8 and r["ladder"] != "collinear" for f in r["facts"]][:256:4], dtype)
    assert len(blocks) == 64
    base = _bits64(handle.plane_rotate(blocks))
    for rows in (1, 63, 64, 65, 513):
        tile = np.arange(rows) % 64
        assert np.array_equal(_bits64(handle.plane_rotate(blocks[tile])), base[tile]), rows

"""plane_rotation()'s two routes to the normal on the device: direct_normal() (the default on healthy rows) against the
cyclic Jacobi (the fallback, and every row under PCT_FIT_JACOBI=1, read per call).

tests/test_eig_direct_route.py states the direct route on the CPU and holds it to eig_exact's bars; here the kernels are:

  rungs      Handle.plane_rotate on every rung of eig_exact.rungs(dtype, ms=(8, 50), rows=4): each route passes
             check_rung, and the two agree within the sum of their bars
  one wave   130 blocks of m = 8 (a wave boundary inside), healthy blocks alternating with collinear blocks, blocks
             whose two small eigenvalues tie, and gap3 = 1e-10 blocks: the healthy rows carry the bits of the all-healthy
             batch, the others the bits of the PCT_FIT_JACOBI=1 run
  fused      a 192-point cloud of three clusters at k = 8, default against the switch: K, H within the contract,
             the same rows handed to k_fit_svd
  scaling    a block scaled by 2^-200 and 2^+200 comes back with the same bits, scaled
"""
import numpy as np
import pytest

import eig_exact as ee
import fit_exact as fe
import pct_oracle as oracle
from test_eig_direct_route import direct_normal

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]


@pytest.fixture
def handle(gpu):
    h = gpu["capi"].Handle(0)
    yield h
    h.close()


def _route(monkeypatch, jacobi):
    if jacobi:
        monkeypatch.setenv("PCT_FIT_JACOBI", "1")
    else:
        monkeypatch.delenv("PCT_FIT_JACOBI", raising=False)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _healthy(block):
    """The CPU statement of the health test on k_plane_rotate's (two-pass) moments."""
    return direct_normal(ee._moments(block, False))[0] is not None


# ------------------------------------------------------------------------------------------------ rungs
@pytest.mark.parametrize("dtype", DTYPES)
def test_both_routes_on_every_rung(handle, monkeypatch, dtype):
    rungs = ee.rungs(dtype, ms=(8, 50), rows=4)
    worst = {False: 0.0, True: 0.0}
    apart = differ = 0.0
    for m in sorted({r["m"] for r in rungs}):
        mine = [r for r in rungs if r["m"] == m]
        blocks = np.array([f["block"] for r in mine for f in r["facts"]], dtype)
        out = {}
        for jacobi in (False, True):
            _route(monkeypatch, jacobi)
            out[jacobi] = handle.plane_rotate(blocks)
        differ += float((_bits64(out[False]) != _bits64(out[True])).any())
        at = 0
        for r in mine:
            n = len(r["facts"])
            for jacobi in (False, True):
                res = out[jacobi][at:at + n]
                if r["ladder"] == "collinear":             # no normal: finiteness and the row norms are all there is
                    assert np.isfinite(res).all()
                    assert all(ee.align_shares(f, o)["norm"] <= 1.0 for f, o in zip(r["facts"], res))
                    continue
                wr = ee.check_rung(r, res, f"{dtype.__name__} {'jacobi' if jacobi else 'direct'}")[0]
                worst[jacobi] = max(worst[jacobi], wr)
            for i, f in enumerate(r["facts"]):              # route against route: within the sum of the two bars
                if ee.rotation_defined(f):
                    gap = np.abs(out[False][at + i] - out[True][at + i]).max(1)
                    bar = 2.0 * ee.C_ROT * ee.rot_unit(f)
                    nz = f["pnorm"] > 0
                    assert (gap[nz] <= bar[nz]).all(), (dtype.__name__, r["ladder"], r["cond"], m, (gap[nz] / bar[nz]).max())
                    apart = max(apart, float((gap[nz] / bar[nz]).max()))
            at += n
    assert differ > 0                                       # the switch switches: some batch differs in some bit
    print(f"plane_rotate {dtype.__name__}: worst rotation error direct {worst[False]:.3f}, Jacobi {worst[True]:.3f} of the bar; "
          f"the routes at most {apart:.3f} of the summed bars apart")


# ------------------------------------------------------------------------------------------------ one wave
def _small_tie_block(dtype):
    """The corners (+-1, +-1/4, +-1/4): cov == diag(8, 1/2, 1/2) / 7, l2 == l3 exactly -- a double root of the cubic."""
    return np.array([[x, y, z] for x in (1, -1) for y in (0.25, -0.25) for z in (0.25, -0.25)], dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fallback_rows_inside_one_wave(handle, monkeypatch, dtype):
    rungs = ee.rungs(dtype)
    healthy = [f["block"] for r in rungs if r["m"] == 8 and r["ladder"] in ("shape", "tilt+z", "grading", "dot") for f in r["facts"]]
    healthy = [b for b in healthy if _healthy(b)][:32]
    sick = [ee.collinear_block(8, dtype), _small_tie_block(dtype)] + ee.gap_blocks(3, 1e-10, 8, dtype, 2)
    assert len(healthy) == 32 and not any(_healthy(b) for b in sick)
    slots = 130
    base = np.array([healthy[i % 32] for i in range(slots)], dtype)
    mixed = base.copy()
    odd = np.arange(1, slots, 2)
    for i in odd:
        mixed[i] = sick[(i // 2) % len(sick)]
    _route(monkeypatch, False)
    out_base, out_mixed = handle.plane_rotate(base), handle.plane_rotate(mixed)
    _route(monkeypatch, True)
    out_jacobi = handle.plane_rotate(mixed)
    even = np.arange(0, slots, 2)
    assert np.isfinite(out_mixed).all()
    assert np.array_equal(_bits64(out_mixed[even]), _bits64(out_base[even]))           # healthy rows: untouched by their neighbours
    assert np.array_equal(_bits64(out_mixed[odd]), _bits64(out_jacobi[odd]))           # fallback rows: the Jacobi's bits
    assert (_bits64(out_mixed[even]) != _bits64(out_jacobi[even])).any()               # ... and the healthy rows took another route


# ------------------------------------------------------------------------------------------------ fused
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_step_default_against_the_switch(handle, gpu, monkeypatch, dtype):
    rng = np.random.default_rng(ee.LADDER_SEED + 21)
    blocks = [ee.make_block(rng, 63, lam, ee.GENERIC_NORMAL, 0.3, np.float64) for lam in ((1.0, 0.6, 0.2), (1.0, 0.5, 1e-2), (1.0, 0.06, 0.05))]
    cloud, _ = ee.cluster_cloud(blocks, dtype)
    assert cloud.shape == (192, 3)
    got = {}
    for jacobi in (False, True):
        _route(monkeypatch, jacobi)
        handle.set_points(cloud)
        handle.curvature(8, algo=gpu["capi"].KNN_AUTO)
        _, K, H, _ = handle.get_fit(0, len(cloud))
        got[jacobi] = (K.copy(), H.copy(), handle.timings()["fit_svd_rows"])
    (K, H, svd), (rK, rH, rsvd) = got[False], got[True]
    assert svd == rsvd, (svd, rsvd)
    assert np.isfinite(rK).all() and np.isfinite(rH).all()
    for name, x, ref in (("K", K, rK), ("H", H, rH)):
        ok = oracle.curvature_tolerance_ok(x, ref, fe.FLOOR * np.abs(ref).max(), fe.RTOL)
        assert ok.all(), (name, dtype.__name__, np.flatnonzero(~ok), x[~ok], ref[~ok])
    print(f"fused {dtype.__name__}: {int((K != rK).sum())} K and {int((H != rH).sum())} H of {len(K)} rows differ in a bit; {svd} rows to k_fit_svd")


# ------------------------------------------------------------------------------------------------ scaling
def test_scaled_blocks_keep_their_bits(handle):
    rng = np.random.default_rng(ee.LADDER_SEED + 14)
    b = ee.make_block(rng, 50, (1.0, 0.6, 0.2), ee.GENERIC_NORMAL, 0.3, np.float64)
    assert _healthy(b)
    f = ee.exact_align(b)
    base = handle.plane_rotate(b[None])[0]
    sh = ee.align_shares(f, base)
    assert sh["rot"] <= 1.0 and sh["norm"] <= 1.0 and sh["oriented"], sh
    for e in (-200, 200):
        out = handle.plane_rotate((b * 2.0 ** e)[None])[0]
        assert np.array_equal(_bits64(out), _bits64(base * 2.0 ** e)), e        # the same rotation bits: R p scales exactly

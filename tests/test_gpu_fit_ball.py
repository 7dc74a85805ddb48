"""Curvature over radius neighbourhoods on the device (pct_fit_ball; csrc/pct_fit_ball.hip) against
``ball_fit_exact.reference`` -- the oracle's reference-faithful loop on the ranked members of every ball -- under the
project's contract: ``curvature_tolerance_ok``, rtol 1e-5, floor 1e-2 x the curvature scale (torus: K 9, H 3; the float64
torus scaled by 0.2: K 225, H 15; flat, line, twins, clump: 1 for both).

Every row of at least four members is held to the contract; rows of two or three members must be finite, rows of fewer
than two NaN; nothing else is left out (tests/test_ball_fit_exact.py pins on the CPU that the exemption is exactly
``members < 4`` and that the order of the members between near and far does not matter).  ``used`` is compared exactly."""
import numpy as np
import pytest

import ball_exact as be
import ball_fit_exact as bfe
import pct_oracle as oracle
import wide_exact as we

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bench(gpu):
    capi = gpu["capi"]
    h = capi.Handle(0)
    cache = {}

    def once(key, make):
        if key not in cache:
            cache[key] = make()
            for a in cache[key] if isinstance(cache[key], tuple) else ():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        return cache[key]
    yield {"h": h, "capi": capi, "once": once, "PointCloud": gpu["PointCloud"]}
    h.close()


def _fit(h, centres):
    used = h.fit_ball(centres)
    coefs, K, H, H2 = h.get_fit(0, len(centres))
    return coefs, K, H, H2, used


def _ball_fit(bench, pts, centres, r, queries=None, flags=None, algo=None, fresh=True):
    h, capi = bench["h"], bench["capi"]
    if fresh:
        h.set_points(pts)
    q = np.asarray(pts)[centres].astype(np.float64) if queries is None else queries
    st, _ = h.query_ball(q, r, capi.BALL_SORTED if flags is None else flags, capi.QUERY_AUTO if algo is None else algo)
    assert st == capi.PCT_OK
    return _fit(h, centres)


def _hold(got, ref, scales, where, members=None):
    """used exactly; NaN exactly where used < 2; finite elsewhere; the contract on every row of >= 4 members."""
    coefs, K, H, H2, used = got
    rused = ref[4] if members is None else members
    assert used.dtype == np.int32 and np.array_equal(used, rused), (where, "used", np.flatnonzero(used != rused)[:8])
    none = rused < 2
    for name, a in (("coefs", coefs), ("K", K), ("H", H), ("H2", H2)):
        a2 = a.reshape(len(a), -1)
        assert np.isnan(a2[none]).all(), (where, name, "not NaN below two members")
        assert np.isfinite(a2[~none]).all(), (where, name, "not finite", np.flatnonzero(~np.isfinite(a2).all(1) & ~none)[:8], rused[np.flatnonzero(~np.isfinite(a2).all(1) & ~none)[:8]])
    rows = rused >= bfe.MIN_MEMBERS
    okK = oracle.curvature_tolerance_ok(K[rows], ref[1][rows], 1e-2 * scales[0])
    okH = oracle.curvature_tolerance_ok(H[rows], ref[2][rows], 1e-2 * scales[1])
    dK = np.abs(K[rows].astype(np.float64) - ref[1][rows]).max(initial=0.0)
    dH = np.abs(H[rows].astype(np.float64) - ref[2][rows]).max(initial=0.0)
    print(f"{where}: {int(rows.sum())} rows held, max|dK| {dK:.3e} max|dH| {dH:.3e}, K misses {int((~okK).sum())} H misses {int((~okH).sum())}")
    bad = np.flatnonzero(~(okK & okH))
    assert okK.all() and okH.all(), (where, "contract", np.flatnonzero(rows)[bad][:8], rused[np.flatnonzero(rows)[bad][:8]])
    assert np.array_equal(H2[rows].view(np.uint32), (H[rows] * H[rows]).view(np.uint32)), (where, "H2 is not H * H in float32")


def _ladder(bench):
    def make():
        pts, centres, q, r = bfe.ladder_case(we)
        ranked = bfe.ranked_rows(pts, centres, r, queries=q)
        return (pts, centres, q, r, ranked, bfe.reference(pts, centres, ranked=ranked))
    return bench["once"]("ladder", make)


def _same_bytes(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


# ---- the length ladder ---------------------------------------------------------------------------------------------------
def test_length_ladder(bench):
    pts, centres, q, r, ranked, ref = _ladder(bench)
    members = bfe.ladder_members()
    assert set(members.tolist()) >= set(range(130)) | {254, 255, 256, 510, 511, 512, 1022, 1023, 1024, 2046, 2047, 2048}
    got = _ball_fit(bench, pts, centres, r, queries=q)
    _hold(got, ref, bfe.SCALES["torus"], "ladder", members=members.astype(np.int32))
    t = bench["h"].timings()
    assert t["fit_svd_rows"] >= int((members < 6).sum()), (t["fit_svd_rows"], int((members < 6).sum()))
    assert t["fit_ms"] > 0


def test_ladder_rows_through_the_pinned_path(bench):
    """Rows of at most 511 members as ranked, padded rows through pct_fit_indices: the pinned k_fit / k_fit_svd."""
    pts, centres, q, r, ranked, ref = _ladder(bench)
    h = bench["h"]
    used = ref[4]
    take = np.flatnonzero((used >= 2) & (used <= 511))
    idx, count = bfe.padded([ranked[i] for i in take])
    h.set_points(pts)
    h.fit_indices(idx, count, centres[take])
    coefs, K, H, H2 = h.get_fit(0, len(take))
    sub = tuple(a[take] for a in ref)
    _hold((coefs, K, H, H2, count), sub, bfe.SCALES["torus"], "ladder through pct_fit_indices")


def test_wave_route_against_table_route(bench, monkeypatch):
    pts, centres, q, r, ranked, ref = _ladder(bench)
    monkeypatch.setenv("PCT_FIT_BALL_ROUTE", "wave")
    wave = _ball_fit(bench, pts, centres, r, queries=q)
    monkeypatch.setenv("PCT_FIT_BALL_ROUTE", "table")
    table = _ball_fit(bench, pts, centres, r, queries=q)
    monkeypatch.delenv("PCT_FIT_BALL_ROUTE")
    _hold(wave, ref, bfe.SCALES["torus"], "ladder, wave route")
    _hold(table, ref, bfe.SCALES["torus"], "ladder, table route")
    # the rows both routes can take, route against route
    both = (ref[4] >= bfe.MIN_MEMBERS) & (ref[4] <= 64)
    assert both.sum() >= 16 * 60
    assert oracle.curvature_tolerance_ok(wave[1][both], table[1][both], 1e-2 * 9.0).all()
    assert oracle.curvature_tolerance_ok(wave[2][both], table[2][both], 1e-2 * 3.0).all()
    long_rows = ref[4] > 64                                        # beyond the pitch `table` changes nothing
    assert _same_bytes([a[long_rows] for a in wave], [a[long_rows] for a in table])


# ---- against the k-NN path -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (30, 80))
def test_against_knn_fit(bench, k):
    h, capi = bench["h"], bench["capi"]
    pts = we.torus()
    ranking = bench["once"]("torus ranking", lambda: we.ranked(pts, width=82))
    assert not we.tie_at(ranking, k).any()
    r = bfe.knn_radii(we, pts, k, ranking)
    h.set_points(pts)
    h.knn(k)
    h.fit()
    _, Kk, Hk, _ = h.get_fit(0, len(pts))
    centres = np.arange(len(pts), dtype=np.int64)
    coefs, K, H, H2, used = _ball_fit(bench, pts, centres, r, fresh=False)
    assert (used == k).all()
    okK = oracle.curvature_tolerance_ok(K, Kk, 1e-2 * 9.0)
    okH = oracle.curvature_tolerance_ok(H, Hk, 1e-2 * 3.0)
    print(f"k={k}: max|dK| {np.abs(K - Kk).max():.3e} max|dH| {np.abs(H - Hk).max():.3e}")
    assert okK.all() and okH.all(), (int((~okK).sum()), int((~okH).sum()))


# ---- other clouds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(bfe.cloud_cases(we)))
def test_other_clouds(bench, name):
    key, pts, centres, r = bfe.cloud_cases(we)[name]
    ref = bench["once"](name, lambda: bfe.reference(pts, centres, r))
    if key == "clump":
        assert ref[4].max() > 2048
    got = _ball_fit(bench, pts, centres, r)
    _hold(got, ref, bfe.SCALES[key], name)


# ---- determinism and state -------------------------------------------------------------------------------------------------
def _mixed_case():
    pts = we.torus()
    centres = bfe.seeded_centres(len(pts), 6)
    r = np.linspace(0.03, 0.45, len(centres))                      # rows of a few to a few hundred members: both routes
    return pts, centres, r


def test_same_bytes_by_every_query_route_and_on_repeat(bench):
    h, capi = bench["h"], bench["capi"]
    pts, centres, r = _mixed_case()
    q = pts[centres].astype(np.float64)
    got = {}
    for way in ("build", "resident", "sweep"):
        h.set_points(pts)
        if way == "resident":
            h.knn(20, 0.0, capi.KNN_GRID)
        st, _ = h.query_ball(q, r, capi.BALL_SORTED, capi.QUERY_SWEEP if way == "sweep" else capi.QUERY_GRID)
        assert st == capi.PCT_OK and h.ball_stats()["route"] == {"sweep": 0, "resident": 1, "build": 2}[way]
        got[way] = _fit(h, centres)
        assert _same_bytes(got[way], _fit(h, centres)), (way, "a repeat call differs")
    assert got["build"][4].min() < 16 and got["build"][4].max() > 128
    assert _same_bytes(got["build"], got["resident"]) and _same_bytes(got["build"], got["sweep"])
    ref = bench["once"]("mixed", lambda: bfe.reference(pts, centres, r))
    _hold(got["build"], ref, bfe.SCALES["torus"], "mixed radii, sorted")
    # unsorted rows, with distances: the same members in another order
    st, _ = h.query_ball(q, r, capi.BALL_DISTANCES, capi.QUERY_GRID)
    assert st == capi.PCT_OK
    raw = _fit(h, centres)
    assert _same_bytes(raw, _fit(h, centres))
    _hold(raw, ref, bfe.SCALES["torus"], "mixed radii, unsorted")


def test_table_and_rows_survive(bench):
    h, capi = bench["h"], bench["capi"]
    pts, centres, r = _mixed_case()
    h.set_points(pts)
    h.knn(20)
    table = h.get_neighbors(0, len(pts), True, True, True)
    h.fit()
    fit0 = h.get_fit(0, len(pts))
    got = _ball_fit(bench, pts, centres, r, fresh=False)
    rows = h.get_ball(0, len(centres))
    again = h.get_neighbors(0, len(pts), True, True, True)
    assert _same_bytes(table, again)
    assert _same_bytes(got, _fit(h, centres)) and np.array_equal(rows, h.get_ball(0, len(centres)))
    h.fit()
    assert _same_bytes(fit0, h.get_fit(0, len(pts)))


def test_waits_for_a_pending_call(bench):
    h, capi = bench["h"], bench["capi"]
    pts, centres, r = _mixed_case()
    ref = bench["once"]("mixed", lambda: bfe.reference(pts, centres, r))
    h.set_points(pts)
    st, _ = h.query_ball(pts[centres].astype(np.float64), r, capi.BALL_SORTED)
    assert st == capi.PCT_OK
    h.set_async(True)
    try:
        h.curvature(30)                                            # returns with its kernels enqueued
        got = _fit(h, centres)
    finally:
        h.set_async(False)
    _hold(got, ref, bfe.SCALES["torus"], "behind a pending call")


# ---- errors ------------------------------------------------------------------------------------------------------------------
def test_errors(bench):
    h, capi = bench["h"], bench["capi"]
    pts = we.torus()
    centres = np.arange(50, dtype=np.int64)
    q = pts[centres].astype(np.float64)
    h.set_points(pts)
    with pytest.raises(AttributeError):                            # PCT_ERR_NO_NEIGHBORS: nothing queried
        h.fit_ball(centres)
    h.query_ball(q, 0.1, capi.BALL_COUNT_ONLY)
    with pytest.raises(AttributeError):                            # a count-only query leaves no rows
        h.fit_ball(centres)
    st, off = h.query_ball(q, 0.1, capi.BALL_SORTED, capi.QUERY_AUTO, 5)
    assert st == capi.PCT_ERR_LIMIT
    with pytest.raises(AttributeError):                            # a capped query neither
        h.fit_ball(centres)
    st, off = h.query_ball(q, 0.1)
    assert st == capi.PCT_OK
    with pytest.raises(ValueError):                                # not the row count of the last query
        h.fit_ball(centres[:49])
    with pytest.raises(ValueError):
        h.fit_ball(np.arange(51, dtype=np.int64))
    for bad in (-1, len(pts), 1 << 40):
        c = centres.copy()
        c[17] = bad
        with pytest.raises(ValueError):                            # a centre outside [0, n)
            h.fit_ball(c)
    assert (h.fit_ball(centres) == np.diff(off) - 1).all()         # ... and the rows are still there
    h.set_query_slab(0, 1)
    try:
        with pytest.raises(ValueError):                            # a slab handle
            h.fit_ball(centres)
    finally:
        h.set_query_range(0, len(pts))
    h.fit_ball(centres)
    h.set_points(pts)                                              # a new cloud drops the rows
    with pytest.raises(AttributeError):
        h.fit_ball(centres)


# ---- the class ---------------------------------------------------------------------------------------------------------------
def test_class_chunks_subsets_and_radii(bench):
    PointCloud = bench["PointCloud"]
    pts = we.torus()
    pc = PointCloud(points=pts, normals=np.zeros((len(pts), 0)))
    try:
        K, H = pc.compute_curvature_ball(0.1)
        whole = (K.copy(), H.copy(), pc.K_H_sq_quadratic.copy(), np.array(pc.quadratic_coefficients), pc.neighbor_counts.copy())
        assert K.dtype == np.float32 and H.dtype == np.float32 and len(K) == len(pts)
        counts = whole[4]
        entries = int(counts.sum()) + len(pts)
        K2, H2 = pc.compute_curvature_ball(0.1, max_entries=entries // 3)           # at least three chunks
        assert entries // 3 < entries and -(-entries // (entries // 3)) >= 3
        chunked = (K2, H2, pc.K_H_sq_quadratic, np.array(pc.quadratic_coefficients), pc.neighbor_counts)
        assert _same_bytes(whole, chunked)
        sample = bfe.seeded_centres(len(pts), 7)
        ref = bench["once"]("class r=0.1", lambda: bfe.reference(pts, sample, 0.1))
        assert np.array_equal(counts[sample], ref[4])
        _hold(tuple(a[sample] for a in (whole[3], whole[0], whole[1], whole[2], whole[4])), ref, bfe.SCALES["torus"], "class, r = 0.1")
        # a subset of rows (unordered, one repeated) with one radius per centre
        rows = np.concatenate([sample[::-1][:200], sample[:1]])
        radii = np.linspace(0.05, 0.3, len(rows))
        Ks, Hs = pc.compute_curvature_ball(radii, rows=rows)
        ref2 = bfe.reference(pts, rows, radii)
        got = (np.array(pc.quadratic_coefficients), Ks, Hs, pc.K_H_sq_quadratic, pc.neighbor_counts)
        _hold(got, ref2, bfe.SCALES["torus"], "class, rows= and per-centre radii")
        with pytest.raises(ValueError):
            pc.compute_curvature_ball(0.1, rows=[len(pts)])
    finally:
        pc.close()

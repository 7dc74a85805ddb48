"""The kernels that plan the passes of the chained sweep (csrc/pct_levels.hip) on the device, against tests/levels_exact.py.

pct_selftest_levels_classify / _bands / _merge launch k_classify, k_band_hist, k_band_box and k_merge_rows as
pct_knn_levels launches them, on arrays made here.  Every word that comes back is compared bit for bit with the NumPy
restatement (which tests/test_levels_exact.py holds the host build of csrc/pct_levels_plan.h to) -- bins, counts, boxes,
brackets, merged tables with their padding columns and everything a kernel must leave alone.  The one allowance is the
population step of k_classify, which goes through log2f: the device's value must follow exactly from the float64 logarithm
rounded to float32 or one of its two float32 neighbours (the 1 ulp HIP documents); the test prints how many rows were
not the nearest.  Measured on the MI355X: 2 681 of the 55 055 rows through log2f in the largest case (4.9 %), none outside
the three values; the host's log2f gave the nearest in every case of tests/test_levels_exact.py.

Wanted edges no pass can produce (infinities, huge values, the strip [0.4e30, 0.5e30) that bin 159 counts and no window
owns) are in the band cases as documented behaviour; `window members == hist[b .. b + 3]` is asserted with the strip
taken off the last window, which is the only place the two differ.

The last test is one fused PCT_KNN_GRID_LEVELS call of at least two passes under an eps bound that leaves
under-determined rows: the rows handed to k_fit_svd, summed over the passes, equal those of PCT_KNN_BRUTE.

Run time on one MI355X: 1.6 s for the file (23 tests; the slowest, test_bands[131329], 0.2 s)."""
import numpy as np
import pytest

import levels_exact as lx
import pct_oracle as oracle

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def handle(gpu):
    h = gpu["capi"].Handle(0)
    yield h
    h.close()


# ---------------------------------------------------------------------------------------------------------------- bands
BAND_N = [1, 255, 256, 257, 131072 + 257]          # the last: more than 512 blocks x 256 threads, the grid-stride loop runs
BAND_EDGES = [lx.LOG_EDGE0[0], lx.LOG_EDGE0[1], F(-5.0)]


def band_cloud(n, log_edge0, seed):
    """want: the boundary set (every bound and its neighbours, far values, NaN, the exact class) in shuffled order, tiled
    to n; xyz: normal coordinates with signed zeros, denormals and +-3e38 strewn in, y never positive, z never negative."""
    rng = np.random.default_rng(seed)
    vals = lx.boundary_values(log_edge0)
    want = vals[rng.permutation(len(vals))][np.arange(n) % len(vals)] if n > 1 else vals[1:2].copy()
    if n > 1:
        want = want[rng.permutation(n)]
    xyz = rng.normal(size=(n, 3)).astype(F)
    special = np.array([-0.0, 0.0, 1e-45, -1e-45, 1e-40, -1e-40, 3e38, -3e38, -1.5, 2.5], dtype=F)
    hit = rng.random((n, 3)) < 0.4
    xyz[hit] = special[rng.integers(0, len(special), size=int(hit.sum()))]
    xyz[:, 1] = -np.abs(xyz[:, 1])
    xyz[:, 2] = np.abs(xyz[:, 2])
    zero = rng.random((n, 2)) < 0.3                 # both signs of zero as the extreme of an axis
    xyz[:, 1][zero[:, 0]] = rng.choice(np.array([-0.0, 0.0], dtype=F), size=int(zero[:, 0].sum()))
    xyz[:, 2][zero[:, 1]] = rng.choice(np.array([-0.0, 0.0], dtype=F), size=int(zero[:, 1].sum()))
    return want.astype(F), xyz


def ordered(x):
    """float32 -> the integers whose order is the order of the floats, -0.0 below +0.0 (what the box is reduced in)."""
    i = np.asarray(x, dtype=F).view(np.int32).astype(np.int64)
    return np.where(i >= 0, i, i ^ 0x7FFFFFFF)


def box_of(xyz, member):
    """Bit patterns of (min xyz, max xyz) over the members; the untouched (+inf, -inf) box without one."""
    if not member.any():
        return lx.bits(np.array([np.inf] * 3 + [-np.inf] * 3, dtype=F))
    p = xyz[member]
    o = ordered(p)
    return np.concatenate([lx.bits(p[o.argmin(axis=0), np.arange(3)]), lx.bits(p[o.argmax(axis=0), np.arange(3)])])


@pytest.mark.parametrize("n", BAND_N)
def test_bands(handle, n):
    rng = np.random.default_rng(n)
    seen_zero = set()
    for which, log_edge0 in enumerate(BAND_EDGES):
        want, xyz = band_cloud(n, log_edge0, 1000 + n + which)
        ranges = [(0, n), (0, 0)] if n == 1 else [(0, n), (n // 3 + 1, n - n // 5 - 3)]          # whole; inner, not aligned to 256
        assert n == 1 or (ranges[1][0] % 256 and ranges[1][1] % 256)
        for begin, end in ranges:
            w, p = want[begin:end], xyz[begin:end]
            ref_hist, ref_exact = lx.histogram(w, log_edge0)
            strip = int(((w >= lx.WINDOW_TOP) & (w < lx.EXACT_FROM)).sum())
            # every window on the shape around a block at one edge, a sample of windows elsewhere
            every = which == 0 and n == 257
            starts = range(157) if every else sorted({0, 1, 78, 155, 156, *rng.integers(0, 157, size=12).tolist()})
            for b in starts:
                hist, exact, used, box, count = handle.selftest_levels_bands(want, xyz, begin, end, log_edge0, window=b)
                lo, hi = lx.window(log_edge0, b)
                assert np.array_equal(lx.bits(used), lx.bits(np.array([lo, hi]))), (n, b)
                assert np.array_equal(hist, ref_hist) and exact == ref_exact, (n, begin, end, b)
                member = lx.members(w, lo, hi)
                assert count == int(member.sum()), (n, begin, end, b, count)
                assert np.array_equal(lx.bits(box), box_of(p, member)), (n, begin, end, b, box, lx.from_bits(box_of(p, member)))
                assert count == int(hist[b:b + 4].sum()) - (strip if b == 156 else 0), (n, begin, end, b)
                if member.any():
                    seen_zero |= {int(u) for u in lx.bits(box) if u in (0, 0x80000000)}
        # bounds of the caller's own: a closed top, an empty interval, everything
        for lo, hi in ((F(-np.inf), F(np.inf)), (lx.bounds(log_edge0)[80], lx.bounds(log_edge0)[80]), (F(-np.inf), lx.K_WANT_EXACT)):
            hist, exact, used, box, count = handle.selftest_levels_bands(want, xyz, 0, n, log_edge0, lo=lo, hi=hi)
            member = lx.members(want, lo, hi)
            assert (float(used[0]), float(used[1])) == (float(lo), float(hi))
            assert count == int(member.sum()) and np.array_equal(lx.bits(box), box_of(xyz, member)), (n, lo, hi)
    if n >= 255:
        assert seen_zero == {0, 0x80000000}          # -0.0 came back as a minimum and +0.0 as a maximum somewhere


def test_a_window_without_members_leaves_the_box_untouched(handle):
    want = np.array([np.nan, lx.K_WANT_EXACT, F(-5.0) - F(17.4), np.nan], dtype=F)
    xyz = np.arange(12, dtype=F).reshape(4, 3)
    hist, exact, _, box, count = handle.selftest_levels_bands(want, xyz, 0, 4, F(-5.0), window=100)
    assert count == 0 and exact == 1 and hist.sum() == 1 and hist[10] == 1
    assert np.array_equal(box, np.array([np.inf] * 3 + [-np.inf] * 3, dtype=F))
    hist, exact, _, box, count = handle.selftest_levels_bands(want, xyz, 0, 4, F(-5.0), window=8)
    assert count == 1 and np.array_equal(box, np.array([6, 7, 8, 6, 7, 8], dtype=F))


# -------------------------------------------------------------------------------------------------------------- classify
def classify_case(n_rows, log_edge, target, seed):
    """n_rows rows of one pass in a shuffled public order: (row_done, redo_m, pub, want0, bracket0, rows by row)."""
    rng = np.random.default_rng(seed)
    rows, generated, dropped = lx.classify_rows(log_edge, target)
    assert dropped < 0.01 * generated
    m = len(rows["why"])
    if n_rows >= m:
        pick = np.arange(n_rows) % m                 # the whole product, tiled
    else:
        took_log = lx.classify(rows["why"], rows["pop"], log_edge, target, rows["bx"], rows["by"])[3]
        pick = np.concatenate([np.flatnonzero(took_log)[:max(n_rows // 4, 1)], rng.choice(m, size=n_rows, replace=False)])[:n_rows]
    r = {k: v[pick] for k, v in rows.items()}
    n_pub = n_rows + 7                               # seven public indices belong to no row
    pub = rng.permutation(n_pub)[:n_rows].astype(np.int32)
    done = np.where(rng.random(n_rows) < 0.3, rng.choice(np.array([1, 7, -1]), size=n_rows), 0).astype(np.int32)
    if n_rows == 1:
        done[:] = 0
    redo = (r["why"].astype(np.uint32) << np.uint32(29)) | r["pop"].astype(np.uint32)
    want0 = rng.normal(size=n_pub).astype(F)         # whatever the last pass left there
    bracket0 = rng.normal(size=(n_pub, 2)).astype(F)
    bracket0[pub, 0], bracket0[pub, 1] = r["bx"], r["by"]
    return done, redo, pub, want0, bracket0, r


@pytest.mark.parametrize("n_rows", [1, 256, 262144 + 300])        # the last: more than 1024 blocks x 256 threads, the stride runs
def test_classify(handle, n_rows):
    passes = [(F(0.0), lx.CLASSIFY_TARGETS[0]), (F(-3.3125), lx.CLASSIFY_TARGETS[1]), (lx.LOG_EDGE0[0], lx.CLASSIFY_TARGETS[2])]
    n_log = off = 0
    for i, (log_edge, target) in enumerate(passes):
        done, redo, pub, want0, bracket0, r = classify_case(n_rows, log_edge, target, 50 + i)
        want, bracket = handle.selftest_levels_classify(done, redo, pub, log_edge, target, want0, bracket0)
        # rows that were answered, and public indices of no row, keep their bytes
        keep = np.ones(len(want0), bool)
        keep[pub[done == 0]] = False
        assert np.array_equal(lx.bits(want[keep]), lx.bits(want0[keep])) and np.array_equal(lx.bits(bracket[keep]), lx.bits(bracket0[keep]))
        live = done == 0
        ref = [lx.classify(r["why"][live], r["pop"][live], log_edge, target, r["bx"][live], r["by"][live], s) for s in (0, -1, 1)]
        w0, x0, y0, took_log = ref[0]
        got_w, got_b = want[pub[live]], bracket[pub[live]]
        assert np.array_equal(lx.bits(got_b[:, 0]), lx.bits(x0)) and np.array_equal(lx.bits(got_b[:, 1]), lx.bits(y0))
        assert np.array_equal(lx.bits(got_w[~took_log]), lx.bits(w0[~took_log]))
        allowed = np.stack([lx.bits(x[0]) for x in ref])
        inside = (lx.bits(got_w)[None, :] == allowed).any(axis=0)
        assert inside[took_log].all(), (n_rows, i, got_w[took_log & ~inside][:5], w0[took_log & ~inside][:5])
        n_log += int(took_log.sum())
        off += int((lx.bits(got_w) != allowed[0])[took_log].sum())
        assert n_rows < 256 or (took_log.sum() >= 10 and (~took_log).sum() >= 10 and (done != 0).sum() >= 10)
    print(f"k_classify, {n_rows} rows x {len(passes)} passes: {n_log} rows through log2f, {off} not the nearest float32 of the float64 logarithm")


# ----------------------------------------------------------------------------------------------------------------- merge
@pytest.mark.parametrize("k", [1, 30, 127])
@pytest.mark.parametrize("counts", ["both", "pass_null", "none", "public_null"])
def test_merge(handle, k, counts):
    rng = np.random.default_rng(k)
    pitch = (k + 3) & ~3
    assert pitch in (4, 32, 128) and pitch > k
    n_pos, n_rows, q_begin, n_out, n_want = 500, 301, 11, 320, 503
    assert (n_rows * k) % 256 and n_rows * k > 256
    pub = rng.permutation(n_pos).astype(np.int32)                        # public index of every position of the cell order
    owned_public = q_begin + rng.permutation(n_out)[:n_rows]             # the queries of the pass, in the order of its rows
    where = np.empty(n_pos, np.int64)
    where[pub] = np.arange(n_pos)
    owned_pos = where[owned_public].astype(np.int32)
    nbr_pos = rng.integers(0, n_pos, size=(n_rows, pitch)).astype(np.int32)
    nbr_pos[rng.random((n_rows, pitch)) < 0.2] = -1                      # rows cut short by an eps bound
    nbr_pos[rng.random((n_rows, pitch)) < 0.05] = np.iinfo(np.int32).min
    nbr_pos[:, k:] = 0x7FFFFFF0                                          # padding columns of the pass table: never read
    nbr_dist = rng.random((n_rows, pitch)).astype(F)
    nbr_dist[rng.random((n_rows, pitch)) < 0.1] = np.inf
    nbr_cnt = rng.integers(0, k + 1, size=n_rows).astype(np.int32) if counts in ("both", "public_null") else None
    row_done = np.where(rng.random(n_rows) < 0.6, rng.choice(np.array([1, 3, -2]), size=n_rows), 0).astype(np.int32)
    pub_pos = np.full((n_out, pitch), SENTINEL, np.int32)
    pub_dist = np.full((n_out, pitch), SENTINEL, np.uint32).view(F)
    pub_cnt = np.full(n_out, SENTINEL, np.int32) if counts in ("both", "pass_null") else None
    want = rng.normal(size=n_want).astype(F)
    got = handle.selftest_levels_merge(pub, owned_pos, q_begin, nbr_pos, nbr_dist, nbr_cnt, row_done, k, pub_pos, pub_dist, pub_cnt, want)
    ref = lx.merge_rows(pub, owned_pos, q_begin, nbr_pos, nbr_dist, nbr_cnt, row_done, k, pub_pos, pub_dist, pub_cnt, want)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(lx.bits(got[1]), lx.bits(ref[1]))
    assert (got[2] is None and ref[2] is None) or np.array_equal(got[2], ref[2])
    assert np.array_equal(lx.bits(got[3]), lx.bits(ref[3]))
    # what the comparison above holds, spelled out on the result
    done_rows = owned_public[row_done != 0] - q_begin
    idle = np.setdiff1d(np.arange(n_out), done_rows)
    assert len(done_rows) > 100 and len(idle) > 100
    assert (got[0][:, k:] == SENTINEL).all() and (got[0][idle] == SENTINEL).all() and (lx.bits(got[1][idle]) == SENTINEL).all()
    assert (got[0][done_rows, :k] >= -1).all() and (got[0][done_rows, :k] == -1).any() and (got[0][done_rows, :k] < n_pos).all()
    assert (lx.bits(got[3][owned_public[row_done != 0]]) == 0x7FC00000).all()
    untouched = np.setdiff1d(np.arange(n_want), owned_public[row_done != 0])
    assert np.array_equal(lx.bits(got[3][untouched]), lx.bits(want[untouched]))
    if pub_cnt is not None:
        assert (got[2][idle] == SENTINEL).all() and np.array_equal(got[2][done_rows], (nbr_cnt[row_done != 0] if nbr_cnt is not None else np.full(len(done_rows), k)))


def test_entries_refuse_what_would_leave_the_arrays(handle):
    one = np.zeros(1, np.int32)
    with pytest.raises(ValueError):
        handle.selftest_levels_classify(one, one.astype(np.uint32), np.array([2], np.int32), 0.0, 341.0, np.zeros(2, F), np.zeros((2, 2), F))
    with pytest.raises(ValueError):
        handle.selftest_levels_classify(np.zeros(2, np.int32), np.zeros(2, np.uint32), np.array([1, 1], np.int32), 0.0, 341.0, np.zeros(2, F), np.zeros((2, 2), F))
    with pytest.raises(ValueError):
        handle.selftest_levels_bands(np.zeros(4, F), np.zeros((4, 3), F), 2, 5, 0.0)
    with pytest.raises(ValueError):
        handle.selftest_levels_bands(np.zeros(4, F), np.zeros((4, 3), F), 0, 4, 0.0, window=157)
    tab, dist = np.zeros((1, 4), np.int32), np.zeros((1, 4), F)
    for pub, owned, q_begin, pos in (([0, 1], [2], 0, 0), ([0, 5], [1], 0, 0), ([0, 1], [0], 1, 0), ([0, 1], [1], 0, 2)):
        with pytest.raises(ValueError):
            handle.selftest_levels_merge(np.array(pub, np.int32), np.array(owned, np.int32), q_begin, tab + pos, dist, None, np.ones(1, np.int32), 1,
                                         np.zeros((2, 4), np.int32), np.zeros((2, 4), F), None, np.zeros(2, F))


# ------------------------------------------------------------------------------------------------------------ end to end
def test_svd_rows_are_summed_over_the_passes(gpu):
    """A torus under the eps bound of test_eps_bound_that_leaves_rows_shorter_than_the_quadric (rows of 0 to 24 neighbours)
    beside a clump far denser than the bound and a sparse box: the first pass, its cells held at eps, overflows on the
    clump, so the chain runs further passes -- and every pass hands its own under-determined and ill-conditioned rows to
    k_fit_svd.  Their sum, the table and the curvatures equal those of a fresh handle's exhaustive sweep."""
    capi, k = gpu["capi"], 30
    rng = np.random.default_rng(78)
    torus = gpu["shapes"].torus_random(2000, seed=78)
    p = torus.astype(np.float64)
    d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))
    eps = float(np.median(np.sort(d, axis=1)[:, 9]))          # about nine points inside the bound, self included
    clump = rng.normal(scale=0.02 * eps, size=(3000, 3)) + np.array([4.0, 0.0, 0.0])
    sparse = rng.uniform(-1.0, 1.0, size=(1000, 3)) * 12.0 * eps + np.array([0.0, 6.0, 0.0])
    pts = np.concatenate([torus, clump.astype(torus.dtype), sparse.astype(torus.dtype)])
    pts = pts[rng.permutation(len(pts))]
    _, _, cnt = oracle.knn(pts, k, eps=eps)
    short = int(((cnt >= 2) & (cnt < 6)).sum())
    assert short >= 20 and (cnt == k).sum() >= 3000 and (cnt < 2).any()
    out = {}
    for algo in ("GRID_LEVELS", "BRUTE"):
        h = capi.Handle(0)
        try:
            h.set_points(pts)
            h.curvature(k, eps, getattr(capi, "KNN_" + algo))
            t = h.timings()
            idx, _, got_cnt = h.get_neighbors(0, len(pts), want_count=True)
            _, K, H, _ = h.get_fit(0, len(pts), coefs=False, H2=False)
            out[algo] = (t, idx, got_cnt, K, H)
        finally:
            h.close()
    t, idx, got_cnt, K, H = out["GRID_LEVELS"]
    bt, bidx, bcnt, bK, bH = out["BRUTE"]
    print(f"chain: {t['levels']} passes, {t['fit_svd_rows']} rows to k_fit_svd (exhaustive sweep: {bt['fit_svd_rows']}), {short} under-determined")
    assert t["algo"] == capi.KNN_GRID_LEVELS and t["levels"] >= 2
    assert np.array_equal(bcnt, cnt) and np.array_equal(got_cnt, bcnt)
    assert np.array_equal(idx, bidx)
    assert bt["fit_svd_rows"] >= short and t["fit_svd_rows"] == bt["fit_svd_rows"]
    assert np.array_equal(K, bK, equal_nan=True) and np.array_equal(H, bH, equal_nan=True)

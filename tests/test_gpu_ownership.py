"""Ownership by slab and by index range on the device against its restatement (tests/ownership_exact.py).

K, H and the rows of a sharded handle equal the unsharded run whatever it kept: a lopsided cut, a margin of 40 edges, a
retry on every call only cost time.  Here the decisions themselves are asserted, per case on a fresh handle with the
statistics on, and for every way a cloud reaches a handle:

  host         pct_set_points_f32
  device_copy  pct_set_points_device_f32
  use_base     pct_use_points_device_f32 on an allocation's first byte
  use_0 .. 12  pct_use_points_device_f32 at 0, 4, 8 and 12 bytes into a larger buffer with 64 bytes of NaN either side: at 4,
               8 and 12 the view is not 16-byte aligned and slab_split / pack_near_owned take k_cloud_box<false>,
               k_slab_hist<false> and k_cull_pack<*, false>, the scalar path of load_four_points; a read past either end
               would show as PCT_ERR_NONFINITE or a wrong count

Slabs (parts 1, 2, 3, 7, 64, every part on one handle): pct_slab_counts and the sorted public indices of pct_slab_records
EQUAL the restated counts and member sets, every index once over the parts; K and H of every record are the bits of the
whole-cloud pct_curvature of the same handle; limit_retries EQUALS the restated verdict (no call of these cases is
undecided: tests/test_ownership_exact.py) and grid_points the restated kept count, n after a retry.  Index ranges
(pct_knn and pct_curvature, PCT_KNN_GRID): grid_points, limit_retries, the rows; the restart rule at k and k + 1 kept
points; a float64 cloud; the box of the previous cloud reused, dropped by a retry and measured again; a row exactly as
far from its k-th kept neighbour as from the face, which the slack of 1e-6 sends to the retry.

Measured on the MI355X: the 30 tests of this file 12.7 s together, the restatement's share included; the longest are the
stream of four clouds (2.0 s per call kind, three ways), egg_24577_k30 (1.6 s: 7 ways x 77 slab passes) and
zcut_12290_k200 (1.1 s); every other test takes 0.01 - 0.7 s.  Device and restatement agreed in every figure of every case
on the first run; nothing in the library changed.

Mutations of the library, one at a time, each a value or a condition (the tests of this file that fail; of the older
slab and shard tests of tests/test_gpu_parity.py only the last mutation fails any):
  want = ceil(p n / parts) in the cut       test_slabs_are_the_restated_ones, 9 of its 11 cases
  axis choice >= for >                      test_slabs_are_the_restated_ones[lattice_4096_k30]
  slab_bin in double                        test_slabs_are_the_restated_ones[egg_4097_k30_on_cut]
  slab margin 3 a0                          test_slabs_are_the_restated_ones, every case
  range margin 3 a0                         test_ranges_keep_the_restated_points[quarter-*, begin_not_by_4-*], the stream of four
                                            clouds, test_a_row_as_far_from_its_neighbour_as_from_the_face_retries
  in_box with < on the upper faces          test_slabs_are_the_restated_ones[egg_8193_k30_on_face]
  limit_r2 without (1 - 1e-6)               test_a_row_as_far_from_its_neighbour_as_from_the_face_retries
  restart below k, not k + 1                test_fewer_than_k_plus_one_kept_points_take_every_point[k_kept-knn] (the curvature
                                            variant was not run on this build: its fit would read rows with missing entries)
  scalar load_four_points, j < 3 have - 1   22 tests here; older: test_random_cross_check_of_slab_ownership and the two
                                            *_driver_on_four_handles_with_a_loopback_exchange
  box kept valid after a retry              test_the_box_of_the_previous_cloud_is_reused_and_measured_again_after_a_retry[*]
"""
import numpy as np
import pytest

import ownership_exact as oe

pytestmark = pytest.mark.gpu

F32 = np.float32
SLACK = 64
WAYS = ("host", "device_copy", "use_base", "use_0", "use_4", "use_8", "use_12")


class Supplied:
    """a fresh handle with the statistics on and the cloud on it, one of WAYS; frees what it allocated"""

    def __init__(self, capi, pts, way, factor=0.0):
        self.capi, self.way, self.bufs = capi, way, []
        self.h = capi.Handle(0)
        self.h.set_stats(True)
        if factor:
            self.h.set_grid_param(factor)
        self.load(pts)

    def load(self, pts):
        h, way, n = self.h, self.way, len(pts)
        if way == "host" or pts.dtype == np.float64:
            h.set_points(pts)
            return
        if way in ("device_copy", "use_base"):
            buf = h.device_alloc(n * 12)
            self.bufs.append(buf)
            h.device_upload(buf, pts)
            (h.set_points_device if way == "device_copy" else h.use_points_device)(buf, n)
            return
        off = int(way[4:])
        host = np.full((2 * SLACK + 16) // 4 + 3 * n, np.nan, F32)
        first = (SLACK + off) // 4
        host[first:first + 3 * n] = pts.ravel()
        buf = h.device_alloc(host.nbytes)
        self.bufs.append(buf)
        h.device_upload(buf, host)
        assert buf % 16 == 0 and ((buf + SLACK + off) % 16 != 0) == (off != 0)
        h.use_points_device(buf + SLACK + off, n)

    def __enter__(self):
        return self.h

    def __exit__(self, *exc):
        self.h.synchronize()
        self.h.close()                 # (the handle reads a used buffer until it is destroyed)
        h = self.capi.Handle(0)
        for b in self.bufs:
            h.device_free(b)
        h.close()


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _slab_passes(h, c, k, eps, parts, split, calls, K0, H0, rec, tag):
    n = c.n
    seen = np.zeros(n, np.int64)
    for part in range(parts):
        where = f"{tag} part {part} of {parts}"
        h.set_query_slab(part, parts)
        h.curvature(k, eps)
        t = h.timings()
        assert h.slab_counts(parts) == [int(x) for x in split.counts], where
        rows = h.slab_records(rec, n)
        r = np.empty((rows, 3), F32)
        if rows:
            h.device_download(rec, r)
        pub = r[:, 0].copy().view(np.int32).astype(np.int64)
        assert np.array_equal(np.sort(pub), split.members(part)), where
        assert np.array_equal(_bits(r[:, 1]), _bits(K0[pub])) and np.array_equal(_bits(r[:, 2]), _bits(H0[pub])), where
        e = calls[part]
        print(f"{where}: rows {rows} grid_points {t['grid_points']} ({e['grid_points']}) limit_retries {t['limit_retries']} ({e['limit_retries']})")
        assert (t["limit_retries"], t["grid_points"]) == (e["limit_retries"], e["grid_points"]), where
        seen[pub] += 1
    assert np.all(seen == 1), tag


@pytest.mark.parametrize("name", list(oe.SLAB_CASES))
def test_slabs_are_the_restated_ones(gpu, name):
    capi = gpu["capi"]
    kind, n, seed, k, eps, factor = oe.SLAB_CASES[name]
    c, expect = oe.slab_cloud(name), oe.slab_expectation(name)
    for way in WAYS:
        with Supplied(capi, c.pts, way, factor) as h:
            h.curvature(k, eps)
            assert h.timings()["grid_points"] == n
            _, K0, H0, _ = h.get_fit(0, n, coefs=False, H2=False)
            rec = h.device_alloc(n * 12)
            try:
                for parts in oe.PARTS:
                    split, calls = expect[parts]
                    _slab_passes(h, c, k, eps, parts, split, calls, K0, H0, rec, f"{name} {way}")
            finally:
                h.device_free(rec)


def test_slab_margin_on_both_sides_of_the_verdict(gpu, monkeypatch):
    """PCT_SLAB_MARGIN at two values that the restatement puts on opposite sides: every slab retries at the thin one and
    holds every point, none retries at the wide one and each holds the restated count."""
    capi = gpu["capi"]
    kind, n, seed, k, parts = oe.MARGIN_CASE
    for margin in oe.MARGINS:
        split, calls = oe.margin_expectation(margin)
        c = oe.margin_cloud()
        for way in WAYS:
            with Supplied(capi, c.pts, way) as h:
                h.curvature(k)
                _, K0, H0, _ = h.get_fit(0, n, coefs=False, H2=False)
                rec = h.device_alloc(n * 12)
                monkeypatch.setenv("PCT_SLAB_MARGIN", repr(margin))
                try:
                    _slab_passes(h, c, k, 0.0, parts, split, calls, K0, H0, rec, f"margin {margin} {way}")
                finally:
                    monkeypatch.delenv("PCT_SLAB_MARGIN")
                    h.device_free(rec)


# ---- index ranges -----------------------------------------------------------------------------------------------------------
def _whole(h, n, k, call, capi):
    if call == "knn":
        h.knn(k, algo=capi.KNN_GRID)
        return h.get_neighbors(0, n)[:2]
    h.curvature(k, algo=capi.KNN_GRID)
    return h.get_fit(0, n)[:3]


def _owned(h, b, e, k, call, capi):
    """the call on rows [b, e): (timings, rows)"""
    h.set_query_range(b, e)
    if call == "knn":
        h.knn(k, algo=capi.KNN_GRID)
        return h.timings(), h.get_neighbors(b, e)[:2]
    h.curvature(k, algo=capi.KNN_GRID)
    return h.timings(), h.get_fit(b, e)[:3]


def _same_rows(got, whole, b, e, where):
    for g, w in zip(got, whole):
        assert np.array_equal(g.view(np.uint32) if g.dtype == F32 else g, w[b:e].view(np.uint32) if w.dtype == F32 else w[b:e]), where


@pytest.mark.parametrize("call", ["knn", "curvature"])
@pytest.mark.parametrize("name", list(oe.RANGES))
def test_ranges_keep_the_restated_points(gpu, name, call):
    capi = gpu["capi"]
    c, (b, e), expect = oe.range_cloud(), oe.RANGES[name], oe.range_expectation(name)
    for way in WAYS:
        with Supplied(capi, c.pts, way) as h:
            whole = _whole(h, c.n, oe.RANGE_K, call, capi)
            t, got = _owned(h, b, e, oe.RANGE_K, call, capi)
            where = f"{name} {call} {way}"
            print(f"{where}: grid_points {t['grid_points']} ({expect['grid_points']}) limit_retries {t['limit_retries']} ({expect['limit_retries']})")
            assert (t["limit_retries"], t["grid_points"]) == (expect["limit_retries"], expect["grid_points"]), where
            _same_rows(got, whole, b, e, where)


@pytest.mark.parametrize("call", ["knn", "curvature"])
@pytest.mark.parametrize("in_box", [0, 10, 11], ids=["nobody_in_the_box", "k_kept", "k_plus_one_kept"])
def test_fewer_than_k_plus_one_kept_points_take_every_point(gpu, in_box, call):
    """20 owned rows, k = 30: with nobody else in the box, and with exactly k points kept, the build starts over with every
    point and counts no retry; with k + 1 kept it goes on with them."""
    capi = gpu["capi"]
    pts = oe.restart_cloud(in_box)
    m = oe.Handle()
    m.set_cloud(pts)
    m.set_range(0, 20)
    expect = m.ranged(30)
    assert expect["kept"] == 20 + in_box and expect["verdict"] == "no retry"
    for way in ("host", "use_4"):
        with Supplied(capi, pts, way) as h:
            whole = _whole(h, len(pts), 30, call, capi)
            t, got = _owned(h, 0, 20, 30, call, capi)
            assert (t["limit_retries"], t["grid_points"]) == (0, expect["grid_points"]), (way, t)
            _same_rows(got, whole, 0, 20, way)


def test_a_float64_cloud_is_never_culled(gpu):
    capi = gpu["capi"]
    c = oe.range_cloud()
    b, e = oe.RANGES["quarter"]
    with Supplied(capi, c.pts.astype(np.float64), "host") as h:
        for call in ("knn", "curvature"):
            t, _ = _owned(h, b, e, oe.RANGE_K, call, capi)
            assert (t["limit_retries"], t["grid_points"]) == (0, c.n)


@pytest.mark.parametrize("call", ["knn", "curvature"])
def test_the_box_of_the_previous_cloud_is_reused_and_measured_again_after_a_retry(gpu, call):
    capi = gpu["capi"]
    clouds = oe.stream_clouds()
    n, k = len(clouds[0]), 30
    b, e = n // 4, n // 2
    for way in ("host", "use_4", "use_12"):
        m = oe.Handle()
        sup = Supplied(capi, clouds[0], way)
        with sup as h:
            for i, pts in enumerate(clouds):
                if i:
                    sup.load(pts)                      # (the next cloud of the stream, in a buffer of its own)
                m.set_cloud(pts)
                m.set_range(b, e)
                expect = m.ranged(k)
                whole = _whole(h, n, k, call, capi)
                t, got = _owned(h, b, e, k, call, capi)
                print(f"{way} cloud {i}: grid_points {t['grid_points']} ({expect['grid_points']}, first attempt kept {expect['kept']}) "
                      f"limit_retries {t['limit_retries']} ({expect['verdict']})")
                assert expect["verdict"] != "undecided"
                assert (t["limit_retries"], t["grid_points"]) == (expect["limit_retries"], expect["grid_points"]), (way, i)
                _same_rows(got, whole, b, e, (way, i))


def test_a_row_as_far_from_its_neighbour_as_from_the_face_retries(gpu):
    """The device compares min(d_k, eps)^2 with ((1 - 1e-6) d_face)^2: a row whose k-th kept neighbour is EXACTLY as far as
    the nearest face (it sits on the face, which is inclusive) must not pass for proven.  The restatement calls such a
    row undecided (tests/test_ownership_exact.py); the definition, and the device, say retry -- under every rounding of
    the face through cell units, which is what the slack is there for.  PCT_KNN_GRID_EXACT: the wave-per-query sweep
    decides every row in double."""
    capi = gpu["capi"]
    a = oe.stream_clouds()[0]
    n, k = len(a), 8
    b, e = n // 4, n // 2
    m = oe.Handle()
    m.set_cloud(a)
    m.set_range(b, e)
    first = m.ranged(k)
    h = capi.Handle(0)
    h.set_stats(True)
    for d0 in oe.TIE_DISTANCES:
        h.set_points(a)
        h.set_query_range(b, e)
        h.knn(k, algo=capi.KNN_GRID_EXACT)                     # measures the box (again, after the retry below)
        t = h.timings()
        assert (t["limit_retries"], t["grid_points"]) == (0, first["grid_points"])
        pts, d = oe.tie_cloud(a, b, m.box, k, d0)
        h.set_points(pts)
        h.set_query_range(b, e)
        h.knn(k, algo=capi.KNN_GRID_EXACT)
        t = h.timings()
        assert (t["limit_retries"], t["grid_points"]) == (1, n), (d0, d, t)
    h.close()

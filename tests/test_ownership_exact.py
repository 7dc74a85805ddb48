"""tests/ownership_exact.py against its own definitions: the cut against brute force, the edges of the bin, the retry
verdict against what it means, the handle's box against the rules of reuse -- and the condition under which
tests/test_gpu_ownership.py may assert the device's limit_retries: no call of its cases is undecided."""
import numpy as np
import pytest

import ownership_exact as oe

F32 = np.float32


# ---- the cut ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", [("egg", 4099), ("lattice", 4096), ("flat", 8191), ("two", 8192), ("zcut", 5000)])
@pytest.mark.parametrize("parts", oe.PARTS)
def test_the_cut_against_brute_force(kind, n, parts):
    pts = oe.make_cloud(kind, n, 2)
    s = oe.Split(pts, parts)
    below = np.array([np.count_nonzero(s.bins < b) for b in range(oe.BINS + 1)])
    seen = np.zeros(n, int)
    for p in range(parts):
        want = p * n // parts
        first = next(b for b in range(oe.BINS + 1) if below[b] >= want)
        assert s.cut[p] == min(first, oe.BINS)
        m = s.members(p)
        seen[m] += 1
        assert len(m) == s.counts[p]
        # cum[cut[p]] lies in [want_p, want_p + largest bin): populations differ from n / parts by a bin's worth
        assert abs(s.counts[p] - n / parts) <= s.hist.max() + 1
    assert s.cut[parts] == oe.BINS and np.all(seen == 1)


def test_the_first_axis_wins_a_tie_and_the_longest_wins_otherwise():
    assert oe.cut_axis(F32([0, 0, 0]), F32([2, 2, 2])) == 0
    assert oe.cut_axis(F32([0, 0, 0]), F32([1, 2, 2])) == 1
    assert oe.cut_axis(F32([0, 0, 0]), F32([1, 2, 3])) == 2
    # compared as float32 differences: 1 + 2^-24 - 0 ties with 1 in float32 only because the box is float32 already
    lat = oe.make_cloud("lattice", 4096)
    assert oe.Split(lat, 2).axis == 0 and np.ptp(lat[:, 0]) == np.ptp(lat[:, 1])


def test_edges_of_the_bin():
    pts = oe.make_cloud("egg", 5000, 1)
    s = oe.Split(pts, 3)
    assert s.bins[np.argmax(pts[:, s.axis])] == oe.BINS - 1 and s.bins[np.argmin(pts[:, s.axis])] == 0
    # no extent: everything in bin 0, everything in part 0
    same = np.ones((4096, 3), F32)
    s = oe.Split(same, 7)
    assert s.inv == 0 and list(s.counts) == [4096] + [0] * 6 and list(s.cut) == [0] + [1] * 6 + [oe.BINS]
    lo, hi = oe.slab_box(s, 0, 1.0)
    assert np.all(np.isinf(lo)) and np.all(np.isinf(hi))                 # no scale, no faces
    # an extent so small that 4096 / ext is not a float32: the same
    tiny = np.zeros((4096, 3), F32)
    tiny[1::2, 0] = F32(1e-42)
    with np.errstate(over="ignore"):
        assert np.ptp(tiny[:, 0]) > 0 and not np.isfinite(F32(4096) / np.ptp(tiny[:, 0]))
    s = oe.Split(tiny, 2)
    assert s.inv == 0 and list(s.counts) == [4096, 0]
    # a lattice: every plane across the cut axis falls whole into one bin
    lat = oe.make_cloud("lattice", 4096)
    s = oe.Split(lat, 7)
    for x in np.unique(lat[:, 0]):
        assert len(np.unique(s.bins[lat[:, 0] == x])) == 1
    assert np.all(s.hist[s.hist > 0] % 64 == 0) and np.all(s.counts % 64 == 0)


def test_a_coordinate_on_a_bin_boundary_takes_the_float32_bin():
    pts = oe.make_cloud("egg", 4097, 12)
    s = oe.Split(pts, 2)
    found = 0
    for b in range(1, oe.BINS, 97):
        x = oe.rounds_across(s.x0, s.inv, b)
        found += len(x)
        assert np.all(oe.bins_of(x, s.x0, s.inv) == b) and np.all(oe.bins_in_double(x, s.x0, s.inv) == b - 1)
    assert found > 0
    planted, i = oe.plant_on_cut(pts)
    t = oe.Split(planted, 2)
    assert t.cut[1] == s.cut[1] and t.axis == s.axis and t.x0 == s.x0 and t.inv == s.inv
    assert t.bins[i] == t.cut[1] and t.owned(1)[i]
    assert oe.bins_in_double(planted[i, t.axis], t.x0, t.inv) == t.cut[1] - 1          # in double it would belong to part 0


def test_a_point_on_the_upper_face_is_kept():
    kind, n, seed, k, eps, factor = oe.SLAB_CASES["egg_8193_k30_on_face"]
    c = oe.slab_cloud("egg_8193_k30_on_face")
    s = oe.Split(c.pts, 2)
    lo, hi = oe.slab_box(s, 0, oe.first_edge(c.lo, c.hi, c.n, oe.target_of(k)))
    on = np.flatnonzero(c.pts[:, s.axis] == hi[s.axis])
    assert len(on) == 1 and not s.owned(0)[on[0]] and oe.in_box(c.pts, lo, hi)[on[0]]


# ---- the target ------------------------------------------------------------------------------------------------------------
def test_the_table_of_occupancy_factors():
    f = oe.default_factor
    assert [f(10) * 11, f(47) * 48, f(52) * 53, f(60) * 61] == pytest.approx([27.0, 27.0, 29.5, 29.5])
    assert f(49) * 50 == pytest.approx(28.0)                                            # linear between 47 and 52
    assert f(61) == 0.52 and f(84) == 0.52 and f(100) == pytest.approx(0.45) and f(127) == pytest.approx(0.40)
    assert f(128) == 0.35 and f(200) == 0.35
    assert oe.target_of(30) == pytest.approx(27.0) and oe.target_of(30, 2.0) == 62.0


def test_the_first_guess_edge_and_its_fallbacks():
    lo = F32([0, 0, 0])
    assert oe.first_edge(lo, F32([1, 1, 1]), 3600, 10.0) == pytest.approx(np.sqrt(10.0 * 3.6 / 3600))
    assert oe.first_edge(lo, F32([2, 0, 0]), 100, 25.0) == pytest.approx(np.sqrt(25.0 * 4.0 / 100))      # a line: emax^2
    assert oe.first_edge(lo, lo, 1, 27.0) == 0.0                                                        # a point: emax


# ---- the retry verdict ---------------------------------------------------------------------------------------------------
def _naive_kth(q, pool, kth):
    d = np.sqrt(((q[:, None, :].astype(np.float64) - pool[None, :, :].astype(np.float64)) ** 2).sum(-1))
    return np.sort(d, axis=1)[:, kth]


def test_windowed_brute_force_is_brute_force():
    rng = np.random.default_rng(5)
    pool = rng.normal(size=(700, 3)).astype(F32)
    q = pool[:200]
    for kth, w in ((1, 0.05), (8, 0.3), (30, 0.5), (30, 0.0), (699, 0.2)):
        assert np.allclose(oe.kth_distance(q, pool, kth, w), _naive_kth(q, pool, kth), rtol=1e-14, atol=0)
    assert np.all(np.isinf(oe.kth_distance(q, pool[:5], 5, 1.0)))


@pytest.mark.parametrize("seed", range(12))
def test_the_verdict_against_its_meaning(seed):
    """Whenever a point left out is among a row's true k nearest, or nearer than the k-th kept neighbour within eps, the row
    says retry or undecided, never no retry; and the call's verdict through the whole-cloud shortcut is the one of the
    rows measured directly."""
    rng = np.random.default_rng(seed)
    n, k = 400, int(rng.choice([1, 4, 9]))
    pts = (rng.uniform(-1, 1, (n, 3)) * [1, 0.7, 0.1]).astype(F32)
    eps = 0.0 if seed % 3 else float(rng.uniform(0.05, 0.3))
    c = oe.Cloud(pts)
    b = int(rng.integers(0, n - 60))
    owned = np.arange(b, b + int(rng.integers(1, 60)))
    olo, ohi = oe.box_of(pts[owned])
    grow = F32(rng.uniform(0.0, 0.4))
    lo, hi = olo - grow, ohi + grow
    kept = oe.in_box(pts, lo, hi)
    kept[owned] = True
    if kept.sum() < k + 1:           # (a restart: no verdict is asked for)
        return
    d_face = oe.face_distance(pts[owned], lo, hi)
    d_k = _naive_kth(pts[owned], pts[kept], k)
    v = oe.row_verdicts(d_k, d_face, eps)
    if (~kept).any():
        d_left = _naive_kth(pts[owned], pts[~kept], 0)
        m = np.minimum(d_k, eps) if eps > 0 else d_k
        matters = d_left < m
        assert np.all(v[matters] != 0)
        true_k = _naive_kth(pts[owned], pts, k)
        assert np.all(v[true_k < d_k] != 0)
    got, undecided, retry = c.verdict(owned, kept, k, eps, lo, hi)
    assert (got, undecided, retry) == (oe.call_verdict(v), int(np.sum(v == -1)), int(np.sum(v == 1)))


def test_the_band_of_the_verdict():
    d_face = np.array([1.0, 1.0, 1.0, 1.0, 0.0, 0.0, np.inf])
    d_k = np.array([0.5, 1.0, 1.0 + 2e-5, 1.0 - 2e-5, 0.0, 1e-30, 5.0])
    assert list(oe.row_verdicts(d_k, d_face)) == [0, -1, 1, 0, 0, 1, 0]
    assert list(oe.row_verdicts(d_k, d_face, eps=0.9)) == [0, 0, 0, 0, 0, 1, 0]          # the eps ball is inside


# ---- the handle ----------------------------------------------------------------------------------------------------------------
def test_the_box_is_reused_until_a_retry_or_a_restart_drops_it():
    a, b, c, d = oe.stream_clouds()
    n = len(a)
    h = oe.Handle()
    h.set_cloud(a)
    h.set_range(n // 4, n // 2)
    first = h.ranged(30)
    assert first["limit_retries"] == 0 and first["grid_points"] == first["kept"] < n
    box = h.box
    h.set_cloud(b)                                    # a new cloud owns every row again ...
    assert h.ranged(30)["grid_points"] == n
    h.set_range(n // 4, n // 2)                       # ... and the range set again finds the box of the first cloud
    second = h.ranged(30)
    assert second["box"][0] is box[0] and second["verdict"] == "no retry" and second["grid_points"] == second["kept"]
    fresh = oe.Handle()
    fresh.set_cloud(b)
    fresh.set_range(n // 4, n // 2)
    assert fresh.ranged(30)["kept"] == first["kept"] != second["kept"]          # the stale box shows in the count
    h.set_cloud(c)
    h.set_range(n // 4, n // 2)
    third = h.ranged(30)
    assert third["box"][0] is box[0] and third["verdict"] == "retry" and third["limit_retries"] == 1
    assert third["grid_points"] == n and third["kept"] < first["kept"] and h.box_key is None
    assert h.ranged(30)["grid_points"] == n           # the handle takes every point until its ownership changes
    h.set_cloud(d)
    h.set_range(n // 4, n // 2)
    fourth = h.ranged(30)                             # measured again
    assert fourth["limit_retries"] == 0 and fourth["kept"] == fourth["grid_points"] and abs(fourth["kept"] - first["kept"]) < 20
    assert np.allclose(fourth["box"][0], box[0] + F32([1.5, 0, 0]), atol=1e-5)
    # another range: measured
    h.set_range(n // 4, n // 2 + 1)
    assert h.ranged(30)["box"][0] is not fourth["box"][0]


def test_a_row_as_far_from_its_k_th_neighbour_as_from_the_face_is_undecided_here():
    """... and a retry by the definition: min(d_k, eps) > (1 - 1e-6) d_face.  tests/test_gpu_ownership.py asserts that retry."""
    a = oe.stream_clouds()[0]
    n, k = len(a), 8
    h = oe.Handle()
    h.set_cloud(a)
    h.set_range(n // 4, n // 2)
    h.ranged(k)
    for d0 in oe.TIE_DISTANCES:
        pts, d = oe.tie_cloud(a, n // 4, h.box, k, d0)
        c = oe.Cloud(pts)
        owned = np.arange(n // 4, n // 2)
        kept = oe.in_box(pts, *h.box)
        assert kept[:k].all() and kept.sum() < n
        kept[owned] = True
        d_face = oe.face_distance(pts[owned], *h.box)
        d_k = oe.kth_distance(pts[owned], pts[kept], k, np.inf)
        v = oe.row_verdicts(d_k, d_face)
        assert v[0] == -1 and abs(d_k[0] - d_face[0]) <= 1e-12 * d and d_face[0] == d and not v[1:].any()
        assert c.verdict(owned, kept, k, 0.0, *h.box) == ("undecided", 1, 0)


def test_the_restart_rule_counts_k_plus_one():
    for in_box, grid_points in ((0, 5020), (10, 5030), (11, 31)):
        h = oe.Handle()
        h.set_cloud(oe.restart_cloud(in_box))
        h.set_range(0, 20)
        e = h.ranged(30)
        assert (e["kept"], e["grid_points"], e["limit_retries"]) == (20 + in_box, grid_points, 0)
        assert h.box_key is None or in_box == 11


def test_no_culling_at_all():
    pts = oe.make_cloud("scan", 6000, 3)
    h = oe.Handle()
    h.set_cloud(oe.Cloud(pts.astype(np.float64)))
    h.set_range(100, 600)
    assert h.ranged(30)["grid_points"] == 6000                           # a float64 cloud
    h.set_cloud(pts)
    assert h.ranged(30)["grid_points"] == 6000                           # the whole cloud
    h.set_range(700, 700)
    assert h.ranged(30)["grid_points"] == 6000                           # nobody owned
    h.set_range(100, 600)
    assert h.ranged(30)["grid_points"] < 6000


# ---- the condition of the GPU tests ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(oe.SLAB_CASES))
def test_no_call_of_a_gpu_case_is_undecided(name):
    c = oe.slab_cloud(name)
    for parts, (s, calls) in oe.slab_expectation(name).items():
        rows = sum(int(s.counts[p]) for p in range(parts))
        undecided = sum(e["undecided"] for e in calls)
        print(f"{name} parts {parts}: axis {s.axis}, {undecided} of {rows} rows undecided ({100.0 * undecided / rows:.3f} %), "
              f"verdicts {sorted(set(e['verdict'] for e in calls))}, calls with clamped rows {sum(e['trimmed'] for e in calls)}")
        assert all(e["verdict"] != "undecided" for e in calls)
        assert sum(int(x) for x in s.counts) == c.n


def test_the_margin_case_lands_on_both_sides():
    thin, wide = (oe.margin_expectation(m)[1] for m in oe.MARGINS)
    print("thin:", [(e["verdict"], e["undecided"]) for e in thin], "wide:", [(e["verdict"], e["undecided"]) for e in wide])
    assert all(e["verdict"] == "retry" for e in thin) and all(e["verdict"] == "no retry" for e in wide)
    assert all(e["kept"] < oe.MARGIN_CASE[1] for e in thin + wide)


def test_no_call_of_a_range_case_is_undecided():
    for name in oe.RANGES:
        e = oe.range_expectation(name)
        print(name, e["verdict"], e["undecided"], e["kept"], e["grid_points"])
        assert e["verdict"] != "undecided"

"""Ownership by slab and by index range, stated again in NumPy from include/pct_hip.h ("Ownership by SLAB"), the comments of
csrc/pct_grid.hip (slab_split, pack_near_owned, select_source) and csrc/pct_api.hip (retry_without_cull, own_rows).

Everything that decides who owns what and what a sharded handle keeps only costs time when it is off: a lopsided cut, a
margin ten times too wide, a retry on every call return the right K and H.  This module says what the decisions ARE, so
that tests/test_gpu_ownership.py can hold the device to them, and tests/test_ownership_exact.py holds this module to its
own definitions.  float32 where the device computes in float32 (box, bins, box comparisons, the range's margin), float64
where the host computes in double (bin scale, first-guess edge, slab faces); the library is built with -ffp-contract=off.

  cloud box      float32 min / max per axis
  cut axis       the longest extent, compared as float32 differences; the first axis wins a tie
  bin scale      inv = float32(4096 / ext), ext in double; 0 when ext is 0 or the quotient is not finite in float32
  bin            float32 (x - x0) * inv, truncated, clamped to [0, 4095]
  cuts           cut[p] = the smallest b with cum[b] >= floor(p n / parts); cut[parts] = 4096; part p owns the bins
                 [cut[p], cut[p + 1])
  first guess    a0 = sqrt(target area / n), area = 1.2 (ex ey + ey ez + ex ez) or, where that is not positive, emax^2;
                 a0 = emax where a0 is not positive and finite; target = factor (k + 1), factor from pct_set_grid_param
                 or the table of pct_default_factor (csrc/pct_internal.h, PCT_FAST_R1_MAX = 61)
  slab's box     along the cut axis float32(x0 + bin_lo / inv - 4 a0) .. float32(x0 + bin_hi / inv + 4 a0) in double; the
                 outer faces of the first and the last slab and the other axes are open (PCT_SLAB_MARGIN: another multiple)
  range's box    the float32 box of the owned rows grown by float32(4 a0), a0 from the owned rows' box and count
  kept           the owned points and the others inside the box, faces inclusive, compared in float32
  restart        fewer than k + 1 kept: every point, limit_retries stays 0
  no culling     a float64 cloud, no owned point, a whole-cloud range
  reused box     an index-range handle measures the box once per (n, begin, end) and reuses it for the next cloud; a limit
                 retry and a restart drop it (cull_box_valid), nothing else does -- a new cloud and a new range keep it
  retry          a call whose kept part is smaller than the cloud repeats with every point when, for some owned row,
                 min(d_k, eps) > (1 - 1e-6) d_face: d_k the distance to its k-th neighbour among the KEPT points, d_face the
                 distance to the nearest closed face of the box (0 outside it)

The retry is restated with a band: a row whose two distances differ by less than 1e-5 d_face is "undecided" (ten times the
kernel's own slack; the device's d_face goes through cell units in double, 1e-13 relative at worst on the clouds here).  A
call is "retry" when a row says so whatever the others say, "no retry" when every row says so, else "undecided".  The device
forms the row's position in cell units as cell + fraction, and the fraction is taken from the UNclamped position, so the sum
is the position itself also for a row that the trimmed grid box clamps into a boundary cell: such rows are restated like any
other (trimmed() says whether a kept set has them).
"""
import numpy as np

BINS = 4096
MARGIN_EDGES = 4.0
FAST_R1_MAX = 61
SLACK = 1e-6
BAND = 1e-5
F32 = np.float32


# ---- the occupancy target ---------------------------------------------------------------------------------------------
def default_factor(k):
    """cell occupancy as a multiple of k + 1 (the comment above pct_default_factor): about 27 points per cell up to k = 47,
    29.5 from k = 52, linear between; two list registers (k + 1 > 61): 0.52 up to k + 1 = 85, 0.45 at 101, 0.40 at 128,
    linear between; beyond 128: 0.35"""
    m = k + 1
    if m <= FAST_R1_MAX:
        per_cell = 27.0 if k <= 47 else 29.5 if k >= 52 else 27.0 + 0.5 * (k - 47)
        return per_cell / m
    if m > 128:
        return 0.35
    if m <= 85:
        return 0.52
    if m <= 101:
        return 0.52 - 0.07 * (m - 85) / 16.0
    return 0.45 - 0.05 * (m - 101) / 27.0


def target_of(k, factor=0.0):
    return (factor if factor > 0 else default_factor(k)) * (k + 1)


# ---- box, axis, bins, cuts --------------------------------------------------------------------------------------------
def box_of(pts):
    pts = np.asarray(pts, F32)
    return pts.min(0), pts.max(0)


def cut_axis(lo, hi):
    ext = np.asarray(hi, F32) - np.asarray(lo, F32)
    axis = 0
    for a in (1, 2):
        if ext[a] > ext[axis]:
            axis = a
    return axis


def bin_scale(lo, hi, axis):
    ext = float(hi[axis]) - float(lo[axis])
    if not ext > 0:
        return F32(0)
    with np.errstate(over="ignore"):
        inv = F32(BINS / ext)
    return inv if np.isfinite(inv) else F32(0)


def bins_of(x, x0, inv):
    """float32 throughout: the difference, the product, then truncation"""
    t = (np.asarray(x, F32) - F32(x0)) * F32(inv)
    assert t.dtype == F32
    return np.clip(np.trunc(t), 0, BINS - 1).astype(np.int64)


def bins_in_double(x, x0, inv):
    """what the bin would be with the same scale and exact arithmetic (NOT what the device computes)"""
    t = (np.asarray(x, np.float64) - float(x0)) * float(inv)
    return np.clip(np.trunc(t), 0, BINS - 1).astype(np.int64)


def cuts_of(hist, n, parts):
    cum = np.concatenate([[0], np.cumsum(np.asarray(hist, np.int64))])
    cut = np.empty(parts + 1, np.int64)
    for p in range(parts):
        cut[p] = np.searchsorted(cum[:BINS], (p * n) // parts, "left")
    cut[parts] = BINS
    return cut, cum


class Split:
    """the cut of a cloud into `parts` slabs"""

    def __init__(self, pts, parts):
        pts = np.asarray(pts, F32)
        self.n, self.parts = len(pts), parts
        self.lo, self.hi = box_of(pts)
        self.axis = cut_axis(self.lo, self.hi)
        self.x0 = self.lo[self.axis]
        self.inv = bin_scale(self.lo, self.hi, self.axis)
        self.bins = bins_of(pts[:, self.axis], self.x0, self.inv)
        self.hist = np.bincount(self.bins, minlength=BINS)
        self.cut, self.cum = cuts_of(self.hist, self.n, parts)
        self.counts = self.cum[self.cut[1:]] - self.cum[self.cut[:-1]]

    def owned(self, part):
        return (self.bins >= self.cut[part]) & (self.bins < self.cut[part + 1])

    def members(self, part):
        return np.flatnonzero(self.owned(part))


# ---- what is kept -----------------------------------------------------------------------------------------------------
def first_edge(lo, hi, n, target):
    ex, ey, ez = (float(hi[a]) - float(lo[a]) for a in range(3))
    emax = max(ex, ey, ez)
    area = 1.2 * (ex * ey + ey * ez + ex * ez)
    if not area > 0:
        area = emax * emax
    a0 = np.sqrt(target * area / float(n))
    if not (a0 > 0 and np.isfinite(a0)):
        a0 = emax
    return float(a0)


def slab_box(split, part, a0, margin_edges=MARGIN_EDGES):
    lo, hi = np.full(3, -np.inf, F32), np.full(3, np.inf, F32)
    margin = margin_edges * a0
    if split.inv > 0:
        b0, b1 = int(split.cut[part]), int(split.cut[part + 1])
        if b0 > 0:
            lo[split.axis] = F32(float(split.x0) + b0 / float(split.inv) - margin)
        if b1 < BINS:
            hi[split.axis] = F32(float(split.x0) + b1 / float(split.inv) + margin)
    return lo, hi


def range_box(pts, begin, end, target):
    olo, ohi = box_of(pts[begin:end])
    margin = F32(MARGIN_EDGES * first_edge(olo, ohi, end - begin, target))
    return olo - margin, ohi + margin


def in_box(pts, lo, hi):
    pts = np.asarray(pts, F32)
    return np.all((pts >= np.asarray(lo, F32)) & (pts <= np.asarray(hi, F32)), axis=1)


def trimmed(kept_pts):
    """does the grid box of this kept set lose a good part of an axis to mean +- 6 sigma (trim_box)?  Then the rows outside
    are clamped into the boundary cells."""
    p = np.asarray(kept_pts, np.float64)
    if len(p) < 2:
        return False
    lo, hi, mean, sd = p.min(0), p.max(0), p.mean(0), p.std(0)
    tlo, thi = np.maximum(lo, mean - 6 * sd), np.minimum(hi, mean + 6 * sd)
    gone = np.maximum(tlo - lo, 0) + np.maximum(hi - thi, 0)
    return bool(np.any((gone > 0.25 * (thi - tlo)) & (thi > tlo)))


# ---- the retry verdict --------------------------------------------------------------------------------------------------
def kth_distance(q, pool, kth, w):
    """Distance from each q to the kth-smallest (0-based, so kth = k counts the row itself at distance 0) point of the pool,
    float64 brute force.  Exact where the answer is <= w: candidates are all pool points within w along the longest axis,
    and whatever lies farther along one axis lies farther.  Rows whose answer exceeds w are done again over the whole pool."""
    q, pool = np.asarray(q, np.float64), np.asarray(pool, np.float64)
    out = np.full(len(q), np.inf)
    if len(q) == 0 or len(pool) <= kth:
        return out
    axis = int(np.argmax(pool.max(0) - pool.min(0)))
    P = pool[np.argsort(pool[:, axis], kind="stable")]
    key = P[:, axis]
    qo = np.argsort(q[:, axis], kind="stable")
    for s in range(0, len(q), 128):
        idx = qo[s:s + 128]
        Q = q[idx]
        a = np.searchsorted(key, Q[:, axis].min() - w, "left")
        b = np.searchsorted(key, Q[:, axis].max() + w, "right")
        if b - a > kth:
            d = Q[:, None, :] - P[None, a:b, :]
            d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
            out[idx] = np.sqrt(np.partition(d2, kth, axis=1)[:, kth])
    for i in np.flatnonzero(out > w):
        d = pool - q[i]
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        out[i] = np.sqrt(np.partition(d2, kth)[kth])
    return out


def face_distance(q, lo, hi):
    q = np.asarray(q, np.float64)
    t = np.minimum(q - np.asarray(lo, np.float64), np.asarray(hi, np.float64) - q).min(1)
    return np.maximum(t, 0.0)


def row_verdicts(d_k, d_face, eps=0.0):
    """per row: +1 retry, 0 no retry, -1 undecided"""
    m = np.minimum(d_k, eps) if eps > 0 else np.asarray(d_k, np.float64)
    with np.errstate(invalid="ignore"):
        v = np.where(m > (1.0 - SLACK) * d_face, 1, 0)
        v[np.abs(m - d_face) < BAND * d_face] = -1
    v[np.isinf(d_face)] = 0
    return v


def call_verdict(v):
    return "retry" if np.any(v == 1) else "undecided" if np.any(v == -1) else "no retry"


class Cloud:
    """a cloud and what is computed once for it: the distance of every row to its k-th neighbour in the WHOLE cloud"""

    def __init__(self, pts):
        self.f64 = np.asarray(pts).dtype == np.float64
        self.pts = np.ascontiguousarray(pts, F32)
        self.pts.setflags(write=False)
        self.n = len(self.pts)
        self.lo, self.hi = box_of(self.pts)
        self._dk = {}

    def d_k(self, k):
        if k not in self._dk:
            w = 3.0 * first_edge(self.lo, self.hi, self.n, max(27.0, k + 1.0))        # (only a first window: rows beyond it are done again)
            self._dk[k] = kth_distance(self.pts, self.pts, k, w)
        return self._dk[k]

    def verdict(self, owned_idx, kept_mask, k, eps, lo, hi):
        """(call verdict, rows undecided, rows saying retry).  A row whose k nearest in the whole cloud lie within its
        distance to the faces has them all kept: its d_k among the kept is the cloud's.  The others are measured."""
        q = self.pts[owned_idx].astype(np.float64)
        d_face = face_distance(q, lo, hi)
        d_k = self.d_k(k)[owned_idx].copy()
        rest = np.flatnonzero(~(d_k <= (1.0 - 2 * BAND) * d_face))
        if len(rest):
            w = float(d_face[rest].max()) * (1.0 + 2 * BAND)
            d_k[rest] = kth_distance(q[rest], self.pts[kept_mask], k, w)
        v = row_verdicts(d_k, d_face, eps)
        return call_verdict(v), int(np.sum(v == -1)), int(np.sum(v == 1))


# ---- a handle: what a call keeps and whether it repeats ------------------------------------------------------------------
class Handle:
    """The state of one pct_ctx that ownership reads.  slab() and ranged() answer one pct_curvature / pct_knn call:
    dict(grid_points, limit_retries, verdict, undecided, kept (first attempt), box, trimmed)."""

    def __init__(self, factor=0.0):
        self.factor = factor
        self.box_key = None        # (n, begin, end) the kept box was measured for, None: not valid
        self.box = None
        self.cloud = None

    def set_cloud(self, cloud):
        self.cloud = cloud if isinstance(cloud, Cloud) else Cloud(cloud)
        self.begin, self.end = 0, self.cloud.n
        self.no_cull = False

    def set_range(self, begin, end):
        self.begin, self.end = begin, end
        self.no_cull = False

    def _decide(self, owned_idx, kept_mask, k, eps, lo, hi):
        c = self.cloud
        kept = int(kept_mask.sum())
        out = dict(kept=kept, box=(lo, hi), verdict="no retry", undecided=0, limit_retries=0, grid_points=kept,
                   trimmed=trimmed(c.pts[kept_mask]))
        if kept < k + 1:                                   # restart: every point, no retry counted
            self.no_cull, self.box_key = True, None
            out.update(grid_points=c.n, trimmed=False)
        elif kept < c.n:
            out["verdict"], out["undecided"], _ = c.verdict(owned_idx, kept_mask, k, eps, lo, hi)
            if out["verdict"] == "retry":
                self.no_cull, self.box_key = True, None
                out.update(grid_points=c.n, limit_retries=1)
        return out

    def slab(self, part, parts, k, eps=0.0, margin_edges=MARGIN_EDGES, split=None):
        c = self.cloud
        self.no_cull = False                               # (pct_set_query_slab precedes every slab call here)
        s = split or Split(c.pts, parts)
        owned = s.owned(part)
        if not owned.any():
            return dict(kept=c.n, box=None, verdict="no retry", undecided=0, limit_retries=0, grid_points=c.n, trimmed=False)
        a0 = first_edge(c.lo, c.hi, c.n, target_of(k, self.factor))
        lo, hi = slab_box(s, part, a0, margin_edges)
        return self._decide(np.flatnonzero(owned), owned | in_box(c.pts, lo, hi), k, eps, lo, hi)

    def ranged(self, k, eps=0.0):
        c = self.cloud
        b, e = self.begin, self.end
        if c.f64 or e == b or (b == 0 and e == c.n) or self.no_cull:
            return dict(kept=c.n, box=None, verdict="no retry", undecided=0, limit_retries=0, grid_points=c.n, trimmed=False)
        if self.box_key != (c.n, b, e):
            self.box = range_box(c.pts, b, e, target_of(k, self.factor))
            self.box_key = (c.n, b, e)
        lo, hi = self.box
        owned = np.zeros(c.n, bool)
        owned[b:e] = True
        return self._decide(np.arange(b, e), owned | in_box(c.pts, lo, hi), k, eps, lo, hi)


# ---- the clouds of tests/test_gpu_ownership.py (tests/test_ownership_exact.py shows that no call of theirs is undecided) --
def _egg(n, rng):
    xy = rng.uniform(-1, 1, (n, 2))
    return np.column_stack([xy, 0.1 * np.sin(np.pi * xy[:, 0]) * np.cos(np.pi * xy[:, 1])])


def _torus(n, rng, R=1.0, r=0.4):
    th, ph = rng.uniform(0, 2 * np.pi, (2, n))
    return np.column_stack([(R + r * np.cos(ph)) * np.cos(th), (R + r * np.cos(ph)) * np.sin(th), r * np.sin(ph)])


def make_cloud(kind, n, seed=1):
    rng = np.random.default_rng(seed)
    if kind == "egg":                       # rows in no spatial order
        p = _egg(n, rng)
    elif kind == "torus":
        p = _torus(n, rng)
    elif kind == "lattice":                 # x and y extents tie exactly; whole planes of points share a bin
        side = int(np.ceil(np.sqrt(n)))
        g = np.linspace(-1, 1, side)
        X, Y = np.meshgrid(g, g, indexing="ij")
        p = np.column_stack([X.ravel(), Y.ravel(), 0.1 * np.sin(np.pi * X.ravel()) * np.cos(np.pi * Y.ravel())])
        p = p[rng.permutation(len(p))[:n]] if n < len(p) else p
    elif kind == "flat":                    # half the cloud in one plane across the cut axis: one bin, half of the slabs empty
        xy = rng.uniform(-1e-3, 1e-3, (n, 2))
        z = np.where(np.arange(n) % 2 == 0, 0.0, rng.uniform(0, 1, n))
        p = np.column_stack([xy, z])[rng.permutation(n)]
    elif kind == "two":                     # two densities, 10 : 1, along the cut axis
        nd = n * 10 // 11
        x = np.concatenate([rng.uniform(-1, 0, nd), rng.uniform(0, 1, n - nd)])
        y = rng.uniform(-0.4, 0.4, n)
        p = np.column_stack([x, y, 0.05 * np.sin(3 * x) * np.cos(3 * y)])[rng.permutation(n)]
    elif kind == "ycut":
        p = _egg(n, rng) * [0.5, 1.5, 1.0]
    elif kind == "zcut":
        p = _egg(n, rng)[:, [2, 0, 1]] * [1.0, 0.6, 1.3]
    elif kind == "scan":                    # a torus whose rows follow the major angle: index ranges are spatial
        p = _torus(n, rng)
        p = p[np.argsort(np.arctan2(p[:, 1], p[:, 0]), kind="stable")]
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(p, F32)


def plant_on_cut(pts, parts=2, part=1):
    """One point of the cloud moved, from the first occupied bin at or past cut[part], onto a coordinate whose float32
    product reaches bin cut[part] while the exact product stays below it.  The box and this cut are what they were.
    Returns (cloud, index)."""
    pts = np.array(pts, F32)
    s = Split(pts, parts)
    b = int(s.cut[part])
    x = rounds_across(s.x0, s.inv, b)
    if not len(x):
        raise ValueError("no coordinate at this cut rounds across it")
    cand = np.flatnonzero((s.bins >= b) & (pts[:, s.axis] < s.hi[s.axis]))       # (from a bin at or past the cut: cum[b] stays)
    i = int(cand[np.argmin(pts[cand, s.axis])])
    pts[i, s.axis] = x[0]
    assert Split(pts, parts).cut[part] == b
    return pts, i


def rounds_across(x0, inv, b, ulps=256):
    """the float32 coordinates within `ulps` of the lower boundary of bin b whose float32 product lands in b and whose exact
    product lands in b - 1"""
    x = np.empty(2 * ulps + 1, F32)
    x[ulps] = F32(float(x0) + b / float(inv))
    for j in range(ulps):
        x[ulps + j + 1] = np.nextafter(x[ulps + j], F32(np.inf))
        x[ulps - j - 1] = np.nextafter(x[ulps - j], F32(-np.inf))
    return x[(bins_of(x, x0, inv) == b) & (bins_in_double(x, x0, inv) == b - 1)]


def plant_on_face(pts, parts, part, k, factor=0.0):
    """One point beyond the upper face of slab `part` moved exactly onto that face (inclusive: it is kept).  It stays in a
    bin past the slab, so the cuts up to this slab, the box and a0 are what they were.  Returns (cloud, index)."""
    pts = np.array(pts, F32)
    s = Split(pts, parts)
    a0 = first_edge(s.lo, s.hi, s.n, target_of(k, factor))
    _, hi = slab_box(s, part, a0)
    beyond = np.flatnonzero((pts[:, s.axis] > hi[s.axis]) & (pts[:, s.axis] < s.hi[s.axis]))
    i = int(beyond[np.argmin(pts[beyond, s.axis])])
    pts[i, s.axis] = hi[s.axis]
    assert not Split(pts, parts).owned(part)[i]
    return pts, i


PARTS = (1, 2, 3, 7, 64)

# name: (kind, n, seed, k, eps, factor); the sizes cover every n mod 4, one and two chunk boundaries of 8192 and a last chunk
# of one point; k covers one and two list registers, the boundary between them (61) and the exact sweep (200)
SLAB_CASES = {
    "egg_4099_k30": ("egg", 4099, 3, 30, 0.0, 0.0),
    "torus_4097_k8": ("torus", 4097, 4, 8, 0.0, 0.0),
    "lattice_4096_k30": ("lattice", 4096, 5, 30, 0.0, 0.0),
    "flat_8191_k61": ("flat", 8191, 6, 61, 0.0, 0.0),
    "two_8192_k80": ("two", 8192, 7, 80, 0.0, 0.0),
    "ycut_8193_k30_eps": ("ycut", 8193, 8, 30, 0.05, 0.0),
    "zcut_12290_k200": ("zcut", 12290, 9, 200, 0.0, 0.0),
    "egg_24577_k30": ("egg", 24577, 10, 30, 0.0, 0.0),
    "torus_8193_k30_factor2": ("torus", 8193, 11, 30, 0.0, 2.0),
    "egg_4097_k30_on_cut": ("egg", 4097, 12, 30, 0.0, 0.0),
    "egg_8193_k30_on_face": ("egg", 8193, 13, 30, 0.0, 0.0),
}
MARGIN_CASE = ("egg", 8193, 14, 30, 4)      # kind, n, seed, k, parts: PCT_SLAB_MARGIN at two values either side of the verdict

_cache = {}


def slab_cloud(name):
    if name not in _cache:
        kind, n, seed, k, eps, factor = SLAB_CASES[name]
        pts = make_cloud(kind, n, seed)
        if name.endswith("on_cut"):
            pts, _ = plant_on_cut(pts)
        if name.endswith("on_face"):
            pts, _ = plant_on_face(pts, 2, 0, k, factor)
        _cache[name] = Cloud(pts)
    return _cache[name]


def slab_expectation(name):
    """per parts: (Split, [the restated call of every part])"""
    key = ("expect", name)
    if key not in _cache:
        kind, n, seed, k, eps, factor = SLAB_CASES[name]
        c, h, out = slab_cloud(name), Handle(factor), {}
        h.set_cloud(c)
        for parts in PARTS:
            s = Split(c.pts, parts)
            out[parts] = (s, [h.slab(p, parts, k, eps, split=s) for p in range(parts)])
        _cache[key] = out
    return _cache[key]


def margin_cloud():
    if "margin_cloud" not in _cache:
        kind, n, seed, k, parts = MARGIN_CASE
        _cache["margin_cloud"] = Cloud(make_cloud(kind, n, seed))
    return _cache["margin_cloud"]


def margin_expectation(margin_edges):
    """the restated calls of MARGIN_CASE's slabs under PCT_SLAB_MARGIN = margin_edges"""
    key = ("margin", margin_edges)
    if key not in _cache:
        kind, n, seed, k, parts = MARGIN_CASE
        h = Handle()
        h.set_cloud(margin_cloud())
        s = Split(h.cloud.pts, parts)
        _cache[key] = (s, [h.slab(p, parts, k, 0.0, margin_edges, split=s) for p in range(parts)])
    return _cache[key]


MARGINS = (0.25, 3.0)

# ---- index ranges ---------------------------------------------------------------------------------------------------------
RANGE_N, RANGE_K = 8193, 30
RANGES = {"quarter": (RANGE_N // 4, RANGE_N // 2), "one_row": (100, 101), "last_three": (RANGE_N - 3, RANGE_N),
          "begin_not_by_4": (RANGE_N // 4 + 1, RANGE_N // 2 + 3)}


def range_cloud():
    if "range_cloud" not in _cache:
        _cache["range_cloud"] = Cloud(make_cloud("scan", RANGE_N, 21))
    return _cache["range_cloud"]


def range_expectation(name):
    h = Handle()
    h.set_cloud(range_cloud())
    h.set_range(*RANGES[name])
    return h.ranged(RANGE_K)


def restart_cloud(in_box):
    """rows [0, 20) a tight cluster, `in_box` more rows of it behind them (not owned, inside any box around the 20), the
    rest far away: owning [0, 20) with k = 30 keeps 20 + in_box points"""
    rng = np.random.default_rng(23)
    cluster = rng.normal(scale=1e-3, size=(20 + in_box, 3))
    rest = rng.uniform(2.0, 3.0, size=(5000, 3))
    return np.vstack([cluster, rest]).astype(F32)


def stream_clouds():
    """four clouds of one size for one handle that owns rows [n/4, n/2): the second is the first moved a little along x (the
    box measured on the first keeps another count, no owned row leaves it), the third moved by half the extent (owned rows
    leave the box), the fourth is the third again"""
    a = make_cloud("scan", 6001, 22)
    return a, (a + F32([0.11, 0, 0])).astype(F32), (a + F32([1.5, 0, 0])).astype(F32), (a + F32([1.5, 0, 0])).astype(F32)


def tie_cloud(base, begin, box, k, d0):
    """`base` with the owned row `begin` lifted to d (about d0) below the upper z face of `box`, above the middle of the box,
    k - 1 rows of the front of the cloud (not owned) close around it and one exactly on the face above it: the row's k-th
    neighbour among the kept is as far as the face, to the last bit.  Returns (cloud, d)."""
    pts = np.array(base, F32)
    lo, hi = box
    cx, cy, fz = F32(0.5) * (lo[0] + hi[0]), F32(0.5) * (lo[1] + hi[1]), hi[2]
    qz = F32(float(fz) - d0)
    d = float(fz) - float(qz)
    pts[begin] = (cx, cy, qz)
    rng = np.random.default_rng(int(d0 * 1e6))
    pts[:k - 1] = pts[begin] + (rng.uniform(-0.2, 0.2, (k - 1, 3)) * d).astype(F32)
    pts[k - 1] = (cx, cy, fz)
    return pts, d


TIE_DISTANCES = (0.05, 0.06, 0.07, 0.08, 0.09, 0.1, 0.11, 0.12, 0.13, 0.14, 0.15, 0.16)

"""The build of the uniform cell list (pct_build_grid, csrc/pct_grid.hip), the census PCT_KNN_AUTO takes of it (k_item_census,
csrc/pct_knn.hip) and the ring at which the exact sweep stops (k_knn_exact, csrc/pct_knn_sweep.h), restated from their
definitions in NumPy.  Nothing here imports the package.

A wrong decision of the build -- an edge an octave off, a pass too many, a point filed one cell over, a miscounted
occupancy -- returns the right rows, only slowly.  This module says what the decisions ARE, for a whole-cloud handle or an
index range with culling off (PCT_NO_CULL); tests/test_gpu_grid_exact.py holds the device to them and
tests/test_grid_exact.py holds this module to the project's own records.  float32 where the device computes in float32 (the
box, the deferred-box check), float64 where the host and the kernels compute in double (everything else); the library is
built with -ffp-contract=off.  The rules, quoted:

  target      factor (k + 1): ownership_exact.target_of (pct_default_factor)
  box         "bbox and moments per block": float32 min / max per axis of the float32-rounded cloud (every point, owned or not)
  trim        "take mean +- 6 sigma per axis (re-estimated inside the box until it settles)": at most 5 passes, each counted in
              grid_iters; an axis shrinks where "cut > 0.25 * (hi - lo) && hi > lo".  The device sums its moments in another
              order: the DECISION is restated with a relative band of 1e-9, and of a trimmed cloud only the decision and the
              number of trim passes are reported (no grid).
  speculation "a handle fed a stream of similar clouds builds the cell list over the (trimmed) box of the previous call":
              hint_edge > 0, a box remembered for a cloud of this size, no PCT_NO_SPEC.  The cloud's own box is checked after
              the first pass, "within 2 % of the previous cloud's extent per face" in float32 (tol = 0.02f * ext + 1e-30f);
              a miss starts over the regular way (the pass lines of the dropped attempt were printed, its passes not counted).
  first edge  EdgeSearch::first: emax = the longest extent, 1 where that is not positive; area = 1.2 (ex ey + ey ez + ex ez),
              emax^2 where that is not positive; a = sqrt(target area / n), emax where that is not positive and finite; warm
              start: r = guess / hint_guess * sqrt(hint_target / target); for 0.5 < r < 2 a = hint_edge * r * sqrt(target /
              hint_target); min(a, cap()), cap() = emax * 1.0001 + 1e-30.
  per pass    a = clamp_eps(a): eps * 1.000001 where eps > 0 and a is larger;
              size_grid: inv = 1 / a, dims floor(e * inv) + 1 per axis in double; "an absurdly small edge must read as far
              too many cells": dims 2^30 and 2^62 cells unless the product is below 4e18 and every dimension below 2e9;
              ncell > 16 n and ncell > 2^20 (the give-up test of PCT_KNN_AUTO): on pass 0 of a warm-started search the
              cloud's own first guess replaces the edge (fallback_first, not clamped again); otherwise GaveUp where the
              caller may give up, else nothing;
              while ncell > cell_cap: a *= cbrt(ncell / cell_cap) * 1.01 (hit_cap); cell_cap = 2^27, or 32 n up to 2^30
              above that; 2^24 under level_mode;
              cell of a point = clamp(floor((double(x32) - double(o32)) * inv), 0, dim - 1) per axis, id = (cz ny + cy) nx + cx;
              per cell owned and total points; sumsq = sum owned * total, m = sumsq / n_owned; items = sum ceil(owned /
              items_q) (16, or PCT_ITEMS_Q in [1, 64]); non-empty cells;
              accept: 0.88 target <= m <= 1.12 target, or the last pass (max_iter = 8), or (eps > 0, a >= eps, m < target),
              or (2 ncell > cell_cap, m < target), or (a >= emax, m < target), or (hit_cap, m > target), or -- NO_EXTENT_STOPS
              -- the box has no extent (one cell at every edge: no step can change the occupancy);
              next: d = log(m / m_prev) / log(a / a_prev) clamped to [1, 3] once two passes differ in both, else 2;
              a * clamp((target / m)^(1/d), 1/16, 16), min with cap().
  result      grid_iters (trim passes + passes of the accepted attempt), cells, cell_size, grid_points, occupied_cells (the
              work items: commit_grid stores tot.y there), occupancy, as pct_timings reports them; the next build's warm
              start hint_after = cell * (target / m)^(1/d_last), with this cloud's own first guess and target.
              Refused: "the cell list cannot resolve this cloud" where m > 64 target and 27 m n_owned > 1e12.
  census      k_item_census, per work item (cell, chunk): nq = min(items_q, owned - chunk items_q); stencil = the cells of
              the 3 x 3 x 3 cube inside the grid; m = their points, occupied = those that hold any.  Words: sum nq | sum nq
              where m > cap | sum nq where m <= cap and 2 m < 5 (k + 1) | sum nq * occupied over the rest.  cap =
              PCT_STAGE_CAP (512) for k + 1 <= 61, else PCT_STAGE_CAP2 (768) (pct_item_census).  census_shares: cells =
              word 3 / (word 0 - word 1 - word 2), 27 where that count is not positive.
  overflow    item_overflows, uniform list: m > cap, the same m and the same caps (k_knn_pair 512, k_knn_duo 768,
              k_knn_fast 512 | 768): every item of such a cell is handed to the exact sweep and counted in lds_overflows.
  final ring  k_knn_exact: rings 1, 2, 3, 4, then ring + (ring + 1) / 2 (6, 9, 14, ...); stops at the first with
              min(tau, eps^2) <= guaranteed_r2(ring) (tree_exact.guaranteed_r2 per axis: the minimum over the axes commutes
              with the monotone rounding steps behind it).  The sweep's own tau after a ring is the (k+1)-th smallest
              distance inside that ring's cube; it is the row's true one exactly when the test passes (the guaranteed ball
              lies inside the cube), so the true tau -- the fp64 ((dx dx + dy dy) + dz dz) to the (k+1)-th nearest float32
              record, self included -- decides the same ring.  The cell is that of the float32 record, the offset inside
              it (q - o) * inv - c with the native float64 coordinates where the cloud has them.  A row is undecided when
              at a ring it tests the two sides lie within a relative 2^-40 (tree_exact.UNDECIDED_REL, for its reason).
"""
import ctypes
import ctypes.util
import math

import numpy as np

import ownership_exact as oe
import tree_exact as te

F32 = np.float32
WIN_LO, WIN_HI = 0.88, 1.12
MAX_ITER = 8
STAGE_CAP, STAGE_CAP2 = 512, 768            # PCT_STAGE_CAP, PCT_STAGE_CAP2 (csrc/pct_internal.h); PCT_DUO_CAP is 768 too
TRIM_BAND = 1e-9
NO_EXTENT_STOPS = True                      # EdgeSearch::accept ends the search of a box without extent at its first pass

try:
    cbrt = math.cbrt                        # the C library's, as the host code calls it (NumPy's own differs in the last bit)
except AttributeError:
    _libm = ctypes.CDLL(ctypes.util.find_library("m"))
    _libm.cbrt.restype, _libm.cbrt.argtypes = ctypes.c_double, [ctypes.c_double]
    cbrt = _libm.cbrt

_OFFSETS = np.array([(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)], np.int64)


def stage_cap(k):
    return STAGE_CAP if k + 1 <= oe.FAST_R1_MAX else STAGE_CAP2


def cell_cap_of(n, level_mode=False):
    if level_mode:
        return 1 << 24
    cap = 1 << 27
    if 32 * n > cap:
        cap = min(32 * n, 1 << 30)
    return cap


def items_q_of(env_value=None):
    """PCT_ITEMS_Q as pct_build_grid reads it"""
    if env_value is not None and 1 <= int(env_value) <= 64:
        return int(env_value)
    return 16


# ---- EdgeSearch (csrc/pct_grid_edge.h) ------------------------------------------------------------------------------------
class EdgeSearch:
    def __init__(self, target, n, ext, eps=0.0, hint=(0.0, 0.0, 0.0), max_iter=MAX_ITER):
        self.target, self.n, self.eps, self.max_iter = float(target), int(n), float(eps), max_iter
        self.ex, self.ey, self.ez = (float(e) for e in ext)
        self.hint_edge, self.hint_guess, self.hint_target = hint
        self.emax, self.first_guess, self.hinted, self.no_extent = 1.0, 0.0, False, False
        self.a_prev, self.m_prev, self.d_last = 0.0, 0.0, 2.0

    def cap(self):
        return self.emax * 1.0001 + 1e-30

    def first(self):
        self.emax = max(self.ex, self.ey, self.ez)
        self.no_extent = not self.emax > 0
        if self.no_extent:
            self.emax = 1.0
        area = 1.2 * (self.ex * self.ey + self.ey * self.ez + self.ex * self.ez)
        if not area > 0:
            area = self.emax * self.emax
        a = math.sqrt(self.target * area / float(self.n))
        if not (a > 0 and math.isfinite(a)):
            a = self.emax
        self.first_guess, self.hinted = a, False
        if self.hint_edge > 0 and self.hint_guess > 0:
            r = self.first_guess / self.hint_guess * math.sqrt(self.hint_target / self.target)
            if 0.5 < r < 2.0:
                a = self.hint_edge * r * math.sqrt(self.target / self.hint_target)
                self.hinted = True
        return min(a, self.cap())

    def fallback_first(self):
        self.hinted = False
        return min(self.first_guess, self.cap())

    def clamp_eps(self, a):
        return self.eps * 1.000001 if self.eps > 0 and a > self.eps * 1.000001 else a

    def accept(self, m, a, ncell, cell_cap, hit_cap, it):
        eps_bound = self.eps > 0 and a >= self.eps
        capped = ncell * 2 > cell_cap and m < self.target
        return bool((WIN_LO * self.target <= m <= WIN_HI * self.target) or it == self.max_iter - 1 or (eps_bound and m < self.target)
                    or capped or (a >= self.emax and m < self.target) or (hit_cap and m > self.target)
                    or (NO_EXTENT_STOPS and self.no_extent))

    def next(self, m, a):
        d = 2.0
        if self.a_prev > 0 and m != self.m_prev and a != self.a_prev:
            d = math.log(m / self.m_prev) / math.log(a / self.a_prev)
            if not d >= 1.0:
                d = 1.0
            if d > 3.0:
                d = 3.0
        self.a_prev, self.m_prev, self.d_last = a, m, d
        f = math.pow(self.target / m, 1.0 / d)
        f = min(max(f, 1.0 / 16.0), 16.0)
        return min(a * f, self.cap())

    def hint_after(self, cell, m_last):
        return cell * math.pow(self.target / m_last, 1.0 / self.d_last)


# ---- the grid of one pass ---------------------------------------------------------------------------------------------------
def size_grid(lo32, hi32, a):
    """(inv, (nx, ny, nz), ncell); the sentinel of an absurd edge is ((2^30,) * 3, 2^62)"""
    inv = 1.0 / a
    ext = [float(hi32[i]) - float(lo32[i]) for i in range(3)]
    ext = [e if e >= 0 else 0.0 for e in ext]
    d = [math.floor(e * inv) + 1.0 if math.isfinite(e * inv) else math.inf for e in ext]
    if not (d[0] * d[1] * d[2] < 4.0e18) or not all(v < 2.0e9 for v in d):
        return inv, (1 << 30,) * 3, 1 << 62
    dims = tuple(int(v) for v in d)
    return inv, dims, dims[0] * dims[1] * dims[2]


def cell_coords(p32, lo32, inv, dims):
    """clamp(floor((double(x32) - double(o32)) * inv), 0, dim - 1) per axis: (n, 3) int64"""
    t = np.floor((np.asarray(p32, F32).astype(np.float64) - np.asarray(lo32, F32).astype(np.float64)) * inv)
    return np.clip(t, 0.0, np.asarray(dims, np.float64) - 1.0).astype(np.int64)


def cell_ids(c, dims):
    return (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]


class Cells:
    """the occupied cells of a grid: ids (sorted), total and owned points of each, and every point's cell"""

    def __init__(self, p32, owned, lo32, inv, dims):
        self.dims = dims
        self.coord = cell_coords(p32, lo32, inv, dims)
        self.ids, self.of_point, self.total = np.unique(cell_ids(self.coord, dims), return_inverse=True, return_counts=True)
        self.of_point = self.of_point.ravel()
        self.total = self.total.astype(np.int64)
        self.owned = np.bincount(self.of_point, weights=owned.astype(np.float64), minlength=len(self.ids)).astype(np.int64)

    def population(self, ids):
        """points of the cells `ids` (any shape), 0 for a cell that holds none"""
        at = np.minimum(np.searchsorted(self.ids, ids), len(self.ids) - 1)
        return np.where(self.ids[at] == ids, self.total[at], 0)

    def stencils(self, drop=None):
        """per occupied cell: (points, non-empty cells) of the 3 x 3 x 3 cube inside the grid; drop: a stencil cell (0 .. 26)
        left out, for the tests"""
        nx, ny, nz = self.dims
        cx, cy, cz = self.ids % nx, (self.ids // nx) % ny, self.ids // (nx * ny)
        x, y, z = cx[:, None] + _OFFSETS[:, 0], cy[:, None] + _OFFSETS[:, 1], cz[:, None] + _OFFSETS[:, 2]
        inside = (x >= 0) & (x < nx) & (y >= 0) & (y < ny) & (z >= 0) & (z < nz)
        pop = np.where(inside, self.population(np.where(inside, (z * ny + y) * nx + x, 0)), 0)
        if drop is not None:
            pop[:, drop] = 0
        return pop.sum(1), (pop > 0).sum(1)


# ---- box, trim ----------------------------------------------------------------------------------------------------------------
def trim_box(p32, lo32, hi32):
    """trim_box: (lo32, hi32, passes, undecided).  passes = the trim passes counted in grid_iters."""
    p = np.asarray(p32, F32)
    lo, hi = np.array(lo32, F32), np.array(hi32, F32)
    shift = np.zeros(3)
    inside = np.ones(len(p), bool)
    passes, undecided = 0, False
    for _ in range(5):
        cnt = int(inside.sum())
        if cnt < 2:
            break
        d = p[inside].astype(np.float64) - shift
        mean = d.sum(0) / cnt
        var = np.maximum((d * d).sum(0) / cnt - mean * mean, 0.0)
        sd, c = np.sqrt(var), shift + mean
        nlo, nhi, shrunk = lo.copy(), hi.copy(), False
        for a in range(3):
            l, h = max(float(lo[a]), c[a] - 6.0 * sd[a]), min(float(hi[a]), c[a] + 6.0 * sd[a])
            cut = max(l - float(lo[a]), 0.0) + max(float(hi[a]) - h, 0.0)
            if h > l and abs(cut - 0.25 * (h - l)) <= TRIM_BAND * (h - l):
                undecided = True
            if cut > 0.25 * (h - l) and h > l:
                nlo[a], nhi[a], shrunk = F32(l), F32(h), True
        if not shrunk:
            break
        lo, hi = nlo, nhi
        shift = (F32(0.5) * (lo + hi)).astype(np.float64)
        inside = np.all((p >= lo) & (p <= hi), axis=1)
        passes += 1
    return lo, hi, passes, undecided


def same_box(lo32, hi32, raw_lo, raw_hi):
    """check_deferred_box, in float32"""
    for a in range(3):
        tol = F32(0.02) * (F32(raw_hi[a]) - F32(raw_lo[a])) + F32(1e-30)
        if not (abs(F32(lo32[a]) - F32(raw_lo[a])) <= tol and abs(F32(hi32[a]) - F32(raw_hi[a])) <= tol):
            return False
    return True


# ---- a handle and its builds ----------------------------------------------------------------------------------------------------
class Handle:
    """what one pct_ctx carries from build to build: the warm start and the remembered box (nothing resets them)"""

    def __init__(self, factor=0.0):
        self.factor = factor
        self.hint = (0.0, 0.0, 0.0)          # hint_edge, hint_guess, hint_target
        self.spec_valid, self.spec_n, self.spec_box, self.spec_raw = False, 0, None, None
        self.unknown = False                 # a trimmed build went by: its edge is not restated

    def build(self, pts, k, eps=0.0, begin=0, end=None, items_q=16, no_spec=False, may_give_up=False):
        """pct_build_grid for rows [begin, end) owned (culling off).  Returns a dict:
        trimmed, trim_passes, trim_undecided; and, unless trimmed: verdict ("built" | "gave_up" | "refused"), give_up_test
        (the ncell test was met on some pass), grid_iters, cells, cell_size, grid_points, occupied_cells, occupancy, nonempty,
        dims, lo (the grid's origin), inv, lines [(pass, "%g" of the edge, (nx, ny, nz), cells)] as PCT_GRID_DEBUG prints
        them (dropped attempts included), edges (of the accepted attempt), speculative, hinted, cells_obj (Cells)."""
        assert not self.unknown, "the handle's warm start is not restated after a trimmed build"
        p32 = np.ascontiguousarray(np.asarray(pts).astype(F32))
        n = len(p32)
        end = n if end is None else end
        owned = np.zeros(n, bool)
        owned[begin:end] = True
        n_owned = end - begin
        target = oe.target_of(k, self.factor)
        cell_cap = cell_cap_of(n)
        raw_lo, raw_hi = oe.box_of(p32)
        lines = []
        for attempt in range(3):
            spec = not no_spec and self.hint[0] > 0 and self.spec_valid and self.spec_n == n
            out = dict(trimmed=False, trim_passes=0, trim_undecided=False, speculative=spec)
            if spec:
                lo, hi = self.spec_box
            else:
                lo, hi, out["trim_passes"], out["trim_undecided"] = trim_box(p32, raw_lo, raw_hi)
                if out["trim_passes"] > 0:
                    self.unknown = True
                    return dict(out, trimmed=True, lines=lines)
            es = EdgeSearch(target, n, [float(hi[i]) - float(lo[i]) for i in range(3)], eps, self.hint)
            a = es.first()
            out["hinted"] = es.hinted
            iters, m, give_up_test, edges, restart = 0, 0.0, False, [], False
            for it in range(es.max_iter):
                a = es.clamp_eps(a)
                inv, dims, ncell = size_grid(lo, hi, a)
                if ncell > 16 * n and ncell > (1 << 20):
                    give_up_test = True
                    if it == 0 and es.hinted:
                        a = es.fallback_first()
                        inv, dims, ncell = size_grid(lo, hi, a)
                    elif may_give_up:
                        return dict(out, verdict="gave_up", give_up_test=True, lines=lines)
                hit_cap = False
                while ncell > cell_cap:
                    a *= cbrt(float(ncell) / float(cell_cap)) * 1.01
                    inv, dims, ncell = size_grid(lo, hi, a)
                    hit_cap = True
                lines.append((it, "%g" % a, dims, ncell))
                if spec and it == 0 and not same_box(raw_lo, raw_hi, *self.spec_raw):
                    self.spec_valid = False
                    restart = True
                    break
                edges.append(a)
                cells = Cells(p32, owned, lo, inv, dims)
                sumsq = int((cells.owned * cells.total).sum())
                m = float(sumsq) / float(n_owned if n_owned > 0 else 1)
                iters += 1
                if es.accept(m, a, ncell, cell_cap, hit_cap, it):
                    break
                a = es.next(m, a)
            if restart:
                continue
            # commit_grid
            self.spec_box, self.spec_raw, self.spec_n, self.spec_valid = (lo, hi), (raw_lo, raw_hi), n, True
            if m > 0:
                self.hint = (es.hint_after(a, m), es.first_guess, es.target)
            items = int(((cells.owned + items_q - 1) // items_q).sum())
            refused = m > 64.0 * target and m * 27.0 * float(n_owned) > 1e12
            out.update(verdict="refused" if refused else "built", give_up_test=give_up_test, grid_iters=out["trim_passes"] + iters,
                       cells=ncell, cell_size=a, grid_points=n, occupied_cells=items, occupancy=m, nonempty=int((cells.total > 0).sum()),
                       dims=dims, lo=np.asarray(lo, F32), inv=inv, lines=lines, edges=edges, cells_obj=cells, owned=owned, items_q=items_q,
                       target=target, d_last=es.d_last)
            return out
        raise AssertionError("restarted more than twice")


def build(pts, k, eps=0.0, **kw):
    """a fresh handle's build"""
    return Handle().build(pts, k, eps, **kw)


def row_of(b):
    """a build as a row of test_gpu_grid_plan.EXPECTED"""
    return (b["grid_iters"], b["cells"], float(b["cell_size"]).hex(), b["grid_points"], b["occupied_cells"], float(b["occupancy"]).hex())


# ---- census, overflowing items --------------------------------------------------------------------------------------------------
def census(b, k, drop=None):
    """the four words of k_item_census, and census_shares' cells figure"""
    c = b["cells_obj"]
    m, occupied = c.stencils(drop)
    cap = stage_cap(k)
    over = m > cap
    short = ~over & (2 * m < 5 * (k + 1))
    rest = ~over & ~short
    w = (int(c.owned.sum()), int(c.owned[over].sum()), int(c.owned[short].sum()), int((c.owned[rest] * occupied[rest]).sum()))
    fine = float(w[0]) - float(w[1] + w[2])
    return w, (float(w[3]) / fine if fine > 0 else 27.0)


def overflowing(b, k):
    """(work items handed over whole, their queries, per point: is it a query of one)"""
    c = b["cells_obj"]
    m, _ = c.stencils()
    over = m > stage_cap(k)
    q = b["items_q"]
    return int(((c.owned[over] + q - 1) // q).sum()), int(c.owned[over].sum()), over[c.of_point] & b["owned"]


# ---- the ring at which the exact sweep stops --------------------------------------------------------------------------------------
def tau_of(pts, k, rows, eps=0.0):
    """fp64 squared distance ((dx dx + dy dy) + dz dz) of the rows to their (k+1)-th nearest float32 record, self included;
    +inf where fewer than k + 1 records lie within eps (the sweep's list keeps what the eps ball holds).  A k-d tree names
    the k + 9 nearest records (eight to spare for its own rounding); the distances are then formed as the sweep forms them."""
    from scipy.spatial import cKDTree
    pts = np.asarray(pts)
    rec = pts.astype(F32).astype(np.float64)
    qry = pts.astype(np.float64)[rows] if pts.dtype == np.float64 else rec[rows]
    kk = min(k + 9, len(rec))
    _, cand = cKDTree(rec).query(qry, kk)
    c = rec[cand.reshape(len(qry), kk)]
    dx, dy, dz = c[:, :, 0] - qry[:, None, 0], c[:, :, 1] - qry[:, None, 1], c[:, :, 2] - qry[:, None, 2]
    out = np.sort((dx * dx + dy * dy) + dz * dz, axis=1)[:, k]
    if eps > 0:
        out[out > eps * eps] = np.inf
    return out


def tau_from_rows(pts, rows, idx, cnt=None):
    """the same from a neighbour table of the rows (k columns, self excluded, nearest first; cnt: valid columns under eps)"""
    pts = np.asarray(pts)
    rec = pts.astype(F32).astype(np.float64)
    qry = pts.astype(np.float64)[rows] if pts.dtype == np.float64 else rec[rows]
    k = idx.shape[1]
    last = rec[np.clip(idx[:, k - 1], 0, len(rec) - 1)]
    dx, dy, dz = last[:, 0] - qry[:, 0], last[:, 1] - qry[:, 1], last[:, 2] - qry[:, 2]
    tau = (dx * dx + dy * dy) + dz * dz
    if cnt is not None:
        tau = np.where(cnt >= k, tau, np.inf)
    return tau


def ring_sequence():
    ring = 1
    while True:
        yield ring
        ring = ring + 1 if ring < 4 else ring + (ring + 1) // 2


def guaranteed_r2(b, c, g, ring):
    """guaranteed_r2 of the grid of build b: cells c (m, 3), offsets g (m, 3)"""
    out = np.full(len(c), np.inf)
    for a in range(3):
        out = np.minimum(out, te.guaranteed_r2(b["dims"][a], b["cell_size"], c[:, a], c[:, a], c[:, a], g[:, a], g[:, a], g[:, a], ring))
    return out


def final_rings(pts, b, tau, eps=0.0):
    """per owned row (in index order): (final ring, decided)"""
    pts = np.asarray(pts)
    rows = np.flatnonzero(b["owned"])
    c = b["cells_obj"].coord[rows]
    q = pts.astype(np.float64)[rows] if pts.dtype == np.float64 else pts.astype(F32).astype(np.float64)[rows]
    g = (q - b["lo"].astype(np.float64)) * b["inv"] - c
    m = np.minimum(tau, eps * eps) if eps > 0 else np.asarray(tau, np.float64)
    ring_of = np.zeros(len(rows), np.int64)
    decided = np.ones(len(rows), bool)
    active = np.arange(len(rows))
    for ring in ring_sequence():
        if not len(active):
            break
        r2 = guaranteed_r2(b, c[active], g[active], ring)
        with np.errstate(invalid="ignore"):
            close = np.isfinite(r2) & (np.abs(m[active] - r2) <= te.UNDECIDED_REL * r2)
        decided[active[close]] = False
        stop = m[active] <= r2
        ring_of[active[stop]] = ring
        active = active[~stop]
    return ring_of, decided


def expected_counters(pts, b, k, tau, eps=0.0):
    """What the statistics words must hold.  lds_overflows: the overflowing items.  ring_fallbacks (k_knn_exact counts a row
    it answered beyond ring 1): between the decided rows with a final ring above 1 and that plus the undecided rows.
    redone_queries: at least the queries of the overflowing items plus the other decided rows with a final ring above 1."""
    ring, decided = final_rings(pts, b, tau, eps)
    items, queries, handed = overflowing(b, k)
    handed = handed[b["owned"]]
    wide = decided & (ring > 1)
    return dict(lds_overflows=items, overflow_queries=queries, fallbacks=(int(wide.sum()), int(wide.sum() + (~decided).sum())),
                redone_min=int(queries + (wide & ~handed).sum()), undecided=int((~decided).sum()), max_ring=int(ring.max()), ring=ring,
                decided=decided)

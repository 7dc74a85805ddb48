"""The build of the hierarchical cell list (csrc/pct_tree.hip) and the walk of its exact sweep (k_knn_exact_tree,
csrc/pct_knn_sweep.h), restated from their definitions in NumPy.  Nothing here imports the package.

Everything the build decides is a function of the float32 records, k, eps and four switches (PCT_TREE_NMIN, PCT_ITEMS_Q,
PCT_TREE_SPLIT, PCT_TREE_NO_REFINE).  What is restated is WHAT the kernels compute, not how:

  cube      box of the float32 records, ext = largest extent (1 if 0), root = ext (1 + 2^-18), cell = root 2^-21;
            q = clamp(floor((double(p) - o) / cell ... as (p - o) * (1 / cell)), 0, 2^21 - 1) per axis, code = the 3 x 21
            bit Morton interleave with x lowest.  Refused ("not built") unless cell^2 > 1e-30, root^2 < 1e30 and, with an
            eps, eps^2 > 1e-36.
  order     the codes sorted; rows of equal codes are interchangeable for everything below.
  level     of a row: the smallest l whose cell around it (rows with the same code >> 3 l) holds >= n_min rows, 21 if
            none does, capped at max_level.  It is COUNTED here, level by level; k_tree_level finds it by merging two
            monotone sequences of join levels, and that merge is what the count checks.
  segment   a maximal run of consecutive rows with the same level and the same cell of that level; ceil(L / items_q)
            work items, the last one short.
  stencil   population of a segment: rows in the in-range cells of the 3 x 3 x 3 cube around its cell at its level.
            "Over": population > cap at a level above 0.
  refine    every over segment is split by the octants of the level below, depth first: an octant still over (its OWN
            stencil population, level above 0) is split again, every other non-empty octant becomes a new segment with
            new items and its rows take the new level.  Old segments and items stay counted.
  sample    every 64th initial segment, weighted by its rows: the level histogram behind the spread and the share that
            PCT_KNN_AUTO reads.

exact_walk replays k_knn_exact_tree per sorted row from the level the build left: the 27 ranges of the level, the steps
(sum of ceil(range / 64)), tau = the (k+1)-th smallest float64 squared distance to the float32 records of those ranges
(self included; +inf with fewer than k+1 of them: Sweep::tau_d stays where reset() put it), the round ends when
min(tau, eps^2) <= r^2 (query_guaranteed_r2 of csrc/pct_query_plan.h, ring 1, the level's grid) or at level 21, else one
level up.  A row is undecided when a round's min(tau, eps^2) lies within a relative 2^-40 of r^2: the device evaluates the
same float64 expressions, only a contracted multiply-add can differ, and 2^-40 is 4096 ulp.  For such a row the walk
reports both ends: stopped at the first such round (fewest) and carried past every such round (most).
"""
import math

import numpy as np

BITS = 21
TOP = (1 << BITS) - 1
CAP_R1, CAP_R2, R1_MAX = 768, 1024, 61          # PCT_TREE_CAP, PCT_TREE_CAP2, PCT_FAST_R1_MAX (csrc/pct_internal.h)
UNDECIDED_REL = 2.0 ** -40

_OFFSETS = np.array([(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)], np.int64)     # 27 cells


def spread3(v):
    """bit i -> bit 3 i, one bit at a time"""
    v = np.asarray(v, np.uint64)
    out = np.zeros(v.shape, np.uint64)
    for i in range(BITS):
        out |= ((v >> np.uint64(i)) & np.uint64(1)) << np.uint64(3 * i)
    return out


def compact3(c):
    c = np.asarray(c, np.uint64)
    out = np.zeros(c.shape, np.uint64)
    for i in range(BITS):
        out |= ((c >> np.uint64(3 * i)) & np.uint64(1)) << np.uint64(i)
    return out.astype(np.int64)


def morton(qx, qy, qz):
    return spread3(qx) | spread3(qy) << np.uint64(1) | spread3(qz) << np.uint64(2)


def _shl(prefix, l):
    """prefix << 3 l in 64 bits; at l = 21 the only prefixes are 0 and 1, and 1 << 63 lies above every code"""
    return np.asarray(prefix, np.uint64) << np.uint64(3 * l)


def stencil_ranges(codes, l, cx, cy, cz):
    """(first, rows) of the 27 cells around cells (cx, cy, cz) of level l (arrays of one length m): two (m, 27) arrays;
    cells outside the level's grid are (0, 0)."""
    cx, cy, cz = (np.atleast_1d(np.asarray(a, np.int64)) for a in (cx, cy, cz))
    dim = 1 << (BITS - l)
    x, y, z = cx[:, None] + _OFFSETS[:, 0], cy[:, None] + _OFFSETS[:, 1], cz[:, None] + _OFFSETS[:, 2]
    inside = (x >= 0) & (x < dim) & (y >= 0) & (y < dim) & (z >= 0) & (z < dim)
    prefix = morton(np.where(inside, x, 0), np.where(inside, y, 0), np.where(inside, z, 0))
    lo = np.searchsorted(codes, _shl(prefix, l), "left")
    hi = np.searchsorted(codes, _shl(prefix + np.uint64(1), l), "left")
    return np.where(inside, lo, 0), np.where(inside, hi - lo, 0)


def knobs(k, f_min=None, items_q=None, split=None, refine=True):
    """The four switches as pct_build_tree reads them (values outside a switch's range leave its default)."""
    f = 0.45 if f_min is None or not (0.05 < f_min < 8) else f_min
    n_min = max(2, int(np.rint(f * (k + 1))))
    q = 12 if items_q is None or not (1 <= items_q <= 64) else int(items_q)
    cap = CAP_R1 if k + 1 <= R1_MAX else CAP_R2
    kernel_cap = cap
    if split is not None and 64 <= split <= cap:
        cap = int(split)
    return dict(n_min=n_min, items_q=q, cap=cap, kernel_cap=kernel_cap, refine=bool(refine))


def cube(pts, eps=0.0):
    """The cube of the float32 records: dict(o, cell, inv, root, built)."""
    p32 = np.asarray(pts).astype(np.float32)
    lo, hi = p32.min(0).astype(np.float64), p32.max(0).astype(np.float64)
    ext = float((hi - lo).max())
    if not ext > 0:
        ext = 1.0
    root = ext * (1.0 + 2.0 ** -18)
    cell = math.ldexp(root, -BITS)
    built = cell * cell > 1e-30 and root * root < 1e30 and (not eps > 0 or eps * eps > 1e-36)
    return dict(o=lo, cell=cell, inv=1.0 / cell, root=root, built=built)


def max_level(eps, cell):
    if not eps > 0:
        return BITS
    need = math.log2(eps * 1.000001 / cell)
    return 0 if need <= 0 else BITS if need >= BITS else int(math.ceil(need))


def level_by_count(codes, n_min, cap_level=BITS):
    """Per sorted row: the smallest l with >= n_min rows sharing code >> 3 l (21 if none), capped."""
    n = len(codes)
    lvl = np.full(n, BITS, np.int64)
    todo = np.ones(n, bool)
    for l in range(BITS + 1):
        key = codes >> np.uint64(3 * l)
        _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
        hit = todo & (cnt[inv.ravel()] >= n_min)
        lvl[hit] = l
        todo &= ~hit
    return np.minimum(lvl, cap_level)


def segments_of(codes, lvl):
    """(first, rows) of the maximal runs of rows with one level and one cell of that level."""
    n = len(codes)
    cellkey = codes >> (np.uint64(3) * lvl.astype(np.uint64))
    head = np.ones(n, bool)
    head[1:] = (lvl[1:] != lvl[:-1]) | (cellkey[1:] != cellkey[:-1])
    first = np.flatnonzero(head)
    return first, np.diff(np.append(first, n))


def _items(length, q):
    return (np.asarray(length) + q - 1) // q


def build(pts, k, eps=0.0, f_min=None, items_q=None, split=None, refine=True):
    """The whole build.  Returns a dict; `built` False (and nothing else but the cube) where the cube is refused."""
    kn = knobs(k, f_min, items_q, split, refine)
    cb = cube(pts, eps)
    out = dict(cb, **kn)
    if not cb["built"]:
        return out
    p32 = np.asarray(pts).astype(np.float32)
    n = len(p32)
    q = np.clip(np.floor((p32.astype(np.float64) - cb["o"]) * cb["inv"]), 0, TOP).astype(np.int64)
    code_pub = morton(q[:, 0], q[:, 1], q[:, 2])
    order = np.argsort(code_pub, kind="stable")
    codes = code_pub[order]
    ml = max_level(eps, cb["cell"])
    lvl = level_by_count(codes, kn["n_min"], ml)
    first, length = segments_of(codes, lvl)
    cap, iq = kn["cap"], kn["items_q"]
    n_seg0, n_item0 = len(first), int(_items(length, iq).sum())

    # stencil populations of the initial segments, level by level
    seg_l = lvl[first]
    fx, fy, fz = compact3(codes[first]), compact3(codes[first] >> np.uint64(1)), compact3(codes[first] >> np.uint64(2))
    pop = np.zeros(n_seg0, np.int64)
    nonempty = np.zeros(n_seg0, np.int64)
    for l in np.unique(seg_l):
        m = seg_l == l
        _, ln = stencil_ranges(codes, int(l), fx[m] >> l, fy[m] >> l, fz[m] >> l)
        pop[m], nonempty[m] = ln.sum(1), (ln > 0).sum(1)
    over = (pop > cap) & (seg_l > 0)

    # the sample behind PCT_KNN_AUTO's reading of the cloud
    hist = np.zeros(22, np.int64)
    np.add.at(hist, np.minimum(seg_l[::64], 21), length[::64])
    tot = int(hist.sum())
    lo_l, hi_l, acc = 0, 21, 0
    for l in range(22):
        acc += int(hist[l])
        if acc * 20 >= tot:
            lo_l = l
            break
    acc = 0
    for l in range(21, -1, -1):
        acc += int(hist[l])
        if acc * 20 >= tot:
            hi_l = l
            break
    spread = hi_l - lo_l if tot > 0 and hi_l > lo_l else 0
    best2 = max(int(hist[l] + hist[l + 1]) for l in range(21))
    share = best2 / tot if tot > 0 else 1.0

    # live pieces: (level, cx, cy, cz, first, rows, stencil population, non-empty ranges)
    pieces = []
    new_segs = new_items = 0
    final_lvl = lvl.copy()
    for s in range(n_seg0):
        l = int(seg_l[s])
        if not (over[s] and kn["refine"]):
            pieces.append((l, int(fx[s] >> l), int(fy[s] >> l), int(fz[s] >> l), int(first[s]), int(length[s]), int(pop[s]), int(nonempty[s])))
            continue
        stack = [(l, int(first[s]), int(length[s]))]
        while stack:
            el, ef, en = stack.pop()
            cl = el - 1
            run = codes[ef:ef + en]
            octant = (run >> np.uint64(3 * cl)) & np.uint64(7)
            bounds = ef + np.searchsorted(octant, np.arange(9, dtype=np.uint64), "left")
            live = np.flatnonzero(np.diff(bounds) > 0)
            c0 = codes[bounds[live]]
            ox, oy, oz = compact3(c0) >> cl, compact3(c0 >> np.uint64(1)) >> cl, compact3(c0 >> np.uint64(2)) >> cl
            _, ln = stencil_ranges(codes, cl, ox, oy, oz)
            for j, c in enumerate(live):
                cs, ce = int(bounds[c]), int(bounds[c + 1])
                p = int(ln[j].sum())
                if p > cap and cl > 0:
                    stack.append((cl, cs, ce - cs))
                    continue
                pieces.append((cl, int(ox[j]), int(oy[j]), int(oz[j]), cs, ce - cs, p, int((ln[j] > 0).sum())))
                new_segs += 1
                new_items += int(_items(ce - cs, iq))
                final_lvl[cs:ce] = cl
    pieces.sort(key=lambda t: t[4])
    # live items: (first row, rows, stencil population of the piece, its non-empty ranges)
    items = [(pf + i, min(iq, pn - i), pp, pr) for (_, _, _, _, pf, pn, pp, pr) in pieces for i in range(0, pn, iq)]
    out.update(n=n, order=order, codes=codes, max_level=ml, level0=lvl, level=final_lvl,
               segments0=n_seg0, items0=n_item0, over_segments=int(over.sum()), over_points=int(length[over].sum()),
               segments=n_seg0 + new_segs, items=n_item0 + new_items, hist=hist, spread=spread, share=share,
               pieces=pieces, live_items=items)
    return out


def guaranteed_r2(dim, cell, cx, cy, cz, gx, gy, gz, ring=1):
    """query_guaranteed_r2 (csrc/pct_query_plan.h) in float64, operation for operation; arrays over queries."""
    inf = np.inf
    gmin = np.full(np.shape(gx), inf)
    for c, g in ((cx, gx), (cy, gy), (cz, gz)):
        gmin = np.minimum(gmin, np.where(c - ring <= 0, inf, g + ring))
        gmin = np.minimum(gmin, np.where(c + ring >= dim - 1, inf, (1.0 - g) + ring))
    rr = gmin * cell * (1.0 - 1e-6)
    return rr * rr


def exact_walk(pts, k, eps, b, pair_budget=1 << 22):
    """k_knn_exact_tree for every sorted row of build b.  Returns dict(rounds, steps, rounds_hi, steps_hi, decided):
    rounds / steps with every undecided round taken as vouched (fewest), *_hi with it taken as not vouched (most)."""
    pts = np.asarray(pts)
    n, codes, order = b["n"], b["codes"], b["order"]
    rec = pts.astype(np.float32).astype(np.float64)[order]                       # the candidates: float32 records
    qry = pts.astype(np.float64)[order] if pts.dtype == np.float64 else rec       # float64 clouds: the native query
    fx, fy, fz = compact3(codes), compact3(codes >> np.uint64(1)), compact3(codes >> np.uint64(2))
    eps2 = eps * eps if eps > 0 else np.inf
    level = b["level"].copy()
    rounds = np.zeros(n, np.int64)
    steps = np.zeros(n, np.int64)
    rounds_lo = np.full(n, -1, np.int64)
    steps_lo = np.zeros(n, np.int64)
    active = np.arange(n)
    while len(active):
        nxt = []
        at = level[active].copy()                    # one round per pass: a row that climbs waits for the next pass
        for l in np.unique(at):
            l = int(l)
            rows = active[at == l]
            key = codes[rows] >> np.uint64(3 * l)
            # rows of one cell share the 27 ranges
            _, start = np.unique(key, return_index=True)
            cells = np.sort(start)
            groups = np.split(np.arange(len(rows)), cells[1:])
            cell_l, inv_l, dim = math.ldexp(b["cell"], l), math.ldexp(b["inv"], -l), 1 << (BITS - l)
            r0 = rows[cells]
            s_all, n_all = stencil_ranges(codes, l, fx[r0] >> l, fy[r0] >> l, fz[r0] >> l)
            for gi, g in enumerate(groups):
                rr = rows[g]
                s, ln = s_all[gi], n_all[gi]
                st = int(((ln + 63) // 64).sum())
                cand = np.concatenate([np.arange(a, a + c) for a, c in zip(s, ln) if c > 0]) if ln.sum() else np.zeros(0, np.int64)
                cpts = rec[cand]
                tau = np.full(len(rr), np.inf)
                if len(cand) >= k + 1:
                    chunk = max(1, pair_budget // len(cand))
                    for a in range(0, len(rr), chunk):
                        qq = qry[rr[a:a + chunk]]
                        dx, dy, dz = (cpts[None, :, 0] - qq[:, None, 0], cpts[None, :, 1] - qq[:, None, 1], cpts[None, :, 2] - qq[:, None, 2])
                        d2 = (dx * dx + dy * dy) + dz * dz
                        tau[a:a + chunk] = np.partition(d2, k, axis=1)[:, k]
                cx, cy, cz = int(fx[rr[0]] >> l), int(fy[rr[0]] >> l), int(fz[rr[0]] >> l)
                gx = (qry[rr, 0] - b["o"][0]) * inv_l - cx
                gy = (qry[rr, 1] - b["o"][1]) * inv_l - cy
                gz = (qry[rr, 2] - b["o"][2]) * inv_l - cz
                r2 = guaranteed_r2(dim, cell_l, cx, cy, cz, gx, gy, gz)
                m = np.minimum(tau, eps2)
                steps[rr] += st
                with np.errstate(invalid="ignore"):
                    close = np.isfinite(r2) & (np.abs(m - r2) <= UNDECIDED_REL * r2)
                stop = (m <= r2) | (l >= BITS)
                if l >= BITS:
                    close[:] = False
                # an undecided round: the fewest rounds end here (once), the most go on
                first_close = close & (rounds_lo[rr] < 0)
                rounds_lo[rr[first_close]] = rounds[rr[first_close]]
                steps_lo[rr[first_close]] = steps[rr[first_close]]
                go = close | ~stop
                level[rr[go]] += 1
                rounds[rr[go]] += 1
                nxt.append(rr[go])
        active = np.sort(np.concatenate(nxt)) if nxt else np.zeros(0, np.int64)
    decided = rounds_lo < 0
    return dict(rounds=np.where(decided, rounds, rounds_lo), steps=np.where(decided, steps, steps_lo),
                rounds_hi=rounds, steps_hi=steps, decided=decided)


def expected_counters(b, w):
    """What the statistics words must hold: the exact-only call's (candidate_steps, ring_fallbacks) as (lo, hi) pairs
    -- equal where every row is decided --, and of the normal call lds_overflows with the lower bound of redone_queries.

    lds_overflows: k_knn_pair (k + 1 <= 61, capacity PCT_TREE_CAP) and k_knn_duo (capacity PCT_TREE_CAP2) hand a live
    item over when its segment's stencil population exceeds the KERNEL's capacity (PCT_TREE_SPLIT lowers the build's cap
    only) or when more than 16 of its 27 ranges are non-empty (item_overflows, csrc/pct_knn_item.h); k_knn_fast's own
    decode reads the same two conditions.  Every row of such an item is redone; so is every decided row whose level cube
    cannot vouch for it (rounds > 0): the fast sweep proves a row from the same guarantee, rounded down."""
    kcap = b["kernel_cap"]
    handed = np.zeros(b["n"], bool)
    overflows = 0
    for first, rows, pop, ranges in b["live_items"]:
        if pop > kcap or ranges > 16:
            overflows += 1
            handed[first:first + rows] = True
    d = w["decided"]
    redone_min = int(handed.sum() + (~handed & d & (w["rounds"] > 0)).sum())
    return dict(steps=(int(w["steps"].sum()), int(w["steps_hi"].sum())),
                fallbacks=(int((w["rounds"] > 0).sum()), int((w["rounds_hi"] > 0).sum())),
                lds_overflows=overflows, redone_min=redone_min, undecided=int((~d).sum()))

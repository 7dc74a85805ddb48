"""What decides a pass of the chained sweep (csrc/pct_levels_plan.h), restated in NumPy.

Written from the rule, not from the header: float32 wherever the code computes in float, float64 where it computes in
double.  tests/test_levels_exact.py holds the header, compiled alone by the host compiler, to these functions bit for
bit; tests/test_gpu_levels_exact.py holds the kernels of csrc/pct_levels.hip to them on the device.

The rule.  A query a fast pass could not answer says why -- 1: the cells were too small for it, 2: too large -- and how
many candidates its 27-cell stencil held.  Per query the chain keeps a bracket (x, y) of log2 cell edges: x the largest
known too small, y the smallest known too large.  A failure at an edge outside the bracket says nothing new and ends the
search (the query wants the exact sweep: kWantExact); so does every other `why`.  Otherwise the bracket takes the edge
in; once both ends are known the query wants their mean, unless they are closer than 0.6 octaves (exact sweep); with one
end still open it moves by half the log2 of target / population, at least 0.75 and at most 3 octaves in the direction of
the failure.

Wanted edges are counted in 160 quarter-octave bins whose bounds are bin_lo(b) = log_edge0 - 20 + b / 4 in float32, bin
0 open below and bin 159 open above up to the exact class (w >= 0.5e30).  The next pass owns the first window of four
bins with the largest sum: [bin_lo(best), bin_lo(best + 4)), open below at best = 0, up to 0.4e30 at best = 156; its cell
edge is 2^(centre of the window).  The chain stops when no more than `enough` = max(nq / 256, 1024) queries are banded,
after 14 passes, or when the best window holds no more than enough / 8.  The closing exact pass sizes its cells for the
middle of the bin in which the running sum first reaches half of the banded queries."""
import ctypes
import ctypes.util
import decimal
import functools

import numpy as np

F = np.float32
K_BINS, K_BIN_LO, K_WINDOW = 160, F(-20.0), 4
K_WANT_EXACT = F(1.0e30)
K_STEP_MIN, K_STEP_MAX, K_BRACKET_MIN = F(0.75), F(3.0), F(0.6)
K_MAX_PASSES = 14
EXACT_FROM = F(0.5) * K_WANT_EXACT            # the exact class begins here ...
WINDOW_TOP = F(0.4) * K_WANT_EXACT            # ... the last window ends here: the strip in between belongs to no pass
CLAMP_MARGIN = 1e-4                            # float64 steps this close to a clamp are ambiguous under the log2 allowance


def _libm_exp2():
    f = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").exp2
    f.restype, f.argtypes = ctypes.c_double, [ctypes.c_double]
    return f


_exp2 = _libm_exp2()      # the edges are exp2() of the C library in the code; the rule is its float64 ARGUMENT, the function is shared


def exp2_exact(x):
    """2^x of a float64 x, correctly rounded to float64 (60 decimal digits in between): what the C library's exp2 is near."""
    with decimal.localcontext() as c:
        c.prec = 60
        return float((decimal.Decimal(float(x)) * decimal.Decimal(2).ln()).exp())


def bits(x):
    return np.asarray(x, dtype=F).view(np.uint32)


def from_bits(u):
    return np.asarray(u, dtype=np.uint32).view(F)


def enough(nq):
    return max(int(nq) // 256, 1024)


# ---- bins ------------------------------------------------------------------------------------------------------------------
def bin_lo(log_edge0, b):
    """float32 bound between bins b - 1 and b (b = 0 .. 160): (log_edge0 + -20) + 0.25 b, each operation rounded once."""
    return (F(log_edge0) + K_BIN_LO) + F(0.25) * np.asarray(b, dtype=F)


def bounds(log_edge0):
    return bin_lo(log_edge0, np.arange(K_BINS + 1))


def bin_of(w, log_edge0):
    """-1: NaN (answered); 160: the exact class; else the bin whose [bin_lo(b), bin_lo(b + 1)) holds w, clamped to 0 .. 159."""
    w = np.asarray(w, dtype=F)
    edges = bounds(log_edge0)
    assert (np.diff(edges) > 0).all(), "the bounds are strictly increasing for every log_edge0 a cloud can have"
    with np.errstate(invalid="ignore"):
        b = np.clip(np.searchsorted(edges, w, side="right") - 1, 0, K_BINS - 1)
        b = np.where(w >= EXACT_FROM, K_BINS, b)
    return np.where(np.isnan(w), -1, b).astype(np.int64)


def histogram(w, log_edge0):
    """(hist[160], exact) of k_band_hist."""
    b = bin_of(w, log_edge0)
    return np.bincount(b[(b >= 0) & (b < K_BINS)], minlength=K_BINS).astype(np.uint32), int((b == K_BINS).sum())


def window(log_edge0, best):
    """[lo, hi) of the pass whose window starts at bin `best`."""
    lo = F(-np.inf) if best == 0 else F(bin_lo(log_edge0, best))
    hi = WINDOW_TOP if best + K_WINDOW >= K_BINS else F(bin_lo(log_edge0, best + K_WINDOW))
    return lo, hi


def members(w, lo, hi):
    w = np.asarray(w, dtype=F)
    with np.errstate(invalid="ignore"):
        return (w >= lo) & (w < hi)            # NaN belongs to no window


# ---- the wanted edge ---------------------------------------------------------------------------------------------------------
def population_ratio(pop, target):
    """float32 argument of the logarithm: max(target / max(pop, 0.5), 1e-6)."""
    pop = np.asarray(pop, dtype=F)
    return np.maximum(F(target) / np.maximum(pop, F(0.5)), F(1e-6))


def step64(pop, target):
    """The population step in float64 (of the float32 ratio): what decides whether a case is ambiguous near a clamp."""
    return 0.5 * np.log2(population_ratio(pop, target).astype(np.float64))


def classify(why, pop, log_edge, target, bx, by, log2_shift=0):
    """Arrays in, (want, bx, by, took_log) float32 out.  log2_shift = -1, 0, +1: the float32 logarithm taken as the
    neighbour below, the nearest, the neighbour above of the float64 logarithm rounded to float32 -- everything after it
    (halving, clamp, addition) is float32 arithmetic on that value.  took_log: the rows whose want went through it."""
    why, pop, le, bx, by = np.broadcast_arrays(np.asarray(why), np.asarray(pop, dtype=F), np.asarray(log_edge, dtype=F),
                                               np.asarray(bx, dtype=F), np.asarray(by, dtype=F))
    small, large = why == 1, why == 2
    news = (small & (le > bx)) | (large & (le < by))
    nx = np.where(small, np.maximum(bx, le), bx).astype(F)
    ny = np.where(large, np.minimum(by, le), by).astype(F)
    closed = (nx > F(-np.inf)) & (ny < F(np.inf))
    with np.errstate(invalid="ignore", over="ignore"):
        narrow = (ny - nx).astype(F) < K_BRACKET_MIN
        mean = (F(0.5) * (nx + ny).astype(F)).astype(F)
        lg = np.log2(population_ratio(pop, target).astype(np.float64)).astype(F)
        if log2_shift:
            lg = np.nextafter(lg, F(np.inf) if log2_shift > 0 else F(-np.inf)).astype(F)
        step = (F(0.5) * lg).astype(F)
        up = (le + np.minimum(np.maximum(step, K_STEP_MIN), K_STEP_MAX)).astype(F)
        down = (le + np.maximum(np.minimum(step, -K_STEP_MIN), -K_STEP_MAX)).astype(F)
    want = np.full(why.shape, K_WANT_EXACT, dtype=F)
    bisect = news & closed
    want = np.where(bisect & ~narrow, mean, want)
    took_log = news & ~closed
    want = np.where(took_log, np.where(small, up, down), want).astype(F)
    return want, nx, ny, took_log


def near_a_clamp(pop, target):
    s = np.abs(step64(pop, target))
    return (np.abs(s - float(K_STEP_MIN)) < CLAMP_MARGIN) | (np.abs(s - float(K_STEP_MAX)) < CLAMP_MARGIN)


# ---- the next pass -------------------------------------------------------------------------------------------------------------
def next_pass(hist, exact, passes, nq, log_edge0):
    hist = [int(h) for h in hist]
    assert len(hist) == K_BINS
    banded = sum(hist)
    sums = [sum(hist[b:b + K_WINDOW]) for b in range(K_BINS - K_WINDOW + 1)]
    best = sums.index(max(sums))                   # the lowest start among equals
    lo, hi = window(log_edge0, best)
    e = enough(nq)
    centre = float(F(log_edge0)) + float(K_BIN_LO) + 0.25 * (best + 2)
    return {"pending": banded + int(exact), "banded": banded, "best": best, "best_cnt": sums[best],
            "stop": banded <= e or passes >= K_MAX_PASSES or sums[best] <= e // 8,
            "lo": lo, "hi": hi, "edge": _exp2(centre)}


def closing_edge(hist, log_edge0):
    hist = [int(h) for h in hist]
    banded = sum(hist)
    if banded == 0:
        return _exp2(float(F(log_edge0)))
    acc = 0
    for b, h in enumerate(hist):
        acc += h
        if 2 * acc >= banded:
            return _exp2(float(F(log_edge0)) + float(K_BIN_LO) + 0.25 * (b + 0.5))
    raise AssertionError("unreachable: the running sum reaches the total")


# ---- the merge -------------------------------------------------------------------------------------------------------------------
def merge_rows(pub, owned_pos, q_begin, nbr_pos, nbr_dist, nbr_cnt, row_done, k, pub_pos, pub_dist, pub_cnt, want):
    """k_merge_rows: copies of (pub_pos, pub_dist, pub_cnt, want) with the answered rows merged in."""
    pub = np.asarray(pub)
    pp, pd, want = pub_pos.copy(), pub_dist.copy(), want.copy()
    pc = None if pub_cnt is None else pub_cnt.copy()
    for r in np.flatnonzero(np.asarray(row_done) != 0):
        me = int(pub[owned_pos[r]])
        pos = nbr_pos[r, :k]
        pp[me - q_begin, :k] = np.where(pos < 0, -1, pub[np.maximum(pos, 0)])
        pd[me - q_begin, :k] = nbr_dist[r, :k]
        if pc is not None:
            pc[me - q_begin] = k if nbr_cnt is None else nbr_cnt[r]
        want[me] = np.nan
    return pp, pd, pc, want


# ---- cases shared by the CPU and the GPU test ------------------------------------------------------------------------------------
# first-pass log2 edges: values at which log_edge0 - 20 + b / 4 rounds (log2 of 0.0371, 1/3, 1e-20, 0.7, 1234.5) and dyadic ones
LOG_EDGE0 = [F(np.log2(0.0371)), F(np.log2(1.0 / 3.0)), F(np.log2(1e-20)), F(np.log2(0.7)), F(np.log2(1234.5)),
             F(0.0), F(-5.0), F(-4.75), F(3.5), F(-0.125)]
# values no pass can produce (classify adds a bounded step to a finite log2 edge or halves a finite sum): far outside both
# ends, the strip [0.4e30, 0.5e30) that the last bin counts and no window owns, the exact class, infinities, NaN
FAR_VALUES = [F(-3.0e38), F(-1.0e6), F(-200.0), F(200.0), F(1.0e6), F(1.0e29), np.nextafter(WINDOW_TOP, F(0)), WINDOW_TOP,
              np.nextafter(WINDOW_TOP, F(np.inf)), F(0.45e30), np.nextafter(EXACT_FROM, F(0)), EXACT_FROM, np.nextafter(EXACT_FROM, F(np.inf)),
              K_WANT_EXACT, F(3.0e38), F(-np.inf), F(np.inf), F(np.nan)]


def boundary_values(log_edge0):
    """Every bound with its float32 neighbour on each side, then FAR_VALUES."""
    e = bounds(log_edge0)
    near = np.stack([np.nextafter(e, F(-np.inf)), e, np.nextafter(e, F(np.inf))], axis=1).ravel()
    return np.concatenate([near, np.array(FAR_VALUES, dtype=F)]).astype(F)


def reachable(w):
    """Wanted edges a pass can produce lie below WINDOW_TOP or are kWantExact itself (NaN: answered)."""
    w = np.asarray(w, dtype=F)
    with np.errstate(invalid="ignore"):
        return np.isnan(w) | (np.isfinite(w) & (w < WINDOW_TOP)) | (w == K_WANT_EXACT)


CLASSIFY_K = 30
CLASSIFY_TARGETS = [F(11.0 * 1.0 * (CLASSIFY_K + 1)), F(7.5), F(4.0e6)]


def classify_brackets():
    inf = F(np.inf)
    out = [(-inf, inf), (F(-2.25), inf), (F(0.0), inf), (-inf, F(1.5)), (-inf, F(0.0))]
    widths = [F(0.59), np.nextafter(K_BRACKET_MIN, F(0)), K_BRACKET_MIN, np.nextafter(K_BRACKET_MIN, F(1)), F(0.61), F(2.0)]
    for w in widths:
        # the width itself, and brackets that a failure at log_edge = 0 narrows to exactly that width from either side
        out += [(F(0.0), w), (F(-1.0), w), (-w, F(0.0)), (-w, F(1.0)), (F(-2.25), F(F(-2.25) + w))]
    out += [(F(1.0), F(-1.0)), (F(0.5), F(0.0)), (F(0.0), F(0.0))]           # inverted, and empty
    return out


@functools.lru_cache(maxsize=None)
def classify_cases(n_random=3000, seed=7):
    """The product why x pop x bracket x log_edge x target, then random populations with an open bracket (the logarithm).
    Columns: why, pop (int), log_edge, target, bx, by.  Cases whose float64 step lies within CLAMP_MARGIN of a clamp are
    left out; returns (cases, number generated, number left out)."""
    pops = [0, 1, CLASSIFY_K, None, (1 << 29) - 1]                         # None: the target itself
    rows = []
    for target in CLASSIFY_TARGETS:
        for bx, by in classify_brackets():
            lo = bx if np.isfinite(bx) else (by if np.isfinite(by) else F(0.0))
            hi = by if np.isfinite(by) else (bx if np.isfinite(bx) else F(0.0))
            a, b = min(lo, hi), max(lo, hi)
            edges = sorted({float(F(a - F(1.0))), float(a), float(F(F(0.5) * (a + b))), float(b), float(F(b + F(1.0))), 0.0, -3.3125})
            for why in range(8):
                for pop in pops:
                    p = int(min(max(round(float(target)), 0), (1 << 29) - 1)) if pop is None else pop
                    rows += [(why, p, le, float(target), float(bx), float(by)) for le in edges]
    rng = np.random.default_rng(seed)
    inf = float(np.inf)
    for i in range(n_random):
        pop = int(2.0 ** rng.uniform(0, 29))
        target = float(F(2.0 ** rng.uniform(3, 12)))
        le = float(F(rng.uniform(-12, 4)))
        why = 1 + (i & 1)
        rows.append((why, pop, le, target, -inf, inf) if i % 3 else (why, pop, le, target, *((le - 1.0, inf) if why == 1 else (-inf, le + 1.0))))
    # each clamp driven from far beyond it, in both directions
    for why in (1, 2):
        rows += [(why, 1, 0.25, 1.0e9, -inf, inf), (why, (1 << 29) - 1, 0.25, 1.0, -inf, inf), (why, 1000, 0.25, 1000.0, -inf, inf),
                 (why, 1000, 0.25, 1001.0, -inf, inf), (why, 1001, 0.25, 1000.0, -inf, inf)]
    cols = list(zip(*rows))
    c = {"why": np.array(cols[0], dtype=np.int64), "pop": np.array(cols[1], dtype=np.int64), "log_edge": np.array(cols[2], dtype=F),
         "target": np.array(cols[3], dtype=F), "bx": np.array(cols[4], dtype=F), "by": np.array(cols[5], dtype=F)}
    took_log = classify(c["why"], c["pop"], c["log_edge"], c["target"], c["bx"], c["by"])[3]
    drop = took_log & near_a_clamp(c["pop"], c["target"])
    kept = {k: v[~drop] for k, v in c.items()}
    for v in kept.values():
        v.setflags(write=False)                    # (computed once, shared)
    return kept, len(drop), int(drop.sum())


def classify_rows(log_edge, target):
    """The cases above as the rows of ONE pass (k_classify takes the pass's log2 edge and the target once per launch):
    every case's bracket is moved so that it lies about `log_edge` as it lay about the case's own edge, the populations
    are kept, the target is the pass's.  Returns (rows: why, pop, bx, by; number generated; number left out near a clamp)."""
    c, _, _ = classify_cases()
    L = F(log_edge)
    with np.errstate(invalid="ignore"):
        bx = ((c["bx"] - c["log_edge"]).astype(F) + L).astype(F)
        by = ((c["by"] - c["log_edge"]).astype(F) + L).astype(F)
    rows = {"why": c["why"], "pop": c["pop"], "bx": bx, "by": by}
    took_log = classify(rows["why"], rows["pop"], L, target, bx, by)[3]
    drop = took_log & near_a_clamp(rows["pop"], target)
    return {k: v[~drop] for k, v in rows.items()}, len(drop), int(drop.sum())

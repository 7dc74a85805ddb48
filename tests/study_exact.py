"""The neighbour study's K(n) table and bisection, restated  --  TEST INFRASTRUCTURE ONLY (CPU, no GPU, no import of the package).

explicit_quadratic_neighbor_study (pct:732-800) asks, per sampled point and neighbour count n, for the Gaussian curvature of
"the point itself + its n nearest" (pct:759-761) and bisects on |K(n + 1) - K(n)| < tol (pct:772-789).  The package
evaluates every K(n) of a sample in one call (pct_neighbor_study_curvatures: k_prefix_rows builds the rows from the resident
neighbour table, the fit kernel solves them with per-row counts) and bisects on the host.  The contract, with nothing left open:

* ``table``    row (i, n) = [i] + the first n entries of i's neighbour row.  The neighbour row is ``wide_exact.ranked``'s:
               float32-rounded candidates, native query, order by (d2, public index), element 0 dropped -- the contract
               the device tables are already pinned to (tests/test_gpu_wide_rows.py).  Among coinciding points the row
               therefore starts with the sample and may contain the sample again in place of its twin: coordinates decide,
               not indices.  The fit is ``oracle.curvature_loop`` of that row with query i (centring in the cloud's
               dtype, pct:761); K comes back as float32.
* ``bisect``   pct:772-789 on one row of the table, in the reference's own arithmetic: float32 K, a float32 difference, a
               comparison with tol as NumPy makes it (a Python float is a weak scalar: it is rounded to float32).  Returns
               the converged count and the (mid, |dK|) pairs it looked at.
* ``bars``     per entry, the larger of the project's contract -- 1e-5 max(|ref|, 1e-2 max|ref| of the column), the bar of
               ``fit_exact.foreign_bars`` -- and ``fit_exact.R_SPREAD`` x the reference's own spread over permuted,
               mathematically equivalent rows (``fit_exact.reference_with_spread``: the permutations keep the first and the
               last entry in place, which is all the orientation test reads).  Entries with n + 1 = 2 carry no bar (inf):
               the covariance of two points has a two-dimensional null space and the reference's normal is LAPACK's pick in
               it.  Entries with n + 1 = 3 are compared as K, which is even under the flip that the orientation test
               -- rounding noise on three points -- decides; their exact K is 0, so their bar is ``special_bar``'s bound
               on rounding noise, not a share of the reference's noise.  ``special_bar`` applies the same two rules to
               any row whose points are flat or whose normal is not determined.
* ``stable``   a sample is comparable when every |dK| its bisection looked at is further than 4 x the bar from tol, the bar
               being the larger one of the two entries in the difference: each of the two values may be off by one bar, so
               the difference by two, and 4 leaves a margin of 2.  At most ``CAP`` = 10 % of a case's samples may be left
               out; tests/test_study_exact.py asserts that every case of the suite stays under it for the reference alone.

Cost: one ranking per cloud, one reference fit per entry and six more for its spread, 0.3 ms each: 64 samples x 98 counts
take 13 s.  ``Study`` therefore keeps a cloud's tables for a whole test module, and measures the spread of the entries a
bisection looked at alone where only decisions are compared.
"""
import numpy as np

import fit_exact as fe
import pct_oracle as oracle
import wide_exact as we

CAP = 0.10            # share of a case's samples that may be left out as undecidable
MARGIN = 4.0          # distance of a decision from tol, in bars (see ``stable``)

SEED_STUDY = 5        # the golden's cloud: wide_exact.torus_random(3000, seed=5)
GOLDEN_CASES = ((0.03, 3, 99), (0.1, 3, 99), (0.03, 10, 40))      # (tol, lower, upper) of g13 on the float32 torus
F64_SCALE, F64_OFFSET = 0.2, 40.0                                 # the float64 copy: float32 rounding is 1.9e-6 of 0.02 spacings


def torus32():
    return we.torus_random(3000, SEED_STUDY)


def torus64():
    return we.torus_random(3000, SEED_STUDY, np.float64) * F64_SCALE + F64_OFFSET


def f64_tol(tol):
    """K is an inverse area: the cloud scaled by s has K / s^2.  The tolerance of the scaled cloud that asks the same
    question as ``tol`` on the unit torus."""
    return tol / (F64_SCALE * F64_SCALE)


# ======================================================================================================================
# the table
# ======================================================================================================================
def neighbour_rows(points, rows, n_hi, ranking=None):
    """(m, n_hi) int32: the first n_hi entries of every sample's neighbour row (element 0 of the order dropped)."""
    rows = np.asarray(rows, np.int64)
    if ranking is None:
        ranking = we.ranked(points, rows, width=n_hi + 1)
        order = ranking[0]
    else:
        order = ranking[0][rows]                       # a ranking of the whole cloud
    assert order.shape[1] >= n_hi + 1, "the ranking is shorter than the longest row"
    return np.ascontiguousarray(order[:, 1:n_hi + 1])


def prefix_rows(nbr, rows, n):
    """(m, n + 1): [sample] + its first n neighbours."""
    return np.concatenate([np.asarray(rows, np.int32)[:, None], nbr[:, :n]], 1)


def table(points, rows, n_lo, n_hi, ranking=None, spread=False):
    """K (m, n_hi - n_lo + 1) float32, column j for n = n_lo + j.  spread=True: also the reference's own spread (float64).
    Repeated samples are computed once."""
    points = np.asarray(points)
    rows = np.asarray(rows, np.int64)
    assert 1 <= n_lo <= n_hi
    uniq, back = np.unique(rows, return_inverse=True)
    nbr = neighbour_rows(points, uniq, n_hi, ranking)
    K = np.empty((len(uniq), n_hi - n_lo + 1), np.float32)
    S = np.zeros(K.shape, np.float64)
    for j, n in enumerate(range(n_lo, n_hi + 1)):
        idx = prefix_rows(nbr, uniq, n)
        if spread:
            k, _, s, _ = fe.reference_with_spread(points, idx, uniq)
            K[:, j], S[:, j] = k.astype(np.float32), s
        else:
            K[:, j] = oracle.curvature_loop(points, idx, uniq)[1]
    return (K[back], S[back]) if spread else K[back]


# ======================================================================================================================
# the bisection
# ======================================================================================================================
def bisect(row, tol, lower, upper):
    """pct:772-789.  ``row``: K(n) for n = lower ... upper + 1, float32.  Returns (converged count, [(mid, |dK|), ...])."""
    row = np.asarray(row, np.float32)
    assert len(row) >= upper - lower + 2
    base = lower
    best, seen = None, []
    while lower <= upper:
        mid = (lower + upper) // 2
        d = abs(row[mid + 1 - base] - row[mid - base])             # np.float32 - np.float32
        seen.append((mid, d))
        if d < tol:                                                # tol: a Python float, weak -- compared in float32
            best, upper = mid, mid - 1
        else:
            lower = mid + 1
    return (upper if best is None else best), seen


def counts(K, tol, lower, upper, n_lo=None):
    """Bisection of every row of a table whose column 0 is n = n_lo (default: lower).  (counts (m,), decisions per row)."""
    off = 0 if n_lo is None else lower - n_lo
    assert off >= 0
    out = [bisect(r[off:], tol, lower, upper) for r in np.asarray(K)]
    return np.array([c for c, _ in out], np.int64), [s for _, s in out]


def result(conv):
    """pct:797-800."""
    return 0 if len(conv) == 0 else int(np.mean(conv)) + 1


# ======================================================================================================================
# the bars
# ======================================================================================================================
C_NOISE = 64.0        # roundings between the centred points and the rotated z of a flat row (see ``special_bar``)
GAP_MIN = 1e-9        # (l1 - l0) / l2 below which the normal is LAPACK's pick in a degenerate eigenspace
FLAT_MAX = 1e-13      # l0 / l2 below which a row is flat: the rounding of a float64 covariance of <= 512 points


def special_bar(points, row, query):
    """NaN for an ordinary row; otherwise the bar that replaces the contract, from the eigenvalues l0 <= l1 <= l2 of the
    row's covariance (float64, np.cov as pct:277):

    inf   (no bar) two points, coinciding or collinear points, or l1 - l0 <= GAP_MIN l2: the normal is the reference's pick
          in an eigenspace of dimension two or three.  n + 1 = 2 is always this; complete shells of a cubic lattice are too.
    flat  l0 <= FLAT_MAX l2: the points lie in a plane -- any three do, n + 1 = 3 is always this.  Rotated onto the plane
          every z is 0, the least-squares solution of X c = 0 is c = 0 and K is EXACTLY 0.  What the reference returns
          (1e-28 ... 1e-39 on the torus) is the square of rounding noise, and 1e-5 of it is no bar.  What a careful float64
          implementation can be held to: the normal is good to eps * l2 / l1; the rotated z are therefore at most
          C_NOISE eps R l2 / l1 in size (R the largest distance from the query); the coefficients are at most |z|_2 / s_min
          (s_min the smallest singular value of the design matrix that gelsd keeps) and |K| = |4AB - C^2| <= 5 |c|^2.
          C_NOISE = 64 stands for the few dozen roundings of covariance, eigenvector and Rodrigues rotation;
          tests/test_study_exact.py asserts that the reference's own noise stays below this bar."""
    points = np.asarray(points)
    q = (points[np.asarray(row)] - points[query]).astype(np.float64)
    if len(q) < 3:
        return np.inf
    lam = np.linalg.eigvalsh(np.cov(q, rowvar=False))
    if not lam[2] > 0 or lam[1] - lam[0] <= GAP_MIN * lam[2]:
        return np.inf
    if lam[0] > FLAT_MAX * lam[2]:
        return np.nan
    sv = np.linalg.svd(fe.design(oracle.plane_align(q))[0].astype(np.float64), compute_uv=False)
    s_min = sv[sv > fe.gelsd_cut(len(q)) * sv[0]].min()
    z = C_NOISE * fe.EPS64 * np.sqrt((q * q).sum(1).max()) * lam[2] / lam[1]
    return 5.0 * (np.sqrt(len(q)) * z / s_min) ** 2


def bars(ref, spread, n_lo=3, special=None):
    """(m, nn) float64: per entry max(contract, R_SPREAD x spread).  The contract's floor is per column: every entry of a
    column is a fit of the same size.  ``special`` (m, nn): what ``special_bar`` says of every entry; without it only the
    rule that needs no coordinates is applied (n + 1 = 2: no bar)."""
    ref = np.asarray(ref, np.float64)
    out = np.empty(ref.shape)
    for j in range(ref.shape[1]):
        contract, own, _ = fe.foreign_bars(ref[:, j], np.asarray(spread)[:, j], np.zeros(len(ref)))
        out[:, j] = np.maximum(contract, own)
        if n_lo + j + 1 == 2:
            out[:, j] = np.inf
    if special is not None:
        out = np.where(np.isnan(special), out, np.maximum(out, special))
    return out


def check_values(got, ref, bar):
    """(ok (m, nn) bool, worst error as a fraction of its bar over the entries that carry one)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    has = np.isfinite(bar)
    ok = ~has | (err <= bar)                           # (NaN fails: the comparison is False)
    frac = float((err[has] / bar[has]).max()) if has.any() else 0.0
    return ok, frac


def stable(decisions, tol, bar, n_lo=3):
    """decisions: per sample the (mid, |dK|) list of ``bisect``; bar: (m, nn) with column 0 at n = n_lo.
    Returns a bool per sample: True where every decision is further than MARGIN bars from tol."""
    tol32 = float(np.float32(tol))
    out = np.ones(len(decisions), bool)
    for s, seen in enumerate(decisions):
        for mid, d in seen:
            b = max(bar[s, mid - n_lo], bar[s, mid + 1 - n_lo])
            if not abs(float(d) - tol32) > MARGIN * b:
                out[s] = False
    return out


def under_cap(comparable):
    return (~np.asarray(comparable)).sum() <= CAP * len(comparable)


# ======================================================================================================================
# one cloud's reference, computed once
# ======================================================================================================================
def spread_at(points, nbr, uniq, n, which):
    """The reference's own spread of K for count n on the samples uniq[which] (fit_exact.reference_with_spread)."""
    idx = prefix_rows(nbr[which], uniq[which], n)
    return fe.reference_with_spread(points, idx, uniq[which])[2]


class Study:
    """Reference table, spread and bars of (points, samples, n_lo ... n_hi); read-only for its users.

    full=True measures the spread of every entry (six reference loops per entry): what a value check of a whole table
    needs.  full=False measures it on demand, for the entries a bisection looked at: what a check of decisions needs."""

    def __init__(self, points, samples, n_lo, n_hi, ranking=None, full=True):
        self.points, self.samples, self.n_lo, self.n_hi = np.asarray(points), np.asarray(samples, np.int64), n_lo, n_hi
        self.uniq, self.back = np.unique(self.samples, return_inverse=True)
        self.nbr = neighbour_rows(self.points, self.uniq, n_hi, ranking)
        nn = n_hi - n_lo + 1
        self._Ku = np.empty((len(self.uniq), nn), np.float32)
        self._Su = np.full((len(self.uniq), nn), np.nan)
        for j in range(nn):
            self._Ku[:, j] = oracle.curvature_loop(self.points, prefix_rows(self.nbr, self.uniq, n_lo + j), self.uniq)[1]
        self.K = self._Ku[self.back]
        self.K.setflags(write=False)
        sp = np.array([[special_bar(self.points, np.concatenate([[i], r[:n]]), i) for n in range(n_lo, n_hi + 1)]
                       for r, i in zip(self.nbr, self.uniq)])
        self.special = sp[self.back]
        # rows whose points all coincide with the sample: every centred coordinate is an exact zero, nothing is ever
        # rounded, and K is 0 without noise (the reference returns 0.0)
        same = (self.points[self.nbr] == self.points[self.uniq][:, None, :]).all(2)
        self.zero = np.logical_and.accumulate(same, 1)[:, n_lo - 1:n_hi][self.back]
        if full:
            self.measure(np.ones(self._Ku.shape, bool))

    def measure(self, want):
        """Spread of the entries want[(unique sample, column)] that have none yet."""
        todo = want & np.isnan(self._Su)
        for j in np.flatnonzero(todo.any(0)):
            which = np.flatnonzero(todo[:, j])
            self._Su[which, j] = spread_at(self.points, self.nbr, self.uniq, self.n_lo + j, which)

    @property
    def spread(self):
        return self._Su[self.back]

    @property
    def bar(self):
        """NaN where the spread has not been measured: a comparison with it fails."""
        return bars(self.K, self.spread, self.n_lo, self.special)

    def decide(self, tol, lower, upper, only=None):
        """(counts, comparable, decisions) of the reference table.  only: the samples (indices into ``samples``) to judge --
        the spread is measured for what their bisections looked at, every other sample reads not comparable."""
        c, seen = counts(self.K, tol, lower, upper, self.n_lo)
        judged = np.arange(len(seen)) if only is None else np.arange(len(seen))[only]
        want = np.zeros(self._Ku.shape, bool)
        for s in judged:
            for mid, _ in seen[s]:
                want[self.back[s], mid - self.n_lo: mid - self.n_lo + 2] = True
        self.measure(want)
        comparable = np.zeros(len(seen), bool)
        comparable[judged] = stable([seen[s] for s in judged], tol, self.bar[judged], self.n_lo)
        return c, comparable, seen

    def compare(self, got, tol=None, lower=None, upper=None):
        """Value check of a device table (needs full=True) and, with tol, the decision check.  A dict of findings."""
        got = np.asarray(got)
        assert got.shape == self.K.shape and got.dtype == np.float32, (got.shape, got.dtype, self.K.shape)
        bar = self.bar
        assert not np.isnan(bar).any(), "value checks need the spread of every entry"
        ok, frac = check_values(got, self.K, bar)
        out = dict(values_ok=bool(ok.all()), worst=frac, bad=np.argwhere(~ok)[:6].tolist(), left_out=0.0, counts_ok=True)
        if tol is not None:
            want, comparable, _ = self.decide(tol, lower, upper)
            have, _ = counts(got, tol, lower, upper, self.n_lo)
            out["left_out"] = float((~comparable).mean())
            out["counts_ok"] = bool((have[comparable] == want[comparable]).all()) and bool(under_cap(comparable))
            out["wrong"] = np.flatnonzero(comparable & (have != want))[:6].tolist()
        out["ok"] = out["values_ok"] and out["counts_ok"]
        return out


_MEMO = {}


def cached(key, make):
    """One Study per key and process: the CPU tests of two modules share the golden's tables."""
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


# ======================================================================================================================
# the cases of tests/test_gpu_study.py (tests/test_study_exact.py holds each of them to the cap on the CPU)
# ======================================================================================================================
def torus_pairs():
    """The golden's torus with 60 of its points present twice: the copies are appended and the whole is shuffled, so for
    about half of the pairs the copy has the smaller index.  Returns (points float32, rows whose twin has the SMALLER index):
    element 0 of such a row's order is the twin, the neighbour row holds the sample itself in its place."""
    rng = np.random.default_rng(SEED_STUDY + 100)
    base = torus32()
    pts = np.vstack([base, base[rng.choice(len(base), 60, replace=False)]])
    pts = pts[rng.permutation(len(pts))]
    first = {}
    later = []
    for i, p in enumerate(map(bytes, pts)):
        if p in first:
            later.append(i)
        first.setdefault(p, i)
    return pts, np.array(later, np.int64)


def _lattice_case():
    pts = we.lattice()
    rows = np.random.default_rng(71).choice(len(pts), 12, replace=False)
    return pts, rows


def _twins_case():
    pts = we.twins()
    copies = we.twin_rows(pts)
    others = np.setdiff1d(np.arange(len(pts)), copies)
    return pts, np.concatenate([copies[[1, 7, 300, 599]], others[[3, 500, 1200, 1799]]])


def _pairs_case():
    pts, later = torus_pairs()
    return pts, later[:16]


WIDE_KS = (127, 128, 255, 256, 511)
# name: (cloud and samples, n_lo, n_hi, the bisections (tol, lower, upper) decided on it)
CASES = {
    "kinds": (lambda: (we.torus(), np.random.default_rng(61).choice(6000, 64, replace=False)), 3, 100, GOLDEN_CASES),
    "wide": (lambda: (we.torus(), np.random.default_rng(62).choice(6000, 6, replace=False)), 3, 511,
             ((0.03, 3, 126), (0.01, 3, 254), (0.003, 3, 510))),
    "lattice": (_lattice_case, 3, 40, ()),
    "twins": (_twins_case, 3, 40, ()),
    "pairs": (_pairs_case, 3, 60, ((0.03, 3, 59), (0.1, 3, 59))),
}


def case(name, full=True):
    make, n_lo, n_hi, decisions = CASES[name]
    pts, rows = make()
    return Study(pts, rows, n_lo, n_hi, full=full), decisions


# the (case of g13, whole-sample seeds) that tests/test_gpu_study.py compares through the class, per cloud: the unscaled
# first case on the float32 torus, its scaled twin on the float64 copy
WHOLE_CASES = {"32": 0, "64": 3}

// The pure rules of pct_query_ball (pct_api.hip, pct_ball.hip): which path answers a radius query, how wide a cube of
// cells a query of radius r must search, and when a query streams the whole cell-sorted cloud instead of walking the
// runs of its cube.  Nothing here knows a handle or a device; the ring and the streaming rule are also what the kernels
// evaluate (QP_HD) -- tests/test_ball_plan.py compiles this header alone with the host compiler.
#pragma once

#include "pct_query_plan.h"

// ---- the route -----------------------------------------------------------------------------------------------------------
// The states and the fall-backs are query_route's: the cell list answers where PCT_QUERY_GRID would use it (resident, or
// built by the call), the exhaustive path wherever that rule falls back (hierarchical table in place, owned range, slab,
// results in cell order without their list).  PCT_QUERY_AUTO keeps query_route's two floors (kQueryAutoMinM queries,
// kQueryAutoMinN points).  Above them the k-NN pair-count crossover does not apply: a ball query through the cell list
// reads the candidates of a cube sized by r, the exhaustive path reads all n points per query whatever r is, and the
// k-NN sweeps' running list -- what made the exhaustive k-NN path cheap per candidate -- has no counterpart here.
// kBallAutoCrossover is the pair count m n from which AUTO takes the cell list.  It is measured (tools/query_probe.py ball
// on one MI355X, the table in DESIGN 4.3f): random torus, n in {65 536, 1 M} x m in {1024 .. 1 M}, rows of ~9 .. ~320
// entries, wall time of the whole call with the rows' download.  The cell list -- resident, and built by the call -- won
// on EVERY measured pair, by 1.2x (rows of ~320 at n = 65 536) to 600x (n = m = 1 M); 2^26 is the smallest m n that was
// measured (n = 65 536, m = 1024: 0.20 | 0.28 ms against 0.41 ms).  Below it nothing was measured, so AUTO stays where
// it was.
constexpr int64_t kBallAutoCrossover = (int64_t)1 << 26;

inline bool ball_route(int32_t algo, int64_t n, int64_t m, const QueryState& s, QueryRoute* route) {
    *route = QueryRoute::Sweep;
    if (algo != PCT_QUERY_AUTO && algo != PCT_QUERY_SWEEP && algo != PCT_QUERY_GRID) return false;
    if (algo == PCT_QUERY_SWEEP) return true;
    if (algo == PCT_QUERY_AUTO) {
        if (m < kQueryAutoMinM || n < kQueryAutoMinN) return true;
        if (!query_pairs_reach(m, n, kBallAutoCrossover)) return true;
    }
    return query_route(PCT_QUERY_GRID, n, m, 1, s, route);
}

// ---- the cube a radius needs ---------------------------------------------------------------------------------------------
// r2 = r * r, the product taken in fp64 by the caller (a negative r has become |r|^2, an infinite one +inf, a NaN stays
// a NaN).  Returns the smallest ring >= 1 with r2 <= query_guaranteed_r2(..., ring) for a finite r2: every point filed outside the cube
// of that ring is farther than r, so the cube holds every member of the ball.  -1 for a NaN: the membership test
// d2 <= NaN keeps nothing, nothing is searched.
// The search is a bisection over [1, max(nx, ny, nz) - 1] (at least 1): query_guaranteed_r2 never decreases with the ring
// (every finite term grows with it and turns +inf for good once the cube reaches that face), and at the upper end the
// cube covers the grid from any cell, where it is +inf and any r2 -- +inf included -- is vouched for.  No double is ever
// converted to an int: r = inf, 1e300 or NaN cannot reach an undefined conversion.
// Ring 0 (the query's cell alone) is never returned: the shrink by 1e-6 that covers the two roundings of a cell
// coordinate is relative, and only from ring 1 on is the guaranteed distance at least one cell.
QP_HD inline int ball_ring(int nx, int ny, int nz, double cell, int cx, int cy, int cz, double gx, double gy, double gz, double r2) {
    if (!(r2 == r2)) return -1;
    int hi = nx > ny ? nx : ny;
    hi = (hi > nz ? hi : nz) - 1;
    if (hi < 1) hi = 1;
    // r*r = +inf (r = inf, or |r| past 1.3e154) keeps every point whose d2 is +inf too -- and around a query at 1e300
    // the guarantee of a small cube overflows to +inf as well, where the comparison below would take that cube: an
    // infinite r2 is answered by the whole grid, whatever the guarantee says.  (A finite r2 under an overflowed
    // guarantee is decided rightly: the points outside the cube are farther than 1e154, their d2 is +inf > r2.)
    if (r2 == (double)INFINITY) return hi;
    int lo = 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (r2 <= query_guaranteed_r2(nx, ny, nz, cell, cx, cy, cz, gx, gy, gz, mid)) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// the cube of `ring` around (cx, cy, cz) covers the grid: nothing lies outside it
QP_HD inline bool ball_cube_covers(int nx, int ny, int nz, int cx, int cy, int cz, int ring) {
    return cx - ring <= 0 && cx + ring >= nx - 1 && cy - ring <= 0 && cy + ring >= ny - 1 && cz - ring <= 0 && cz + ring >= nz - 1;
}

// (y, z) rows of the cube clipped to the grid
QP_HD inline int64_t ball_cube_rows(int ny, int nz, int cy, int cz, int ring) {
    const int64_t y0 = cy - (int64_t)ring > 0 ? cy - (int64_t)ring : 0, y1 = cy + (int64_t)ring < ny - 1 ? cy + (int64_t)ring : ny - 1;
    const int64_t z0 = cz - (int64_t)ring > 0 ? cz - (int64_t)ring : 0, z1 = cz + (int64_t)ring < nz - 1 ? cz + (int64_t)ring : nz - 1;
    return (y1 - y0 + 1) * (z1 - z0 + 1);
}

// ---- the streaming rule ----------------------------------------------------------------------------------------------------
// A query whose cube covers the grid, or whose clipped cube has more (y, z) rows than a sixteenth of the n candidates,
// reads the cell-sorted cloud linearly: n / 64 full steps of 64 candidates.  Walking the
// cube costs one step per run of a non-empty row -- mostly idle lanes once rows are short -- and one fetch of run bounds
// per 64 rows: between n / 64 rows (every row holds points: the walk already costs as many steps as the stream) and n
// rows (every row empty) the walk loses.  n / 16 is the geometric middle of the two; any threshold gives the same rows.
constexpr int64_t kBallStreamDivisor = 16;
QP_HD inline bool ball_streams(int64_t n, int nx, int ny, int nz, int cx, int cy, int cz, int ring) {
    if (ball_cube_covers(nx, ny, nz, cx, cy, cz, ring)) return true;
    return ball_cube_rows(ny, nz, cy, cz, ring) * kBallStreamDivisor > n;
}

// The pure rules of the queries of caller-supplied points (pct_api.hip, pct_query.hip, pct_ball.hip): which path answers a
// set of query points, the cell a query is filed in, its position inside that cell, and the radius a searched cube of
// cells vouches for.  That radius is the guarantee of EVERY sweep over the cell list: guaranteed_r2 (pct_knn_sweep.h)
// forwards here, for the cloud's own points as for a caller's, which may lie outside the grid box.  Nothing here knows a
// handle, a device or the environment; the cell, the position and the radius are what the kernels evaluate (QP_HD) --
// tests/test_query_plan.py compiles this header alone with the host compiler and checks the radius against brute force.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/pct_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QP_HD __host__ __device__
#else
#define QP_HD
#endif

// ---- the route -----------------------------------------------------------------------------------------------------------
enum class QueryRoute { Sweep = 0, GridResident = 1, GridBuild = 2 };     // (the numbers pct_query_stats reports)

// PCT_QUERY_AUTO leaves the exhaustive sweep only for m >= kQueryAutoMinM queries of a cloud of n >= kQueryAutoMinN
// points (the bound resolve_request has for PCT_KNN_AUTO, pct_auto_route.h) -- the neighbour study's 500 sample points
// and every caller of pct_query_points stay where they were -- and from m n >= kQueryAutoCrossover pairs on.
// The crossover is measured (tools/query_probe.py crossover on one MI355X, the table in DESIGN 4.3e): random torus,
// k = 16, n in {4096 .. 1 M} x m in {1024 .. 1 M}, wall time of the whole call.  2^34 is the smallest m n from which the
// cell list -- resident, and built by the call -- won on every measured pair; at 2^32 it still lost at n = 4096, m = 1 M
// and at 2^30 it tied at n = 4096, m = 262 144.
constexpr int64_t kQueryAutoMinM = 1024;
constexpr int64_t kQueryAutoMinN = 4096;
constexpr int64_t kQueryAutoCrossover = (int64_t)1 << 34;

struct QueryState {
    bool uniform_resident;      // a uniform cell list over the WHOLE cloud is in place
    bool tree_resident;         // the table in place came from the hierarchical list or the chain of cell lists
    bool sorted_resident;       // a table or fit results in place refer to the cell order: a rebuild would invalidate them
    bool sharded;               // an owned range, a culled grid (any finite lim_lo / lim_hi)
    bool slab;                  // slab ownership (the entry refuses before it asks; a rule of its own all the same)
};

// m n >= pairs without forming the product (m n may pass 2^63): m >= ceil(pairs / n).  n >= 1.
inline bool query_pairs_reach(int64_t m, int64_t n, int64_t pairs) { return m >= (pairs + n - 1) / n; }

// *route is written for every known algo.  false: unknown algo (PCT_ERR_INVALID).
inline bool query_route(int32_t algo, int64_t n, int64_t m, int32_t k, const QueryState& s, QueryRoute* route) {
    (void)k;                    // (every k of the entry, 1 .. 128, fits both paths)
    *route = QueryRoute::Sweep;
    if (algo != PCT_QUERY_AUTO && algo != PCT_QUERY_SWEEP && algo != PCT_QUERY_GRID) return false;
    if (algo == PCT_QUERY_SWEEP) return true;
    if (algo == PCT_QUERY_AUTO) {
        if (m < kQueryAutoMinM || n < kQueryAutoMinN) return true;
        if (!query_pairs_reach(m, n, kQueryAutoCrossover)) return true;
    }
    // the cell list cannot answer: same rows from the exhaustive sweep, nothing resident is touched
    if (s.tree_resident || s.sharded || s.slab) return true;
    if (s.uniform_resident) { *route = QueryRoute::GridResident; return true; }
    if (s.sorted_resident) return true;
    *route = QueryRoute::GridBuild;
    return true;
}

// ---- the query's cell ----------------------------------------------------------------------------------------------------
// floor((x - o) inv) clamped to [0, n - 1] IN DOUBLE, then converted: a caller's query may lie anywhere (1e30, 1e300:
// the product may even be +-inf), where the conversion of the unclamped value to int is undefined.
QP_HD inline int query_cell_coord(double x, double o, double inv, int n) {
    double c = floor((x - o) * inv);
    if (!(c >= 0.0)) c = 0.0;                         // (also a NaN, which finite inputs cannot give)
    if (c > (double)(n - 1)) c = (double)(n - 1);
    return (int)c;
}

// the query's position relative to the low corner of its cell c, in cell units
QP_HD inline double query_cell_offset(double x, double o, double inv, int c) { return (x - o) * inv - c; }

// a query inside the grid box has every in-cell offset in [0, 1); a clamped one (or an overflowed offset) has not
QP_HD inline bool query_inside_cell(double g) { return g >= 0.0 && g < 1.0; }

// ---- the radius a searched cube vouches for ------------------------------------------------------------------------------
// The cube of cells within Chebyshev distance `ring` of the query's cell (cx, cy, cz), clipped to the grid, has been
// searched.  gx, gy, gz: query_cell_offset per axis -- in [0, 1) for a query inside the grid box (every point of the cloud
// is one); below 0 (cell 0) or at and above 1 (cell n - 1) for a query clamped into a boundary cell.
// Returns a lower bound, in cell units, on the distance from the query to any point filed in a cell OUTSIDE the cube;
// +inf when the cube covers the grid.
//
// Why it holds, a clamped query included.  A point outside the cube is outside it along some axis, say x, on one side.
// High side: its cell index is > cx + ring, so its coordinate is at least that cell's low face, cx + ring + 1 (points
// clamped into the last cell lie beyond its outer face: farther still); the query sits at cx + gx, the gap is
// ring + 1 - gx for ANY gx, and it only grows for gx < 0.  Low side: the point lies below the face cx - ring, the gap is
// gx + ring for any gx, growing for gx >= 1.  A term could only turn small or negative for gx < -ring on the low side or
// gx > ring + 1 on the high side -- but gx < 0 happens in cell 0 alone, where the low side is open (cx - ring <= 0: no
// cell beyond, the term is +inf), and gx >= 1 in cell n - 1 alone, where the high side is open.  So every finite term is
// >= ring > 0 and is a true gap; the smallest one bounds the distance.
// An overflowing gx (+-inf for a query at 1e300 over a tiny cell) gives +inf terms, never a NaN: inf is only added to.
QP_HD inline double query_guarantee_cells(int nx, int ny, int nz, int cx, int cy, int cz, double gx, double gy, double gz, int ring) {
    const double inf = INFINITY;
    double gmin = inf;
    gmin = fmin(gmin, cx - ring <= 0 ? inf : gx + ring);
    gmin = fmin(gmin, cx + ring >= nx - 1 ? inf : (1.0 - gx) + ring);
    gmin = fmin(gmin, cy - ring <= 0 ? inf : gy + ring);
    gmin = fmin(gmin, cy + ring >= ny - 1 ? inf : (1.0 - gy) + ring);
    gmin = fmin(gmin, cz - ring <= 0 ? inf : gz + ring);
    gmin = fmin(gmin, cz + ring >= nz - 1 ? inf : (1.0 - gz) + ring);
    return gmin;
}
// ... squared, in the cloud's units, shrunk by 1e-6 (the cell coordinates are rounded twice)
QP_HD inline double query_guaranteed_r2(int nx, int ny, int nz, double cell, int cx, int cy, int cz, double gx, double gy, double gz, int ring) {
    const double rr = query_guarantee_cells(nx, ny, nz, cx, cy, cz, gx, gy, gz, ring) * cell * (1.0 - 1e-6);
    return rr * rr;
}

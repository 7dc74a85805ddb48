// The pure host rules of a sweep's route (run_knn, pct_api.hip): what a request resolves to and what PCT_KNN_AUTO makes
// of a cloud -- the remembered verdict, the give-up of the uniform list, the skew gate, the census.  Nothing here knows a
// handle, a device or the environment (the caller reads the two switches) -- tests/test_auto_route.py compiles this
// header alone with the host compiler.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/pct_hip.h"

struct RouteSwitches { bool no_tree, no_auto_levels; };       // PCT_NO_TREE, PCT_NO_AUTO_LEVELS

// ---- the request ---------------------------------------------------------------------------------------------------------
struct Request {
    int32_t algo;          // the algorithm asked for, PCT_KNN_AUTO resolved
    bool auto_req;         // PCT_KNN_AUTO was asked and is still free to choose
    bool tree_ok;          // the hierarchical cell list takes whole clouds below 2^26 points; a shard asked of it goes down the chain of cell lists
};
enum class Refusal { None, UnknownAlgorithm, SlabNeedsFusedGrid };

inline Refusal resolve_request(int32_t asked, int32_t k, int64_t n, bool whole_cloud, bool slab, bool fused, Request* out) {
    int32_t algo = asked;
    bool auto_req = algo == PCT_KNN_AUTO;
    if (algo == PCT_KNN_AUTO) algo = n >= 4096 ? PCT_KNN_GRID : PCT_KNN_BRUTE;
    // cKDTree.query takes any k (pct:83).  The fast sweeps sort lists of one or two registers per lane (k <= 127);
    // longer rows go through the wave-per-query sweeps, whose running list is 64 R wide for any power of two R: the
    // exact sweep over the cell list (any cloud size), the exhaustive sweep where that was asked for.
    if (k > 127) {
        if (algo != PCT_KNN_BRUTE) algo = PCT_KNN_GRID_EXACT;
        auto_req = false;
    }
    *out = Request{algo, auto_req, whole_cloud && n < ((int64_t)1 << 26)};
    if (algo != PCT_KNN_GRID && algo != PCT_KNN_BRUTE && algo != PCT_KNN_GRID_EXACT && algo != PCT_KNN_GRID_LEVELS && algo != PCT_KNN_TREE)
        return Refusal::UnknownAlgorithm;
    if (slab) {            // one cell list over the slab and its margin (include/pct_hip.h)
        if (!fused || (algo != PCT_KNN_GRID && algo != PCT_KNN_GRID_EXACT)) return Refusal::SlabNeedsFusedGrid;
        out->auto_req = false;
    }
    return Refusal::None;
}

// ---- the remembered verdict ----------------------------------------------------------------------------------------------
// A handle fed a stream of similar clouds: what the census said about the last one of this size still holds.  *calls
// counts the calls that got as far as asking (same size): every 16th is examined afresh.
inline bool remembered_applies(const Request& r, int64_t n, int64_t remembered_n, int32_t* calls, RouteSwitches sw) {
    return r.auto_req && r.tree_ok && remembered_n == n && (++*calls & 15) != 0 && !sw.no_tree && !sw.no_auto_levels;
}
// ... for clouds of this size AND this bounding box {min xyz, max xyz}, within 2 % of the extent per face -- the same test
// the speculative cell-list build applies to "a stream of similar clouds"
inline bool same_box(const float* box, const float* remembered) {
    bool same = true;
    for (int a = 0; a < 3; ++a) {
        const float tol = 0.02f * (remembered[3 + a] - remembered[a]) + 1e-30f;
        same = same && fabsf(box[a] - remembered[a]) <= tol && fabsf(box[3 + a] - remembered[3 + a]) <= tol;
    }
    return same;
}

// ---- the uniform list: given up, kept, or left for another structure ----------------------------------------------------
// pct_build_grid may give up (nothing built) where the hierarchical list is there to take the cloud
inline bool may_give_up(const Request& r, int64_t n, RouteSwitches sw) {
    return r.auto_req && r.algo == PCT_KNN_GRID && r.tree_ok && n >= 16384 && !sw.no_tree && !sw.no_auto_levels;
}

// PCT_KNN_AUTO on a whole cloud: is one cell size enough?  A point of a cloud of even density shares its cell with about
// as many points as a non-empty cell holds on average; where the density spans decades the first figure (size-biased)
// runs away from the second.  Only then the work items are counted (the census).
inline bool skew_gate(const Request& r, bool whole_cloud, int64_t n, int64_t nonempty_cells, RouteSwitches sw) {
    return r.auto_req && r.algo == PCT_KNN_GRID && whole_cloud && n >= 65536 && n < ((int64_t)1 << 29) && nonempty_cells > 0 && !sw.no_auto_levels;
}
inline double cell_skew(double occupancy, int64_t nonempty_cells, int64_t n) { return occupancy * (double)nonempty_cells / (double)n; }
inline double skew_min(bool tree_reachable) { return tree_reachable ? 1.25 : 1.5; }      // (the chain needs a wider spread to pay)

// The census of the cell list in place (pct_item_census): c = {queries, queries whose stencil overflows the staging area,
// queries whose stencil is too short, non-empty stencil cells summed over the other queries}.  The share of queries that
// would all go through the wave-per-query exact sweep, and how many stencil cells the others find non-empty (about 9-13
// on a surface, up to 27 in a volume, where the chain of cell lists does not pay).
struct CensusShares { double q, fail, fine, cells; };
inline CensusShares census_shares(const unsigned long long c[4]) {
    CensusShares s;
    s.q = (double)(c[0] ? c[0] : 1);
    s.fail = (double)(c[1] + c[2]) / s.q;
    s.fine = (double)c[0] - (double)(c[1] + c[2]);
    s.cells = s.fine > 0 ? (double)c[3] / s.fine : 27.0;
    return s;
}
enum class Route { Stay, Tree, Levels };      // the uniform list in place | the hierarchical list | the chain of cell lists
inline Route census_route(const CensusShares& s, int64_t n, bool tree_reachable) {
    // (the hierarchical list costs ~1.7x a uniform one whatever the density; every query the uniform list would hand
    // to the exact sweep costs about as much as twelve it answers itself)
    // (the hierarchical list's build -- a dozen launches, three read-backs -- costs ~0.45 ms more than the uniform one
    // whatever the cloud's size, a query handed to the exact sweep ~12 ns: below a million points the predicted share
    // must be larger for the switch to pay)
    const double fail_min = fmax(0.08, 37500.0 / (double)n);
    if (tree_reachable) return s.fail > fail_min && s.cells < 15.0 ? Route::Tree : Route::Stay;
    return s.fail > 0.30 && s.fine > 0.02 * s.q && s.cells < 15.0 ? Route::Levels : Route::Stay;
}

// The pure host decisions of the cell-list build (pct_grid.hip): the source of its points, the cell-edge search and the
// shape of the two-level counting sort.  Nothing here knows a handle, a device or the environment -- tests/test_grid_edge.py
// compiles this header alone with the host compiler and drives it with plain values and occupancy models.
#pragma once

#include <math.h>
#include <stdint.h>

// ---- where the grid's points come from ---------------------------------------------------------------------------------
enum class GridSource {
    LevelBase,     // later passes of the density-adaptive sweep: the points in the cell order of its first pass, and that pass's box
    CulledPack,    // sharded handle: the owned rows and the points near them (pack_near_owned)
    CallerRows,    // the caller's rows on the (trimmed) box of the previous similar cloud; this cloud's box is checked later
    FullPack,      // every point, packed and measured first
};
struct SourceInputs {
    bool by_want, base_usable;     // the pass owns by wanted edge; the first pass's records hold every point
    bool chained;                  // a pass of the chained sweep, the first included
    bool slab, sharded;            // ownership by slab; some points are candidates only
    int64_t n_owned;
    bool has_f64, no_cull, env_no_cull, env_no_spec;      // of the handle; PCT_NO_CULL, PCT_NO_SPEC
    double hint_edge; bool spec_valid; int64_t spec_n, n; // the handle's warm start, the record of its last plain build, this cloud
};
inline GridSource choose_source(const SourceInputs& in) {
    // (a slab's owned points are found by the pack itself: it always runs, with an open box after a limit retry)
    const bool try_cull = in.slab ? in.n_owned > 0
                                  : !in.by_want && in.sharded && in.n_owned > 0 && !in.has_f64 && !in.no_cull && !in.env_no_cull;
    // Speculation: a handle fed a stream of similar clouds builds the cell list over the (trimmed) box of the previous
    // call without waiting for the new bounding box -- any box is a valid grid box, points outside are clamped into
    // the boundary cells -- and checks the new box at the synchronisation that ends the first pass.  One host round
    // trip less per build.
    const bool spec = !try_cull && !in.by_want && !in.chained && in.hint_edge > 0 && in.spec_valid && in.spec_n == in.n && !in.env_no_spec;
    return in.by_want && in.base_usable ? GridSource::LevelBase : try_cull ? GridSource::CulledPack : spec ? GridSource::CallerRows : GridSource::FullPack;
}

// ---- cell size ---------------------------------------------------------------------------------------------------------
// The edge is steered until a point shares its cell with about `target` points (the occupancy m the build measures).
// One pass: a = clamp_eps(a); [build, measure m]; accept(...) ? done : a = next(m, a).
struct EdgeSearch {
    // inputs
    double target;                 // wanted occupancy: factor * (k + 1)
    int64_t n;                     // points the grid holds
    double ex, ey, ez;             // extents of the grid box
    double eps;                    // > 0: one ring must cover the eps ball, the edge cannot grow past it
    double hint_edge, hint_guess, hint_target;     // what the previous build on this handle converged to (0: none)
    double level_edge;             // > 0: a level pass of the density-adaptive sweep, the edge is given
    int max_iter;
    // state
    double emax = 1.0;             // longest extent (1 for a point)
    bool no_extent = false;        // the box is a point: one cell at every edge, no step changes the occupancy
    double first_guess = 0;        // this cloud's own first guess, before the warm start and the clamps
    bool hinted = false;           // the first edge came from the previous cloud on this handle
    double a_prev = 0, m_prev = 0, d_last = 2.0;

    static constexpr double kWinLo = 0.88, kWinHi = 1.12;      // accept window around target

    double cap() const { return emax * 1.0001 + 1e-30; }       // one cell holds the whole box: larger is pointless

    double first() {
        emax = fmax(ex, fmax(ey, ez));
        no_extent = !(emax > 0);
        if (no_extent) emax = 1.0;
        // first guess: the cloud is a surface whose area is about the bbox's half-surface * 1.2
        double area = 1.2 * (ex * ey + ey * ez + ex * ez);
        if (!(area > 0)) area = emax * emax;
        double a = sqrt(target * area / (double)n);
        if (!(a > 0) || !isfinite(a)) a = emax;
        first_guess = a;
        hinted = false;
        // Warm start: a handle that sees a stream of similar clouds (same scanner, same shard of the same job) reuses
        // the edge the last build converged to, rescaled by the first-guess ratio, and so normally needs one pass.
        if (level_edge > 0) {
            a = level_edge;
        } else if (hint_edge > 0 && hint_guess > 0) {
            const double r = first_guess / hint_guess * sqrt(hint_target / target);   // guess ~ sqrt(target)
            if (r > 0.5 && r < 2.0) { a = hint_edge * r * sqrt(target / hint_target); hinted = true; }
        }
        return fmin(a, cap());
    }

    // the inherited edge was absurd for this cloud (pct_build_grid's PCT_KNN_AUTO test): its own first guess, then
    double fallback_first() {
        hinted = false;
        return fmin(first_guess, cap());
    }

    double clamp_eps(double a) const { return eps > 0 && a > eps * 1.000001 ? eps * 1.000001 : a; }   // one ring already covers the eps ball

    // is the pass that measured occupancy m at edge a (ncell cells, pass `it`) the last one?
    bool accept(double m, double a, int64_t ncell, int64_t cell_cap, bool hit_cap, int it) const {
        const bool eps_bound = eps > 0 && a >= eps;            // cannot grow past eps
        const bool capped = ncell * 2 > cell_cap && m < target;
        return (m >= kWinLo * target && m <= kWinHi * target) || it == max_iter - 1 || (eps_bound && m < target) ||
               capped || (a >= emax && m < target) || (hit_cap && m > target) ||      // (cannot refine past the cell budget)
               no_extent;             // (identical points: the same one-cell grid whatever the edge)
    }

    // secant step on the measured dimension d (m ~ a^d; 2 for a surface, until two passes have measured it)
    double next(double m, double a) {
        double d = 2.0;
        if (a_prev > 0 && m != m_prev && a != a_prev) {
            d = log(m / m_prev) / log(a / a_prev);
            if (!(d >= 1.0)) d = 1.0;
            if (d > 3.0) d = 3.0;
        }
        a_prev = a;
        m_prev = m;
        d_last = d;
        double f = pow(target / m, 1.0 / d);
        f = fmin(fmax(f, 1.0 / 16.0), 16.0);
        return fmin(a * f, cap());
    }

    // what the heuristic first guess should have been for this cloud (the next build's hint_edge)
    double hint_after(double cell, double m_last) const { return cell * pow(target / m_last, 1.0 / d_last); }
};

// ---- two-level counting sort -------------------------------------------------------------------------------------------
constexpr int kBinTileRows = 4096;       // input rows per tile (times a whole factor for clouds above kBinMaxTiles tiles)
constexpr int kBinMaxTiles = 1024;
constexpr int kBinMaxBuckets = 4096;     // LDS counters of the coarse level
constexpr int kBinMaxCounters = 8192;    // LDS counters of the fine level: cells per bucket x classes
constexpr int kBinMinChunk = 4096;       // records per work item (at least; never below the fine counters)

struct BinShape {
    bool ok;             // the bucket scheme covers this grid
    int shift;           // log2 cells per bucket
    int nb;              // buckets
    int cls;             // classes: 1 = every point owned, 2 = owned / other
    int tile_rows, ntiles;
    int chunk;           // records per work item
    int max_items;       // upper bound of the work list: every bucket at least one item
    int max_shared;      // upper bound of the items of shared buckets
};

// Sizing: about a thousand buckets (each a few thousand points at the sweep's occupancies), cells per bucket a power of
// two from 256 up to what the fine LDS counters hold; a grid that would still need more than kBinMaxBuckets is not covered.
inline BinShape bin_shape(int64_t n, int64_t ncell, bool sharded) {
    BinShape s = {};
    s.cls = sharded ? 2 : 1;
    int max_shift = 8;                                // 2^shift * cls <= kBinMaxCounters
    while ((s.cls << (max_shift + 1)) <= kBinMaxCounters) ++max_shift;
    s.shift = 8;
    while (((ncell + ((int64_t)1 << s.shift) - 1) >> s.shift) > 1024 && s.shift < max_shift) ++s.shift;
    const int64_t nb = (ncell + ((int64_t)1 << s.shift) - 1) >> s.shift;
    s.ok = n >= 1 && n < ((int64_t)1 << 31) - kBinTileRows && ncell >= 1 && nb <= kBinMaxBuckets;
    if (!s.ok) return s;
    s.nb = (int)nb;
    const int64_t f = (n + (int64_t)kBinTileRows * kBinMaxTiles - 1) / ((int64_t)kBinTileRows * kBinMaxTiles);
    s.tile_rows = (int)(kBinTileRows * (f < 1 ? 1 : f));
    s.ntiles = (int)((n + s.tile_rows - 1) / s.tile_rows);
    s.chunk = (s.cls << s.shift) > kBinMinChunk ? (s.cls << s.shift) : kBinMinChunk;
    s.max_items = s.nb + (int)(n / s.chunk);
    s.max_shared = 2 * (int)(n / s.chunk) + 1;          // sum of ceil(c / chunk) over the buckets with c > chunk
    return s;
}

// Which fast sweep a call takes: decided once (plan_sweep), launched once (launch_sweep, pct_knn.hip), reported in
// pct_timings.sweep_variant.  Every choice returns the same rows bit for bit; only the timings tell them apart.
// Pure host arithmetic over plain values: nothing here knows a handle, a device or the environment (the caller fills
// SweepInputs from the handle and reads the switches) -- tests/test_sweep_plan.py compiles this header alone with the
// host compiler.
#pragma once

#include <math.h>
#include <stdint.h>

enum SweepFamily { kNoSweep = 0, kFast = 1, kPair = 2, kDuo = 3 };      // none | k_knn_fast | k_knn_pair | k_knn_duo

// the six (PRE, PAIR, Q64, TREE) forms k_knn_fast exists in: its static assertions and launch bounds know no other
enum FastForm { kPlain, kPre, kPrePair, kPrePairQ64, kTree, kTreeQ64, kFastForms };
struct FastFlags { bool pre, pair, q64, tree; };
constexpr FastFlags kFastFlags[kFastForms] = {{false, false, false, false}, {true, false, false, false}, {true, true, false, false},
                                              {true, true, true, false},    {true, true, false, true},   {true, true, true, true}};

struct SweepPlan {
    SweepFamily family = kNoSweep;
    FastForm form = kPlain;             // family == kFast: which of the six (the four flags below, as one value)
    int R = 1;                          // list registers per lane
    bool eps = false, pre = false, pair = false, q64 = false, tree = false;
    bool dist = true;                   // the distance table is written
    bool lean() const { return family == kPair || family == kDuo; }
    // pct_timings.sweep_variant (include/pct_hip.h)
    int32_t variant() const {
        if (family == kNoSweep) return 0;
        return family | (R == 2) << 2 | eps << 3 | pre << 4 | pair << 5 | q64 << 6 | tree << 7 | dist << 8;
    }
};

// what the rule reads of the handle: the work items, the cloud's flags, the R = 1 limit (pct_fast_r1_max) and the
// uniform grid's box
struct SweepInputs {
    int64_t n_items;
    bool has_f64, level_mode, own_flag;
    int r1_max;
    double cell, ox, oy, oz;
    int nx, ny, nz;
};
// the tuning switches (PCT_*: A/B aids, read per call -- tests flip them)
struct SweepSwitches { bool no_pair, no_pair_kernel, no_duo_kernel, keep_dist; };      // PCT_NO_PAIR, PCT_NO_PAIR_KERNEL, PCT_NO_DUO_KERNEL, PCT_KEEP_DIST

// tree: the hierarchical cell list is in place (whole clouds, one pass), else the uniform one; exact_only / phase as in
// pct_launch_knn_grid; want_dist = false: the caller reads no distances from the table.
inline SweepPlan plan_sweep(const SweepInputs& in, const SweepSwitches& sw, int32_t k, double eps, bool tree, bool exact_only, int phase,
                            bool want_dist) {
    SweepPlan p;
    if (exact_only || phase == 2 || in.n_items <= 0) return p;
    p.eps = eps > 0;
    p.tree = tree;
    const bool r1 = k + 1 <= in.r1_max, f64 = in.has_f64;
    const bool no_pair = sw.no_pair;
    bool lean = in.n_items < ((int64_t)1 << 31) - 8 && !no_pair;
    if (tree) {
        // float64 clouds: the variant whose bounds are widened by the distance between a query and its float32 rounding
        // (Q64); where that distance is not small against the item's cells the proofs fail and the exact sweep answers
        p.form = f64 ? kTreeQ64 : kTree;
    } else {
        // The float32 pre-selection squares coordinate differences of up to three cell edges: outside this window
        // they overflow (or the eps ball's radius underflows) and every candidate would fail the threshold test,
        // so such clouds take the variant that keys every candidate in float64.
        const double c2 = in.cell * in.cell;
        const bool f32_ok = c2 > 1e-30 && c2 < 1e30 && (!(eps > 0) || eps * eps > 1e-36);
        // Float64 clouds pre-select too (Q64: bounds widened by the rounding distance of the query) unless that
        // distance is not small against a cell edge -- coordinates so large that float32 resolves them barely finer
        // than the cells: there every query would be sent to the exact sweep.
        const double far = fmax(fmax(fabs(in.ox), fabs(in.ox + in.nx * in.cell)),
                                fmax(fmax(fabs(in.oy), fabs(in.oy + in.ny * in.cell)), fmax(fabs(in.oz), fabs(in.oz + in.nz * in.cell))));
        const bool near = far * 0x1p-23 < in.cell * 0x1p-7;
        p.form = f64 ? (f32_ok && near && !in.level_mode && !no_pair ? kPrePairQ64 : kPlain) : !f32_ok ? kPlain : no_pair ? kPre : kPrePair;
        // the scalar-lean kernels take the plain sweep only: one pass, ownership by index range
        lean = lean && phase == 0 && (!f64 || near) && f32_ok && !in.own_flag && !in.level_mode;
    }
    // rows of up to kFastR1Max entries: k_knn_pair; up to 128 (two list registers): k_knn_duo; anything else: k_knn_fast
    if (lean && r1 && !sw.no_pair_kernel) p.family = kPair;
    else if (lean && !r1 && k + 1 <= 128 && !sw.no_duo_kernel) p.family = kDuo;
    else p.family = kFast;
    p.R = p.family == kDuo || (p.family == kFast && !r1) ? 2 : 1;
    const FastFlags f = p.lean() ? FastFlags{true, true, f64, tree} : kFastFlags[p.form];
    p.pre = f.pre; p.pair = f.pair; p.q64 = f.q64;
    // the fused curvature call, whose fit never reads distances, has the lean kernels write no distance table
    // (pct_get_neighbors derives the same bits from the positions when asked)
    p.dist = !(p.lean() && !want_dist && !sw.keep_dist);
    return p;
}

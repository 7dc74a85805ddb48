// The state rules of include/pct_hip.h as the library keeps them: which results a handle holds -- and for each of them,
// here and nowhere else, the order it is stored in and the rows it covers --, which events drop which of them, what a
// result is derived from.  Pure host code that knows no handle and no device -- tests/test_residents.py
// compiles this header alone with the host compiler and holds every set below equal to the table of tests/call_model.py.
#pragma once

#include <stdint.h>

// What one handle holds at most one of each: the neighbour table, the fit results, the point areas, the point frames, their
// orientation, the fans and triangles, the PCA results, the ball rows, the boundary loops and patches of the triangles
// (order and names: call_model.RESIDENTS)
enum pct_resident : uint32_t {
    PCT_R_TABLE = 1, PCT_R_FIT = 2, PCT_R_AREAS = 4, PCT_R_FRAMES = 8, PCT_R_ORIENT = 16, PCT_R_TRIANGLES = 32, PCT_R_PCA = 64, PCT_R_BALL = 128,
    PCT_R_HOLES = 256
};
constexpr int kPctResidents = 9;
constexpr const char* kPctResidentNames[kPctResidents] = {"table", "fit", "areas", "frames", "orient", "triangles", "pca", "ball", "holes"};
constexpr uint32_t kPctEveryResident = (1u << kPctResidents) - 1;
// what is computed per owned row; ball rows and PCA results answer for the whole cloud
constexpr uint32_t kPctPerOwnedRow = PCT_R_TABLE | PCT_R_FIT | PCT_R_AREAS | PCT_R_FRAMES | PCT_R_ORIENT | PCT_R_TRIANGLES | PCT_R_HOLES;

// ---- the events that drop results, each with its constant set ---------------------------------------------------------------
struct pct_drop { uint32_t set; };
constexpr pct_drop PCT_NEW_CLOUD = {kPctEveryResident};                    // pct_set_points_*, pct_use_points_*: every result
constexpr pct_drop PCT_OWNERSHIP = {kPctPerOwnedRow};                      // pct_set_query_range, pct_set_query_slab
constexpr pct_drop PCT_PLANTING = {kPctPerOwnedRow};                       // pct_knn, pct_curvature, pct_surface_variation, pct_pca_curvatures
constexpr pct_drop PCT_TABLE_LOST = {PCT_R_TABLE};                         // pct_voxel_downsample: its buffers were reused, nothing replanted
constexpr pct_drop PCT_TABLE_AND_FIT_LOST = {PCT_R_TABLE | PCT_R_FIT};     // pct_pca_curvatures: the table in place holds over-fetched candidates
constexpr pct_drop PCT_UNFINISHED_TABLE = {kPctEveryResident};             // pct_selftest_sweep: a fast sweep without its exact sweep -- as a new cloud

// ---- what a result is derived from ------------------------------------------------------------------------------------------
// Frames come from the fit, the orientation from the frames, the hole results from the triangles (include/pct_hip_holes.h).
// (Fit, areas and triangles are computed from the table but do not refer to it afterwards: they outlive it, PCT_TABLE_LOST.)
constexpr uint32_t pct_made_from(uint32_t r) {
    return r == PCT_R_FRAMES ? PCT_R_FIT : r == PCT_R_ORIENT ? PCT_R_FRAMES : r == PCT_R_HOLES ? PCT_R_TRIANGLES : 0u;
}
// ... so whatever replaces a result drops everything made from it, directly or through another result: "a fit drops the
// frames and the orientation", "pct_point_frames drops the orientation"
constexpr pct_drop pct_replacing(pct_resident r) {
    uint32_t set = r;
    for (int pass = 0; pass < kPctResidents; ++pass)
        for (int b = 0; b < kPctResidents; ++b)
            if (pct_made_from(1u << b) & set) set |= 1u << b;
    return pct_drop{set};
}

// ---- what a handle holds ----------------------------------------------------------------------------------------------------
struct pct_residents {
    uint32_t live = 0;             // the results in place
    uint32_t by_row = 0;           // of those, the ones stored in neighbour-table row (cell) order, not in public order
    int64_t rows[kPctResidents] = {};      // the rows each of them covers (0: not in place)
    void drop(pct_drop d) {
        live &= ~d.set;
        by_row &= ~d.set;
        for (int b = 0; b < kPctResidents; ++b)
            if (d.set >> b & 1) rows[b] = 0;
    }
    // r has just been computed for n rows; row_order: as its launcher stored it
    void leave(pct_resident r, bool row_order, int64_t n) {
        drop(pct_replacing(r));
        live |= r;
        by_row |= row_order ? r : 0u;
        for (int b = 0; b < kPctResidents; ++b)
            if (r >> b & 1) rows[b] = n;
    }
    bool has(pct_resident r) const { return (live & r) != 0; }
    bool in_row_order(pct_resident r) const { return (by_row & r) != 0; }
    int64_t rows_of(pct_resident r) const {
        for (int b = 0; b < kPctResidents; ++b)
            if (r >> b & 1) return rows[b];
        return 0;
    }
    // r is in place and covers exactly n rows
    bool covers(pct_resident r, int64_t n) const { return has(r) && rows_of(r) == n; }
    // something in place is indexed by the cell order: a query must not rebuild the cell list under it
    bool any_in_cell_order() const { return by_row != 0; }
};

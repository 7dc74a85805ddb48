/*
 * pct_hip.h -- C ABI of the MI355X (gfx950) per-point curvature path.
 *
 * The reference has no FFI layer: its boundary is the Python class PointCloud
 * (/root/reference/pointCloudToolbox.py:24).  These entry points are what the
 * methods on that class's hot path bind to through ctypes; each one cites the
 * reference method it replaces.  Plain C types only, caller-allocated output
 * buffers, int status return (PCT_OK == 0), blocking semantics, one HIP stream
 * per handle, no global mutable state (several handles / ranks may coexist).
 */
#ifndef PCT_HIP_H
#define PCT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pct_ctx pct_ctx;

enum pct_status {
    PCT_OK = 0,
    PCT_ERR_HIP = 1,          /* a HIP runtime call failed (see pct_last_error)        */
    PCT_ERR_NO_DEVICE = 2,    /* no usable gfx950 device                               */
    PCT_ERR_INVALID = 3,      /* bad argument / call order                             */
    PCT_ERR_NONFINITE = 4,    /* NaN/Inf in the cloud (pointCloudToolbox.py:273-274)   */
    PCT_ERR_K_TOO_LARGE = 5,  /* k + 1 > N (reference: IndexError at pct:640)          */
    PCT_ERR_OOM = 6,
    PCT_ERR_NO_NEIGHBORS = 7, /* fit requested before a neighbour table exists         */
    PCT_ERR_LIMIT = 8         /* pct_query_ball: more entries than the caller allows   */
};

enum pct_knn_algo {
    PCT_KNN_AUTO = 0,
    PCT_KNN_BRUTE = 1,        /* exhaustive wave-per-query sweep                        */
    PCT_KNN_GRID = 2,         /* uniform cell list, LDS-staged 27-cell stencil          */
    PCT_KNN_GRID_EXACT = 3,   /* same cell list, every query through the exact sweep    */
    PCT_KNN_GRID_LEVELS = 4,  /* chain of cell lists, each sized for the queries the previous
                                 one could not answer (clouds of very uneven density)    */
    PCT_KNN_TREE = 5          /* hierarchical cell list: the cloud in Morton order, every
                                 query swept at the octree level that suits ITS density
                                 (whole clouds below 2^26 points; anything else asked for
                                 it takes GRID_LEVELS).  PCT_KNN_AUTO takes it
                                 by itself where a census of the uniform list's work items
                                 predicts that it pays: surface-like clouds whose density
                                 spans a decade or more                                  */
};

/* Per-stage device times of the most recent call in milliseconds, from device clock stamps or events: the stages of an
 * explicit PCT_KNN_GRID / PCT_KNN_GRID_EXACT sweep or fused call are stamped by its own kernels (the device's wall clock
 * at the entry of the first kernel of every stage and at the end of the last), everything else is bracketed by hipEvents
 * (PCT_TIME_EVENTS=1: every call). */
typedef struct pct_timings {
    float upload_ms;          /* H2D of coordinates (0 when device-resident)            */
    float grid_ms;            /* bounding box + cell sizing + counting sort (device clock stamps or events) */
    float knn_ms;             /* neighbour sweep kernel(s) only (fast + exact redo) (device clock stamps or events) */
    float knn_fast_ms;        /* of which the fast sweep alone: k_knn_pair, k_knn_duo or k_knn_fast, see sweep_variant (device clock stamps or events) */
    float fit_ms;             /* fused plane-align + quadric fit + curvature kernel (device clock stamps or events) */
    float export_ms;          /* sorted-space -> public index translation               */
    float total_ms;           /* the stages above, first to last (device clock stamps or events) */
    int32_t knn_launches;
    int32_t grid_iters;       /* builds of the cell-size search, plus the passes that trimmed the grid box to 6 sigma */
    int32_t redo_adopted;     /* of redone_queries: rows whose list from the fast sweep the exact sweep took over as the
                                 answer of the 27-cell stencil and widened from there (a sweep statistic like
                                 ring_fallbacks; it sits here, in what was padding, so that no other field moves) */
    int64_t cells;            /* grid cells                                             */
    int64_t occupied_cells;   /* work items of the sweep (cells split into query chunks) */
    int64_t ring_fallbacks;   /* rows the exact sweep answered beyond the 27-cell stencil (of the rows it ran over) */
    int64_t lds_overflows;    /* work items whose stencil exceeded the LDS staging capacity (handed over whole) */
    int64_t flushes;          /* wave-wide sort/merge passes of the sweep               */
    int64_t candidate_steps;  /* 64-candidate distance steps of the sweep               */
    int64_t redone_queries;   /* queries re-done by the exact sweep (overflowing items, rows the stencil cannot vouch for, float-key collisions) */
    double cell_size;
    int64_t grid_points;      /* points held by the cell list: the cloud, or (sharded handles) the part of it
                                 near the owned range                                    */
    int32_t limit_retries;    /* 1 = the sweep was repeated with every point because a query reached past
                                 the part kept                                            */
    int32_t levels;           /* passes of the density-adaptive sweep (0 = not used)       */
    double occupancy;         /* mean number of points sharing a point's cell (the cell-size search steers on it) */
    int64_t fit_svd_rows;     /* rows of the last fit solved by the SVD kernel (lstsq's gelsd semantics: ill-conditioned
                                 or under-determined design matrices) instead of the normal equations */
    int32_t algo;             /* the sweep that produced the table in place (pct_knn_algo; what PCT_KNN_AUTO chose) */
    int32_t sweep_variant;    /* the fast sweep kernel the call launched last, 0 = none (exact-only or exhaustive sweep,
                                 k > 127, no work items).  Bits 0-1: family (1 k_knn_fast, 2 k_knn_pair, 3 k_knn_duo);
                                 then one bit per template argument: 2 R = 2, 3 EPS, 4 PRE, 5 PAIR, 6 Q64, 7 TREE, 8 DIST
                                 (k_knn_pair and k_knn_duo report PRE = PAIR = 1).  Every variant returns the same rows */
} pct_timings;

/* ---- state rules: what a call needs, what it leaves, what it drops --------------------------------------------------------
 * One handle holds at most one of each: a cloud, an owned range or slab, a neighbour table, fit results, point areas, point
 * frames with their orientation, fans and triangles, PCA results, ball rows.  The entry points below and in
 * pct_hip_surface.h say what they compute; these rules say how they meet on one handle.  The library keeps them as one
 * table, csrc/pct_residents.h: which event drops which results, and what a result is derived from.  tests/call_model.py
 * states them again as a table and quotes every sentence it relies on (tests/test_residents.py holds the two tables equal);
 * tests/call_driver.py runs random call sequences against them.
 *
 * Refusals.  A refused call changes nothing: after a call that returns an error status for its arguments or for the state
 * of the handle, whatever was resident before it is resident still, with the same contents.  The one exception is
 * pct_query_ball: once its arguments are accepted it drops the rows of the previous query, so a query that then ends in
 * PCT_ERR_LIMIT, PCT_ERR_OOM or PCT_ERR_HIP leaves none; a query refused for its arguments or for the state of the handle
 * leaves them (every PCT_ERR_INVALID and PCT_ERR_NONFINITE of it, a refusal of the cell-list build included, comes first).
 * A state refusal is decided on the host before anything is launched.
 *
 * A new cloud (pct_set_points_f32, pct_set_points_f64, pct_set_points_device_f32, pct_use_points_device_f32) drops every
 * result on the handle: the table, the fit results, the areas, the frames, the orientation, the PCA results and the ball
 * rows, and the triangles with them.  It ends slab mode and owns the whole cloud.  What pct_set_async, pct_set_stats and pct_set_grid_param set stays.
 *
 * Ownership.  pct_set_query_range and pct_set_query_slab need a cloud (PCT_ERR_INVALID) and drop what is computed per
 * owned row: the table, the fit results, the areas, the frames and the orientation, and the triangles -- also where the
 * range is the one already set.  Ball rows and PCA results answer for the whole cloud and are untouched by a change of ownership.
 * Slab mode begins with pct_set_query_slab(parts >= 1) and ends with pct_set_query_range, a new cloud or
 * pct_set_query_slab(parts <= 0).  While a handle owns a slab these refuse with PCT_ERR_INVALID: pct_knn, pct_fit,
 * pct_fit_indices, pct_fit_ball, pct_get_neighbors, pct_get_neighbor_rows, pct_get_fit, pct_neighbor_study_curvatures,
 * pct_query_points, pct_query_points_algo, pct_query_ball, pct_point_areas, pct_get_point_areas, pct_point_energies,
 * pct_point_frames, pct_get_point_frames, pct_orient_frames, pct_get_orientation, pct_point_triangles,
 * pct_surface_variation and pct_pca_curvatures; pct_curvature refuses every algo but PCT_KNN_AUTO and PCT_KNN_GRID.  pct_get_ball, pct_get_pca,
 * pct_fit_indices_f64, pct_voxel_downsample and the stateless helpers keep working on a slab handle.
 * pct_slab_counts and pct_slab_records refuse with PCT_ERR_INVALID until a pct_curvature has run in slab mode.
 *
 * Plantings.  pct_knn, pct_curvature, pct_surface_variation and pct_pca_curvatures need a cloud (PCT_ERR_INVALID) and
 * drop the table in place, the fit results, the areas, the frames and the orientation, and the triangles.  Ball rows are untouched by a
 * planting, and so are PCA results unless the planting is pct_pca_curvatures.  pct_knn leaves its table; pct_curvature
 * leaves its table and the cloud-aligned fit of it; pct_surface_variation leaves a plain table of k_total - 1 neighbours
 * and no fit; pct_pca_curvatures leaves no readable table (the one in place holds its over-fetched candidates:
 * pct_get_neighbors and pct_fit answer PCT_ERR_NO_NEIGHBORS until the next planting) and no fit.
 *
 * Fits.  pct_fit, pct_curvature, pct_fit_indices and pct_fit_ball replace the fit results and drop the frames and the
 * orientation; the table, the areas, the ball rows and the PCA results are untouched by a fit, and so are the triangles.  The results of pct_fit and
 * pct_curvature are cloud-aligned (pct_get_fit takes rows of the owned range), those of pct_fit_indices and pct_fit_ball
 * are row-aligned (pct_get_fit(ctx, 0, rows, ...)).  pct_point_frames and pct_point_energies need the cloud-aligned fit of
 * the owned rows: PCT_ERR_INVALID "no fit results" after pct_fit_indices or pct_fit_ball.
 *
 * What needs the table: pct_fit, pct_get_neighbors, pct_get_neighbor_rows, pct_point_areas, pct_point_frames,
 * pct_point_triangles and pct_neighbor_study_curvatures answer PCT_ERR_NO_NEIGHBORS without one; pct_orient_frames answers PCT_ERR_INVALID.
 * What needs results: pct_get_fit PCT_ERR_INVALID without fit results; pct_get_point_areas PCT_ERR_INVALID without areas;
 * pct_get_point_frames and pct_orient_frames PCT_ERR_INVALID without frames; pct_get_orientation PCT_ERR_INVALID without
 * an orientation; pct_get_pca PCT_ERR_INVALID without PCA results, and for idx unless keep_neighbors was set; pct_get_ball
 * PCT_ERR_INVALID and pct_fit_ball PCT_ERR_NO_NEIGHBORS without ball rows.
 * pct_point_areas replaces the areas and touches nothing else.  pct_point_frames replaces the frames, drops the
 * orientation and touches nothing else.  pct_orient_frames turns the frames in place -- a second call starts from the
 * frames as the first left them -- and replaces the orientation.
 *
 * Triangles (pct_hip_surface.h).  pct_point_triangles needs the table and a whole-cloud handle, because agreement reads other
 * rows' corners: PCT_ERR_INVALID for an owned range, as pct_orient_frames.  Unknown flag bits: PCT_ERR_INVALID.
 * PCT_TRI_WIND_FRAMES without resident frames: PCT_ERR_INVALID "no point frames"; without the flag no frames are needed.
 * pct_point_triangles replaces the fans and triangles and touches nothing else: table, fit results, areas, frames,
 * orientation, PCA results, ball rows and pct_timings keep their bytes.  A new cloud, a change of ownership and every
 * planting drop the triangles; a fit, pct_point_frames, pct_orient_frames and pct_voxel_downsample do not: they are kept by
 * public index, and the winding is a snapshot of the flipped bits at the call.  pct_get_point_fans and pct_get_triangles
 * PCT_ERR_INVALID without triangles.
 *
 * Side calls.  pct_query_points, pct_query_points_algo, pct_fit_indices_f64, pct_neighbor_study_curvatures,
 * pct_curvatures_from_coefficients, pct_plane_rotate, pct_fit_quadric, pct_mesh_energies, every pct_get_* and every
 * *_stats call leave everything resident untouched, whichever path they take.  The point queries need a cloud
 * (PCT_ERR_INVALID), and so do pct_fit_indices and pct_fit_indices_f64.
 * pct_voxel_downsample and pct_voxel_downsample_f32 drop the table and nothing else: fit results, areas, frames, the
 * orientation, ball rows and PCA results computed before stay readable, whichever sweep planted the table; so do the
 * triangles.
 *
 * Asynchronous steps (pct_set_async): whatever a pending pct_curvature will leave is what every later call finds; no call
 * is served from the state before it. */

/* ---- lifetime ---------------------------------------------------------- */
int pct_device_count(int* count);
int pct_create(int device, pct_ctx** out);
void pct_destroy(pct_ctx* ctx);
const char* pct_last_error(const pct_ctx* ctx);    /* never NULL */
const char* pct_version(void);

/* ---- cloud upload: PointCloud.__init__ / read_from_file (pct:26-66) ----- */
/* (n,3) row-major host coordinates.  The float32 form is the file path's
 * dtype (pct:52); the float64 form keeps native-dtype queries and centring
 * (pct:83, pct:641) while the search structure holds float32-rounded
 * coordinates (pct:74). */
int pct_set_points_f32(pct_ctx* ctx, const float* xyz, int64_t n);
int pct_set_points_f64(pct_ctx* ctx, const double* xyz, int64_t n);
/* Same, from a device pointer on this handle's device (multi-GPU: the buffer
 * an RCCL all-gather has just filled). */
int pct_set_points_device_f32(pct_ctx* ctx, const void* dev_xyz, int64_t n);
/* Same without the copy: the handle reads the caller's buffer in place.  The
 * buffer must stay allocated and unchanged until the next pct_set_points_* /
 * pct_use_points_* call on this handle or pct_destroy, and whatever filled it
 * must have completed (the handle's stream does not wait for other streams). */
int pct_use_points_device_f32(pct_ctx* ctx, const void* dev_xyz, int64_t n);
/* Queries owned by this handle: global index range [begin, end).  Default all. */
int pct_set_query_range(pct_ctx* ctx, int64_t begin, int64_t end);
/* Ownership by SLAB instead of by index range (multi-GPU, clouds whose row order is not a spatial order: the
 * neighbourhood of a random index range is the whole cloud, so every rank would bin every point).  The gathered cloud
 * is cut into `parts` slabs of equal population along its longest axis -- from a 4096-bin histogram that every rank
 * computes alike, with the same arithmetic on the same bytes -- and this handle answers the points of slab `part`:
 * its cell list holds that slab and a margin (checked per query like an index range's box, pct_timings.limit_retries).
 * pct_curvature only (float32 clouds of >= 4096 points, one cell list: PCT_KNN_AUTO / PCT_KNN_GRID; k > 127 goes
 * through the exact sweep); the rows come back as records, not by index:
 *   pct_slab_counts    points per slab of the last pct_curvature (what every rank will send)
 *   pct_slab_records   (public index as int32 bits, K, H) x rows of this slab -> a DEVICE buffer of 3 floats per row
 *   pct_scatter_records   gathered records (device) -> K, H of the public rows [begin, end) (device); fails unless
 *                         exactly end - begin records fell into the range (the slabs of the ranks partition the cloud)
 * parts = 1 is the same path with the whole cloud as its one slab (a world of one rank); pct_set_query_range, a new
 * cloud or parts <= 0 return the handle to index ranges.  pct_get_fit / pct_get_neighbors and
 * the other by-index getters refuse while slab ownership is on. */
#define PCT_SLAB_PARTS_MAX 64
int pct_set_query_slab(pct_ctx* ctx, int32_t part, int32_t parts);
int pct_slab_counts(pct_ctx* ctx, int64_t* counts, int32_t parts);
int pct_slab_records(pct_ctx* ctx, float* dev_records, int64_t capacity_rows, int64_t* rows);
int pct_scatter_records(pct_ctx* ctx, const float* dev_records, int64_t n_records, int64_t begin, int64_t end,
                        float* dev_K, float* dev_H);
/* Cell-occupancy target of the grid search as a multiple of (k+1); <= 0 keeps
 * the default. */
int pct_set_grid_param(pct_ctx* ctx, double occupancy_factor);
/* Sweep statistics in pct_timings (ring_fallbacks ... redone_queries, redo_adopted); off by default
 * because the counters cost same-address atomics. */
int pct_set_stats(pct_ctx* ctx, int32_t enable);

/* ---- plant_kdtree(k) (pct:69-89) ---------------------------------------- */
/* k nearest neighbours of every owned point, self dropped, rows ascending.
 * eps > 0 adds the hybrid bound "distance < eps" (SURVEY A11); rows then carry
 * a valid count, missing slots index N / distance +inf. */
int pct_knn(pct_ctx* ctx, int32_t k, double eps, int32_t algo);
/* Lazy download of the neighbour table for rows [begin,end) of the cloud:
 * idx (rows,k) int32, dist (rows,k) float32, count (rows) int32 (any may be NULL). */
int pct_get_neighbors(pct_ctx* ctx, int64_t begin, int64_t end,
                      int32_t* idx, float* dist, int32_t* count);

/* Same for an explicit list of cloud rows (sampled checks on clouds whose full table is tens of GB). */
int pct_get_neighbor_rows(pct_ctx* ctx, const int64_t* rows, int64_t n_rows,
                          int32_t* idx, float* dist, int32_t* count);

/* ---- fit_explicit_quadratic_surfaces_to_neighborhoods (pct:635-647)
 *      + calculate_curvatures_of_explicit_quadratic_surfaces_for_all_points
 *        (pct:657-674) ---------------------------------------------------- */
/* From the device-resident neighbour table left by pct_knn. */
int pct_fit(pct_ctx* ctx);
/* From host-supplied neighbours: idx (rows,k) int32 for query points
 * query[rows] (NULL = 0..rows-1), optional per-row valid count.  The results replace those of an
 * earlier fit; a resident neighbour table stays as it is (pct_get_neighbors / pct_fit keep working), and so do the areas.
 * Refused on a slab handle, as pct_fit is: the results of a slab pass are read as records, never replaced row by row. */
int pct_fit_indices(pct_ctx* ctx, const int32_t* idx, const int32_t* count,
                    const int64_t* query, int64_t rows, int32_t k);
/* Diagnostics variant of pct_fit_indices: the same neighbourhoods through the same kernel, but the
 * solution of the normal equations is returned unrounded (float64, where pct:359 casts to float32) and K, H are the
 * formulas of pct:403-419 evaluated in float64 from it.  The design matrix stays float32 (pct:350, 358): this shows
 * what the float32 rounding of the last two stages costs, not a different algorithm.  coefs (rows,6), K, H (rows)
 * float64 host arrays.  Leaves the resident neighbour table and float32 results untouched. */
int pct_fit_indices_f64(pct_ctx* ctx, const int32_t* idx, const int32_t* count,
                        const int64_t* query, int64_t rows, int32_t k,
                        double* coefs, double* K, double* H);
/* plant_kdtree + compute_pointwise_explicit_quadratic_curvature (pct:505-509)
 * without materialising the neighbour table on the host. */
int pct_curvature(pct_ctx* ctx, int32_t k, double eps, int32_t algo);

/* Results of the last fit for cloud rows [begin,end) (pct_fit / pct_curvature)
 * or for the rows of the last pct_fit_indices call.  Any pointer may be NULL.
 * coefs (rows,6) float32 [A,B,C,D,E,F]; K, H, H2 (rows) float32. */
int pct_get_fit(pct_ctx* ctx, int64_t begin, int64_t end,
                float* coefs, float* K, float* H, float* H2);

/* calculate_explicit_quadratic_curvatures (pct:398-431) on caller-supplied
 * coefficients: coefs (rows,6) float32 host -> K, H, H2 (rows) float32 host. */
int pct_curvatures_from_coefficients(pct_ctx* ctx, const float* coefs, int64_t rows,
                                     float* K, float* H, float* H2);

/* The two per-neighbourhood staticmethods of the class on their own, batched (batch neighbourhoods of m points):
 * get_best_fit_plane_and_rotate (pct:270-321): nbrs (batch, m, 3) float32 (is_f64 == 0) or float64 ->
 * rotated (batch, m, 3) float64: np.cov in float64 (ddof 1), normal = direction of least variance, flipped by
 * points[-1] - points[0] (subtracted in the input's dtype), Rodrigues rotation of the normal onto +z, R p per point.
 * PCT_ERR_NONFINITE for NaN/Inf in the input (pct:273) -- the caller checks the output (pct:318).  m >= 2. */
int pct_plane_rotate(pct_ctx* ctx, const void* nbrs, int32_t is_f64, int64_t batch, int32_t m, double* rotated);
/* fit_quadratic_surface (pct:331-360): pts (batch, m, 3) float32 (the cast of pct:350 is the caller's) ->
 * coefs (batch, 6) float32: numpy.linalg.lstsq(rcond=None) of the float32 design rows [a^2, b^2, ab, a, b, 1] --
 * float64 SVD-based solve, singular values below eps max(m, 6) sigma_1 cut off, minimum-norm solution. */
int pct_fit_quadric(pct_ctx* ctx, const float* pts, int64_t batch, int32_t m, float* coefs);

/* self.kdtree.query(x, k[, distance_upper_bound=eps]) (the reference's tree object, pointCloudToolbox.py:74; called
 * with arbitrary points at pct:625, 759, 844): the k nearest CLOUD points of each of m caller-supplied float64 query
 * points -- nothing is dropped (a query that coincides with a cloud point gets that point first, distance 0).
 * The cloud is the float32-rounded one the tree is built from (pct:74); squared distances are accumulated in float64
 * as ((dx^2 + dy^2) + dz^2), rows ascending, exact ties by index.  idx (m,k) int32, dist (m,k) float64; missing
 * entries (k > N, or beyond eps when eps > 0): index N and +inf, as SciPy pads.  1 <= k <= 128.
 * Exhaustive sweep, one wave per query, reading all N cloud points for each: what the hundreds of sample points of
 * the neighbour study want.  The points of another cloud go through pct_query_points_algo below, which sends large
 * query sets through the cell list; a cloud's own points are pct_knn's. */
int pct_query_points(pct_ctx* ctx, const double* q_xyz, int64_t m, int32_t k, double eps,
                     int32_t* idx, double* dist);

/* The same rows with the path named.  PCT_QUERY_SWEEP: pct_query_points' exhaustive sweep.  PCT_QUERY_GRID: the
 * uniform cell list -- the resident one where a whole-cloud list is in place, else one built by this call and left
 * resident --, queries binned by cell, the 27-cell stencil of a cell staged once for its queries, an exact shell-by-
 * shell sweep for the queries the stencil cannot vouch for.  It takes the exhaustive sweep instead (same rows) where
 * the table in place came from the hierarchical list or the chain of cell lists, on a handle with an owned range, and
 * where a table or fit results in place would be invalidated by a build.  PCT_QUERY_AUTO: the sweep below 1024
 * queries, below 4096 cloud points and below m * N = 2^34 pairs (the measured crossover); the cell list
 * from there on.  A refusal of the cell-list build is returned, not rerouted.
 * Errors as pct_query_points; PCT_ERR_INVALID for an unknown algo.  The resident neighbour table, fit results and
 * PCA results are untouched. */
#define PCT_QUERY_AUTO 0
#define PCT_QUERY_SWEEP 1
#define PCT_QUERY_GRID 2
int pct_query_points_algo(pct_ctx* ctx, const double* q_xyz, int64_t m, int32_t k, double eps, int32_t algo,
                          int32_t* idx, double* dist);
/* Of the last pct_query_points_algo call: out = {route: 0 exhaustive sweep, 1 resident cell list, 2 cell list built by
 * the call; queries answered from the staged 27-cell stencil; queries redone by the exact sweep; largest ring of cells
 * a query reached}.  Zeros after the exhaustive sweep. */
int pct_query_stats(pct_ctx* ctx, int64_t out[4]);

/* self.kdtree.query_ball_point(x, r): every cloud point within r of each of m caller-supplied float64 query points, as
 * CSR rows of any length.  Candidates are the float32-rounded cloud widened to float64 (pct:74), as in
 * pct_query_points; d2 = (dx*dx + dy*dy) + dz*dz in float64, three separate operations, nothing fused.  A point is a
 * member when d2 <= r*r, the product taken in float64: the test is INCLUSIVE -- unlike the strict d < eps of
 * pct_query_points' bound.  Nothing else is special-cased: r = 0 keeps coinciding points, r = inf every point, a NaN r
 * nothing, a negative r behaves as |r| (as SciPy's tree does); a query that coincides with a cloud point gets that
 * point.  r: n_r = 1 radius for all queries, or n_r = m, one per query.
 * Row i is the set of public indices that pass: ascending with PCT_BALL_SORTED, otherwise in an unspecified order that
 * the same call on the same handle state reproduces byte for byte.  PCT_BALL_DISTANCES: float64 sqrt(d2) beside every
 * index.  PCT_BALL_COUNT_ONLY: offsets alone, nothing is filled or kept.
 * offsets (m + 1, host) is complete on return from PCT_OK, PCT_ERR_LIMIT and PCT_ERR_OOM.  offsets[m] > max_entries
 * (max_entries <= 0: no cap) returns PCT_ERR_LIMIT: no rows are resident, the caller chunks its queries by the offsets.
 * PCT_ERR_OOM: the row buffer could not be reserved.  m = 0 is accepted (offsets = {0}).  PCT_ERR_NONFINITE for a
 * non-finite query coordinate; PCT_ERR_INVALID for an unknown algo or flag, n_r other than 1 or m, a slab handle.
 * algo: PCT_QUERY_SWEEP reads all N points per query; PCT_QUERY_GRID goes through the uniform cell list -- the resident
 * one, or one built by this call and left resident -- and falls back to the exhaustive path exactly where
 * pct_query_points_algo does; PCT_QUERY_AUTO takes the cell list from 1024 queries, 4096 points and 2^26 pairs m N on.
 * The rows are the same on every path.  They stay on the device until the next pct_query_ball or pct_set_points*; the
 * resident neighbour table, fit results, PCA results and their timings are untouched. */
#define PCT_BALL_SORTED 1
#define PCT_BALL_DISTANCES 2
#define PCT_BALL_COUNT_ONLY 4
int pct_query_ball(pct_ctx* ctx, const double* q_xyz, int64_t m, const double* r, int64_t n_r, int32_t flags, int32_t algo,
                   int64_t max_entries, int64_t* offsets);
/* Rows [row_begin, row_end) of the last pct_query_ball: idx holds offsets[row_end] - offsets[row_begin] entries, dist
 * (may be NULL; needs PCT_BALL_DISTANCES) as many.  PCT_ERR_INVALID without resident rows. */
int pct_get_ball(pct_ctx* ctx, int64_t row_begin, int64_t row_end, int32_t* idx, double* dist);
/* Of the last pct_query_ball: out = {route as pct_query_stats; queries answered from a cube of cells staged once for
 * their work item; queries that streamed their candidates from global memory; largest cube half-width in cells}.
 * Zeros behind the route after the exhaustive path. */
int pct_ball_stats(pct_ctx* ctx, int64_t out[4]);

/* Curvature over radius neighbourhoods: the quadric fit (pct:635-647, 657-674) of the m resident rows of the last
 * pct_query_ball, row i about the cloud point c = self_rows[i] (a public index in [0, n)) -- "every point within r", at any
 * row length, where pct_fit / pct_fit_indices take a rectangular table of at most 511 neighbours.
 * Members of row i: its entries e != c.  Only the centre's own index is skipped: a coinciding twin of the centre is a
 * member.  An entry outside [0, n) is never dereferenced; the row reads NaN.
 * Key: key(e) = (d2(e), e) with d2 = (dx*dx + dy*dy) + dz*dz in float64, three separate operations, nothing fused, dx = the
 * float32-rounded record of e widened to float64 minus the centre's coordinate -- native float64 for float64 clouds, else
 * the float32 value widened: pct_query_ball's expression with the centre as the query.  near / far = the member with the
 * smallest / largest key.
 * Result: get_best_fit_plane_and_rotate, fit_quadratic_surface and calculate_explicit_quadratic_curvatures (pct:270-321,
 * 331-360, 398-431) applied to the block points[ranked] - points[c], centred in the cloud's native dtype (pct:641), ranked =
 * the members ascending by key: pct:286's points[-1] - points[0] is far - near in the native dtype, every other step is a
 * sum over the members and does not depend on their order (up to the rounding of fp64 sums).
 * Fewer than 2 members: NaN coefficients, K, H and H^2 (np.cov of one point).  Fewer than 6 members, or normal equations
 * whose Cholesky pivot ratio falls below the fit's threshold: numpy.linalg.lstsq's minimum-norm (gelsd) answer, by the
 * solver pct_fit uses for such rows.
 * Outputs: coefficients (m,6), K, H, H^2 row-aligned; they replace the results of an earlier fit exactly as
 * pct_fit_indices' do and are read with pct_get_fit(ctx, 0, m, ...).  used (host, m entries, may be NULL): members fitted
 * per row.  The resident ball rows, the resident neighbour table, PCA results and the cell list are untouched;
 * pct_timings.fit_ms and fit_svd_rows describe this call.  Works on sorted and unsorted rows, with or without
 * PCT_BALL_DISTANCES; the same rows in the same order give the same bytes.  Under pct_set_async it first waits for a
 * pending call, like every blocking entry point.
 * PCT_ERR_NO_NEIGHBORS without resident rows (none queried, a PCT_BALL_COUNT_ONLY or capped query, a new cloud since);
 * PCT_ERR_INVALID when m is not the row count of the last query, for a centre outside [0, n), for a slab handle.
 * Environment, read per call: PCT_FIT_BALL_ROUTE=wave|table forces one of the two device routes (A/B runs). */
int pct_fit_ball(pct_ctx* ctx, const int64_t* self_rows, int64_t m, int32_t* used);

/* explicit_quadratic_neighbor_study (pct:732-800), the numeric part: for every sample row s and every
 * neighbour count n in [n_lo, n_hi], the Gaussian curvature of the quadric fitted to the point itself plus
 * its n nearest neighbours (pct:759-761).  Needs a resident plain k-NN table with k >= n_hi.
 * K_out: (n_samples, n_hi - n_lo + 1) float32.  The bisection over n stays on the host. */
int pct_neighbor_study_curvatures(pct_ctx* ctx, const int64_t* sample_rows, int64_t n_samples,
                                   int32_t n_lo, int32_t n_hi, float* K_out);

/* load_mesh_compute_energies (utils.py:702-765), the consumer of K/H: bending energy sum(mean(H^2) * area),
 * stretching energy sum(mean(K) * area) (both nansum) and total area over a triangle mesh.  vertices (V,3)
 * float64, triangles (T,3) int32, curvature arrays (V) float32 (curvature_is_f64 == 0, what the path
 * produces) or float64 (1); the two arrays may differ (2: K float64, H float32; 3: K float32, H float64).  Each face
 * mean is taken in the dtype of its own array, as NumPy does.  No triangles: zeros.  out3 = {bending, stretching, area}. */
#define PCT_MESH_F32 0
#define PCT_MESH_F64 1
#define PCT_MESH_K64_H32 2
#define PCT_MESH_K32_H64 3
int pct_mesh_energies(pct_ctx* ctx, const double* vertices, int64_t n_vertices, const int32_t* triangles,
                      int64_t n_triangles, const void* gaussian, const void* mean, int32_t curvature_is_f64,
                      double* out3);

/* Mesh-free energies.  calculate_energies(voronoi_areas, gaussian_curvature, mean_curvature) (pct:650-655) sums
 * (h ** 2) * area and k * area over per-point areas that nothing in the reference produces.  pct_point_areas produces
 * them from the rows of the resident neighbour table (pct_knn / pct_curvature; owned rows, eps counts and rows of up to
 * 511 neighbours included): the area of every point's Voronoi cell in its own tangent plane.  Row i, count_i neighbours:
 *   block   Q_j = p_j - p_i, centred in the cloud's dtype (pct:641), float64 from there on;
 *   frame   R = the rotation pct_fit takes for this row (pct:270-312); (a_j, b_j) = the first two components of R Q_j;
 *   bound   L^2 = max_j |Q_j|^2;
 *   cell    the square [-L, L]^2 cut by the half-plane a_j x + b_j y <= rho_j^2 / 2 of every neighbour with
 *           rho_j^2 = a_j^2 + b_j^2 > 0, in row order (rho_j^2 == 0 -- a coinciding point, or one straight along the
 *           normal -- cuts nothing: each of two twins keeps its full cell);
 *   area    (float64) the shoelace area of the polygon left; nverts (int32) its vertex count; closed (uint8) 1 iff it has
 *           at least 3 vertices and every one of them has x^2 + y^2 < L^2 (independent of the in-plane basis).  A row that
 *           is not closed is open -- the rim of an open surface, k too small, fewer than 3 neighbours -- and reports the
 *           area of the square as far as it was cut;
 *   NaN     count_i < 2, a frame that is not finite: area NaN, closed 0, nverts 0 -- the rows whose fit is NaN.
 * PCT_ERR_NO_NEIGHBORS without a resident table, as pct_fit.  A new cloud, owned range or planting drops the areas, as it
 * drops the fit.  pct_timings is untouched (its size is part of the ABI): pct_point_area_profile has the time. */
int pct_point_areas(pct_ctx* ctx);
/* Cloud rows [begin, end) of the owned range; any pointer may be NULL.  PCT_ERR_INVALID without areas. */
int pct_get_point_areas(pct_ctx* ctx, int64_t begin, int64_t end, double* area, uint8_t* closed, int32_t* nverts);
/* Of the last pct_point_areas: out = {rows, closed rows, NaN rows, rows whose polygon outgrew the fast kernel's vertex
 * capacity and were redone with room for k + 4 vertices (the same code, the same result)}. */
int pct_point_area_stats(pct_ctx* ctx, int64_t out[4]);
/* ... and out = {device milliseconds of its kernels (hipEvent), neighbours that passed the rejection test, summed over
 * the rows -- the cuts that were actually examined}. */
int pct_point_area_profile(pct_ctx* ctx, double out[2]);
/* calculate_energies (pct:650-655) on the device: out = {bending = sum (double)H2_i * A_i with H2 the fit's float32
 * h ** 2 (pct:652), stretching = sum (double)K_i * A_i (pct:653), area = sum A_i, rows used}, over the owned rows whose
 * area, K and H are no NaN -- closed_only != 0: and whose cell is closed.  float64 sums in a fixed order over the table's rows (per-
 * block partials, then one block): the same bytes for the same resident table; another planting may order the rows of a
 * cell differently, and the sums then differ in their last bits.  Needs the fit (pct_fit / pct_curvature) and the areas of the
 * table in place: PCT_ERR_INVALID "no fit results" / "no point areas" otherwise. */
int pct_point_energies(pct_ctx* ctx, int32_t closed_only, double out[4]);

/* Per-point surface frames from the quadric fit.  The fit builds, for every row, a tangent-plane rotation R and a patch
 * z = A a^2 + B b^2 + C ab + D a + E b + F, and keeps K and H.  pct_point_frames keeps the rest: the fitted normal, the
 * principal curvatures k1 >= k2 (calculate_explicit_quadratic_curvatures returns them per call, pct:425-431) and their
 * directions, and -- with a viewpoint -- one side of the surface for all rows.  It needs the resident table (else
 * PCT_ERR_NO_NEIGHBORS) and the fit of that table (pct_fit / pct_curvature; else PCT_ERR_INVALID "no fit results", the
 * condition of pct_point_energies).  Row i of the table, count_i = m valid neighbours:
 *   block   Q_j = p_j - p_i, centred in the cloud's dtype (pct:641), float64 from there on;
 *   R       the rotation pct_fit takes for this row (pct:270-312), from the same moments in the same order (PCT_FIT_JACOBI
 *           applies as in the fit);
 *   coefs   (A, B, C, D, E) = the row's float32 fit coefficients, widened to float64; nothing is fitted again;
 *   patch normal   w = sqrt((1 + D D) + E E), m = (-D, -E, 1) / w: the unit normal of the patch at a = b = 0, on the +z
 *           side of the rotated frame;
 *   tangent basis  g2 = 1 + D D, g = sqrt(g2), e1 = (1, 0, D) / g, e2 = m x e1 = (-D E, g2, E) / (g w);
 *   second fundamental form   for tangent vectors given by their first two components,
 *           II(x, y) = ((2A xa ya + C (xa yb + xb ya)) + 2B xb yb) / w;
 *   shape operator   the symmetric S = [[s11, s12], [s12, s22]], s11 = II(e1, e1), s12 = II(e1, e2), s22 = II(e2, e2); in
 *           exact arithmetic tr S = 2H and det S = K of pct:416-419;
 *   principal curvatures   h = (s11 + s22) / 2, d = (s11 - s22) / 2, r = sqrt(d d + s12 s12): k1 = h + r, k2 = h - r;
 *   principal directions in the rotated frame   the rotation that annihilates s12, Jacobi's small root, no atan2:
 *           t = s12 / (|d| + r), cj = 1 / sqrt(t t + 1), sj = t cj, (c, s) = (cj, sj) where d > 0 and (sj, cj) otherwise;
 *           t1 = c e1 + s e2 belongs to k1, t2 = -s e1 + c e2 to k2.  r == 0 exactly (umbilic): t1 = e1, t2 = e2; such
 *           rows are counted;
 *   world frame   n = R^T m, d1 = R^T t1, d2 = R^T t2 (component i: (R[0][i] v0 + R[1][i] v1) + R[2][i] v2); d1 and d2
 *           under the sign rule of pct_get_pca: the component of largest magnitude is positive, the first among equals;
 *   viewpoint (optional)   v, three doubles in the cloud's own coordinates.  Where
 *           ((vx - px) n0 + (vy - py) n1) + (vz - pz) n2 < 0, p = p_i in the cloud's native dtype widened:
 *           n <- -n, (k1, k2) <- (-k2, -k1), (d1, d2) <- (d2, d1), flipped = 1;
 *   without a viewpoint   n stays on the side the fit's own far-minus-near rule chose (pct:286-297) -- the side the fit's
 *           H is signed against, which jumps from point to point -- and flipped = 0.  Either way H and k1, k2 are signed
 *           relative to n: with a viewpoint, H_signed = flipped ? -H : H;
 *   NaN rows   m < 2, a table entry outside the cloud, a non-finite R or coefficient: every output of the row is NaN and
 *           flipped = 0.  Such rows are counted.
 * A non-finite viewpoint: PCT_ERR_INVALID.  A new cloud, owned range, planting or fit drops the frames.  pct_timings is
 * untouched: pct_point_frame_stats has the time. */
int pct_point_frames(pct_ctx* ctx, const double* viewpoint /* 3 doubles or NULL */);
/* Cloud rows [begin, end) of the owned range, float64 host arrays: normal (rows, 3), k12 (rows, 2) = [k1, k2], dirs
 * (rows, 3, 2) C order with d1, d2 as columns (as pct_get_pca delivers its frame), flipped (rows) uint8; any pointer may
 * be NULL.  PCT_ERR_INVALID without frames. */
int pct_get_point_frames(pct_ctx* ctx, int64_t begin, int64_t end, double* normal, double* k12, double* dirs, uint8_t* flipped);
/* Of the last pct_point_frames: out = {rows, NaN rows, flipped rows, umbilic rows}; *ms (may be NULL) the device
 * milliseconds of its kernel (hipEvent). */
int pct_point_frame_stats(pct_ctx* ctx, int64_t out[4], double* ms);

/* Consistent normal orientation.  The fit picks a side per row (pct:286-297), and one viewpoint orients only what is seen
 * from it; pct_orient_frames turns the resident frames of a whole-cloud handle so that neighbouring rows agree, by a
 * level-synchronous flood over the resident neighbour table (the role of Open3D's
 * orient_normals_consistent_tangent_plane in the reference's pipeline, utils:80).  Every choice is a keyed 64-bit maximum:
 * the result is a pure function of the normals as they stand before the call and of the table, whatever order either is
 * stored in.  tests/orient_exact.py states it again in NumPy.
 *   valid     a row whose normal holds no NaN.  Invalid rows are never labelled, never parents, and keep every output;
 *   entries   of row i: its table entries before its eps count that are records of the cloud.  The graph is undirected:
 *             i ~ j when j is an entry of row i or i one of row j;
 *   claim     a labelled row p on an unlabelled valid row c: dot = (n_p0 n_c0 + n_p1 n_c1) + n_p2 n_c2 in float64, nothing
 *             fused; key = (uint64(bits of (float)|dot|) << 32) | (0xFFFFFFFF - public index of p).  The largest key wins
 *             (the best aligned parent, the lowest index among equals); c takes toggle[c] = toggle[p] XOR (dot < 0),
 *             parent p, level[p] + 1 and p's component;
 *   flood     until no unlabelled valid row is left or max_components components exist:
 *               seed   the unlabelled valid row of lowest public index: toggle 0, level 0, parent -1, the next component
 *                      id (ids count up from 0);
 *               push   every row labelled in the previous level claims the unlabelled valid entries of its own row; all
 *                      claims of a level are in before any is decided; until a level labels nothing;
 *               pull   once: every unlabelled valid row claims for itself from the entries of its own row that carry this
 *                      component's id, the entry as parent.  Rows labelled: they are the next frontier, push again; none:
 *                      the component is complete.  This reaches an outlier that lists the surface while nothing lists it;
 *   anchor    each component may be turned as a whole.  PCT_ORIENT_SEED: as flooded.  PCT_ORIENT_TOP (Hoppe's rule): the
 *             component's row of largest z of its float32 record (-0 = +0), lowest public index among equals; its oriented
 *             normal has n_z < 0: every toggle of the component is inverted.  PCT_ORIENT_VIEW: with the oriented normal,
 *             s = ((vx - px) n0 + (vy - py) n1) + (vz - pz) n2 (pct_point_frames' expression, p in the cloud's dtype); rows
 *             with s < 0 face away, rows with s > 0 face the viewpoint; more away than facing: inverted; a tie leaves it;
 *   apply     every row with toggle 1, exactly as pct_point_frames' flip: n <- -n, (k1, k2) <- (-k2, -k1), (d1, d2) <-
 *             (d2, d1), flipped ^= 1; H_signed = flipped ? -H : H keeps holding.  Rows beyond max_components stay
 *             untouched with component -1.
 * PCT_ERR_INVALID "no point frames" without resident frames; PCT_ERR_INVALID for an owned range or slab handle, an unknown
 * anchor, or PCT_ORIENT_VIEW without a finite viewpoint.  max_components <= 0: 65536.  A new cloud, owned range, planting,
 * fit or pct_point_frames call drops the orientation; a refused pct_orient_frames does not (the orientation of an earlier
 * call and the frames it turned stay as they are).  The flood reads the resident table: PCT_ERR_INVALID without one (after
 * pct_voxel_downsample).  pct_get_point_frames serves the turned frames; pct_point_frame_stats keeps describing the
 * pct_point_frames call.  pct_timings is untouched. */
#define PCT_ORIENT_SEED 0
#define PCT_ORIENT_TOP  1
#define PCT_ORIENT_VIEW 2
int pct_orient_frames(pct_ctx* ctx, int32_t anchor, const double* viewpoint /* 3 doubles or NULL */, int32_t max_components);
/* Cloud rows [begin, end): component, parent, level int32 (-1 where unlabelled; a seed's parent is -1), toggled uint8 (the
 * row was turned by the call, the anchor included); any pointer may be NULL.  PCT_ERR_INVALID without an orientation. */
int pct_get_orientation(pct_ctx* ctx, int64_t begin, int64_t end, int32_t* component, int32_t* parent, int32_t* level, uint8_t* toggled);
/* Of the last pct_orient_frames: out = {valid rows, components, rows left unlabelled, toggled rows, push levels that labelled
 * a row (summed over the components), pull rounds that labelled a row, kernel launches, host waits}; *ms (may be NULL) the
 * device milliseconds between two events around the call's work. */
int pct_orient_stats(pct_ctx* ctx, int64_t out[8], double* ms);

/* ---- scan preparation (next row N4) ---------------------------------------- */
/* Voxel-grid down-sampling of convert_asc_to_ply.py:20-51: voxel = floor(coordinate / voxel_size) evaluated in the
 * coordinates' own dtype as NumPy does (the _f32 form divides by (float)voxel_size in float32), the
 * first point of every voxel is kept.  indices (caller-allocated, n entries) receives the kept input indices in
 * increasing order (= the reference's order of first occurrence), *count their number.  Works on any handle, with or
 * without a resident cloud; it borrows the cell list's scratch buffers, so a resident neighbour table is dropped
 * (plant it again before pct_fit / pct_get_neighbors); fit results, areas, frames and the orientation already computed
 * stay readable, whichever sweep planted the table (state rules above). */
int pct_voxel_downsample(pct_ctx* ctx, const double* xyz, int64_t n, double voxel_size, int64_t* indices, int64_t* count);
int pct_voxel_downsample_f32(pct_ctx* ctx, const float* xyz, int64_t n, double voxel_size, int64_t* indices, int64_t* count);
/* PCA surface variation as utils.py:778-829 DOCUMENTS it, for the loaded cloud: k_total neighbours including the point
 * itself, out[i] = lambda_min / (lambda_0 + lambda_1 + lambda_2 + 1e-10) of their 3 x 3 covariance, (owned rows)
 * float32.  (As WRITTEN, utils.py:822 builds the k x k Gram matrix, whose smallest eigenvalue is zero: the function
 * returns LAPACK round-off around 0.  The Python wrapper's default follows the code as written -- zeros -- and offers
 * this estimator as an option.) */
int pct_surface_variation(pct_ctx* ctx, int32_t k_total, float* out);

/* ---- principal_curvatures_via_principal_component_analysis (pct:901-950) ------------------------------------- */
/* For every point of the loaded (whole) cloud: its k nearest points as the reference ranks them --
 * np.linalg.norm(points - point, axis=1) in the cloud's dtype, the nearest entry (the point itself or a duplicate of it)
 * dropped; k >= N takes N - 1 --, np.cov of their raw coordinates in float64 (about their own mean, ddof 1), its
 * eigen-decomposition: lambda_1 >= lambda_2 the two largest eigenvalues, their eigenvectors, K = lambda_1 lambda_2,
 * H = (lambda_1 + lambda_2) / 2.  Kept on the device for pct_get_pca.  2 <= min(k, N - 1) <= 511, else PCT_ERR_INVALID;
 * PCT_ERR_NONFINITE for any non-finite coordinate.  algo: the sweep that fetches the candidates (pct_knn_algo; every
 * choice gives the same bits).  Float32 clouds: near-ties of the float32 norm at the k-th place may resolve differently
 * from NumPy's argsort.  Float64 clouds: ranked by float64 distances; the sweep ranks the cloud recentred on its first
 * point and rounded to float32, rows it cannot vouch for go through an exhaustive float64 pass (O(N) per row),
 * *exact_rows (may be NULL) counts them.  That pass is limited to 2^30 point visits (rows x N): beyond, PCT_ERR_INVALID
 * with the reason, before it runs -- k = 511 on a float64 cloud of more than ~32 000 points (no room for candidates
 * beyond k), or float32 rounding of the recentred cloud that is not small against the neighbour spacing.  keep_neighbors != 0 keeps every row's
 * neighbour indices for pct_get_pca.  Like pct_surface_variation this REPLACES the neighbour table and drops the fit
 * results of the handle: a caller that keeps those runs it on a handle of its own. */
int pct_pca_curvatures(pct_ctx* ctx, int32_t k, int32_t algo, int32_t keep_neighbors, int64_t* exact_rows);
/* Rows [begin, end) of the last pct_pca_curvatures, float64 host arrays (any pointer may be NULL): l1, l2, K, H (rows),
 * dirs (rows, 3, 2) C order -- column 0 the eigenvector of lambda_1, column 1 that of lambda_2, each with its component
 * of largest magnitude positive (the reference's signs are LAPACK's) -- and idx (rows, k) int32, the neighbours used. */
int pct_get_pca(pct_ctx* ctx, int64_t begin, int64_t end, double* l1, double* l2, double* dirs, double* K, double* H,
                int32_t* idx);

/* ---- ingest / egress around the path (host code, no device needed) ------- */
/* The text scans read_from_file parses with np.loadtxt (pct:51): rows x cols of whitespace-separated numbers,
 * '#' comments and blank lines skipped.  Values are correctly rounded float64 (what Python's float() gives). */
int pct_text_shape(const char* path, int64_t* rows, int32_t* cols);
int pct_text_load(const char* path, int64_t rows, int32_t cols, double* out);
/* The constructor's three matrix norms (pct:45-47) from one multi-threaded pass over the (N, 3) array: out10 =
 * {sum|x|, sum|y|, sum|z| (float64), largest row sum (|x| + |y|) + |z| in the array's dtype, Gram matrix xx xy xz yy yz
 * zz (float64)}; the spectral norm is the square root of the Gram matrix' largest eigenvalue.  NaN input: NaN out. */
int pct_matrix_norms_f32(const float* xyz, int64_t n, double* out10);
int pct_matrix_norms_f64(const double* xyz, int64_t n, double* out10);
/* repr(float(x)) as Python prints it -- what an f-string gives for a np.float32 widened to double -- into out32
 * (>= 32 bytes, not NUL-terminated); returns the length. */
int pct_format_float(double x, char* out32);
/* The ASCII PLY of utils.py:538-551: header + one line 'x y z K H' per vertex, numbers as the reference's f-string
 * prints them. */
int pct_write_ply_ascii(const char* path, const float* xyz, const float* gaussian, const float* mean, int64_t n);
/* export_ply_with_curvature_and_normals (pct:699-726) without faces: header + one line 'x y z nx ny nz K H' per vertex
 * (normals (n, 3) float32), numbers in pct_write_ply_ascii's format. */
int pct_write_ply_ascii_normals(const char* path, const float* xyz, const float* normals, const float* gaussian,
                                const float* mean, int64_t n);

/* ---- multi-GPU exchange --------------------------------------------------------------------------
 * The reference is one process; here the cloud shards by point-index range over up to 8 GPUs, one process per GPU,
 * and the only exchange is an all-gather of the float32 coordinate shards (12 B / point): RCCL over xGMI, called from
 * this library (librccl.so is opened at run time; no PyTorch in the process).  Rank 0 creates the unique id and the
 * host code hands its 128 bytes to every rank (point-cloud-toolbox_amd/dist.py: a TCP socket on MASTER_ADDR). */
int pct_comm_unique_id(void* id128);
int pct_comm_init(pct_ctx* ctx, int32_t rank, int32_t world, const void* id128);
int pct_comm_destroy(pct_ctx* ctx);
/* Rank r contributes counts[r] floats at dev_send; dev_recv receives all shards back to back in rank order.
 * Asynchronous: runs on the handle's exchange stream, ordered after the work the compute stream holds at the call.
 * One exchange in flight per handle: a second call before pct_comm_wait / pct_comm_synchronize is PCT_ERR_INVALID.
 * Equal shards: ncclAllGather into dev_recv; unequal ones (zero-sized too): shards padded to the largest, one
 * ncclAllGather, one compaction pass.  PCT_COMM_FORCE=allgather|padded|bcast (environment) picks the form. */
int pct_comm_allgather_f32(pct_ctx* ctx, const void* dev_send, void* dev_recv, const int64_t* counts);
/* Collectives issued so far by this handle: out4 = {ncclAllGather in place, padded ncclAllGather + compaction, groups
 * of per-rank ncclBroadcast, ncclAllReduce}. */
int pct_comm_counters(pct_ctx* ctx, int64_t* out4);
/* The compute stream waits for the last exchange on the device (the host does not block) ... */
int pct_comm_wait(pct_ctx* ctx);
/* ... or the host does. */
int pct_comm_synchronize(pct_ctx* ctx);
/* values[0..n) reduced over the ranks in place (op 0 sum, 2 max, 3 min; n <= 8); blocking, also drains this handle's
 * compute stream first: with n == 0 it is the barrier of the bench's timed region. */
int pct_comm_allreduce_f64(pct_ctx* ctx, double* values, int32_t n, int32_t op);

/* ---- measurement -------------------------------------------------------- */
int pct_get_timings(const pct_ctx* ctx, pct_timings* out);
/* Streams of clouds.  With pct_set_async(ctx, 1) a pct_curvature call on a whole-cloud handle (no query range or slab,
 * statistics off) returns as soon as its kernels are enqueued: the host uploads and enqueues cloud i + 1 while the device
 * still fits cloud i.  Every other entry point (getters, pct_synchronize, pct_get_timings, a new cloud ...) first waits
 * for the pending call, so results are never observed early; an error of the pending call's kernels is reported by the
 * call that waits.  pct_get_timings_done does NOT wait: it returns the timings of the most recent call whose kernels are
 * known to have finished (the call before the pending one) -- what a loop polls after every step.  Off by default. */
int pct_set_async(pct_ctx* ctx, int32_t enable);
int pct_get_timings_done(const pct_ctx* ctx, pct_timings* out);
/* sizeof(pct_timings) as the library was built: a binding checks its own struct against it at load time. */
int pct_timings_size(void);
/* Device pointer helpers for zero-copy interop (multi-GPU all-gather target). */
int pct_device_alloc(pct_ctx* ctx, int64_t bytes, void** dev_ptr);
int pct_device_free(pct_ctx* ctx, void* dev_ptr);
int pct_device_upload(pct_ctx* ctx, void* dev_dst, const void* host_src, int64_t bytes);
int pct_device_download(pct_ctx* ctx, void* host_dst, const void* dev_src, int64_t bytes);
int pct_synchronize(pct_ctx* ctx);
/* Hardware self-test of the cross-lane primitives the sweep relies on
 * (DPP / ds_swizzle lane exchanges); *failures == 0 on a healthy gfx950. */
int pct_selftest(pct_ctx* ctx, int32_t* failures);
/* Self-tests of the wave-level sorters every neighbour row passes through (tests/test_gpu_sort_net.py).  They run the
 * very code the sweeps run on lists the caller supplies: host arrays in, host arrays out, device memory of their own for
 * the length of the call -- nothing resident on the handle is read, written or dropped.
 *
 * pct_selftest_sort: the fast sweeps' sorting network on n_lists lists of uint32, each returned in ascending order.
 *   network             code under test                               list length   lists per wave
 *   PCT_NET_FAST1       the C++ network, one list register            64            1
 *   PCT_NET_FAST2       the C++ network, two list registers           128           1
 *   PCT_NET_SETS1       two lists side by side, one register each     64            2
 *   PCT_NET_SETS2       two lists side by side, two registers each    128           2
 *   PCT_NET_PAIR        the assembly block of k_knn_pair              64            2
 *   PCT_NET_DUO         the assembly block of k_knn_duo               128           1
 * Lists lie one after the other in `in` and `out`; with two lists per wave, lists 2 w and 2 w + 1 share wave w and
 * n_lists must be even.  PCT_ERR_INVALID for another network, a null array, n_lists < 1.
 *
 * pct_selftest_sort_exact: the exact sweep's sorters over (float64 d2, int32 position) elements, lists of 64 * regs
 * (regs = 1, 2, 4, 8), in its total order: d2, then the public index pub[position]; padding is (+inf, INT32_MAX).
 * PCT_EXACT_ASCENDING / PCT_EXACT_DESCENDING sort each list; PCT_EXACT_MERGE_MIN replaces each ascending list (d2, pos)
 * by the 64 * regs smallest of its union with the DESCENDING list (batch_d2, batch_pos), ascending (both null otherwise).
 * Every real position must be in [0, n_pub).
 *
 * pct_selftest_order_keys: the in-place repair of equal keys on n_lists sorted lists of 64 * regs elements
 * key << slot_bits | payload (padding 0xFFFFFFFF).  Per list, d2[list * 2^slot_bits + payload] is the exact value of the
 * element with that payload and pub[list * 2^slot_bits + payload] its public index.  (regs, slot_bits) is one of
 * (1, 6), (1, 9), (2, 7), (2, 10).  out: the lists; done[list] = 1 if the repair finished, 0 if it gave up. */
enum { PCT_NET_FAST1 = 0, PCT_NET_FAST2 = 1, PCT_NET_SETS1 = 2, PCT_NET_SETS2 = 3, PCT_NET_PAIR = 4, PCT_NET_DUO = 5 };
enum { PCT_EXACT_ASCENDING = 0, PCT_EXACT_DESCENDING = 1, PCT_EXACT_MERGE_MIN = 2 };
int pct_selftest_sort(pct_ctx* ctx, int32_t network, const uint32_t* in, int64_t n_lists, uint32_t* out);
int pct_selftest_sort_exact(pct_ctx* ctx, int32_t regs, int32_t mode, const double* d2, const int32_t* pos, const double* batch_d2,
                            const int32_t* batch_pos, const int32_t* pub, int64_t n_pub, int64_t n_lists, double* out_d2, int32_t* out_pos);
int pct_selftest_order_keys(pct_ctx* ctx, int32_t regs, int32_t slot_bits, const uint32_t* elems, const double* d2, const int32_t* pub,
                            int64_t n_lists, uint32_t* out, int32_t* done);
/* Self-test of the planned fast sweep alone (tests/test_gpu_select.py): which rows it stores as final, which it hands to the
 * exact sweep and which of those it marks as trusted.  Unlike the self-tests above it works on the handle's cloud: it builds
 * the cell list as pct_knn(k, eps, algo) would for the owned rows (algo: PCT_KNN_GRID only; k <= 127; needs a cloud of at
 * most 2^24 points, PCT_ERR_INVALID otherwise, and on a handle that owns a slab), plans the sweep by the same rule under the
 * same PCT_* switches, fills the kernel's argument as pct_knn does, launches the planned kernel once -- and stops: no exact
 * sweep follows.  want_dist = 0: the plan of the fused call, which keeps no distances.
 * Out, for the owned rows in public index order: idx (rows, k) public indices, -1 where the sweep stored none; dist
 * (rows, k; may be null) the float32 distances, written only where the plan keeps them (info[9]); count (rows; may be
 * null) the eps counts, meaningful for rows that are not flagged; flags (rows): bit 0 = the row is on the redo list,
 * bit 1 = its entry carries the trusted mark; info (12): sweep_variant, redo_count, cell size, nx, ny, nz, origin x, y,
 * z, distances kept, queries per work item, work items.
 * PCT_ERR_INVALID where the redo list names a row twice or does not hold exactly redo_count entries; nothing is repaired.
 * The table it leaves is unfinished: pct_selftest_sweep drops every result on the handle, as a new cloud does, and
 * pct_get_neighbors after it answers PCT_ERR_NO_NEIGHBORS. */
int pct_selftest_sweep(pct_ctx* ctx, int32_t k, double eps, int32_t algo, int32_t want_dist, int32_t* idx, float* dist, int32_t* count,
                       uint8_t* flags, double* info);
/* Self-tests of the kernels that plan the passes of the chained sweep (PCT_KNN_GRID_LEVELS; tests/test_gpu_levels_exact.py).
 * As above: the very kernels, launched as the chain launches them, on host arrays of the caller; device memory of their
 * own for the length of the call, nothing resident on the handle is read, written or dropped.
 *
 * pct_selftest_levels_classify: the wanted edge of the rows a pass left unanswered.  Row i of n_rows is the query with
 * public index pub[i] (distinct, in [0, n_pub)); row_done[i] != 0: answered, nothing of it is touched; redo_m[i] =
 * why << 29 | stencil population.  log_edge: log2 of the pass's cell edge; target: the stencil population of a
 * well-sized pass.  want (n_pub) and bracket (n_pub pairs: largest log2 edge known too small, smallest known too
 * large) are indexed by public index, read and rewritten in place.
 *
 * pct_selftest_levels_bands: the histogram of the wanted edges want[begin, end) of n points xyz (n, 3) about log_edge0,
 * the first pass's log2 edge -- hist (160 quarter octaves) and *exact, the queries only the exact sweep answers -- and
 * the bounding box (min xyz, max xyz) and *count of the points with lo <= want < hi.  window = -1: lo and hi as given;
 * 0 .. 156: the bounds the chain gives the pass whose one-octave window starts at that bin.  bounds (2) answers the lo
 * and hi used.  No member: *count = 0 and the box (+inf x 3, -inf x 3).
 *
 * pct_selftest_levels_merge: the answered rows of a pass into the public-space table.  pub (n_pos): public index of
 * every position of the cell order; row r of n_rows is the query at position owned_pos[r]; nbr_pos / nbr_dist
 * (n_rows, pitch) the pass's table (positions, negative: no neighbour), nbr_cnt (n_rows, may be null: every row holds
 * k).  A row with row_done != 0 goes to row pub - q_begin of pub_pos / pub_dist (n_out, pitch; read and rewritten in
 * place, as are pub_cnt (n_out, may be null) and want (n_want, by public index)): its k entries as public indices, its
 * count, and its wanted edge set to NaN. */
int pct_selftest_levels_classify(pct_ctx* ctx, const int32_t* row_done, const uint32_t* redo_m, const int32_t* pub, int64_t n_rows,
                                 int64_t n_pub, float log_edge, float target, float* want, float* bracket);
int pct_selftest_levels_bands(pct_ctx* ctx, const float* want, const float* xyz, int64_t n, int64_t begin, int64_t end, float log_edge0,
                              int32_t window, float lo, float hi, uint32_t* hist, uint32_t* exact, float* bounds, float* box, uint32_t* count);
int pct_selftest_levels_merge(pct_ctx* ctx, const int32_t* pub, int64_t n_pos, const int32_t* owned_pos, int32_t q_begin, const int32_t* nbr_pos,
                              const float* nbr_dist, const int32_t* nbr_cnt, const int32_t* row_done, int64_t n_rows, int32_t k, int32_t pitch,
                              int64_t n_out, int32_t* pub_pos, float* pub_dist, int32_t* pub_cnt, float* want, int64_t n_want);

#ifdef __cplusplus
}
#endif
#endif /* PCT_HIP_H */

// Internal declarations shared by the HIP translation units (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>

#include "../../include/pct_hip.h"
#include "../../include/pct_hip_surface.h"
#include "../../include/pct_hip_holes.h"
#include "pct_stamp.h"
#include "pct_clock.h"
#include "pct_residents.h"

#define PCT_WAVE 64
#define PCT_K_MAX 511           // longest neighbour row: k + 1 <= 512 = 64 lanes x 8 list registers (wave-per-query sweeps, pct_knn_wide.hip)

// Every kernel launch of the library leaves its source position and kernel name here; the abort hook
// (pct_api.hip: install_abort_trace) prints it, so that the log of a GPU memory fault -- ROCr aborts the process from
// its own thread -- names the launch that preceded it (exactly the faulting one under HIP_LAUNCH_BLOCKING=1).
extern const char* pct_last_launch;
#define PCT_STR2(x) #x
#define PCT_STR(x) PCT_STR2(x)
// (a macro of the library's own at its launch sites: HIP's hipLaunchKernelGGL is left alone, also for the rocPRIM
// headers included after this one; the last-launch word is one relaxed atomic store, any handle's thread may write it)
#define PCT_LAUNCH(kernelName, ...)                                                          \
    do {                                                                                     \
        __atomic_store_n(&pct_last_launch, __FILE__ ":" PCT_STR(__LINE__) "  " #kernelName, __ATOMIC_RELAXED); \
        hipLaunchKernelGGL((kernelName), __VA_ARGS__);                                       \
    } while (0)
// The same from a launcher template, whose kernel argument is spelled in template parameters: the instantiation's own
// __PRETTY_FUNCTION__ follows the position, so the word still names every template argument by value.  One string per
// instantiation, composed at its first launch and never freed (the abort hook may read it at any time).
const char* pct_launch_name(const char* where, const char* instantiation);
#define PCT_LAUNCH_T(kernelName, ...)                                                        \
    do {                                                                                     \
        static const char* const name_ = pct_launch_name(__FILE__ ":" PCT_STR(__LINE__) "  " #kernelName, __PRETTY_FUNCTION__); \
        __atomic_store_n(&pct_last_launch, name_, __ATOMIC_RELAXED);                         \
        hipLaunchKernelGGL((kernelName), __VA_ARGS__);                                       \
    } while (0)

// Staging capacities of the fast sweeps (candidates of a work item's stencil held in LDS per wave), defined HERE ONLY:
// the sweep kernels (pct_knn_fast.hip, pct_knn_pair.hip, pct_knn_duo.hip) are compiled for them, the work-item census counts overflows against them and the
// hierarchical list's build (pct_tree.hip) refines its segments down to them.  A -D that overrides one must reach EVERY
// translation unit (PCT_EXTRA_FLAGS does; a per-file flag would size the tree's refinement for another capacity than
// the kernels stage).
#ifndef PCT_STAGE_CAP
#define PCT_STAGE_CAP 512                  // uniform list, one list register (k_knn_fast<1>, k_knn_pair)
#endif
#ifndef PCT_STAGE_CAP2
#define PCT_STAGE_CAP2 768                 // ... two list registers (k_knn_fast<2>)
#endif
#ifndef PCT_TREE_CAP
#define PCT_TREE_CAP 768                   // staged candidates of a work item of the hierarchical cell list (A/B: 512 | 768 | 1024)
#endif
#ifndef PCT_TREE_CAP2
#define PCT_TREE_CAP2 1024                 // ... for k + 1 > 64 (two list registers): the proofs want ~2.6 (k+1) stencil points
#endif

// ---------------------------------------------------------------------------
// Uniform cell list over the float32-rounded cloud.
// Cell id = (cz * ny + cy) * nx + cx; cell coordinates are computed in fp64 so
// that the "distance to the stencil boundary >= ring * cell" guarantee holds.
// ---------------------------------------------------------------------------
struct pct_grid {
    double ox, oy, oz;      // origin (bbox min)
    double cell;            // edge length
    double inv_cell;
    int32_t nx, ny, nz;
    int64_t ncell;
    // Faces beyond which points of the cloud were left out of this grid (a sharded handle keeps only the points
    // near its owned range), in cell units from the origin; -inf / +inf = nothing was left out on that side.
    double lim_lo[3], lim_hi[3];
};

// One device allocation and its only owner: it frees itself, cannot be copied, and changes hands by swap alone.
struct pct_buf;
void pct_release(pct_buf* b);              // frees early what the destructor would free
struct pct_buf {
    void* p = nullptr;
    size_t cap = 0;
    pct_buf() = default;
    pct_buf(const pct_buf&) = delete;
    pct_buf& operator=(const pct_buf&) = delete;
    pct_buf(pct_buf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }     // (a std::vector of them may grow)
    ~pct_buf() { pct_release(this); }
    void swap(pct_buf& o) { void* const q = p; const size_t c = cap; p = o.p; cap = o.cap; o.p = q; o.cap = c; }
};

// The two word blocks a step's kernels and its host side talk through are laid out here and nowhere else.
// Statistics of one sweep: 64 bytes, cleared (k_scan_tiles, reserve_table) and mirrored to the host as eight 64-bit words.
struct pct_sweep_words {
    unsigned long long ring_fallbacks, lds_overflows, flushes, candidate_steps, redone_queries;   // under pct_set_stats only
    unsigned long long beyond_limits;      // queries the points left out of a culled grid could matter to (always counted)
    unsigned long long costliest;          // the costliest exact query: 64-candidate steps << 32 | row
    int redo_count;                        // rows on the redo list (always counted)
    int redo_adopted;                      // of which k_knn_exact took the fast sweep's list over as the answer of ring 1 (under pct_set_stats only)
};
static_assert(sizeof(pct_sweep_words) == 64, "eight 64-bit words");
struct pct_dev_words {                     // ctx->counters: 512 bytes of device memory
    union {
        pct_sweep_words sweep;
        unsigned long long census[4];      // pct_item_census, between a cell-list build and its sweep
    };
    pct_stamp_block stamps[2];             // by parity of the call: the stage boundaries its kernels stamp (pct_stamp.h)
    unsigned long long unused[8];
    unsigned long long scatter_hits;       // pct_scatter_records: records that fell into the asked rows
    unsigned long long tail[31];
};
static_assert(sizeof(pct_dev_words) == 512, "what every user reserves");
// ctx->pin: 4 KiB of pinned, device-visible host memory.  Kernels and small copies drop their few result words here, so
// that a read-back is one stream synchronisation.  One field per read-back; no two share bytes.  A record type that
// belongs to one file is aligned bytes here, whose size that file asserts.  The fields a kernel stores to directly
// (scan_totals, stats, svd_rows, tree_totals, slab_cut, slab_counts, stamps) are aligned as they always were.
struct pct_pinned {
    alignas(128) unsigned char pack_red[128];        // PackRed, the pack reduction (pct_grid.hip)
    alignas(128) unsigned char scan_totals[32];      // ScanTotals (pct_grid.hip)
    unsigned cull_kept, cull_owned;                  // the cull pass: points kept beside the owned ones, owned points
    unsigned long long scatter_hits;
    // by parity of the fused call (pct_set_async: the next call's kernels must not overwrite what the pending one's left)
    alignas(64) pct_sweep_words stats[2];            // the sweep's statistics, mirrored by the fit kernel or copied
    alignas(64) unsigned char band_stats[704];       // BandStats of the chained sweep (pct_levels.hip)
    alignas(32) int band_box[8];                     // ... and the box of its next band: min xyz, max xyz (ordered ints), count
    alignas(2048) long long svd_rows[2];             // by parity: rows the call's fits handed to k_fit_svd
    alignas(64) unsigned long long census[4];
    alignas(128) long long tree_totals[2];           // the tree build: {items, segments}
    alignas(32) int tree_counts[26];                 // ... its counts and level histogram
    alignas(512) int slab_cut[PCT_SLAB_PARTS_MAX + 1];
    alignas(512) long long slab_counts[PCT_SLAB_PARTS_MAX];
    alignas(64) unsigned long long area_words[8];    // pct_point_areas (pct_area.hip): overflow rows, closed rows, NaN rows, neighbours past the rejection test
    // by parity: the stamps of a call timed by the device clock, mirrored whole by the step's last kernel; the host clears
    // the end stamp before it enqueues the call and reads the block once that word is non-zero (pct_stamp.h)
    alignas(64) pct_stamp_block stamps[2];
    alignas(64) unsigned long long frame_words[8];   // pct_point_frames (pct_frame.hip): NaN rows, flipped rows, umbilic rows
    alignas(64) int orient_words[16];                // pct_orient_frames (pct_orient.hip): its control words, OrientWord
    alignas(64) unsigned long long tri_words[8];     // pct_point_triangles (pct_fan.hip): FanWord; [7] the triangle count
    alignas(64) long long hole_words[8];             // pct_fill_holes (pct_hole.hip): HoleWord
};
static_assert(sizeof(pct_pinned) <= 4096, "pct_create allocates 4096 bytes");

// The handle's stopwatch pairs.  The stages of a sweep or a fused call are not among them: they are timed by the call's
// clock (pct_clock.h), which owns the events of its boundaries.
// The surface stages (pct_stage, below) share one triple: every call that records it ends in a wait for the stream and
// turns the events into milliseconds before it returns, so no event's meaning outlives its call.
enum pct_event {                           // ctx->ev
    PCT_EV_IO_BEGIN, PCT_EV_IO_END,        // an upload or an export
    PCT_EV_FIT_BEGIN, PCT_EV_FIT_END,      // a fit on its own (pct_fit and its siblings)
    PCT_EV_SCAN_TOTALS,                    // the cell list's scan totals are in pinned memory (pct_build_grid)
    PCT_EV_STAGE_BEGIN, PCT_EV_STAGE_MID, PCT_EV_STAGE_END,   // a surface stage (pct_api_surface.hip: run_stage); mid: pct_point_triangles alone
    PCT_EV_COUNT
};

// The surface stages -- what is computed from the resident neighbour table, one resident result each -- and the numbers of a
// stage's last call as its statistics getters serve them while that result is in place (zeros once it is gone).
enum pct_stage { PCT_STAGE_AREAS, PCT_STAGE_FRAMES, PCT_STAGE_ORIENT, PCT_STAGE_TRIANGLES, PCT_STAGE_HOLES, PCT_STAGE_COUNT };
constexpr pct_resident kPctStageResident[PCT_STAGE_COUNT] = {PCT_R_AREAS, PCT_R_FRAMES, PCT_R_ORIENT, PCT_R_TRIANGLES, PCT_R_HOLES};
// stats: the public counters in their getter's order; ms: device milliseconds of the call, then whatever doubles the stage's
// profile getter serves (triangles: fan kernels, agreement and emission; areas: the survivor count)
struct pct_stage_report { int64_t stats[8]; double ms[3]; };

constexpr int kPctStageSlots = 4;   // pct_ctx::stage, where the chain of claims that sets the count is named

struct pct_comm;            // RCCL communicator + exchange stream (pct_comm.hip); null on a single-GPU handle

struct pct_ctx {
    int device = 0;
    pct_comm* comm = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev[PCT_EV_COUNT] = {};
    pct_call_clock clock[2];       // stage timing of a sweep or a fused call, by parity of the call (blocking calls: 0)
    // Streams of clouds (pct_set_async): a fused call returns once its kernels are enqueued; its clock, its statistics
    // words and its SVD row count wait in the slots of the call's parity until the NEXT fused call has passed its
    // mid-build wait (everything of the previous call has completed by then) or until anything else is asked of the
    // handle (which first waits for the stream).  The host prepares step i + 1 while the device fits step i.
    bool async_mode = false;
    pct_residents res;             // which results are in place, each one's order (table-row or public) and the rows it covers
                                   // -- recorded there alone (the state rules of include/pct_hip.h: pct_residents.h)
    // the pending call -- on: a fused call has been enqueued and its bookkeeping has not been done; par: its parity (which
    // clock times it, which pinned slots its kernels write); sorted: its table is in a sorted space, knn_fast_ms applies;
    // tm: the host-side fields of its timings
    struct { bool on = false; int par = 0; bool sorted = false; pct_timings tm = {}; } pend;
    pct_buf stamp_tickets;         // unsigned (kStampTicketLines lines): blocks of the step's last kernel that have finished (pct_stamp_last_out;
                                   // zero between launches: cleared when allocated, by the first call that opens on stamps)
    pct_timings tm_done = {};      // timings of the last call whose bookkeeping has been done
    char err[512] = {0};

    int64_t n = 0;                 // cloud size (candidates)
    int64_t q_begin = 0, q_end = 0;
    // Points the grid holds: all n, or -- sharded handles -- the points inside the owned range's bounding box plus
    // a margin, compacted in public order (pts4.w keeps the public index).  g_begin = position of the first owned
    // point in that compacted array (== q_begin when nothing was left out).
    int64_t n_grid = 0, g_begin = 0;
    bool culled = false;           // the grid holds fewer than n points
    bool no_cull = false;          // set after a sweep met a query the kept points cannot answer
    float cull_box[6] = {0, 0, 0, 0, 0, 0};    // box of the last sharded pack (reused for the next similar cloud)
    bool cull_box_valid = false;
    int64_t cull_box_n = 0, cull_box_q0 = 0, cull_box_q1 = 0;
    int32_t retries = 0;
    // Ownership by slab (pct_set_query_slab): the cloud is cut into slab_parts slabs of equal population along its
    // longest axis and this handle answers the points of slab_part.  The cut comes from a 4096-bin histogram every
    // rank computes alike from the gathered cloud; q_begin / q_end then refer to the PACKED array (owned first).
    int32_t slab_part = 0, slab_parts = 0;
    int32_t slab_axis = 0, slab_bin_lo = 0, slab_bin_hi = 0;
    float slab_x0 = 0, slab_inv = 0;
    float slab_bbox[6] = {0, 0, 0, 0, 0, 0};
    int64_t slab_counts[PCT_SLAB_PARTS_MAX] = {};
    bool slab_split_valid = false;
    double hint_edge = 0, hint_guess = 0, hint_target = 0;   // warm start of the cell-size search (pct_build_grid)
    float spec_bbox[6] = {0, 0, 0, 0, 0, 0};   // grid box of the last plain build (trimmed), reused speculatively
    float spec_raw[6] = {0, 0, 0, 0, 0, 0};    // raw bounding box of that cloud
    int64_t spec_n = 0;
    bool spec_valid = false;
    // density-adaptive sweep (pct_levels.hip): the queries one pass could not answer are re-owned by the next pass, which
    // sizes its cells for THEM and says so in a LevelPass (below); what lives here are the allocations the passes reuse
    pct_buf lvl_src;                // float4 (n): the points in the cell order of the first pass (input of the later passes' builds)
    // hierarchical cell list (pct_tree.hip)
    int tree_bits = 0;
    int64_t tree_segs = 0;
    double tree_two_level_share = 1.0;   // share of the points on the two most populated adjacent octree levels (same sample)
    int tree_level_spread = 0;      // octree levels between the 5th and 95th percentile of the points (a sample of the segments)
    pct_buf tree_codes, tree_vals;  // u64 / u32 (2 n): Morton codes and public positions, unsorted | sorted
    pct_buf tree_lvl;               // u8 (n): octree level every point is served at
    pct_buf tree_head, tree_marks;  // segment / item marks and their scans
    pct_buf tree_seg, tree_runs;    // int4 per segment {level, cx, cy, cz}; int2 x 27 per segment {first position, points}
    pct_buf tree_range;             // int2 per segment {first position, points} + int per segment: stencil population + device totals
    pct_buf tree_bucket;            // int (2^18 + 2): first position of every 18-bit code prefix (pct_code_lower_bound)
    pct_buf tree_tmp;
    pct_buf row_done;               // int32 (rows of the pass)
    pct_buf redo_m;                 // int32, parallel to redo: stencil population of the row's item
    pct_buf flag_buf;               // float (n): wanted log2 cell edge of every point still unanswered (NaN = answered)
    pct_buf dens_buf;               // float2 (n): log2 of the largest edge known too small / the smallest known too large
    pct_buf pub_pos, pub_dist, pub_cnt;   // public-space neighbour table the passes are merged into
    float tree_bbox[6] = {0, 0, 0, 0, 0, 0};        // bounding box of the cloud the hierarchical list was last built for
    int64_t auto_tree_n = 0;        // PCT_KNN_AUTO sent a cloud of this size to the hierarchical list: the next one of the same
    int32_t auto_tree_calls = 0;    // size goes there directly (no uniform build first); re-examined every 16th call
    float auto_tree_bbox[6] = {0, 0, 0, 0, 0, 0};   // ... whose bounding box was this (the next cloud must match it within 2 %)
    bool has_f64 = false;
    double occupancy_factor = 0.0; // 0 = default
    bool collect_stats = false;    // sweep statistics (costly same-address atomics)

    // coordinates
    pct_buf xyz;        // float  (n,3) public order (owned copy)
    const float* xyz_view = nullptr;   // the coordinates in use: xyz.p, or a caller's buffer (pct_use_points_device_f32)
    pct_buf pts4;       // float4 (n_grid) public order, w = public index bits
    pct_buf pts4d;      // double4 (n) public order (only when has_f64), w = index
    // grid
    pct_grid grid = {};
    pct_buf cell_of;    // int32 (n) cell id per public point
    pct_buf cell_cnt;   // int32 (ncell+1) exclusive cell starts in the sorted cloud
    pct_buf cell_own;   // int32 (ncell) owned points per cell (stored first inside the cell)
    pct_buf cell_oth;   // int32 (ncell) other points per cell (sharded handles only)
    pct_buf own_start;  // int32 (ncell+1) first neighbour-table row of every cell
    pct_buf cell_fill;  // int32 (n) arrival rank of every point in its cell and class
    pct_buf scan_tmp;   // block sums
    // two-level counting sort of the whole-cloud builds (pct_grid.hip, k_bin_*), sized per pass
    pct_buf bin_rec;    // float4 (n_grid) the records partitioned by bucket (a contiguous range of cell ids)
    pct_buf bin_mat;    // u32 (tiles, buckets) records of every input tile per bucket, then their column-wise exclusive scan
    pct_buf bin_plan;   // plan words, bucket starts, column totals, int4 work list {bucket, chunk, offset slot, 0}
    pct_buf bin_base;   // int32 (shared items, cells per bucket x classes) run offsets of the items that share a bucket
    pct_buf occ;        // int2 (n_items) work items {cell id, chunk of items_q queries}
    pct_buf redo;       // int32 (n) queries the fast sweep handed to the exact sweep
    int64_t n_items = 0;
    int64_t nonempty_cells = 0;    // cells of the current cell list that hold at least one point
    int32_t items_q = 12;
    pct_buf sorted4;    // float4 (n) cell-sorted, w = public index bits
    pct_buf sorted4d;   // double4 (n) cell-sorted native coords (has_f64)
    pct_buf row_of;     // int32 (owned) neighbour-table row of public index q_begin + i
    // the k_bin_* build leaves row_of to the first reader (pct_ensure_row_of: from w of the sorted records)
    bool row_of_valid = true;
    int64_t row_of_rows = 0;
    int32_t row_of_begin = 0;
    pct_buf owned_pos;  // int32 (owned) sorted position of every table row
    pct_buf red;        // small reduction scratch
    pct_pinned* pin = nullptr;
    int64_t n_occ = 0;
    bool grid_valid = false;
    bool grid_whole = false;       // the cell list in place is one uniform list over the WHOLE cloud, every point owned (commit_grid)
    bool pts4_valid = false;

    // neighbour table: one row per OWNED query (cell order, see own_start); entries are sorted positions
    pct_buf nbr_pos;    // int32 (n,k) sorted positions of the neighbours
    pct_buf nbr_dist;   // float (n,k)
    pct_buf nbr_cnt;    // int32 (n)
    int32_t k = 0;
    int32_t nbr_pitch = 0;   // row pitch of nbr_pos / nbr_dist in elements (k rounded up to 4)
    double eps = 0.0;
    bool counters_clean = false;   // the sweep's statistics words were zeroed by the cell-list build just enqueued (k_scan_tiles)
    int fit_parity = 0;            // which of the two counts of fit_flag the next fit launch uses (the launch zeroes the other one)
    void* fit_flag_seen = nullptr; // the fit_flag allocation (pointer and capacity) whose head has been zeroed
    size_t fit_flag_cap_seen = 0;
    bool knn_hier = false;         // the table in place came from the hierarchical list or the chain of cell lists (run_knn)
    bool knn_sorted_space = false; // the table's rows are in cell order, its entries sorted positions; false: public indices (brute force)
    bool dist_valid = true;        // nbr_dist holds the distances of the table in place (else: derived on demand)
    pct_buf counters;   // pct_dev_words: the sweep's statistics words, the census, the scatter hit count

    // fit results (PCT_R_FIT; in table-row order behind a sweep of a cell list: res.in_row_order)
    pct_buf coefs;      // float (n,6)
    pct_buf K, H, H2;   // float (n)
    bool fit_cloud_aligned = false;// results belong to cloud rows [q_begin, q_end) (pct_fit / pct_curvature) rather than to the
                                   // rows of a pct_fit_indices call; kept apart from the table, which helpers may drop

    pct_buf fit_flag;   // int: [0] number of rows k_fit handed to k_fit_svd, [16..] the rows
    // Staging scratch of a call, claimed in stack order and never named (pct_claim and pct_stage_scope, below).
    // The reuse rule: a slot given back by a scope may be claimed again while kernels that read it are still queued.  Safe
    // only because EVERY write to a slot is an operation on ctx->stream (and pct_reserve waits for the stream before it
    // moves a buffer): nothing may write a slot any other way -- no blocking hipMemcpy, no other stream.
    // kPctStageSlots is the deepest chain of claims: pct_fit_ball holds two (centres, member counts) while its launcher
    // holds two more; pct_get_neighbor_rows, pct_mesh_energies, the study and pct_fit_indices_f64 reach four on their own.
    pct_buf stage[kPctStageSlots];
    int stage_top = 0;
    pct_buf qpts4;      // float4 {x,y,z,index} of EVERY point in public order, for pct_query_points (built on first use)
    bool qpts4_valid = false;
    // pct_query_points_algo (pct_query.hip): scratch of a query through the cell list -- its words, the queries' cell ids
    // and their order by cell, work items, redo list, sort scratch --, the words read back, and what pct_query_stats reports
    pct_buf qry;
    int32_t query_words[4] = {0, 0, 0, 0};
    int64_t query_stats[4] = {0, 0, 0, 0};

    // pct_query_ball (pct_ball.hip): the CSR rows of the last radius query, resident until the next one or a new cloud
    pct_buf ball_off;   // int64 (m + 1) offsets
    pct_buf ball_idx;   // int32 (entries) public indices
    pct_buf ball_alt;   // ... the other buffer of the library's segmented sort (rows longer than k_ball_sort takes)
    pct_buf ball_dist;  // double (entries), when asked for
    bool ball_has_dist = false;
    int64_t ball_stats[4] = {0, 0, 0, 0};

    // PCA principal curvatures (pct_pca.hip), public order: double [lambda_1 | lambda_2 | K | H | frame (n,3,2)]
    pct_buf pca;
    pct_buf pca_aux;    // float32 rounding offset, flags, rows handed to the exact pass and their bounds
    pct_buf pca_nbr;    // int32 (n,k): the neighbourhoods used (pct_pca_curvatures with keep_neighbors)
    pct_buf pca_orig;   // double4 (n): float64 clouds' uploaded records while the sweep sees them recentred
    bool pca_has_nbr = false, pca_recentred = false;
    int32_t pca_k = 0;

    pct_timings tm = {};

    pct_stage_report report[PCT_STAGE_COUNT] = {};    // of every surface stage's last call (pct_api_surface.hip: run_stage fills, stage_numbers serves)

    // per-point tangent-plane Voronoi areas (pct_area.hip) of the owned rows of the resident table (PCT_R_AREAS: in the order
    // and for the rows res records, as the fit)
    pct_buf area;          // double (owned)
    pct_buf area_closed;   // uint8 (owned)
    pct_buf area_nverts;   // int32 (owned)
    pct_buf area_over;     // eight statistics words, then int32 (owned): the rows redone with room for k + 4 vertices

    // per-point surface frames (pct_frame.hip) of the owned rows of the resident table and its fit (PCT_R_FRAMES: as the areas)
    pct_buf frame;         // double (owned): normal (rows, 3) | k1 k2 (rows, 2) | directions (rows, 3, 2)
    pct_buf frame_flip;    // eight statistics words, then uint8 (owned): the viewpoint turned the row's normal

    // consistent orientation of those frames (pct_orient.hip): one allocation, carved up per call; the four results in
    // public order, int32 / uint8 (owned)
    pct_buf orient;
    const int* orient_comp = nullptr;
    const int* orient_parent = nullptr;
    const int* orient_level = nullptr;
    const unsigned char* orient_toggle = nullptr;

    // fans and triangles of the resident table of a whole-cloud handle (pct_fan.hip), everything by public index: they
    // depend on neither the table nor row_of once computed
    pct_buf fan_head;      // int2 (n): {vertices of the row's cell, slot in fan_wide or -1}
    pct_buf fan_fast;      // int32 (n, kAreaCap): the fan codes of the rows the fast kernel finished
    pct_buf fan_wide;      // int32 (overflow rows, k + 4): ... of the rows redone with room for k + 4 vertices
    pct_buf fan_side;      // uint8 (n): the frames' flipped bits as the call found them
    pct_buf fan_over;      // eight statistics words, then int32 (n): the overflow list
    pct_buf tri_mask, tri_count, tri_off, tri_tmp;   // agreed corners per row, triangles per row, their scan, scan scratch
    pct_buf tri_part;      // u64 (blocks, 4): the statistics' per-block partial sums
    pct_buf tri;           // int32 (triangles, 3), ascending
    int32_t tri_wpitch = 0;
    int64_t tri_total = 0;

    // boundary loops and patches of those triangles (pct_hole.hip, include/pct_hip_holes.h): PCT_R_HOLES, made from the
    // triangles -- whatever drops or replaces them drops these
    pct_buf hole_cnt, hole_off;     // int64 (n + 1): gaps per row, their scan
    pct_buf hole_part;              // u64 (blocks, 4): the statistics' per-block partial sums
    pct_buf hole_gap;               // int2 (gaps): the gaps' members {a, b}; int (gaps): their rows
    pct_buf hole_slot;              // per gap: HoleSlot, PCT_HOLE_MAX_VERTICES loop vertices, 3 (PCT_HOLE_MAX_VERTICES - 2) patch indices
    pct_buf hole_scan;              // HoleSum (gaps + 1): loops, loop vertices and patch triangles before every gap
    pct_buf hole_loop;              // the owned loops packed: int64 offsets (loops + 1) | int32 vertices | uint8 status
    pct_buf hole_tri, hole_alt;     // int32 (patches, 3) ascending; the sort's other buffer
    pct_buf hole_filled;            // int32 (triangles + patches, 3) ascending
    pct_buf hole_tmp;               // scan, sort and merge scratch
    int64_t hole_loops = 0, hole_loop_verts = 0, hole_patches = 0;
};

int pct_fail(pct_ctx* ctx, int code, const char* fmt, ...);
// getenv() for the library's switches (PCT_*), cached: a fused call used to make ~20 getenv() scans of the environment
// (~6 us per step).  The cache is dropped whenever the environment block changes (a fingerprint of its string pointers,
// ~50 loads per lookup), so tests and tools that flip a switch between calls keep working.  `name` must be a literal.
const char* pct_getenv(const char* name);
void pct_comm_release(pct_ctx* ctx);

// The fast sweep sorts <= 64 survivors in one register per lane (R = 1) or <= 128 in two (R = 2).  R = 1 would hold
// k + 1 <= 64, but near that limit the window k+1 <= count <= 64 for the threshold gets narrow and the larger cells
// overflow the 512-slot staging area: from k + 1 > kFastR1Max on, R = 2 (768 slots, window up to 128) is faster.
// (Round 3, k_knn_pair against k_knn_duo on the 1 M torus: 0.51 | 0.60 ms at k = 56, 0.59 | 0.60 at 60, 0.80 | 0.61 at 63.)
#ifndef PCT_FAST_R1_MAX
#define PCT_FAST_R1_MAX 61
#endif
inline int pct_fast_r1_max() {
    static const int v = [] { const char* e = getenv("PCT_FAST_R1_MAX"); const int x = e ? atoi(e) : PCT_FAST_R1_MAX; return x < 2 ? 2 : x > 64 ? 64 : x; }();
    return v;
}
// cell occupancy (points sharing a point's cell) the grid is sized for, as a multiple of k + 1 (tools/tune_factor.py)
// R = 1: the optimum is set by the 512 staged slots, not by k: ~27 points per cell for k <= 47 (measured optimum
// 2.4 (k+1) at k = 10, 1.2-1.4 at 20, 0.85 at 30, 0.55-0.60 at 40), rising to ~29.5 from k = 52 on (0.55 at 50, 0.50 at
// 56 and 60): larger cells mean fewer work items and ring fallbacks until the 27-cell stencil of a surface outgrows
// the staging area.
inline double pct_default_factor(int k) {
    if (k + 1 <= pct_fast_r1_max()) {
        const double per_cell = k <= 47 ? 27.0 : k >= 52 ? 29.5 : 27.0 + 0.5 * (k - 47);
        return per_cell / (k + 1);
    }
    const double n = k + 1;                           // R = 2 (768 slots): 0.52 up to k ~ 84, 0.45 at 100, 0.40 at 127
    if (n > 128) return 0.35;                         // wave-per-query exact sweep only: ~3 (k+1) candidates in the 27 cells of a surface
    return n <= 85 ? 0.52 : n <= 101 ? 0.52 - 0.07 * (n - 85) / 16.0 : 0.45 - 0.05 * (n - 101) / 27.0;
}

// Morton codes of the hierarchical cell list: 21 bits per axis, x in bit 0 of every triple
__host__ __device__ inline unsigned long long pct_spread3(unsigned v) {         // bit i -> bit 3 i
    unsigned long long x = v & 0x1fffffu;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}
__host__ __device__ inline unsigned pct_compact3(unsigned long long x) {        // bit 3 i -> bit i
    x &= 0x1249249249249249ull;
    x = (x ^ (x >> 2)) & 0x10c30c30c30c30c3ull;
    x = (x ^ (x >> 4)) & 0x100f00f00f00f00full;
    x = (x ^ (x >> 8)) & 0x1f0000ff0000ffull;
    x = (x ^ (x >> 16)) & 0x1f00000000ffffull;
    x = (x ^ (x >> 32)) & 0x1fffffull;
    return (unsigned)x;
}
// offset of stencil cell t (0..26) from the centre cell; t = 0 is the centre (staged / scanned first)
__host__ __device__ inline void pct_stencil_cell(int t, int* dx, int* dy, int* dz) {
    const int i = t == 0 ? 13 : t == 13 ? 0 : t;
    *dx = i % 3 - 1;
    *dy = (i / 3) % 3 - 1;
    *dz = i / 9 - 1;
}
// first position of the Morton-sorted code array whose code is >= key
__device__ inline int64_t pct_code_lower_bound(const unsigned long long* __restrict__ codes, int64_t n, unsigned long long key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (codes[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// The same through the bucket table of the tree build: bucket[p] = first position whose code >= p << kTreeBucketShift
// (2^18 + 2 entries).  A search is a chain of dependent loads, ~20 over a million codes; the table leaves the two or
// three inside one bucket (the refinement of a segment next to a much denser region is a chain of such searches).
constexpr int kTreeBucketBits = 18, kTreeBucketShift = 63 - kTreeBucketBits;
__device__ inline int64_t pct_code_lower_bound(const unsigned long long* __restrict__ codes, const int* __restrict__ bucket,
                                               unsigned long long key) {
    const unsigned p = (unsigned)(key >> kTreeBucketShift);
    int64_t lo = bucket[p], hi = bucket[p + 1];
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (codes[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

#define PCT_HIP(ctx, call)                                                        \
    do {                                                                          \
        hipError_t e_ = (call);                                                   \
        if (e_ != hipSuccess)                                                     \
            return pct_fail((ctx), e_ == hipErrorOutOfMemory ? PCT_ERR_OOM : PCT_ERR_HIP, \
                            "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define PCT_TRY(expr)            \
    do {                         \
        int s_ = (expr);         \
        if (s_ != PCT_OK) return s_; \
    } while (0)

int pct_reserve(pct_ctx* ctx, pct_buf* b, size_t bytes);
int pct_reserve_fit(pct_ctx* ctx, int64_t rows);     // the handle's fit results (ctx->coefs, K, H, H2) for `rows` rows
inline pct_dev_words* pct_dev(pct_ctx* ctx) { return (pct_dev_words*)ctx->counters.p; }     // after pct_reserve(&ctx->counters, sizeof(pct_dev_words))
// The call's staging slots (pct_ctx::stage has the rules).  Every helper counts elements of T and enqueues on ctx->stream;
// who: the claimant, for the error that refuses a claim past the last slot -- the caller's name unless given.
int pct_claim_bytes(pct_ctx* ctx, size_t bytes, void** out, const char* who);        // the lowest unclaimed slot, reserved to `bytes`
struct pct_stage_scope {                   // what is claimed while it lives is given back when it dies
    pct_ctx* const ctx;
    const int mark;
    explicit pct_stage_scope(pct_ctx* c) : ctx(c), mark(c->stage_top) {}
    ~pct_stage_scope() { ctx->stage_top = mark; }
};
template <class T>
int pct_claim(pct_ctx* ctx, size_t count, T** out, const char* who = __builtin_FUNCTION()) {
    return pct_claim_bytes(ctx, count * sizeof(T), (void**)out, who);
}
template <class T>                         // ... filled with the host array, which must outlive the copy
int pct_claim_upload(pct_ctx* ctx, const T* host, size_t count, T** out, const char* who = __builtin_FUNCTION()) {
    PCT_TRY(pct_claim(ctx, count, out, who));
    PCT_HIP(ctx, hipMemcpyAsync(*out, host, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return PCT_OK;
}
template <class T>                         // count elements to the host; host == null: not asked for
int pct_enqueue_download(pct_ctx* ctx, T* host, const T* dev, size_t count) {
    if (host && count) PCT_HIP(ctx, hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    return PCT_OK;
}
// pct_api.hip: the first statement of every entry point (device, error text, the pending asynchronous call, no staging
// claimed), and of those a slab handle refuses (the header's list under "Ownership": its rows are not rows by index)
int pct_begin_call(pct_ctx* ctx, bool wait_for_pending = true);
int pct_begin_row_call(pct_ctx* ctx, const char* what);
inline float pct_ev_ms(pct_ctx* ctx, pct_event a, pct_event b) { return pct_event_ms(ctx->ev[a], ctx->ev[b]); }   // after the wait for both

// What one call asks of another, and what it answers, travels in arguments and results -- never parked on the handle.
// Which pinned parity slot (statistics mirror, SVD row count) the fits of a call write, and whether its fit kernel may
// mirror the sweep's statistics words there (the fused call: one copy less in the step's tail).
// clock (may be null): the fused call's, whose end the fit kernels may be asked to stamp (pct_call_clock::end_words).
struct FitSlot { int par; bool mirror_stats; pct_call_clock* clock; };
enum class GridVerdict { Built, GaveUp };                  // GaveUp: more than 16 cells per point wanted, nothing built
enum class TreeVerdict { Built, Unusable, OtherCloud };    // Unusable: not a cloud for it; OtherCloud: not the expected box; nothing built
// What one pass of the chained sweep (pct_knn_levels) asks of the cell-list build and of the sweep over it.  A null
// pointer to it is a plain call; the first pass of a chain carries no wanted-edge array and owns by index range.
struct LevelPass {
    const float* want = nullptr;   // device float (n): wanted log2 cell edge of every unanswered point (NaN = answered)
    float lo = 0, hi = 0; int64_t owned = 0;   // the pass owns the points with lo <= wanted < hi: this many, one table row each
    double edge = 0;               // > 0: the first cell edge is given (and, with want, is the only one tried)
    const float* box = nullptr;    // float (6): bounding box of the owned points of a fast pass, whose grid covers only them
    const float4* base = nullptr;  // float4 (n): the points in the cell order of the first pass, input of the later builds ...
    float base_box[6] = {0, 0, 0, 0, 0, 0};   // ... on that pass's (trimmed) grid box: ANSWERED by the first pass's pct_build_grid
};
inline int64_t pct_call_rows(const pct_ctx* ctx, const LevelPass* pass) { return pass && pass->want ? pass->owned : ctx->q_end - ctx->q_begin; }   // one per owned query

// grid build (pct_grid.hip)
int pct_pack_points(pct_ctx* ctx, float* bbox6);
int pct_pack_points_f64(pct_ctx* ctx, const double* d_xyz64);
// may_give_up: PCT_KNN_AUTO on a cloud the hierarchical list could take (pct_auto_route.h)
// clock (may be null: a build outside a timed call): the call's, whose begin the build's first launch marks
// pass (null: a plain build): the chained sweep's; its first pass gets the box of the accepted build back in base_box
int pct_build_grid(pct_ctx* ctx, int32_t k, double eps, bool may_give_up, GridVerdict* out, pct_call_clock* clock, LevelPass* pass);
// neighbour sweeps (pct_knn.hip); want_dist = false: the caller reads no distances from the table (the fused call);
// clock: the call's -- the end of the fast sweep is a boundary of its sweep stage; pass (null: a plain sweep): as above
int pct_launch_knn_grid(pct_ctx* ctx, int32_t k, double eps, bool exact_only, int phase, bool want_dist, pct_call_clock* clock, const LevelPass* pass);
int pct_launch_knn_brute(pct_ctx* ctx, int32_t k, double eps);
unsigned pct_redo_trusted_bit();         // kRedoTrusted (pct_knn_sweep.h), for the host code that reads a redo list (pct_selftest_sweep)
// census of the work items of the cell list in place: out4 = {queries, queries whose stencil overflows the staging
// area, queries whose stencil holds fewer than 2.5 (k+1) points (too few to vouch for k+1 within one cell edge), sum over the other queries of the non-empty cells in their
// 27-cell stencil} -- what decides between the plain and the density-adaptive sweep before anything is swept
int pct_item_census(pct_ctx* ctx, int32_t k, unsigned long long out4[4]);
// pct_levels.hip; fuse_par: every pass fits the rows it answered, into the pinned slots of this parity (null: no fits)
int pct_knn_levels(pct_ctx* ctx, int32_t k, double eps, const int* fuse_par, pct_call_clock* clock);
// pct_tree.hip; expect_bbox: the box a remembered verdict of PCT_KNN_AUTO was given for (null: any cloud)
int pct_build_tree(pct_ctx* ctx, int32_t k, double eps, const float* expect_bbox, TreeVerdict* out);
int pct_launch_knn_tree(pct_ctx* ctx, int32_t k, double eps, bool want_dist, pct_call_clock* clock);
int pct_launch_export_neighbors(pct_ctx* ctx, int64_t begin, int64_t end,
                                int32_t* d_idx, float* d_dist, int32_t* d_cnt);
// fit (pct_fit.hip)
// *mirrored (may be null): a fit kernel mirrored the statistics words; *by_row: the results are stored in table-row order
int pct_launch_fit_table(pct_ctx* ctx, FitSlot slot, bool* mirrored, bool* by_row);
int pct_launch_fit_pass(pct_ctx* ctx, int64_t rows, int par);
int pct_launch_fit_rows(pct_ctx* ctx, const int32_t* d_idx, const int32_t* d_cnt,
                        const int64_t* d_query, int64_t rows, int32_t k, int32_t pitch,
                        float* d_coefs, float* d_K, float* d_H, float* d_H2, bool sorted_space);
int pct_launch_fit_rows32(pct_ctx* ctx, const int32_t* d_idx, const int32_t* d_cnt, const int32_t* d_query32, int64_t rows,
                          int32_t k, int32_t pitch, float* d_coefs, float* d_K, float* d_H, float* d_H2);
// pct_fit_ball.hip: the resident CSR rows of the last pct_query_ball fitted about the centres d_self32 (rows); d_used (rows)
// receives the members per row; results row-aligned in ctx->coefs / K / H / H2, SVD row count in pinned slot 0
int pct_launch_fit_ball(pct_ctx* ctx, const int* d_self32, int64_t rows, int* d_used);
int pct_launch_prefix_rows(pct_ctx* ctx, const int* d_sample_pos, int64_t n_samples, int n_lo, int n_hi, int* d_table,
                           int pitch, int* d_cnt, int64_t* d_row_query);
int pct_launch_curvatures(pct_ctx* ctx, const float* d_coefs, int64_t rows, float* d_K, float* d_H, float* d_H2);
int pct_launch_plane_rotate(pct_ctx* ctx, const void* d_nbrs, bool f64, int64_t batch, int32_t m, double* d_out);
int pct_launch_quadric_rows(pct_ctx* ctx, const float* d_pts, int64_t batch, int32_t m, float* d_coefs);
int pct_launch_selftest(pct_ctx* ctx, int* d_fails);
// the sorters' self-tests (pct_knn.hip): device arrays, one wave per list (per pair of lists where the network sorts two)
int pct_selftest_sort_regs(int network);             // list registers of a wave under that network; 0: no such network
int pct_launch_selftest_sort(pct_ctx* ctx, int network, const unsigned* d_in, int n_waves, unsigned* d_out);
int pct_launch_selftest_exact(pct_ctx* ctx, int regs, int mode, const double* d2, const int* pos, const double* bd2, const int* bpos,
                              const float4* pts, int n_lists, double* out_d2, int* out_pos);
int pct_launch_selftest_order(pct_ctx* ctx, int regs, int slot_bits, const unsigned* elems, const double* d2, const float4* pts, int n_lists,
                              unsigned* out, int* done);
// the chained sweep's planning kernels on device arrays of the caller (pct_levels.hip), launched as pct_knn_levels launches
// them.  bands: stats = 162 words (160 bins, exact, pad), window >= 0 takes [lo, hi) from the plan's window of bins that
// starts there, used2 (host) answers the bounds the box kernel ran with, box7 = six ordered ints and the count
int pct_launch_selftest_levels_classify(pct_ctx* ctx, const int* row_done, const int* redo_m, int64_t n_rows, const float4* sorted4,
                                        const int* owned_pos, float log_edge, float target, float* want, float* bracket2);
int pct_launch_selftest_levels_bands(pct_ctx* ctx, const float* want, const float* xyz, int64_t begin, int64_t end, float log_edge0,
                                     int window, float lo, float hi, unsigned* stats, float used2[2], int* box7);
float pct_levels_box_float(int ordered);             // an ordered int of box7 as the float the chain reads
int pct_launch_selftest_levels_merge(pct_ctx* ctx, const float4* sorted4, const int* owned_pos, int q_begin, const int* nbr_pos,
                                     const float* nbr_dist, const int* nbr_cnt, const int* row_done, int64_t n_rows, int k, int pitch,
                                     int* pub_pos, float* pub_dist, int* pub_cnt, float* want);
int pct_ensure_plain_records(pct_ctx* ctx);
int pct_launch_fit_rows_f64(pct_ctx* ctx, const int32_t* d_idx, const int32_t* d_cnt, const int64_t* d_query, int64_t rows,
                            int32_t k, int32_t pitch, double* d_coefs, double* d_K, double* d_H);
int pct_launch_query_points(pct_ctx* ctx, const double* d_q, int64_t m, int32_t k, double eps, int32_t* d_idx, double* d_dist);
// pct_query.hip: the queries through the uniform cell list in place; host_words4 = {work items, rows redone by the exact
// sweep, largest ring of those, 0} is complete once the stream has been waited for
int pct_launch_query_grid(pct_ctx* ctx, const double* d_q, int64_t m, int32_t k, double eps, int32_t* d_idx, double* d_dist, int32_t* host_words4);
// pct_ball.hip: radius search, m >= 1 queries and 1 (r_stride 0) or m (r_stride 1) radii on the device; grid: through the
// cell list in place, else all n points per query.  h_offsets (m + 1) is complete on return whatever the status;
// stat3 = {queries answered from a staged cube, queries streamed, largest ring}
int pct_launch_ball(pct_ctx* ctx, bool grid, const double* d_q, int64_t m, const double* d_r, int r_stride, int32_t flags,
                    int64_t max_entries, int64_t* h_offsets, int64_t stat3[3]);
int pct_launch_gather_int(pct_ctx* ctx, const int* d_map, int* d_inout, int64_t n);
// pct_rows.hip.  One column of a per-row result on its way to the host: where row 0 lies on the device, the bytes of a row,
// the caller's array (null: not asked for).  pct_download_columns: rows [first, first + rows) of every column asked for,
// one copy each (one for a run of columns adjacent on both sides) and one wait; map (null: the rows lie in the order asked
// for) names the stored row of every row -- then at most kPctRowColumns columns, gathered by one kernel into a staging claim
// of its own first.
// pct_enqueue_columns: without the wait.
struct pct_column { const void* base; int bytes; void* host; };
constexpr int kPctRowColumns = 4;
int pct_enqueue_columns(pct_ctx* ctx, const pct_column* cols, int ncol, int64_t first, int64_t rows, const int* map);
int pct_download_columns(pct_ctx* ctx, const pct_column* cols, int ncol, int64_t first, int64_t rows, const int* map);
int pct_ensure_row_of(pct_ctx* ctx);     // before any read of ctx->row_of
// pct_api.hip, for every row getter (pct_api_surface.hip has the surface stages'): the range error of rows [begin, end)
// outside the rows r covers, which start at base (what: "the owned range", ...); rows [first, first + rows) of r's columns
// to the caller, in whichever order r is stored
int pct_check_owned_span(pct_ctx* ctx, const char* what, pct_resident r, int64_t begin, int64_t end, int64_t base);
int pct_get_rows(pct_ctx* ctx, pct_resident r, const pct_column* cols, int ncol, int64_t first, int64_t rows);
int pct_launch_export_rows(pct_ctx* ctx, const int64_t* d_rows, int64_t n_rows, int32_t* d_idx, float* d_dist, int32_t* d_cnt);
int pct_launch_mesh_energies(pct_ctx* ctx, const double* d_v, const int* d_tri, int64_t n_tri, const void* d_K, const void* d_H,
                             bool k_f64, bool h_f64, double* d_partial, int nblk, double* d_out);
// The surface stages.  A launcher enqueues its kernels and the copy of its statistics words into pinned memory; its
// pct_*_report, called once the stream has been waited for, turns those words into the public counters of rep->stats --
// the words' layout is known to the stage's file alone.  What a launcher knows on the host it writes into rep itself.
// pct_area.hip: areas of the owned rows of the resident table (*by_row: stored in table-row order), and the energies over
// them: d_out4 = {bending, stretching, area, rows used}
int pct_launch_point_areas(pct_ctx* ctx, bool* by_row);
void pct_area_report(pct_ctx* ctx, pct_stage_report* rep);
int pct_launch_point_energies(pct_ctx* ctx, bool closed_only, double* d_partial, double* d_out4);
// pct_frame.hip: surface frames of the owned rows of the resident table from its resident fit (viewpoint: three finite
// doubles or null; *by_row: stored in table-row order)
int pct_launch_point_frames(pct_ctx* ctx, const double* viewpoint, bool* by_row);
void pct_frame_report(pct_ctx* ctx, pct_stage_report* rep);
// pct_orient.hip: the flood over the resident table, the anchor and the apply pass on the resident frames of a whole-cloud
// handle; rep->stats[6] and [7] (kernel launches, host waits) are filled here, the rest by the report
int pct_run_orient(pct_ctx* ctx, int anchor, const double* viewpoint, int max_comp, pct_stage_report* rep);
void pct_orient_report(pct_ctx* ctx, pct_stage_report* rep);
// pct_fan.hip: fans and triangles of the resident table of a whole-cloud handle (mid: recorded between the fan kernels and
// the agreement; the report also leaves ctx->tri_total), and the natural neighbours of public rows [first, first + rows)
// as CSR (d_count: rows + 1 words of scratch)
int pct_launch_point_triangles(pct_ctx* ctx, bool wind_frames, hipEvent_t mid);
void pct_fan_report(pct_ctx* ctx, pct_stage_report* rep);
int pct_launch_point_fans(pct_ctx* ctx, int64_t first, int64_t rows, int64_t* d_count, int64_t* d_off, int* d_nbr);
// pct_hole.hip: gaps, loops, patches and the filled array of the resident fans and triangles; waits for the stream three
// times (the gap count, the loop and patch counts, the end) and leaves ctx->hole_loops / hole_loop_verts / hole_patches and
// rep->stats = {boundary edges, gaps, odd gaps, loops, filled, left for the perimeter, blocked, patch triangles}: every
// one of its words has been read on the host by then, so it has no report of its own
int pct_launch_fill_holes(pct_ctx* ctx, int max_vertices, double max_perimeter, pct_stage_report* rep);
int pct_voxel_downsample_device(pct_ctx* ctx, const void* d_xyz, bool f64, int64_t n, double voxel, int64_t* d_out, int64_t* count);
int pct_launch_surface_variation(pct_ctx* ctx, float* d_out);
// PCA principal curvatures (pct_pca.hip).  The sweep fetches up to PCT_PCA_EXTRA candidates beyond k per point, re-ranked
// in the cloud's dtype.  prep: non-finite coordinates; float64 clouds: the cloud recentred on its first point for the
// sweep (origin), the float32 rounding offset R of that; restore: the uploaded cloud back after the sweep
#define PCT_PCA_EXTRA 16
int pct_pca_prep(pct_ctx* ctx, double* round_off, bool* nonfinite, double origin[3]);
int pct_pca_restore(pct_ctx* ctx);
int pct_launch_pca(pct_ctx* ctx, int32_t k, double round2, const double origin[3], bool keep_neighbors, int64_t* exact_rows);

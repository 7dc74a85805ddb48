// Caller-supplied query points through the uniform cell list (pct_query_points_algo, PCT_QUERY_GRID): what
// PointCloud.kdtree.query(x, k) computes for the points of ANOTHER cloud, without reading all n cloud points per query.
//
// Semantics are k_query_points' (pct_knn.hip): candidates are the float32-rounded records of the cell-sorted cloud
// (.w = public index; native float64 coordinates are never candidates), the query is the caller's float64 point, the
// squared distance is ((dx*dx + dy*dy) + dz*dz) in fp64 without contraction, the order is (d2, public index), eps is
// strict, padding is index n and +inf.  Every comparison is on exact fp64 keys (Sweep<R>, pct_knn_sweep.h): no float32
// pre-selection here.
//
//   stage 1  pct_query_stage1 (pct_query_items.h, shared with pct_ball.hip, as are the item decode and the launch
//            geometry below): the cell of every query, the query indices sorted by cell, work items {cell, first
//            sorted query, <= kItemQ queries}.
//   stage 2  k_query_cells: one wave = one work item.  The item's 27-cell stencil is staged into LDS once (16-byte
//            records {x, y, z, sorted position}, PCT_STAGE_CAP2 of them per wave), Sweep<R> runs over the staged
//            candidates for each query of the item; a row is stored only if the 27 cells vouch for it
//            (min(tau, eps^2) <= query_guaranteed_r2(ring = 1)), every other query -- and every query of an item whose
//            stencil overflows the staging area -- goes to the redo list, one counter increment per item.
//   stage 3  k_query_exact: k_knn_exact's loop (pct_knn_sweep.h) for the redo list, the query read from the caller's
//            array: candidates shell by shell from global memory, one step ahead of their use, until the searched cube
//            vouches for the row or covers the grid.
// Rows go straight to the caller's (m, k) arrays in the caller's query order, sorted positions translated to public indices.
#include "pct_query_items.h"

namespace {

constexpr int kQueryCap = PCT_STAGE_CAP2;            // staged candidates per wave: 768 x 16 B = 12 KiB, 4 waves + their pending
                                                     // buffers ~ 57 KiB per block, two blocks per CU's 160 KiB

struct QueryArgs {
    const float4* pts;          // cell-sorted candidate records {x, y, z, public index}
    const int* cell_start;
    pct_grid g;
    const double* q;            // (m, 3) the caller's queries
    int64_t m;
    int n;                      // cloud size: the padding index
    int k;
    double eps2;                // +inf when no bound
    const unsigned* q_sorted;   // query indices in cell order
    const int4* items;          // {cell, first position in q_sorted, queries, 0}
    QueryWords* words;
    int* redo;                  // query indices handed to k_query_exact
    int* idx_out;
    double* dist_out;
};

// the k nearest of the running list -> row qi of the caller's arrays
template <int R>
__device__ __forceinline__ void store_query_row(const Sweep<R>& sw, const QueryArgs& a, int64_t qi, int lane) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = lane + 64 * r;
        if (i < a.k) {
            const bool real = sw.best.p[r] != INT_MAX;
            a.idx_out[qi * a.k + i] = real ? pub_index(a.pts, sw.best.p[r]) : a.n;
            a.dist_out[qi * a.k + i] = real ? sqrt(sw.best.d[r]) : (double)INFINITY;
        }
    }
}

template <int R>
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_query_cells(QueryArgs a) {
    __shared__ float4 s_stage[kWavesPerBlock][kQueryCap];
    __shared__ double s_pend_d[kWavesPerBlock][64 * R + 64];
    __shared__ int s_pend_p[kWavesPerBlock][64 * R + 64];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const pct_grid g = a.g;
    const int* __restrict__ cs = a.cell_start;
    float4* __restrict__ stage = s_stage[w];
    const int total = a.words->n_items;                // written by k_query_items, the launch before this one
    const int nwaves = (int)gridDim.x * kWavesPerBlock;

    Sweep<R> sw;
    sw.k = a.k - 1;                                    // the list keeps elements 0 .. sw.k: the k nearest
    sw.eps2 = a.eps2;
    sw.pts = a.pts;
    sw.pend_d = s_pend_d[w];
    sw.pend_p = s_pend_p[w];

    for (int item = (int)blockIdx.x * kWavesPerBlock + w; item < total; item += nwaves) {
        const QueryItem it = query_item(a.items, item, g);
        const int qs = it.qs, nq = it.nq, cx = it.cx, cy = it.cy, cz = it.cz;
        // bounds of the 9 x-runs of the 27-cell stencil, lanes 0..8 (centre row first); at the rim of the grid a run
        // is clamped to the row, rows outside the grid stay empty
        int run_s = 0, run_len = 0;
        if (lane < 9) {
            const int z = cz + kRowOrder[lane][0], y = cy + kRowOrder[lane][1];
            if (z >= 0 && z < g.nz && y >= 0 && y < g.ny) {
                const int row = (z * g.ny + y) * g.nx;
                run_s = cs[row + max(cx - 1, 0)];
                run_len = cs[row + min(cx + 1, g.nx - 1) + 1] - run_s;
            }
        }
        int my_pre = 0, mtot = 0;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            my_pre = lane == t ? mtot : my_pre;
            mtot += __builtin_amdgcn_readlane(run_len, t);
        }
        if (mtot > kQueryCap) {                        // the stencil does not fit: the exact sweep takes the whole item
            int base = 0;
            if (lane == 0) base = atomicAdd(&a.words->redo_count, nq);
            base = __builtin_amdgcn_readfirstlane(base);
            if (lane < nq) a.redo[base + lane] = (int)a.q_sorted[qs + lane];
            continue;
        }
        // ---- stage the stencil: the record with its sorted position in .w (the list keeps positions; the public index
        // is read from the cloud only where two distances tie, and when a row is stored)
        wave_lds_sync();                               // (the previous item's reads are done)
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int s0 = __builtin_amdgcn_readlane(run_s, t), len = __builtin_amdgcn_readlane(run_len, t);
            const int pre = __builtin_amdgcn_readlane(my_pre, t);
            for (int b = lane; b < len; b += 64) {     // pre + b < mtot <= kQueryCap
                float4 c = a.pts[s0 + b];
                c.w = __int_as_float(s0 + b);
                stage[pre + b] = c;
            }
        }
        wave_lds_sync();

        int my_redo = 0, nredo = 0;                    // lane j: the j-th query of this item the stencil cannot vouch for
        for (int j = 0; j < nq; ++j) {
            const int64_t qi = (int64_t)a.q_sorted[qs + j];
            sw.qx = a.q[3 * qi]; sw.qy = a.q[3 * qi + 1]; sw.qz = a.q[3 * qi + 2];
            sw.reset();
            for (int base = 0;; base += 64) {
                const bool have = base < mtot;
                if (have) {
                    const int slot = base + lane;
                    const bool valid = slot < mtot;
                    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (valid) c = stage[slot];
                    sw.consider(c, __float_as_int(c.w), valid);
                    if (sw.npend < 64 * R) continue;
                }
                if (sw.npend > 0 || sw.empty) sw.flush();
                if (!have) break;
            }
            const double gx = query_cell_offset(sw.qx, g.ox, g.inv_cell, cx);
            const double gy = query_cell_offset(sw.qy, g.oy, g.inv_cell, cy);
            const double gz = query_cell_offset(sw.qz, g.oz, g.inv_cell, cz);
            if (fmin(sw.tau_d, sw.eps2) <= query_guaranteed_r2(g.nx, g.ny, g.nz, g.cell, cx, cy, cz, gx, gy, gz, 1)) {
                store_query_row<R>(sw, a, qi, lane);
            } else {
                if (lane == nredo) my_redo = (int)qi;
                ++nredo;
            }
        }
        if (nredo > 0) {                               // one counter increment per item
            int base = 0;
            if (lane == 0) base = atomicAdd(&a.words->redo_count, nredo);
            base = __builtin_amdgcn_readfirstlane(base);
            if (lane < nredo) a.redo[base + lane] = my_redo;
        }
    }
}

// k_knn_exact's loop for the redo list.  Every loop ends: a shell is a finite set of runs (ShellIter), each round widens
// the cube (ring + 1, then by half the radius), and once the cube covers the grid -- after at most max(nx, ny, nz)
// widenings -- query_guaranteed_r2 is +inf and vouches for any row: the grid's extent bounds the work of a query.
template <int R>
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_query_exact(QueryArgs a) {
    __shared__ double s_pend_d[kWavesPerBlock][64 * R + 64];
    __shared__ int s_pend_p[kWavesPerBlock][64 * R + 64];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const pct_grid g = a.g;
    const int* __restrict__ cs = a.cell_start;
    const int total = a.words->redo_count;             // final: k_query_cells has completed
    const int nwaves = (int)gridDim.x * kWavesPerBlock;

    Sweep<R> sw;
    sw.k = a.k - 1;
    sw.eps2 = a.eps2;
    sw.pts = a.pts;
    sw.pend_d = s_pend_d[w];
    sw.pend_p = s_pend_p[w];

    int ring_max = 0;
    for (int item = (int)blockIdx.x * kWavesPerBlock + w; item < total; item += nwaves) {
        const int64_t qi = (int64_t)__builtin_amdgcn_readfirstlane(a.redo[item]);
        sw.qx = a.q[3 * qi]; sw.qy = a.q[3 * qi + 1]; sw.qz = a.q[3 * qi + 2];
        const int cx = __builtin_amdgcn_readfirstlane(query_cell_coord(sw.qx, g.ox, g.inv_cell, g.nx));
        const int cy = __builtin_amdgcn_readfirstlane(query_cell_coord(sw.qy, g.oy, g.inv_cell, g.ny));
        const int cz = __builtin_amdgcn_readfirstlane(query_cell_coord(sw.qz, g.oz, g.inv_cell, g.nz));
        sw.reset();
        const double gx = query_cell_offset(sw.qx, g.ox, g.inv_cell, cx);
        const double gy = query_cell_offset(sw.qy, g.oy, g.inv_cell, cy);
        const double gz = query_cell_offset(sw.qz, g.oz, g.inv_cell, cz);
        const bool inside = query_inside_cell(gx) && query_inside_cell(gy) && query_inside_cell(gz);
        ShellIter sh;
        sh.start(g, cy, cz, -1, 1);
        // candidate loads run one step ahead of their use (a shell is many short runs, each a dependent load)
        int nbase = 0, nlim = 0;
        bool have_next = sh.next(g, cs, cx, cy, cz, nbase, nlim);
        float4 c_next = make_float4(0.f, 0.f, 0.f, 0.f);
        if (have_next && nbase + lane < nlim) c_next = a.pts[nbase + lane];
        for (;;) {
            const bool have = have_next;
            if (have) {
                const int pos = nbase + lane;
                const bool valid = pos < nlim;
                const float4 c = c_next;
                have_next = sh.next(g, cs, cx, cy, cz, nbase, nlim);
                if (have_next && nbase + lane < nlim) c_next = a.pts[nbase + lane];
                sw.consider(c, pos, valid);
                if (sw.npend < 64 * R) continue;
            }
            if (sw.npend > 0 || sw.empty) sw.flush();
            if (have) continue;
            if (fmin(sw.tau_d, sw.eps2) <= query_guaranteed_r2(g.nx, g.ny, g.nz, g.cell, cx, cy, cz, gx, gy, gz, sh.ring)) break;
            // widen: one ring at a time near the query, then by half the radius (k_knn_exact's stride rule; the
            // guarantee is that of the outer radius)
            // The shell's pruning converts offsets near the query's in-cell position to int: only for a query inside
            // the box, whose position lies in [0, 1).  A clamped query (anywhere up to 1e300, its offset possibly +-inf)
            // widens unpruned: prune = +inf, and ShellIter::fetch then never reads the position.
            sh.start(g, cy, cz, sh.ring, sh.ring < 4 ? sh.ring + 1 : sh.ring + (sh.ring + 1) / 2, inside ? fmin(sw.tau_d, sw.eps2) : (double)INFINITY,
                     inside ? gx : 0.0, inside ? gy : 0.0, inside ? gz : 0.0);
            have_next = sh.next(g, cs, cx, cy, cz, nbase, nlim);
            if (have_next && nbase + lane < nlim) c_next = a.pts[nbase + lane];
        }
        ring_max = max(ring_max, sh.ring);
        store_query_row<R>(sw, a, qi, lane);
    }
    if (lane == 0 && ring_max > 0) atomicMax(&a.words->max_ring, ring_max);       // once per wave
}

}  // namespace

// m >= 1 queries (device array d_q) against the uniform cell list in place.  host_words4 = {work items, rows redone by
// the exact sweep, largest ring of those, 0} is complete once the stream has been waited for (the caller copies the rows
// anyway); rows stored by stage 2 = m - rows redone.
int pct_launch_query_grid(pct_ctx* ctx, const double* d_q, int64_t m, int32_t k, double eps, int32_t* d_idx, double* d_dist, int32_t* host_words4) {
    const pct_grid& g = ctx->grid;
    QueryItems st;
    PCT_TRY(pct_query_stage1(ctx, d_q, m, (size_t)m * sizeof(int), &st));       // extra: the redo list
    QueryWords* words = st.words;
    QueryArgs a = {};
    a.pts = (const float4*)ctx->sorted4.p;
    a.cell_start = (const int*)ctx->cell_cnt.p;
    a.g = g;
    a.q = d_q;
    a.m = m;
    a.n = (int)ctx->n;
    a.k = k;
    a.eps2 = eps > 0 ? eps * eps : (double)INFINITY;
    a.q_sorted = st.q_sorted;
    a.items = st.items;
    a.words = words;
    a.redo = (int*)st.extra;
    a.idx_out = d_idx;
    a.dist_out = d_dist;
    // device-side counts, fixed grids: at most m items / m redone queries, one per wave
    const dim3 block(64 * kWavesPerBlock), cells_grid(query_blocks(m)), exact_grid(query_blocks(m, 8192));
    if (k <= 64) {
        PCT_LAUNCH(k_query_cells<1>, cells_grid, block, 0, ctx->stream, a);
        PCT_LAUNCH(k_query_exact<1>, exact_grid, block, 0, ctx->stream, a);
    } else {
        PCT_LAUNCH(k_query_cells<2>, cells_grid, block, 0, ctx->stream, a);
        PCT_LAUNCH(k_query_exact<2>, exact_grid, block, 0, ctx->stream, a);
    }
    PCT_HIP(ctx, hipGetLastError());
    PCT_HIP(ctx, hipMemcpyAsync(host_words4, words, sizeof(QueryWords), hipMemcpyDeviceToHost, ctx->stream));
    return PCT_OK;
}

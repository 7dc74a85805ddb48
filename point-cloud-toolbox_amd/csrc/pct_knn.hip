// Neighbour sweep kernels: what PointCloud.plant_kdtree computes with one
// cKDTree.query(point, k+1) per point (pointCloudToolbox.py:81-85).
//
// Semantics reproduced: candidates are the float32-rounded coordinates
// (pct:74); squared distances are accumulated in fp64 as ((dx*dx + dy*dy) +
// dz*dz) with no FMA contraction, which is bit-for-bit what SciPy evaluates
// for 3-D data; the k+1 smallest are taken, result 0 is dropped (pct:84-85),
// and sqrt(d2) is rounded to float32 (pct:78).  Exact-distance ties are ordered
// by public index so the result does not depend on the cell order.
//
// Kernels (all hand-written for gfx950, 64-lane waves) and where they live:
//   k_knn_fast   (pct_knn_fast.hip) one wave = one work item (a cell and <= items_q of its owned queries).  The 27-cell
//                stencil is staged once into LDS (12 B per candidate, all global loads in flight together), the item's
//                queries are prefetched into registers.  Per PAIR of queries: float32 squared distances of all staged
//                candidates in packed arithmetic, a threshold that leaves k+1 .. 64 R of them (ballot counts,
//                secant steps), compaction of the survivors, exact fp64 keys for those only, ONE wave-wide
//                bitonic network in registers on 32-bit elements (DPP row operations, v_permlane16/32_swap,
//                v_med3_u32 compare-exchanges), proof checks, stores.  R = 1 holds k+1 <= 64, R = 2 k+1 <= 128.
//                Anything it cannot prove exact goes to the redo list (one counter increment per item).
//                Every form: level passes, owned subsets, clouds outside the float32 window, the A/B switches.
//   k_knn_pair   (pct_knn_pair.hip) the same sweep for the headline case -- one list register, a plain sweep -- written
//                for the scalar unit as much as for the vector units; what a default call takes up to k + 1 = 61.
//   k_knn_duo    (pct_knn_duo.hip) k_knn_pair's scheme for rows of up to 128 entries: one query per trip, two list registers.
//                The three share the start of a work item (pct_knn_item.h) and the sorting network (pct_knn_net.h);
//                which one a call takes is plan_sweep's rule (pct_sweep_plan.h).
//   k_knn_exact, k_knn_exact_tree  (pct_knn_sweep.h; R = 4, 8 in pct_knn_wide.hip) one wave = one query of the redo list
//                (or every query, for testing): candidates cube by cube from global memory, (fp64 d2, public index)
//                comparisons, shell-by-shell widening until the searched cube guarantees the answer.
//   k_knn_brute  (pct_knn_sweep.h) exhaustive sweep, wave per query: small clouds and the on-device cross-check.
//   k_query_points, k_export*, k_item_census, k_selftest*  (this file) caller-supplied queries; neighbour table (sorted
//                space, owned rows) -> public (rows, k) index / distance arrays; the work-item census; the self-tests of
//                the cross-lane primitives, the sorting networks and the repair of equal keys.
// This file also holds the host side of a sweep: the kernel argument, the table, the one launch of the planned kernel.
#include "pct_knn_net.h"

namespace {

// cKDTree.query for caller-supplied points (pct_query_points): the exhaustive sweep with the query read from a
// separate array and every element of the list stored (nothing is "the point itself" here).
__global__ __launch_bounds__(256) void k_plain_records(const float* __restrict__ xyz, int64_t n, float4* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], __int_as_float((int)i));
}

template <int R>
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_query_points(const float4* __restrict__ pts, int n, const double* __restrict__ q_xyz,
                                                                      int64_t m, int k, double eps2, int* __restrict__ idx_out,
                                                                      double* __restrict__ dist_out) {
    __shared__ double s_pend_d[kWavesPerBlock][64 * R + 64];
    __shared__ int s_pend_p[kWavesPerBlock][64 * R + 64];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const int64_t q = (int64_t)blockIdx.x * kWavesPerBlock + w;
    if (q >= m) return;
    Sweep<R> sw;
    sw.k = k - 1;                        // the list keeps elements 0 .. sw.k: the k nearest
    sw.eps2 = eps2;
    sw.pts = pts;
    sw.pend_d = s_pend_d[w];
    sw.pend_p = s_pend_p[w];
    sw.qx = q_xyz[3 * q]; sw.qy = q_xyz[3 * q + 1]; sw.qz = q_xyz[3 * q + 2];
    sw.reset();
    for (int base = 0;; base += 64) {
        const bool have = base < n;
        if (have) {
            const int pos = base + lane;
            const bool valid = pos < n;
            float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid) c = pts[pos];
            sw.consider(c, pos, valid);
            if (sw.npend < 64 * R) continue;
        }
        if (sw.npend > 0 || sw.empty) sw.flush();
        if (!have) break;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = lane + 64 * r;
        if (i < k) {
            const bool real = sw.best.p[r] != INT_MAX;
            idx_out[q * k + i] = real ? sw.best.p[r] : n;
            dist_out[q * k + i] = real ? sqrt(sw.best.d[r]) : (double)INFINITY;
        }
    }
}

// The float32 distance of a table entry, from the two records: the sweep's own expression -- fp64 ((dx^2 + dy^2) +
// dz^2) without contraction, correctly rounded root, one rounding to float32 (pct:78) -- so a table written without
// distances (the fused curvature call) yields the very bits the sweep would have stored.
__device__ __forceinline__ float table_distance(const float4* pts, const double4* ptsd, int qpos, const float4 c) {
    double qx, qy, qz;                 // the query as the sweep measured from it: native float64 coordinates where the cloud has them (pct:83)
    if (ptsd) { const double4 q = ptsd[qpos]; qx = q.x; qy = q.y; qz = q.z; }
    else { const float4 q = pts[qpos]; qx = (double)q.x; qy = (double)q.y; qz = (double)q.z; }
    const double dx = (double)c.x - qx, dy = (double)c.y - qy, dz = (double)c.z - qz;
    return (float)sqrt((dx * dx + dy * dy) + dz * dz);
}

// neighbour table -> public (rows,k) arrays for public rows [begin,end).  owned_pos == nullptr: the table came
// from the exhaustive sweep (row = public index - q_begin, entries = public indices).
__global__ __launch_bounds__(256) void k_export(const float4* __restrict__ pts, const double4* __restrict__ ptsd, const int* __restrict__ owned_pos, int q_begin,
                                                const int* __restrict__ nbr_pos, const float* __restrict__ nbr_dist,
                                                const int* __restrict__ nbr_cnt, int64_t n, int64_t n_rows, int k, int pitch,
                                                int64_t begin, int64_t end, int* __restrict__ idx_out,
                                                float* __restrict__ dist_out, int* __restrict__ cnt_out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = t / k;
    const int j = (int)(t - row * k);
    if (row >= n_rows) return;
    const int pub = owned_pos ? __float_as_int(pts[owned_pos[row]].w) : (int)row + q_begin;
    if (pub < begin || pub >= end) return;
    const int64_t o = (int64_t)(pub - begin) * k + j;
    const int pos = nbr_pos[row * pitch + j];
    const float4 c = pos < 0 ? make_float4(0.f, 0.f, 0.f, 0.f) : pts[pos];
    if (idx_out) idx_out[o] = pos < 0 ? (int)n : __float_as_int(c.w);
    if (dist_out) dist_out[o] = nbr_dist ? nbr_dist[row * pitch + j] : pos < 0 ? INFINITY : table_distance(pts, ptsd, owned_pos[row], c);
    if (cnt_out && j == 0) cnt_out[pub - begin] = nbr_cnt ? nbr_cnt[row] : k;
}

// the same for an explicit list of public rows (one block per listed row)
__global__ __launch_bounds__(128) void k_export_rows(const float4* __restrict__ pts, const double4* __restrict__ ptsd, const int* __restrict__ row_of, const int* __restrict__ owned_pos, int q_begin,
                                                     const int* __restrict__ nbr_pos, const float* __restrict__ nbr_dist,
                                                     const int* __restrict__ nbr_cnt, int64_t n, int k, int pitch,
                                                     const int64_t* __restrict__ rows, int* __restrict__ idx_out,
                                                     float* __restrict__ dist_out, int* __restrict__ cnt_out) {
    const int64_t r = blockIdx.x;
    const int64_t pub = rows[r];
    const int64_t row = row_of ? row_of[pub - q_begin] : pub - q_begin;
    for (int j = threadIdx.x; j < k; j += 128) {
        const int pos = nbr_pos[row * pitch + j];
        const float4 c = pos < 0 ? make_float4(0.f, 0.f, 0.f, 0.f) : pts[pos];
        if (idx_out) idx_out[r * k + j] = pos < 0 ? (int)n : __float_as_int(c.w);
        if (dist_out) dist_out[r * k + j] = nbr_dist ? nbr_dist[row * pitch + j] : pos < 0 ? INFINITY : table_distance(pts, ptsd, owned_pos[row], c);
    }
    if (cnt_out && threadIdx.x == 0) cnt_out[r] = nbr_cnt ? nbr_cnt[row] : k;
}

// lane_xor<S>() against the generic shuffle, every S (hardware self-test)
__global__ __launch_bounds__(64) void k_selftest(int* fails) {
    const int lane = lane_id();
    const int v = lane * 7919 + 13;
    int bad = 0;
    bad += lane_xor<1>(v) != __shfl_xor(v, 1);
    bad += lane_xor<2>(v) != __shfl_xor(v, 2);
    bad += lane_xor<4>(v) != __shfl_xor(v, 4);
    bad += lane_xor<8>(v) != __shfl_xor(v, 8);
    bad += lane_xor<16>(v) != __shfl_xor(v, 16);
    bad += lane_xor<32>(v) != __shfl_xor(v, 32);
    if (bad) atomicAdd(fails, bad);
}

// ---------------------------------------------------------------------------
// The wave-level sorters on caller-supplied lists (pct_selftest_sort, pct_selftest_sort_exact, pct_selftest_order_keys):
// one wave per list -- or per pair of lists, for the forms that sort two side by side -- several waves per block as in
// the sweeps, register j of a wave at  base + 64 j + lane.  Each kernel instantiates what a sweep instantiates and calls
// it the way the sweep does; nothing else is computed.
// ---------------------------------------------------------------------------
constexpr int net_regs(int net) { return net == PCT_NET_FAST1 ? 1 : net == PCT_NET_SETS2 ? 4 : 2; }      // list registers of a wave

template <int NET>
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_selftest_sort(const unsigned* __restrict__ in, unsigned* __restrict__ out, int n_waves, unsigned zero) {
    constexpr int NR = net_regs(NET);
    const int w = (int)blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (w >= n_waves) return;
    const int lane = lane_id();
    const SortLanes c = make_sort_lanes();
    const size_t base = (size_t)w * (64 * NR) + lane;
    unsigned raw[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) raw[j] = in[base + 64 * j];
    // `zero` is 0: the xor changes nothing, but it is a VALU write of every list register directly ahead of the network.
    // The assembly blocks assume exactly that of their caller (their leading s_nop 1 covers a DPP read two wait states
    // after it), so the blocks meet here the hazard window they meet in k_knn_pair / k_knn_duo -- a register that came
    // straight from a load would be settled long before and could hide a missing wait state.
    FastK<NR> t;
#pragma unroll
    for (int j = 0; j < NR; ++j) t.e[j] = raw[j] ^ zero;
    if constexpr (NET == PCT_NET_FAST1) fast_sort_from<1, 2>(t, c);
    else if constexpr (NET == PCT_NET_FAST2) fast_sort_from<2, 2>(t, c);
    else if constexpr (NET == PCT_NET_SETS1) fast_sort_sets<1, 2, 2>(t, c);
    else if constexpr (NET == PCT_NET_SETS2) fast_sort_sets<2, 2, 2>(t, c);
    else if constexpr (NET == PCT_NET_PAIR) sort_pair_asm(t.e[0], t.e[1], c);
    else sort_duo_asm(t.e[0], t.e[1], c);
#pragma unroll
    for (int j = 0; j < NR; ++j) out[base + 64 * j] = t.e[j];
}

// the exact sweep's sorters: MODE 0 / 1 = bitonic_sort_from<R, 2> ascending / descending, 2 = bitonic_merge_min<R> of
// list (d2, pos) (ascending) with batch (bd2, bpos) (descending)
template <int R, int MODE>
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_selftest_exact(const double* __restrict__ d2, const int* __restrict__ pos,
                                                                        const double* __restrict__ bd2, const int* __restrict__ bpos,
                                                                        const float4* __restrict__ pts, int n_lists,
                                                                        double* __restrict__ out_d2, int* __restrict__ out_pos) {
    const int w = (int)blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (w >= n_lists) return;
    const size_t base = (size_t)w * (64 * R) + lane_id();
    TopK<R> t;
#pragma unroll
    for (int r = 0; r < R; ++r) { t.d[r] = d2[base + 64 * r]; t.p[r] = pos[base + 64 * r]; }
    if constexpr (MODE == 2) {
        TopK<R> b;
#pragma unroll
        for (int r = 0; r < R; ++r) { b.d[r] = bd2[base + 64 * r]; b.p[r] = bpos[base + 64 * r]; }
        bitonic_merge_min<R>(t, b, pts);
    } else {
        bitonic_sort_from<R, 2>(t, MODE == 1, pts);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) { out_d2[base + 64 * r] = t.d[r]; out_pos[base + 64 * r] = t.p[r]; }
}

// order_equal_keys<R, SLOT_BITS> on each list: the exact value of payload p is d2[list][p], its position is p itself and
// its public index pts[list][p].w -- tables of 2^SLOT_BITS entries per list
template <int R, int SLOT_BITS>
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_selftest_order(const unsigned* __restrict__ elems, const double* __restrict__ d2,
                                                                        const float4* __restrict__ pts, int n_lists,
                                                                        unsigned* __restrict__ out, int* __restrict__ done) {
    const int w = (int)blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (w >= n_lists) return;
    const int lane = lane_id();
    const size_t base = (size_t)w * (64 * R) + lane;
    const double* const my_d2 = d2 + ((size_t)w << SLOT_BITS);
    unsigned e[R];
#pragma unroll
    for (int r = 0; r < R; ++r) e[r] = elems[base + 64 * r];
    const bool ok = order_equal_keys<R, SLOT_BITS>(e, pts + ((size_t)w << SLOT_BITS),
        [&](unsigned payload) { return my_d2[payload]; },
        [&](unsigned payload) { return (int)payload; });
#pragma unroll
    for (int r = 0; r < R; ++r) out[base + 64 * r] = e[r];
    if (lane == 0) done[w] = ok ? 1 : 0;
}

// One thread per work item: population and non-empty cells of its 27-cell stencil (pct_item_census).
__global__ __launch_bounds__(256) void k_item_census(const int2* __restrict__ items, int64_t n_items, int items_q,
                                                     const int* __restrict__ cs, const int* __restrict__ cell_own, pct_grid g, int k,
                                                     int cap, pct_dev_words* __restrict__ out) {
    __shared__ unsigned long long sh[4][4];
    unsigned long long v[4] = {0, 0, 0, 0};
    for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < n_items; it += (int64_t)gridDim.x * 256) {
        const int2 e = items[it];
        const int cell = e.x;
        const int cx = cell % g.nx, cy = (cell / g.nx) % g.ny, cz = cell / (g.nx * g.ny);
        const int nq = min(items_q, cell_own[cell] - e.y * items_q);
        int m = 0, occupied = 0;
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy) {
                const int z = cz + dz, y = cy + dy;
                if (z < 0 || z >= g.nz || y < 0 || y >= g.ny) continue;
                const int row = (z * g.ny + y) * g.nx;
                int prev = cs[row + max(cx - 1, 0)];
                for (int x = max(cx - 1, 0); x <= min(cx + 1, g.nx - 1); ++x) {
                    const int next = cs[row + x + 1];
                    occupied += next > prev;
                    m += next - prev;
                    prev = next;
                }
            }
        v[0] += (unsigned)nq;
        // the stencil vouches for about one cell edge around the query: on a surface that disc holds ~pi/9 of the
        // stencil's population, so a stencil below ~2.5 (k+1) points will mostly fail the proof ("short")
        if (m > cap) v[1] += (unsigned)nq;
        else if (2 * m < 5 * (k + 1)) v[2] += (unsigned)nq;
        else v[3] += (unsigned long long)nq * (unsigned)occupied;
    }
    for (int j = 0; j < 4; ++j) {
        for (int o = 32; o > 0; o >>= 1) v[j] += __shfl_xor(v[j], o);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][j] = v[j];
    }
    __syncthreads();
    if (threadIdx.x < 4) atomicAdd(&out->census[threadIdx.x], sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x]);
}

KnnArgs make_args(pct_ctx* ctx, int32_t k, double eps, bool grid, const LevelPass* pass = nullptr) {    // pass: the chained sweep's
    KnnArgs a = {};
    a.pts = (const float4*)(grid ? ctx->sorted4.p : ctx->pts4.p);
    a.ptsd = ctx->has_f64 ? (const double4*)(grid ? ctx->sorted4d.p : ctx->pts4d.p) : nullptr;
    a.cell_start = (const int*)ctx->cell_cnt.p;
    a.cell_own = (const int*)ctx->cell_own.p;
    a.own_start = (const int*)ctx->own_start.p;
    a.owned_pos = (const int*)ctx->owned_pos.p;
    a.n_owned = pct_call_rows(ctx, pass);
    a.occ = (const int*)ctx->occ.p;
    a.n_occ = ctx->n_occ;
    a.n = ctx->n;
    a.g = ctx->grid;
    a.k = k;
    a.pitch = (k + 3) & ~3;
    a.eps2 = eps > 0 ? eps * eps : INFINITY;
    a.q_begin = (int)ctx->q_begin;
    a.q_end = (int)ctx->q_end;
    a.nbr_pos = (int*)ctx->nbr_pos.p;
    a.nbr_dist = (float*)ctx->nbr_dist.p;
    a.nbr_cnt = eps > 0 ? (int*)ctx->nbr_cnt.p : nullptr;
    a.row_done = pass ? (int*)ctx->row_done.p : nullptr;
    a.redo_m = a.row_done ? (int*)ctx->redo_m.p : nullptr;
    a.counters = &pct_dev(ctx)->sweep;
    a.stats = ctx->collect_stats ? 1 : 0;
    return a;
}

int reserve_table(pct_ctx* ctx, int32_t k, double eps, bool with_dist = true, const LevelPass* pass = nullptr) {
    ctx->nbr_pitch = (k + 3) & ~3;                        // 16-byte aligned rows (the fit kernel reads int4)
    const size_t rows = (size_t)pct_call_rows(ctx, pass);
    PCT_TRY(pct_reserve(ctx, &ctx->nbr_pos, rows * ctx->nbr_pitch * sizeof(int)));
    if (with_dist) PCT_TRY(pct_reserve(ctx, &ctx->nbr_dist, rows * ctx->nbr_pitch * sizeof(float)));
    ctx->dist_valid = with_dist;
    if (eps > 0) PCT_TRY(pct_reserve(ctx, &ctx->nbr_cnt, rows * sizeof(int)));
    PCT_TRY(pct_reserve(ctx, &ctx->counters, sizeof(pct_dev_words)));
    if (!ctx->counters_clean) PCT_HIP(ctx, hipMemsetAsync(&pct_dev(ctx)->sweep, 0, sizeof(pct_sweep_words), ctx->stream));
    ctx->counters_clean = false;
    return PCT_OK;
}

// Which fast sweep a call takes is decided by plan_sweep (pct_sweep_plan.h) from plain values: what it reads of the
// handle, and every tuning switch (PCT_*: A/B aids, read per call -- tests flip them), is gathered here.
SweepPlan plan_for(const pct_ctx* ctx, int32_t k, double eps, bool tree, bool exact_only, int phase, bool want_dist, const LevelPass* pass) {
    const pct_grid& g = ctx->grid;
    const SweepInputs in = {ctx->n_items, ctx->has_f64, pass != nullptr, pass && pass->want, pct_fast_r1_max(), g.cell, g.ox, g.oy, g.oz, g.nx, g.ny, g.nz};
    const SweepSwitches sw = {pct_getenv("PCT_NO_PAIR") != nullptr, pct_getenv("PCT_NO_PAIR_KERNEL") != nullptr,
                              pct_getenv("PCT_NO_DUO_KERNEL") != nullptr, pct_getenv("PCT_KEEP_DIST") != nullptr};
    return plan_sweep(in, sw, k, eps, tree, exact_only, phase, want_dist);
}

// launched once: the family's own translation unit picks the instantiation
int launch_sweep(pct_ctx* ctx, const SweepPlan& p, const KnnArgs& a, int* redo, int* redo_count) {
    if (p.family == kNoSweep) return PCT_OK;
    if (p.family == kFast) pct_launch_sweep_fast(ctx, p, a, redo, redo_count);
    else if (p.family == kDuo) pct_launch_sweep_duo(ctx, p, a, redo, redo_count);
    else pct_launch_sweep_pair(ctx, p, a, redo, redo_count);
    PCT_HIP(ctx, hipGetLastError());
    ctx->tm.sweep_variant = p.variant();
    return PCT_OK;
}

}  // namespace

// phase 0: fast sweep + exact sweep of what it flagged (or, exact_only, the exact sweep of every query);
// phase 1: fast sweep only, the flagged rows stay in ctx->redo (level passes); phase 2: exact sweep of ctx->redo;
// phase 3 (pct_selftest_sweep): phase 0 -- its plan, its argument, its one launch -- without the exact sweep: the flagged
// rows stay in ctx->redo and the table is unfinished
int pct_launch_knn_grid(pct_ctx* ctx, int32_t k, double eps, bool exact_only, int phase, bool want_dist, pct_call_clock* clock, const LevelPass* pass) {
    const bool sweep_only = phase == 3;
    if (sweep_only) phase = 0;
    const int64_t n_rows = pct_call_rows(ctx, pass);
    const SweepPlan plan = plan_for(ctx, k, eps, false, exact_only, phase, want_dist, pass);
    if (phase != 2) {
        PCT_TRY(reserve_table(ctx, k, eps, plan.dist, pass));
        PCT_TRY(pct_reserve(ctx, &ctx->redo, ((size_t)n_rows + 16) * sizeof(int)));
        if (pass) PCT_TRY(pct_reserve(ctx, &ctx->redo_m, ((size_t)n_rows + 16) * sizeof(int)));
    }
    KnnArgs a = make_args(ctx, k, eps, true, pass);
    if (!ctx->dist_valid) a.nbr_dist = nullptr;
    int* redo_count = &pct_dev(ctx)->sweep.redo_count;
    int* redo = (int*)ctx->redo.p;
    const dim3 block(64 * kWavesPerBlock);
    // the words of the clock's boundaries (null: it records them): the first kernel launched here stamps the end of the cell
    // list; no fast sweep: one reading for both, knn_fast_ms = 0
    const bool fast = plan.family != kNoSweep;
    a.stamp_sweep = clock->word(PCT_ST_GRID_END);
    a.stamp_exact = clock->word(fast ? PCT_ST_FAST_END : PCT_ST_GRID_END);
    a.stamp_exact_also = fast ? nullptr : clock->word(PCT_ST_FAST_END);
    // k_knn_pair / k_knn_duo leave their lists in the rows they could not prove, and the exact sweep starts from them
    // (PCT_REDO_SEED=0, read per call: neither; an A/B aid)
    const char* seed_env = pct_getenv("PCT_REDO_SEED");
    a.redo_seed = plan.lean() && !plan.tree && phase == 0 && !(seed_env && seed_env[0] == '0' && seed_env[1] == 0);
    // ... and mark the rows whose list is the proven set of their 27 cells, which the exact sweep takes over whole
    // (Sweep::adopt; PCT_REDO_ADOPT=0, read per call: no marks)
    const char* adopt_env = pct_getenv("PCT_REDO_ADOPT");
    a.redo_adopt = a.redo_seed && !(adopt_env && adopt_env[0] == '0' && adopt_env[1] == 0);
    PCT_TRY(launch_sweep(ctx, plan, a, redo, redo_count));
    PCT_HIP(ctx, clock->boundary(PCT_ST_FAST_END, ctx->stream));      // end of the dominant kernel
    // exact pass: the flagged queries (device-side count, fixed grid) or, for testing, every query
    if (phase != 1 && !sweep_only) {
        const int64_t waves = exact_only ? n_rows : 32768;   // one query per wave for typical redo counts
        const int blocks = (int)((waves + kWavesPerBlock - 1) / kWavesPerBlock);
        const int* list = exact_only ? nullptr : redo;
        if (k + 1 <= 64)
            PCT_LAUNCH(k_knn_exact<1>, dim3(blocks), block, 0, ctx->stream, a, list, (const int*)redo_count);
        else if (k + 1 <= 128)
            PCT_LAUNCH(k_knn_exact<2>, dim3(blocks), block, 0, ctx->stream, a, list, (const int*)redo_count);
        else
            PCT_TRY(pct_launch_knn_exact_wide(ctx, a, blocks, list, (const int*)redo_count));
        PCT_HIP(ctx, hipGetLastError());
    }
    ctx->knn_sorted_space = true;
    return PCT_OK;
}

// Neighbour sweep on the hierarchical cell list (pct_build_tree): fast sweep over its work items, then the exact sweep
// on the same structure for what the fast one flagged.  The table is in Morton order (a sorted space like the uniform
// list's: sorted4, owned_pos = identity, row_of).
int pct_launch_knn_tree(pct_ctx* ctx, int32_t k, double eps, bool want_dist, pct_call_clock* clock) {
    if (ctx->q_begin != 0 || ctx->q_end != ctx->n) return pct_fail(ctx, PCT_ERR_INVALID, "the tree sweep takes whole clouds");
    const int64_t n_rows = ctx->n;
    const bool exact_only = pct_getenv("PCT_TREE_EXACT_ONLY") != nullptr;        // testing: every query through the exact sweep
    const SweepPlan plan = plan_for(ctx, k, eps, true, exact_only, 0, want_dist, nullptr);
    PCT_TRY(reserve_table(ctx, k, eps, plan.dist));
    PCT_TRY(pct_reserve(ctx, &ctx->redo, ((size_t)n_rows + 16) * sizeof(int)));
    KnnArgs a = make_args(ctx, k, eps, true);
    if (!ctx->dist_valid) a.nbr_dist = nullptr;
    a.tree_seg = (const int4*)ctx->tree_seg.p;
    a.tree_runs = (const int2*)ctx->tree_runs.p;
    a.tree_bits = ctx->tree_bits;
    a.tree_codes = (const unsigned long long*)ctx->tree_codes.p + ctx->n;     // second half: the sorted codes
    a.tree_lvl = (const unsigned char*)ctx->tree_lvl.p;
    a.tree_bucket = (const int*)ctx->tree_bucket.p;
    int* redo_count = &pct_dev(ctx)->sweep.redo_count;
    int* redo = (int*)ctx->redo.p;
    PCT_TRY(launch_sweep(ctx, plan, a, redo, redo_count));
    PCT_HIP(ctx, clock->boundary(PCT_ST_FAST_END, ctx->stream));
    const int blocks = (32768 + kWavesPerBlock - 1) / kWavesPerBlock;        // device-side count, fixed grid
    const int* list = exact_only ? nullptr : redo;
    if (k + 1 <= 64)
        PCT_LAUNCH(k_knn_exact_tree<1>, dim3(blocks), dim3(64 * kWavesPerBlock), 0, ctx->stream, a, list, (const int*)redo_count);
    else
        PCT_LAUNCH(k_knn_exact_tree<2>, dim3(blocks), dim3(64 * kWavesPerBlock), 0, ctx->stream, a, list, (const int*)redo_count);
    PCT_HIP(ctx, hipGetLastError());
    ctx->knn_sorted_space = true;
    return PCT_OK;
}

unsigned pct_redo_trusted_bit() { return kRedoTrusted; }

int pct_item_census(pct_ctx* ctx, int32_t k, unsigned long long out4[4]) {
    PCT_TRY(pct_reserve(ctx, &ctx->counters, sizeof(pct_dev_words)));
    PCT_HIP(ctx, hipMemsetAsync(pct_dev(ctx), 0, sizeof(pct_sweep_words), ctx->stream));      // (the census shares its words with the sweep's, cleared whole)
    ctx->counters_clean = false;
    const int cap = k + 1 <= pct_fast_r1_max() ? kStageCap : PCT_STAGE_CAP2_HOST;
    const int blocks = (int)((ctx->n_items + 255) / 256 < 1024 ? (ctx->n_items + 255) / 256 : 1024);
    if (blocks > 0) {
        PCT_LAUNCH(k_item_census, dim3(blocks), dim3(256), 0, ctx->stream, (const int2*)ctx->occ.p, ctx->n_items, ctx->items_q,
                           (const int*)ctx->cell_cnt.p, (const int*)ctx->cell_own.p, ctx->grid, k, cap, pct_dev(ctx));
        PCT_HIP(ctx, hipGetLastError());
    }
    PCT_HIP(ctx, hipMemcpyAsync(ctx->pin->census, pct_dev(ctx)->census, sizeof(ctx->pin->census), hipMemcpyDeviceToHost, ctx->stream));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(out4, ctx->pin->census, sizeof(ctx->pin->census));
    return PCT_OK;
}

int pct_launch_knn_brute(pct_ctx* ctx, int32_t k, double eps) {
    PCT_TRY(reserve_table(ctx, k, eps));
    KnnArgs a = make_args(ctx, k, eps, false);
    const int64_t nq = ctx->q_end - ctx->q_begin;
    const int blocks = (int)((nq + kWavesPerBlock - 1) / kWavesPerBlock);
    if (blocks > 0) {
        if (k + 1 <= 64)
            PCT_LAUNCH(k_knn_brute<1>, dim3(blocks), dim3(64 * kWavesPerBlock), 0, ctx->stream, a);
        else if (k + 1 <= 128)
            PCT_LAUNCH(k_knn_brute<2>, dim3(blocks), dim3(64 * kWavesPerBlock), 0, ctx->stream, a);
        else
            PCT_TRY(pct_launch_knn_brute_wide(ctx, a, blocks));
        PCT_HIP(ctx, hipGetLastError());
    }
    ctx->knn_sorted_space = false;
    return PCT_OK;
}

int pct_launch_export_neighbors(pct_ctx* ctx, int64_t begin, int64_t end, int32_t* d_idx, float* d_dist,
                                int32_t* d_cnt) {
    const bool sorted = ctx->knn_sorted_space;
    const int64_t n_rows = ctx->q_end - ctx->q_begin;
    const int64_t total = n_rows * ctx->k;
    const int blocks = (int)((total + 255) / 256);
    PCT_LAUNCH(k_export, dim3(blocks), dim3(256), 0, ctx->stream,
                       (const float4*)(sorted ? ctx->sorted4.p : ctx->pts4.p), sorted && ctx->has_f64 ? (const double4*)ctx->sorted4d.p : nullptr,
                       sorted ? (const int*)ctx->owned_pos.p : nullptr,
                       (int)ctx->q_begin, (const int*)ctx->nbr_pos.p, ctx->dist_valid ? (const float*)ctx->nbr_dist.p : nullptr,
                       ctx->eps > 0 ? (const int*)ctx->nbr_cnt.p : nullptr, ctx->n, n_rows, ctx->k, ctx->nbr_pitch, begin, end,
                       d_idx, d_dist, d_cnt);
    PCT_HIP(ctx, hipGetLastError());
    return PCT_OK;
}

int pct_launch_export_rows(pct_ctx* ctx, const int64_t* d_rows, int64_t n_rows, int32_t* d_idx, float* d_dist, int32_t* d_cnt) {
    const bool sorted = ctx->knn_sorted_space;
    if (sorted) PCT_TRY(pct_ensure_row_of(ctx));
    PCT_LAUNCH(k_export_rows, dim3((unsigned)n_rows), dim3(128), 0, ctx->stream,
                       (const float4*)(sorted ? ctx->sorted4.p : ctx->pts4.p), sorted && ctx->has_f64 ? (const double4*)ctx->sorted4d.p : nullptr,
                       sorted ? (const int*)ctx->row_of.p : nullptr,
                       sorted ? (const int*)ctx->owned_pos.p : nullptr,
                       (int)ctx->q_begin, (const int*)ctx->nbr_pos.p, ctx->dist_valid ? (const float*)ctx->nbr_dist.p : nullptr,
                       ctx->eps > 0 ? (const int*)ctx->nbr_cnt.p : nullptr, ctx->n, ctx->k, ctx->nbr_pitch, d_rows, d_idx,
                       d_dist, d_cnt);
    PCT_HIP(ctx, hipGetLastError());
    return PCT_OK;
}

// {x, y, z, index} records of every point in public order, kept apart from the sweep's own arrays (a side query or
// a diagnostics fit must not disturb a resident table)
int pct_ensure_plain_records(pct_ctx* ctx) {
    if (!ctx->qpts4_valid) {
        PCT_TRY(pct_reserve(ctx, &ctx->qpts4, (size_t)ctx->n * sizeof(float4)));
        PCT_LAUNCH(k_plain_records, dim3((unsigned)((ctx->n + 255) / 256)), dim3(256), 0, ctx->stream,
                           ctx->xyz_view, ctx->n, (float4*)ctx->qpts4.p);
        PCT_HIP(ctx, hipGetLastError());
        ctx->qpts4_valid = true;
    }
    return PCT_OK;
}

int pct_launch_query_points(pct_ctx* ctx, const double* d_q, int64_t m, int32_t k, double eps, int32_t* d_idx, double* d_dist) {
    PCT_TRY(pct_ensure_plain_records(ctx));
    const double eps2 = eps > 0 ? eps * eps : (double)INFINITY;
    const int blocks = (int)((m + kWavesPerBlock - 1) / kWavesPerBlock);
    if (k <= 64)
        PCT_LAUNCH(k_query_points<1>, dim3(blocks), dim3(64 * kWavesPerBlock), 0, ctx->stream,
                           (const float4*)ctx->qpts4.p, (int)ctx->n, d_q, m, k, eps2, d_idx, d_dist);
    else
        PCT_LAUNCH(k_query_points<2>, dim3(blocks), dim3(64 * kWavesPerBlock), 0, ctx->stream,
                           (const float4*)ctx->qpts4.p, (int)ctx->n, d_q, m, k, eps2, d_idx, d_dist);
    PCT_HIP(ctx, hipGetLastError());
    return PCT_OK;
}

int pct_launch_selftest(pct_ctx* ctx, int* d_fails) {
    PCT_LAUNCH(k_selftest, dim3(1), dim3(64), 0, ctx->stream, d_fails);
    PCT_HIP(ctx, hipGetLastError());
    return PCT_OK;
}

int pct_selftest_sort_regs(int network) { return network >= PCT_NET_FAST1 && network <= PCT_NET_DUO ? net_regs(network) : 0; }

int pct_launch_selftest_sort(pct_ctx* ctx, int network, const unsigned* d_in, int n_waves, unsigned* d_out) {
    const dim3 grid((unsigned)((n_waves + kWavesPerBlock - 1) / kWavesPerBlock)), block(64 * kWavesPerBlock);
    switch (network) {
#define PCT_NET_CASE(N) case N: PCT_LAUNCH(k_selftest_sort<N>, grid, block, 0, ctx->stream, d_in, d_out, n_waves, 0u); break
        PCT_NET_CASE(PCT_NET_FAST1); PCT_NET_CASE(PCT_NET_FAST2); PCT_NET_CASE(PCT_NET_SETS1);
        PCT_NET_CASE(PCT_NET_SETS2); PCT_NET_CASE(PCT_NET_PAIR); PCT_NET_CASE(PCT_NET_DUO);
#undef PCT_NET_CASE
        default: return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_sort: no network %d", network);
    }
    PCT_HIP(ctx, hipGetLastError());
    return PCT_OK;
}

namespace {
template <int R>
void launch_selftest_exact(pct_ctx* ctx, int mode, const double* d2, const int* pos, const double* bd2, const int* bpos, const float4* pts,
                           int n_lists, double* out_d2, int* out_pos) {
    const dim3 grid((unsigned)((n_lists + kWavesPerBlock - 1) / kWavesPerBlock)), block(64 * kWavesPerBlock);
    if (mode == PCT_EXACT_ASCENDING) PCT_LAUNCH_T((k_selftest_exact<R, 0>), grid, block, 0, ctx->stream, d2, pos, bd2, bpos, pts, n_lists, out_d2, out_pos);
    else if (mode == PCT_EXACT_DESCENDING) PCT_LAUNCH_T((k_selftest_exact<R, 1>), grid, block, 0, ctx->stream, d2, pos, bd2, bpos, pts, n_lists, out_d2, out_pos);
    else PCT_LAUNCH_T((k_selftest_exact<R, 2>), grid, block, 0, ctx->stream, d2, pos, bd2, bpos, pts, n_lists, out_d2, out_pos);
}
}  // namespace

int pct_launch_selftest_exact(pct_ctx* ctx, int regs, int mode, const double* d2, const int* pos, const double* bd2, const int* bpos,
                              const float4* pts, int n_lists, double* out_d2, int* out_pos) {
    if (mode != PCT_EXACT_ASCENDING && mode != PCT_EXACT_DESCENDING && mode != PCT_EXACT_MERGE_MIN)
        return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_sort_exact: no mode %d", mode);
    switch (regs) {
        case 1: launch_selftest_exact<1>(ctx, mode, d2, pos, bd2, bpos, pts, n_lists, out_d2, out_pos); break;
        case 2: launch_selftest_exact<2>(ctx, mode, d2, pos, bd2, bpos, pts, n_lists, out_d2, out_pos); break;
        case 4: launch_selftest_exact<4>(ctx, mode, d2, pos, bd2, bpos, pts, n_lists, out_d2, out_pos); break;
        case 8: launch_selftest_exact<8>(ctx, mode, d2, pos, bd2, bpos, pts, n_lists, out_d2, out_pos); break;
        default: return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_sort_exact: list registers are 1, 2, 4 or 8, not %d", regs);
    }
    PCT_HIP(ctx, hipGetLastError());
    return PCT_OK;
}

int pct_launch_selftest_order(pct_ctx* ctx, int regs, int slot_bits, const unsigned* elems, const double* d2, const float4* pts, int n_lists,
                              unsigned* out, int* done) {
    const dim3 grid((unsigned)((n_lists + kWavesPerBlock - 1) / kWavesPerBlock)), block(64 * kWavesPerBlock);
    // the pairs the sweeps instantiate: 6 | 7 slot bits behind a pre-selection (k_knn_pair, k_knn_duo, k_knn_fast), 9 | 10 without
    if (regs == 1 && slot_bits == 6) PCT_LAUNCH_T((k_selftest_order<1, 6>), grid, block, 0, ctx->stream, elems, d2, pts, n_lists, out, done);
    else if (regs == 1 && slot_bits == 9) PCT_LAUNCH_T((k_selftest_order<1, 9>), grid, block, 0, ctx->stream, elems, d2, pts, n_lists, out, done);
    else if (regs == 2 && slot_bits == 7) PCT_LAUNCH_T((k_selftest_order<2, 7>), grid, block, 0, ctx->stream, elems, d2, pts, n_lists, out, done);
    else if (regs == 2 && slot_bits == 10) PCT_LAUNCH_T((k_selftest_order<2, 10>), grid, block, 0, ctx->stream, elems, d2, pts, n_lists, out, done);
    else return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_order_keys: (regs, slot_bits) is (1, 6), (1, 9), (2, 7) or (2, 10), not (%d, %d)", regs, slot_bits);
    PCT_HIP(ctx, hipGetLastError());
    return PCT_OK;
}

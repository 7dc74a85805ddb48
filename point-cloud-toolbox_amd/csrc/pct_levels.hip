// Density-adaptive neighbour sweep: a chain of cell lists instead of one.
//
// One cell size serves one density: where the cloud is much sparser than the cells were sized for, the 27-cell
// stencil does not hold k+1 points and the query falls to the exact sweep's ring-by-ring widening; where it is
// much denser the stencil overflows the LDS staging area.  Both are correct but an order of magnitude slower
// (tools/density_probe.py: two densities 10:1 -> 3x, a 1/r scan -> 10x).  Here every query a pass could not
// answer records WHY (cells too small / too large for it) and from that the cell edge it wants: a first estimate
// from the population of its cell, then a bisection between the largest edge known too small and the smallest
// known too large.  The next pass takes the most populated one-octave band of wanted edges, sizes its cells for
// it, owns exactly those queries (every point is still binned as a candidate; the cells only span the owned
// points' bounding box) and sweeps them.  Answered rows are merged into a public-space table (row = public index
// - q_begin, entries = public indices -- the representation of the exhaustive sweep, so every consumer already
// understands it).  What is left after the passes goes to the exact sweep.
#include "pct_internal.h"
#include "pct_levels_plan.h"

#include <math.h>
#include <stdlib.h>
#include <time.h>

namespace {

// (the rule -- constants, bins, windows, classify, next_pass, closing_edge -- is pct_levels_plan.h; here are the kernels
// that evaluate it per query and the host loop that runs the passes)

__device__ __forceinline__ int pub_of(const float4* __restrict__ sorted4, int pos) { return __float_as_int(sorted4[pos].w); }

__global__ __launch_bounds__(256) void k_init_want(float* __restrict__ want, float2* __restrict__ bracket, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    want[i] = __int_as_float(0x7fc00000);                  // NaN: not pending
    bracket[i] = make_float2(-INFINITY, INFINITY);
}

// answered rows of the pass (sorted space) -> public-space table; they stop being pending
__global__ __launch_bounds__(256) void k_merge_rows(const float4* __restrict__ sorted4, const int* __restrict__ owned_pos, int q_begin,
                                                    const int* __restrict__ nbr_pos, const float* __restrict__ nbr_dist,
                                                    const int* __restrict__ nbr_cnt, const int* __restrict__ row_done,
                                                    int64_t n_rows, int k, int pitch, int* __restrict__ pub_pos,
                                                    float* __restrict__ pub_dist, int* __restrict__ pub_cnt,
                                                    float* __restrict__ want) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = t / k;
    const int j = (int)(t - row * k);
    if (row >= n_rows || !row_done[row]) return;
    const int pub = pub_of(sorted4, owned_pos[row]);
    const int64_t out_row = (int64_t)pub - q_begin;
    const int pos = nbr_pos[row * pitch + j];
    pub_pos[out_row * pitch + j] = pos < 0 ? -1 : pub_of(sorted4, pos);
    pub_dist[out_row * pitch + j] = nbr_dist[row * pitch + j];
    if (j == 0) {
        if (pub_cnt) pub_cnt[out_row] = nbr_cnt ? nbr_cnt[row] : k;
        want[pub] = __int_as_float(0x7fc00000);
    }
}

// rows the pass left unanswered: update the bracket of the query's wanted edge and the wanted edge itself
__global__ __launch_bounds__(256) void k_classify(const int* __restrict__ row_done, const int* __restrict__ redo_m, int64_t n_rows,
                                                  const float4* __restrict__ sorted4, const int* __restrict__ owned_pos,
                                                  float log_edge, float target,
                                                  float* __restrict__ want, float2* __restrict__ bracket) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_rows; i += (int64_t)gridDim.x * 256) {
        if (row_done[i]) continue;
        const unsigned e = (unsigned)redo_m[i];      // the row's own slot: why << 29 | stencil population
        const int why = (int)(e >> 29);
        const int pub = pub_of(sorted4, owned_pos[i]);
        const float pop = (float)(e & 0x1FFFFFFFu);  // candidates the 27-cell stencil of the query's item held
        const float2 b = bracket[pub];
        const LevelWant c = classify(why, pop, log_edge, target, LevelBracket{b.x, b.y});
        bracket[pub] = make_float2(c.bracket.x, c.bracket.y);
        want[pub] = c.want;
    }
}

struct BandStats {
    unsigned hist[kBins];          // pending queries per quarter octave of wanted edge
    unsigned exact;                // pending queries only the exact sweep can answer
    unsigned pad;
};
static_assert(sizeof(BandStats) <= sizeof(pct_pinned::band_stats) && alignof(BandStats) <= 64, "pct_pinned::band_stats holds a BandStats");

__global__ __launch_bounds__(256) void k_band_hist(const float* __restrict__ want, int64_t begin, int64_t end, float log_edge0,
                                                   BandStats* __restrict__ out) {
    __shared__ unsigned sh[kBins + 1];
    for (int i = threadIdx.x; i <= kBins; i += 256) sh[i] = 0;
    __syncthreads();
    for (int64_t i = begin + (int64_t)blockIdx.x * 256 + threadIdx.x; i < end; i += (int64_t)gridDim.x * 256) {
        const float w = want[i];
        if (w == w) {                                   // bin_of(w, log_edge0), one atomic per class
            if (wants_exact(w)) atomicAdd(&sh[kBins], 1u);
            else atomicAdd(&sh[banded_bin(w, log_edge0)], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kBins; i += 256)
        if (sh[i]) atomicAdd(&out->hist[i], sh[i]);
    if (threadIdx.x == 0 && sh[kBins]) atomicAdd(&out->exact, sh[kBins]);
}

__device__ __forceinline__ int float_order_i(float f) {
    int i = __float_as_int(f);
    return i >= 0 ? i : i ^ 0x7fffffff;
}

// bounding box (ordered ints) and count of the points whose wanted edge lies in [lo, hi)
__global__ __launch_bounds__(256) void k_band_box(const float* __restrict__ want, const float* __restrict__ xyz, int64_t begin,
                                                  int64_t end, float lo, float hi, int* __restrict__ box, unsigned* __restrict__ count) {
    __shared__ int s_box[4][6];
    __shared__ unsigned s_cnt[4];
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    unsigned cnt = 0;
    for (int64_t i = begin + (int64_t)blockIdx.x * 256 + threadIdx.x; i < end; i += (int64_t)gridDim.x * 256) {
        const float w = want[i];
        if (in_window(w, lo, hi)) {
            ++cnt;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float v = xyz[3 * i + a];
                mn[a] = fminf(mn[a], v);
                mx[a] = fmaxf(mx[a], v);
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            mn[a] = fminf(mn[a], __shfl_xor(mn[a], o));
            mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o));
        }
    }
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        for (int a = 0; a < 3; ++a) { s_box[w][a] = float_order_i(mn[a]); s_box[w][3 + a] = float_order_i(mx[a]); }
        s_cnt[w] = cnt;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        int lo_i = s_box[0][a], hi_i = s_box[0][3 + a];
        for (int w = 1; w < 4; ++w) { lo_i = min(lo_i, s_box[w][a]); hi_i = max(hi_i, s_box[w][3 + a]); }
        atomicMin(&box[a], lo_i);
        atomicMax(&box[3 + a], hi_i);
    }
    if (threadIdx.x == 3) atomicAdd(count, s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]);
}

float order_to_float(int i) {
    const int j = i >= 0 ? i : i ^ 0x7fffffff;
    float f;
    memcpy(&f, &j, 4);
    return f;
}

// The launches of the rule's kernels with the grid sizes of the chain: pct_knn_levels and the self-test entries
// (pct_launch_selftest_levels_*) both go through these, so the self-tests run what the chain runs.
int launch_classify(pct_ctx* ctx, const int* row_done, const int* redo_m, int64_t n_rows, const float4* sorted4, const int* owned_pos,
                    float log_edge, float target, float* want, float2* bracket) {
    PCT_LAUNCH(k_classify, dim3(1024), dim3(256), 0, ctx->stream, row_done, redo_m, n_rows, sorted4, owned_pos, log_edge, target, want, bracket);
    PCT_HIP(ctx, hipGetLastError());
    return PCT_OK;
}

int launch_merge_rows(pct_ctx* ctx, const float4* sorted4, const int* owned_pos, int q_begin, const int* nbr_pos, const float* nbr_dist,
                      const int* nbr_cnt, const int* row_done, int64_t n_rows, int k, int pitch, int* pub_pos, float* pub_dist, int* pub_cnt,
                      float* want) {
    const int64_t total = n_rows * k;
    PCT_LAUNCH(k_merge_rows, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, sorted4, owned_pos, q_begin, nbr_pos, nbr_dist,
                       nbr_cnt, row_done, n_rows, k, pitch, pub_pos, pub_dist, pub_cnt, want);
    PCT_HIP(ctx, hipGetLastError());
    return PCT_OK;
}

// d_st: cleared, then the histogram of want[begin, end)
int launch_band_hist(pct_ctx* ctx, const float* want, int64_t begin, int64_t end, float log_edge0, BandStats* d_st) {
    PCT_HIP(ctx, hipMemsetAsync(d_st, 0, sizeof(BandStats), ctx->stream));
    PCT_LAUNCH(k_band_hist, dim3(512), dim3(256), 0, ctx->stream, want, begin, end, log_edge0, d_st);
    PCT_HIP(ctx, hipGetLastError());
    return PCT_OK;
}

// d_box (7 ints): the empty box in ordered ints and a count of 0, then box and count of the members of [lo, hi)
constexpr int kBandBoxWords = 7;
int launch_band_box(pct_ctx* ctx, const float* want, const float* xyz, int64_t begin, int64_t end, float lo, float hi, int* d_box) {
    static const int init[kBandBoxWords] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN, 0};
    PCT_HIP(ctx, hipMemcpyAsync(d_box, init, sizeof(init), hipMemcpyHostToDevice, ctx->stream));
    PCT_LAUNCH(k_band_box, dim3(512), dim3(256), 0, ctx->stream, want, xyz, begin, end, lo, hi, d_box, (unsigned*)(d_box + 6));
    PCT_HIP(ctx, hipGetLastError());
    return PCT_OK;
}

}  // namespace

int pct_knn_levels(pct_ctx* ctx, int32_t k, double eps, const int* fuse_par, pct_call_clock* clock) {
    ctx->pin->svd_rows[fuse_par ? *fuse_par : 0] = 0;                   // rows the passes' fits hand to k_fit_svd: summed over the passes of this call
    const int64_t nq = ctx->q_end - ctx->q_begin;
    if (ctx->n >= ((int64_t)1 << 29)) return pct_fail(ctx, PCT_ERR_INVALID, "the chained sweep handles clouds below 2^29 points");
    const int pitch = (k + 3) & ~3;
    const double factor = ctx->occupancy_factor > 0 ? ctx->occupancy_factor : pct_default_factor(k);
    const double target = factor * (k + 1);
    const bool debug = pct_getenv("PCT_LEVELS_DEBUG") != nullptr;

    ctx->no_cull = true;            // the merged table and the public-space fit need every point packed
    LevelPass pass;                 // what the pass in hand asks of the build and the sweep; the first one: every owned query by index
    int passes = 0;

    // one pass over the owned set in place: cell list, fast sweep (or the exact one), wanted edges, merge
    const auto tick = [&]() -> double {
        (void)hipStreamSynchronize(ctx->stream);
        struct timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
    };
    const auto run_pass = [&](int64_t owned, bool exact) -> int {
        const double t0 = debug ? tick() : 0;
        GridVerdict built;                                       // (nobody to give up for: always Built)
        PCT_TRY(pct_build_grid(ctx, k, eps, false, &built, nullptr, &pass));
        const double t1 = debug ? tick() : 0;
        PCT_TRY(pct_reserve(ctx, &ctx->row_done, (size_t)owned * sizeof(int)));
        PCT_HIP(ctx, hipMemsetAsync(ctx->row_done.p, 0, (size_t)owned * sizeof(int), ctx->stream));
        PCT_TRY(pct_launch_knn_grid(ctx, k, eps, exact, exact ? 0 : 1, true, clock, &pass));      // (k_merge_rows below reads the distances)
        if (!exact) {
            // the stencil of a well-sized pass holds about 11 cells' worth of points on a surface
            PCT_TRY(launch_classify(ctx, (const int*)ctx->row_done.p, (const int*)ctx->redo_m.p, owned, (const float4*)ctx->sorted4.p,
                                    (const int*)ctx->owned_pos.p, (float)log2(ctx->grid.cell), (float)(11.0 * target),
                                    (float*)ctx->flag_buf.p, (float2*)ctx->dens_buf.p));
        }
        if (fuse_par) PCT_TRY(pct_launch_fit_pass(ctx, owned, *fuse_par));       // before the next pass reorders the cloud
        const double t2 = debug ? tick() : 0;
        PCT_TRY(launch_merge_rows(ctx, (const float4*)ctx->sorted4.p, (const int*)ctx->owned_pos.p, (int)ctx->q_begin,
                                  (const int*)ctx->nbr_pos.p, (const float*)ctx->nbr_dist.p,
                                  eps > 0 ? (const int*)ctx->nbr_cnt.p : nullptr, (const int*)ctx->row_done.p, owned, k, pitch,
                                  (int*)ctx->pub_pos.p, (float*)ctx->pub_dist.p, eps > 0 ? (int*)ctx->pub_cnt.p : nullptr,
                                  (float*)ctx->flag_buf.p));
        if (debug) {
            const double t3 = tick();
            fprintf(stderr, "[levels] pass %d: owned %lld exact %d | build %.3f ms (iters %d, %lld cells) sweep+classify %.3f merge %.3f\n", passes,
                    (long long)owned, (int)exact, t1 - t0, ctx->tm.grid_iters, (long long)ctx->grid.ncell, t2 - t1, t3 - t2);
        }
        ++passes;
        return PCT_OK;
    };

    PCT_TRY(pct_reserve(ctx, &ctx->pub_pos, (size_t)nq * pitch * sizeof(int)));
    PCT_TRY(pct_reserve(ctx, &ctx->pub_dist, (size_t)nq * pitch * sizeof(float)));
    if (eps > 0) PCT_TRY(pct_reserve(ctx, &ctx->pub_cnt, (size_t)nq * sizeof(int)));
    PCT_TRY(pct_reserve(ctx, &ctx->flag_buf, (size_t)ctx->n * sizeof(float)));
    PCT_TRY(pct_reserve(ctx, &ctx->dens_buf, (size_t)ctx->n * sizeof(float2)));
    pct_stage_scope stage(ctx);      // the band statistics, for all the passes
    char* d_bands = nullptr;
    PCT_TRY(pct_claim(ctx, sizeof(BandStats) + 64, &d_bands));
    PCT_LAUNCH(k_init_want, dim3((unsigned)((ctx->n + 255) / 256)), dim3(256), 0, ctx->stream, (float*)ctx->flag_buf.p,
                       (float2*)ctx->dens_buf.p, ctx->n);
    PCT_HIP(ctx, hipGetLastError());
    // pass 0: every owned query, cells sized as for a plain sweep
    PCT_TRY(run_pass(nq, false));
    // the later passes bin the points in THIS pass's cell order (lanes of a wave then share their cells: the
    // histogram's atomics combine, k_hist_agg) and reuse its box (pass.base_box, the build's answer)
    PCT_TRY(pct_reserve(ctx, &ctx->lvl_src, (size_t)ctx->n * sizeof(float4)));
    PCT_HIP(ctx, hipMemcpyAsync(ctx->lvl_src.p, ctx->sorted4.p, (size_t)ctx->n * sizeof(float4), hipMemcpyDeviceToDevice, ctx->stream));
    pass.base = ctx->n_grid == ctx->n ? (const float4*)ctx->lvl_src.p : nullptr;
    pass.want = (const float*)ctx->flag_buf.p;
    float band_box[6];               // of the owned points of a banded pass
    const float log_edge0 = (float)log2(ctx->grid.cell);
    BandStats* d_st = (BandStats*)d_bands;
    int* d_box = (int*)(d_bands + sizeof(BandStats));        // 6 ints + count
    BandStats st;
    int64_t pending = 0;
    for (;;) {
        PCT_TRY(launch_band_hist(ctx, (const float*)ctx->flag_buf.p, ctx->q_begin, ctx->q_end, log_edge0, d_st));
        PCT_HIP(ctx, hipMemcpyAsync(ctx->pin->band_stats, d_st, sizeof(BandStats), hipMemcpyDeviceToHost, ctx->stream));
        PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        memcpy(&st, ctx->pin->band_stats, sizeof(BandStats));
        // the one-octave window that holds the most queries, or the end of the chain (pct_levels_plan.h)
        const NextPass next = next_pass(st.hist, st.exact, passes, nq, log_edge0);
        pending = next.pending;
        if (debug)
            fprintf(stderr, "[levels] after pass %d (edge %.5g, %lld cells): pending %lld (exact-only %u), best octave at edge %.5g holds %lld\n",
                    passes - 1, ctx->grid.cell, (long long)ctx->grid.ncell, (long long)pending, st.exact,
                    exp2(log_edge0 + kBinLo + 0.25 * (next.best + 2)), (long long)next.best_cnt);
        if (next.stop) break;
        pass.lo = next.lo;
        pass.hi = next.hi;
        PCT_TRY(launch_band_box(ctx, (const float*)ctx->flag_buf.p, ctx->xyz_view, ctx->q_begin, ctx->q_end, pass.lo, pass.hi, d_box));
        PCT_HIP(ctx, hipMemcpyAsync(ctx->pin->band_box, d_box, kBandBoxWords * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const int* hb = ctx->pin->band_box;
        for (int a = 0; a < 6; ++a) band_box[a] = order_to_float(hb[a]);
        pass.box = band_box;
        pass.owned = (int64_t)(unsigned)hb[6];
        if (pass.owned <= 0) break;            // (cannot happen while histogram and window agree; never build a cell list for nobody)
        pass.edge = next.edge;                 // centre of the window
        PCT_TRY(run_pass(pass.owned, false));
    }
    if (pending > 0) {               // the exact sweep answers whatever is left, over the whole box
        pass.lo = -INFINITY;
        pass.hi = INFINITY;
        pass.owned = pending;
        pass.box = nullptr;
        pass.edge = closing_edge(st.hist, log_edge0);
        PCT_TRY(run_pass(pending, true));
    }
    // the merged table takes the place of the pass table: public space, as after the exhaustive sweep
    ctx->nbr_pos.swap(ctx->pub_pos);
    ctx->nbr_dist.swap(ctx->pub_dist);
    if (eps > 0) ctx->nbr_cnt.swap(ctx->pub_cnt);
    ctx->nbr_pitch = pitch;
    ctx->knn_sorted_space = false;
    ctx->tm.levels = passes;
    return PCT_OK;
}

// ---- the rule's kernels on caller-supplied device arrays (pct_selftest_levels_*): nothing of the handle but its stream -------
int pct_launch_selftest_levels_classify(pct_ctx* ctx, const int* row_done, const int* redo_m, int64_t n_rows, const float4* sorted4,
                                        const int* owned_pos, float log_edge, float target, float* want, float* bracket2) {
    return launch_classify(ctx, row_done, redo_m, n_rows, sorted4, owned_pos, log_edge, target, want, (float2*)bracket2);
}

// stats: kBins + 2 words (BandStats); window >= 0: [lo, hi) of the window of bins that starts there, as the chain's
// host loop takes them from the plan; used2: the bounds the box kernel ran with; box7: six ordered ints and the count
int pct_launch_selftest_levels_bands(pct_ctx* ctx, const float* want, const float* xyz, int64_t begin, int64_t end, float log_edge0,
                                     int window, float lo, float hi, unsigned* stats, float used2[2], int* box7) {
    static_assert(sizeof(BandStats) == (kBins + 2) * sizeof(unsigned), "BandStats is its words");
    if (window >= 0) {
        lo = window_lo(log_edge0, window);
        hi = window_hi(log_edge0, window);
    }
    used2[0] = lo;
    used2[1] = hi;
    PCT_TRY(launch_band_hist(ctx, want, begin, end, log_edge0, (BandStats*)stats));
    return launch_band_box(ctx, want, xyz, begin, end, lo, hi, box7);
}

float pct_levels_box_float(int ordered) { return order_to_float(ordered); }

int pct_launch_selftest_levels_merge(pct_ctx* ctx, const float4* sorted4, const int* owned_pos, int q_begin, const int* nbr_pos,
                                     const float* nbr_dist, const int* nbr_cnt, const int* row_done, int64_t n_rows, int k, int pitch,
                                     int* pub_pos, float* pub_dist, int* pub_cnt, float* want) {
    return launch_merge_rows(ctx, sorted4, owned_pos, q_begin, nbr_pos, nbr_dist, nbr_cnt, row_done, n_rows, k, pitch, pub_pos, pub_dist,
                             pub_cnt, want);
}

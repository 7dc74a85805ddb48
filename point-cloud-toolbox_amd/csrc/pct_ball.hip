// Radius search for caller-supplied query points (pct_query_ball): what SciPy's tree answers to query_ball_point, as CSR
// rows of any length.
//
// Semantics (include/pct_hip.h): candidates are the float32-rounded records of the cloud, the query is the caller's
// float64 point, d2 = ((dx*dx + dy*dy) + dz*dz) in fp64 without contraction, a candidate is a member when d2 <= r*r
// (inclusive).  There is no ranking, so there is no running list: a pass over a query's candidates is a ballot per 64.
//
//   stage 1  pct_query_stage1 (pct_query_items.h, shared with pct_query.hip, as are the item decode and the launch
//            geometry below): the queries' cells, their order by cell, work items of <= kItemQ queries of one cell.
//   count    k_ball_count: one wave = one work item.  Every query's cube half-width is ball_ring (pct_ball_plan.h).  Where
//            the cube of the item's largest ring has at most 64 (y, z) rows (ring <= kBallStageRing) and at most kBallCap
//            candidates it is staged into LDS once for all queries of the item; otherwise every query streams its own
//            cube from global memory, run by run (ShellIter) with the loads one step ahead of their use -- or, where
//            ball_streams says so, the whole cell-sorted cloud linearly.  One int64 count per query.
//   scan     rocprim::exclusive_scan of the counts into int64 offsets[m + 1].
//   fill     k_ball_fill: the same enumeration and predicate.  The wave owns its query's row: the write position is a
//            wave-uniform cursor plus the rank of the lane within the ballot.  No atomics on rows, no scratch sized by
//            the candidates.
//   sort     (PCT_BALL_SORTED) k_ball_sort: ascending public index, in registers for rows of <= 64 entries, in LDS up to
//            kBallSortCap; if any row is longer, the library's segmented sort takes all rows instead.
//   dist     (PCT_BALL_DISTANCES) unsorted rows get sqrt(d2) from the fill; sorted rows from k_ball_dist afterwards, one
//            thread per entry, the same expression from (the row's query, the entry's record).
// The exhaustive path (k_ball_count_all / k_ball_fill_all) is the linear stream over the records in public order, one
// wave per query.
#include "pct_query_items.h"
#include "pct_ball_plan.h"

#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace {

constexpr int kBallCap = PCT_STAGE_CAP2;       // staged candidates per wave: 768 x 16 B = 12 KiB, 48 KiB per block of 4 waves:
                                               // three blocks per CU's 160 KiB (k_query_cells: two)
constexpr int kBallStageRing = 3;              // 7 x 7 = 49 (y, z) rows: their run bounds are one load per lane
constexpr int kBallSortCap = 1024;             // longest row k_ball_sort takes: 4 KiB of keys per wave

struct BallWords { int staged, streamed, max_ring, reserved; };     // device words of one call, cleared before it

struct BallArgs {
    const float4* pts;          // grid: cell-sorted records; exhaustive: records in public order.  .w = public index
    const int* cell_start;
    pct_grid g;
    int n;
    const double* q;            // (m, 3)
    int64_t m;
    const double* r;            // one radius, or m of them
    int r_stride;               // 0 | 1
    const unsigned* q_sorted;
    const int4* items;
    const QueryWords* words;
    BallWords* stat;
    int64_t* counts;            // count pass
    const int64_t* offsets;     // fill pass
    int* idx;
    double* dist;               // null: no distances from the fill
};

// One query's row while its candidates pass by: the count, or the write position.
template <bool FILL>
struct BallRow {
    double qx, qy, qz, r2;
    int64_t cursor, end;        // fill: the row's write position and its end (a write past it is dropped: the tests would show
                                // the row, the device no stray store)
    int* idx;
    double* dist;
    __device__ __forceinline__ void consider(const float4 c, bool valid) {
        const double dx = (double)c.x - qx, dy = (double)c.y - qy, dz = (double)c.z - qz;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        const bool pass = valid && d2 <= r2;           // inclusive; a NaN r2 keeps nothing
        const unsigned long long mask = __ballot(pass);
        if (FILL && pass) {
            const int64_t at = cursor + __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
            if (at < end) {
                idx[at] = __float_as_int(c.w);
                if (dist) dist[at] = sqrt(d2);
            }
        }
        cursor += __popcll(mask);
    }
    // all n records of `pts`, 64 at a time, the next load issued before the current one is used
    __device__ __forceinline__ void stream(const float4* __restrict__ pts, int n, int lane) {
        float4 c_next = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane < n) c_next = pts[lane];
        for (int base = 0; base < n; base += 64) {     // n <= INT32_MAX - 1024: base + 128 does not overflow
            const float4 c = c_next;
            const bool valid = base + lane < n;
            if (base + 64 + lane < n) c_next = pts[base + 64 + lane];
            consider(c, valid);
        }
    }
};

template <bool FILL>
__device__ __forceinline__ void ball_items(const BallArgs& a, float4* __restrict__ stage) {
    const int lane = lane_id();
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const pct_grid g = a.g;
    const int* __restrict__ cs = a.cell_start;
    const int total = a.words->n_items;                // written by k_query_items, launches before this one
    const int nwaves = (int)gridDim.x * kWavesPerBlock;
    int n_staged = 0, n_streamed = 0, ring_max = 0;

    BallRow<FILL> row;
    row.idx = a.idx;
    row.dist = a.dist;

    for (int item = (int)blockIdx.x * kWavesPerBlock + w; item < total; item += nwaves) {
        const QueryItem it = query_item(a.items, item, g);
        const int qs = it.qs, nq = it.nq, cx = it.cx, cy = it.cy, cz = it.cz;
        // lane j < nq: the j-th query of the item, its r*r and its ring
        int my_ring = -1;
        double my_r2 = 0.0;
        if (lane < nq) {
            const int64_t qi = (int64_t)a.q_sorted[qs + lane];
            const double r = a.r[qi * a.r_stride];
            my_r2 = r * r;
            const double gx = query_cell_offset(a.q[3 * qi], g.ox, g.inv_cell, cx);
            const double gy = query_cell_offset(a.q[3 * qi + 1], g.oy, g.inv_cell, cy);
            const double gz = query_cell_offset(a.q[3 * qi + 2], g.oz, g.inv_cell, cz);
            my_ring = ball_ring(g.nx, g.ny, g.nz, g.cell, cx, cy, cz, gx, gy, gz, my_r2);
        }
        int ring_item = my_ring;
        for (int o = 32; o > 0; o >>= 1) ring_item = max(ring_item, __shfl_xor(ring_item, o));
        ring_item = __builtin_amdgcn_readfirstlane(ring_item);
        ring_max = max(ring_max, ring_item);

        // ---- the cube of the item's largest ring, staged once where it fits
        bool staged = false;
        int mtot = 0;
        if (ring_item >= 1 && ring_item <= kBallStageRing) {
            const int zlo = max(-ring_item, -cz), zhi = min(ring_item, g.nz - 1 - cz);
            const int ylo = max(-ring_item, -cy), yhi = min(ring_item, g.ny - 1 - cy);
            const int wy = yhi - ylo + 1, nrows = (zhi - zlo + 1) * wy;              // <= 49
            int run_s = 0, run_len = 0;
            if (lane < nrows) {
                const int base = ((cz + zlo + lane / wy) * g.ny + (cy + ylo + lane % wy)) * g.nx;
                run_s = cs[base + max(cx - ring_item, 0)];
                run_len = cs[base + min(cx + ring_item, g.nx - 1) + 1] - run_s;
            }
            int incl = min(run_len, kBallCap + 1);     // (the sum of 49 capped runs cannot overflow; one run past the cap decides already)
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_up(incl, o);
                if (lane >= o) incl += v;
            }
            mtot = __builtin_amdgcn_readlane(incl, 63);
            if (mtot <= kBallCap) {                    // (then no run was capped: incl is the true prefix sum)
                staged = true;
                const int excl = incl - run_len;
                wave_lds_sync();                       // (the previous item's reads are done)
                for (int t = 0; t < nrows; ++t) {
                    const int s0 = __builtin_amdgcn_readlane(run_s, t), len = __builtin_amdgcn_readlane(run_len, t);
                    const int pre = __builtin_amdgcn_readlane(excl, t);
                    for (int b = lane; b < len; b += 64) stage[pre + b] = a.pts[s0 + b];      // pre + b < mtot <= kBallCap
                }
                wave_lds_sync();
            }
        }

        for (int j = 0; j < nq; ++j) {
            const int64_t qi = (int64_t)a.q_sorted[qs + j];
            const int ring = __builtin_amdgcn_readlane(my_ring, j);
            row.qx = a.q[3 * qi]; row.qy = a.q[3 * qi + 1]; row.qz = a.q[3 * qi + 2];
            row.r2 = __shfl(my_r2, j);
            row.cursor = FILL ? a.offsets[qi] : 0;
            row.end = FILL ? a.offsets[qi + 1] : 0;
            if (ring < 0) {
                // a NaN radius: nothing is a member
            } else if (staged) {
                for (int base = 0; base < mtot; base += 64) {
                    const int slot = base + lane;
                    const bool valid = slot < mtot;
                    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (valid) c = stage[slot];
                    row.consider(c, valid);
                }
            } else if (ball_streams(a.n, g.nx, g.ny, g.nz, cx, cy, cz, ring)) {
                row.stream(a.pts, a.n, lane);
            } else {
                ShellIter sh;
                sh.start(g, cy, cz, -1, ring);         // the whole cube, nothing pruned
                int nbase = 0, nlim = 0;
                bool have_next = sh.next(g, cs, cx, cy, cz, nbase, nlim);
                float4 c_next = make_float4(0.f, 0.f, 0.f, 0.f);
                if (have_next && nbase + lane < nlim) c_next = a.pts[nbase + lane];
                while (have_next) {
                    const bool valid = nbase + lane < nlim;
                    const float4 c = c_next;
                    have_next = sh.next(g, cs, cx, cy, cz, nbase, nlim);
                    if (have_next && nbase + lane < nlim) c_next = a.pts[nbase + lane];
                    row.consider(c, valid);
                }
            }
            if (!FILL && lane == 0) a.counts[qi] = row.cursor;
        }
        if (staged) n_staged += nq; else n_streamed += nq;
    }
    if (!FILL && lane == 0) {                          // once per wave
        if (n_staged) atomicAdd(&a.stat->staged, n_staged);
        if (n_streamed) atomicAdd(&a.stat->streamed, n_streamed);
        if (ring_max > 0) atomicMax(&a.stat->max_ring, ring_max);
    }
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void k_ball_count(BallArgs a) {
    __shared__ float4 s_stage[kWavesPerBlock][kBallCap];
    ball_items<false>(a, s_stage[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)]);
}
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_ball_fill(BallArgs a) {
    __shared__ float4 s_stage[kWavesPerBlock][kBallCap];
    ball_items<true>(a, s_stage[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)]);
}

// The exhaustive path: every query reads all n records (public order), one wave per query.
template <bool FILL>
__device__ __forceinline__ void ball_all(const BallArgs& a) {
    const int lane = lane_id();
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
    BallRow<FILL> row;
    row.idx = a.idx;
    row.dist = a.dist;
    for (int64_t qi = (int64_t)blockIdx.x * kWavesPerBlock + w; qi < a.m; qi += nwaves) {
        const double r = a.r[qi * a.r_stride];
        row.qx = a.q[3 * qi]; row.qy = a.q[3 * qi + 1]; row.qz = a.q[3 * qi + 2];
        row.r2 = r * r;
        row.cursor = FILL ? a.offsets[qi] : 0;
        row.end = FILL ? a.offsets[qi + 1] : 0;
        row.stream(a.pts, a.n, lane);
        if (!FILL && lane == 0) a.counts[qi] = row.cursor;
    }
}
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_ball_count_all(BallArgs a) { ball_all<false>(a); }
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_ball_fill_all(BallArgs a) { ball_all<true>(a); }

// Rows of 2 .. kBallSortCap entries, ascending public index (the entries of a row are distinct), one wave per row, in
// place.  Up to 64 entries: a bitonic network over the lanes.  Longer: the same network over LDS, padded to a power of two.
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_ball_sort(const int64_t* __restrict__ offsets, int64_t m, int* __restrict__ idx) {
    __shared__ int s_keys[kWavesPerBlock][kBallSortCap];
    const int lane = lane_id();
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int* __restrict__ s = s_keys[w];
    const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
    for (int64_t rowi = (int64_t)blockIdx.x * kWavesPerBlock + w; rowi < m; rowi += nwaves) {
        const int64_t b = offsets[rowi], len64 = offsets[rowi + 1] - b;
        if (len64 < 2 || len64 > kBallSortCap) continue;
        const int len = (int)len64;
        if (len <= 64) {
            int v = lane < len ? idx[b + lane] : INT_MAX;
            for (int k = 2; k <= 64; k <<= 1)
                for (int j = k >> 1; j > 0; j >>= 1) {
                    const int p = __shfl_xor(v, j);
                    const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
                    v = keep_min ? min(v, p) : max(v, p);
                }
            if (lane < len) idx[b + lane] = v;
            continue;
        }
        int P = 128;
        while (P < len) P <<= 1;                       // <= kBallSortCap, a power of two
        wave_lds_sync();                               // (the previous row's reads are done)
        for (int i = lane; i < P; i += 64) s[i] = i < len ? idx[b + i] : INT_MAX;
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                wave_lds_sync();
                for (int t = lane; t < P / 2; t += 64) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                    const int x = s[i], y = s[l];
                    if ((x > y) == ((i & k) == 0)) { s[i] = y; s[l] = x; }
                }
            }
        wave_lds_sync();
        for (int i = lane; i < len; i += 64) idx[b + i] = s[i];
    }
}
static_assert((kBallSortCap & (kBallSortCap - 1)) == 0 && kBallSortCap >= 128, "k_ball_sort pads a row to a power of two");

// distance of every entry from its row's query: one thread per entry, the row by bisection over the offsets
__global__ __launch_bounds__(256) void k_ball_dist(const float4* __restrict__ pub, const double* __restrict__ q, const int64_t* __restrict__ offsets,
                                                   int64_t m, const int* __restrict__ idx, int n, double* __restrict__ dist) {
    const int64_t total = offsets[m];
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        int64_t lo = 0, hi = m - 1;                    // the row: the smallest p with offsets[p + 1] > e
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (offsets[mid + 1] > e) hi = mid; else lo = mid + 1;
        }
        const unsigned p = (unsigned)idx[e];
        if (p >= (unsigned)n) { dist[e] = NAN; continue; }        // (an entry the fill never wrote: the tests would show it, no stray load)
        const float4 c = pub[p];
        const double dx = (double)c.x - q[3 * lo], dy = (double)c.y - q[3 * lo + 1], dz = (double)c.z - q[3 * lo + 2];
        dist[e] = sqrt((dx * dx + dy * dy) + dz * dz);
    }
}

struct RelOffset {              // int64 offsets of a chunk of rows as the 32-bit ones the library's segmented sort reads
    int64_t base;
    __host__ __device__ unsigned operator()(int64_t o) const { return (unsigned)(o - base); }
};

}  // namespace

// m >= 1 queries and their radii on the device.  grid: through the cell list in place, else the exhaustive path.
// h_offsets (m + 1) is complete on return whatever the status.  stat3 = {queries answered from a staged cube, queries
// streamed, largest ring} (zeros on the exhaustive path).
int pct_launch_ball(pct_ctx* ctx, bool grid, const double* d_q, int64_t m, const double* d_r, int r_stride, int32_t flags,
                    int64_t max_entries, int64_t* h_offsets, int64_t stat3[3]) {
    stat3[0] = stat3[1] = stat3[2] = 0;
    if (m > ((int64_t)1 << 30)) return pct_fail(ctx, PCT_ERR_INVALID, "pct_query_ball: %lld queries out of range", (long long)m);
    BallArgs a = {};
    a.n = (int)ctx->n;
    a.q = d_q;
    a.m = m;
    a.r = d_r;
    a.r_stride = r_stride;
    size_t scan_bytes = 0;
    int64_t* nul = nullptr;
    PCT_HIP(ctx, rocprim::exclusive_scan(nullptr, scan_bytes, nul, nul, (int64_t)0, (size_t)(m + 1), rocprim::plus<int64_t>(), ctx->stream));
    // extra scratch behind stage 1's (or alone): words | counts (m + 1) | scan scratch
    const size_t cnt_bytes = round256((size_t)(m + 1) * sizeof(int64_t));
    const size_t extra = 256 + cnt_bytes + round256(scan_bytes);
    char* x = nullptr;
    if (grid) {
        QueryItems st;
        PCT_TRY(pct_query_stage1(ctx, d_q, m, extra, &st));
        a.pts = (const float4*)ctx->sorted4.p;
        a.cell_start = (const int*)ctx->cell_cnt.p;
        a.g = ctx->grid;
        a.q_sorted = st.q_sorted;
        a.items = st.items;
        a.words = st.words;
        x = st.extra;
    } else {
        PCT_TRY(pct_ensure_plain_records(ctx));
        PCT_TRY(pct_reserve(ctx, &ctx->qry, extra));
        a.pts = (const float4*)ctx->qpts4.p;
        x = (char*)ctx->qry.p;
    }
    a.stat = (BallWords*)x;
    a.counts = (int64_t*)(x + 256);
    void* scan_tmp = x + 256 + cnt_bytes;
    PCT_TRY(pct_reserve(ctx, &ctx->ball_off, (size_t)(m + 1) * sizeof(int64_t)));
    int64_t* d_off = (int64_t*)ctx->ball_off.p;
    PCT_HIP(ctx, hipMemsetAsync(a.stat, 0, sizeof(BallWords), ctx->stream));
    PCT_HIP(ctx, hipMemsetAsync(a.counts + m, 0, sizeof(int64_t), ctx->stream));

    const dim3 block(64 * kWavesPerBlock), blocks(query_blocks(m));
    if (grid) PCT_LAUNCH(k_ball_count, blocks, block, 0, ctx->stream, a);
    else PCT_LAUNCH(k_ball_count_all, blocks, block, 0, ctx->stream, a);
    PCT_HIP(ctx, hipGetLastError());
    PCT_HIP(ctx, rocprim::exclusive_scan(scan_tmp, scan_bytes, a.counts, d_off, (int64_t)0, (size_t)(m + 1), rocprim::plus<int64_t>(), ctx->stream));
    PCT_HIP(ctx, hipMemcpyAsync(h_offsets, d_off, (size_t)(m + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    BallWords hw = {};
    PCT_HIP(ctx, hipMemcpyAsync(&hw, a.stat, sizeof(BallWords), hipMemcpyDeviceToHost, ctx->stream));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    stat3[0] = hw.staged; stat3[1] = hw.streamed; stat3[2] = hw.max_ring;
    const int64_t total = h_offsets[m];
    if (flags & PCT_BALL_COUNT_ONLY) return PCT_OK;
    if (max_entries > 0 && total > max_entries)
        return pct_fail(ctx, PCT_ERR_LIMIT, "pct_query_ball: %lld entries, the caller allows %lld (chunk the queries by the offsets returned)",
                        (long long)total, (long long)max_entries);

    // ---- fill.  (The row buffers are reserved last: nothing above moves or reads them.)
    const bool sorted = (flags & PCT_BALL_SORTED) != 0, want_dist = (flags & PCT_BALL_DISTANCES) != 0;
    PCT_TRY(pct_reserve(ctx, &ctx->ball_idx, (size_t)total * sizeof(int32_t)));
    if (want_dist) PCT_TRY(pct_reserve(ctx, &ctx->ball_dist, (size_t)total * sizeof(double)));
    if (total > 0) {
        a.offsets = d_off;
        a.idx = (int*)ctx->ball_idx.p;
        a.dist = want_dist && !sorted ? (double*)ctx->ball_dist.p : nullptr;
        if (grid) PCT_LAUNCH(k_ball_fill, blocks, block, 0, ctx->stream, a);
        else PCT_LAUNCH(k_ball_fill_all, blocks, block, 0, ctx->stream, a);
        PCT_HIP(ctx, hipGetLastError());
    }
    if (sorted && total > 0) {
        int64_t longest = 0;
        for (int64_t i = 0; i < m; ++i) longest = h_offsets[i + 1] - h_offsets[i] > longest ? h_offsets[i + 1] - h_offsets[i] : longest;
        if (longest <= kBallSortCap) {
            PCT_LAUNCH(k_ball_sort, blocks, block, 0, ctx->stream, (const int64_t*)d_off, m, (int*)ctx->ball_idx.p);
            PCT_HIP(ctx, hipGetLastError());
        } else {
            // the library's segmented sort, every row, into a second buffer that then becomes the rows'.  Its offsets
            // are 32-bit: rows are taken in chunks of fewer than 2^31 entries (one row always is: n < 2^31).
            PCT_TRY(pct_reserve(ctx, &ctx->ball_alt, (size_t)total * sizeof(int32_t)));
            int bits = 1;
            while (bits < 31 && ((int64_t)1 << bits) < ctx->n) ++bits;
            const int64_t chunk_max = ((int64_t)1 << 31) - 1;
            for (int64_t r0 = 0; r0 < m;) {
                int64_t r1 = r0 + 1;
                while (r1 < m && h_offsets[r1 + 1] - h_offsets[r0] <= chunk_max) ++r1;
                const int64_t base = h_offsets[r0], size = h_offsets[r1] - base;
                if (size > 0) {
                    const unsigned* in = (const unsigned*)ctx->ball_idx.p + base;
                    unsigned* out = (unsigned*)ctx->ball_alt.p + base;
                    auto begin = rocprim::make_transform_iterator((const int64_t*)d_off + r0, RelOffset{base});
                    auto end = rocprim::make_transform_iterator((const int64_t*)d_off + r0 + 1, RelOffset{base});
                    size_t tmp_bytes = 0;
                    PCT_HIP(ctx, rocprim::segmented_radix_sort_keys(nullptr, tmp_bytes, in, out, (unsigned)size, (unsigned)(r1 - r0), begin, end, 0, bits, ctx->stream));
                    pct_stage_scope stage(ctx);            // (every chunk's scratch in the same slot)
                    char* tmp = nullptr;
                    PCT_TRY(pct_claim(ctx, tmp_bytes, &tmp));
                    PCT_HIP(ctx, rocprim::segmented_radix_sort_keys(tmp, tmp_bytes, in, out, (unsigned)size, (unsigned)(r1 - r0), begin, end, 0, bits, ctx->stream));
                }
                r0 = r1;
            }
            ctx->ball_idx.swap(ctx->ball_alt);
        }
    }
    if (sorted && want_dist && total > 0) {
        PCT_TRY(pct_ensure_plain_records(ctx));
        const int64_t nb = (total + 255) / 256;
        PCT_LAUNCH(k_ball_dist, dim3((unsigned)(nb < 65536 ? nb : 65536)), dim3(256), 0, ctx->stream, (const float4*)ctx->qpts4.p, d_q,
                   (const int64_t*)d_off, m, (const int*)ctx->ball_idx.p, (int)ctx->n, (double*)ctx->ball_dist.p);
        PCT_HIP(ctx, hipGetLastError());
    }
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PCT_OK;
}

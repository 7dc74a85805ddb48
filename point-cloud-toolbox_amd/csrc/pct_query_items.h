// What every query of caller-supplied points through the uniform cell list shares (pct_query.hip: k nearest;
// pct_ball.hip: radius search), kept in this header so that no other translation unit's code depends on it:
//   stage 1       pct_query_stage1: the cell of every query (query_cell_coord, pct_query_plan.h), the query indices sorted
//                 by cell, work items {cell, first sorted query, <= kItemQ queries}.
//                 (The sort is the library's, as in pct_tree.hip, not a histogram over the cells: m is the small side,
//                 the grid may hold 2^27 cells, and no pass here is sized by the grid.)
//   query_item    a work item decoded: its cell, its queries, the cell's coordinates.
//   query_blocks  the launch geometry of the kernels that give one wave to one item (or one query).
// The LDS staging of the two files stays apart: k_query_cells stages nine runs nearest-first, so that tau tightens early,
// and rewrites .w to the sorted position; ball_items stages up to 49 rows in grid order and keeps the public index -- one
// routine for both would branch on its caller.  The prefetching cube walk (ShellIter's steps, each issued one step ahead
// of its use) is written out in k_query_exact and in ball_items as it is in k_knn_exact: a shared cursor over ShellIter was
// measured and cost k_query_exact 7 % of the whole call at n = m = 65 536 (tools/query_probe.py gain).
#pragma once

#include "pct_knn_sweep.h"
#include "pct_query_plan.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace {

constexpr int kItemQ = 16;                           // queries per work item (the cloud's own items: pct_build_grid)

struct QueryWords { int n_items, redo_count, max_ring, reserved; };      // device words of one call, cleared before it

__global__ __launch_bounds__(256) void k_query_cell_ids(const double* __restrict__ q, int64_t m, pct_grid g, unsigned* __restrict__ keys,
                                                        unsigned* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int cx = query_cell_coord(q[3 * i], g.ox, g.inv_cell, g.nx);
    const int cy = query_cell_coord(q[3 * i + 1], g.oy, g.inv_cell, g.ny);
    const int cz = query_cell_coord(q[3 * i + 2], g.oz, g.inv_cell, g.nz);
    keys[i] = (unsigned)((cz * g.ny + cy) * g.nx + cx);       // < ncell <= 2^30 (pct_build_grid's cell budget)
    vals[i] = (unsigned)i;
}

// One thread per sorted query: the thread at offset 0, kItemQ, 2 kItemQ ... of its cell's run appends an item.  (Both
// bounds of the run by binary search over the sorted keys: ~20 cached loads, m is the small side of the problem.)
__global__ __launch_bounds__(256) void k_query_items(const unsigned* __restrict__ keys, int64_t m, int4* __restrict__ items,
                                                     QueryWords* __restrict__ words) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool head = false;
    unsigned key = 0;
    int nq = 0;
    if (i < m) {
        key = keys[i];
        int64_t lo = 0, hi = i;                       // first position of the run: the smallest p with keys[p] >= key
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (keys[mid] < key) lo = mid + 1; else hi = mid;
        }
        head = ((i - lo) % kItemQ) == 0;
        if (head) {
            int64_t a = i, b = m;                     // end of the run: the smallest p > i with keys[p] > key
            while (a < b) {
                const int64_t mid = (a + b) >> 1;
                if (keys[mid] <= key) a = mid + 1; else b = mid;
            }
            nq = (int)(a - i < kItemQ ? a - i : kItemQ);
        }
    }
    const unsigned long long mask = __ballot(head);
    int base = 0;
    if ((threadIdx.x & 63) == 0 && mask) base = atomicAdd(&words->n_items, __popcll(mask));
    base = __shfl(base, 0);
    if (head) {
        const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
        items[base + rank] = make_int4((int)key, (int)i, nq, 0);         // at most m items: one per query
    }
}

struct QueryItem { int cell, qs, nq, cx, cy, cz; };   // wave-uniform: the cell, the first position in q_sorted, the queries

__device__ __forceinline__ QueryItem query_item(const int4* __restrict__ items, int item, const pct_grid& g) {
    const int4 it = items[item];
    QueryItem qi;
    qi.cell = __builtin_amdgcn_readfirstlane(it.x);
    qi.qs = __builtin_amdgcn_readfirstlane(it.y);
    qi.nq = __builtin_amdgcn_readfirstlane(it.z);
    qi.cx = qi.cell % g.nx; qi.cy = (qi.cell / g.nx) % g.ny; qi.cz = qi.cell / (g.nx * g.ny);
    return qi;
}

// one wave per item, kWavesPerBlock of them per block; the kernels stride over what the grid does not cover
unsigned query_blocks(int64_t m, int64_t most = 16384) {
    const int64_t want = (m + kWavesPerBlock - 1) / kWavesPerBlock;
    return (unsigned)(want < most ? want : most);
}

size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

// What stage 1 leaves in ctx->qry for the kernels of its caller; `extra` = the first byte behind it, 256-aligned, of the
// extra_bytes the caller asked for.
struct QueryItems {
    QueryWords* words;
    const unsigned* q_sorted;   // query indices in cell order
    const int4* items;          // {cell, first position in q_sorted, queries, 0}; words->n_items of them
    char* extra;
};

// m >= 1 queries (device array d_q) filed in the cell list in place.  One allocation:
// words | keys | sorted keys | query indices | sorted query indices | items | extra | sort scratch
int pct_query_stage1(pct_ctx* ctx, const double* d_q, int64_t m, size_t extra_bytes, QueryItems* out) {
    const pct_grid& g = ctx->grid;
    if (g.ncell > ((int64_t)1 << 31) - 1 || m > ((int64_t)1 << 30))
        return pct_fail(ctx, PCT_ERR_INVALID, "query through the cell list: %lld cells / %lld queries out of range", (long long)g.ncell, (long long)m);
    int bits = 1;
    while (bits < 31 && ((int64_t)1 << bits) < g.ncell) ++bits;
    unsigned* nul = nullptr;
    size_t tmp_bytes = 0;
    PCT_HIP(ctx, rocprim::radix_sort_pairs(nullptr, tmp_bytes, nul, nul, nul, nul, (size_t)m, 0, bits, ctx->stream));
    const size_t um = round256((size_t)m * sizeof(unsigned));
    const size_t off_keys = 256, off_keys2 = off_keys + um, off_vals = off_keys2 + um, off_vals2 = off_vals + um;
    const size_t off_items = off_vals2 + um, off_extra = off_items + round256((size_t)m * sizeof(int4));
    const size_t off_tmp = off_extra + round256(extra_bytes);
    PCT_TRY(pct_reserve(ctx, &ctx->qry, off_tmp + round256(tmp_bytes) + 256));
    char* base = (char*)ctx->qry.p;
    QueryWords* words = (QueryWords*)base;
    unsigned *keys = (unsigned*)(base + off_keys), *keys2 = (unsigned*)(base + off_keys2);
    unsigned *vals = (unsigned*)(base + off_vals), *vals2 = (unsigned*)(base + off_vals2);
    PCT_HIP(ctx, hipMemsetAsync(words, 0, sizeof(QueryWords), ctx->stream));
    const unsigned nb = (unsigned)((m + 255) / 256);
    PCT_LAUNCH(k_query_cell_ids, dim3(nb), dim3(256), 0, ctx->stream, d_q, m, g, keys, vals);
    PCT_HIP(ctx, hipGetLastError());
    PCT_HIP(ctx, rocprim::radix_sort_pairs(base + off_tmp, tmp_bytes, keys, keys2, vals, vals2, (size_t)m, 0, bits, ctx->stream));
    PCT_LAUNCH(k_query_items, dim3(nb), dim3(256), 0, ctx->stream, (const unsigned*)keys2, m, (int4*)(base + off_items), words);
    PCT_HIP(ctx, hipGetLastError());
    out->words = words;
    out->q_sorted = vals2;
    out->items = (const int4*)(base + off_items);
    out->extra = base + off_extra;
    return PCT_OK;
}

}  // namespace

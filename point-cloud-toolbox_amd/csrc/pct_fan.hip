// Faces from the tangent-plane Voronoi cells: the cell pct_area.hip cuts for every row, with a label on every edge, gives the
// row's natural (Delaunay) neighbours in counter-clockwise order; two consecutive ones around a vertex of the cell propose
// a triangle, and the triangles that all three of their corners propose are the faces (include/pct_hip_surface.h has the
// contract; tests/fan_exact.py states it again in NumPy).
//
// k_fan / k_fan_wide: k_area / k_area_wide with the labels -- area_row<.., LAB = true>, the same block, the same rotation,
// the same cuts in the same order; the labels (int16, [vertex][lane] beside x and y) cost 2 KiB of LDS per wave on top of
// the 16 KiB.  What a row leaves is its fan, one int32 code per vertex of the cell, in polygon order:
//   -1              the edge leaving the vertex lies on the square
//   p >= 0          ... on the bisector of the cloud record of public index p, and the vertex lies inside the disc
//   -2 - p          ... the same, the vertex on or outside the disc x^2 + y^2 < L^2
// Vertex v is a proper corner when the edge arriving (the code of v - 1, cyclic) and the edge leaving both carry a record and v
// lies inside; the corner is the pair (arriving record, leaving record).  Everything is stored by PUBLIC index -- fans at a
// pitch of kAreaCap for the rows k_fan finishes, at k + 4 in a second buffer (by position on the overflow list) for those
// k_fan_wide finishes; the head {vertices, slot or -1} tells where -- so nothing here reads the table or row_of afterwards.
// k_tri_count: one thread per public row: for the corners whose lowest public index the row is, do both other rows propose
// the triangle too?  Then it is marked in all three rows' 64-bit masks (an OR: the masks do not depend on who comes first)
// and counted for the row.  rocprim::exclusive_scan.  k_tri_fill: writes the row's triangles wound about its normal, sorted
// among themselves, and counts the edges with one face from the row's own mask.  No atomics on the output: the same bytes
// for the same state.
#include "pct_fan_row.h"

#include <rocprim/device/device_scan.hpp>

namespace {

enum FanWord { FW_OVERFLOW = 0, FW_ROWS_CORNER, FW_CORNERS, FW_MAX_FAN, FW_BOUNDARY, FW_COUNT };   // unsigned long long words

struct FanOut {
    int2* head;                     // (n) by public index: {vertices of the cell (0: a NaN row), slot in `wide` or -1}
    int* fast;                      // (n, kAreaCap) by public index
    int* wide;                      // (overflow rows, k + 4) by position on the overflow list
    unsigned char* side;            // (n) by public index: the flipped bit of the resident frames as this call found it
    const unsigned char* flipped;   // the resident frames' bits (null: none asked for), by table row or by public index
    int flipped_by_row;
    unsigned long long* words;      // eight words, zeroed per call: FanWord
    int* over_list;                 // rows k_fan hands to k_fan_wide
};

// the fan of a finished row: the polygon's labels as cloud records, the disc test per vertex
template <int STRIDE>
__device__ __forceinline__ void store_fan(const FitArgs& a, int64_t row, const Poly<STRIDE, true>& P, int n, double L2, int* __restrict__ dst) {
    const TableRows rows;
    const int* my = rows.start(a, row);
    for (int v = 0; v < n; ++v) {
        const int lab = P.Lab(v);
        int code = -1;
        if (lab >= 0) {
            const int pub = __float_as_int(a.pts[my[lab]].w);       // (a finished row holds no entry outside the cloud)
            const double x = P.X(v), y = P.Y(v);
            code = x * x + y * y < L2 ? pub : -2 - pub;
        }
        dst[v] = code;
    }
}

template <bool F64>
__global__ __launch_bounds__(kAreaBlock) void k_fan(FitArgs a, FanOut o) {
    __shared__ double s_x[kAreaCap][kAreaBlock], s_y[kAreaCap][kAreaBlock];
    __shared__ short s_l[kAreaCap][kAreaBlock];
    const int lane = threadIdx.x;
    const int64_t row0 = (a.blocks_per_xcd ? (int64_t)(blockIdx.x & 7u) * a.blocks_per_xcd + (blockIdx.x >> 3) : (int64_t)blockIdx.x) * kAreaBlock;
    if (row0 >= a.rows) return;
    const int64_t row = row0 + lane;
    int status = AREA_SKIP;
    if (row < a.rows) {
        const TableRows rows;
        const int64_t qid = rows.query(a, row);
        const float4 qp = a.pts[qid];
        const int64_t pub = __float_as_int(qp.w);
        const Poly<kAreaBlock, true> P = {&s_x[0][lane], &s_y[0][lane], kAreaCap, &s_l[0][lane]};
        double area, L2 = 0;
        int nverts, closed;
        unsigned survivors;
        status = area_row<F64>(a, row, qid, qp, P, area, nverts, closed, survivors, &L2);
        o.side[pub] = o.flipped ? o.flipped[o.flipped_by_row ? row : pub] : (unsigned char)0;
        if (status == AREA_DONE) {
            store_fan(a, row, P, nverts, L2, o.fast + pub * kAreaCap);
            o.head[pub] = make_int2(nverts, -1);
        } else if (status == AREA_NAN) {
            o.head[pub] = make_int2(0, -1);
        }
    }
    const unsigned long long om = __ballot(status == AREA_OVERFLOW);          // one increment of the list cursor per wave
    if (om) {
        const int leader = (int)__builtin_ctzll(om);
        unsigned long long base = 0;
        if (lane == leader) base = atomicAdd(&o.words[FW_OVERFLOW], (unsigned long long)__popcll(om));
        base = __shfl(base, leader);
        if (status == AREA_OVERFLOW) o.over_list[base + __popcll(om & ((1ull << lane) - 1ull))] = (int)row;
    }
}

// The rows k_fan could not hold: one wave per listed row, lane 0 walks it, room for k + 4 vertices (x | y | labels).
template <bool F64>
__global__ __launch_bounds__(kAreaBlock) void k_fan_wide(FitArgs a, FanOut o) {
    extern __shared__ double s_poly[];
    if (threadIdx.x != 0) return;
    const int64_t total = (int64_t)o.words[FW_OVERFLOW];
    const int cap = a.k + 4;
    const TableRows rows;
    for (int64_t it = blockIdx.x; it < total; it += gridDim.x) {
        const int64_t row = o.over_list[it];
        const int64_t qid = rows.query(a, row);
        const float4 qp = a.pts[qid];
        const int64_t pub = __float_as_int(qp.w);
        const Poly<1, true> P = {s_poly, s_poly + cap, cap, (short*)(s_poly + 2 * cap)};
        double area, L2 = 0;
        int nverts, closed;
        unsigned survivors;
        const int status = area_row<F64>(a, row, qid, qp, P, area, nverts, closed, survivors, &L2);
        if (status == AREA_DONE) {
            store_fan(a, row, P, nverts, L2, o.wide + it * cap);
            o.head[pub] = make_int2(nverts, (int)it);
        } else {
            o.head[pub] = make_int2(0, -1);
        }
    }
}

// ---- agreement and emission: one thread per public row --------------------------------------------------------------
struct TriArgs {
    const int2* head;
    const int* fast;
    const int* wide;
    int wpitch;
    const unsigned char* side;      // null: wound about the fit's own side
    int64_t n;
    unsigned long long* mask;       // (n): corner v < 64 of the row is agreed (zeroed before k_tri_count)
    int64_t* count;                 // (n + 1): triangles the row emits
    const int64_t* off;             // (n + 1): their exclusive scan
    int* tri;                       // (triangles, 3)
    unsigned long long* words;      // FanWord
    unsigned long long* part;       // (blocks, 4): every block's {rows with a corner, corners, largest fan, edges with one face}
};

// (a block's share of one statistic goes into its slot of TriArgs::part through block_partial, pct_fan_row.h: k_tri_stats
// adds the slots up)
__global__ __launch_bounds__(256) void k_tri_stats(const unsigned long long* __restrict__ part, int blocks, unsigned long long* __restrict__ words) {
    __shared__ unsigned long long sh[4][256];
    unsigned long long v[4] = {0, 0, 0, 0};
    for (int b = threadIdx.x; b < blocks; b += 256)
        for (int q = 0; q < 4; ++q) {
            const unsigned long long x = part[(int64_t)b * 4 + q];
            v[q] = q == 2 ? (x > v[q] ? x : v[q]) : v[q] + x;
        }
    for (int q = 0; q < 4; ++q) sh[q][threadIdx.x] = v[q];
    __syncthreads();
    if (threadIdx.x < 4) {
        const int q = threadIdx.x;
        unsigned long long r = 0;
        for (int i = 0; i < 256; ++i) r = q == 2 ? (sh[q][i] > r ? sh[q][i] : r) : r + sh[q][i];
        words[q == 0 ? FW_ROWS_CORNER : q == 1 ? FW_CORNERS : q == 2 ? FW_MAX_FAN : FW_BOUNDARY] = r;
    }
}

// vertex v of the fan: a proper corner of two different records?
__device__ __forceinline__ bool fan_corner(const int* __restrict__ codes, int n, int v, int& a, int& b) {
    const int cv = codes[v];
    a = code_record(codes[v == 0 ? n - 1 : v - 1]);
    b = code_record(cv);
    return a >= 0 && cv >= 0 && a != b;
}
// Another row's fan for a look-up: its head and, at the same time, the kAreaCap codes of its slot in the fast buffer (the
// slot exists for every row; what lies behind the row's vertices, or in the slot of a wide row, is never looked at) -- one
// memory latency per look-up instead of one per vertex.
struct FanRow {
    int2 head;
    int c[kAreaCap];
};
__device__ __forceinline__ void load_fan_row(const TriArgs& t, int x, FanRow& r) {
    r.head = t.head[x];
    const int* p = t.fast + (int64_t)x * kAreaCap;
    if constexpr (kAreaCap % 4 == 0) {
#pragma unroll
        for (int q = 0; q < kAreaCap / 4; ++q) {
            const int4 w = ((const int4*)p)[q];
            r.c[4 * q] = w.x; r.c[4 * q + 1] = w.y; r.c[4 * q + 2] = w.z; r.c[4 * q + 3] = w.w;
        }
    } else {
#pragma unroll
        for (int v = 0; v < kAreaCap; ++v) r.c[v] = p[v];
    }
}
// the vertex of the loaded row x whose corner has the unordered pair {p, q}; -1: none
__device__ __forceinline__ int row_proposes(const TriArgs& t, int x, const FanRow& r, int p, int q) {
    const int n = r.head.x;
    if (r.head.y >= 0) {                          // a wide row: from its own buffer, vertex by vertex
        const int* codes = t.wide + (int64_t)r.head.y * t.wpitch;
        for (int v = 0; v < n; ++v) {
            int a, b;
            if (fan_corner(codes, n, v, a, b) && ((a == p && b == q) || (a == q && b == p))) return v;
        }
        return -1;
    }
    int prev = r.c[0];                            // the code of vertex n - 1
#pragma unroll
    for (int v = 1; v < kAreaCap; ++v) prev = v == n - 1 ? r.c[v] : prev;
    int found = -1;
#pragma unroll
    for (int v = 0; v < kAreaCap; ++v) {
        const int cv = r.c[v];
        const int a = code_record(prev), b = code_record(cv);
        if (v < n && found < 0 && a >= 0 && cv >= 0 && a != b && ((a == p && b == q) || (a == q && b == p))) found = v;
        prev = cv;
    }
    return found;
}
// the corner (a, b) of row i: the vertices of rows a and b that propose the triangle too (both loaded before either is read)
__device__ __forceinline__ bool corner_agreed(const TriArgs& t, int i, int a, int b, int& va, int& vb) {
    FanRow ra, rb;
    load_fan_row(t, a, ra);
    load_fan_row(t, b, rb);
    va = row_proposes(t, a, ra, b, i);
    vb = row_proposes(t, b, rb, i, a);
    return va >= 0 && vb >= 0;
}
__device__ __forceinline__ bool corner_agreed(const TriArgs& t, int i, int a, int b) {
    int va, vb;
    return corner_agreed(t, i, a, b, va, vb);
}
// corner v of row r is agreed: an OR into the row's mask, whichever of the triangle's rows finds it (the mask is complete
// when the kernel is; rows of more than 64 vertices -- wide rows only -- are asked again where they are read)
__device__ __forceinline__ void mark_agreed(const TriArgs& t, int r, int v) {
    if (v < 64) atomicOr(&t.mask[r], 1ull << v);
}

// Agreement, decided once per triangle: by the row of lowest public index among its three, which looks the pair up in the
// two others and marks the corner in all three masks (zeroed before the launch).  count: the triangles the row emits.
__global__ __launch_bounds__(256) void k_tri_count(TriArgs t) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long corners = 0, fan = 0;
    if (i < t.n) {
        int n;
        const int* codes = fan_codes(t.head, t.fast, t.wide, t.wpitch, i, n);
        int64_t emit = 0;
        for (int v = 0; v < n; ++v) {
            int a, b;
            fan += codes[v] != -1 ? 1 : 0;
            if (!fan_corner(codes, n, v, a, b)) continue;
            ++corners;
            if (!(i < a && i < b)) continue;
            int va, vb;
            if (!corner_agreed(t, (int)i, a, b, va, vb)) continue;
            ++emit;
            mark_agreed(t, (int)i, v);
            mark_agreed(t, a, va);
            mark_agreed(t, b, vb);
        }
        t.count[i] = emit;
    }
    unsigned long long* part = t.part + (int64_t)blockIdx.x * 4;
    block_partial(corners > 0 ? 1ull : 0ull, false, part);
    block_partial(corners, false, part + 1);
    block_partial(fan, true, part + 2);
}

// Emission, and the edges with one face: every face on an edge (i, x) is an agreed corner of row i that holds x, so row i
// counts its edges to higher indices from its own fan and mask alone.
__global__ __launch_bounds__(256) void k_tri_fill(TriArgs t) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long boundary = 0;
    if (i < t.n) {
        int n;
        const int* codes = fan_codes(t.head, t.fast, t.wide, t.wpitch, i, n);
        const unsigned long long m = t.mask[i];
        const auto agreed = [&](int v, int a, int b) { return v < 64 ? (m >> v & 1ull) != 0 : corner_agreed(t, (int)i, a, b); };
        const int64_t base = t.off[i], cnt = t.off[i + 1] - base;
        const bool turned = t.side && t.side[i];
        int* out = t.tri + base * 3;
        int64_t at = 0;
        for (int v = 0; v < n && (m != 0 || n > 64); ++v) {
            int a, b;
            if (!fan_corner(codes, n, v, a, b) || !agreed(v, a, b)) continue;
            for (int s = 0; s < 2; ++s) {
                const int x = s ? b : a;
                if (x < i) continue;
                int faces = 0;
                for (int w = 0; w < n; ++w) {
                    int c, d;
                    if (fan_corner(codes, n, w, c, d) && (c == x || d == x) && agreed(w, c, d)) ++faces;
                }
                if (faces == 1) ++boundary;
            }
            if (!(i < a && i < b) || at >= cnt) continue;
            // (i, a, b) is counter-clockwise about +z of the row's rotation; insertion by (v1, v2) among the row's own
            const int v1 = turned ? b : a, v2 = turned ? a : b;
            int64_t j = at++;
            for (; j > 0 && (out[(j - 1) * 3 + 1] > v1 || (out[(j - 1) * 3 + 1] == v1 && out[(j - 1) * 3 + 2] > v2)); --j) {
                out[j * 3 + 1] = out[(j - 1) * 3 + 1];
                out[j * 3 + 2] = out[(j - 1) * 3 + 2];
            }
            out[j * 3 + 1] = v1;
            out[j * 3 + 2] = v2;
        }
        for (int64_t j = 0; j < cnt; ++j) out[j * 3] = (int)i;
    }
    block_partial(boundary, false, t.part + (int64_t)blockIdx.x * 4 + 3);
}

// ---- the natural neighbours of public rows [first, first + rows) as CSR ---------------------------------------------------
__global__ __launch_bounds__(256) void k_fan_sizes(const int2* __restrict__ head, const int* __restrict__ fast, const int* __restrict__ wide,
                                                   int wpitch, int64_t first, int64_t rows, int64_t* __restrict__ count) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > rows) return;
    int64_t c = 0;
    if (r < rows) {
        int n;
        const int* codes = fan_codes(head, fast, wide, wpitch, first + r, n);
        for (int v = 0; v < n; ++v) c += codes[v] != -1 ? 1 : 0;
    }
    count[r] = c;                   // (count[rows] = 0: the scan's last entry is the total)
}

__global__ __launch_bounds__(256) void k_fan_entries(const int2* __restrict__ head, const int* __restrict__ fast, const int* __restrict__ wide,
                                                     int wpitch, int64_t first, int64_t rows, const int64_t* __restrict__ off,
                                                     int* __restrict__ nbr) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    int n;
    const int* codes = fan_codes(head, fast, wide, wpitch, first + r, n);
    int64_t at = off[r];
    for (int v = 0; v < n; ++v)
        if (codes[v] != -1) nbr[at++] = code_record(codes[v]);
}

int scan_counts(pct_ctx* ctx, const int64_t* d_count, int64_t* d_off, int64_t entries) {
    size_t bytes = 0;
    int64_t* nul = nullptr;
    PCT_HIP(ctx, rocprim::exclusive_scan(nullptr, bytes, nul, nul, (int64_t)0, (size_t)entries, rocprim::plus<int64_t>(), ctx->stream));
    PCT_TRY(pct_reserve(ctx, &ctx->tri_tmp, bytes > 0 ? bytes : 1));
    PCT_HIP(ctx, rocprim::exclusive_scan(ctx->tri_tmp.p, bytes, d_count, d_off, (int64_t)0, (size_t)entries, rocprim::plus<int64_t>(), ctx->stream));
    return PCT_OK;
}

}  // namespace

// Fans, corners and triangles of the resident table of a whole-cloud handle.  mid (an event): recorded between the fan
// kernels and the agreement.  On return the stream has been waited for twice (the overflow count sizes the wide buffer,
// the triangle count the output) and the statistics words are on their way to ctx->pin->tri_words.
int pct_launch_point_triangles(pct_ctx* ctx, bool wind_frames, hipEvent_t mid) {
    const int64_t n = ctx->n;
    const bool sorted = ctx->knn_sorted_space;
    FitArgs a = {};
    PCT_TRY(fit_source(ctx, sorted ? FitSpace::Sorted : FitSpace::Packed, &a));
    a.table = (const int*)ctx->nbr_pos.p;
    a.cnt = ctx->eps > 0 ? (const int*)ctx->nbr_cnt.p : nullptr;
    a.row_query32 = sorted ? (const int*)ctx->owned_pos.p : nullptr;
    a.row_offset = 0;
    a.rows = n;
    a.k = ctx->k;
    a.pitch = ctx->nbr_pitch;
    a.force_jacobi = fit_jacobi_forced();
    PCT_TRY(pct_reserve(ctx, &ctx->fan_head, (size_t)n * sizeof(int2)));
    PCT_TRY(pct_reserve(ctx, &ctx->fan_fast, (size_t)n * kAreaCap * sizeof(int)));
    PCT_TRY(pct_reserve(ctx, &ctx->fan_side, (size_t)n));
    PCT_TRY(pct_reserve(ctx, &ctx->fan_over, 64 + (size_t)n * sizeof(int)));
    FanOut o = {};
    o.head = (int2*)ctx->fan_head.p;
    o.fast = (int*)ctx->fan_fast.p;
    o.side = (unsigned char*)ctx->fan_side.p;
    o.flipped = wind_frames ? (const unsigned char*)ctx->frame_flip.p + 64 : nullptr;
    o.flipped_by_row = ctx->res.in_row_order(PCT_R_FRAMES) ? 1 : 0;
    o.words = (unsigned long long*)ctx->fan_over.p;
    o.over_list = (int*)ctx->fan_over.p + 16;
    PCT_HIP(ctx, hipMemsetAsync(ctx->fan_over.p, 0, 64, ctx->stream));
    int blocks = (int)((n + kAreaBlock - 1) / kAreaBlock);
    a.blocks_per_xcd = pct_getenv("PCT_NO_XCD_MAP") ? 0 : (blocks + 7) / 8;
    if (a.blocks_per_xcd) blocks = a.blocks_per_xcd * 8;
    if (ctx->has_f64) PCT_LAUNCH(k_fan<true>, dim3(blocks), dim3(kAreaBlock), 0, ctx->stream, a, o);
    else PCT_LAUNCH(k_fan<false>, dim3(blocks), dim3(kAreaBlock), 0, ctx->stream, a, o);
    PCT_HIP(ctx, hipGetLastError());
    PCT_HIP(ctx, hipMemcpyAsync(ctx->pin->tri_words, ctx->fan_over.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int64_t over = (int64_t)ctx->pin->tri_words[FW_OVERFLOW];
    const int wpitch = a.k + 4;
    PCT_TRY(pct_reserve(ctx, &ctx->fan_wide, (size_t)(over > 0 ? over : 1) * wpitch * sizeof(int)));
    o.wide = (int*)ctx->fan_wide.p;
    if (over > 0) {
        const int wblocks = (int)(over < 1024 ? over : 1024);
        const size_t wlds = (size_t)wpitch * (2 * sizeof(double) + sizeof(short));
        if (ctx->has_f64) PCT_LAUNCH(k_fan_wide<true>, dim3(wblocks), dim3(kAreaBlock), wlds, ctx->stream, a, o);
        else PCT_LAUNCH(k_fan_wide<false>, dim3(wblocks), dim3(kAreaBlock), wlds, ctx->stream, a, o);
        PCT_HIP(ctx, hipGetLastError());
    }
    PCT_HIP(ctx, hipEventRecord(mid, ctx->stream));

    PCT_TRY(pct_reserve(ctx, &ctx->tri_mask, (size_t)n * sizeof(unsigned long long)));
    PCT_TRY(pct_reserve(ctx, &ctx->tri_count, (size_t)(n + 1) * sizeof(int64_t)));
    PCT_TRY(pct_reserve(ctx, &ctx->tri_off, (size_t)(n + 1) * sizeof(int64_t)));
    TriArgs t = {};
    t.head = o.head;
    t.fast = o.fast;
    t.wide = o.wide;
    t.wpitch = wpitch;
    t.side = wind_frames ? o.side : nullptr;
    t.n = n;
    t.mask = (unsigned long long*)ctx->tri_mask.p;
    t.count = (int64_t*)ctx->tri_count.p;
    t.off = (const int64_t*)ctx->tri_off.p;
    t.words = o.words;
    const dim3 tblocks((unsigned)((n + 255) / 256));
    PCT_TRY(pct_reserve(ctx, &ctx->tri_part, (size_t)tblocks.x * 4 * sizeof(unsigned long long)));
    t.part = (unsigned long long*)ctx->tri_part.p;
    PCT_HIP(ctx, hipMemsetAsync(t.part, 0, (size_t)tblocks.x * 4 * sizeof(unsigned long long), ctx->stream));
    PCT_HIP(ctx, hipMemsetAsync(t.count + n, 0, sizeof(int64_t), ctx->stream));
    PCT_HIP(ctx, hipMemsetAsync(t.mask, 0, (size_t)n * sizeof(unsigned long long), ctx->stream));
    PCT_LAUNCH(k_tri_count, tblocks, dim3(256), 0, ctx->stream, t);
    PCT_HIP(ctx, hipGetLastError());
    PCT_TRY(scan_counts(ctx, t.count, (int64_t*)ctx->tri_off.p, n + 1));
    PCT_HIP(ctx, hipMemcpyAsync(&ctx->pin->tri_words[7], t.off + n, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int64_t total = (int64_t)ctx->pin->tri_words[7];
    if (total > (int64_t)INT32_MAX) return pct_fail(ctx, PCT_ERR_INVALID, "pct_point_triangles: %lld triangles out of range", (long long)total);
    PCT_TRY(pct_reserve(ctx, &ctx->tri, (size_t)(total > 0 ? total : 1) * 3 * sizeof(int)));
    t.tri = (int*)ctx->tri.p;
    if (total > 0) {
        PCT_LAUNCH(k_tri_fill, tblocks, dim3(256), 0, ctx->stream, t);
        PCT_HIP(ctx, hipGetLastError());
    }
    PCT_LAUNCH(k_tri_stats, dim3(1), dim3(256), 0, ctx->stream, (const unsigned long long*)t.part, (int)tblocks.x, t.words);
    PCT_HIP(ctx, hipGetLastError());
    PCT_HIP(ctx, hipMemcpyAsync(ctx->pin->tri_words, ctx->fan_over.p, FW_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    ctx->tri_wpitch = wpitch;
    return PCT_OK;
}

// rows, rows with a corner, corners, triangles, rows redone wide, largest fan, boundary edges; the triangle count stays on
// the handle for the getters and the hole filling
void pct_fan_report(pct_ctx* ctx, pct_stage_report* rep) {
    const unsigned long long* w = ctx->pin->tri_words;
    ctx->tri_total = (int64_t)w[7];
    const int64_t st[8] = {ctx->n, (int64_t)w[FW_ROWS_CORNER], (int64_t)w[FW_CORNERS], ctx->tri_total, (int64_t)w[FW_OVERFLOW],
                           (int64_t)w[FW_MAX_FAN], (int64_t)w[FW_BOUNDARY], 0};
    for (int i = 0; i < 8; ++i) rep->stats[i] = st[i];
}

// Natural neighbours of public rows [first, first + rows): d_off (rows + 1) always, d_nbr (may be null) the entries
int pct_launch_point_fans(pct_ctx* ctx, int64_t first, int64_t rows, int64_t* d_count, int64_t* d_off, int* d_nbr) {
    const int2* head = (const int2*)ctx->fan_head.p;
    const int *fast = (const int*)ctx->fan_fast.p, *wide = (const int*)ctx->fan_wide.p;
    PCT_LAUNCH(k_fan_sizes, dim3((unsigned)((rows + 256) / 256)), dim3(256), 0, ctx->stream, head, fast, wide, ctx->tri_wpitch, first, rows, d_count);
    PCT_HIP(ctx, hipGetLastError());
    PCT_TRY(scan_counts(ctx, d_count, d_off, rows + 1));
    if (d_nbr && rows > 0) {
        PCT_LAUNCH(k_fan_entries, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, ctx->stream, head, fast, wide, ctx->tri_wpitch, first, rows,
                   (const int64_t*)d_off, d_nbr);
        PCT_HIP(ctx, hipGetLastError());
    }
    return PCT_OK;
}

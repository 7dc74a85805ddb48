// Watertight faces: the boundary loops of the resident triangles and the filling of the small ones (include/pct_hip_holes.h
// has the definition; tests/hole_exact.py states it again in NumPy).  Everything is read from what pct_fan.hip keeps by
// public index: the fans (head, codes), the agreed-corner masks, the triangles and their per-row offsets.
//
// What the definition asks of the triangles is answered from a row's own data:
//   resident?     {a, b, c} is emitted by its lowest row: a look at that row's few triangles (tri_off, tri);
//   faces(v, x)   every triangle on the edge (v, x) is a corner of row v, and a corner's pair is two neighbours in the fan:
//                 the faces on the edge to F[t] are sector t - 1 and sector t (one face where both are the same triangle, a fan
//                 of two);
//   faces(x, y)   > 0 for a diagonal: y is in the fan of x and one of the two sectors beside it is filled.
// k_hole_gaps   one thread per public row, run twice (count | rocprim scan | fill): a row whose corners are all agreed -- its
//               mask alone says so -- is closed, has no gap and is not read further; the other rows' sectors, face counts
//               and gaps.  Boundary edges and odd gaps through per-block partial sums (k_hole_words adds them up).
// k_hole_walk   one thread per gap: the walk, a for loop bounded by max_vertices, writing its vertices to the gap's slot;
//               it stops at a vertex below v0 (whatever becomes of that walk, it does not own a loop).
// k_hole_fill   one wave per gap, gone at once where the walk owns no loop: vertices and float64 coordinates in LDS, the
//               perimeter, the taken diagonals (lanes over the pairs), the dynamic programme span by span (one state per
//               lane, W and the splits in LDS), the back-trace by lane 0 into the slot's triangles.
// rocprim scan over the slots' {loops, vertices, triangles, filled, perimeter, blocked}; k_hole_pack: loops and patches to
// their places; rocprim::merge_sort of the patches; rocprim::merge with the triangles.  No atomics on any output.
#include "pct_fan_row.h"

#include <rocprim/device/device_merge.hpp>
#include <rocprim/device/device_merge_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace {

constexpr int kHoleMax = PCT_HOLE_MAX_VERTICES;
constexpr int kHoleTris = kHoleMax - 2;
static_assert(kHoleMax <= 32, "k_hole_fill: one state of a span per lane, 32 x 32 tables");

enum HoleStatus { HS_FILLED = 0, HS_PERIMETER = 1, HS_BLOCKED = 2 };

struct HoleView {                   // the resident fans and triangles, by public index
    const int2* head;
    const int* fast;
    const int* wide;
    int wpitch;
    const unsigned long long* mask; // (n): agreed corners
    const int64_t* tri_off;         // (n + 1): the triangles row i emits are [tri_off[i], tri_off[i + 1])
    const int* tri;
    int64_t n;
};

struct HoleSlot { int len, reversed, status, ntri; };        // per gap; len 0: the walk owns no loop
struct HoleSum { long long loops, verts, tris, filled, perimeter, blocked; };
struct HoleSumPlus {
    __host__ __device__ HoleSum operator()(const HoleSum& a, const HoleSum& b) const {
        return HoleSum{a.loops + b.loops, a.verts + b.verts, a.tris + b.tris, a.filled + b.filled, a.perimeter + b.perimeter, a.blocked + b.blocked};
    }
};
struct Tri3 { int a, b, c; };
struct Tri3Less {
    __host__ __device__ bool operator()(const Tri3& x, const Tri3& y) const {
        return x.a != y.a ? x.a < y.a : x.b != y.b ? x.b < y.b : x.c < y.c;
    }
};

struct HoleSlots {
    HoleSlot* slot;                 // (gaps)
    int* verts;                     // (gaps, kHoleMax)
    int* tris;                      // (gaps, kHoleTris, 3)
};

// the position of the resident triangle {a, b, c} in the array; -1: none
__device__ __forceinline__ int64_t tri_resident(const HoleView& h, int a, int b, int c) {
    const int lo = min(a, min(b, c));
    const int x = a == lo ? b : a, y = c == lo ? b : c;      // the two others (lo is one of a, b, c exactly once in a triangle)
    if (a == b || b == c || a == c) return -1;
    const int64_t end = h.tri_off[lo + 1];
    for (int64_t j = h.tri_off[lo]; j < end; ++j) {
        const int t1 = h.tri[j * 3 + 1], t2 = h.tri[j * 3 + 2];
        if ((t1 == x && t2 == y) || (t1 == y && t2 == x)) return j;
    }
    return -1;
}

// a row's fan over its polygon positions: the records are the codes that are not -1
struct Fan {
    const int* codes;
    int n;
    __device__ __forceinline__ bool at(int p) const { return codes[p] != -1; }
    __device__ __forceinline__ int rec(int p) const { return code_record(codes[p]); }
    __device__ __forceinline__ int next(int p) const {
        for (int s = 0; s < n; ++s) {
            p = p + 1 == n ? 0 : p + 1;
            if (codes[p] != -1) break;
        }
        return p;
    }
    __device__ __forceinline__ int prev(int p) const {
        for (int s = 0; s < n; ++s) {
            p = p == 0 ? n - 1 : p - 1;
            if (codes[p] != -1) break;
        }
        return p;
    }
    __device__ __forceinline__ int records() const {
        int m = 0;
        for (int p = 0; p < n; ++p) m += codes[p] != -1 ? 1 : 0;
        return m;
    }
    __device__ __forceinline__ int find(int x) const {
        for (int p = 0; p < n; ++p)
            if (codes[p] != -1 && code_record(codes[p]) == x) return p;
        return -1;
    }
};
__device__ __forceinline__ Fan fan_of(const HoleView& h, int64_t v) {
    Fan F;
    F.codes = fan_codes(h.head, h.fast, h.wide, h.wpitch, v, F.n);
    return F;
}
// sector p of row v (p a record's position; the fan has at least two records)
__device__ __forceinline__ bool sector_filled(const HoleView& h, int v, const Fan& F, int p) {
    return tri_resident(h, v, F.rec(p), F.rec(F.next(p))) >= 0;
}
// faces(x, y) > 0
__device__ __forceinline__ bool edge_taken(const HoleView& h, int x, int y) {
    const Fan F = fan_of(h, x);
    const int p = F.find(y);
    if (p < 0 || F.records() < 2) return false;
    return sector_filled(h, x, F, F.prev(p)) || sector_filled(h, x, F, p);
}

// ---- gaps: one thread per public row ---------------------------------------------------------------------------------------
struct GapArgs {
    int64_t* count;                 // (n + 1): gaps of the row
    const int64_t* off;             // (n + 1): their scan
    int2* gap;                      // (gaps): {F[t], F[s]}
    int* gap_row;                   // (gaps)
    unsigned long long* part;       // (blocks, 4): every block's {boundary edges, odd gaps, -, -}
};

template <bool FILL>
__global__ __launch_bounds__(256) void k_hole_gaps(HoleView h, GapArgs g) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long boundary = 0, odd = 0;
    if (i < h.n) {
        const int2 hd = h.head[i];
        const int n = hd.x;
        const int64_t room = FILL ? g.off[i + 1] - g.off[i] : 0;
        int64_t found = 0;
        // every corner agreed (a bit is only ever set on a proper corner): every sector filled, two faces on every edge
        const bool closed = n >= 3 && n <= 64 && h.mask[i] == (n == 64 ? ~0ull : (1ull << n) - 1ull);
        if (!closed && n >= 2 && (!FILL || room > 0)) {
            const Fan F = fan_of(h, i);
            const int m = F.records();
            if (m >= 2) {
                unsigned long long bits = 0;      // sector p < 64 filled (rows of more vertices -- wide rows only -- ask again)
                for (int p = 0; p < n && p < 64; ++p)
                    if (F.at(p) && sector_filled(h, (int)i, F, p)) bits |= 1ull << p;
                const auto filled = [&](int p) { return p < 64 ? (bits >> p & 1ull) != 0 : sector_filled(h, (int)i, F, p); };
                const auto faces = [&](int p) {
                    const int before = F.prev(p);
                    const bool fb = filled(before), fa = filled(p);
                    return F.rec(F.next(p)) == F.rec(before) ? (fb ? 1 : 0) : (fb ? 1 : 0) + (fa ? 1 : 0);
                };
                for (int p = 0; p < n; ++p) {
                    if (!F.at(p)) continue;
                    const int fp = faces(p);
                    if (!FILL && fp == 1 && F.rec(p) > i) ++boundary;
                    if (!(fp == 1 && !filled(p) && filled(F.prev(p)))) continue;
                    int s = p, fs = 0;
                    for (int step = 0; step < m; ++step) {
                        s = F.next(s);
                        fs = faces(s);
                        if (fs > 0) break;
                    }
                    if (s != p && fs == 1 && filled(s)) {
                        if (FILL && found < room) {
                            g.gap[g.off[i] + found] = make_int2(F.rec(p), F.rec(s));
                            g.gap_row[g.off[i] + found] = (int)i;
                        }
                        ++found;
                    } else {
                        ++odd;
                    }
                }
            }
        }
        if (!FILL) g.count[i] = found;
    }
    if (!FILL) {
        unsigned long long* part = g.part + (int64_t)blockIdx.x * 4;
        block_partial(boundary, false, part);
        block_partial(odd, false, part + 1);
    }
}

// words = {boundary edges, odd gaps}
__global__ __launch_bounds__(256) void k_hole_words(const unsigned long long* __restrict__ part, int blocks, long long* __restrict__ words) {
    __shared__ unsigned long long sh[2][256];
    unsigned long long v[2] = {0, 0};
    for (int b = threadIdx.x; b < blocks; b += 256)
        for (int q = 0; q < 2; ++q) v[q] += part[(int64_t)b * 4 + q];
    for (int q = 0; q < 2; ++q) sh[q][threadIdx.x] = v[q];
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long r = 0;
        for (int t = 0; t < 256; ++t) r += sh[threadIdx.x][t];
        words[threadIdx.x] = (long long)r;
    }
}

// ---- walks: one thread per gap ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_hole_walk(const int64_t* __restrict__ off, const int2* __restrict__ gap, const int* __restrict__ gap_row,
                                                   int64_t gaps, int max_vertices, HoleSlots o) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= gaps) return;
    const int v0 = gap_row[e];
    const int a = gap[e].x, b = gap[e].y;
    int* verts = o.verts + e * kHoleMax;
    verts[0] = v0;
    int len = 1, prev = v0, cur = b;
    bool closed = false;
    for (int it = 0; it < max_vertices; ++it) {
        if (cur == v0) {
            closed = prev == a && len >= 3;
            break;
        }
        if (cur < v0) break;                      // a lower vertex: this walk owns nothing, however it ends
        bool seen = false;
        for (int q = 1; q < len; ++q) seen |= verts[q] == cur;
        if (seen || len == max_vertices) break;
        verts[len++] = cur;
        int nxt = -1;
        const int64_t end = off[cur + 1];
        for (int64_t x = off[cur]; x < end; ++x) {
            const int2 p = gap[x];
            if (p.x == prev || p.y == prev) {
                nxt = p.x == prev ? p.y : p.x;
                break;
            }
        }
        if (nxt < 0) break;
        prev = cur;
        cur = nxt;
    }
    // as walked: [v0, b, ...]; the canonical order starts towards the smaller of a and b
    o.slot[e] = HoleSlot{closed ? len : 0, closed && a < b ? 1 : 0, 0, 0};
}

// ---- perimeter, taken diagonals, dynamic programme, back-trace: one wave per gap ---------------------------------------------
struct Cloud {
    const float* xyz;               // (n, 3) float32, or
    const double4* xyzd;            // (n) the float64 records (null: a float32 cloud)
};

__global__ __launch_bounds__(64) void k_hole_fill(HoleView h, Cloud c, int64_t gaps, double max_perimeter, HoleSlots o, HoleSum* __restrict__ sums) {
    __shared__ double s_w[kHoleMax][kHoleMax + 1];            // (rows padded: lanes read a column)
    __shared__ double s_x[kHoleMax], s_y[kHoleMax], s_z[kHoleMax], s_len[kHoleMax];
    __shared__ int s_v[kHoleMax];
    __shared__ unsigned char s_split[kHoleMax][kHoleMax], s_taken[kHoleMax][kHoleMax];
    __shared__ short s_stack[kHoleMax][2];
    const int64_t e = blockIdx.x;
    const int lane = threadIdx.x;
    if (e >= gaps) return;
    const HoleSlot sl = o.slot[e];
    const int L = sl.len;
    if (L < 3 || L > kHoleMax) {                  // (the walk leaves 0 or 3 .. max_vertices)
        if (lane == 0) sums[e] = HoleSum{0, 0, 0, 0, 0, 0};
        return;
    }
    int* verts = o.verts + e * kHoleMax;
    int mine = -1;
    if (lane < L) {
        mine = verts[lane == 0 ? 0 : sl.reversed ? L - lane : lane];
        s_v[lane] = mine;
        double x, y, z;
        if (c.xyzd) {
            const double4 p = c.xyzd[mine];
            x = p.x; y = p.y; z = p.z;
        } else {
            x = c.xyz[(int64_t)mine * 3]; y = c.xyz[(int64_t)mine * 3 + 1]; z = c.xyz[(int64_t)mine * 3 + 2];
        }
        s_x[lane] = x; s_y[lane] = y; s_z[lane] = z;
    }
    __syncthreads();
    if (lane < L) {
        verts[lane] = mine;                       // the slot in canonical order from here on
        const int nx = lane + 1 == L ? 0 : lane + 1;
        const double dx = s_x[nx] - s_x[lane], dy = s_y[nx] - s_y[lane], dz = s_z[nx] - s_z[lane];
        s_len[lane] = sqrt((dx * dx + dy * dy) + dz * dz);
    }
    for (int idx = lane; idx < kHoleMax * kHoleMax; idx += 64) s_taken[idx / kHoleMax][idx % kHoleMax] = 0;
    __syncthreads();
    double perimeter = 0.0;
    for (int q = 0; q < L; ++q) perimeter = perimeter + s_len[q];          // (every lane the same sum)
    int status = HS_FILLED, ntri = 0;
    if (!(perimeter < max_perimeter)) {
        status = HS_PERIMETER;
    } else {
        // the diagonals that carry a face already; the polygon of three has none and is held against the triangles itself
        for (int idx = lane; idx < L * L; idx += 64) {
            const int x = idx / L, y = idx % L;
            if (x < y && y - x > 1 && !(x == 0 && y == L - 1) && edge_taken(h, s_v[x], s_v[y])) s_taken[x][y] = s_taken[y][x] = 1;
        }
        if (L == 3 && lane == 0 && tri_resident(h, s_v[0], s_v[1], s_v[2]) >= 0) s_taken[0][2] = s_taken[2][0] = 1;
        for (int idx = lane; idx < L - 1; idx += 64) s_w[idx][idx + 1] = 0.0;
        __syncthreads();
        for (int d = 2; d < L; ++d) {
            const int i = lane, j = lane + d;
            if (j < L) {
                double best = __builtin_inf();
                int at = 0;
                const double xi = s_x[i], yi = s_y[i], zi = s_z[i];
                const double vx = s_x[j] - xi, vy = s_y[j] - yi, vz = s_z[j] - zi;
                const bool tij = s_taken[i][j] != 0;
                for (int m = i + 1; m < j; ++m) {
                    const double ux = s_x[m] - xi, uy = s_y[m] - yi, uz = s_z[m] - zi;
                    const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
                    const double w = tij || s_taken[i][m] || s_taken[m][j] ? __builtin_inf() : 0.25 * ((cx * cx + cy * cy) + cz * cz);
                    const double cand = (s_w[i][m] + s_w[m][j]) + w;
                    if (cand < best) {
                        best = cand;
                        at = m;
                    }
                }
                s_w[i][j] = best;
                s_split[i][j] = (unsigned char)at;
            }
            __syncthreads();
        }
        if (!(s_w[0][L - 1] < __builtin_inf())) {
            status = HS_BLOCKED;
        } else {
            ntri = L - 2;
            if (lane == 0) {
                // the one resident face on the edge (v0, w): does it run v0 -> w, as the canonical order does?
                const int v0 = s_v[0], w = s_v[1];
                const Fan F = fan_of(h, v0);
                const int p = F.find(w);
                bool reverse = false;
                if (p >= 0 && F.records() >= 2) {
                    const int before = F.prev(p);
                    const int64_t jb = tri_resident(h, v0, F.rec(before), w), ja = tri_resident(h, v0, w, F.rec(F.next(p)));
                    if ((jb >= 0) != (ja >= 0) || (jb >= 0 && jb == ja)) {
                        const int* t = h.tri + (jb >= 0 ? jb : ja) * 3;
                        reverse = (t[0] == v0 && t[1] == w) || (t[1] == v0 && t[2] == w) || (t[2] == v0 && t[0] == w);
                    }
                }
                int* out = o.tris + e * kHoleTris * 3;
                int top = 0, made = 0;
                s_stack[top][0] = 0; s_stack[top][1] = (short)(L - 1); ++top;
                while (top > 0 && made < kHoleTris) {         // (L - 2 triangles, at most L - 1 intervals waiting)
                    --top;
                    const int i = s_stack[top][0], j = s_stack[top][1];
                    if (j - i < 2) continue;
                    const int m = s_split[i][j];
                    int t0 = s_v[i], t1 = s_v[m], t2 = s_v[j];
                    if (t1 < t0 && t1 < t2) { const int k = t0; t0 = t1; t1 = t2; t2 = k; }
                    else if (t2 < t0 && t2 < t1) { const int k = t2; t2 = t1; t1 = t0; t0 = k; }
                    out[made * 3] = t0; out[made * 3 + 1] = reverse ? t2 : t1; out[made * 3 + 2] = reverse ? t1 : t2;
                    ++made;
                    if (top + 2 <= kHoleMax) {
                        s_stack[top][0] = (short)i; s_stack[top][1] = (short)m; ++top;
                        s_stack[top][0] = (short)m; s_stack[top][1] = (short)j; ++top;
                    }
                }
            }
        }
    }
    if (lane == 0) {
        o.slot[e] = HoleSlot{L, 0, status, ntri};
        sums[e] = HoleSum{1, L, ntri, status == HS_FILLED ? 1 : 0, status == HS_PERIMETER ? 1 : 0, status == HS_BLOCKED ? 1 : 0};
    }
}

// ---- loops and patches to their places: one thread per gap, one more for the offsets' last entry ----------------------------
__global__ __launch_bounds__(256) void k_hole_pack(int64_t gaps, HoleSlots o, const HoleSum* __restrict__ before, int64_t* __restrict__ loop_off,
                                                   int* __restrict__ loop_verts, unsigned char* __restrict__ loop_status, int* __restrict__ patch) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e > gaps) return;
    const HoleSum at = before[e];
    if (e == gaps) {
        loop_off[at.loops] = at.verts;
        return;
    }
    const HoleSlot sl = o.slot[e];
    if (sl.len == 0) return;
    loop_off[at.loops] = at.verts;
    loop_status[at.loops] = (unsigned char)sl.status;
    for (int q = 0; q < sl.len && q < kHoleMax; ++q) loop_verts[at.verts + q] = o.verts[e * kHoleMax + q];
    for (int q = 0; q < sl.ntri * 3 && q < kHoleTris * 3; ++q) patch[at.tris * 3 + q] = o.tris[e * kHoleTris * 3 + q];
}

}  // namespace

int pct_launch_fill_holes(pct_ctx* ctx, int max_vertices, double max_perimeter, pct_stage_report* rep) {
    const int64_t n = ctx->res.rows_of(PCT_R_TRIANGLES), total = ctx->tri_total;
    hipStream_t st = ctx->stream;
    HoleView h = {};
    h.head = (const int2*)ctx->fan_head.p;
    h.fast = (const int*)ctx->fan_fast.p;
    h.wide = (const int*)ctx->fan_wide.p;
    h.wpitch = ctx->tri_wpitch;
    h.mask = (const unsigned long long*)ctx->tri_mask.p;
    h.tri_off = (const int64_t*)ctx->tri_off.p;
    h.tri = (const int*)ctx->tri.p;
    h.n = n;
    const dim3 rblocks((unsigned)((n + 255) / 256));
    PCT_TRY(pct_reserve(ctx, &ctx->hole_cnt, (size_t)(n + 1) * sizeof(int64_t)));
    PCT_TRY(pct_reserve(ctx, &ctx->hole_off, (size_t)(n + 1) * sizeof(int64_t)));
    PCT_TRY(pct_reserve(ctx, &ctx->hole_part, ((size_t)rblocks.x * 4 + 8) * sizeof(unsigned long long)));
    GapArgs g = {};
    g.count = (int64_t*)ctx->hole_cnt.p;
    g.off = (const int64_t*)ctx->hole_off.p;
    g.part = (unsigned long long*)ctx->hole_part.p;
    long long* d_words = (long long*)(g.part + (size_t)rblocks.x * 4);
    long long* pin = ctx->pin->hole_words;
    PCT_HIP(ctx, hipMemsetAsync(g.count + n, 0, sizeof(int64_t), st));
    PCT_LAUNCH(k_hole_gaps<false>, rblocks, dim3(256), 0, st, h, g);
    PCT_HIP(ctx, hipGetLastError());
    PCT_LAUNCH(k_hole_words, dim3(1), dim3(256), 0, st, (const unsigned long long*)g.part, (int)rblocks.x, d_words);
    PCT_HIP(ctx, hipGetLastError());
    size_t bytes = 0;
    int64_t* nul = nullptr;
    PCT_HIP(ctx, rocprim::exclusive_scan(nullptr, bytes, nul, nul, (int64_t)0, (size_t)(n + 1), rocprim::plus<int64_t>(), st));
    PCT_TRY(pct_reserve(ctx, &ctx->hole_tmp, bytes > 0 ? bytes : 1));
    PCT_HIP(ctx, rocprim::exclusive_scan(ctx->hole_tmp.p, bytes, g.count, (int64_t*)ctx->hole_off.p, (int64_t)0, (size_t)(n + 1), rocprim::plus<int64_t>(), st));
    PCT_HIP(ctx, hipMemcpyAsync(pin, d_words, 2 * sizeof(long long), hipMemcpyDeviceToHost, st));
    PCT_HIP(ctx, hipMemcpyAsync(pin + 2, g.off + n, sizeof(long long), hipMemcpyDeviceToHost, st));
    PCT_HIP(ctx, hipStreamSynchronize(st));
    const int64_t boundary = pin[0], odd = pin[1], gaps = pin[2];
    if (gaps > (int64_t)INT32_MAX / (kHoleTris * 3)) return pct_fail(ctx, PCT_ERR_INVALID, "pct_fill_holes: %lld gaps out of range", (long long)gaps);

    HoleSum sum = {0, 0, 0, 0, 0, 0};
    HoleSlots o = {};
    if (gaps > 0) {
        PCT_TRY(pct_reserve(ctx, &ctx->hole_gap, (size_t)gaps * (sizeof(int2) + sizeof(int))));
        g.gap = (int2*)ctx->hole_gap.p;
        g.gap_row = (int*)(g.gap + gaps);
        PCT_LAUNCH(k_hole_gaps<true>, rblocks, dim3(256), 0, st, h, g);
        PCT_HIP(ctx, hipGetLastError());
        const size_t per_gap = sizeof(HoleSlot) + (size_t)(kHoleMax + kHoleTris * 3) * sizeof(int);
        PCT_TRY(pct_reserve(ctx, &ctx->hole_slot, (size_t)gaps * per_gap));
        o.slot = (HoleSlot*)ctx->hole_slot.p;
        o.verts = (int*)(o.slot + gaps);
        o.tris = o.verts + gaps * kHoleMax;
        PCT_LAUNCH(k_hole_walk, dim3((unsigned)((gaps + 255) / 256)), dim3(256), 0, st, g.off, (const int2*)g.gap, (const int*)g.gap_row, gaps,
                   max_vertices, o);
        PCT_HIP(ctx, hipGetLastError());
        PCT_TRY(pct_reserve(ctx, &ctx->hole_scan, (size_t)(gaps + 1) * 2 * sizeof(HoleSum)));
        HoleSum* d_sum = (HoleSum*)ctx->hole_scan.p;
        HoleSum* d_before = d_sum + (gaps + 1);
        PCT_HIP(ctx, hipMemsetAsync(d_sum + gaps, 0, sizeof(HoleSum), st));
        Cloud c = {ctx->xyz_view, ctx->has_f64 ? (const double4*)ctx->pts4d.p : nullptr};
        PCT_LAUNCH(k_hole_fill, dim3((unsigned)gaps), dim3(64), 0, st, h, c, gaps, max_perimeter, o, d_sum);
        PCT_HIP(ctx, hipGetLastError());
        HoleSum* snul = nullptr;
        PCT_HIP(ctx, rocprim::exclusive_scan(nullptr, bytes, snul, snul, sum, (size_t)(gaps + 1), HoleSumPlus(), st));
        PCT_TRY(pct_reserve(ctx, &ctx->hole_tmp, bytes > 0 ? bytes : 1));
        PCT_HIP(ctx, rocprim::exclusive_scan(ctx->hole_tmp.p, bytes, d_sum, d_before, sum, (size_t)(gaps + 1), HoleSumPlus(), st));
        static_assert(sizeof(HoleSum) == 6 * sizeof(long long), "pct_pinned::hole_words");
        PCT_HIP(ctx, hipMemcpyAsync(pin + 2, d_before + gaps, sizeof(HoleSum), hipMemcpyDeviceToHost, st));
        PCT_HIP(ctx, hipStreamSynchronize(st));
        memcpy(&sum, pin + 2, sizeof(HoleSum));
    }
    const int64_t loops = sum.loops, patches = sum.tris;
    if (total + patches > (int64_t)INT32_MAX) return pct_fail(ctx, PCT_ERR_INVALID, "pct_fill_holes: %lld triangles out of range", (long long)(total + patches));

    // the packed loops: offsets | vertices | status
    const size_t off_bytes = (size_t)(loops + 1) * sizeof(int64_t), vert_bytes = (size_t)sum.verts * sizeof(int);
    PCT_TRY(pct_reserve(ctx, &ctx->hole_loop, off_bytes + vert_bytes + (size_t)loops + 1));
    PCT_TRY(pct_reserve(ctx, &ctx->hole_alt, (size_t)(patches > 0 ? patches : 1) * sizeof(Tri3)));
    PCT_TRY(pct_reserve(ctx, &ctx->hole_tri, (size_t)(patches > 0 ? patches : 1) * sizeof(Tri3)));
    PCT_TRY(pct_reserve(ctx, &ctx->hole_filled, (size_t)(total + patches > 0 ? total + patches : 1) * sizeof(Tri3)));
    int64_t* loop_off = (int64_t*)ctx->hole_loop.p;
    int* loop_verts = (int*)((char*)ctx->hole_loop.p + off_bytes);
    unsigned char* loop_status = (unsigned char*)ctx->hole_loop.p + off_bytes + vert_bytes;
    if (gaps > 0) {
        PCT_LAUNCH(k_hole_pack, dim3((unsigned)((gaps + 256) / 256)), dim3(256), 0, st, gaps, o, (const HoleSum*)((HoleSum*)ctx->hole_scan.p + (gaps + 1)),
                   loop_off, loop_verts, loop_status, (int*)ctx->hole_alt.p);
        PCT_HIP(ctx, hipGetLastError());
    } else {
        PCT_HIP(ctx, hipMemsetAsync(loop_off, 0, sizeof(int64_t), st));
    }
    const Tri3* resident = (const Tri3*)ctx->tri.p;
    Tri3* sorted = (Tri3*)ctx->hole_tri.p;
    Tri3* merged = (Tri3*)ctx->hole_filled.p;
    if (patches > 0) {
        PCT_HIP(ctx, rocprim::merge_sort(nullptr, bytes, (Tri3*)ctx->hole_alt.p, sorted, (size_t)patches, Tri3Less(), st));
        PCT_TRY(pct_reserve(ctx, &ctx->hole_tmp, bytes > 0 ? bytes : 1));
        PCT_HIP(ctx, rocprim::merge_sort(ctx->hole_tmp.p, bytes, (Tri3*)ctx->hole_alt.p, sorted, (size_t)patches, Tri3Less(), st));
        PCT_HIP(ctx, rocprim::merge(nullptr, bytes, resident, sorted, merged, (size_t)total, (size_t)patches, Tri3Less(), st));
        PCT_TRY(pct_reserve(ctx, &ctx->hole_tmp, bytes > 0 ? bytes : 1));
        PCT_HIP(ctx, rocprim::merge(ctx->hole_tmp.p, bytes, resident, sorted, merged, (size_t)total, (size_t)patches, Tri3Less(), st));
    } else if (total > 0) {
        PCT_HIP(ctx, hipMemcpyAsync(merged, resident, (size_t)total * sizeof(Tri3), hipMemcpyDeviceToDevice, st));
    }
    ctx->hole_loops = loops;
    ctx->hole_loop_verts = sum.verts;
    ctx->hole_patches = patches;
    const int64_t out[8] = {boundary, gaps, odd, loops, sum.filled, sum.perimeter, sum.blocked, patches};
    for (int q = 0; q < 8; ++q) rep->stats[q] = out[q];
    return PCT_OK;
}

// Mesh-free area weights: the area of every point's Voronoi cell in its own tangent plane, taken from the rows of the
// resident neighbour table -- the `voronoi_areas` that calculate_energies (pct:650-655) sums over and that nothing in
// the reference produces -- and the two energies over them.
//
// Row i, count_i valid neighbours (the contract; tests/voronoi_exact.py states it again in NumPy):
//   block   Q_j = p_j - p_i, load_centred(): cloud dtype, float64 arithmetic from there on
//   frame   R = plane_rotation() of the block from the moments k_fit takes (about the first neighbour, the same
//           operations in the same order: the same rotation bit for bit); (a_j, b_j) = the first two components of
//           R Q_j, (r0 x + r1 y) + r2 z in float64
//   bound   L^2 = max_j (x^2 + y^2) + z^2
//   cell    the square [-L, L]^2, counter-clockwise from (-L, -L), cut by a_j x + b_j y <= rho_j^2 / 2 for every
//           neighbour with rho_j^2 = a_j^2 + b_j^2 > 0, in row order (clip_cell(): one cut, in place)
//   out     area = shoelace, closed = (nverts >= 3 and every vertex has x^2 + y^2 < L^2), nverts
//   NaN     count_i < 2, a table entry outside the cloud, a frame or bound that is not finite: NaN, 0, 0
//
// k_area: one thread per owned row.  The polygon lives in LDS, [vertex][lane] (a wave's accesses to one vertex slot are
// 64 consecutive doubles: conflict-free), kAreaCap vertices per lane; as a private array it would be indexed at run
// time and become scratch.  A neighbour whose bisector lies beyond the farthest vertex cannot cut the cell and never
// touches LDS (the rejection test below; exact up to its slack, so a skipped cut is one that changes nothing).
// A row whose polygon would outgrow kAreaCap goes on a device list (one atomic per wave on the list cursor) and is
// redone by k_area_wide -- one wave per listed row, lane 0 walks it, k + 4 vertices of dynamic LDS: a cut adds at most one
// vertex, so that bound is hard.  Both kernels run area_row(), the same code on the same values: which of them
// finished a row cannot be told from its result.
// Index rows are read from global memory as int4 (rows are 16-byte aligned: the pitch is a multiple of 4), eight
// entries and their eight gathers in flight per lane; one path for every k up to 511, no index staging in LDS -- the LDS
// goes to the polygons.
// Compiled with -ffp-contract=off: the reference restatement rounds every product and sum separately.
#include "pct_fit_core.h"

namespace {

constexpr int kAreaBlock = 64;
// Vertices per lane on the fast path.  16 x 2 doubles x 64 lanes = 16 KiB per wave: ten waves per CU by LDS (DESIGN 4.3h
// has the compiler's resource report and the overflow counts this was chosen from).  -DPCT_AREA_CAP=<n>: an A/B build.
#ifndef PCT_AREA_CAP
#define PCT_AREA_CAP 16
#endif
constexpr int kAreaCap = PCT_AREA_CAP;
constexpr int kAreaAhead = 8;                       // table entries (two int4) and gathers a lane issues together
// rho^2 / 4 > kRejectSlack * (largest vertex radius^2): no vertex can lie beyond the bisector, also after rounding
// (|a x + b y| <= rho |v| <= rho^2 / 2 in exact arithmetic; the slack covers the four roundings of the test it replaces)
constexpr double kRejectSlack = 1.0 + 0x1p-40;

enum AreaStatus { AREA_DONE = 0, AREA_NAN = 1, AREA_OVERFLOW = 2, AREA_SKIP = 3 };
enum AreaWord { AW_OVERFLOW = 0, AW_CLOSED = 1, AW_NAN = 2, AW_SURVIVORS = 3 };     // unsigned long long words of AreaOut::words

struct AreaOut {
    double* area;
    unsigned char* closed;
    int* nverts;
    unsigned long long* words;      // eight words, zeroed per call: AreaWord
    int* over_list;                 // rows k_area hands to k_area_wide
};

// The polygon of one row: vertex i at x[i * STRIDE], y[i * STRIDE] (STRIDE = lanes per block on the fast path)
template <int STRIDE>
struct Poly {
    double* x;
    double* y;
    int cap;
    __device__ __forceinline__ double& X(int i) const { return x[i * STRIDE]; }
    __device__ __forceinline__ double& Y(int i) const { return y[i * STRIDE]; }
};

// One cut of the convex polygon (n vertices, counter-clockwise) by a x + b y <= h, in place.  Vertex v is outside where
// d_v = (a x_v + b y_v) - h > 0.  The outside vertices of a convex polygon are one cyclic run s .. e: the run is
// replaced by the two points where the boundary crosses the line, each taken from its inside end,
// I = P + (d_P / (d_P - d_Q)) (Q - P).  Returns the new count, -1 where it would exceed the capacity (nothing is
// written then), 0 where every vertex is outside (not possible in exact arithmetic: the origin is inside every cut).
// The walk that classes the vertices also takes the largest radius^2 of those that stay: with the two new vertices' that
// is the polygon's new largest radius^2, maxr2 -- the value a second walk over the result would find (a maximum does not
// depend on the order it is taken in).  The next vertex is loaded while this one is classed.
template <int STRIDE>
__device__ __forceinline__ int clip_cell(const Poly<STRIDE>& P, int n, double a, double b, double h, bool& changed, double& maxr2) {
    int s = -1, e = -1, r = 0;
    changed = false;
    double x = P.X(0), y = P.Y(0);
    const bool out0 = (a * x + b * y) - h > 0.0;
    bool prev = out0;
    r = out0 ? 1 : 0;
    double keep = out0 ? 0.0 : x * x + y * y;
    double nx = P.X(n > 1 ? 1 : 0), ny = P.Y(n > 1 ? 1 : 0);
    for (int i = 1; i < n; ++i) {
        x = nx;
        y = ny;
        const int nxt = min(i + 1, n - 1);
        nx = P.X(nxt);
        ny = P.Y(nxt);
        const bool out = (a * x + b * y) - h > 0.0;
        r += out ? 1 : 0;
        if (!out) keep = fmax(keep, x * x + y * y);
        if (out && !prev) s = i;
        if (!out && prev) e = i - 1;
        prev = out;
    }
    if (out0 && !prev) s = 0;
    if (!out0 && prev) e = n - 1;
    if (r == 0) return n;
    changed = true;
    if (r == n || s < 0 || e < 0) return 0;
    const int grown = n - r + 2;
    if (grown > P.cap) return -1;
    const int sp = s == 0 ? n - 1 : s - 1, en = e == n - 1 ? 0 : e + 1;
    double i1x, i1y, i2x, i2y;
    {
        const double px = P.X(sp), py = P.Y(sp), qx = P.X(s), qy = P.Y(s);
        const double dp = (a * px + b * py) - h, dq = (a * qx + b * qy) - h;
        const double t = dp / (dp - dq);
        i1x = px + t * (qx - px);
        i1y = py + t * (qy - py);
    }
    {
        const double px = P.X(en), py = P.Y(en), qx = P.X(e), qy = P.Y(e);
        const double dp = (a * px + b * py) - h, dq = (a * qx + b * qy) - h;
        const double t = dp / (dp - dq);
        i2x = px + t * (qx - px);
        i2y = py + t * (qy - py);
    }
    maxr2 = fmax(keep, fmax(i1x * i1x + i1y * i1y, i2x * i2x + i2y * i2y));
    if (s <= e) {                    // the run s .. e inside the array: I1, I2 take its place, the tail moves by 2 - r
        if (r == 1) {
            for (int i = n - 1; i > e; --i) { P.X(i + 1) = P.X(i); P.Y(i + 1) = P.Y(i); }
        } else if (r > 2) {
            for (int i = e + 1; i < n; ++i) { P.X(i + 2 - r) = P.X(i); P.Y(i + 2 - r) = P.Y(i); }
        }
        P.X(s) = i1x; P.Y(s) = i1y;
        P.X(s + 1) = i2x; P.Y(s + 1) = i2y;
    } else {                         // the run wraps (s .. n-1, 0 .. e): the inside vertices e+1 .. s-1 move to the front
        const int keep = n - r;
        for (int i = 0; i < keep; ++i) { P.X(i) = P.X(i + e + 1); P.Y(i) = P.Y(i + e + 1); }
        P.X(keep) = i1x; P.Y(keep) = i1y;
        P.X(keep + 1) = i2x; P.Y(keep + 1) = i2y;
    }
    return grown;
}

// One row from its table entries to (area, nverts, closed).  survivors: the neighbours the rejection test let through.
template <bool F64, int STRIDE>
__device__ __forceinline__ int area_row(const FitArgs& a, int64_t row, int64_t qid, const float4 qp, const Poly<STRIDE>& P,
                                        double& area, int& nverts, int& closed, unsigned& survivors) {
    const TableRows rows;
    area = (double)__int_as_float(0x7fc00000);
    nverts = 0;
    closed = 0;
    survivors = 0;
    double qx = qp.x, qy = qp.y, qz = qp.z;
    if (F64) {
        const double4 qd = a.ptsd[qid];
        qx = qd.x; qy = qd.y; qz = qd.z;
    }
    const int m = min(rows.length(a, row), a.k);
    if (m < 2) return AREA_NAN;                          // np.cov of fewer than two points: the rows whose fit is NaN
    const int* my = rows.start(a, row);
    const int last4 = a.pitch - 4;

    // kAreaAhead entries from j0 on, every gather issued before the first use.  Entries behind the row's count, and
    // entries that are no record of the cloud, are clamped -- loaded from inside the arrays, never used.
    // The entries of a group are loaded one group ahead (prime() before a pass, then by the gather of the group before):
    // a group waits out one memory latency, not the entries' and then the records'.
    bool bad_id = false;
    int4 w0, w1;
    const auto prime = [&](int j0) {
        w0 = *(const int4*)(my + min(j0, last4));
        w1 = *(const int4*)(my + min(j0 + 4, last4));                   // (clamped only where all four lie behind the row)
    };
    const auto gather = [&](int j0, double (&x)[kAreaAhead], double (&y)[kAreaAhead], double (&z)[kAreaAhead]) {
        const int4 v0 = w0, v1 = w1;
        prime(j0 + kAreaAhead);
        const int id[kAreaAhead] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
        for (int u = 0; u < kAreaAhead; ++u) {
            bad_id |= j0 + u < m && (unsigned)id[u] >= a.n_pts;
            load_centred<F64>(a, (int)min((unsigned)id[u], a.n_pts - 1u), qx, qy, qz, qp.x, qp.y, qp.z, x[u], y[u], z[u]);
        }
    };

    // ---- pass 1: k_fit's moments (about the first neighbour, the same operations in the same order) and L^2 ----------
    double sx = 0, sy = 0, sz = 0, sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
    double fx = 0, fy = 0, fz = 0, lx = 0, ly = 0, lz = 0, L2 = 0;
    prime(0);
    for (int j0 = 0; j0 < m; j0 += kAreaAhead) {
        double x[kAreaAhead], y[kAreaAhead], z[kAreaAhead];
        gather(j0, x, y, z);
        if (j0 == 0) { fx = x[0]; fy = y[0]; fz = z[0]; }
#pragma unroll
        for (int u = 0; u < kAreaAhead; ++u) {
            if (j0 + u < m) {
                const double dx = x[u] - fx, dy = y[u] - fy, dz = z[u] - fz;
                sx += dx; sy += dy; sz += dz;
                sxx = fma(dx, dx, sxx); sxy = fma(dx, dy, sxy); sxz = fma(dx, dz, sxz);
                syy = fma(dy, dy, syy); syz = fma(dy, dz, syz); szz = fma(dz, dz, szz);
                L2 = fmax(L2, (x[u] * x[u] + y[u] * y[u]) + z[u] * z[u]);
                lx = x[u]; ly = y[u]; lz = z[u];
            }
        }
    }
    if (bad_id) return AREA_NAN;
    double rot[9];
    plane_rotation<F64>(m, sx, sy, sz, sxx, sxy, sxz, syy, syz, szz, fx, fy, fz, lx, ly, lz, a.force_jacobi != 0, rot);
    bool finite = L2 < (double)INFINITY;                 // (false for NaN too)
#pragma unroll
    for (int i = 0; i < 6; ++i) finite = finite && fabs(rot[i]) < (double)INFINITY;
    if (!finite) return AREA_NAN;
    const double r00 = rot[0], r01 = rot[1], r02 = rot[2], r10 = rot[3], r11 = rot[4], r12 = rot[5];

    // ---- the cell: [-L, L]^2 cut by every neighbour's bisector, in row order ------------------------------------------
    const double L = sqrt(L2);
    P.X(0) = -L; P.Y(0) = -L;
    P.X(1) = L;  P.Y(1) = -L;
    P.X(2) = L;  P.Y(2) = L;
    P.X(3) = -L; P.Y(3) = L;
    int n = 4;
    double maxr2 = L * L + L * L;                        // the largest x^2 + y^2 over the vertices in place
    bool over = false;
    prime(0);
    for (int j0 = 0; j0 < m && n > 0 && !over; j0 += kAreaAhead) {
        double x[kAreaAhead], y[kAreaAhead], z[kAreaAhead];
        gather(j0, x, y, z);
        // the group's bisectors, and which of them can reach the polygon as it stands: most never leave the registers
        double pa[kAreaAhead], pb[kAreaAhead];
        unsigned need = 0;
#pragma unroll
        for (int u = 0; u < kAreaAhead; ++u) {
            pa[u] = (r00 * x[u] + r01 * y[u]) + r02 * z[u];
            pb[u] = (r10 * x[u] + r11 * y[u]) + r12 * z[u];
            const double rho2 = pa[u] * pa[u] + pb[u] * pb[u];
            // rho2 == 0: a coinciding point, or one straight along the normal -- it keeps its own full cell
            if (j0 + u < m && rho2 > 0.0 && !(0.25 * rho2 > kRejectSlack * maxr2)) need |= 1u << u;
        }
        while (need && n > 0 && !over) {             // in row order; the polygon shrinks, so each is tested again
            const int u = __builtin_ctz(need);
            need &= need - 1;
            double ca = pa[0], cb = pb[0];
#pragma unroll
            for (int v = 1; v < kAreaAhead; ++v) {
                ca = u == v ? pa[v] : ca;
                cb = u == v ? pb[v] : cb;
            }
            const double rho2 = ca * ca + cb * cb;
            if (0.25 * rho2 > kRejectSlack * maxr2) continue;
            ++survivors;
            bool changed;
            const int got = clip_cell(P, n, ca, cb, 0.5 * rho2, changed, maxr2);
            if (got < 0) over = true;
            else if (changed) n = got;
        }
    }
    if (over) return AREA_OVERFLOW;
    double twice = 0;
    for (int i = 0; i < n; ++i) {
        const int nx = i + 1 == n ? 0 : i + 1;
        twice += P.X(i) * P.Y(nx) - P.X(nx) * P.Y(i);
    }
    area = n >= 3 ? 0.5 * twice : 0.0;
    nverts = n;
    closed = n >= 3 && maxr2 < L2 ? 1 : 0;
    return AREA_DONE;
}

template <bool F64>
__global__ __launch_bounds__(kAreaBlock) void k_area(FitArgs a, AreaOut o) {
    __shared__ double s_x[kAreaCap][kAreaBlock], s_y[kAreaCap][kAreaBlock];
    const int lane = threadIdx.x;
    const int64_t row0 = (a.blocks_per_xcd ? (int64_t)(blockIdx.x & 7u) * a.blocks_per_xcd + (blockIdx.x >> 3) : (int64_t)blockIdx.x) * kAreaBlock;
    if (row0 >= a.rows) return;
    const int64_t row = row0 + lane;
    int status = AREA_SKIP, nverts = 0, closed = 0;
    unsigned survivors = 0;
    double area = 0;
    int64_t out = 0;
    if (row < a.rows) {
        const TableRows rows;
        const int64_t qid = rows.query(a, row);
        const float4 qp = a.pts[qid];
        const int pub = __float_as_int(qp.w);
        if (a.out_by_row || (pub >= a.q_begin && pub < a.q_end)) {             // owned rows only
            out = a.out_by_row ? row : (int64_t)pub - a.out_base;
            const Poly<kAreaBlock> P = {&s_x[0][lane], &s_y[0][lane], kAreaCap};
            status = area_row<F64>(a, row, qid, qp, P, area, nverts, closed, survivors);
        }
    }
    if (status == AREA_DONE || status == AREA_NAN) {
        o.area[out] = area;
        o.closed[out] = (unsigned char)closed;
        o.nverts[out] = nverts;
    }
    // the wave's bookkeeping: the rows handed over (one increment of the list cursor per wave), the counts of the statistics
    const unsigned long long om = __ballot(status == AREA_OVERFLOW);
    if (om) {
        const int leader = (int)__builtin_ctzll(om);
        unsigned long long base = 0;
        if (lane == leader) base = atomicAdd(&o.words[AW_OVERFLOW], (unsigned long long)__popcll(om));
        base = __shfl(base, leader);
        if (status == AREA_OVERFLOW) o.over_list[base + __popcll(om & ((1ull << lane) - 1ull))] = (int)row;
    }
    const unsigned long long cm = __ballot(status == AREA_DONE && closed), nm = __ballot(status == AREA_NAN);
    unsigned long long sv = status == AREA_DONE ? survivors : 0u;
    for (int s = 32; s > 0; s >>= 1) sv += __shfl_xor(sv, s);
    if (lane == 0) {
        if (cm) atomicAdd(&o.words[AW_CLOSED], (unsigned long long)__popcll(cm));
        if (nm) atomicAdd(&o.words[AW_NAN], (unsigned long long)__popcll(nm));
        if (sv) atomicAdd(&o.words[AW_SURVIVORS], sv);
    }
}

// The rows k_area could not hold: one wave per listed row, the list length read on the device, room for k + 4 vertices.
template <bool F64>
__global__ __launch_bounds__(kAreaBlock) void k_area_wide(FitArgs a, AreaOut o) {
    extern __shared__ double s_poly[];                   // x[k + 4] | y[k + 4]
    if (threadIdx.x != 0) return;
    const int64_t total = (int64_t)o.words[AW_OVERFLOW];
    const TableRows rows;
    for (int64_t it = blockIdx.x; it < total; it += gridDim.x) {
        const int64_t row = o.over_list[it];
        const int64_t qid = rows.query(a, row);
        const float4 qp = a.pts[qid];
        const int64_t out = a.out_by_row ? row : (int64_t)__float_as_int(qp.w) - a.out_base;
        const Poly<1> P = {s_poly, s_poly + (a.k + 4), a.k + 4};
        double area;
        int nverts, closed;
        unsigned survivors;
        (void)area_row<F64>(a, row, qid, qp, P, area, nverts, closed, survivors);
        o.area[out] = area;
        o.closed[out] = (unsigned char)closed;
        o.nverts[out] = nverts;
        if (closed) atomicAdd(&o.words[AW_CLOSED], 1ull);
        atomicAdd(&o.words[AW_SURVIVORS], (unsigned long long)survivors);
    }
}

// public rows [first, first + rows) of the owned range out of row-ordered results
__global__ __launch_bounds__(256) void k_gather_area(const int* __restrict__ row_of, int64_t first, int64_t rows,
                                                     const double* __restrict__ area, const unsigned char* __restrict__ closed,
                                                     const int* __restrict__ nverts, double* __restrict__ o_area,
                                                     unsigned char* __restrict__ o_closed, int* __restrict__ o_nverts) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const int64_t r = row_of[first + i];
    if (o_area) o_area[i] = area[r];
    if (o_closed) o_closed[i] = closed[r];
    if (o_nverts) o_nverts[i] = nverts[r];
}

// calculate_energies (pct:650-655) over per-point areas: bending = sum double(H2_i) A_i (H2 = the fit's float32 h ** 2),
// stretching = sum double(K_i) A_i, area = sum A_i, over the owned rows i whose area, K and H2 are no NaN -- and whose cell
// is closed, with closed_only.  area_map / fit_map (nullable): where row i of the sum lies in the areas / in the fit.
// Per-block partials in a fixed order, then one block: float64, no atomics on the result, the same bytes for the same table.
constexpr int kEnergyBlock = 256;

__global__ __launch_bounds__(kEnergyBlock) void k_point_energy(const double* __restrict__ area, const unsigned char* __restrict__ closed,
                                                               const float* __restrict__ K, const float* __restrict__ H2,
                                                               const int* __restrict__ area_map, const int* __restrict__ fit_map,
                                                               int64_t rows, int closed_only, double* __restrict__ partial) {
    double bend = 0, stretch = 0, area_sum = 0, used = 0;
    for (int64_t i = (int64_t)blockIdx.x * kEnergyBlock + threadIdx.x; i < rows; i += (int64_t)gridDim.x * kEnergyBlock) {
        const int64_t ia = area_map ? area_map[i] : i, jf = fit_map ? fit_map[i] : i;
        const double A = area[ia];
        const float kg = K[jf], h2 = H2[jf];
        if (!isnan(A) && !isnan(kg) && !isnan(h2) && (!closed_only || closed[ia])) {
            bend += (double)h2 * A;
            stretch += (double)kg * A;
            area_sum += A;
            used += 1.0;
        }
    }
    __shared__ double sh[4][kEnergyBlock / 64];
    for (int o = 32; o > 0; o >>= 1) {
        bend += __shfl_xor(bend, o);
        stretch += __shfl_xor(stretch, o);
        area_sum += __shfl_xor(area_sum, o);
        used += __shfl_xor(used, o);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[0][w] = bend; sh[1][w] = stretch; sh[2][w] = area_sum; sh[3][w] = used; }
    __syncthreads();
    if (threadIdx.x < 4) {
        double s = 0;
        for (int i = 0; i < kEnergyBlock / 64; ++i) s += sh[threadIdx.x][i];
        partial[(int64_t)blockIdx.x * 4 + threadIdx.x] = s;
    }
}

__global__ __launch_bounds__(64) void k_point_final(const double* __restrict__ partial, int nblk, double* __restrict__ out) {
    if (threadIdx.x < 4) {
        double s = 0;
        for (int b = 0; b < nblk; ++b) s += partial[(int64_t)b * 4 + threadIdx.x];   // fixed order
        out[threadIdx.x] = s;
    }
}

}  // namespace

// Areas of the owned rows of the resident table, in the order pct_launch_fit_table leaves its results in (table-row order
// behind a sweep of a cell list, public order otherwise).  The statistics words go to ctx->pin->area_words; both are
// complete once the stream has been waited for.
int pct_launch_point_areas(pct_ctx* ctx) {
    const int64_t rows = ctx->q_end - ctx->q_begin;
    const bool sorted = ctx->knn_sorted_space;
    FitArgs a = {};
    PCT_TRY(fit_source(ctx, sorted ? FitSpace::Sorted : FitSpace::Packed, &a));
    a.table = (const int*)ctx->nbr_pos.p;
    a.cnt = ctx->eps > 0 ? (const int*)ctx->nbr_cnt.p : nullptr;
    a.row_query32 = sorted ? (const int*)ctx->owned_pos.p : nullptr;
    a.row_offset = sorted ? 0 : ctx->q_begin;
    a.rows = rows;
    a.k = ctx->k;
    a.pitch = ctx->nbr_pitch;
    a.out_by_row = sorted ? 1 : 0;
    a.out_base = ctx->q_begin;
    a.q_begin = (int)ctx->q_begin;
    a.q_end = (int)ctx->q_end;
    a.force_jacobi = fit_jacobi_forced();
    PCT_TRY(pct_reserve(ctx, &ctx->area, (size_t)rows * sizeof(double)));
    PCT_TRY(pct_reserve(ctx, &ctx->area_closed, (size_t)rows));
    PCT_TRY(pct_reserve(ctx, &ctx->area_nverts, (size_t)rows * sizeof(int)));
    PCT_TRY(pct_reserve(ctx, &ctx->area_over, 64 + (size_t)rows * sizeof(int)));
    AreaOut o = {(double*)ctx->area.p, (unsigned char*)ctx->area_closed.p, (int*)ctx->area_nverts.p,
                 (unsigned long long*)ctx->area_over.p, (int*)ctx->area_over.p + 16};
    PCT_HIP(ctx, hipMemsetAsync(ctx->area_over.p, 0, 64, ctx->stream));
    int blocks = (int)((rows + kAreaBlock - 1) / kAreaBlock);
    if (blocks > 0) {
        a.blocks_per_xcd = pct_getenv("PCT_NO_XCD_MAP") ? 0 : (blocks + 7) / 8;
        if (a.blocks_per_xcd) blocks = a.blocks_per_xcd * 8;
        const int wblocks = blocks < 1024 ? blocks : 1024;
        const size_t wlds = (size_t)(a.k + 4) * 2 * sizeof(double);
        if (ctx->has_f64) {
            PCT_LAUNCH(k_area<true>, dim3(blocks), dim3(kAreaBlock), 0, ctx->stream, a, o);
            PCT_LAUNCH(k_area_wide<true>, dim3(wblocks), dim3(kAreaBlock), wlds, ctx->stream, a, o);
        } else {
            PCT_LAUNCH(k_area<false>, dim3(blocks), dim3(kAreaBlock), 0, ctx->stream, a, o);
            PCT_LAUNCH(k_area_wide<false>, dim3(wblocks), dim3(kAreaBlock), wlds, ctx->stream, a, o);
        }
        PCT_HIP(ctx, hipGetLastError());
    }
    PCT_HIP(ctx, hipMemcpyAsync(ctx->pin->area_words, ctx->area_over.p, sizeof(ctx->pin->area_words), hipMemcpyDeviceToHost, ctx->stream));
    ctx->area_row_order = sorted;
    return PCT_OK;
}

int pct_launch_gather_areas(pct_ctx* ctx, int64_t first, int64_t rows, double* d_area, unsigned char* d_closed, int* d_nverts) {
    PCT_TRY(pct_ensure_row_of(ctx));
    PCT_LAUNCH(k_gather_area, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, ctx->stream, (const int*)ctx->row_of.p, first, rows,
               (const double*)ctx->area.p, (const unsigned char*)ctx->area_closed.p, (const int*)ctx->area_nverts.p, d_area, d_closed,
               d_nverts);
    PCT_HIP(ctx, hipGetLastError());
    return PCT_OK;
}

// d_out4 = {bending, stretching, area, rows used}; d_partial: room for 4 doubles per block (at most 1024 blocks)
int pct_launch_point_energies(pct_ctx* ctx, bool closed_only, double* d_partial, double* d_out4) {
    const int64_t rows = ctx->q_end - ctx->q_begin;
    const int nblk = (int)((rows + kEnergyBlock - 1) / kEnergyBlock < 1024 ? (rows + kEnergyBlock - 1) / kEnergyBlock : 1024);
    const int *area_map = nullptr, *fit_map = nullptr;
    if (ctx->area_row_order != ctx->fit_row_order) {      // one of the two in table-row order, the other in public order
        PCT_TRY(pct_ensure_row_of(ctx));
        (ctx->area_row_order ? area_map : fit_map) = (const int*)ctx->row_of.p;
    }
    PCT_LAUNCH(k_point_energy, dim3(nblk > 0 ? nblk : 1), dim3(kEnergyBlock), 0, ctx->stream, (const double*)ctx->area.p,
               (const unsigned char*)ctx->area_closed.p, (const float*)ctx->K.p, (const float*)ctx->H2.p, area_map, fit_map, rows,
               closed_only ? 1 : 0, d_partial);
    PCT_LAUNCH(k_point_final, dim3(1), dim3(64), 0, ctx->stream, (const double*)d_partial, nblk > 0 ? nblk : 1, d_out4);
    PCT_HIP(ctx, hipGetLastError());
    return PCT_OK;
}

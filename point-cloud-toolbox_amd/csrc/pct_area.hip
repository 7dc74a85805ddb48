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
// clip_cell() and area_row() live in pct_area_row.h, which pct_fan.hip shares (the same cuts with a label per edge).
#include "pct_area_row.h"

namespace {

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
int pct_launch_point_areas(pct_ctx* ctx, bool* by_row) {
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
    *by_row = sorted;
    return PCT_OK;
}

// rows, closed rows, NaN rows, overflow rows; behind the milliseconds, as a double: neighbours past the rejection test
void pct_area_report(pct_ctx* ctx, pct_stage_report* rep) {
    const unsigned long long* w = ctx->pin->area_words;
    const int64_t st[4] = {ctx->q_end - ctx->q_begin, (int64_t)w[AW_CLOSED], (int64_t)w[AW_NAN], (int64_t)w[AW_OVERFLOW]};
    for (int i = 0; i < 4; ++i) rep->stats[i] = st[i];
    rep->ms[1] = (double)w[AW_SURVIVORS];
}

// d_out4 ={bending, stretching, area, rows used}; d_partial: room for 4 doubles per block (at most 1024 blocks)
int pct_launch_point_energies(pct_ctx* ctx, bool closed_only, double* d_partial, double* d_out4) {
    const int64_t rows = ctx->q_end - ctx->q_begin;
    const int nblk = (int)((rows + kEnergyBlock - 1) / kEnergyBlock < 1024 ? (rows + kEnergyBlock - 1) / kEnergyBlock : 1024);
    const int *area_map = nullptr, *fit_map = nullptr;
    const bool area_by_row = ctx->res.in_row_order(PCT_R_AREAS);
    if (area_by_row != ctx->res.in_row_order(PCT_R_FIT)) {      // one of the two in table-row order, the other in public order
        PCT_TRY(pct_ensure_row_of(ctx));
        (area_by_row ? area_map : fit_map) = (const int*)ctx->row_of.p;
    }
    PCT_LAUNCH(k_point_energy, dim3(nblk > 0 ? nblk : 1), dim3(kEnergyBlock), 0, ctx->stream, (const double*)ctx->area.p,
               (const unsigned char*)ctx->area_closed.p, (const float*)ctx->K.p, (const float*)ctx->H2.p, area_map, fit_map, rows,
               closed_only ? 1 : 0, d_partial);
    PCT_LAUNCH(k_point_final, dim3(1), dim3(64), 0, ctx->stream, (const double*)d_partial, nblk > 0 ? nblk : 1, d_out4);
    PCT_HIP(ctx, hipGetLastError());
    return PCT_OK;
}

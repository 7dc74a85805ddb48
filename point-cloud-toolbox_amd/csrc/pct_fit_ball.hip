// Quadric fit of radius neighbourhoods (pct_fit_ball): the CSR rows the last pct_query_ball left on the device, fitted
// about their centres -- A5-A7 of the reference (pct:270-321, 331-360, 398-431) on the block points[ranked] - points[c],
// `ranked` the members of the row ascending by key.  Semantics: include/pct_hip.h; the route of a row: pct_fit_ball_plan.h.
//
//   members   the row's entries e != c (c the centre's public index); key(e) = (d2, e), d2 = (dx*dx + dy*dy) + dz*dz in
//             fp64 from the float32 record of e and the centre (pct_query_ball's expression with the centre as the query).
//             `near` / `far` = the members with the smallest / largest key: all of the ranking the reference's steps use
//             (pct:286 takes points[-1] - points[0]; everything else is a sum over the members).
//   split     k_ball_table, one thread per row: a row of at most kBallFitShortMax members is copied into row `row` of a
//             (rows, pitch) table -- near in slot 0, far in the last valid slot, the rest in row order -- with its member
//             count; any other row reads count 0 there and is appended to the list of the wave kernel.  The table goes
//             through pct_launch_fit_rows32, i.e. k_fit and its k_fit_svd as they are (one thread per row: 64 short rows
//             per wave, where a wave of its own would reduce 27 sums for 17 members).
//   wave      k_fit_ball<F64>, one wave per listed row, grid-stride.  Pass 1: the lanes stride the members, gather their
//             public-order records, centre them in the native dtype and keep fp64 moments about the row's first member
//             (known before the pass) and the two keyed extremes; a butterfly over the lanes leaves the nine sums and the
//             extremes in every lane.  plane_rotation() runs wave-uniformly.  Pass 2: rotate, round to float32, float32
//             design row, per-lane fp64 normal equations, the same butterfly over the 21 + 6 sums, then k_fit's pivot-ratio
//             gate and Cholesky solve in every lane; lane 0 stores.  A lane's members, their order and the butterfly are
//             fixed by the row alone: the grid size, the list position and the route of other rows change no bit.
//   svd       rows of fewer than six members and rows that fail the gate go to a device list and from there through
//             fit_svd_rows (pct_fit_core.h) with the CSR accessor: k_fit_svd's body, Lstsq6 and all (NaN below two members).
#include "pct_fit_core.h"
#include "pct_fit_ball_plan.h"

namespace {

constexpr int kBallFitWaves = 4;               // waves per block of k_fit_ball
constexpr int kBallFitMaxBlocks = 4096;        // grid cap: 256 CUs x 16 blocks; the rest by grid stride

struct BallFitArgs {
    FitArgs f;                  // pts / ptsd (public order), n_pts, outputs (row-aligned), flag list, force_jacobi, svd_accumulate
    const int64_t* off;         // (rows + 1) CSR offsets
    const int* idx;             // entries: public indices
    const int* self32;          // (rows) the centre of every row
    int64_t rows;
    const int* list;            // rows of the wave kernel ...
    const int* list_count;      // ... and how many (device word)
    int* used;                  // (rows) members fitted
};

__device__ __forceinline__ int clamp_id(int id, unsigned n) { return (int)min((unsigned)id, n - 1u); }

// CSR rows for fit_svd_rows: the row's entries, the centre skipped, near / far by key
struct CsrRows {
    static constexpr bool kKeyed = true;
    const int64_t* off;
    const int* idx;
    const int* self32;
    __device__ __forceinline__ int64_t query(const FitArgs&, int64_t row) const { return self32[row]; }
    __device__ __forceinline__ const int* start(const FitArgs&, int64_t row) const { return idx + off[row]; }
    __device__ __forceinline__ int length(const FitArgs&, int64_t row) const { return (int)(off[row + 1] - off[row]); }
};

template <bool F64>
__global__ __launch_bounds__(64) void k_fit_ball_svd(FitArgs a, CsrRows rows, const int* __restrict__ list,
                                                     const int* __restrict__ list_count, long long* __restrict__ host_count) {
    fit_svd_rows<F64, false>(a, rows, list, list_count, host_count);
}

// sum over the wave, the same bits in every lane: lane i adds what lane i ^ o holds, and a + b == b + a
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <bool F64>
__global__ __launch_bounds__(64 * kBallFitWaves) void k_fit_ball(BallFitArgs b) {
    const FitArgs& a = b.f;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int total = *b.list_count;
    const float nanf_ = __int_as_float(0x7fc00000);
    for (int64_t it = (int64_t)blockIdx.x * kBallFitWaves + w; it < total; it += (int64_t)gridDim.x * kBallFitWaves) {
        const int row = b.list[it];
        const int64_t beg = b.off[row];
        const int len = (int)(b.off[row + 1] - beg);
        const int* __restrict__ my = b.idx + beg;
        const int c = b.self32[row];
        const float4 qp = a.pts[c];
        double qx = qp.x, qy = qp.y, qz = qp.z;
        if (F64) { const double4 qd = a.ptsd[c]; qx = qd.x; qy = qd.y; qz = qd.z; }

        // the shift of the moments: the row's first member, centred (any point of the neighbourhood serves: the
        // covariance does not depend on it, its rounding does -- see k_fit's pass 1)
        double hx = 0, hy = 0, hz = 0;
        if (len > 0) {
            int e0 = my[0];
            if (e0 == c && len > 1) e0 = my[1];
            load_centred<F64>(a, clamp_id(e0, a.n_pts), qx, qy, qz, qp.x, qp.y, qp.z, hx, hy, hz);
        }

        // ---- pass 1: moments about the shift, the keyed extremes, the member count ----------------------------
        double sx = 0, sy = 0, sz = 0, sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
        double nd = (double)INFINITY, fd = -1.0;
        int ne = 0x7fffffff, fe = -1;
        int members = 0;
        bool bad = false;
        for (int j0 = 0; j0 < len; j0 += 64) {
            const int j = j0 + lane;
            const int e = j < len ? my[j] : c;
            const bool mem = e != c;
            members += (int)__popcll(__ballot(mem));
            if (mem) {
                bad |= (unsigned)e >= a.n_pts;
                const int id = clamp_id(e, a.n_pts);
                const float4 p = a.pts[id];
                const double kx = (double)p.x - qx, ky = (double)p.y - qy, kz = (double)p.z - qz;
                const double d2 = (kx * kx + ky * ky) + kz * kz;
                if (d2 < nd || (d2 == nd && e < ne)) { nd = d2; ne = e; }
                if (d2 > fd || (d2 == fd && e > fe)) { fd = d2; fe = e; }
                double x, y, z;
                load_centred<F64>(a, id, qx, qy, qz, qp.x, qp.y, qp.z, x, y, z);
                const double dx = x - hx, dy = y - hy, dz = z - hz;
                sx += dx; sy += dy; sz += dz;
                sxx = fma(dx, dx, sxx); sxy = fma(dx, dy, sxy); sxz = fma(dx, dz, sxz);
                syy = fma(dy, dy, syy); syz = fma(dy, dz, syz); szz = fma(dz, dz, szz);
            }
        }
        float* co = a.coefs + (int64_t)row * 6;
        const auto store_nan = [&]() {
            if (lane < 6) co[lane] = nanf_;
            if (lane == 0) { a.K[row] = nanf_; a.H[row] = nanf_; a.H2[row] = nanf_; }
        };
        const auto hand_over = [&]() {          // (wave-uniform: one increment per row)
            if (lane == 0) a.flag_list[atomicAdd(a.flag_count, 1)] = row;
        };
        if (lane == 0) b.used[row] = members;
        if (__any(bad)) {                        // an entry that is no record of the cloud
            store_nan();
            continue;
        }
        if (members < 6) {                       // under-determined: lstsq's minimum-norm answer; fewer than two members: NaN (fit_svd_rows)
            store_nan();
            hand_over();
            continue;
        }
        sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz);
        sxx = wave_sum(sxx); sxy = wave_sum(sxy); sxz = wave_sum(sxz);
        syy = wave_sum(syy); syz = wave_sum(syz); szz = wave_sum(szz);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double od = __shfl_xor(nd, o);
            const int oe = __shfl_xor(ne, o);
            if (od < nd || (od == nd && oe < ne)) { nd = od; ne = oe; }
            const double pd = __shfl_xor(fd, o);
            const int pe = __shfl_xor(fe, o);
            if (pd > fd || (pd == fd && pe > fe)) { fd = pd; fe = pe; }
        }
        double fx, fy, fz, lx, ly, lz;
        load_centred<F64>(a, clamp_id(ne, a.n_pts), qx, qy, qz, qp.x, qp.y, qp.z, fx, fy, fz);
        load_centred<F64>(a, clamp_id(fe, a.n_pts), qx, qy, qz, qp.x, qp.y, qp.z, lx, ly, lz);
        double rot[9];
        plane_rotation<F64>(members, sx, sy, sz, sxx, sxy, sxz, syy, syz, szz, fx, fy, fz, lx, ly, lz, a.force_jacobi != 0, rot);

        // ---- pass 2: float32 design rows -> fp64 normal equations (k_fit's PASS2_ACC) -------------------------
        double g[21];
        double rhs[6];
#pragma unroll
        for (int i = 0; i < 21; ++i) g[i] = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i) rhs[i] = 0;
        for (int j0 = 0; j0 < len; j0 += 64) {
            const int j = j0 + lane;
            const int e = j < len ? my[j] : c;
            if (e != c) {
                double x, y, z;
                load_centred<F64>(a, e, qx, qy, qz, qp.x, qp.y, qp.z, x, y, z);      // (pass 1 found every entry inside the cloud)
                const float pa = (float)((rot[0] * x + rot[1] * y) + rot[2] * z);
                const float pb = (float)((rot[3] * x + rot[4] * y) + rot[5] * z);
                const float pz = (float)((rot[6] * x + rot[7] * y) + rot[8] * z);
                double cc[6];
                cc[0] = (double)(pa * pa);
                cc[1] = (double)(pb * pb);
                cc[2] = (double)(pa * pb);
                cc[3] = (double)pa;
                cc[4] = (double)pb;
                cc[5] = 1.0;
                const double zz = (double)pz;
                int t = 0;
#pragma unroll
                for (int i = 0; i < 6; ++i) {
#pragma unroll
                    for (int jj = 0; jj <= i; ++jj) { g[t] = fma(cc[i], cc[jj], g[t]); ++t; }
                    rhs[i] = fma(cc[i], zz, rhs[i]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 21; ++i) g[i] = wave_sum(g[i]);
#pragma unroll
        for (int i = 0; i < 6; ++i) rhs[i] = wave_sum(rhs[i]);

        // ---- Cholesky G = L L^T, the pivot-ratio gate, the two triangular solves: as k_fit, in every lane ------
#define GI(i, j) ((i) * ((i) + 1) / 2 + (j))
        double dinv[6];
        bool well = true;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double d = g[GI(j, j)];
#pragma unroll
            for (int p = 0; p < j; ++p) d -= g[GI(j, p)] * g[GI(j, p)];
            well = well && d > kPivotRatioMin * g[GI(j, j)];
            const double inv = rsqrt(d);
            dinv[j] = inv;
#pragma unroll
            for (int i = j + 1; i < 6; ++i) {
                double s = g[GI(i, j)];
#pragma unroll
                for (int p = 0; p < j; ++p) s -= g[GI(i, p)] * g[GI(j, p)];
                g[GI(i, j)] = s * inv;
            }
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double s = rhs[i];
#pragma unroll
            for (int p = 0; p < i; ++p) s -= g[GI(i, p)] * rhs[p];
            rhs[i] = s * dinv[i];
        }
#pragma unroll
        for (int i = 5; i >= 0; --i) {
            double s = rhs[i];
#pragma unroll
            for (int p = i + 1; p < 6; ++p) s -= g[GI(p, i)] * rhs[p];
            rhs[i] = s * dinv[i];
        }
#undef GI
        if (!well) hand_over();                  // (its answer replaces the one stored below)
        if (lane == 0) {
            const float A = (float)rhs[0], B = (float)rhs[1], C = (float)rhs[2];
            const float D = (float)rhs[3], E = (float)rhs[4], F = (float)rhs[5];
            co[0] = A; co[1] = B; co[2] = C; co[3] = D; co[4] = E; co[5] = F;
            float Kg, Kh;
            monge_curvatures(A, B, C, D, E, Kg, Kh);
            a.K[row] = Kg;
            a.H[row] = Kh;
            a.H2[row] = Kh * Kh;
        }
    }
}

// One thread per row: its class (pct_fit_ball_plan.h); a table row and its count for the short ones, a place on the wave
// kernel's list for the others.  words[0] = rows listed, words[1] = rows in the table.  table == null: every row is listed.
template <bool F64>
__global__ __launch_bounds__(256) void k_ball_table(BallFitArgs b, int short_max, int pitch, int* __restrict__ table,
                                                    int* __restrict__ cnt, int* __restrict__ list, int* __restrict__ words) {
    const FitArgs& a = b.f;
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = row < b.rows;
    bool listed = false;
    if (live) {
        const int64_t beg = b.off[row];
        const int64_t len = b.off[row + 1] - beg;
        const int* __restrict__ my = b.idx + beg;
        const int c = b.self32[row];
        // at most one entry is the centre's unless the caller names another row's centre: count, do not assume
        int members = 0;
        listed = table == nullptr || len > (int64_t)short_max + 1;
        if (!listed) {
            for (int j = 0; j < (int)len; ++j) members += my[j] != c;
            listed = ball_fit_class(members, short_max, true) == kBallFitWave;
        }
        if (!listed) {
            const float4 qp = a.pts[c];
            double qx = qp.x, qy = qp.y, qz = qp.z;
            if (F64) { const double4 qd = a.ptsd[c]; qx = qd.x; qy = qd.y; qz = qd.z; }
            double nd = (double)INFINITY, fd = -1.0;
            int ne = 0x7fffffff, fe = -1;
            for (int j = 0; j < (int)len; ++j) {
                const int e = my[j];
                if (e == c) continue;
                const float4 p = a.pts[clamp_id(e, a.n_pts)];
                const double dx = (double)p.x - qx, dy = (double)p.y - qy, dz = (double)p.z - qz;
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 < nd || (d2 == nd && e < ne)) { nd = d2; ne = e; }
                if (d2 > fd || (d2 == fd && e > fe)) { fd = d2; fe = e; }
            }
            int* __restrict__ t = table + row * pitch;           // 2 <= members <= short_max <= pitch
            t[0] = ne;
            t[members - 1] = fe;
            int slot = 1;
            for (int j = 0; j < (int)len; ++j) {
                const int e = my[j];
                if (e == c || e == ne || e == fe) continue;
                if (slot < members - 1) t[slot] = e;             // (a row with a repeated entry would run past its count: dropped)
                ++slot;
            }
            cnt[row] = members;
            b.used[row] = members;
        } else if (table) {
            cnt[row] = 0;                                        // k_fit stores NaN there, k_fit_ball the fit behind it
        }
    }
    // the rows listed: one counter increment per wave
    const unsigned long long lm = __ballot(listed);
    if (lm) {
        const int lane = threadIdx.x & 63;
        const int leader = (int)__builtin_ctzll(lm);
        int base = 0;
        if (lane == leader) base = atomicAdd(&words[0], (int)__popcll(lm));
        base = __shfl(base, leader);
        if (listed) list[base + (int)__popcll(lm & ((1ull << lane) - 1ull))] = (int)row;
    }
    const unsigned long long tm = __ballot(live && !listed);
    if (tm && (threadIdx.x & 63) == (int)__builtin_ctzll(tm)) atomicAdd(&words[1], (int)__popcll(tm));
}

int ball_fit_route_knob() { return ball_fit_knob(pct_getenv("PCT_FIT_BALL_ROUTE")); }

int ball_fit_short_max() {                    // PCT_FIT_BALL_SHORT=<members>: a developer's A/B runs of kBallFitShortMax (tools/ball_fit_probe.py)
    const char* e = pct_getenv("PCT_FIT_BALL_SHORT");
    const int v = e ? atoi(e) : kBallFitShortMax;
    return v < 1 ? 1 : v > 255 ? 255 : v;       // (up to 255 members k_fit stages its rows in LDS)
}

}  // namespace

// d_self32 (rows): the centres, validated by the caller.  d_used (rows): members per row.  Outputs row-aligned in
// ctx->coefs / K / H / H2 (reserved by the caller).  The pinned SVD row count of slot 0 is complete at the next
// synchronisation.
int pct_launch_fit_ball(pct_ctx* ctx, const int* d_self32, int64_t rows, int* d_used) {
    BallFitArgs b = {};
    PCT_TRY(fit_source(ctx, FitSpace::Public, &b.f));
    const bool f64 = ctx->has_f64;
    const int short_max = ball_fit_short_max(), pitch = ball_fit_pitch(short_max);
    const bool with_table = ball_fit_table_allowed(rows, short_max, ball_fit_route_knob());

    // scratch: words (64 B) | wave list (rows) | flag list (rows) | counts (rows);  the table apart
    const size_t row_ints = ((size_t)rows + 15) & ~(size_t)15;
    pct_stage_scope stage(ctx);
    int* words = nullptr;                        // [0] listed rows, [1] table rows, [2] flagged rows
    PCT_TRY(pct_claim(ctx, 16 + 3 * row_ints, &words));
    int* list = words + 16;
    int* flag_list = list + row_ints;
    int* cnt = flag_list + row_ints;
    char* table_bytes = nullptr;
    if (with_table) PCT_TRY(pct_claim(ctx, (size_t)ball_fit_table_bytes(rows, short_max), &table_bytes));
    int* table = (int*)table_bytes;
    PCT_HIP(ctx, hipMemsetAsync(words, 0, 64, ctx->stream));

    b.f.out_by_row = 1;
    b.f.coefs = (float*)ctx->coefs.p;
    b.f.K = (float*)ctx->K.p;
    b.f.H = (float*)ctx->H.p;
    b.f.H2 = (float*)ctx->H2.p;
    b.f.flag_list = flag_list;
    b.f.flag_count = words + 2;
    b.f.force_jacobi = fit_jacobi_forced();
    b.off = (const int64_t*)ctx->ball_off.p;
    b.idx = (const int*)ctx->ball_idx.p;
    b.self32 = d_self32;
    b.rows = rows;
    b.list = list;
    b.list_count = words;
    b.used = d_used;

    const dim3 tblocks((unsigned)((rows + 255) / 256));
    if (f64) PCT_LAUNCH(k_ball_table<true>, tblocks, dim3(256), 0, ctx->stream, b, short_max, pitch, table, cnt, list, words);
    else PCT_LAUNCH(k_ball_table<false>, tblocks, dim3(256), 0, ctx->stream, b, short_max, pitch, table, cnt, list, words);
    PCT_HIP(ctx, hipGetLastError());
    int counts[2] = {0, 0};                      // one read-back: what each route has to do
    PCT_HIP(ctx, hipMemcpyAsync(counts, words, sizeof(counts), hipMemcpyDeviceToHost, ctx->stream));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int n_wave = counts[0], n_table = counts[1];

    bool svd_written = false;
    if (n_table > 0) {
        // every row of the query is a row of the table (the listed ones with count 0): outputs stay row-aligned
        PCT_TRY(pct_launch_fit_rows32(ctx, table, cnt, d_self32, rows, short_max, pitch, b.f.coefs, b.f.K, b.f.H, b.f.H2));
        svd_written = true;
    }
    long long* note = &ctx->pin->svd_rows[0];
    if (n_wave > 0) {
        const int wblocks = (n_wave + kBallFitWaves - 1) / kBallFitWaves;
        const dim3 grid((unsigned)(wblocks < kBallFitMaxBlocks ? wblocks : kBallFitMaxBlocks)), block(64 * kBallFitWaves);
        if (f64) PCT_LAUNCH(k_fit_ball<true>, grid, block, 0, ctx->stream, b);
        else PCT_LAUNCH(k_fit_ball<false>, grid, block, 0, ctx->stream, b);
        PCT_HIP(ctx, hipGetLastError());
        b.f.svd_accumulate = svd_written ? 1 : 0;
        const CsrRows csr = {b.off, b.idx, b.self32};
        const int sblocks = (n_wave + 63) / 64 < 1024 ? (n_wave + 63) / 64 : 1024;
        if (f64) PCT_LAUNCH(k_fit_ball_svd<true>, dim3(sblocks), dim3(64), 0, ctx->stream, b.f, csr, (const int*)flag_list, (const int*)(words + 2), note);
        else PCT_LAUNCH(k_fit_ball_svd<false>, dim3(sblocks), dim3(64), 0, ctx->stream, b.f, csr, (const int*)flag_list, (const int*)(words + 2), note);
        PCT_HIP(ctx, hipGetLastError());
        svd_written = true;
    }
    if (!svd_written) *note = 0;                 // (rows == 0 does not get here; kept for a query of empty tables)
    return PCT_OK;
}

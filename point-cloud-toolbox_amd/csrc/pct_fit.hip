// Fused per-point kernel for the three per-neighbourhood staticmethods of the
// reference and the two all-points loops around them:
//   get_best_fit_plane_and_rotate            pointCloudToolbox.py:270-321
//   fit_quadratic_surface                    pointCloudToolbox.py:331-360
//   calculate_explicit_quadratic_curvatures  pointCloudToolbox.py:398-431
//   loops                                    pointCloudToolbox.py:635-647, 657-674
//
// One thread per point (tiny dense per-point algebra, no MFMA).  A 64-thread
// workgroup stages its 64 neighbour-index rows into LDS with coalesced loads
// (odd row pitch -> conflict-free column reads; letting every lane stream its
// own row from global instead was measured 2x slower), then every lane walks
// its own row twice, gathers issued kFitAhead neighbours ahead of their use:
//   pass 1  centred neighbours (native dtype, pct:641) -> fp64 sums about the
//           first neighbour -> 3x3 covariance, ddof=1 (pct:277) -> normal =
//           eigenvector of the smallest eigenvalue (== Vt[-1], pct:283;
//           direct_normal(), cyclic Jacobi where that row is not healthy)
//           -> sign flip by far-minus-near
//           neighbour (pct:286-297) -> Rodrigues rotation to +z (pct:300-312)
//   pass 2  rotate (pct:315), round to float32 (pct:350), float32 design row
//           [a^2,b^2,ab,a,b,1] (pct:358), fp64 normal equations, Cholesky
//           solve, coefficients rounded to float32 (pct:359)
//   then    K, H, H^2 in float32 arithmetic in the reference's operation order
//           (pct:403-422).
// Compiled with -ffp-contract=off so the float32 sequences are not fused.
#include "pct_fit_core.h"

namespace {

constexpr int kFitBlock = 64;

// Gathers a lane issues together in the two neighbour loops, before it uses the first of them: a lane waits out one
// memory latency per group and one per neighbour behind the last full group.  Measured on the 1 M-point torus and on
// C4 / C5 (profiles/r06_a_fit_keep_ab.txt): 10 beats 8 at k = 30, 45, 50, 64, 80 and 100 (k_fit 179 against 185 us at
// k = 50); 12 (162 registers) and 16 (186, two waves per SIMD) lose, and so does every way tried of grouping the
// neighbours behind the last full group, which moves the register allocation of the loops themselves.
// -DPCT_FIT_AHEAD=<n> on this file: a developer's A/B build (tools/build_variant.py).
#ifndef PCT_FIT_AHEAD
#define PCT_FIT_AHEAD 10
#endif
constexpr int kFitAhead = PCT_FIT_AHEAD;

// STAGED = false: rows too long for the LDS staging area (k > 255) are walked in global memory instead.  Both tables
// get here: the resident one of the wide sweeps (k = 256 .. 511: sorted-space positions, the table's pitch, float64
// clouds, eps counts) and caller-supplied rows (pct_fit_indices takes any k the reference's fit would).
// MASKED: a compile-time variant, so that the row test leaves the hot instantiation's register allocation alone.
template <bool F64, bool OUT64 = false, bool STAGED = true, bool MASKED = false>
__global__ __launch_bounds__(kFitBlock) void k_fit(FitArgs a) {
    extern __shared__ int s_idx[];   // 64 rows x kp
    const int lane = threadIdx.x;
    if (a.stamps) pct_stamp(&a.stamps[PCT_ST_SWEEP_END]);
    if (blockIdx.x == 0) {
        if (lane == 0 && a.flag_next) *a.flag_next = 0;
        if (a.stat_dst && lane < 8) ((unsigned long long*)a.stat_dst)[lane] = ((const unsigned long long*)a.stat_src)[lane];
    }
    const int64_t row0 = (a.blocks_per_xcd ? (int64_t)(blockIdx.x & 7u) * a.blocks_per_xcd + (blockIdx.x >> 3) : (int64_t)blockIdx.x) * kFitBlock;
    if (row0 >= a.rows) return;
    const int k = a.k, kp = a.kp;

    // ---- stage 64 index rows: 16 lanes x int4 per row, 4 rows per load instruction, all loads independent
    // (rows are 16-byte aligned: pitch is a multiple of 4) -------------------------------------------------
    const int nrow = (int)min((int64_t)kFitBlock, a.rows - row0);
    if constexpr (STAGED) {
        const int sub = lane >> 4, c4 = (lane & 15) << 2;
        // Every load of a 64-column chunk is issued before the first store: a lane outside the tile reads the tile's
        // last row or the row's last int4 instead (inside the table, never stored), so no load sits behind a branch --
        // with the loads under the row and column tests each one was waited for before the next was issued, sixteen
        // memory latencies in a row per block.
        for (int cb = 0; cb < k; cb += 64) {
            const int c = cb + c4;
            const int cl = min(c, a.pitch - 4);
            int4 v[kFitBlock / 4];
#pragma unroll
            for (int i = 0; i < kFitBlock / 4; ++i)
                v[i] = *(const int4*)(a.table + (row0 + min(i * 4 + sub, nrow - 1)) * a.pitch + cl);
#pragma unroll
            for (int i = 0; i < kFitBlock / 4; ++i) {
                const int r = i * 4 + sub;
                if (r < nrow && c < a.pitch) {
                    int* dst = s_idx + r * kp + c;
                    if (c + 0 < k) dst[0] = v[i].x;
                    if (c + 1 < k) dst[1] = v[i].y;
                    if (c + 2 < k) dst[2] = v[i].z;
                    if (c + 3 < k) dst[3] = v[i].w;
                }
            }
        }
    }
    __syncthreads();

    const int64_t row = row0 + lane;
    if (row >= a.rows) return;
    if constexpr (MASKED) {
        if (!a.row_mask[row]) return;
    }
    const int64_t qid = a.row_query32 ? (int64_t)a.row_query32[row] : a.row_query ? a.row_query[row] : row + a.row_offset;
    const float4 qp = a.pts[qid];
    const int pub = __float_as_int(qp.w);
    if (!a.out_by_row && (pub < a.q_begin || pub >= a.q_end)) return;
    const int64_t out = a.out_by_row ? row : (int64_t)pub - a.out_base;

    double qx = qp.x, qy = qp.y, qz = qp.z;
    if (F64) {
        const double4 qd = a.ptsd[qid];
        qx = qd.x; qy = qd.y; qz = qd.z;
    }
    const int m = a.cnt ? a.cnt[row] : k;
    const int* my = STAGED ? s_idx + lane * kp : a.table + row * a.pitch;
    const float nanf_ = __int_as_float(0x7fc00000);

    const auto store_nan = [&]() {      // rows without an answer here: fewer than six neighbours, an entry outside the cloud
        if constexpr (OUT64) {
            for (int j = 0; j < 6; ++j) a.coefs64[out * 6 + j] = (double)nanf_;
            a.K64[out] = (double)nanf_; a.H64[out] = (double)nanf_;
        } else {
            for (int j = 0; j < 6; ++j) a.coefs[out * 6 + j] = nanf_;
            a.K[out] = nanf_; a.H[out] = nanf_; a.H2[out] = nanf_;
        }
    };
    // rows this kernel does not finish go to k_fit_svd: one counter increment per wave
    const auto hand_over = [&]() {
        const unsigned long long fm = __ballot(1);                  // the lanes that are here together
        const int leader = (int)__builtin_ctzll(fm);
        int base = 0;
        if (lane == leader) base = atomicAdd(a.flag_count, (int)__popcll(fm));
        base = __shfl(base, leader);
        a.flag_list[base + (int)__popcll(fm & ((1ull << lane) - 1ull))] = (int)row;
    };
    if (m < 6) {   // under-determined quadric (eps bound, neighbour study): lstsq's minimum-norm answer, k_fit_svd
        store_nan();
        if (m >= 2) hand_over();       // (np.cov of fewer than two points is NaN in the reference as well)
        return;
    }

    // ---- pass 1: moments of the centred neighbourhood ---------------------
    double sx = 0, sy = 0, sz = 0, sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
    double fx = 0, fy = 0, fz = 0, lx = 0, ly = 0, lz = 0;
    // gathers are issued kFitAhead neighbours ahead of their use (the row walk is latency-bound otherwise)
    // The moments are taken about the FIRST neighbour, not about the query: the covariance does not care, and a query far
    // from its neighbourhood (caller-supplied rows with a foreign query, far outliers) no longer costs sxx - sx * mx its
    // digits -- about the query, 1 000 neighbourhood radii away, the rotation moved by 1e-10, enough to round the
    // float32 design rows differently from np.cov's (centred) rotation and to miss the contract in H 50- to 1 000-fold.
#define PASS1_ACC(x, y, z)                                                          \
    do {                                                                            \
        const double dx = x - fx, dy = y - fy, dz = z - fz;                         \
        sx += dx; sy += dy; sz += dz;                                               \
        sxx = fma(dx, dx, sxx); sxy = fma(dx, dy, sxy); sxz = fma(dx, dz, sxz);     \
        syy = fma(dy, dy, syy); syz = fma(dy, dz, syz); szz = fma(dz, dz, szz);     \
    } while (0)
    // A table entry that is not a record of the cloud (host-supplied rows are validated before they get here, the
    // sweep's rows are the sweep's responsibility: this is the last line of defence) is clamped, never dereferenced,
    // and the row reads NaN.
    bool bad_id = false;
    const auto checked = [&](int id) {
        bad_id |= (unsigned)id >= a.n_pts;
        return (int)min((unsigned)id, a.n_pts - 1u);
    };
    {
        int j = 0;
        for (; j + kFitAhead <= m; j += kFitAhead) {
            double x[kFitAhead], y[kFitAhead], z[kFitAhead];
#pragma unroll
            for (int u = 0; u < kFitAhead; ++u) load_centred<F64>(a, checked(my[j + u]), qx, qy, qz, qp.x, qp.y, qp.z, x[u], y[u], z[u]);
            if (j == 0) { fx = x[0]; fy = y[0]; fz = z[0]; }
#pragma unroll
            for (int u = 0; u < kFitAhead; ++u) PASS1_ACC(x[u], y[u], z[u]);
            lx = x[kFitAhead - 1]; ly = y[kFitAhead - 1]; lz = z[kFitAhead - 1];
        }
        for (; j < m; ++j) {
            double x, y, z;
            load_centred<F64>(a, checked(my[j]), qx, qy, qz, qp.x, qp.y, qp.z, x, y, z);
            if (j == 0) { fx = x; fy = y; fz = z; }
            PASS1_ACC(x, y, z);
            lx = x; ly = y; lz = z;
        }
    }
#undef PASS1_ACC
    if (bad_id) {
        store_nan();
        return;
    }
    double rot[9];
    plane_rotation<F64>(m, sx, sy, sz, sxx, sxy, sxz, syy, syz, szz, fx, fy, fz, lx, ly, lz, a.force_jacobi != 0, rot);
    const double r00 = rot[0], r01 = rot[1], r02 = rot[2], r10 = rot[3], r11 = rot[4], r12 = rot[5], r20 = rot[6], r21 = rot[7], r22 = rot[8];

    // ---- pass 2: float32 design rows -> scaled fp64 normal equations --------
    // No column scaling: scaling the Gram matrix by powers of two commutes with every rounding of an unpivoted
    // Cholesky solve, so it cannot change a single bit of the result (only the overflow/underflow range, which fp64
    // covers down to neighbourhood radii of ~1e-70).
    double g[21];
    double b[6];
#pragma unroll
    for (int i = 0; i < 21; ++i) g[i] = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) b[i] = 0;
#define PASS2_ACC(x, y, z)                                                          \
    do {                                                                            \
        const float pa = (float)((r00 * x + r01 * y) + r02 * z);                    \
        const float pb = (float)((r10 * x + r11 * y) + r12 * z);                    \
        const float pz = (float)((r20 * x + r21 * y) + r22 * z);                    \
        double c[6];                                                                \
        c[0] = (double)(pa * pa);                                                   \
        c[1] = (double)(pb * pb);                                                   \
        c[2] = (double)(pa * pb);                                                   \
        c[3] = (double)pa;                                                          \
        c[4] = (double)pb;                                                          \
        c[5] = 1.0;                                                                 \
        const double zz = (double)pz;                                               \
        int t = 0;                                                                  \
        _Pragma("unroll") for (int i = 0; i < 6; ++i) {                             \
            _Pragma("unroll") for (int jj = 0; jj <= i; ++jj) { g[t] = fma(c[i], c[jj], g[t]); ++t; } \
            b[i] = fma(c[i], zz, b[i]);                                             \
        }                                                                           \
    } while (0)
    {
        int j = 0;
        for (; j + kFitAhead <= m; j += kFitAhead) {
            double x[kFitAhead], y[kFitAhead], z[kFitAhead];
#pragma unroll
            for (int u = 0; u < kFitAhead; ++u) load_centred<F64>(a, my[j + u], qx, qy, qz, qp.x, qp.y, qp.z, x[u], y[u], z[u]);
#pragma unroll
            for (int u = 0; u < kFitAhead; ++u) PASS2_ACC(x[u], y[u], z[u]);
        }
        for (; j < m; ++j) {
            double x, y, z;
            load_centred<F64>(a, my[j], qx, qy, qz, qp.x, qp.y, qp.z, x, y, z);
            PASS2_ACC(x, y, z);
        }
    }
#undef PASS2_ACC

    // ---- Cholesky  G = L L^T  (lower triangle packed row-wise), solve -------
    // packed index of (i,j), j<=i : i*(i+1)/2 + j
#define GI(i, j) ((i) * ((i) + 1) / 2 + (j))
    double dinv[6];                 // 1 / L_jj
    bool well = true;               // every pivot ratio d_j / g_jj above kPivotRatioMin: the columns are far from dependent
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = g[GI(j, j)];
#pragma unroll
        for (int p = 0; p < j; ++p) d -= g[GI(j, p)] * g[GI(j, p)];
        well = well && d > kPivotRatioMin * g[GI(j, j)];               // (false for NaN and for an all-zero column too)
        const double inv = rsqrt(d);                    // NaN for a non-positive pivot: such rows are handed over
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
    for (int i = 0; i < 6; ++i) {   // L y = b
        double s = b[i];
#pragma unroll
        for (int p = 0; p < i; ++p) s -= g[GI(i, p)] * b[p];
        b[i] = s * dinv[i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {  // L^T x = y
        double s = b[i];
#pragma unroll
        for (int p = i + 1; p < 6; ++p) s -= g[GI(p, i)] * b[p];
        b[i] = s * dinv[i];
    }
#undef GI
    // An ill-conditioned design matrix (neighbours on a line or a planar curve, anisotropic lattices, duplicates): the
    // reference's lstsq (pct:359) is LAPACK gelsd -- an SVD-based solve with the singular values below
    // eps * max(m, 6) * sigma_1 cut off -- whose answer the normal equations cannot follow.  k_fit_svd redoes the row.
    if (!well) hand_over();
    if constexpr (OUT64) {
        // diagnostics: what the float32 rounding of the coefficients (pct:359) and the float32 curvature arithmetic
        // (pct:403-422) cost -- the solution as solved, and the same formulas in float64
        double* co64 = a.coefs64 + out * 6;
        for (int j = 0; j < 6; ++j) co64[j] = b[j];
        const double Fx = b[3], Fy = b[4], Fxx = 2.0 * b[0], Fyy = 2.0 * b[1], Fxy = b[2];
        const double wgt = (1.0 + Fx * Fx) + Fy * Fy;
        a.K64[out] = (Fxx * Fyy - Fxy * Fxy) / (wgt * wgt);
        a.H64[out] = (((1.0 + Fx * Fx) * Fyy - ((2.0 * Fx) * Fy) * Fxy) + (1.0 + Fy * Fy) * Fxx) / (2.0 * (wgt * sqrt(wgt)));
        return;
    }
    const float A = (float)b[0], B = (float)b[1], C = (float)b[2];
    const float D = (float)b[3], E = (float)b[4], F = (float)b[5];
    float* co = a.coefs + out * 6;
    co[0] = A; co[1] = B; co[2] = C; co[3] = D; co[4] = E; co[5] = F;

    float Kg, Kh;
    monge_curvatures(A, B, C, D, E, Kg, Kh);
    a.K[out] = Kg;
    a.H[out] = Kh;
    a.H2[out] = Kh * Kh;
}

// calculate_explicit_quadratic_curvatures alone (pct:398-431), one thread per row
__global__ __launch_bounds__(256) void k_curv(const float* __restrict__ coefs, int64_t rows, float* __restrict__ K,
                                              float* __restrict__ H, float* __restrict__ H2) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const float* c = coefs + r * 6;
    float Kg, Kh;
    monge_curvatures(c[0], c[1], c[2], c[3], c[4], Kg, Kh);
    K[r] = Kg;
    H[r] = Kh;
    H2[r] = Kh * Kh;
}

template <bool F64, bool OUT64>
__global__ __launch_bounds__(64) void k_fit_svd(FitArgs a, const int* __restrict__ list, const int* __restrict__ list_count,
                                                long long* __restrict__ host_count) {
    fit_svd_rows<F64, OUT64>(a, TableRows{}, list, list_count, host_count);
    // behind the rows redone here: fit_ms covers them.  (The row count block 0 has sent to the host is stored again by the
    // block that ends the call, in front of the end stamp: a host that sees the stamp reads this call's count.)
    pct_stamp_last_out(a.stamps, a.stamps_pin, a.stamp_ticket, host_count, (long long)*list_count);
}

// ---------------------------------------------------------------------------
// The two per-neighbourhood staticmethods of the class surface on their own ("methods of rows A1-A10"),
// batched: one thread per neighbourhood of m points.
//   k_plane_rotate   get_best_fit_plane_and_rotate (pct:270-321): np.cov (mean first, then centred products, float64,
//                    ddof = 1) -> normal -> flip by points[-1] - points[0] (native dtype) -> Rodrigues -> R p, float64
//   k_quadric_rows   fit_quadratic_surface (pct:331-360): float32 points -> lstsq (gelsd semantics) -> float32 (6,)
// ---------------------------------------------------------------------------
template <bool F64>
__global__ __launch_bounds__(64) void k_plane_rotate(const void* __restrict__ nbrs, int64_t batch, int m, int force_jacobi,
                                                     double* __restrict__ out) {
    const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= batch) return;
    const auto at = [&](int j, double& x, double& y, double& z) {
        if (F64) { const double* p = (const double*)nbrs + (b * m + j) * 3; x = p[0]; y = p[1]; z = p[2]; }
        else { const float* p = (const float*)nbrs + (b * m + j) * 3; x = (double)p[0]; y = (double)p[1]; z = (double)p[2]; }
    };
    double mx = 0, my = 0, mz = 0;
    for (int j = 0; j < m; ++j) { double x, y, z; at(j, x, y, z); mx += x; my += y; mz += z; }
    mx /= (double)m; my /= (double)m; mz /= (double)m;
    double sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
    for (int j = 0; j < m; ++j) {
        double x, y, z;
        at(j, x, y, z);
        x -= mx; y -= my; z -= mz;
        sxx = fma(x, x, sxx); sxy = fma(x, y, sxy); sxz = fma(x, z, sxz);
        syy = fma(y, y, syy); syz = fma(y, z, syz); szz = fma(z, z, szz);
    }
    double fx, fy, fz, lx, ly, lz;
    at(0, fx, fy, fz);
    at(m - 1, lx, ly, lz);
    double rot[9];
    plane_rotation<F64>(m, 0.0, 0.0, 0.0, sxx, sxy, sxz, syy, syz, szz, fx, fy, fz, lx, ly, lz, force_jacobi != 0, rot);
    for (int j = 0; j < m; ++j) {
        double x, y, z;
        at(j, x, y, z);
        double* o = out + (b * m + j) * 3;
        o[0] = (rot[0] * x + rot[1] * y) + rot[2] * z;
        o[1] = (rot[3] * x + rot[4] * y) + rot[5] * z;
        o[2] = (rot[6] * x + rot[7] * y) + rot[8] * z;
    }
}

__global__ __launch_bounds__(64) void k_quadric_rows(const float* __restrict__ pts, int64_t batch, int m, float* __restrict__ coefs) {
    const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= batch) return;
    Lstsq6 ls;
    ls.init();
#pragma unroll 1
    for (int j = 0; j < m; ++j) {
        const float* p = pts + (b * m + j) * 3;
        ls.add(p[0], p[1], p[2]);
    }
    double sol[6];
    ls.solve(m, sol);
    for (int j = 0; j < 6; ++j) coefs[b * 6 + j] = (float)sol[j];
}

// explicit_quadratic_neighbor_study (pct:756-761): row (s, n) = the sample point itself followed by its n nearest
// neighbours, n = n_lo .. n_hi, taken from the resident neighbour table
__global__ __launch_bounds__(256) void k_prefix_rows(const int* __restrict__ sample_row, const int* __restrict__ owned_pos,
                                                     int q_begin, int64_t n_samples, int n_lo, int n_hi,
                                                     const int* __restrict__ nbr_pos, int nbr_pitch,
                                                     int* __restrict__ table, int pitch, int* __restrict__ cnt,
                                                     int64_t* __restrict__ row_query) {
    const int nn = n_hi - n_lo + 1;
    const int64_t row = blockIdx.x;
    if (row >= n_samples * nn) return;
    const int64_t s = row / nn;
    const int n = n_lo + (int)(row - s * nn);
    const int trow = sample_row[s];                                       // neighbour-table row of the sample
    const int q = owned_pos ? owned_pos[trow] : trow + q_begin;           // its id in the point array the table refers to
    int* dst = table + row * pitch;
    for (int j = threadIdx.x; j <= n; j += 256) dst[j] = j == 0 ? q : nbr_pos[(int64_t)trow * nbr_pitch + (j - 1)];
    if (threadIdx.x == 0) { cnt[row] = n + 1; row_query[row] = q; }
}

// k_fit and the k_fit_svd behind it, for one cloud dtype and one output width.  The masked kernel exists for float32 outputs
// only (launch() has refused a masked fit with float64 outputs or rows too long to stage).
template <bool F64, bool OUT64>
int launch_kernels(pct_ctx* ctx, const FitArgs& a, bool staged, int blocks, size_t lds, long long* note) {
    const dim3 grid(blocks), block(kFitBlock);
    if (!OUT64 && a.row_mask && staged) PCT_LAUNCH_T((k_fit<F64, false, true, true>), grid, block, lds, ctx->stream, a);
    else if (staged) PCT_LAUNCH_T((k_fit<F64, OUT64, true>), grid, block, lds, ctx->stream, a);
    else PCT_LAUNCH_T((k_fit<F64, OUT64, false>), grid, block, 0, ctx->stream, a);
    PCT_HIP(ctx, hipGetLastError());
    // the rows handed over: fixed grid, the list length is read on the device
    const int sblocks = blocks < 1024 ? blocks : 1024;
    PCT_LAUNCH_T((k_fit_svd<F64, OUT64>), dim3(sblocks), dim3(64), 0, ctx->stream, a, a.flag_list, a.flag_count, note);
    PCT_HIP(ctx, hipGetLastError());
    return PCT_OK;
}

// slot: the pinned slots of the call (FitSlot); *mirrored (may be null): the fit kernel mirrors the statistics words
int launch(pct_ctx* ctx, const FitArgs& a0, bool f64, FitSlot slot, bool* mirrored) {
    FitArgs a = a0;
    a.kp = a.k | 1;
    if (a.row_mask && ((size_t)kFitBlock * a.kp * sizeof(int) > 64 * 1024 || a.coefs64))
        return pct_fail(ctx, PCT_ERR_INVALID, "masked fit: rows too long");       // (k <= 127 on this path)
    size_t lds = (size_t)kFitBlock * a.kp * sizeof(int);
    const bool staged = lds <= 64 * 1024;                  // the default dynamic LDS limit of a launch
    if (!staged) lds = 0;
    int blocks = (int)((a.rows + kFitBlock - 1) / kFitBlock);
    if (blocks <= 0) return PCT_OK;
    a.blocks_per_xcd = pct_getenv("PCT_NO_XCD_MAP") ? 0 : (blocks + 7) / 8;
    a.force_jacobi = fit_jacobi_forced();
    if (a.blocks_per_xcd) blocks = a.blocks_per_xcd * 8;
    // rows for k_fit_svd: list + its length (first word of the buffer's 64-byte head)
    // two counts used in turn: a launch counts in one and clears the other for the launch after it (both cleared once per
    // allocation) -- the 64-byte memset in front of every fit was a launch of its own, 4 us and a dispatch gap
    PCT_TRY(pct_reserve(ctx, &ctx->fit_flag, 64 + (size_t)a.rows * sizeof(int)));
    if (ctx->fit_flag.p != ctx->fit_flag_seen || ctx->fit_flag.cap != ctx->fit_flag_cap_seen) {
        PCT_HIP(ctx, hipMemsetAsync(ctx->fit_flag.p, 0, 64, ctx->stream));
        ctx->fit_flag_seen = ctx->fit_flag.p;
        ctx->fit_flag_cap_seen = ctx->fit_flag.cap;
        ctx->fit_parity = 0;
    }
    a.stat_src = nullptr;
    a.stat_dst = nullptr;
    if (slot.mirror_stats && ctx->counters.p) {
        a.stat_src = &pct_dev(ctx)->sweep;
        a.stat_dst = &ctx->pin->stats[slot.par];
        if (mirrored) *mirrored = true;
    }
    if (slot.clock) slot.clock->end_words(&a.stamps, &a.stamps_pin, &a.stamp_ticket);
    a.flag_count = (int*)ctx->fit_flag.p + ctx->fit_parity;
    a.flag_next = (int*)ctx->fit_flag.p + (ctx->fit_parity ^ 1);
    ctx->fit_parity ^= 1;
    a.flag_list = (int*)ctx->fit_flag.p + 16;
    long long* note = &ctx->pin->svd_rows[slot.par];
    if (a.coefs64) return f64 ? launch_kernels<true, true>(ctx, a, staged, blocks, lds, note) : launch_kernels<false, true>(ctx, a, staged, blocks, lds, note);
    return f64 ? launch_kernels<true, false>(ctx, a, staged, blocks, lds, note) : launch_kernels<false, false>(ctx, a, staged, blocks, lds, note);
}

// What the two fits of the resident table share: the handle's result buffers for the owned range, the table's own counts
// and the owned public range.
int table_args(pct_ctx* ctx, FitSpace space, FitArgs* a) {
    PCT_TRY(pct_reserve_fit(ctx, ctx->q_end - ctx->q_begin));
    PCT_TRY(fit_source(ctx, space, a));
    a->table = (const int*)ctx->nbr_pos.p;
    a->cnt = ctx->eps > 0 ? (const int*)ctx->nbr_cnt.p : nullptr;
    a->k = ctx->k;
    a->out_base = ctx->q_begin;
    a->q_begin = (int)ctx->q_begin;
    a->q_end = (int)ctx->q_end;
    a->coefs = (float*)ctx->coefs.p;
    a->K = (float*)ctx->K.p;
    a->H = (float*)ctx->H.p;
    a->H2 = (float*)ctx->H2.p;
    return PCT_OK;
}

}  // namespace

// one pass of the density-adaptive sweep (pct_levels.hip): the rows it answered (row_done), fitted while its table is
// still in ITS cell order -- gathers stay local; results go to public order.  The merged public-space table is fitted
// only when a caller asks for the table first and the fit later (1.3 ms instead of 0.25 at 1 M points).
int pct_launch_fit_pass(pct_ctx* ctx, int64_t rows, int par) {
    FitArgs a = {};
    PCT_TRY(table_args(ctx, FitSpace::Sorted, &a));
    a.row_query32 = (const int*)ctx->owned_pos.p;
    a.rows = rows;
    a.pitch = (ctx->k + 3) & ~3;
    a.out_by_row = 0;
    a.row_mask = (const int*)ctx->row_done.p;
    a.svd_accumulate = 1;                      // (pct_knn_levels zeroes the host word before the first pass)
    return launch(ctx, a, ctx->has_f64, FitSlot{par, false}, nullptr);      // (a pass mirrors nothing: the sweep goes on behind it)
}

// fit from the device-resident neighbour table left by the sweep
int pct_launch_fit_table(pct_ctx* ctx, FitSlot slot, bool* mirrored, bool* by_row) {
    FitArgs a = {};
    const bool sorted = ctx->knn_sorted_space;
    PCT_TRY(table_args(ctx, sorted ? FitSpace::Sorted : FitSpace::Packed, &a));
    a.row_query32 = sorted ? (const int*)ctx->owned_pos.p : nullptr;    // table row -> sorted position of its query
    a.row_offset = sorted ? 0 : ctx->q_begin;                           // exhaustive sweep: row = public index - q_begin
    a.rows = ctx->q_end - ctx->q_begin;
    a.pitch = ctx->nbr_pitch;
    // Grid sweep: results stay in TABLE-ROW (cell) order -- a wave's 64 rows are consecutive, so the stores
    // coalesce; written in public order they were 36 B scattered per point and cost 4x the bytes at the HBM
    // (WRITE_SIZE 145 MB vs 36 MB).  pct_get_fit gathers public rows on request (pct_rows.hip).
    a.out_by_row = sorted ? 1 : 0;
    *by_row = sorted;
    return launch(ctx, a, ctx->has_f64, slot, mirrored);
}

// Fit from explicit neighbour rows, outputs row-aligned: the one body of the three entries below.  The query of a row is
// d_query32[row], else d_query[row], else the row's own number; the results are the float32 four or the float64 three.
// (rows with fewer than 6 points get lstsq's minimum-norm answer from k_fit_svd, as in every launch)
static int fit_rows(pct_ctx* ctx, FitSpace space, const int32_t* d_idx, const int32_t* d_cnt, const int64_t* d_query,
                    const int32_t* d_query32, int64_t rows, int32_t k, int32_t pitch, float* d_coefs, float* d_K, float* d_H,
                    float* d_H2, double* d_coefs64, double* d_K64, double* d_H64) {
    FitArgs a = {};
    PCT_TRY(fit_source(ctx, space, &a));
    a.table = d_idx;
    a.cnt = d_cnt;
    a.row_query = d_query;
    a.row_query32 = d_query32;
    a.rows = rows;
    a.k = k;
    a.pitch = pitch;
    a.out_by_row = 1;
    a.q_begin = 0;
    a.q_end = (int)ctx->n;
    a.coefs = d_coefs;
    a.K = d_K;
    a.H = d_H;
    a.H2 = d_H2;
    a.coefs64 = d_coefs64;
    a.K64 = d_K64;
    a.H64 = d_H64;
    return launch(ctx, a, ctx->has_f64, FitSlot{0, false}, nullptr);       // (a blocking entry point: slot 0, no fused tail behind it)
}

// sorted_space: ids refer to the cell-sorted arrays, else to the packed ones
int pct_launch_fit_rows(pct_ctx* ctx, const int32_t* d_idx, const int32_t* d_cnt, const int64_t* d_query,
                        int64_t rows, int32_t k, int32_t pitch, float* d_coefs, float* d_K, float* d_H, float* d_H2,
                        bool sorted_space) {
    return fit_rows(ctx, sorted_space ? FitSpace::Sorted : FitSpace::Packed, d_idx, d_cnt, d_query, nullptr, rows, k, pitch,
                    d_coefs, d_K, d_H, d_H2, nullptr, nullptr, nullptr);
}

// the same for rows built on the device (pct_fit_ball.hip): public-space ids into the plain records, int32 query ids
int pct_launch_fit_rows32(pct_ctx* ctx, const int32_t* d_idx, const int32_t* d_cnt, const int32_t* d_query32, int64_t rows,
                          int32_t k, int32_t pitch, float* d_coefs, float* d_K, float* d_H, float* d_H2) {
    return fit_rows(ctx, FitSpace::Public, d_idx, d_cnt, nullptr, d_query32, rows, k, pitch, d_coefs, d_K, d_H, d_H2, nullptr,
                    nullptr, nullptr);
}

// the diagnostics variant of pct_launch_fit_rows: float64 coefficients and curvatures, public-space ids
int pct_launch_fit_rows_f64(pct_ctx* ctx, const int32_t* d_idx, const int32_t* d_cnt, const int64_t* d_query, int64_t rows,
                            int32_t k, int32_t pitch, double* d_coefs, double* d_K, double* d_H) {
    return fit_rows(ctx, FitSpace::Public, d_idx, d_cnt, d_query, nullptr, rows, k, pitch, nullptr, nullptr, nullptr, nullptr,
                    d_coefs, d_K, d_H);
}

int pct_launch_prefix_rows(pct_ctx* ctx, const int* d_sample_row, int64_t n_samples, int n_lo, int n_hi, int* d_table,
                           int pitch, int* d_cnt, int64_t* d_row_query) {
    const int64_t rows = n_samples * (n_hi - n_lo + 1);
    PCT_LAUNCH(k_prefix_rows, dim3((unsigned)rows), dim3(256), 0, ctx->stream, d_sample_row,
                       ctx->knn_sorted_space ? (const int*)ctx->owned_pos.p : nullptr, (int)ctx->q_begin, n_samples, n_lo, n_hi,
                       (const int*)ctx->nbr_pos.p, ctx->nbr_pitch, d_table, pitch, d_cnt, d_row_query);
    PCT_HIP(ctx, hipGetLastError());
    return PCT_OK;
}

int pct_launch_curvatures(pct_ctx* ctx, const float* d_coefs, int64_t rows, float* d_K, float* d_H, float* d_H2) {
    const int blocks = (int)((rows + 255) / 256);
    if (blocks <= 0) return PCT_OK;
    PCT_LAUNCH(k_curv, dim3(blocks), dim3(256), 0, ctx->stream, d_coefs, rows, d_K, d_H, d_H2);
    PCT_HIP(ctx, hipGetLastError());
    return PCT_OK;
}

int pct_launch_plane_rotate(pct_ctx* ctx, const void* d_nbrs, bool f64, int64_t batch, int32_t m, double* d_out) {
    const unsigned blocks = (unsigned)((batch + 63) / 64);
    const int jacobi = fit_jacobi_forced();
    if (f64)
        PCT_LAUNCH(k_plane_rotate<true>, dim3(blocks), dim3(64), 0, ctx->stream, d_nbrs, batch, m, jacobi, d_out);
    else
        PCT_LAUNCH(k_plane_rotate<false>, dim3(blocks), dim3(64), 0, ctx->stream, d_nbrs, batch, m, jacobi, d_out);
    PCT_HIP(ctx, hipGetLastError());
    return PCT_OK;
}

int pct_launch_quadric_rows(pct_ctx* ctx, const float* d_pts, int64_t batch, int32_t m, float* d_coefs) {
    PCT_LAUNCH(k_quadric_rows, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, ctx->stream, d_pts, batch, m, d_coefs);
    PCT_HIP(ctx, hipGetLastError());
    return PCT_OK;
}

// What the fit kernels share (pct_fit.hip: k_fit, k_fit_svd and the batched staticmethods; pct_fit_ball.hip: the fit of
// CSR rows): the launch arguments and the two host helpers that fill them, the tangent-plane stage, the curvature formulas
// and the gelsd-semantics solver.
// Everything is internal to the translation unit that includes it (anonymous namespace), exactly as when it lived in
// pct_fit.hip: the move changed no token of these functions, and k_fit compiles to the same code.
#pragma once
#include "pct_internal.h"

#include <math.h>

namespace {

struct FitArgs {
    const float4* pts;       // records {x,y,z,public index}
    const double4* ptsd;     // native fp64 coordinates (nullable), same order
    const int* table;        // (rows,k) neighbour ids into pts (-1 = missing)
    const int* cnt;          // (rows) valid neighbours per row (nullable -> k)
    const int64_t* row_query;// (rows) query id into pts per row (nullable -> row + row_offset)
    const int* row_query32;  // the same as int32 (device-built lists); takes precedence
    int64_t row_offset;
    int64_t rows;
    int k;
    int pitch;               // table row pitch in elements, multiple of 4
    int kp;                  // LDS row pitch (odd)
    int out_by_row;          // 1: outputs indexed by row; 0: by public index of the query
    int64_t out_base;        // subtracted from the public index when out_by_row == 0
    int q_begin, q_end;      // owned public range (rows outside are skipped)
    float* coefs;
    float* K;
    float* H;
    float* H2;
    double* coefs64;         // diagnostics variant (OUT64): unrounded coefficients and float64 curvatures, row-aligned
    double* K64;
    double* H64;
    int* flag_list;          // rows k_fit hands to k_fit_svd (ill-conditioned or under-determined design matrices)
    int* flag_count;
    int* flag_next;          // the count the NEXT launch will use: zeroed by this launch's first block (saves a memset launch)
    const pct_sweep_words* stat_src;      // fused call: the sweep's statistics, eight 64-bit words ...
    pct_sweep_words* stat_dst;            // ... copied to pinned host memory by the first block (saves a D2H copy)
    unsigned n_pts;          // records in pts: a table entry outside [0, n_pts) is never dereferenced (the row reads NaN)
    const int* row_mask;     // MASKED instantiation: only the rows with a non-zero entry are fitted (passes of the density-adaptive sweep)
    int svd_accumulate;      // the count of rows handed to k_fit_svd is ADDED to the host word (the passes of one fused call)
    int force_jacobi;        // PCT_FIT_JACOBI=1: every row's normal through the cyclic Jacobi (A/B runs, route-against-route tests)
    // a call timed by the device clock (pct_stamp.h), else null: the call's device stamps -- k_fit stamps the end of the
    // sweep at its entry --, and their pinned mirror and the ticket k_fit_svd's last block out ends the call with
    unsigned long long* stamps;
    unsigned long long* stamps_pin;
    unsigned* stamp_ticket;  // ctx->stamp_tickets
    int blocks_per_xcd;      // blocks are dealt to the 8 XCDs in turn: block b takes rows of block (b % 8) * blocks_per_xcd + b / 8, so
                             // that one XCD's L2 serves neighbouring rows (table rows are in cell order: their neighbours overlap)
};

// The three orders of the cloud's records that the neighbour ids of a fit refer to: the cell-sorted records (ctx->sorted4 /
// sorted4d, n_grid of them), the packed ones (pts4 / pts4d, n) and the public-order records (qpts4 / pts4d, n).
enum class FitSpace { Sorted, Packed, Public };

// pts, ptsd and n_pts of a launch: set here together, and nowhere else
int fit_source(pct_ctx* ctx, FitSpace space, FitArgs* a) {
    if (space == FitSpace::Public) PCT_TRY(pct_ensure_plain_records(ctx));
    const bool sorted = space == FitSpace::Sorted;
    a->pts = (const float4*)(sorted ? ctx->sorted4.p : space == FitSpace::Packed ? ctx->pts4.p : ctx->qpts4.p);
    a->ptsd = ctx->has_f64 ? (const double4*)(sorted ? ctx->sorted4d.p : ctx->pts4d.p) : nullptr;
    a->n_pts = (unsigned)(sorted ? ctx->n_grid : ctx->n);
    return PCT_OK;
}

// PCT_FIT_JACOBI=1 (read per call): the normal of every row through the cyclic Jacobi, the route before direct_normal()
int fit_jacobi_forced() {
    const char* e = pct_getenv("PCT_FIT_JACOBI");
    return e && e[0] == '1' ? 1 : 0;
}

// Smallest Cholesky pivot ratio d_j / g_jj (= sin^2 of the angle between design column j and the span of the columns
// before it; invariant under column scaling) below which the normal equations are not trusted.  Their error grows like
// eps / ratio: measured against LAPACK's gelsd on anisotropic lattices (tools notes in DESIGN 4.3), ratios >= 1e-9 stay
// at float32 rounding noise (<= 2.4e-7 relative in K, H), [1e-10, 1e-9) reach 1.3e-5.  1e-6 leaves three decades.
constexpr double kPivotRatioMin = 1e-6;

// One Jacobi rotation annihilating a_pq of a symmetric 3x3 (r = third index).
// With alpha = (a_qq - a_pp)/2 and beta = a_pq the tangent of the rotation is
// t = sgn(alpha) beta / (|alpha| + sqrt(alpha^2 + beta^2))  (the small root), c = 1/sqrt(1+t^2):
// one sqrt, one division and one reciprocal square root per rotation.
#define JACOBI_ROT(app, aqq, apq, arp, arq, vp0, vp1, vp2, vq0, vq1, vq2)          \
    do {                                                                            \
        if (apq != 0.0) {                                                           \
            const double alpha = 0.5 * (aqq - app);                                 \
            const double beta = apq;                                                \
            const double t = (alpha >= 0.0 ? beta : -beta) / (fabs(alpha) + sqrt(alpha * alpha + beta * beta)); \
            const double c = rsqrt(t * t + 1.0);                                    \
            const double s = t * c;                                                 \
            app -= t * apq;                                                         \
            aqq += t * apq;                                                         \
            apq = 0.0;                                                              \
            const double rp = arp, rq = arq;                                        \
            arp = c * rp - s * rq;                                                  \
            arq = s * rp + c * rq;                                                  \
            double a0 = vp0, b0 = vq0; vp0 = c * a0 - s * b0; vq0 = s * a0 + c * b0; \
            double a1 = vp1, b1 = vq1; vp1 = c * a1 - s * b1; vq1 = s * a1 + c * b1; \
            double a2 = vp2, b2 = vq2; vp2 = c * a2 - s * b2; vq2 = s * a2 + c * b2; \
        }                                                                           \
    } while (0)

// K and H of z = A a^2 + B b^2 + C ab + D a + E b + F at the origin, float32
// arithmetic in the reference's operation order (pct:403-419).
__device__ __forceinline__ void monge_curvatures(float A, float B, float C, float D, float E, float& Kg, float& Kh) {
    const float Fx = D, Fy = E;
    const float Fxx = 2.0f * A, Fyy = 2.0f * B, Fxy = C;
    const float fx2 = Fx * Fx, fy2 = Fy * Fy;
    const float wgt = (1.0f + fx2) + fy2;
    const float den_k = wgt * wgt;                                            // (...) ** 2
    const float den_h = (float)((double)wgt * sqrt((double)wgt));            // (...) ** 1.5
    Kg = (Fxx * Fyy - Fxy * Fxy) / den_k;
    Kh = (((1.0f + fx2) * Fyy - ((2.0f * Fx) * Fy) * Fxy) + (1.0f + fy2) * Fxx) / (2.0f * den_h);
}

template <bool F64>
__device__ __forceinline__ void load_centred(const FitArgs& a, int id, double qx, double qy, double qz,
                                             float qxf, float qyf, float qzf, double& x, double& y, double& z) {
    if (F64) {
        const double4 p = a.ptsd[id];
        x = p.x - qx; y = p.y - qy; z = p.z - qz;         // float64 cloud: float64 centring
    } else {
        const float4 p = a.pts[id];
        x = (double)(p.x - qxf);                           // float32 cloud: float32 centring (pct:641)
        y = (double)(p.y - qyf);
        z = (double)(p.z - qzf);
    }
}

// The direct route to the normal: what the cyclic Jacobi is not needed for.  tests/test_eig_direct_route.py states it
// operation for operation on the CPU and holds it to the exact reference; change the two together.
constexpr int kNewtonCap = 6;                        // steps; a torus neighbourhood takes 2, l3 = l2 / 2 takes 6
constexpr double kNewtonTol = 0x1p-14;               // |step| c2 <= kNewtonTol f': the refinement squares what is left
constexpr double kCrossFloor = 1e-4;                 // |largest cross product| >= kCrossFloor trace^2

// The largest (squared norm, the first of equal ones) of the cross products r0 x r1, r0 x r2, r1 x r2 of the rows of a
// symmetric 3x3: for a matrix of rank two, its null vector.  Returns the squared norm.
__device__ __forceinline__ double largest_row_cross(double b00, double b01, double b02, double b11, double b12, double b22,
                                                    double& n0, double& n1, double& n2) {
    n0 = b01 * b12 - b02 * b11; n1 = b02 * b01 - b00 * b12; n2 = b00 * b11 - b01 * b01;          // r0 x r1
    double best = (n0 * n0 + n1 * n1) + n2 * n2;
    {
        const double c0 = b01 * b22 - b02 * b12, c1 = b02 * b02 - b00 * b22, c2 = b00 * b12 - b01 * b02;   // r0 x r2
        const double nn = (c0 * c0 + c1 * c1) + c2 * c2;
        if (nn > best) { n0 = c0; n1 = c1; n2 = c2; best = nn; }
    }
    {
        const double c0 = b11 * b22 - b12 * b12, c1 = b12 * b02 - b01 * b22, c2 = b01 * b12 - b11 * b02;   // r1 x r2
        const double nn = (c0 * c0 + c1 * c1) + c2 * c2;
        if (nn > best) { n0 = c0; n1 = c1; n2 = c2; best = nn; }
    }
    return best;
}

// Unit eigenvector of the smallest eigenvalue of a symmetric positive semi-definite 3x3, without the Jacobi sweeps:
//   the matrix scaled by the exact power of two that brings its trace into [1/2, 1) (the cubic's coefficients are
//   products of three eigenvalues: unscaled, a neighbourhood of radius 1e-70 underflows);
//   l3 = the smallest root of x^3 - c2 x^2 + c1 x - c0 by Newton from 0 (increasing and concave up to l3: monotone from
//   the left, quadratic at a simple root);
//   n = the largest cross product of two rows of A - l3 I;
//   once more with l3 + n^T (A - l3 I) n / n^T n, the Rayleigh quotient of n: the error of the normal becomes
//   eps l1 / gap3 where the cubic alone leaves eps (l1 / gap3)(l1 / l2);  one reciprocal square root.
// false: the row is not healthy -- f' not positive, no converged step within the cap, a cross product below the floor
// (near-equal small eigenvalues, lines, points, non-finite sums) -- and takes the Jacobi.
__device__ __forceinline__ bool direct_normal(double a00, double a01, double a02, double a11, double a12, double a22,
                                              double& n0, double& n1, double& n2) {
    const double tr = (a00 + a11) + a22;
    if (!(tr > 0.0 && tr < (double)INFINITY)) return false;
    int e;
    (void)frexp(tr, &e);
    a00 = ldexp(a00, -e); a01 = ldexp(a01, -e); a02 = ldexp(a02, -e);
    a11 = ldexp(a11, -e); a12 = ldexp(a12, -e); a22 = ldexp(a22, -e);
    const double c2 = (a00 + a11) + a22;
    const double m01 = a00 * a11 - a01 * a01, m02 = a00 * a22 - a02 * a02, m12 = a11 * a22 - a12 * a12;
    const double c1 = (m01 + m02) + m12;
    const double c0 = (a00 * m12 - a01 * (a01 * a22 - a12 * a02)) + a02 * (a01 * a12 - a11 * a02);
    double lam = 0.0;
    bool ok = false;
#pragma unroll 1
    for (int it = 0; it < kNewtonCap; ++it) {
        const double f = ((lam - c2) * lam + c1) * lam - c0;
        const double fp = (3.0 * lam - 2.0 * c2) * lam + c1;
        if (!(fp > 0.0)) break;
        const double step = f / fp;
        lam -= step;
        if (fabs(step) * c2 <= kNewtonTol * fp) { ok = true; break; }
    }
    const double floor2 = (kCrossFloor * (c2 * c2)) * (kCrossFloor * (c2 * c2));
    double nn = largest_row_cross(a00 - lam, a01, a02, a11 - lam, a12, a22 - lam, n0, n1, n2);
    if (!(ok && nn >= floor2)) return false;
    {
        const double b00 = a00 - lam, b11 = a11 - lam, b22 = a22 - lam;
        const double w0 = (b00 * n0 + a01 * n1) + a02 * n2;
        const double w1 = (a01 * n0 + b11 * n1) + a12 * n2;
        const double w2 = (a02 * n0 + a12 * n1) + b22 * n2;
        lam = lam + ((w0 * n0 + w1 * n1) + w2 * n2) / nn;
    }
    nn = largest_row_cross(a00 - lam, a01, a02, a11 - lam, a12, a22 - lam, n0, n1, n2);
    if (!(nn >= floor2)) return false;
    const double inv = rsqrt(nn);
    n0 *= inv; n1 *= inv; n2 *= inv;
    return true;
}

// Tangent-plane rotation from the moment sums of one centred neighbourhood:
// covariance about the neighbour mean with ddof=1 (pct:277), normal = unit
// eigenvector of the smallest eigenvalue (== Vt[-1], pct:283) -- direct_normal()
// on healthy rows, the cyclic Jacobi on the others and on every row when
// force_jacobi is set (PCT_FIT_JACOBI=1) --, sign flip by the far-minus-near
// reference vector (pct:286-297), Rodrigues rotation taking the normal to +z
// (pct:300-312).  rot = {r00,r01,r02, r10,.., r22}.
template <bool F64>
__device__ __forceinline__ void plane_rotation(int m, double sx, double sy, double sz, double sxx, double sxy, double sxz,
                                               double syy, double syz, double szz, double fx, double fy, double fz,
                                               double lx, double ly, double lz, bool force_jacobi, double (&rot)[9]) {
    const double inv_m = 1.0 / (double)m, inv_m1 = 1.0 / (double)(m - 1);
    const double mx = sx * inv_m, my_ = sy * inv_m, mz = sz * inv_m;
    double a00 = (sxx - sx * mx) * inv_m1, a01 = (sxy - sx * my_) * inv_m1, a02 = (sxz - sx * mz) * inv_m1;
    double a11 = (syy - sy * my_) * inv_m1, a12 = (syz - sy * mz) * inv_m1, a22 = (szz - sz * mz) * inv_m1;

    double n0, n1, n2;          // the unit normal, normalised here once and nowhere below
    if (force_jacobi || !direct_normal(a00, a01, a02, a11, a12, a22, n0, n1, n2)) {
        // ---- cyclic Jacobi on the symmetric 3x3 ----------------------------
        double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;   // v[row][col]
#pragma unroll 1
        for (int sweep = 0; sweep < 8; ++sweep) {
            // off-diagonal mass below 1e-22 of the trace: eigenvectors are converged far beyond fp64 round-off
            const double off = fabs(a01) + fabs(a02) + fabs(a12);
            if (off <= 1e-22 * (fabs(a00) + fabs(a11) + fabs(a22))) break;
            JACOBI_ROT(a00, a11, a01, a02, a12, v00, v10, v20, v01, v11, v21);   // (p,q)=(0,1), r=2
            JACOBI_ROT(a00, a22, a02, a01, a12, v00, v10, v20, v02, v12, v22);   // (0,2), r=1
            JACOBI_ROT(a11, a22, a12, a01, a02, v01, v11, v21, v02, v12, v22);   // (1,2), r=0
        }
        if (a00 <= a11 && a00 <= a22) { n0 = v00; n1 = v10; n2 = v20; }
        else if (a11 <= a22)          { n0 = v01; n1 = v11; n2 = v21; }
        else                          { n0 = v02; n1 = v12; n2 = v22; }
        const double nn = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
        n0 = n0 / nn; n1 = n1 / nn; n2 = n2 / nn;
    }

    // ---- orientation: far-minus-near neighbour (pct:286-297) ---------------
    // the sign of n . r with r as subtracted: normalising r changes no sign, r == 0 gives 0 (no flip), NaN compares false
    double rx, ry, rz;
    if (F64) { rx = lx - fx; ry = ly - fy; rz = lz - fz; }
    else     { rx = (double)((float)lx - (float)fx); ry = (double)((float)ly - (float)fy); rz = (double)((float)lz - (float)fz); }
    if ((n0 * rx + n1 * ry) + n2 * rz < 0) { n0 = -n0; n1 = -n1; n2 = -n2; }
    // ---- Rodrigues rotation taking the normal to +z (pct:300-312) -----------
    double r00 = 1, r01 = 0, r02 = 0, r10 = 0, r11 = 1, r12 = 0, r20 = 0, r21 = 0, r22 = 1;
    {
        const double v0 = n1, v1 = -n0;                    // a x (0,0,1)
        const double c = n2;
        const double ss = v0 * v0 + v1 * v1;               // s^2; s != 0 exactly where ss != 0
        if (ss != 0.0) {
            const double f = (1.0 - c) / ss;
            r00 = 1.0 + (-(v1 * v1)) * f;  r01 = (v1 * v0) * f;            r02 = v1;
            r10 = (v0 * v1) * f;           r11 = 1.0 + (-(v0 * v0)) * f;   r12 = -v0;
            r20 = -v1;                     r21 = v0;                       r22 = 1.0 + (-(v1 * v1) + -(v0 * v0)) * f;
        }
    }

    rot[0] = r00; rot[1] = r01; rot[2] = r02; rot[3] = r10; rot[4] = r11; rot[5] = r12; rot[6] = r20; rot[7] = r21; rot[8] = r22;
}

// Streaming least squares on the reference's design rows [a^2, b^2, ab, a, b, 1] (pct:358), gelsd semantics.
struct Lstsq6 {
    double A[6][6];        // A[c][r]: column c of the triangular factor (rows r <= c in use), after solve(): R V
    double y[6];           // Q^T z

    __device__ __forceinline__ void init() {
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            y[c] = 0;
#pragma unroll
            for (int r = 0; r < 6; ++r) A[c][r] = 0;
        }
    }

    // one neighbour: its float32 coordinates in the rotated frame; the row is annihilated into R by six Givens rotations
    __device__ __forceinline__ void add(float pa, float pb, float pc) {
        double x[6] = {(double)(pa * pa), (double)(pb * pb), (double)(pa * pb), (double)pa, (double)pb, 1.0};   // pct:358
        double zi = (double)pc;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const double xr = x[r];
            if (xr != 0.0) {
                const double rr = A[r][r];
                const double h = sqrt(rr * rr + xr * xr);
                const double inv = 1.0 / h;
                const double c = rr * inv, sn = xr * inv;
                A[r][r] = h;
#pragma unroll
                for (int c2 = r + 1; c2 < 6; ++c2) {
                    const double t = A[c2][r];
                    A[c2][r] = c * t + sn * x[c2];
                    x[c2] = c * x[c2] - sn * t;
                }
                const double t = y[r];
                y[r] = c * t + sn * zi;
                zi = c * zi - sn * t;
            }
        }
    }

    // one-sided Jacobi on R (R V = U Sigma), then c = V Sigma^+ U^T y over the singular values above
    // eps * max(m, 6) * sigma_1 (numpy.linalg.lstsq(rcond=None) on float32 input computes in float64: eps = 2^-52)
    __device__ __forceinline__ void solve(int m, double (&sol)[6]) {
        double V[6][6];        // V[c][r]: column c
#pragma unroll
        for (int c = 0; c < 6; ++c)
#pragma unroll
            for (int r = 0; r < 6; ++r) V[c][r] = c == r ? 1.0 : 0.0;
#pragma unroll 1
        for (int sweep = 0; sweep < 40; ++sweep) {
            bool rotated = false;
#pragma unroll
            for (int p = 0; p < 5; ++p) {
#pragma unroll
                for (int q = p + 1; q < 6; ++q) {
                    double al = 0, be = 0, ga = 0;
#pragma unroll
                    for (int r = 0; r < 6; ++r) {
                        al = fma(A[p][r], A[p][r], al);
                        be = fma(A[q][r], A[q][r], be);
                        ga = fma(A[p][r], A[q][r], ga);
                    }
                    if (ga != 0.0 && fabs(ga) > 1e-15 * sqrt(al * be)) {
                        rotated = true;
                        const double zeta = (be - al) / (2.0 * ga);
                        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                        const double c = rsqrt(1.0 + t * t), sn = c * t;
#pragma unroll
                        for (int r = 0; r < 6; ++r) {
                            const double ap = A[p][r], aq = A[q][r];
                            A[p][r] = c * ap - sn * aq;
                            A[q][r] = sn * ap + c * aq;
                            const double vp = V[p][r], vq = V[q][r];
                            V[p][r] = c * vp - sn * vq;
                            V[q][r] = sn * vp + c * vq;
                        }
                    }
                }
            }
            if (!__any(rotated)) break;
        }
        double sig2[6], smax2 = 0;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            double t = 0;
#pragma unroll
            for (int r = 0; r < 6; ++r) t = fma(A[c][r], A[c][r], t);
            sig2[c] = t;
            smax2 = fmax(smax2, t);
        }
        const double rcond = 2.220446049250313e-16 * (double)(m > 6 ? m : 6);
        const double cut = rcond * sqrt(smax2);
#pragma unroll
        for (int r = 0; r < 6; ++r) sol[r] = 0;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            if (sqrt(sig2[c]) > cut) {
                double t = 0;
#pragma unroll
                for (int r = 0; r < 6; ++r) t = fma(A[c][r], y[r], t);
                const double w = t / sig2[c];
#pragma unroll
                for (int r = 0; r < 6; ++r) sol[r] = fma(V[c][r], w, sol[r]);
            }
        }
    }
};

// Row access of fit_svd_rows: where a listed row's entries start, how many there are, which point it is fitted about, and
// whether an entry is skipped and the first / last neighbour are found by key.  TableRows is the rectangular table of
// FitArgs (k_fit_svd); pct_fit_ball.hip has the CSR form.
struct TableRows {
    static constexpr bool kKeyed = false;
    __device__ __forceinline__ int64_t query(const FitArgs& a, int64_t row) const {
        return a.row_query32 ? (int64_t)a.row_query32[row] : a.row_query ? a.row_query[row] : row + a.row_offset;
    }
    __device__ __forceinline__ const int* start(const FitArgs& a, int64_t row) const { return a.table + row * a.pitch; }
    __device__ __forceinline__ int length(const FitArgs& a, int64_t row) const { return a.cnt ? a.cnt[row] : a.k; }
};

// The body of k_fit_svd: one thread per listed row, the list length read on the device.
// Rows::kKeyed (CSR rows): the entry equal to the query id is no member, and the first / last neighbour of the orientation
// (pct:286) are the members with the smallest / largest key (d2, id), d2 = (dx*dx + dy*dy) + dz*dz in fp64 from the float32
// record and the centre (pct_fit_ball's key); the moments are taken about the nearest member.
template <bool F64, bool OUT64, class Rows>
__device__ __forceinline__ void fit_svd_rows(const FitArgs& a, const Rows& rows, const int* __restrict__ list,
                                             const int* __restrict__ list_count, long long* __restrict__ host_count) {
    const int total = *list_count;
    if (blockIdx.x == 0 && threadIdx.x == 0) *host_count = (a.svd_accumulate ? *host_count : 0ll) + total;   // pinned host word: read at the caller's next synchronisation
    const float nanf_ = __int_as_float(0x7fc00000);
    for (int64_t it = (int64_t)blockIdx.x * 64 + threadIdx.x; it < total; it += (int64_t)gridDim.x * 64) {
        const int64_t row = list[it];
        const int64_t qid = rows.query(a, row);
        const float4 qp = a.pts[qid];
        const int64_t out = a.out_by_row ? row : (int64_t)__float_as_int(qp.w) - a.out_base;
        double qx = qp.x, qy = qp.y, qz = qp.z;
        if (F64) { const double4 qd = a.ptsd[qid]; qx = qd.x; qy = qd.y; qz = qd.z; }
        const int len = rows.length(a, row);
        const int* my = rows.start(a, row);
        int m = len;

        // ---- pass 1: moments -> tangent-plane rotation (as k_fit) ----------------------------------------------
        double sx = 0, sy = 0, sz = 0, sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
        double fx = 0, fy = 0, fz = 0, lx = 0, ly = 0, lz = 0;
        if constexpr (Rows::kKeyed) {
            m = 0;
            double nd = (double)INFINITY, fd = -1.0;
            int ne = 0x7fffffff, fe = -1;
            for (int j = 0; j < len; ++j) {
                const int e = my[j];
                if (e == (int)qid) continue;
                ++m;
                const float4 p = a.pts[(int)min((unsigned)e, a.n_pts - 1u)];
                const double dx = (double)p.x - qx, dy = (double)p.y - qy, dz = (double)p.z - qz;
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 < nd || (d2 == nd && e < ne)) { nd = d2; ne = e; }
                if (d2 > fd || (d2 == fd && e > fe)) { fd = d2; fe = e; }
            }
            if (m > 0) {
                load_centred<F64>(a, (int)min((unsigned)ne, a.n_pts - 1u), qx, qy, qz, qp.x, qp.y, qp.z, fx, fy, fz);
                load_centred<F64>(a, (int)min((unsigned)fe, a.n_pts - 1u), qx, qy, qz, qp.x, qp.y, qp.z, lx, ly, lz);
            }
        }
        for (int j = 0; j < len; ++j) {
            if constexpr (Rows::kKeyed) {
                if (my[j] == (int)qid) continue;
            }
            double x, y, z;
            load_centred<F64>(a, (int)min((unsigned)my[j], a.n_pts - 1u), qx, qy, qz, qp.x, qp.y, qp.z, x, y, z);
            if constexpr (!Rows::kKeyed) {
                if (j == 0) { fx = x; fy = y; fz = z; }
                lx = x; ly = y; lz = z;
            }
            const double dx = x - fx, dy = y - fy, dz = z - fz;      // about the first neighbour, as k_fit
            sx += dx; sy += dy; sz += dz;
            sxx = fma(dx, dx, sxx); sxy = fma(dx, dy, sxy); sxz = fma(dx, dz, sxz);
            syy = fma(dy, dy, syy); syz = fma(dy, dz, syz); szz = fma(dz, dz, szz);
        }
        double rot[9];
        plane_rotation<F64>(m, sx, sy, sz, sxx, sxy, sxz, syy, syz, szz, fx, fy, fz, lx, ly, lz, a.force_jacobi != 0, rot);

        // ---- pass 2: the design rows, one by one ---------------------------------------------------------------
        Lstsq6 ls;
        ls.init();
#pragma unroll 1
        for (int j = 0; j < len; ++j) {
            if constexpr (Rows::kKeyed) {
                if (my[j] == (int)qid) continue;
            }
            double px, py, pz;
            load_centred<F64>(a, (int)min((unsigned)my[j], a.n_pts - 1u), qx, qy, qz, qp.x, qp.y, qp.z, px, py, pz);
            ls.add((float)((rot[0] * px + rot[1] * py) + rot[2] * pz), (float)((rot[3] * px + rot[4] * py) + rot[5] * pz),
                   (float)((rot[6] * px + rot[7] * py) + rot[8] * pz));
        }
        double sol[6];
        ls.solve(m, sol);
        if (m < 2) {
#pragma unroll
            for (int r = 0; r < 6; ++r) sol[r] = (double)nanf_;
        }
        if constexpr (OUT64) {
            double* co64 = a.coefs64 + out * 6;
            for (int j = 0; j < 6; ++j) co64[j] = sol[j];
            const double Fx = sol[3], Fy = sol[4], Fxx = 2.0 * sol[0], Fyy = 2.0 * sol[1], Fxy = sol[2];
            const double wgt = (1.0 + Fx * Fx) + Fy * Fy;
            a.K64[out] = (Fxx * Fyy - Fxy * Fxy) / (wgt * wgt);
            a.H64[out] = (((1.0 + Fx * Fx) * Fyy - ((2.0 * Fx) * Fy) * Fxy) + (1.0 + Fy * Fy) * Fxx) / (2.0 * (wgt * sqrt(wgt)));
        } else {
            const float Af = (float)sol[0], Bf = (float)sol[1], Cf = (float)sol[2], Df = (float)sol[3], Ef = (float)sol[4];
            float* co = a.coefs + out * 6;
            co[0] = Af; co[1] = Bf; co[2] = Cf; co[3] = Df; co[4] = Ef; co[5] = (float)sol[5];
            float Kg, Kh;
            monge_curvatures(Af, Bf, Cf, Df, Ef, Kg, Kh);
            a.K[out] = Kg;
            a.H[out] = Kh;
            a.H2[out] = Kh * Kh;
        }
    }
}

}  // namespace

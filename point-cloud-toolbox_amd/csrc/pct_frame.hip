// Per-point surface frames from the quadric fit: the fitted normal, the principal curvatures k1 >= k2 and their directions,
// for every owned row of the resident neighbour table whose fit is resident.  The fit builds the tangent-plane rotation R
// and the patch z = A a^2 + B b^2 + C ab + D a + E b + F of every row and lets two scalars leave the device (K, H); this
// kernel builds R again from the row and reads the row's coefficients, and keeps the rest.
//
// Row i, count_i = m valid neighbours (the contract, include/pct_hip.h; tests/frame_exact.py states it again in NumPy):
//   block   Q_j = p_j - p_i, load_centred(): cloud dtype, float64 arithmetic from there on
//   R       plane_rotation() of the block from the moments k_fit takes (about the first neighbour, the same operations in
//           the same order as pass 1 of area_row(): the same rotation bit for bit)
//   coefs   (A, B, C, D, E) = the row's float32 fit coefficients, widened; nothing is fitted here
//   patch   w = sqrt((1 + D D) + E E), m = (-D, -E, 1) / w;  g2 = 1 + D D, g = sqrt(g2), e1 = (1, 0, D) / g,
//           e2 = m x e1 = (-D E, g2, E) / (g w)
//   shape   II(x, y) = ((2A xa ya + C (xa yb + xb ya)) + 2B xb yb) / w on the first two components;
//           s11 = II(e1, e1), s12 = II(e1, e2), s22 = II(e2, e2)
//   k1, k2  h = (s11 + s22) / 2, d = (s11 - s22) / 2, r = sqrt(d d + s12 s12): k1 = h + r, k2 = h - r
//   t1, t2  Jacobi's small root, no atan2: t = s12 / (|d| + r), cj = 1 / sqrt(t t + 1), sj = t cj;
//           (c, s) = (cj, sj) where d > 0, (sj, cj) otherwise; t1 = c e1 + s e2, t2 = -s e1 + c e2;
//           r == 0 (umbilic): t1 = e1, t2 = e2
//   world   n = R^T m, d1 = R^T t1, d2 = R^T t2, component i = (R[0][i] v0 + R[1][i] v1) + R[2][i] v2; d1 and d2 under the
//           sign rule of write_frame() (pct_pca.hip): the component of largest magnitude positive, the first among equals
//   view    with a viewpoint v: ((vx - px) n0 + (vy - py) n1) + (vz - pz) n2 < 0, p = p_i in the cloud's dtype, flips:
//           n <- -n, (k1, k2) <- (-k2, -k1), (d1, d2) <- (d2, d1), flipped = 1
//   NaN     m < 2, a table entry outside the cloud, a non-finite R or coefficient: every output NaN, flipped = 0
//
// k_frame: one thread per owned row, 64-thread blocks in k_fit's XCD block order, rows read through FitArgs / TableRows as
// k_area reads them (int4 index loads, eight entries and their gathers in flight).  One pass over the row; no LDS, no
// scratch.  The moments loop is the third copy of a dozen lines (k_fit, area_row): DESIGN 4.3i has why it stays one.
// Compiled with -ffp-contract=off: the restatement rounds every product and sum separately.
#include "pct_fit_core.h"

namespace {

constexpr int kFrameBlock = 64;
constexpr int kFrameAhead = 8;                      // table entries (two int4) and gathers a lane issues together
// A/B builds that tell what the kernel waits for: -DPCT_FRAME_AB=1 computes every row and stores none,
// =2 reads the row's own record in place of every neighbour's (the loads stay, their traffic goes).  Both test a value
// the compiler cannot know (has_view is 0 or 1), so the arithmetic stays as it is.
#ifndef PCT_FRAME_AB
#define PCT_FRAME_AB 0
#endif

enum FrameWord { FW_NAN = 0, FW_FLIPPED = 1, FW_UMBILIC = 2 };     // unsigned long long words of FrameOut::words

struct FrameOut {
    double* normal;                 // (rows, 3)
    double* k12;                    // (rows, 2)
    double* dirs;                   // (rows, 3, 2)
    unsigned char* flipped;         // (rows)
    unsigned long long* words;      // eight words, zeroed per call: FrameWord
    const float* coefs;             // the fit's (rows, 6), in the fit's order
    const int* row_of;              // fit in table-row order, frames in public order: public row -> table row
    int coef_by_row;                // the fit's results are in table-row order
    int has_view;
    double vx, vy, vz;
};

__device__ __forceinline__ void to_world(const double (&rot)[9], double v0, double v1, double v2, double& x, double& y, double& z) {
    x = (rot[0] * v0 + rot[3] * v1) + rot[6] * v2;
    y = (rot[1] * v0 + rot[4] * v1) + rot[7] * v2;
    z = (rot[2] * v0 + rot[5] * v1) + rot[8] * v2;
}

__device__ __forceinline__ void sign_rule(double& x, double& y, double& z) {
    double big = x;
    if (fabs(y) > fabs(big)) big = y;
    if (fabs(z) > fabs(big)) big = z;
    if (big < 0.0) { x = -x; y = -y; z = -z; }
}

struct Frame {
    double n[3], k1, k2, d1[3], d2[3];
    int flipped, umbilic;
};

// One row from its table entries and coefficients to its frame.  false: a NaN row.
template <bool F64>
__device__ __forceinline__ bool frame_row(const FitArgs& a, const FrameOut& o, int64_t row, int64_t qid, const float4 qp,
                                          const float* __restrict__ co, Frame& f) {
    const TableRows rows;
    double qx = qp.x, qy = qp.y, qz = qp.z;
    if (F64) {
        const double4 qd = a.ptsd[qid];
        qx = qd.x; qy = qd.y; qz = qd.z;
    }
    const int m = min(rows.length(a, row), a.k);
    if (m < 2) return false;
    const int* my = rows.start(a, row);
    const int last4 = a.pitch - 4;
    const double A = (double)co[0], B = (double)co[1], C = (double)co[2], D = (double)co[3], E = (double)co[4];

    // kFrameAhead entries from j0 on, every gather issued before the first use; entries behind the row's count, and entries
    // that are no record of the cloud, are clamped -- loaded from inside the arrays, never used (k_area's scheme)
    bool bad_id = false;
    int4 w0, w1;
    const auto prime = [&](int j0) {
        w0 = *(const int4*)(my + min(j0, last4));
        w1 = *(const int4*)(my + min(j0 + 4, last4));
    };
    double sx = 0, sy = 0, sz = 0, sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
    double fx = 0, fy = 0, fz = 0, lx = 0, ly = 0, lz = 0;
    prime(0);
    for (int j0 = 0; j0 < m; j0 += kFrameAhead) {
        double x[kFrameAhead], y[kFrameAhead], z[kFrameAhead];
        const int4 v0 = w0, v1 = w1;
        prime(j0 + kFrameAhead);
        const int id[kFrameAhead] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
        for (int u = 0; u < kFrameAhead; ++u) {
            bad_id |= j0 + u < m && (unsigned)id[u] >= a.n_pts;
            const int at = PCT_FRAME_AB == 2 ? (int)qid + (o.has_view >> 8) : (int)min((unsigned)id[u], a.n_pts - 1u);
            load_centred<F64>(a, at, qx, qy, qz, qp.x, qp.y, qp.z, x[u], y[u], z[u]);
        }
        if (j0 == 0) { fx = x[0]; fy = y[0]; fz = z[0]; }
#pragma unroll
        for (int u = 0; u < kFrameAhead; ++u) {
            if (j0 + u < m) {
                const double dx = x[u] - fx, dy = y[u] - fy, dz = z[u] - fz;
                sx += dx; sy += dy; sz += dz;
                sxx = fma(dx, dx, sxx); sxy = fma(dx, dy, sxy); sxz = fma(dx, dz, sxz);
                syy = fma(dy, dy, syy); syz = fma(dy, dz, syz); szz = fma(dz, dz, szz);
                lx = x[u]; ly = y[u]; lz = z[u];
            }
        }
    }
    if (bad_id) return false;
    double rot[9];
    plane_rotation<F64>(m, sx, sy, sz, sxx, sxy, sxz, syy, syz, szz, fx, fy, fz, lx, ly, lz, a.force_jacobi != 0, rot);
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) finite = finite && fabs(rot[i]) < (double)INFINITY;        // (false for NaN too)
    finite = finite && fabs(A) < (double)INFINITY && fabs(B) < (double)INFINITY && fabs(C) < (double)INFINITY &&
             fabs(D) < (double)INFINITY && fabs(E) < (double)INFINITY;
    if (!finite) return false;

    // ---- the patch at a = b = 0, in the rotated frame ------------------------------------------------------------------
    const double g2 = 1.0 + D * D;
    const double w = sqrt(g2 + E * E), g = sqrt(g2);
    const double m0 = -D / w, m1 = -E / w, m2 = 1.0 / w;
    const double e1a = 1.0 / g, e1c = D / g;                                  // e1 = (e1a, 0, e1c)
    const double gw = g * w;
    const double e2a = (-(D * E)) / gw, e2b = g2 / gw, e2c = E / gw;
    const double A2 = 2.0 * A, B2 = 2.0 * B;
    const auto II = [&](double xa, double xb, double ya, double yb) {
        return ((A2 * xa * ya + C * (xa * yb + xb * ya)) + B2 * xb * yb) / w;
    };
    const double s11 = II(e1a, 0.0, e1a, 0.0), s12 = II(e1a, 0.0, e2a, e2b), s22 = II(e2a, e2b, e2a, e2b);
    const double h = 0.5 * (s11 + s22), d = 0.5 * (s11 - s22);
    const double r = sqrt(d * d + s12 * s12);
    f.k1 = h + r;
    f.k2 = h - r;
    double c = 1.0, s = 0.0;
    f.umbilic = r == 0.0 ? 1 : 0;
    if (r != 0.0) {
        const double t = s12 / (fabs(d) + r);
        const double cj = 1.0 / sqrt(t * t + 1.0), sj = t * cj;
        c = d > 0.0 ? cj : sj;
        s = d > 0.0 ? sj : cj;
    }
    const double t1a = c * e1a + s * e2a, t1b = s * e2b, t1c = c * e1c + s * e2c;
    const double t2a = (-s) * e1a + c * e2a, t2b = c * e2b, t2c = (-s) * e1c + c * e2c;

    // ---- back to the cloud's frame ---------------------------------------------------------------------------------------
    to_world(rot, m0, m1, m2, f.n[0], f.n[1], f.n[2]);
    to_world(rot, t1a, t1b, t1c, f.d1[0], f.d1[1], f.d1[2]);
    to_world(rot, t2a, t2b, t2c, f.d2[0], f.d2[1], f.d2[2]);
    sign_rule(f.d1[0], f.d1[1], f.d1[2]);
    sign_rule(f.d2[0], f.d2[1], f.d2[2]);
    f.flipped = 0;
    if (o.has_view) {
        const double px = F64 ? qx : (double)qp.x, py = F64 ? qy : (double)qp.y, pz = F64 ? qz : (double)qp.z;
        if (((o.vx - px) * f.n[0] + (o.vy - py) * f.n[1]) + (o.vz - pz) * f.n[2] < 0.0) {
            f.flipped = 1;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                f.n[i] = -f.n[i];
                const double t = f.d1[i];
                f.d1[i] = f.d2[i];
                f.d2[i] = t;
            }
            const double k1 = f.k1;
            f.k1 = -f.k2;
            f.k2 = -k1;
        }
    }
    return true;
}

template <bool F64>
__global__ __launch_bounds__(kFrameBlock) void k_frame(FitArgs a, FrameOut o) {
    const int lane = threadIdx.x;
    const int64_t row0 = (a.blocks_per_xcd ? (int64_t)(blockIdx.x & 7u) * a.blocks_per_xcd + (blockIdx.x >> 3) : (int64_t)blockIdx.x) * kFrameBlock;
    if (row0 >= a.rows) return;
    const int64_t row = row0 + lane;
    bool owned = false, ok = false;
    Frame f;
    f.flipped = f.umbilic = 0;
    int64_t out = 0;
    if (row < a.rows) {
        const TableRows rows;
        const int64_t qid = rows.query(a, row);
        const float4 qp = a.pts[qid];
        const int pub = __float_as_int(qp.w);
        if (a.out_by_row || (pub >= a.q_begin && pub < a.q_end)) {             // owned rows only
            owned = true;
            out = a.out_by_row ? row : (int64_t)pub - a.out_base;
            const int64_t at = !o.coef_by_row ? (int64_t)pub - a.out_base : a.out_by_row ? row : (int64_t)o.row_of[(int64_t)pub - a.out_base];
            ok = frame_row<F64>(a, o, row, qid, qp, o.coefs + at * 6, f);
        }
    }
    if (owned && (PCT_FRAME_AB != 1 || o.has_view < 0)) {
        const double nan = (double)__int_as_float(0x7fc00000);
        double* pn = o.normal + out * 3;
        double* pk = o.k12 + out * 2;
        double* pd = o.dirs + out * 6;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            pn[i] = ok ? f.n[i] : nan;
            pd[2 * i] = ok ? f.d1[i] : nan;            // [row][column] of the (3, 2) frame
            pd[2 * i + 1] = ok ? f.d2[i] : nan;
        }
        pk[0] = ok ? f.k1 : nan;
        pk[1] = ok ? f.k2 : nan;
        o.flipped[out] = (unsigned char)(ok ? f.flipped : 0);
    }
    // the wave's counts of the statistics
    const unsigned long long nm = __ballot(owned && !ok), fm = __ballot(ok && f.flipped), um = __ballot(ok && f.umbilic);
    if (lane == 0) {
        if (nm) atomicAdd(&o.words[FW_NAN], (unsigned long long)__popcll(nm));
        if (fm) atomicAdd(&o.words[FW_FLIPPED], (unsigned long long)__popcll(fm));
        if (um) atomicAdd(&o.words[FW_UMBILIC], (unsigned long long)__popcll(um));
    }
}

}  // namespace

// Frames of the owned rows of the resident table, in the order pct_launch_fit_table leaves its results in (table-row order
// behind a sweep of a cell list, public order otherwise).  The statistics words go to ctx->pin->frame_words; both are
// complete once the stream has been waited for.  viewpoint: three finite doubles, or null.
int pct_launch_point_frames(pct_ctx* ctx, const double* viewpoint, bool* by_row) {
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
    PCT_TRY(pct_reserve(ctx, &ctx->frame, (size_t)rows * 11 * sizeof(double)));
    PCT_TRY(pct_reserve(ctx, &ctx->frame_flip, 64 + (size_t)rows));
    FrameOut o = {};
    o.normal = (double*)ctx->frame.p;
    o.k12 = o.normal + rows * 3;
    o.dirs = o.k12 + rows * 2;
    o.words = (unsigned long long*)ctx->frame_flip.p;
    o.flipped = (unsigned char*)ctx->frame_flip.p + 64;
    o.coefs = (const float*)ctx->coefs.p;
    const bool fit_by_row = ctx->res.in_row_order(PCT_R_FIT);
    o.coef_by_row = fit_by_row ? 1 : 0;
    if (fit_by_row && !sorted) {                 // the fit in table-row order, the frames in public order
        PCT_TRY(pct_ensure_row_of(ctx));
        o.row_of = (const int*)ctx->row_of.p;
    }
    if (viewpoint) {
        o.has_view = 1;
        o.vx = viewpoint[0]; o.vy = viewpoint[1]; o.vz = viewpoint[2];
    }
    PCT_HIP(ctx, hipMemsetAsync(ctx->frame_flip.p, 0, 64, ctx->stream));
    int blocks = (int)((rows + kFrameBlock - 1) / kFrameBlock);
    if (blocks > 0) {
        a.blocks_per_xcd = pct_getenv("PCT_NO_XCD_MAP") ? 0 : (blocks + 7) / 8;
        if (a.blocks_per_xcd) blocks = a.blocks_per_xcd * 8;
        if (ctx->has_f64) PCT_LAUNCH(k_frame<true>, dim3(blocks), dim3(kFrameBlock), 0, ctx->stream, a, o);
        else PCT_LAUNCH(k_frame<false>, dim3(blocks), dim3(kFrameBlock), 0, ctx->stream, a, o);
        PCT_HIP(ctx, hipGetLastError());
    }
    PCT_HIP(ctx, hipMemcpyAsync(ctx->pin->frame_words, ctx->frame_flip.p, sizeof(ctx->pin->frame_words), hipMemcpyDeviceToHost, ctx->stream));
    *by_row = sorted;
    return PCT_OK;
}

// rows, NaN rows, flipped rows, umbilic rows
void pct_frame_report(pct_ctx* ctx, pct_stage_report* rep) {
    const unsigned long long* w = ctx->pin->frame_words;
    const int64_t st[4] = {ctx->q_end - ctx->q_begin, (int64_t)w[FW_NAN], (int64_t)w[FW_FLIPPED], (int64_t)w[FW_UMBILIC]};
    for (int i = 0; i < 4; ++i) rep->stats[i] = st[i];
}

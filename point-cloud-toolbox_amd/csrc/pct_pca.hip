// PCA principal curvatures: principal_curvatures_via_principal_component_analysis, pointCloudToolbox.py:901-950.
//
// Per point i the reference takes the k points nearest to it by np.linalg.norm(points - points[i], axis=1), evaluated IN
// THE CLOUD'S DTYPE, drops the first entry of the argsort (the point itself or an exact duplicate of it) and runs
// scipy.linalg.eigh on np.cov of the neighbours' raw coordinates (float64, about the neighbour mean, ddof 1):
// lambda_1 >= lambda_2 are the two largest eigenvalues, their eigenvectors the columns of a (3, 2) frame,
// K = lambda_1 lambda_2, H = (lambda_1 + lambda_2) / 2.
//
// GPU form:
// 1. the handle's sweep with k + m candidates per point (m <= PCT_PCA_EXTRA over-fetched);
// 2. k_pca_frame, one thread per table row: the candidates re-ranked by the reference's own key -- the float32
//    (dx^2 + dy^2) + dz^2 NumPy evaluates for a float32 cloud, the same sum in float64 for a float64 cloud -- the m
//    largest (key, sweep position) dropped, the float64 covariance in two passes (neighbour mean, then centred sums),
//    cyclic Jacobi with eigenvector accumulation;
// 3. float64 clouds: the sweep ranks float32-rounded points.  For it the cloud is recentred on its first point c (a
//    georeferenced scan at a 5e6 m northing would otherwise round to half a metre), then a row is accepted only when
//    its k-th float64 distance lies below the largest candidate distance minus 2 R, R = the largest
//    |(p - c) - fl32(p - c)| of the cloud: no point outside the candidates can then be nearer.  The other rows go to
//    k_pca_exact, one block per row, which reads every point of the cloud, collects those within the row's k-th
//    candidate distance and ranks them exactly by (float64 key, index).  That pass is O(N) per row: the call refuses,
//    before launching it, when it would exceed kExactVisits point visits (k = 511 leaves no room for extra candidates,
//    so every row needs it; float32 rounding of the recentred cloud coarser than the neighbour spacing does the same).
// Eigenvector signs are LAPACK's choice in the reference; here the component of largest magnitude is positive (the first
// of equal magnitudes).
#include "pct_internal.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int kExactCap = 3072;     // points one k_pca_exact block can collect within its row's bound (LDS)
constexpr double kExactVisits = 1073741824.0;   // point visits k_pca_exact may make in one call (rows x N): ~30 ms

struct PcaArgs {
    const float4* pts;      // float32 records of the table's space (sorted4 / pts4), w = public index bits
    const double4* ptsd;    // float64 records of the same space (float64 clouds), w = public index; else null
    const int* row_query;   // table row -> position of its query; null: position = row (public space)
    const int* table;       // kc candidate positions per row, in the sweep's order (distance, then index)
    int pitch, kc, k;
    int all_candidates;     // kc == N - 1: every other point is a candidate (nothing to certify)
    int64_t rows, npts;
    double round2;          // 2 R (float64 clouds)
    double cx, cy, cz;      // float64 clouds: the point the sweep's float32 coordinates are relative to
    double *l1, *l2, *K, *H, *dirs;     // public order; dirs (N, 3, 2) C order
    int* nbr;               // optional (N, k) int32: the public indices each row was computed from
    int* hdr;               // [0] rows handed to k_pca_exact, [1] a k_pca_exact row could not be served
    int* redo_row;
    double* redo_bound;     // squared k-th float64 distance among the row's candidates
};

// np.linalg.norm(points - point, axis=1) before its sqrt (monotone: the order is the same), in the cloud's dtype:
// add.reduce over three elements is (x^2 + y^2) + z^2.  x, y, z: the raw coordinates for the covariance.
template <bool F64>
__device__ __forceinline__ double rank_key(const PcaArgs& a, int pos, double qx, double qy, double qz, float4 qf,
                                           double& x, double& y, double& z, int& pub) {
    if (F64) {
        const double4 p = a.ptsd[pos];
        x = p.x; y = p.y; z = p.z; pub = (int)p.w;
        const double dx = p.x - qx, dy = p.y - qy, dz = p.z - qz;
        return (dx * dx + dy * dy) + dz * dz;
    } else {
        const float4 p = a.pts[pos];
        x = p.x; y = p.y; z = p.z; pub = __float_as_int(p.w);
        const float dx = p.x - qf.x, dy = p.y - qf.y, dz = p.z - qf.z;
        return (double)((dx * dx + dy * dy) + dz * dz);
    }
}

// one Jacobi rotation annihilating a_pq (r = third index), eigenvector columns p and q rotated along (as pct_fit.hip)
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq,
                                              double& vp0, double& vp1, double& vp2, double& vq0, double& vq1, double& vq2) {
    if (apq == 0.0) return;
    const double alpha = 0.5 * (aqq - app), beta = apq;
    const double t = (alpha >= 0.0 ? beta : -beta) / (fabs(alpha) + sqrt(alpha * alpha + beta * beta));
    const double c = rsqrt(t * t + 1.0), s = t * c;
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0;
    const double rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
    double u, w;
    u = vp0; w = vq0; vp0 = c * u - s * w; vq0 = s * u + c * w;
    u = vp1; w = vq1; vp1 = c * u - s * w; vq1 = s * u + c * w;
    u = vp2; w = vq2; vp2 = c * u - s * w; vq2 = s * u + c * w;
}

// covariance (divided by k - 1) -> lambda_1, lambda_2, their eigenvectors, K, H of public row pub
__device__ void write_frame(const PcaArgs& a, int64_t pub, double a00, double a01, double a02, double a11, double a12,
                            double a22) {
    double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;   // v[row][col]
#pragma unroll 1
    for (int sweep = 0; sweep < 16; ++sweep) {
        const double off = fabs(a01) + fabs(a02) + fabs(a12);
        if (off <= 1e-22 * (fabs(a00) + fabs(a11) + fabs(a22))) break;
        jacobi_rotate(a00, a11, a01, a02, a12, v00, v10, v20, v01, v11, v21);   // (p,q)=(0,1), r=2
        jacobi_rotate(a00, a22, a02, a01, a12, v00, v10, v20, v02, v12, v22);   // (0,2), r=1
        jacobi_rotate(a11, a22, a12, a01, a02, v01, v11, v21, v02, v12, v22);   // (1,2), r=0
    }
    int i1, i2;                                       // the largest eigenvalue and the second (ties: lower index first)
    if (a00 >= a11 && a00 >= a22) { i1 = 0; i2 = a11 >= a22 ? 1 : 2; }
    else if (a11 >= a22)          { i1 = 1; i2 = a00 >= a22 ? 0 : 2; }
    else                          { i1 = 2; i2 = a00 >= a11 ? 0 : 1; }
    const double l1 = i1 == 0 ? a00 : i1 == 1 ? a11 : a22;
    const double l2 = i2 == 0 ? a00 : i2 == 1 ? a11 : a22;
    double* d = a.dirs + 6 * pub;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int i = c == 0 ? i1 : i2;
        double x = i == 0 ? v00 : i == 1 ? v01 : v02;
        double y = i == 0 ? v10 : i == 1 ? v11 : v12;
        double z = i == 0 ? v20 : i == 1 ? v21 : v22;
        double big = x;
        if (fabs(y) > fabs(big)) big = y;
        if (fabs(z) > fabs(big)) big = z;
        if (big < 0.0) { x = -x; y = -y; z = -z; }
        d[c] = x; d[2 + c] = y; d[4 + c] = z;         // [row][column] of the (3, 2) frame
    }
    a.l1[pub] = l1;
    a.l2[pub] = l2;
    a.K[pub] = l1 * l2;                               // pct:933-934
    a.H[pub] = (l1 + l2) / 2;
}

template <bool F64>
__global__ __launch_bounds__(64) void k_pca_frame(PcaArgs a) {
    const int64_t row = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (row >= a.rows) return;
    const int qpos = a.row_query ? a.row_query[row] : (int)row;
    float4 qf;
    double qx, qy, qz;
    int qpub;
    if (F64) {
        const double4 q = a.ptsd[qpos];
        qx = q.x; qy = q.y; qz = q.z; qpub = (int)q.w;
        qf = make_float4((float)(q.x - a.cx), (float)(q.y - a.cy), (float)(q.z - a.cz), 0.f);   // as the sweep saw it
    } else {
        qf = a.pts[qpos];
        qx = qf.x; qy = qf.y; qz = qf.z; qpub = __float_as_int(qf.w);
    }
    const int* my = a.table + row * a.pitch;
    const int m = a.kc - a.k;
    double x, y, z;
    int pub;
    // pass 1: the m largest (key, sweep position) pairs, descending -- the candidates the row drops; and (float64
    // clouds) the largest candidate distance in the float32-rounded space the sweep ranked in
    double tk[PCT_PCA_EXTRA];
    int tp[PCT_PCA_EXTRA];
#pragma unroll
    for (int i = 0; i < PCT_PCA_EXTRA; ++i) { tk[i] = -1.0; tp[i] = -1; }
    double far2 = 0.0;
    for (int j = 0; j < a.kc; ++j) {
        const int pos = my[j];
        double key = rank_key<F64>(a, pos, qx, qy, qz, qf, x, y, z, pub);
        int kp = j;
        if (F64) {
            const double dx = (double)(float)(x - a.cx) - (double)qf.x, dy = (double)(float)(y - a.cy) - (double)qf.y,
                         dz = (double)(float)(z - a.cz) - (double)qf.z;
            far2 = fmax(far2, (dx * dx + dy * dy) + dz * dz);
        }
        if (m == 0) continue;                          // nothing to drop
#pragma unroll
        for (int i = 0; i < PCT_PCA_EXTRA; ++i) {
            if (i < m && (key > tk[i] || (key == tk[i] && kp > tp[i]))) {
                const double t = tk[i]; tk[i] = key; key = t;
                const int u = tp[i]; tp[i] = kp; kp = u;
            }
        }
    }
    double tkey = INFINITY;
    int tpos = INT_MAX;
#pragma unroll
    for (int i = 0; i < PCT_PCA_EXTRA; ++i)
        if (i == m - 1) { tkey = tk[i]; tpos = tp[i]; }
    // pass 2: the neighbour mean; the k-th key
    double sx = 0, sy = 0, sz = 0, kth = 0;
    int* nb = a.nbr ? a.nbr + (int64_t)qpub * a.k : nullptr;
    int taken = 0;
    for (int j = 0; j < a.kc; ++j) {
        const double key = rank_key<F64>(a, my[j], qx, qy, qz, qf, x, y, z, pub);
        if (!(key < tkey || (key == tkey && j < tpos))) continue;
        sx += x; sy += y; sz += z;
        kth = fmax(kth, key);
        if (nb) nb[taken] = pub;
        ++taken;
    }
    if (F64 && !a.all_candidates) {
        const double lim = sqrt(far2) - a.round2;
        if (!(sqrt(kth) < lim * (1.0 - 1e-12))) {    // a point beyond the candidates might be nearer: exact pass
            const int slot = atomicAdd(&a.hdr[0], 1);
            a.redo_row[slot] = (int)row;
            a.redo_bound[slot] = kth;
            return;
        }
    }
    const double inv = 1.0 / (double)a.k;
    const double mx = sx * inv, my_ = sy * inv, mz = sz * inv;
    // pass 3: centred sums
    double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0;
    for (int j = 0; j < a.kc; ++j) {
        const double key = rank_key<F64>(a, my[j], qx, qy, qz, qf, x, y, z, pub);
        if (!(key < tkey || (key == tkey && j < tpos))) continue;
        x -= mx; y -= my_; z -= mz;
        a00 = fma(x, x, a00); a01 = fma(x, y, a01); a02 = fma(x, z, a02);
        a11 = fma(y, y, a11); a12 = fma(y, z, a12); a22 = fma(z, z, a22);
    }
    const double s = 1.0 / (double)(a.k - 1);        // np.cov: ddof 1, multiplied by the reciprocal
    write_frame(a, qpub, a00 * s, a01 * s, a02 * s, a11 * s, a12 * s, a22 * s);
}

// float64 rows the certificate could not vouch for: every point of the cloud within the row's k-th candidate distance
// (at least the k candidates themselves), ranked by (float64 key, public index); the k first make the neighbourhood
__global__ __launch_bounds__(256) void k_pca_exact(PcaArgs a) {
    __shared__ double skey[kExactCap];
    __shared__ int spub[kExactCap];
    __shared__ int spos[kExactCap];
    __shared__ int ssel[PCT_K_MAX];
    __shared__ int cnt;
    const int row = a.redo_row[blockIdx.x];
    const double bound = a.redo_bound[blockIdx.x];
    const int qpos = a.row_query ? a.row_query[row] : row;
    const double4 q = a.ptsd[qpos];
    const float4 qf = make_float4(0.f, 0.f, 0.f, 0.f);       // (unused by the float64 key)
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    double x, y, z;
    int pub;
    for (int64_t j = threadIdx.x; j < a.npts; j += 256) {
        if (j == qpos) continue;
        const double key = rank_key<true>(a, (int)j, q.x, q.y, q.z, qf, x, y, z, pub);
        if (key <= bound) {
            const int e = atomicAdd(&cnt, 1);
            if (e < kExactCap) { skey[e] = key; spub[e] = pub; spos[e] = (int)j; }
        }
    }
    __syncthreads();
    const int c = cnt;
    if (c > kExactCap || c < a.k) {
        if (threadIdx.x == 0) atomicOr(&a.hdr[1], 1);
        return;
    }
    for (int e = threadIdx.x; e < c; e += 256) {
        const double ke = skey[e];
        const int pe = spub[e];
        int r = 0;
        for (int f = 0; f < c; ++f) r += skey[f] < ke || (skey[f] == ke && spub[f] < pe);
        if (r < a.k) ssel[r] = e;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int* nb = a.nbr ? a.nbr + (int64_t)q.w * a.k : nullptr;
    double sx = 0, sy = 0, sz = 0;
    for (int r = 0; r < a.k; ++r) {
        const double4 p = a.ptsd[spos[ssel[r]]];
        sx += p.x; sy += p.y; sz += p.z;
        if (nb) nb[r] = spub[ssel[r]];
    }
    const double inv = 1.0 / (double)a.k;
    const double mx = sx * inv, my_ = sy * inv, mz = sz * inv;
    double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0;
    for (int r = 0; r < a.k; ++r) {
        const double4 p = a.ptsd[spos[ssel[r]]];
        x = p.x - mx; y = p.y - my_; z = p.z - mz;
        a00 = fma(x, x, a00); a01 = fma(x, y, a01); a02 = fma(x, z, a02);
        a11 = fma(y, y, a11); a12 = fma(y, z, a12); a22 = fma(z, z, a22);
    }
    const double s = 1.0 / (double)(a.k - 1);
    write_frame(a, (int64_t)q.w, a00 * s, a01 * s, a02 * s, a11 * s, a12 * s, a22 * s);
}

// any non-finite coordinate.  Float64 clouds: the sweep's coordinates recentred on the first point c -- pts4d = p - c,
// xyz = fl32(p - c) -- from the untouched copy `orig`, and R = max |(p - c) - fl32(p - c)| (the float64 subtraction's own
// rounding included) as the bits of a non-negative double (ordered as unsigned integers)
__global__ __launch_bounds__(256) void k_pca_prep(float* __restrict__ xyz, const double4* __restrict__ orig, double4* __restrict__ pts4d,
                                                  int64_t n, unsigned long long* __restrict__ r_bits, int* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double r = 0.0;
    int b = 0;
    if (i < n) {
        if (orig) {
            const double4 c = orig[0], p = orig[i];
            b = !(isfinite(p.x) && isfinite(p.y) && isfinite(p.z));
            const double dx = p.x - c.x, dy = p.y - c.y, dz = p.z - c.z;
            const float fx = (float)dx, fy = (float)dy, fz = (float)dz;
            pts4d[i] = make_double4(dx, dy, dz, p.w);
            xyz[3 * i] = fx; xyz[3 * i + 1] = fy; xyz[3 * i + 2] = fz;
            const double ex = dx - fx, ey = dy - fy, ez = dz - fz;
            r = b ? 0.0 : sqrt((ex * ex + ey * ey) + ez * ez) + 0x1p-52 * ((fabs(dx) + fabs(dy)) + fabs(dz));
            if (!b && !isfinite(r)) r = INFINITY;     // beyond float32's range: nothing can be certified
        } else {
            b = !(isfinite(xyz[3 * i]) && isfinite(xyz[3 * i + 1]) && isfinite(xyz[3 * i + 2]));
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        r = fmax(r, __shfl_xor(r, o));
        b |= __shfl_xor(b, o);
    }
    if ((threadIdx.x & 63) == 0) {
        if (r > 0.0) atomicMax(r_bits, (unsigned long long)__double_as_longlong(r));
        if (b) atomicOr(bad, 1);
    }
}

// float64 clouds after the sweep: the cloud as it was uploaded (public records, their float32 rounding) and, in the cell
// order of the sweep, the original float64 records for the keys and the covariance
__global__ __launch_bounds__(256) void k_pca_restore(const double4* __restrict__ orig, int64_t n, double4* __restrict__ pts4d,
                                                     float* __restrict__ xyz, double4* __restrict__ sorted4d) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double4 p = orig[i];
    pts4d[i] = p;
    xyz[3 * i] = (float)p.x; xyz[3 * i + 1] = (float)p.y; xyz[3 * i + 2] = (float)p.z;
    if (sorted4d) sorted4d[i] = orig[(int64_t)sorted4d[i].w];
}

// pca_aux: [0,8) R bits  [8,12) non-finite flag  [12,20) hdr  [32, ...) redo rows (int), then redo bounds (double)
size_t bounds_offset(int64_t n) { return 32 + ((size_t)n * 4 + 7) / 8 * 8; }

}  // namespace

int pct_pca_prep(pct_ctx* ctx, double* round_off, bool* nonfinite, double origin[3]) {
    const int64_t n = ctx->n;
    PCT_TRY(pct_reserve(ctx, &ctx->pca_aux, bounds_offset(n) + (size_t)n * sizeof(double)));
    char* h = (char*)ctx->pca_aux.p;
    PCT_HIP(ctx, hipMemsetAsync(h, 0, 32, ctx->stream));
    double c[4] = {0, 0, 0, 0};
    if (ctx->has_f64) {            // the uploaded records stay in pca_orig while the sweep sees the recentred cloud
        PCT_TRY(pct_reserve(ctx, &ctx->pca_orig, (size_t)n * sizeof(double4)));
        PCT_HIP(ctx, hipMemcpyAsync(ctx->pca_orig.p, ctx->pts4d.p, (size_t)n * sizeof(double4), hipMemcpyDeviceToDevice, ctx->stream));
        PCT_HIP(ctx, hipMemcpyAsync(c, ctx->pca_orig.p, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
        ctx->pca_recentred = true;
        ctx->grid_valid = ctx->pts4_valid = ctx->qpts4_valid = false;
        ctx->res.drop(PCT_TABLE_AND_FIT_LOST);
    }
    PCT_LAUNCH(k_pca_prep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (float*)ctx->xyz_view,
               ctx->has_f64 ? (const double4*)ctx->pca_orig.p : nullptr, ctx->has_f64 ? (double4*)ctx->pts4d.p : nullptr, n,
               (unsigned long long*)h, (int*)(h + 8));
    PCT_HIP(ctx, hipGetLastError());
    unsigned long long hb[2] = {0, 0};
    PCT_HIP(ctx, hipMemcpyAsync(hb, h, sizeof(hb), hipMemcpyDeviceToHost, ctx->stream));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(round_off, &hb[0], sizeof(double));
    *nonfinite = (hb[1] & 0xffffffffull) != 0;
    origin[0] = c[0]; origin[1] = c[1]; origin[2] = c[2];
    return PCT_OK;
}

int pct_pca_restore(pct_ctx* ctx) {
    if (!ctx->pca_recentred) return PCT_OK;
    const int64_t n = ctx->n;
    const bool sorted = ctx->res.has(PCT_R_TABLE) && ctx->knn_sorted_space;
    PCT_LAUNCH(k_pca_restore, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const double4*)ctx->pca_orig.p, n,
               (double4*)ctx->pts4d.p, (float*)ctx->xyz_view, sorted ? (double4*)ctx->sorted4d.p : nullptr);
    PCT_HIP(ctx, hipGetLastError());
    ctx->pca_recentred = false;
    ctx->pts4_valid = ctx->qpts4_valid = false;       // (float32 packs of the recentred cloud)
    return PCT_OK;
}

int pct_launch_pca(pct_ctx* ctx, int32_t k, double round2, const double origin[3], bool keep_neighbors, int64_t* exact_rows) {
    const int64_t n = ctx->n;
    PCT_TRY(pct_reserve(ctx, &ctx->pca, (size_t)n * 10 * sizeof(double)));
    if (keep_neighbors) PCT_TRY(pct_reserve(ctx, &ctx->pca_nbr, (size_t)n * k * sizeof(int)));
    const bool sorted = ctx->knn_sorted_space;
    PcaArgs a = {};
    a.pts = (const float4*)(sorted ? ctx->sorted4.p : ctx->pts4.p);
    a.ptsd = ctx->has_f64 ? (const double4*)(sorted ? ctx->sorted4d.p : ctx->pts4d.p) : nullptr;
    a.row_query = sorted ? (const int*)ctx->owned_pos.p : nullptr;
    a.table = (const int*)ctx->nbr_pos.p;
    a.pitch = ctx->nbr_pitch;
    a.kc = ctx->k;
    a.k = k;
    a.all_candidates = (int64_t)ctx->k >= n - 1;
    a.rows = n;
    a.npts = sorted ? ctx->n_grid : n;
    a.round2 = round2;
    a.cx = origin[0]; a.cy = origin[1]; a.cz = origin[2];
    double* o = (double*)ctx->pca.p;
    a.l1 = o; a.l2 = o + n; a.K = o + 2 * n; a.H = o + 3 * n; a.dirs = o + 4 * n;
    a.nbr = keep_neighbors ? (int*)ctx->pca_nbr.p : nullptr;
    char* h = (char*)ctx->pca_aux.p;
    a.hdr = (int*)(h + 12);
    a.redo_row = (int*)(h + 32);
    a.redo_bound = (double*)(h + bounds_offset(n));
    PCT_HIP(ctx, hipMemsetAsync(a.hdr, 0, 2 * sizeof(int), ctx->stream));
    const dim3 blocks((unsigned)((n + 63) / 64));
    if (a.ptsd)
        PCT_LAUNCH(k_pca_frame<true>, blocks, dim3(64), 0, ctx->stream, a);
    else
        PCT_LAUNCH(k_pca_frame<false>, blocks, dim3(64), 0, ctx->stream, a);
    PCT_HIP(ctx, hipGetLastError());
    int hb[2] = {0, 0};
    if (a.ptsd) {
        PCT_HIP(ctx, hipMemcpyAsync(hb, a.hdr, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (hb[0] > 0 && (double)hb[0] * (double)a.npts > kExactVisits) {
            if (a.kc == a.k)
                return pct_fail(ctx, PCT_ERR_INVALID, "pct_pca_curvatures: float64 cloud at k = %d leaves no room for candidates "
                                "beyond k (at most %d), so none of its rows can be certified from the float32-rounded sweep; "
                                "the exhaustive float64 pass for %d rows of %lld points exceeds its limit of %.0f point visits",
                                a.k, PCT_K_MAX, hb[0], (long long)a.npts, kExactVisits);
            return pct_fail(ctx, PCT_ERR_INVALID, "pct_pca_curvatures: %d rows of this float64 cloud cannot be certified: its "
                            "float32 rounding after recentring (R = %.3g) is not small against the spacing of their k-th "
                            "neighbours; the exhaustive float64 pass over %lld points exceeds its limit of %.0f point visits",
                            hb[0], 0.5 * round2, (long long)a.npts, kExactVisits);
        }
        if (hb[0] > 0) {
            PCT_LAUNCH(k_pca_exact, dim3((unsigned)hb[0]), dim3(256), 0, ctx->stream, a);
            PCT_HIP(ctx, hipGetLastError());
            PCT_HIP(ctx, hipMemcpyAsync(hb + 1, a.hdr + 1, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
            PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
            if (hb[1])
                return pct_fail(ctx, PCT_ERR_INVALID, "pct_pca_curvatures: an uncertified float64 row has more than %d points "
                                "within its k-th candidate distance (the float32-rounded sweep's candidates lie far beyond the "
                                "row's true neighbours)", kExactCap);
        }
    }
    *exact_rows = hb[0];
    return PCT_OK;
}

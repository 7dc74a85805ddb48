// The row code of the tangent-plane Voronoi cell, shared by pct_area.hip (areas) and pct_fan.hip (fans and corners): one
// cut of the polygon, and one row from its table entries to the polygon left.  LAB = false is the areas instantiation,
// token for token what pct_area.hip held; LAB = true carries one label per polygon vertex beside x and y.
#pragma once
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

// The polygon of one row: vertex i at x[i * STRIDE], y[i * STRIDE] (STRIDE = lanes per block on the fast path).
// LAB: beside them lab[i * STRIDE], the label of the edge from vertex i to vertex i + 1 -- the row slot of the neighbour
// whose bisector the edge lies on, -1 on an edge of the square (k <= 511: sixteen bits).
template <int STRIDE, bool LAB = false>
struct Poly {
    double* x;
    double* y;
    int cap;
    short* lab;
    __device__ __forceinline__ short& Lab(int i) const { return lab[i * STRIDE]; }
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
// LAB, a cut by the neighbour of row slot j: the vertices that stay keep their labels, I1 takes j (the edge I1 -> I2 lies
// on j's bisector), I2 the label vertex e had (the edge it continues) -- wrapped run or not.
template <int STRIDE, bool LAB>
__device__ __forceinline__ int clip_cell(const Poly<STRIDE, LAB>& P, int n, double a, double b, double h, bool& changed, double& maxr2,
                                         int j = -1) {
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
    short le = 0;
    if constexpr (LAB) le = P.Lab(e);
    if (s <= e) {                    // the run s .. e inside the array: I1, I2 take its place, the tail moves by 2 - r
        if (r == 1) {
            for (int i = n - 1; i > e; --i) {
                P.X(i + 1) = P.X(i); P.Y(i + 1) = P.Y(i);
                if constexpr (LAB) P.Lab(i + 1) = P.Lab(i);
            }
        } else if (r > 2) {
            for (int i = e + 1; i < n; ++i) {
                P.X(i + 2 - r) = P.X(i); P.Y(i + 2 - r) = P.Y(i);
                if constexpr (LAB) P.Lab(i + 2 - r) = P.Lab(i);
            }
        }
        P.X(s) = i1x; P.Y(s) = i1y;
        P.X(s + 1) = i2x; P.Y(s + 1) = i2y;
        if constexpr (LAB) { P.Lab(s) = (short)j; P.Lab(s + 1) = le; }
    } else {                         // the run wraps (s .. n-1, 0 .. e): the inside vertices e+1 .. s-1 move to the front
        const int keep = n - r;
        for (int i = 0; i < keep; ++i) {
            P.X(i) = P.X(i + e + 1); P.Y(i) = P.Y(i + e + 1);
            if constexpr (LAB) P.Lab(i) = P.Lab(i + e + 1);
        }
        P.X(keep) = i1x; P.Y(keep) = i1y;
        P.X(keep + 1) = i2x; P.Y(keep + 1) = i2y;
        if constexpr (LAB) { P.Lab(keep) = (short)j; P.Lab(keep + 1) = le; }
    }
    return grown;
}

// One row from its table entries to (area, nverts, closed).  survivors: the neighbours the rejection test let through.
// LAB: the polygon left in P carries its labels, and *bound2 receives L^2 (the disc the corners are tested against).
template <bool F64, int STRIDE, bool LAB = false>
__device__ __forceinline__ int area_row(const FitArgs& a, int64_t row, int64_t qid, const float4 qp, const Poly<STRIDE, LAB>& P,
                                        double& area, int& nverts, int& closed, unsigned& survivors, double* bound2 = nullptr) {
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
    if constexpr (LAB) {
        P.Lab(0) = P.Lab(1) = P.Lab(2) = P.Lab(3) = -1;
        *bound2 = L2;
    }
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
            const int got = clip_cell(P, n, ca, cb, 0.5 * rho2, changed, maxr2, j0 + u);
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

}  // namespace

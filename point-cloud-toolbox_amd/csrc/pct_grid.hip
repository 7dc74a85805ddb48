// Uniform cell list build for the neighbour sweep (the search structure that
// stands where the reference builds scipy's cKDTree, pointCloudToolbox.py:74).
//
//   pack      xyz (n,3) f32 -> float4 {x,y,z,index}; finite check; bbox and moments per block, folded by a one-block
//             kernel (sharded handles: k_cull_pack keeps the owned rows and the points near them)
//   hist      cell id per point + per-cell counts of owned / other points (integer atomics)
//   occupancy mean points-per-cell as seen by a point (drives the cell size)
//   scan      exclusive scan of the counts -> cell starts, ordered occupied list
//   scatter   counting sort of the float4 records into cell order, owned points first in each cell
// hist and scatter of the whole-cloud builds are a two-level counting sort with LDS counters only (k_bin_*, below);
// the level passes, slab-owned handles and very large grids keep the per-point atomics of k_hist / k_scatter.
//
// All kernels are HBM/L2 streaming passes over 16 B records with 64-wide waves.  Host side, top to bottom of a build:
//   select_source   where the points come from (GridSource) and that source's pack pass; outlier-trimmed grid box, or
//                   the previous similar cloud's box with this cloud's own box checked later (check_deferred_box)
//   EdgeSearch      cell size by occupancy, warm-started (pct_grid_edge.h: host arithmetic only, tested on the CPU)
//   choose_build    the counting sort or one of the three per-point-atomics builds, once per pass
//   launch_count, launch_scan, launch_place     every launch of a pass, each expression once
//   commit_grid     everything an accepted build leaves in the handle
//   pct_build_grid  the pass loop, the cell budget, the PCT_KNN_AUTO give-up and the (at most two) restarts
// One host synchronisation per accepted build; small results come back through pinned memory the kernels write.
#include "pct_internal.h"
#include "pct_grid_edge.h"

#include <math.h>
#include <stdlib.h>

namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ float wave_min(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// Reduction record of the packing passes (device memory, ctx->red).
struct PackRed {
    int bb[6];                 // min xyz, max xyz as ordered ints
    int bad;                   // a non-finite coordinate was seen
    int g_begin;               // compacted position of the first owned point (cull pass)
    double s[3], ss[3];        // sums / sums of squares of (coordinate - shift): drives the outlier-trimmed grid box
    unsigned long long cnt;    // points accumulated
};

__device__ __forceinline__ int float_order(float f) {
    int i = __float_as_int(f);
    return i >= 0 ? i : i ^ 0x7fffffff;
}
__host__ __device__ __forceinline__ float order_float(int i) {
    int j = i >= 0 ? i : i ^ 0x7fffffff;
#if defined(__HIP_DEVICE_COMPILE__)
    return __int_as_float(j);
#else
    float f;
    memcpy(&f, &j, 4);
    return f;
#endif
}

__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Per-thread accumulator of the packing passes; commit() folds a block into its own PackRed record.
struct PackAcc {
    float mn[3], mx[3];
    double s[3], ss[3];
    int bad;
    unsigned cnt;
    __device__ void init() {
        for (int a = 0; a < 3; ++a) { mn[a] = INFINITY; mx[a] = -INFINITY; s[a] = 0; ss[a] = 0; }
        bad = 0;
        cnt = 0;
    }
    __device__ void add(float x, float y, float z, const float* sh) {
        mn[0] = fminf(mn[0], x); mx[0] = fmaxf(mx[0], x);
        mn[1] = fminf(mn[1], y); mx[1] = fmaxf(mx[1], y);
        mn[2] = fminf(mn[2], z); mx[2] = fmaxf(mx[2], z);
        const double dx = (double)x - sh[0], dy = (double)y - sh[1], dz = (double)z - sh[2];
        s[0] += dx; ss[0] += dx * dx;
        s[1] += dy; ss[1] += dy * dy;
        s[2] += dz; ss[2] += dz * dz;
        ++cnt;
    }
    __device__ void add_box(float x, float y, float z) {     // extent only (no moments)
        mn[0] = fminf(mn[0], x); mx[0] = fmaxf(mx[0], x);
        mn[1] = fminf(mn[1], y); mx[1] = fmaxf(mx[1], y);
        mn[2] = fminf(mn[2], z); mx[2] = fmaxf(mx[2], z);
        ++cnt;
    }
    template <int NW = kBlock / 64>
    __device__ void commit(PackRed* part) {      // this block's record (plain stores); NW = waves per block
        __shared__ float s_mn[NW][3], s_mx[NW][3];
        __shared__ double s_s[NW][3], s_ss[NW][3];
        __shared__ int s_bad[NW];
        __shared__ unsigned s_cnt[NW];
        for (int a = 0; a < 3; ++a) {
            mn[a] = wave_min(mn[a]);
            mx[a] = wave_max(mx[a]);
            s[a] = wave_sum(s[a]);
            ss[a] = wave_sum(ss[a]);
        }
        bad = __any(bad);
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        const int w = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) {
            for (int a = 0; a < 3; ++a) { s_mn[w][a] = mn[a]; s_mx[w][a] = mx[a]; s_s[w][a] = s[a]; s_ss[w][a] = ss[a]; }
            s_bad[w] = bad;
            s_cnt[w] = cnt;
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            const int a = threadIdx.x;
            float lo = s_mn[0][a], hi = s_mx[0][a];
            double t = s_s[0][a], tt = s_ss[0][a];
            for (int i = 1; i < NW; ++i) {
                lo = fminf(lo, s_mn[i][a]); hi = fmaxf(hi, s_mx[i][a]);
                t += s_s[i][a]; tt += s_ss[i][a];
            }
            part->bb[a] = float_order(lo);
            part->bb[3 + a] = float_order(hi);
            part->s[a] = t;
            part->ss[a] = tt;
        }
        if (threadIdx.x == 3) {
            int b = 0;
            unsigned c = 0;
            for (int i = 0; i < NW; ++i) { b |= s_bad[i]; c += s_cnt[i]; }
            part->bad = b;
            part->cnt = c;
        }
    }
};

// second stage of every packing pass: folds the per-block records into the handle's PackRed.  (Atomics from
// every block onto one cache line cost more than the pass itself.)
// carry = 0: nothing of the pass wrote the record directly (k_pack), so its previous content is not read and the
// 128-byte memset in front of the pass -- a launch of its own -- is not needed.
// (NT = threads of the calling block, all of which call: k_pack_final, and k_bin_plan on the speculative build's chain)
template <int NT>
__device__ __forceinline__ void pack_fold(const PackRed* __restrict__ parts, int n_parts, PackRed* __restrict__ red,
                                          PackRed* __restrict__ host_copy, int carry) {
    constexpr int kBlock = NT;
    __shared__ PackRed sh[kBlock / 64];
    int bb[6] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN};
    double s[3] = {0, 0, 0}, ss[3] = {0, 0, 0};
    int bad = 0;
    unsigned long long cnt = 0;
    for (int i = threadIdx.x; i < n_parts; i += kBlock) {
        const PackRed p = parts[i];
        for (int a = 0; a < 3; ++a) {
            bb[a] = min(bb[a], p.bb[a]);
            bb[3 + a] = max(bb[3 + a], p.bb[3 + a]);
            s[a] += p.s[a];
            ss[a] += p.ss[a];
        }
        bad |= p.bad;
        cnt += p.cnt;
    }
    for (int o = 32; o > 0; o >>= 1) {
        for (int a = 0; a < 3; ++a) {
            bb[a] = min(bb[a], __shfl_xor(bb[a], o));
            bb[3 + a] = max(bb[3 + a], __shfl_xor(bb[3 + a], o));
            s[a] += __shfl_xor(s[a], o);
            ss[a] += __shfl_xor(ss[a], o);
        }
        bad |= __shfl_xor(bad, o);
        cnt += __shfl_xor(cnt, o);
    }
    if ((threadIdx.x & 63) == 0) {
        PackRed& w = sh[threadIdx.x >> 6];
        for (int a = 0; a < 6; ++a) w.bb[a] = bb[a];
        for (int a = 0; a < 3; ++a) { w.s[a] = s[a]; w.ss[a] = ss[a]; }
        w.bad = bad;
        w.cnt = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        PackRed out = {};            // red was zeroed before the pass; bad / g_begin may have been set directly
        for (int a = 0; a < 3; ++a) { out.bb[a] = INT32_MAX; out.bb[3 + a] = INT32_MIN; }
        out.bad = carry ? red->bad : 0;
        out.g_begin = carry ? red->g_begin : 0;
        for (int i = 0; i < kBlock / 64; ++i) {
            for (int a = 0; a < 3; ++a) {
                out.bb[a] = min(out.bb[a], sh[i].bb[a]);
                out.bb[3 + a] = max(out.bb[3 + a], sh[i].bb[3 + a]);
                out.s[a] += sh[i].s[a];
                out.ss[a] += sh[i].ss[a];
            }
            out.bad |= sh[i].bad;
            out.cnt += sh[i].cnt;
        }
        *red = out;
        *host_copy = out;
    }
}

__global__ __launch_bounds__(kBlock) void k_pack_final(const PackRed* __restrict__ parts, int n_parts, PackRed* __restrict__ red,
                                                       PackRed* __restrict__ host_copy, int carry) {
    pack_fold<kBlock>(parts, n_parts, red, host_copy, carry);
}

// xyz (n,3) -> float4 {x,y,z,index}; finite check; bbox and moments (fp64, about the origin: the reference
// shifts every cloud by its per-axis maximum, pct:56-57, so coordinates are of the order of the extent).
// four points = twelve consecutive floats = three 16-byte loads per lane, neighbouring lanes adjacent (the scalar
// x / y / z loads of a 12-byte record reach a third of every line each).  VEC needs a 16-byte aligned array.
template <bool VEC>
__device__ __forceinline__ int load_four_points(const float* __restrict__ xyz, int64_t g, int64_t n, float (&v)[12]) {
    const int64_t i0 = g * 4;
    const int have = (int)min((int64_t)4, n - i0);
    if (VEC && have == 4) {
        const float4* q = (const float4*)(xyz + 3 * i0);
        const float4 a = q[0], b = q[1], c = q[2];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
    } else {
        for (int j = 0; j < 12; ++j) v[j] = j < 3 * have ? xyz[3 * i0 + j] : 0.f;
    }
    return have;
}

// (one point per lane and trip: the float4 stores of a wave are 1 KB contiguous; the four-points-per-lane form of the
// cull / slab passes reads better but scatters these stores over 64 lines per instruction -- 16.7 against 12.7 us)
__global__ __launch_bounds__(kBlock) void k_pack(const float* __restrict__ xyz, int64_t n,
                                                 float4* __restrict__ pts4, PackRed* __restrict__ parts,
                                                 unsigned long long* __restrict__ begin_stamp) {
    pct_stamp(begin_stamp);
    const float sh[3] = {0.f, 0.f, 0.f};
    PackAcc acc;
    acc.init();
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        float x = xyz[3 * i + 0], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        const bool ok = isfinite(x) && isfinite(y) && isfinite(z);
        acc.bad |= !ok;
        pts4[i] = make_float4(x, y, z, __int_as_float((int)i));
        if (ok) acc.add(x, y, z, sh);
    }
    acc.commit(parts + blockIdx.x);
}

// bbox / finite check of the rows [begin, end) only (the owned range of a sharded handle)
__global__ __launch_bounds__(kBlock) void k_range_box(const float* __restrict__ xyz, int64_t begin, int64_t end,
                                                      PackRed* __restrict__ parts) {
    const float sh[3] = {0.f, 0.f, 0.f};
    PackAcc acc;
    acc.init();
    for (int64_t i = begin + (int64_t)blockIdx.x * kBlock + threadIdx.x; i < end; i += (int64_t)gridDim.x * kBlock) {
        float x = xyz[3 * i + 0], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        const bool ok = isfinite(x) && isfinite(y) && isfinite(z);
        acc.bad |= !ok;
        if (ok) acc.add(x, y, z, sh);
    }
    acc.commit(parts + blockIdx.x);
}

// moments of the packed points inside a box (outlier trimming of the grid box)
struct Box3 { float lo[3], hi[3]; };
__device__ __forceinline__ bool in_box(const Box3& b, float x, float y, float z) {
    return x >= b.lo[0] && x <= b.hi[0] && y >= b.lo[1] && y <= b.hi[1] && z >= b.lo[2] && z <= b.hi[2];
}
__global__ __launch_bounds__(kBlock) void k_box_stats(const float4* __restrict__ pts4, int64_t n, Box3 box, Box3 shift,
                                                      PackRed* __restrict__ parts) {
    PackAcc acc;
    acc.init();
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const float4 p = pts4[i];
        if (in_box(box, p.x, p.y, p.z)) acc.add(p.x, p.y, p.z, shift.lo);
    }
    acc.commit(parts + blockIdx.x);
}

// ---- sharded handles: keep only the points near the owned range ------------------------------------------------
// The candidate set of a handle that owns rows [q_begin, q_end) is the whole cloud, but only the points inside
// the owned rows' bounding box plus a margin can be neighbours (the sweep verifies that per query, see
// pct_grid::lim_lo).  One pass: the owned rows go to the front of the packed array in their own order, the kept
// others behind them in whatever order the blocks arrive (one counter increment per 4096-row chunk).
constexpr int kCullBlock = 512;          // (fewer chunks = fewer ticket atomics on one address, the pass's bound)
constexpr int kCullChunk = kCullBlock * 16;

// Ownership by slab (pct_set_query_slab): bin of a coordinate along the cut axis.  Every rank evaluates this very
// expression on the same bytes (the library is built with -ffp-contract=off), in the histogram and in the pack alike.
constexpr int kSlabBins = 4096;
struct SlabCut { int axis, bin_lo, bin_hi; float x0, inv; };
__device__ __forceinline__ int slab_bin(float x, float x0, float inv) {
    const int b = (int)((x - x0) * inv);
    return min(max(b, 0), kSlabBins - 1);
}

// bounding box / finite check of the whole cloud, for the slab cut (count and moments are not needed)
template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_cloud_box(const float* __restrict__ xyz, int64_t n, PackRed* __restrict__ parts) {
    PackAcc acc;
    acc.init();
    const int64_t groups = (n + 3) / 4;
    for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += (int64_t)gridDim.x * kBlock) {
        float v[12];
        const int have = load_four_points<VEC>(xyz, g, n, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < have) {
                const bool ok = isfinite(v[3 * j]) && isfinite(v[3 * j + 1]) && isfinite(v[3 * j + 2]);
                acc.bad |= !ok;
                if (ok) acc.add_box(v[3 * j], v[3 * j + 1], v[3 * j + 2]);
            }
        }
    }
    acc.commit(parts + blockIdx.x);
}

// (few, large blocks: every block ends with one global atomic per non-empty bin)
constexpr int kSlabHistBlock = 1024;
template <bool VEC>
__global__ __launch_bounds__(kSlabHistBlock) void k_slab_hist(const float* __restrict__ xyz, int64_t n, int axis, float x0, float inv,
                                                              unsigned* __restrict__ hist) {
    constexpr int kBlock = kSlabHistBlock;
    __shared__ unsigned s_h[kSlabBins];
    for (int i = threadIdx.x; i < kSlabBins; i += kBlock) s_h[i] = 0;
    __syncthreads();
    const int64_t groups = (n + 3) / 4;
    for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += (int64_t)gridDim.x * kBlock) {
        float v[12];
        const int have = load_four_points<VEC>(xyz, g, n, v);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < have) atomicAdd(&s_h[slab_bin(axis == 0 ? v[3 * j] : axis == 1 ? v[3 * j + 1] : v[3 * j + 2], x0, inv)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kSlabBins; i += kBlock)
        if (s_h[i]) atomicAdd(&hist[i], s_h[i]);
}

// cuts: part p owns the bins [cut[p], cut[p+1]) where cut[p] = the first bin with floor(p n / parts) points below it
__global__ __launch_bounds__(kBlock) void k_slab_cut(const unsigned* __restrict__ hist, long long n, int parts, int* __restrict__ cut,
                                                     long long* __restrict__ counts) {
    __shared__ long long s_cum[kSlabBins + 1];
    __shared__ long long s_part[kBlock];
    __shared__ int s_cut[PCT_SLAB_PARTS_MAX + 1];
    constexpr int per = kSlabBins / kBlock;
    long long mine = 0;
    for (int j = 0; j < per; ++j) mine += hist[threadIdx.x * per + j];
    s_part[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = 0;
        for (int t = 0; t < kBlock; ++t) { const long long c = s_part[t]; s_part[t] = run; run += c; }
    }
    __syncthreads();
    long long run = s_part[threadIdx.x];
    for (int j = 0; j < per; ++j) { s_cum[threadIdx.x * per + j] = run; run += hist[threadIdx.x * per + j]; }
    if (threadIdx.x == kBlock - 1) s_cum[kSlabBins] = run;
    __syncthreads();
    if ((int)threadIdx.x <= parts) {
        const int p = threadIdx.x;
        int b = kSlabBins;
        if (p < parts) {
            const long long want = (long long)p * n / parts;
            int lo = 0, hi = kSlabBins;                // smallest b with cum[b] >= want (cum is non-decreasing)
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_cum[mid] >= want) hi = mid; else lo = mid + 1; }
            b = lo;
        }
        s_cut[p] = b;
        cut[p] = b;
    }
    __syncthreads();
    if ((int)threadIdx.x < parts) counts[threadIdx.x] = s_cum[s_cut[threadIdx.x + 1]] - s_cum[s_cut[threadIdx.x]];
}

// SLAB: the owned points are those of the slab (compacted to the front through a second counter, in whatever order the
// blocks arrive: the public index rides in w); otherwise the rows [q_begin, q_end), in their own order.
template <bool SLAB, bool VEC>
__global__ __launch_bounds__(kCullBlock) void k_cull_pack(const float* __restrict__ xyz, int64_t n, Box3 box, int64_t q_begin,
                                                      int64_t q_end, SlabCut cut, float4* __restrict__ pts4, unsigned* __restrict__ kept_others,
                                                      PackRed* __restrict__ red, PackRed* __restrict__ parts) {
    constexpr int kBlock = kCullBlock, NW = kCullBlock / 64;
    __shared__ int s_cnt[16][NW];
    __shared__ int s_own[16][NW];
    __shared__ int s_base, s_own_base;
    const float sh[3] = {0.f, 0.f, 0.f};
    PackAcc acc;
    acc.init();
    const int64_t base = (int64_t)blockIdx.x * kCullChunk;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t n_owned = q_end - q_begin;
    float px[16], py[16], pz[16];
    unsigned keep_bits = 0, own_bits = 0;
    int bad = 0;
    // slot r of a thread = point 4 (chunk's first group + (r / 4) kBlock + thread) + r % 4: four consecutive points per
    // 48-byte load (load_four_points)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        float v[12];
        load_four_points<VEC>(xyz, base / 4 + rr * kBlock + threadIdx.x, n, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) { px[4 * rr + j] = v[3 * j]; py[4 * rr + j] = v[3 * j + 1]; pz[4 * rr + j] = v[3 * j + 2]; }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t i = base + 4 * ((r >> 2) * kBlock + threadIdx.x) + (r & 3);
        bool keep = false, own = false;
        if (i < n) {
            bad |= !(isfinite(px[r]) && isfinite(py[r]) && isfinite(pz[r]));
            if (SLAB) {
                const int b = slab_bin(cut.axis == 0 ? px[r] : cut.axis == 1 ? py[r] : pz[r], cut.x0, cut.inv);
                own = b >= cut.bin_lo && b < cut.bin_hi;
                keep = !own && in_box(box, px[r], py[r], pz[r]);
            } else if (i >= q_begin && i < q_end) {
                pts4[i - q_begin] = make_float4(px[r], py[r], pz[r], __int_as_float((int)i));
                acc.add(px[r], py[r], pz[r], sh);
            } else {
                keep = in_box(box, px[r], py[r], pz[r]);
            }
        }
        keep_bits |= keep ? 1u << r : 0u;
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_cnt[r][w] = (int)__popcll(m);
        if (SLAB) {
            own_bits |= own ? 1u << r : 0u;
            const unsigned long long mo = __ballot(own);
            if (lane == 0) s_own[r][w] = (int)__popcll(mo);
        }
    }
    __syncthreads();
    // exclusive prefix over (round, wave) by one wave per list, one counter increment per chunk
    if (w == 0 || (SLAB && w == 1)) {
        int* list = w == 0 ? &s_cnt[0][0] : &s_own[0][0];
        constexpr int per = 16 * NW / 64;
        int c[per], mine = 0;
#pragma unroll
        for (int j = 0; j < per; ++j) { c[j] = list[lane * per + j]; mine += c[j]; }
        int incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
        int run = incl - mine;
#pragma unroll
        for (int j = 0; j < per; ++j) { list[lane * per + j] = run; run += c[j]; }
        const int total = __shfl(incl, 63);
        if (lane == 0) {
            if (w == 0) s_base = total ? (int)atomicAdd(kept_others, (unsigned)total) : 0;
            else s_own_base = total ? (int)atomicAdd(kept_others + 32, (unsigned)total) : 0;       // (its own 128-byte line)
        }
    }
    __syncthreads();
    const int64_t out0 = n_owned + s_base;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const bool keep = (keep_bits >> r) & 1u;
        const unsigned long long m = __ballot(keep);
        const int64_t i = base + 4 * ((r >> 2) * kBlock + threadIdx.x) + (r & 3);
        if (keep) {
            const int64_t at = out0 + s_cnt[r][w] + (int)__popcll(m & ((1ull << lane) - 1ull));
            if (!SLAB || at < n) pts4[at] = make_float4(px[r], py[r], pz[r], __int_as_float((int)i));
            acc.add(px[r], py[r], pz[r], sh);
        }
        if (SLAB) {
            const bool own = (own_bits >> r) & 1u;
            const unsigned long long mo = __ballot(own);
            if (own) {
                const int64_t at = (int64_t)s_own_base + s_own[r][w] + (int)__popcll(mo & ((1ull << lane) - 1ull));
                if (at < n_owned) pts4[at] = make_float4(px[r], py[r], pz[r], __int_as_float((int)i));   // (guard: a cut that no longer fits the buffer is reported by the host)
                acc.add(px[r], py[r], pz[r], sh);
            }
        }
    }
    if (__any(bad) && lane == 0) atomicOr(&red->bad, 1);
    acc.commit<NW>(parts + blockIdx.x);
}

// double4 variant: native float64 coordinates ride along (w = index).
__global__ __launch_bounds__(kBlock) void k_pack_f64(const double* __restrict__ xyz, int64_t n,
                                                     double4* __restrict__ pts4d, float* __restrict__ xyz32) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        double x = xyz[3 * i + 0], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        pts4d[i] = make_double4(x, y, z, (double)i);
        xyz32[3 * i + 0] = (float)x;   // tree coordinates are float32-rounded (pct:74)
        xyz32[3 * i + 1] = (float)y;
        xyz32[3 * i + 2] = (float)z;
    }
}

__device__ __forceinline__ int cell_coord(double x, double o, double inv, int n) {
    int c = (int)floor((x - o) * inv);
    return min(max(c, 0), n - 1);
}

// Cell id per point and per-cell populations.  Points this handle owns (public
// index in [q_begin, q_end), the multi-GPU shard) and the others are counted
// separately: inside a cell the owned points are stored first, so that work
// items and neighbour-table rows exist for owned queries only.  The value an
// integer atomic returns is the point's arrival rank in its class -- the
// scatter then needs no second atomic pass.
__global__ __launch_bounds__(kBlock) void k_hist(const float4* __restrict__ pts4, int64_t n, pct_grid g, int q_begin, int q_end,
                                                 const float* __restrict__ own_want, float own_lo, float own_hi, int skip_outside,
                                                 int* __restrict__ cell_of, int* __restrict__ rank_of,
                                                 int* __restrict__ cell_own, int* __restrict__ cell_oth) {
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float4 p = pts4[i];
    if (skip_outside) {
        // fast level pass over a sub-box: a point outside the box would only be clamped into a boundary cell that no
        // owned stencil touches -- and a million of them into the same few cells serialise the atomics.  Leave it out.
        const double fx = floor(((double)p.x - g.ox) * g.inv_cell), fy = floor(((double)p.y - g.oy) * g.inv_cell),
                     fz = floor(((double)p.z - g.oz) * g.inv_cell);
        if (fx < 0 || fx >= g.nx || fy < 0 || fy >= g.ny || fz < 0 || fz >= g.nz) {
            cell_of[i] = -1;
            return;
        }
    }
    int cx = cell_coord((double)p.x, g.ox, g.inv_cell, g.nx);
    int cy = cell_coord((double)p.y, g.oy, g.inv_cell, g.ny);
    int cz = cell_coord((double)p.z, g.oz, g.inv_cell, g.nz);
    int c = (cz * g.ny + cy) * g.nx + cx;
    cell_of[i] = c;
    // level passes (pct_levels.hip) own the still unanswered points whose wanted cell edge (log2) lies in a band
    const float want = own_want ? own_want[__float_as_int(p.w)] : 0.f;
    const bool owned = own_want ? (want >= own_lo && want < own_hi) : (i >= q_begin && i < q_end);
    if (owned) {
        rank_of[i] = atomicAdd(&cell_own[c], 1);
    } else {
        // fast level pass: a cell that already holds far more candidates than the sweep can stage overflows every
        // stencil it is part of (those queries go to another pass whatever happens), so further candidates in it are
        // dead weight -- and a hundred thousand of them on one counter serialise (~88 atomics/us per address)
        if (skip_outside && __builtin_nontemporal_load(&cell_oth[c]) > 2048) {
            cell_of[i] = -1;
            return;
        }
        rank_of[i] = atomicAdd(&cell_oth[c], 1) | (int)0x80000000;
    }
}

// k_pack folded in (a handle fed a stream of similar clouds builds on the previous cloud's box without waiting for the new
// one: no float4 copy of the cloud is needed before the histogram): reads the caller's xyz rows, bins them, and leaves the
// bounding box / moments / finite check of the cloud as per-block records for k_pack_final.  Whole-cloud handles only
// (every point owned or not by its index; no level pass, no sub-box).
__global__ __launch_bounds__(kBlock) void k_hist_raw(const float* __restrict__ xyz, int64_t n, pct_grid g, int q_begin, int q_end,
                                                     int* __restrict__ cell_of, int* __restrict__ rank_of,
                                                     int* __restrict__ cell_own, int* __restrict__ cell_oth, PackRed* __restrict__ parts) {
    const float sh[3] = {0.f, 0.f, 0.f};
    PackAcc acc;
    acc.init();
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) {
        const float x = xyz[3 * i + 0], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        const bool ok = isfinite(x) && isfinite(y) && isfinite(z);
        acc.bad |= !ok;
        if (ok) acc.add(x, y, z, sh);
        // (a non-finite row makes the call fail at its next read-back; it is binned at the origin meanwhile)
        const int cx = cell_coord(ok ? (double)x : g.ox, g.ox, g.inv_cell, g.nx);
        const int cy = cell_coord(ok ? (double)y : g.oy, g.oy, g.inv_cell, g.ny);
        const int cz = cell_coord(ok ? (double)z : g.oz, g.oz, g.inv_cell, g.nz);
        const int c = (cz * g.ny + cy) * g.nx + cx;
        cell_of[i] = c;
        if (i >= q_begin && i < q_end) rank_of[i] = atomicAdd(&cell_own[c], 1);
        else rank_of[i] = atomicAdd(&cell_oth[c], 1) | (int)0x80000000;
    }
    if (parts) acc.commit(parts + blockIdx.x);
}

// The same for the later passes of the density-adaptive sweep (pct_levels.hip), whose cells are sized for ONE band of
// densities while every point is still a candidate: the denser part of the cloud then piles into a handful of cells
// and its atomics serialise at the memory side (~88 per microsecond and address: a 1/r^2 scan spent 1-2 ms per pass
// there).  These passes read the points in the cell order of the first pass, so the lanes of a wave mostly share
// their cell: one atomic per distinct (cell, class) of the wave, ranks handed out by bit counts.
__global__ __launch_bounds__(kBlock) void k_hist_agg(const float4* __restrict__ pts4, int64_t n, pct_grid g,
                                                     const float* __restrict__ own_want, float own_lo, float own_hi, int skip_outside,
                                                     int* __restrict__ cell_of, int* __restrict__ rank_of,
                                                     int* __restrict__ cell_own, int* __restrict__ cell_oth) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int key = -1;                       // 2 * cell + (owned ? 1 : 0); -1 = not counted
    if (i < n) {
        const float4 p = pts4[i];
        bool inside = true;
        if (skip_outside) {
            const double fx = floor(((double)p.x - g.ox) * g.inv_cell), fy = floor(((double)p.y - g.oy) * g.inv_cell),
                         fz = floor(((double)p.z - g.oz) * g.inv_cell);
            inside = !(fx < 0 || fx >= g.nx || fy < 0 || fy >= g.ny || fz < 0 || fz >= g.nz);
        }
        if (inside) {
            const int cx = cell_coord((double)p.x, g.ox, g.inv_cell, g.nx);
            const int cy = cell_coord((double)p.y, g.oy, g.inv_cell, g.ny);
            const int cz = cell_coord((double)p.z, g.oz, g.inv_cell, g.nz);
            const int c = (cz * g.ny + cy) * g.nx + cx;
            const float w = own_want[__float_as_int(p.w)];
            const bool owned = w >= own_lo && w < own_hi;
            // a cell that already holds far more candidates than the sweep can stage overflows every stencil it is
            // part of: further candidates in it are dead weight (its count stays above the staging capacity)
            if (owned || !skip_outside || __builtin_nontemporal_load(&cell_oth[c]) <= 2048) key = 2 * c + (owned ? 1 : 0);
        }
    }
    int rank = 0;
    unsigned long long todo = __builtin_amdgcn_ballot_w64(key >= 0);
    while (todo) {
        const int leader = (int)__builtin_ctzll(todo);
        const int k0 = __builtin_amdgcn_readlane(key, leader);
        const unsigned long long same = __builtin_amdgcn_ballot_w64(key == k0);
        int base = 0;
        if (lane == leader) base = atomicAdd((k0 & 1) ? &cell_own[k0 >> 1] : &cell_oth[k0 >> 1], (int)__popcll(same));
        base = __builtin_amdgcn_readlane(base, leader);
        if (key == k0) rank = base + (int)__popcll(same & ((1ull << lane) - 1ull));
        todo &= ~same;
    }
    if (i < n) {
        cell_of[i] = key < 0 ? -1 : key >> 1;
        if (key >= 0) rank_of[i] = (key & 1) ? rank : (rank | (int)0x80000000);
    }
}

// ---- triple exclusive scan over the cells ---------------------------------
//   x: all points      -> cell_start   (position of the cell in the sorted cloud)
//   y: work items      -> item rank    (ceil(owned / items_q) per cell)
//   z: owned points    -> own_start    (first neighbour-table row of the cell)
constexpr int kScanItems = 8;                    // per thread
constexpr int kScanTile = kBlock * kScanItems;   // 2048 cells per block

// (x, y, z are scanned; w just counts the non-empty cells along)
__device__ __forceinline__ int4 add3(int4 a, int4 b) { return make_int4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

__device__ __forceinline__ int4 cell_counts(const int* __restrict__ own, const int* __restrict__ oth, int64_t c, int64_t ncell, int items_q) {
    if (c >= ncell) return make_int4(0, 0, 0, 0);
    const int o = own[c];
    const int t = o + (oth ? oth[c] : 0);
    return make_int4(t, (o + items_q - 1) / items_q, o, t > 0 ? 1 : 0);
}

// ... of a cell with o owned and x other points (the counting sort holds the counters in LDS)
__device__ __forceinline__ int4 count_record(int o, int x, int items_q) {
    const int t = o + x;
    return make_int4(t, (o + items_q - 1) / items_q, o, t > 0 ? 1 : 0);
}

// first pass: per-tile sums; also accumulates sum_c owned_c * count_c (= sum over the owned points of the
// population of their own cell), the statistic the cell-size loop steers on
__global__ __launch_bounds__(kBlock) void k_scan_sums(const int* __restrict__ own, const int* __restrict__ oth, int64_t ncell, int items_q,
                                                      int4* __restrict__ tmp, unsigned long long* __restrict__ sq_part) {
    __shared__ int4 sh[kBlock / 64];
    __shared__ unsigned long long shq[kBlock / 64];
    unsigned long long sq = 0;
    int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    int4 v = make_int4(0, 0, 0, 0);
    for (int j = 0; j < kScanItems; ++j) {
        const int4 x = cell_counts(own, oth, base + j, ncell, items_q);
        v = add3(v, x);
        sq += (unsigned long long)x.z * (unsigned)x.x;       // owned points x population of their cell
    }
    for (int o = 32; o > 0; o >>= 1) {
        v.x += __shfl_xor(v.x, o); v.y += __shfl_xor(v.y, o); v.z += __shfl_xor(v.z, o); v.w += __shfl_xor(v.w, o);
        sq += __shfl_xor(sq, o);
    }
    if ((threadIdx.x & 63) == 0) {
        sh[threadIdx.x >> 6] = v;
        shq[threadIdx.x >> 6] = sq;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int4 t = make_int4(0, 0, 0, 0);
        unsigned long long q = 0;
        for (int i = 0; i < kBlock / 64; ++i) { t = add3(t, sh[i]); q += shq[i]; }
        tmp[blockIdx.x] = t;
        sq_part[blockIdx.x] = q;        // per-tile partial: no same-address atomics (they serialise at ~88/us)
    }
}

// single block: exclusive scan of the per-tile sums; totals to tmp[nblk]
struct ScanTotals { unsigned long long sumsq; int4 tot; };

// (also clears the sweep's eight statistics words and its redo count, which saves the sweep a 64-byte memset launch)
__global__ __launch_bounds__(1024) void k_scan_tiles(int4* __restrict__ tmp, int nblk, const unsigned long long* __restrict__ sq_part,
                                                      ScanTotals* __restrict__ host_copy, unsigned long long* __restrict__ zero8) {
    __shared__ int4 sh[1024];
    if (zero8 && threadIdx.x < 8) zero8[threadIdx.x] = 0ull;
    __shared__ int4 carry;
    __shared__ unsigned long long shq[16];
    {   // sum of the per-tile sum-of-squares partials
        unsigned long long q = 0;
        for (int i = threadIdx.x; i < nblk; i += 1024) q += sq_part[i];
        for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
        if ((threadIdx.x & 63) == 0) shq[threadIdx.x >> 6] = q;
        __syncthreads();
        if (threadIdx.x == 0) { unsigned long long t = 0; for (int i = 0; i < 16; ++i) t += shq[i]; host_copy->sumsq = t; }
    }
    if (threadIdx.x == 0) carry = make_int4(0, 0, 0, 0);
    __syncthreads();
    for (int base = 0; base < nblk; base += 1024) {
        int i = base + threadIdx.x;
        int4 v = i < nblk ? tmp[i] : make_int4(0, 0, 0, 0);
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            int4 a = make_int4(0, 0, 0, 0);
            if ((int)threadIdx.x >= o) a = sh[threadIdx.x - o];
            __syncthreads();
            sh[threadIdx.x] = add3(sh[threadIdx.x], a);
            __syncthreads();
        }
        int4 incl = sh[threadIdx.x];
        int4 c = carry;
        if (i < nblk) tmp[i] = make_int4(c.x + incl.x - v.x, c.y + incl.y - v.y, c.z + incl.z - v.z, 0);
        __syncthreads();
        if (threadIdx.x == 1023) carry = add3(c, incl);
        __syncthreads();
    }
    if (threadIdx.x == 0) { tmp[nblk] = carry; host_copy->tot = carry; }
}

__global__ __launch_bounds__(kBlock) void k_scan_apply(const int* __restrict__ own, const int* __restrict__ oth, int64_t ncell, int items_q,
                                                       const int4* __restrict__ tmp, int* __restrict__ cell_start,
                                                       int* __restrict__ own_start, int2* __restrict__ items) {
    __shared__ int4 sh[kBlock];
    int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    int4 x[kScanItems];
    int4 v = make_int4(0, 0, 0, 0);
    for (int j = 0; j < kScanItems; ++j) {
        x[j] = cell_counts(own, oth, base + j, ncell, items_q);
        v = add3(v, x[j]);
    }
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < kBlock; o <<= 1) {
        int4 a = make_int4(0, 0, 0, 0);
        if ((int)threadIdx.x >= o) a = sh[threadIdx.x - o];
        __syncthreads();
        sh[threadIdx.x] = add3(sh[threadIdx.x], a);
        __syncthreads();
    }
    const int4 off = tmp[blockIdx.x];
    int s = off.x + sh[threadIdx.x].x - v.x;
    int r = off.y + sh[threadIdx.x].y - v.y;
    int w = off.z + sh[threadIdx.x].z - v.z;
    for (int j = 0; j < kScanItems; ++j) {
        int64_t c = base + j;
        if (c < ncell) {
            cell_start[c] = s;
            own_start[c] = w;
            for (int ch = 0; ch < x[j].y; ++ch) items[r++] = make_int2((int)c, ch);
            s += x[j].x;
            w += x[j].z;
        }
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == kBlock - 1) { cell_start[ncell] = s; own_start[ncell] = w; }
}

// counting-sort scatter, owned points first inside every cell; also records for every owned point its
// neighbour-table row and for every row its sorted position
__global__ __launch_bounds__(kBlock) void k_scatter(const float4* __restrict__ pts4, const int* __restrict__ cell_of,
                                                    const int* __restrict__ cell_start, const int* __restrict__ cell_own,
                                                    const int* __restrict__ own_start, const int* __restrict__ rank_of,
                                                    int64_t n, int g_begin, float4* __restrict__ sorted4,
                                                    int* __restrict__ row_of, int* __restrict__ owned_pos,
                                                    const double4* __restrict__ pts4d, double4* __restrict__ sorted4d) {
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int c = cell_of[i];
    if (c < 0) return;                  // left out of this pass's cell list
    const int r = rank_of[i];
    int pos, row;
    if (r >= 0) {
        pos = cell_start[c] + r;
        row = own_start[c] + r;
        owned_pos[row] = pos;
        row_of[i - g_begin] = row;      // owned points are contiguous in the packed array
    } else {
        pos = cell_start[c] + cell_own[c] + (r & 0x7fffffff);
    }
    const float4 p = pts4[i];
    sorted4[pos] = p;
    if (pts4d) sorted4d[pos] = pts4d[__float_as_int(p.w)];      // float64 records stay in public order (never culled)
}

// ... from the caller's xyz rows (k_hist_raw's counterpart)
__global__ __launch_bounds__(kBlock) void k_scatter_raw(const float* __restrict__ xyz, const int* __restrict__ cell_of,
                                                        const int* __restrict__ cell_start, const int* __restrict__ cell_own,
                                                        const int* __restrict__ own_start, const int* __restrict__ rank_of,
                                                        int64_t n, int g_begin, float4* __restrict__ sorted4,
                                                        int* __restrict__ row_of, int* __restrict__ owned_pos,
                                                        const double4* __restrict__ pts4d, double4* __restrict__ sorted4d) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int c = cell_of[i];
    const int r = rank_of[i];
    int pos;
    if (r >= 0) {
        pos = cell_start[c] + r;
        const int row = own_start[c] + r;
        owned_pos[row] = pos;
        row_of[i - g_begin] = row;
    } else {
        pos = cell_start[c] + cell_own[c] + (r & 0x7fffffff);
    }
    sorted4[pos] = make_float4(xyz[3 * i + 0], xyz[3 * i + 1], xyz[3 * i + 2], __int_as_float((int)i));
    if (pts4d) sorted4d[pos] = pts4d[i];
}

// ---- two-level counting sort with LDS counters only (k_bin_*) -----------------------------------------------------
// The whole-cloud builds (every grid point is owned or not by its public index: the caller's rows, the full pack, the
// range-culled pack) sort without per-point global atomics.  A bucket is a contiguous range of 2^shift cell ids, so
// bucket order followed by cell order inside a bucket is the global cell order and a bucket's points occupy one
// contiguous range of sorted4.
//   k_bin_count    tile of input rows -> per-bucket counts in LDS -> one row of the [tile][bucket] matrix
//                  (+ the PackAcc record of the speculative build, one per tile, folded by a spare block of k_bin_cells)
//   k_bin_colscan  exclusive scan down every column of the matrix, column totals
//   k_bin_plan     bucket starts; work list of (bucket, chunk) items: a bucket above `chunk` records is shared by
//                  several blocks, the way occ feeds the sweep
//   k_bin_scatter  the same tiles again: LDS cursors start at bucket start + matrix entry, every record goes to its
//                  bucket's range of bin_rec (runs of one tile and bucket are adjacent: the L2 combines the stores)
//   k_bin_cells    per item: per-cell, per-class counts in LDS -> cell_own / cell_oth.  The only item of a bucket stores
//                  all its cells (zeros too: no clearing fill); the items of a shared bucket add their non-zero counts
//                  (one atomic per non-empty (item, cell, class)) and keep the value returned, their run's offset.
//                  Also the bucket's scan record (k_scan_sums' work: a bucket is a scan tile): by the only item from its
//                  LDS counters, by the item of a shared bucket that takes the bucket's last ticket from the final counts
//   (k_scan_tiles over the per-bucket records, event: as for every build)
//   k_bin_place    per item: the triple scan inside its bucket (k_scan_apply's work) from cell_own / cell_oth and the
//                  bucket's bases -> LDS cursors (+ the run offset in a shared bucket); the first item of a bucket writes
//                  cell_start / own_start / occ for its cells; every record to its place in sorted4; owned_pos / sorted4d
//                  along; row_of on first need (k_bin_row_of)
// Kernel boundaries are the only ordering between blocks, but for one last-block-out ticket per shared bucket in
// k_bin_cells (nobody waits: the block that finds itself last does the bucket's reduction).
constexpr int kBinBlock = 256;        // fine level: one block per work item
constexpr int kBinWide = 1024;        // coarse level: one block per tile, four rows per thread in flight
// (kBinTileRows, kBinMaxTiles, kBinMaxBuckets, kBinMaxCounters, kBinMinChunk, BinShape and bin_shape: pct_grid_edge.h)

// the cell of a record: k_hist_raw's expression (a non-finite row is binned at the origin)
__device__ __forceinline__ int bin_cell(float x, float y, float z, const pct_grid& g) {
    const bool ok = isfinite(x) && isfinite(y) && isfinite(z);
    const int cx = cell_coord(ok ? (double)x : g.ox, g.ox, g.inv_cell, g.nx);
    const int cy = cell_coord(ok ? (double)y : g.oy, g.oy, g.inv_cell, g.ny);
    const int cz = cell_coord(ok ? (double)z : g.oz, g.oz, g.inv_cell, g.nz);
    return (cz * g.ny + cy) * g.nx + cx;
}

// RAW: rows of the caller's xyz array (public index = row); otherwise float4 records with the public index in w
template <bool RAW>
__device__ __forceinline__ float4 bin_load(const float* __restrict__ xyz, const float4* __restrict__ pts4, int64_t i) {
    if (RAW) return make_float4(xyz[3 * i + 0], xyz[3 * i + 1], xyz[3 * i + 2], __int_as_float((int)i));
    return pts4[i];
}

template <bool RAW>
__global__ __launch_bounds__(kBinWide) void k_bin_count(const float* __restrict__ xyz, const float4* __restrict__ pts4, int64_t n,
                                                         int tile_rows, pct_grid g, int shift, int nb,
                                                         unsigned* __restrict__ mat, PackRed* __restrict__ parts,
                                                         unsigned long long* __restrict__ begin_stamp) {
    pct_stamp(begin_stamp);
    __shared__ unsigned s_cnt[kBinMaxBuckets];
    for (int b = threadIdx.x; b < nb; b += kBinWide) s_cnt[b] = 0;
    __syncthreads();
    const float sh[3] = {0.f, 0.f, 0.f};
    PackAcc acc;
    acc.init();
    const int64_t r0 = (int64_t)blockIdx.x * tile_rows, r1 = min(n, r0 + tile_rows);
    for (int64_t base = r0 + threadIdx.x; base < r1; base += 4 * kBinWide) {
        float4 p[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (base + j * kBinWide < r1) p[j] = bin_load<RAW>(xyz, pts4, base + j * kBinWide);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (base + j * kBinWide >= r1) continue;
            if (parts) {
                const bool ok = isfinite(p[j].x) && isfinite(p[j].y) && isfinite(p[j].z);
                acc.bad |= !ok;
                if (ok) acc.add(p[j].x, p[j].y, p[j].z, sh);
            }
            atomicAdd(&s_cnt[bin_cell(p[j].x, p[j].y, p[j].z, g) >> shift], 1u);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < nb; b += kBinWide) mat[(size_t)blockIdx.x * nb + b] = s_cnt[b];
    if (parts) acc.commit<kBinWide / 64>(parts + blockIdx.x);
}

// 16 columns x 64 groups of tiles per block (a thread holds at most kBinMaxTiles / 64 entries: all of them in flight
// at once): mat[t][b] becomes the number of bucket b's records in the tiles before t
constexpr int kBinScanCols = 16, kBinScanGroups = 64, kBinScanPer = kBinMaxTiles / kBinScanGroups;
__global__ __launch_bounds__(kBinScanCols * kBinScanGroups) void k_bin_colscan(unsigned* __restrict__ mat, int ntiles, int nb, unsigned* __restrict__ tot) {
    __shared__ unsigned s[kBinScanGroups][kBinScanCols];
    const int lane = threadIdx.x % kBinScanCols, grp = threadIdx.x / kBinScanCols;
    const int col = blockIdx.x * kBinScanCols + lane;
    const int per = (ntiles + kBinScanGroups - 1) / kBinScanGroups;
    const int t0 = grp * per;
    unsigned v[kBinScanPer], sum = 0;
#pragma unroll
    for (int j = 0; j < kBinScanPer; ++j) {
        v[j] = (j < per && t0 + j < ntiles && col < nb) ? mat[(size_t)(t0 + j) * nb + col] : 0u;
        sum += v[j];
    }
    s[grp][lane] = sum;
    __syncthreads();
    unsigned run = 0;
    for (int q = 0; q < grp; ++q) run += s[q][lane];
    if (col >= nb) return;
#pragma unroll
    for (int j = 0; j < kBinScanPer; ++j) {
        if (j < per && t0 + j < ntiles) mat[(size_t)(t0 + j) * nb + col] = run;
        run += v[j];
    }
    if (grp == kBinScanGroups - 1) tot[col] = run;
}

// plan words: [0] work items  [1] items of shared buckets  [2] shared buckets; bstart = plan + 16 (nb + 1 words)
// item = {bucket, first record, end of its records, slot of its run offsets or -1 for the only item of its bucket}
__global__ __launch_bounds__(1024) void k_bin_plan(const unsigned* __restrict__ tot, int nb, int chunk, int* __restrict__ plan,
                                                   int4* __restrict__ items) {
    __shared__ int4 sh[1024];
    constexpr int per = kBinMaxBuckets / 1024;
    int4 v[per];
    int4 mine = make_int4(0, 0, 0, 0);
    for (int j = 0; j < per; ++j) {
        const int b = threadIdx.x * per + j;
        const int c = b < nb ? (int)tot[b] : 0;
        const int ni = b < nb ? max(1, (c + chunk - 1) / chunk) : 0;        // an empty bucket's item stores its zeros
        v[j] = make_int4(c, ni, ni > 1 ? ni : 0, ni > 1 ? 1 : 0);
        mine = add3(mine, v[j]);
    }
    sh[threadIdx.x] = mine;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        int4 a = make_int4(0, 0, 0, 0);
        if ((int)threadIdx.x >= o) a = sh[threadIdx.x - o];
        __syncthreads();
        sh[threadIdx.x] = add3(sh[threadIdx.x], a);
        __syncthreads();
    }
    int4 run = make_int4(sh[threadIdx.x].x - mine.x, sh[threadIdx.x].y - mine.y, sh[threadIdx.x].z - mine.z, 0);
    int* bstart = plan + 16;
    for (int j = 0; j < per; ++j) {
        const int b = threadIdx.x * per + j;
        if (b < nb) {
            bstart[b] = run.x;
            for (int ch = 0; ch < v[j].y; ++ch)
                items[run.y + ch] = make_int4(b, run.x + ch * chunk, run.x + min(v[j].x, (ch + 1) * chunk), v[j].z ? run.z + ch : -1);
        }
        run = add3(run, v[j]);
    }
    if (threadIdx.x == 1023) {
        bstart[nb] = run.x;
        plan[0] = run.y;
        plan[1] = run.z;
        plan[2] = sh[1023].w;
    }
}

template <bool RAW>
__global__ __launch_bounds__(kBinWide) void k_bin_scatter(const float* __restrict__ xyz, const float4* __restrict__ pts4, int64_t n,
                                                           int tile_rows, pct_grid g, int shift, int nb, int chunk,
                                                           const unsigned* __restrict__ mat, const int* __restrict__ plan,
                                                           float4* __restrict__ rec, int* __restrict__ cell_own, int* __restrict__ cell_oth,
                                                           unsigned* __restrict__ tickets) {
    __shared__ unsigned s_cur[kBinMaxBuckets];
    const int* bstart = plan + 16;
    for (int b = threadIdx.x; b < nb; b += kBinWide) s_cur[b] = (unsigned)bstart[b] + mat[(size_t)blockIdx.x * nb + b];
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * tile_rows, r1 = min(n, r0 + tile_rows);
    for (int64_t base = r0 + threadIdx.x; base < r1; base += 4 * kBinWide) {
        float4 p[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (base + j * kBinWide < r1) p[j] = bin_load<RAW>(xyz, pts4, base + j * kBinWide);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (base + j * kBinWide >= r1) continue;
            const unsigned pos = atomicAdd(&s_cur[bin_cell(p[j].x, p[j].y, p[j].z, g) >> shift], 1u);
            if (pos < (unsigned)n) rec[pos] = p[j];   // (guard: the caller's rows must not change between the two passes)
        }
    }
    // the counters of the shared buckets are added to by k_bin_cells, and their items take a ticket there: cleared here,
    // a kernel boundary ahead of it
    if (plan[2] > 0) {
        for (int b = blockIdx.x; b < nb; b += gridDim.x) {
            if (bstart[b + 1] - bstart[b] <= chunk) continue;
            if (threadIdx.x == 0) tickets[b] = 0u;
            const int64_t c0 = (int64_t)b << shift, c1 = min(g.ncell, c0 + ((int64_t)1 << shift));
            for (int64_t c = c0 + threadIdx.x; c < c1; c += kBinWide) {
                cell_own[c] = 0;
                if (cell_oth) cell_oth[c] = 0;
            }
        }
    }
}

// 64 consecutive values, one per lane: inclusive sums.  Six data-parallel-primitive adds (shifts by 1, 2, 4, 8 inside the
// rows of 16 lanes, then lane 15 of a row to the next row, lane 31 to the upper half): the scan stands on the latency
// chain of every block of k_bin_place, where six cross-lane LDS permutes per value cost 1 us of the kernel.
__device__ __forceinline__ int wave_incl_sum(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);      // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);      // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);      // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);      // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);      // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);      // row_bcast:31 into rows 2 and 3
    return v;
}

__global__ __launch_bounds__(kBinBlock) void k_bin_cells(const float4* __restrict__ rec, const int* __restrict__ plan,
                                                         const int4* __restrict__ items, pct_grid g, int shift, int q_begin, int q_end,
                                                         int* __restrict__ cell_own, int* __restrict__ cell_oth, int* __restrict__ base,
                                                         const PackRed* __restrict__ parts, int n_parts, PackRed* __restrict__ red,
                                                         PackRed* __restrict__ red_host, int items_q, int chunk,
                                                         int4* __restrict__ brec, unsigned long long* __restrict__ bsq,
                                                         unsigned* __restrict__ tickets) {
    extern __shared__ int s_c[];                    // cells per bucket x classes counters
    __shared__ int4 s_rec[kBinBlock / 64];
    __shared__ unsigned long long s_sq[kBinBlock / 64];
    __shared__ int s_last;
    // the grid's last block is not an item's: it folds the tiles' PackAcc records of a speculative build beside the
    // others (k_pack_final's work, off the chain: a one-block kernel of its own cost 5 us there)
    if (blockIdx.x == gridDim.x - 1) {
        if (parts) pack_fold<kBinBlock>(parts, n_parts, red, red_host, 0);
        return;
    }
    if ((int)blockIdx.x >= plan[0]) return;
    const int4 it = items[blockIdx.x];
    const int r0 = it.y, r1 = it.z, slot = it.w;
    const int cpb = 1 << shift, nc = cell_oth ? 2 * cpb : cpb;
    const int64_t c0 = (int64_t)it.x << shift;
    const int ncl = (int)min((int64_t)cpb, g.ncell - c0);
    for (int k = threadIdx.x; k < nc; k += kBinBlock) s_c[k] = 0;
    __syncthreads();
    for (int base = r0 + threadIdx.x; base < r1; base += 4 * kBinBlock) {
        float4 p[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (base + j * kBinBlock < r1) p[j] = rec[base + j * kBinBlock];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (base + j * kBinBlock >= r1) continue;
            const int l = bin_cell(p[j].x, p[j].y, p[j].z, g) - (int)c0;
            const int idx = __float_as_int(p[j].w);
            const bool owned = !cell_oth || (idx >= q_begin && idx < q_end);
            if ((unsigned)l < (unsigned)cpb) atomicAdd(&s_c[(owned ? 0 : cpb) + l], 1);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nc; k += kBinBlock) {
        const int l = k & (cpb - 1);
        if (l >= ncl) continue;
        int* arr = k < cpb ? cell_own : cell_oth;
        const int v = s_c[k];
        if (slot < 0) arr[c0 + l] = v;
        else base[(size_t)slot * nc + k] = v ? atomicAdd(&arr[c0 + l], v) : 0;
    }
    // The bucket's scan record.  A shared bucket's counts are final when all its items have added theirs: every item
    // takes a ticket of the bucket (cleared by k_bin_scatter) and the one that finds itself last reads the counts back.
    // No release fence in front of the ticket: all an item publishes are the device-scope atomics above, performed at
    // the memory side like the ticket itself, and each has returned before its wave passes the barrier (its value is the
    // operand of a store in front of it).  A fence there writes the L2's dirty lines back, in the longest blocks of the
    // launch (0.6 us of the kernel).  The last item out takes an agent-scope acquire and reads the counts with
    // agent-scope loads.
    if (slot >= 0) {
        __syncthreads();
        if (threadIdx.x == 0) {
            const int* bstart = plan + 16;
            const int ni = (bstart[it.x + 1] - bstart[it.x] + chunk - 1) / chunk;
            const bool last = atomicAdd(&tickets[it.x], 1u) == (unsigned)(ni - 1);
            if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            s_last = last;
        }
        __syncthreads();
        if (!s_last) return;
    }
    int4 v = make_int4(0, 0, 0, 0);
    unsigned long long sq = 0;
    for (int l = threadIdx.x; l < ncl; l += kBinBlock) {
        int o, x = 0;
        if (slot < 0) {
            o = s_c[l];
            if (cell_oth) x = s_c[cpb + l];
        } else {
            o = __hip_atomic_load(&cell_own[c0 + l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cell_oth) x = __hip_atomic_load(&cell_oth[c0 + l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const int4 c = count_record(o, x, items_q);
        v = add3(v, c);
        sq += (unsigned long long)c.z * (unsigned)c.x;           // owned points x population of their cell
    }
    v = make_int4(wave_incl_sum(v.x), wave_incl_sum(v.y), wave_incl_sum(v.z), wave_incl_sum(v.w));     // (lane 63: the wave's)
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
    if ((threadIdx.x & 63) == 63) {
        s_rec[threadIdx.x >> 6] = v;
        s_sq[threadIdx.x >> 6] = sq;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int4 t = make_int4(0, 0, 0, 0);
        unsigned long long q = 0;
        for (int i = 0; i < kBinBlock / 64; ++i) { t = add3(t, s_rec[i]); q += s_sq[i]; }
        brec[it.x] = t;
        bsq[it.x] = q;
    }
}

__global__ __launch_bounds__(kBinBlock) void k_bin_place(const float4* __restrict__ rec, const int* __restrict__ plan,
                                                         const int4* __restrict__ items, pct_grid g, int shift, int q_begin, int q_end,
                                                         int64_t n, int64_t n_owned, int nb, int items_q, const int4* __restrict__ brec,
                                                         const int* __restrict__ cell_own, const int* __restrict__ cell_oth,
                                                         const int* __restrict__ base, int* __restrict__ cell_start,
                                                         int* __restrict__ own_start, int2* __restrict__ occ, int64_t occ_cap,
                                                         float4* __restrict__ sorted4, int* __restrict__ row_of, int* __restrict__ owned_pos,
                                                         const double4* __restrict__ pts4d, double4* __restrict__ sorted4d) {
    extern __shared__ int s_cur[];                  // cells per bucket x classes cursors, then (two classes) cells per bucket words:
                                                    // neighbour-table row minus sorted position of the cell's owned points
    __shared__ int4 s_wave[kBinBlock / 64];         // the sums of the four waves' quarters of the bucket
    if ((int)blockIdx.x >= plan[0]) return;
    const int4 it = items[blockIdx.x];
    const int r0 = it.y, r1 = it.z, slot = it.w;
    const int cpb = 1 << shift, nc = cell_oth ? 2 * cpb : cpb;
    const int64_t c0 = (int64_t)it.x << shift;
    const int ncl = (int)min((int64_t)cpb, g.ncell - c0);
    int* s_row = s_cur + nc;
    // The triple scan inside the bucket (cells, work-item ranks, owned points: k_scan_apply's work), from the bucket's
    // final counts and its bases in brec.  Every wave takes a quarter of the bucket's cells, 64 consecutive cells a trip,
    // one per lane: first its sums, then, behind the sums of the waves in front of it, its cells' starts.
    // (A lane reads back from LDS only what it has stored there itself: no barrier between the two loops.)
    // The item's first records are on their way meanwhile.
    float4 p[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (r0 + (int)threadIdx.x + j * kBinBlock < r1) p[j] = rec[r0 + threadIdx.x + j * kBinBlock];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l_begin = wave * (cpb / (kBinBlock / 64)), l_end = l_begin + cpb / (kBinBlock / 64);     // (cpb >= 256: whole trips)
    {
        int4 v = make_int4(0, 0, 0, 0);
        for (int l = l_begin + lane; l < l_end; l += 64) {
            const int o = l < ncl ? cell_own[c0 + l] : 0, x = cell_oth && l < ncl ? cell_oth[c0 + l] : 0;
            s_cur[l] = o;
            if (cell_oth) s_cur[cpb + l] = x;
            v = add3(v, count_record(o, x, items_q));
        }
        v = make_int4(wave_incl_sum(v.x), wave_incl_sum(v.y), wave_incl_sum(v.z), 0);
        if (lane == 63) s_wave[wave] = v;
    }
    __syncthreads();
    int4 run = brec[it.x];
    for (int w = 0; w < wave; ++w) run = add3(run, s_wave[w]);
    // the first item of a bucket also writes the lists the sweep and the fit read, for the bucket's cells
    const bool first = slot < 0 || r0 == plan[16 + it.x];
    for (int l = l_begin + lane; l < l_end; l += 64) {
        const int o = s_cur[l], x = cell_oth ? s_cur[cpb + l] : 0;
        const int4 c = count_record(o, x, items_q);
        const int4 incl = make_int4(wave_incl_sum(c.x), wave_incl_sum(c.y), wave_incl_sum(c.z), 0);
        const int s = run.x + incl.x - c.x, r = run.y + incl.y - c.y, w = run.z + incl.z - c.z;
        run.x += __builtin_amdgcn_readlane(incl.x, 63);
        run.y += __builtin_amdgcn_readlane(incl.y, 63);
        run.z += __builtin_amdgcn_readlane(incl.z, 63);
        if (l >= ncl) continue;
        const size_t off = slot >= 0 ? (size_t)slot * nc + l : 0;
        const int run_own = slot >= 0 ? base[off] : 0, run_oth = slot >= 0 && cell_oth ? base[off + cpb] : 0;
        if (first) {
            cell_start[c0 + l] = s;
            own_start[c0 + l] = w;
            for (int ch = 0; ch < c.y; ++ch)
                if (r + ch < occ_cap) occ[r + ch] = make_int2((int)(c0 + l), ch);
        }
        s_cur[l] = s + run_own;
        if (cell_oth) {
            s_cur[cpb + l] = s + o + run_oth;           // owned points first inside every cell
            s_row[l] = w - s;
        }
    }
    if (first && it.x == nb - 1 && threadIdx.x == 0) {
        const int4 tot = brec[nb];
        cell_start[g.ncell] = tot.x;
        own_start[g.ncell] = tot.z;
    }
    if (r0 >= r1) return;               // (an empty bucket's item: the lists above were its work)
    __syncthreads();
    for (int base = r0 + threadIdx.x; base < r1; base += 4 * kBinBlock) {
        if (base != r0 + (int)threadIdx.x) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (base + j * kBinBlock < r1) p[j] = rec[base + j * kBinBlock];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (base + j * kBinBlock >= r1) continue;
            const int l = bin_cell(p[j].x, p[j].y, p[j].z, g) - (int)c0;
            const int idx = __float_as_int(p[j].w);
            const bool owned = !cell_oth || (idx >= q_begin && idx < q_end);
            if ((unsigned)l >= (unsigned)ncl) continue;
            const int pos = atomicAdd(&s_cur[(owned ? 0 : cpb) + l], 1);
            if ((unsigned)pos >= (unsigned)n) continue;
            sorted4[pos] = p[j];
            if (pts4d) sorted4d[pos] = pts4d[idx];
            if (owned) {
                const int row = cell_oth ? pos + s_row[l] : pos;   // (every point owned: rows are sorted positions)
                if ((unsigned)row < (unsigned)n_owned && (unsigned)(idx - q_begin) < (unsigned)n_owned) {
                    owned_pos[row] = pos;
                    if (row_of) row_of[idx - q_begin] = row;       // (null: built on first need, pct_ensure_row_of)
                }
            }
        }
    }
}

// row_of from the finished cell list: the public index rides in w of every sorted record.  The fused step never reads
// row_of (its results stay in table-row order); this is the one 4-byte store per point at a random address that the
// build would otherwise make (9 of k_bin_place's 25 us at 1 M points), paid by the first call that gathers through it.
__global__ __launch_bounds__(256) void k_bin_row_of(const float4* __restrict__ sorted4, const int* __restrict__ owned_pos, int64_t n_owned,
                                                    int q_begin, int* __restrict__ row_of) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n_owned) return;
    const int idx = __float_as_int(sorted4[owned_pos[row]].w);
    if ((unsigned)(idx - q_begin) < (unsigned)n_owned) row_of[idx - q_begin] = (int)row;
}

__global__ __launch_bounds__(256) void k_gather_int(const int* __restrict__ map, int* __restrict__ io, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) io[i] = map[io[i]];
}

int grid_1d(int64_t n, int per_block, int cap) {
    int64_t b = (n + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (cap > 0 && b > cap) b = cap;
    return (int)b;
}

}  // namespace

// ---------------------------------------------------------------------------
static PackRed* red_parts(pct_ctx* ctx) { return (PackRed*)((char*)ctx->red.p + 128); }
static_assert(sizeof(PackRed) <= sizeof(pct_pinned::pack_red) && alignof(PackRed) <= 128, "pct_pinned::pack_red holds a PackRed");
static_assert(sizeof(ScanTotals) <= sizeof(pct_pinned::scan_totals) && alignof(ScanTotals) <= 128, "pct_pinned::scan_totals holds a ScanTotals");
static PackRed* pin_red(pct_ctx* ctx) { return (PackRed*)ctx->pin->pack_red; }
static ScanTotals* pin_totals(pct_ctx* ctx) { return (ScanTotals*)ctx->pin->scan_totals; }

static int red_reset(pct_ctx* ctx, int n_parts, bool zero = true) {
    PCT_TRY(pct_reserve(ctx, &ctx->red, 128 + (size_t)n_parts * sizeof(PackRed)));
    if (zero) PCT_HIP(ctx, hipMemsetAsync(ctx->red.p, 0, 128, ctx->stream));
    return PCT_OK;
}

// folds the n_parts block records of the pass just launched (the result also lands in pinned host memory)
static int red_fold(pct_ctx* ctx, int n_parts, bool carry = true) {
    PCT_LAUNCH(k_pack_final, dim3(1), dim3(kBlock), 0, ctx->stream, (const PackRed*)red_parts(ctx), n_parts,
                       (PackRed*)ctx->red.p, pin_red(ctx), carry ? 1 : 0);
    PCT_HIP(ctx, hipGetLastError());
    return PCT_OK;
}

// ... and reads the result back
static int red_read(pct_ctx* ctx, int n_parts, PackRed* out, float* bbox, bool carry = true) {
    PCT_TRY(red_fold(ctx, n_parts, carry));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(out, pin_red(ctx), sizeof(*out));
    for (int a = 0; a < 6; ++a) bbox[a] = order_float(out->bb[a]);
    return PCT_OK;
}

// every point, public order
// defer: do not wait for the result (the caller builds on the previous call's box and checks at its next
// synchronisation, pct_build_grid)
static int pack_all(pct_ctx* ctx, float* bbox, PackRed* red, bool defer = false, unsigned long long* begin_stamp = nullptr) {
    const int64_t n = ctx->n;
    PCT_TRY(pct_reserve(ctx, &ctx->pts4, (size_t)n * sizeof(float4)));
    const int nb = grid_1d(n, kBlock * 4, 512);
    PCT_TRY(red_reset(ctx, nb, false));
    PCT_LAUNCH(k_pack, dim3(nb), dim3(kBlock), 0, ctx->stream, ctx->xyz_view, n, (float4*)ctx->pts4.p, red_parts(ctx), begin_stamp);
    PCT_HIP(ctx, hipGetLastError());
    if (defer) {
        PCT_TRY(red_fold(ctx, nb, false));
    } else {
        PCT_TRY(red_read(ctx, nb, red, bbox, false));
        if (red->bad) return pct_fail(ctx, PCT_ERR_NONFINITE, "Non-finite values in input points");
    }
    ctx->pts4_valid = true;
    ctx->n_grid = n;
    ctx->g_begin = ctx->q_begin;
    ctx->culled = false;
    return PCT_OK;
}

int pct_pack_points(pct_ctx* ctx, float* bbox /*6*/) {
    PackRed red;
    return pack_all(ctx, bbox, &red);
}

// Sharded handle: pack only the points inside the owned rows' bounding box grown by `margin_cells` first-guess
// cell edges.  *kept_box receives the box that was applied (its faces become pct_grid::lim_*).
// Ownership by slab: bounding box of the whole cloud, histogram along its longest axis, the cuts of all parts (on the
// device; the cuts and the populations come back through pinned memory).  Leaves q_begin = 0, q_end = population of
// this handle's slab: the owned points will lead the packed array.
static int slab_split(pct_ctx* ctx) {
    const int64_t n = ctx->n;
    const int parts = ctx->slab_parts;
    const int nb = grid_1d(n, kBlock * 4, 2048);
    const bool vec = ((uintptr_t)ctx->xyz_view & 15) == 0;
    PackRed red;
    float ob[6];
    PCT_TRY(red_reset(ctx, nb));
    if (vec) PCT_LAUNCH(k_cloud_box<true>, dim3(nb), dim3(kBlock), 0, ctx->stream, ctx->xyz_view, n, red_parts(ctx));
    else PCT_LAUNCH(k_cloud_box<false>, dim3(nb), dim3(kBlock), 0, ctx->stream, ctx->xyz_view, n, red_parts(ctx));
    PCT_HIP(ctx, hipGetLastError());
    PCT_TRY(red_read(ctx, nb, &red, ob));
    if (red.bad) return pct_fail(ctx, PCT_ERR_NONFINITE, "Non-finite values in input points");
    int axis = 0;
    for (int a = 1; a < 3; ++a)
        if (ob[3 + a] - ob[a] > ob[3 + axis] - ob[axis]) axis = a;
    const double ext = (double)ob[3 + axis] - ob[axis];
    ctx->slab_axis = axis;
    ctx->slab_x0 = ob[axis];
    ctx->slab_inv = ext > 0 && isfinite((float)(kSlabBins / ext)) ? (float)(kSlabBins / ext) : 0.f;
    for (int a = 0; a < 6; ++a) ctx->slab_bbox[a] = ob[a];
    PCT_TRY(pct_reserve(ctx, &ctx->scan_tmp, 256 + kSlabBins * sizeof(unsigned)));
    unsigned* hist = (unsigned*)((char*)ctx->scan_tmp.p + 256);
    PCT_HIP(ctx, hipMemsetAsync(hist, 0, kSlabBins * sizeof(unsigned), ctx->stream));
    const int nh = grid_1d(n, kSlabHistBlock * 4, 512);
    if (vec) PCT_LAUNCH(k_slab_hist<true>, dim3(nh), dim3(kSlabHistBlock), 0, ctx->stream, ctx->xyz_view, n, axis, ctx->slab_x0, ctx->slab_inv, hist);
    else PCT_LAUNCH(k_slab_hist<false>, dim3(nh), dim3(kSlabHistBlock), 0, ctx->stream, ctx->xyz_view, n, axis, ctx->slab_x0, ctx->slab_inv, hist);
    int* h_cut = ctx->pin->slab_cut;                            // mapped pinned memory: the kernel writes the host's copy
    long long* h_counts = ctx->pin->slab_counts;
    PCT_LAUNCH(k_slab_cut, dim3(1), dim3(kBlock), 0, ctx->stream, (const unsigned*)hist, (long long)n, parts, h_cut, h_counts);
    PCT_HIP(ctx, hipGetLastError());
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    long long total = 0;
    for (int p = 0; p < parts; ++p) { ctx->slab_counts[p] = h_counts[p]; total += h_counts[p]; }
    if (total != n || h_cut[0] != 0 || h_cut[parts] != kSlabBins)
        return pct_fail(ctx, PCT_ERR_INVALID, "slab cut: %lld of %lld points in %d parts", total, (long long)n, parts);
    ctx->slab_bin_lo = h_cut[ctx->slab_part];
    ctx->slab_bin_hi = h_cut[ctx->slab_part + 1];
    ctx->q_begin = 0;
    ctx->q_end = ctx->slab_counts[ctx->slab_part];
    ctx->slab_split_valid = true;
    return PCT_OK;
}

static int pack_near_owned(pct_ctx* ctx, double target, float* bbox, PackRed* red, Box3* kept_box) {
    const int64_t n = ctx->n, n_owned = ctx->q_end - ctx->q_begin;
    const bool slab = ctx->slab_parts >= 1;
    Box3 box;
    if (slab) {
        // the slab and 4 first-guess cell edges either side of it along the cut axis, everything across; the outer
        // faces of the first and the last slab are open.  After a limit retry (no_cull): every point.
        const float* ob = ctx->slab_bbox;
        const double ex = (double)ob[3] - ob[0], ey = (double)ob[4] - ob[1], ez = (double)ob[5] - ob[2];
        const double emax = fmax(ex, fmax(ey, ez));
        double area = 1.2 * (ex * ey + ey * ez + ex * ez);
        if (!(area > 0)) area = emax * emax;
        double a0 = sqrt(target * area / (double)n);
        if (!(a0 > 0) || !isfinite(a0)) a0 = emax;
        double margin = 4.0 * a0;
        if (const char* e = pct_getenv("PCT_SLAB_MARGIN")) margin = atof(e) * a0;      // test aid: a thin margin forces the limit retry
        for (int a = 0; a < 3; ++a) { box.lo[a] = -INFINITY; box.hi[a] = INFINITY; }
        if (!ctx->no_cull && ctx->slab_inv > 0) {
            const int ax = ctx->slab_axis;
            if (ctx->slab_bin_lo > 0) box.lo[ax] = (float)((double)ctx->slab_x0 + (double)ctx->slab_bin_lo / ctx->slab_inv - margin);
            if (ctx->slab_bin_hi < kSlabBins) box.hi[ax] = (float)((double)ctx->slab_x0 + (double)ctx->slab_bin_hi / ctx->slab_inv + margin);
        }
    } else {
    // A handle that is fed a stream of similar clouds (same size, same owned range) reuses the box of the last call
    // instead of measuring the owned rows first (one pass and one host synchronisation less).  A stale box is safe:
    // the owned rows are packed whatever it says, and a query that reaches past a face makes the sweep repeat
    // with every point (pct_grid::lim_*) -- after which the box is measured again.
    const bool reuse = ctx->cull_box_valid && ctx->cull_box_n == n && ctx->cull_box_q0 == ctx->q_begin &&
                       ctx->cull_box_q1 == ctx->q_end;
    if (reuse) {
        for (int a = 0; a < 3; ++a) { box.lo[a] = ctx->cull_box[a]; box.hi[a] = ctx->cull_box[3 + a]; }
    } else {
        const int nb = grid_1d(n_owned, kBlock * 4, 512);
        PCT_TRY(red_reset(ctx, nb));
        PCT_LAUNCH(k_range_box, dim3(nb), dim3(kBlock), 0, ctx->stream,
                           ctx->xyz_view, ctx->q_begin, ctx->q_end, red_parts(ctx));
        PCT_HIP(ctx, hipGetLastError());
        float ob[6];
        PCT_TRY(red_read(ctx, nb, red, ob));
        if (red->bad) return pct_fail(ctx, PCT_ERR_NONFINITE, "Non-finite values in input points");
        // margin: 4 cell edges of the cell size the owned points alone would get (an over-estimate of the final
        // edge whenever other handles' points share the region); the sweep checks the assumption per query
        const double ex = (double)ob[3] - ob[0], ey = (double)ob[4] - ob[1], ez = (double)ob[5] - ob[2];
        const double emax = fmax(ex, fmax(ey, ez));
        double area = 1.2 * (ex * ey + ey * ez + ex * ez);
        if (!(area > 0)) area = emax * emax;
        double a0 = sqrt(target * area / (double)n_owned);
        if (!(a0 > 0) || !isfinite(a0)) a0 = emax;
        const float margin = (float)(4.0 * a0);
        for (int a = 0; a < 3; ++a) { box.lo[a] = ob[a] - margin; box.hi[a] = ob[3 + a] + margin; }
        for (int a = 0; a < 3; ++a) { ctx->cull_box[a] = box.lo[a]; ctx->cull_box[3 + a] = box.hi[a]; }
        ctx->cull_box_valid = true;
        ctx->cull_box_n = n;
        ctx->cull_box_q0 = ctx->q_begin;
        ctx->cull_box_q1 = ctx->q_end;
    }
    }
    *kept_box = box;

    const int nchunk = (int)((n + kCullChunk - 1) / kCullChunk);
    PCT_TRY(pct_reserve(ctx, &ctx->pts4, (size_t)n * sizeof(float4)));           // worst case: everything is kept
    PCT_TRY(pct_reserve(ctx, &ctx->scan_tmp, 256));
    PCT_TRY(red_reset(ctx, nchunk));
    PCT_HIP(ctx, hipMemsetAsync(ctx->scan_tmp.p, 0, 33 * sizeof(unsigned), ctx->stream));
    const SlabCut cut = {ctx->slab_axis, ctx->slab_bin_lo, ctx->slab_bin_hi, ctx->slab_x0, ctx->slab_inv};
    const bool vec = ((uintptr_t)ctx->xyz_view & 15) == 0;
#define PCT_CULL(S, V) PCT_LAUNCH((k_cull_pack<S, V>), dim3(nchunk), dim3(kCullBlock), 0, ctx->stream, ctx->xyz_view, n, box, ctx->q_begin, \
                                  ctx->q_end, cut, (float4*)ctx->pts4.p, (unsigned*)ctx->scan_tmp.p, (PackRed*)ctx->red.p, red_parts(ctx))
    if (slab) { if (vec) PCT_CULL(true, true); else PCT_CULL(true, false); }
    else { if (vec) PCT_CULL(false, true); else PCT_CULL(false, false); }
#undef PCT_CULL
    PCT_HIP(ctx, hipGetLastError());
    PCT_HIP(ctx, hipMemcpyAsync(&ctx->pin->cull_kept, ctx->scan_tmp.p, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    PCT_HIP(ctx, hipMemcpyAsync(&ctx->pin->cull_owned, (const unsigned*)ctx->scan_tmp.p + 32, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    PCT_TRY(red_read(ctx, nchunk, red, bbox));
    if (red->bad) return pct_fail(ctx, PCT_ERR_NONFINITE, "Non-finite values in input points");
    if (slab && (int64_t)ctx->pin->cull_owned != n_owned)
        return pct_fail(ctx, PCT_ERR_INVALID, "slab pack found %u owned points, the cut said %lld (was the cloud's buffer written meanwhile?)",
                        ctx->pin->cull_owned, (long long)n_owned);
    const int64_t kept = n_owned + (int64_t)ctx->pin->cull_kept;
    if ((int64_t)red->cnt != kept || kept > n)
        return pct_fail(ctx, PCT_ERR_INVALID, "cull pass kept %lld / counted %lld points", (long long)red->cnt, (long long)kept);
    ctx->pts4_valid = false;                 // pts4 is not the full public-order pack
    ctx->n_grid = kept;
    ctx->g_begin = 0;                        // the owned rows lead the packed array
    ctx->culled = kept < n;
    return PCT_OK;
}

// Outlier-trimmed grid box.  A few far outliers would stretch the bounding box until the whole cloud falls into
// a handful of cells.  Cell coordinates are clamped, and a clamped point is never nearer than its boundary cell
// suggests, so the grid may cover any sub-box: take mean +- 6 sigma per axis (re-estimated inside the box until
// it settles) and let the points outside share the boundary cells.  Clouds without outliers keep their bbox:
// a uniform or surface-like distribution spans about +-1.7 sigma.
static int trim_box(pct_ctx* ctx, const PackRed& first, float* bbox) {
    PackRed r = first;
    float sh[3] = {0.f, 0.f, 0.f};           // the moments in `first` are about the origin
    for (int pass = 0; pass < 5; ++pass) {
        if (r.cnt < 2) break;
        bool shrunk = false;
        float nb[6];
        for (int a = 0; a < 3; ++a) {
            const double mean = r.s[a] / (double)r.cnt, var = fmax(r.ss[a] / (double)r.cnt - mean * mean, 0.0);
            const double sd = sqrt(var), c = (double)sh[a] + mean;
            const double lo = fmax((double)bbox[a], c - 6.0 * sd), hi = fmin((double)bbox[3 + a], c + 6.0 * sd);
            const double cut = fmax(lo - bbox[a], 0.0) + fmax((double)bbox[3 + a] - hi, 0.0);
            nb[a] = bbox[a];
            nb[3 + a] = bbox[3 + a];
            if (cut > 0.25 * (hi - lo) && hi > lo) {           // worth it only if a good part of the extent goes
                nb[a] = (float)lo;
                nb[3 + a] = (float)hi;
                shrunk = true;
            }
        }
        if (!shrunk) break;
        for (int a = 0; a < 6; ++a) bbox[a] = nb[a];
        Box3 box, shift;
        for (int a = 0; a < 3; ++a) { box.lo[a] = bbox[a]; box.hi[a] = bbox[3 + a]; shift.lo[a] = shift.hi[a] = 0.5f * (bbox[a] + bbox[3 + a]); }
        for (int a = 0; a < 3; ++a) sh[a] = shift.lo[a];
        const int nblk = grid_1d(ctx->n_grid, kBlock * 4, 512);
        PCT_TRY(red_reset(ctx, nblk));
        PCT_LAUNCH(k_box_stats, dim3(nblk), dim3(kBlock), 0, ctx->stream,
                           (const float4*)ctx->pts4.p, ctx->n_grid, box, shift, red_parts(ctx));
        PCT_HIP(ctx, hipGetLastError());
        float inner[6];
        PCT_TRY(red_read(ctx, nblk, &r, inner));
        ++ctx->tm.grid_iters;     // counted with the cell-size passes
    }
    return PCT_OK;
}

int pct_pack_points_f64(pct_ctx* ctx, const double* d_xyz64) {
    const int64_t n = ctx->n;
    PCT_TRY(pct_reserve(ctx, &ctx->pts4d, (size_t)n * sizeof(double4)));
    PCT_TRY(pct_reserve(ctx, &ctx->xyz, (size_t)n * 3 * sizeof(float)));
    PCT_LAUNCH(k_pack_f64, dim3(grid_1d(n, kBlock, 2048)), dim3(kBlock), 0, ctx->stream,
                       d_xyz64, n, (double4*)ctx->pts4d.p, (float*)ctx->xyz.p);
    ctx->xyz_view = (const float*)ctx->xyz.p;
    PCT_HIP(ctx, hipGetLastError());
    return PCT_OK;
}

// ---- where the grid's points come from (GridSource, choose_source: pct_grid_edge.h) --------------------------------------
struct GridPoints {
    GridSource src;
    float bbox[6];           // grid box
    PackRed red;             // the pack pass's record (CallerRows: filled in by check_deferred_box)
    Box3 kept_box;           // CulledPack: the box that was applied
    int64_t n;               // points the grid holds
    int g_begin, g_end;      // the owned range of the grid's records (0, 0: ownership by wanted edge)
    bool raw;                // the histogram and the placement read the caller's rows (k_bin_*<true>, k_hist_raw, k_scatter_raw)
    bool from_base;          // ... or the level base (k_hist_agg)
    bool deferred_box;       // the cloud's own box rides on the first pass and has not been checked yet
};

// Decides the source (choose_source) from ctx and the pass and runs its pack pass.  *restart: the kept part cannot fill a
// row; culling is ruled out on the handle and the caller starts over.
// clock (may be null): the call's begin -- the full pack's kernel takes its word; every other pack pass has its event in front.
static int select_source(pct_ctx* ctx, int32_t k, double target, bool slab, int64_t n_owned, bool sharded, const LevelPass* pass,
                         GridPoints* s, bool* restart, pct_call_clock* clock) {
    const bool by_want = pass && pass->want;
    *s = GridPoints{};
    s->src = choose_source({by_want, pass && pass->base, pass != nullptr, slab, sharded, n_owned, ctx->has_f64, ctx->no_cull,
                            pct_getenv("PCT_NO_CULL") != nullptr, pct_getenv("PCT_NO_SPEC") != nullptr, ctx->hint_edge, ctx->spec_valid,
                            ctx->spec_n, ctx->n});
    if (clock && s->src != GridSource::CallerRows && s->src != GridSource::FullPack) PCT_HIP(ctx, clock->begin_event(ctx->stream));
    switch (s->src) {
    case GridSource::LevelBase:
        for (int a = 0; a < 6; ++a) s->bbox[a] = pass->base_box[a];
        ctx->n_grid = ctx->n;
        ctx->g_begin = 0;
        ctx->culled = false;
        break;
    case GridSource::CulledPack:
        PCT_TRY(pack_near_owned(ctx, target, s->bbox, &s->red, &s->kept_box));
        if (ctx->n_grid < (int64_t)k + 1) {
            // The kept part cannot even fill a row (a few owned rows and a culling box -- possibly a stale one of the
            // previous cloud -- that holds nobody else): the table would carry "missing" entries that the fused fit,
            // launched before the limits are checked, must never see without a count array.  Take every point.
            ctx->no_cull = true;
            ctx->cull_box_valid = false;
            *restart = true;
            return PCT_OK;
        }
        PCT_TRY(trim_box(ctx, s->red, s->bbox));
        break;
    case GridSource::CallerRows:
        // no pack pass at all: the histogram reads the caller's rows and takes the cloud's box along (k_hist_raw)
        PCT_TRY(red_reset(ctx, grid_1d(ctx->n, kBlock, 0), false));
        ctx->pts4_valid = false;
        ctx->n_grid = ctx->n;
        ctx->g_begin = ctx->q_begin;
        ctx->culled = false;
        for (int a = 0; a < 6; ++a) s->bbox[a] = ctx->spec_bbox[a];
        break;
    case GridSource::FullPack:
        PCT_TRY(pack_all(ctx, s->bbox, &s->red, false, clock ? clock->begin_word() : nullptr));
        PCT_TRY(trim_box(ctx, s->red, s->bbox));
        break;
    }
    s->raw = s->deferred_box = s->src == GridSource::CallerRows;
    s->from_base = s->src == GridSource::LevelBase;
    s->n = ctx->n_grid;
    s->g_begin = by_want ? 0 : (int)ctx->g_begin;
    s->g_end = by_want ? 0 : (int)(ctx->g_begin + n_owned);
    return PCT_OK;
}

// The deferred pack result is in: was the old box still right?  (Within 2 % of the previous cloud's extent per face.)
enum class BoxCheck { Accept, Restart, NonFinite };
static BoxCheck check_deferred_box(pct_ctx* ctx, GridPoints* s) {
    s->deferred_box = false;
    memcpy(&s->red, pin_red(ctx), sizeof(s->red));
    if (s->red.bad) return BoxCheck::NonFinite;
    bool same = true;
    for (int ax = 0; ax < 3; ++ax) {
        const float lo = order_float(s->red.bb[ax]), hi = order_float(s->red.bb[3 + ax]);
        const float tol = 0.02f * (ctx->spec_raw[3 + ax] - ctx->spec_raw[ax]) + 1e-30f;
        same = same && fabsf(lo - ctx->spec_raw[ax]) <= tol && fabsf(hi - ctx->spec_raw[3 + ax]) <= tol;
    }
    return same ? BoxCheck::Accept : BoxCheck::Restart;
}

// ---- the grid of one pass ----------------------------------------------------------------------------------------------
// The box and the dimensions for edge a.  sub_box (a fast level pass: the box of its owned points, else null): 2.5 edges
// of THIS cell size around them (their stencils must end inside the box: the points outside it are left out of the cell list).
static void size_grid(const float* sub_box, float* bbox, double a, pct_grid* g) {
    if (sub_box)
        for (int ax = 0; ax < 3; ++ax) {
            bbox[ax] = sub_box[ax] - (float)(2.5 * a);
            bbox[3 + ax] = sub_box[3 + ax] + (float)(2.5 * a);
        }
    g->ox = bbox[0]; g->oy = bbox[1]; g->oz = bbox[2];
    g->cell = a;
    g->inv_cell = 1.0 / a;
    double ex = (double)bbox[3] - bbox[0], ey = (double)bbox[4] - bbox[1], ez = (double)bbox[5] - bbox[2];
    if (!(ex >= 0)) ex = 0;          // an empty or non-finite box is one cell, not INT_MIN cells
    if (!(ey >= 0)) ey = 0;
    if (!(ez >= 0)) ez = 0;
    // counted in double first: an absurdly small edge (eps = 1e-30) must read as "far too many cells" for the caller's
    // budget loop, not overflow the int32 dimensions
    const double dx = floor(ex * g->inv_cell) + 1, dy = floor(ey * g->inv_cell) + 1, dz = floor(ez * g->inv_cell) + 1;
    if (!(dx * dy * dz < 4.0e18) || !(dx < 2.0e9) || !(dy < 2.0e9) || !(dz < 2.0e9)) {
        g->nx = g->ny = g->nz = 1 << 30;
        g->ncell = (int64_t)1 << 62;
        return;
    }
    g->nx = (int32_t)dx;
    g->ny = (int32_t)dy;
    g->nz = (int32_t)dz;
    g->ncell = (int64_t)g->nx * g->ny * g->nz;
}

// what every pass of a build writes, sized by the points and not by the grid
static int reserve_lists(pct_ctx* ctx, int64_t n, int64_t n_owned, bool by_want) {
    PCT_TRY(pct_reserve(ctx, &ctx->cell_of, (size_t)n * sizeof(int)));
    PCT_TRY(pct_reserve(ctx, &ctx->cell_fill, (size_t)n * sizeof(int)));   // in-cell arrival ranks
    PCT_TRY(pct_reserve(ctx, &ctx->sorted4, (size_t)n * sizeof(float4)));
    PCT_TRY(pct_reserve(ctx, &ctx->row_of, (size_t)((by_want ? n : n_owned) + 1) * sizeof(int)));
    PCT_TRY(pct_reserve(ctx, &ctx->owned_pos, (size_t)n_owned * sizeof(int)));
    if (ctx->has_f64) PCT_TRY(pct_reserve(ctx, &ctx->sorted4d, (size_t)n * sizeof(double4)));
    return PCT_OK;
}

// the cell-size search of one build (pct_grid_edge.h) on the box of its source and the handle's warm start
static EdgeSearch edge_search(const pct_ctx* ctx, const GridPoints& s, double target, double eps, const LevelPass* pass) {
    EdgeSearch es = {};
    es.target = target; es.n = s.n; es.eps = eps;
    es.ex = (double)s.bbox[3] - s.bbox[0]; es.ey = (double)s.bbox[4] - s.bbox[1]; es.ez = (double)s.bbox[5] - s.bbox[2];
    es.hint_edge = ctx->hint_edge; es.hint_guess = ctx->hint_guess; es.hint_target = ctx->hint_target;
    es.level_edge = pass ? pass->edge : 0;
    // a level pass takes the edge it is given: its owned set is a mix of densities, and the mean population the search
    // steers on would be pulled to the dense minority (pct_levels.hip sizes by the geometric mean instead)
    es.max_iter = es.level_edge > 0 ? 1 : pass ? 2 : 8;
    return es;
}

// ---- which build, and its launches -------------------------------------------------------------------------------------
// Dispatch: the two-level LDS counting sort (k_bin_*) wherever a grid point is owned or not by its public index alone and
// every point is binned -- the caller's rows, the full pack, the range-culled pack -- and the bucket scheme covers the
// grid (bin_shape, per pass).  The level passes (by wanted edge, sub_box), the slab-owned handles and larger grids keep the
// per-point atomics; PCT_GRID_ATOMIC=1 forces those everywhere (A/B runs, parity tests).
enum class GridBuild {
    Bin,             // k_bin_count, k_bin_colscan, k_bin_plan, k_bin_scatter, k_bin_cells | k_bin_place
    AtomicRaw,       // k_hist_raw (+ k_pack_final while the box is deferred)                 | k_scatter_raw
    AtomicBase,      // k_hist_agg                                                             | k_scatter
    AtomicPacked,    // k_hist                                                                 | k_scatter
};
static GridBuild choose_build(bool bin_allowed, const BinShape& bs, const GridPoints& s) {
    return bin_allowed && bs.ok ? GridBuild::Bin : s.raw ? GridBuild::AtomicRaw : s.from_base ? GridBuild::AtomicBase : GridBuild::AtomicPacked;
}

// Scratch of one bin pass (sized by its grid): bucket-partitioned records (bin_rec), [tile][bucket] matrix (bin_mat),
// plan words + bucket starts + column totals + work list + the buckets' scan records and tickets (bin_plan), run offsets of
// the shared buckets' items (bin_base).
struct BinScratch {
    int* plan;
    unsigned* tot;       // column totals, inside bin_plan
    int4* items;         // work list, inside bin_plan
    int4* brec;          // per bucket: sums of cell_counts() over its cells, then (k_scan_tiles) the sums of the buckets in
                         // front of it; [nb] the totals.  Inside bin_plan, as are
    unsigned long long* bsq;     // per bucket: sum of owned x total over its cells
    unsigned* tickets;   // per shared bucket: items that have added their counts
    size_t lds;          // fine counters of one class
};
static int bin_scratch(pct_ctx* ctx, const BinShape& bs, int64_t n, BinScratch* b) {
    PCT_TRY(pct_reserve(ctx, &ctx->bin_rec, (size_t)n * sizeof(float4)));
    PCT_TRY(pct_reserve(ctx, &ctx->bin_mat, (size_t)bs.ntiles * bs.nb * sizeof(unsigned)));
    const size_t plan_words = 16 + (size_t)(bs.nb + 1) + (size_t)bs.nb;
    const size_t items_at = (plan_words * sizeof(int) + 15) / 16 * 16;
    const size_t brec_at = items_at + (size_t)bs.max_items * sizeof(int4);
    const size_t bsq_at = brec_at + (size_t)(bs.nb + 1) * sizeof(int4);
    const size_t tickets_at = bsq_at + (size_t)bs.nb * sizeof(unsigned long long);
    PCT_TRY(pct_reserve(ctx, &ctx->bin_plan, tickets_at + (size_t)bs.nb * sizeof(unsigned)));
    PCT_TRY(pct_reserve(ctx, &ctx->bin_base, (size_t)bs.max_shared * (bs.cls << bs.shift) * sizeof(int)));
    b->plan = (int*)ctx->bin_plan.p;
    b->tot = (unsigned*)(b->plan + 16 + bs.nb + 1);
    b->items = (int4*)((char*)ctx->bin_plan.p + items_at);
    b->brec = (int4*)((char*)ctx->bin_plan.p + brec_at);
    b->bsq = (unsigned long long*)((char*)ctx->bin_plan.p + bsq_at);
    b->tickets = (unsigned*)((char*)ctx->bin_plan.p + tickets_at);
    b->lds = (size_t)(bs.cls << bs.shift) * sizeof(int);
    return PCT_OK;
}

// what the launches of one pass share
struct GridPass {
    GridBuild build;
    pct_grid g;
    BinShape bs;
    BinScratch bin;
    const float4* src;       // packed records (pts4 or the level base)
    int64_t n_owned;
    const LevelPass* level;  // the pass of the chained sweep that asked for the build (null: a plain call)
    bool sharded, sub_box;
    int items_q;             // queries per work item of the sweep
    int64_t occ_cap;         // entries of the sweep's work list (occ) that are reserved
};

// the two passes over the input tiles, from the caller's rows (RAW) or from packed records
template <bool RAW>
static void launch_bin_count(pct_ctx* ctx, int64_t n, const GridPass& p, PackRed* parts, unsigned long long* begin_stamp) {
    PCT_LAUNCH_T(k_bin_count<RAW>, dim3(p.bs.ntiles), dim3(kBinWide), 0, ctx->stream, ctx->xyz_view, p.src, n, p.bs.tile_rows, p.g, p.bs.shift,
                 p.bs.nb, (unsigned*)ctx->bin_mat.p, parts, begin_stamp);
}
template <bool RAW>
static void launch_bin_scatter(pct_ctx* ctx, int64_t n, const GridPass& p, int* cell_oth) {
    PCT_LAUNCH_T(k_bin_scatter<RAW>, dim3(p.bs.ntiles), dim3(kBinWide), 0, ctx->stream, ctx->xyz_view, p.src, n, p.bs.tile_rows, p.g, p.bs.shift,
                 p.bs.nb, p.bs.chunk, (const unsigned*)ctx->bin_mat.p, (const int*)p.bin.plan, (float4*)ctx->bin_rec.p, (int*)ctx->cell_own.p, cell_oth,
                 p.bin.tickets);
}

// First half of a pass: per-cell counts of owned / other points in cell_own / cell_oth (and, while the box is deferred,
// the cloud's PackRed record on its way to pinned memory).  clock (may be null): a call's begin that has not been marked
// yet goes to k_bin_count as its word where that is the first launch, else in front of the clearing fills as its event.
static int launch_count(pct_ctx* ctx, const GridPoints& s, GridPass& p, pct_call_clock* clock) {
    const pct_grid& g = p.g;
    const int64_t n = s.n;
    const LevelPass no_pass, &lv = p.level ? *p.level : no_pass;         // (no wanted-edge array: ownership by the records' index range)
    const bool bin = p.build == GridBuild::Bin;            // (writes every counter itself: no clearing fill)
    PCT_TRY(pct_reserve(ctx, &ctx->cell_own, (size_t)g.ncell * sizeof(int)));
    if (clock && !bin) PCT_HIP(ctx, clock->begin_event(ctx->stream));
    if (!bin) PCT_HIP(ctx, hipMemsetAsync(ctx->cell_own.p, 0, (size_t)g.ncell * sizeof(int), ctx->stream));
    if (p.sharded) {
        PCT_TRY(pct_reserve(ctx, &ctx->cell_oth, (size_t)g.ncell * sizeof(int)));
        if (!bin) PCT_HIP(ctx, hipMemsetAsync(ctx->cell_oth.p, 0, (size_t)g.ncell * sizeof(int), ctx->stream));
    }
    if (bin) PCT_TRY(bin_scratch(ctx, p.bs, n, &p.bin));
    int* cell_oth = p.sharded ? (int*)ctx->cell_oth.p : nullptr;
    PackRed* parts = s.deferred_box ? red_parts(ctx) : nullptr;
    const int nhb = grid_1d(n, kBlock, 0);
    if (bin) {
        const BinShape& bs = p.bs;
        unsigned long long* begin_stamp = clock ? clock->begin_word() : nullptr;
        s.raw ? launch_bin_count<true>(ctx, n, p, parts, begin_stamp) : launch_bin_count<false>(ctx, n, p, parts, begin_stamp);
        PCT_LAUNCH(k_bin_colscan, dim3((bs.nb + kBinScanCols - 1) / kBinScanCols), dim3(kBinScanCols * kBinScanGroups), 0, ctx->stream,
                   (unsigned*)ctx->bin_mat.p, bs.ntiles, bs.nb, p.bin.tot);
        PCT_LAUNCH(k_bin_plan, dim3(1), dim3(1024), 0, ctx->stream, (const unsigned*)p.bin.tot, bs.nb, bs.chunk, p.bin.plan, p.bin.items);
        s.raw ? launch_bin_scatter<true>(ctx, n, p, cell_oth) : launch_bin_scatter<false>(ctx, n, p, cell_oth);
        PCT_LAUNCH(k_bin_cells, dim3(bs.max_items + 1), dim3(kBinBlock), p.bin.lds, ctx->stream, (const float4*)ctx->bin_rec.p, (const int*)p.bin.plan,
                   (const int4*)p.bin.items, g, bs.shift, (int)ctx->q_begin, (int)ctx->q_end, (int*)ctx->cell_own.p, cell_oth,
                   (int*)ctx->bin_base.p, (const PackRed*)parts, bs.ntiles, (PackRed*)ctx->red.p, pin_red(ctx), p.items_q, bs.chunk,
                   p.bin.brec, p.bin.bsq, p.bin.tickets);
    } else if (p.build == GridBuild::AtomicRaw) {
        PCT_LAUNCH(k_hist_raw, dim3(nhb), dim3(kBlock), 0, ctx->stream, ctx->xyz_view, n, g, s.g_begin, s.g_end, (int*)ctx->cell_of.p,
                   (int*)ctx->cell_fill.p, (int*)ctx->cell_own.p, cell_oth, parts);
        if (parts) PCT_TRY(red_fold(ctx, nhb, false));
    } else if (p.build == GridBuild::AtomicBase) {
        PCT_LAUNCH(k_hist_agg, dim3(nhb), dim3(kBlock), 0, ctx->stream, p.src, n, g, lv.want, lv.lo, lv.hi, p.sub_box ? 1 : 0,
                   (int*)ctx->cell_of.p, (int*)ctx->cell_fill.p, (int*)ctx->cell_own.p, (int*)ctx->cell_oth.p);
    } else {
        PCT_LAUNCH(k_hist, dim3(nhb), dim3(kBlock), 0, ctx->stream, p.src, n, g, s.g_begin, s.g_end, lv.want, lv.lo, lv.hi,
                   p.sub_box ? 1 : 0, (int*)ctx->cell_of.p, (int*)ctx->cell_fill.p, (int*)ctx->cell_own.p, cell_oth);
    }
    return PCT_OK;
}

// Between the halves: cell starts, the ordered work list (occ) and -- in pinned memory from PCT_EV_SCAN_TOTALS on -- the
// totals and the occupancy statistic the pass is judged by.
// The counting sort (Bin) has left one scan record per bucket (k_bin_cells) and scans inside the buckets itself
// (k_bin_place): one launch here, over the buckets' records.  The other builds: k_scan_sums and k_scan_apply over tiles of
// kScanTile cells.
static int launch_scan(pct_ctx* ctx, const GridPass& p, int nblk) {
    const bool bin = p.build == GridBuild::Bin;
    const int items_q = p.items_q;
    const int* cell_oth = p.sharded ? (const int*)ctx->cell_oth.p : nullptr;
    if (!bin) PCT_TRY(pct_reserve(ctx, &ctx->scan_tmp, (size_t)(nblk + 1) * sizeof(int4) + (size_t)nblk * sizeof(unsigned long long)));
    int4* tmp = bin ? p.bin.brec : (int4*)ctx->scan_tmp.p;
    unsigned long long* sq_part = bin ? p.bin.bsq : (unsigned long long*)((int4*)ctx->scan_tmp.p + nblk + 1);
    if (bin) nblk = p.bs.nb;
    PCT_TRY(pct_reserve(ctx, &ctx->cell_cnt, (size_t)(p.g.ncell + 1) * sizeof(int)));
    PCT_TRY(pct_reserve(ctx, &ctx->own_start, (size_t)(p.g.ncell + 1) * sizeof(int)));
    PCT_TRY(pct_reserve(ctx, &ctx->occ, (size_t)p.occ_cap * sizeof(int2)));
    if (!bin)
        PCT_LAUNCH(k_scan_sums, dim3(nblk), dim3(kBlock), 0, ctx->stream, (const int*)ctx->cell_own.p, cell_oth, p.g.ncell, items_q, tmp, sq_part);
    PCT_TRY(pct_reserve(ctx, &ctx->counters, sizeof(pct_dev_words)));
    PCT_LAUNCH(k_scan_tiles, dim3(1), dim3(1024), 0, ctx->stream, tmp, nblk,
               (const unsigned long long*)sq_part, pin_totals(ctx), (unsigned long long*)&pct_dev(ctx)->sweep);
    ctx->counters_clean = true;
    // the totals this pass is judged by (and, with a deferred pack, the cloud's box) are in pinned memory from here on:
    // the host waits for THIS point, not for the end of the stream -- while it wakes up, decides and enqueues the
    // sweep, the device applies the scan and scatters the records (18 us at 1 M points in the counting sort, which does
    // both in k_bin_place, and no gap in front of the sweep: profiles/r11_bucket_scan_ab.txt; the read-back used to be
    // ~25 us of an idle device).  A pass that is rejected has scattered for nothing, as before.
    PCT_HIP(ctx, hipEventRecord(ctx->ev[PCT_EV_SCAN_TOTALS], ctx->stream));
    if (!bin)
        PCT_LAUNCH(k_scan_apply, dim3(nblk), dim3(kBlock), 0, ctx->stream, (const int*)ctx->cell_own.p, cell_oth, p.g.ncell, items_q,
                   (const int4*)tmp, (int*)ctx->cell_cnt.p, (int*)ctx->own_start.p, (int2*)ctx->occ.p);
    return PCT_OK;
}

// Second half, after the scan: every record to its place in sorted4 (owned_pos, sorted4d and -- unless lazy -- row_of along).
static int launch_place(pct_ctx* ctx, const GridPoints& s, const GridPass& p) {
    const pct_grid& g = p.g;
    const int64_t n = s.n;
    // (the chained sweep's passes read each other's lists: its first pass keeps row_of complete)
    const bool lazy_rows = p.build == GridBuild::Bin && !p.level;
    ctx->row_of_valid = !lazy_rows;
    ctx->row_of_rows = p.n_owned;
    ctx->row_of_begin = (int)ctx->q_begin;
    const int* cell_oth = p.sharded ? (const int*)ctx->cell_oth.p : nullptr;
    const double4* pts4d = ctx->has_f64 ? (const double4*)ctx->pts4d.p : nullptr;
    double4* sorted4d = ctx->has_f64 ? (double4*)ctx->sorted4d.p : nullptr;
    if (p.build == GridBuild::Bin)
        PCT_LAUNCH(k_bin_place, dim3(p.bs.max_items), dim3(kBinBlock), p.bin.lds + (p.sharded ? p.bin.lds / 2 : 0), ctx->stream,
                   (const float4*)ctx->bin_rec.p, (const int*)p.bin.plan, (const int4*)p.bin.items, g, p.bs.shift, (int)ctx->q_begin,
                   (int)ctx->q_end, n, p.n_owned, p.bs.nb, p.items_q, (const int4*)p.bin.brec, (const int*)ctx->cell_own.p, cell_oth,
                   (const int*)ctx->bin_base.p, (int*)ctx->cell_cnt.p, (int*)ctx->own_start.p, (int2*)ctx->occ.p, p.occ_cap,
                   (float4*)ctx->sorted4.p,
                   lazy_rows ? nullptr : (int*)ctx->row_of.p, (int*)ctx->owned_pos.p, pts4d, sorted4d);
    else if (p.build == GridBuild::AtomicRaw)
        PCT_LAUNCH(k_scatter_raw, dim3(grid_1d(n, kBlock, 0)), dim3(kBlock), 0, ctx->stream, ctx->xyz_view, (const int*)ctx->cell_of.p,
                   (const int*)ctx->cell_cnt.p, (const int*)ctx->cell_own.p, (const int*)ctx->own_start.p, (const int*)ctx->cell_fill.p, n,
                   s.g_begin, (float4*)ctx->sorted4.p, (int*)ctx->row_of.p, (int*)ctx->owned_pos.p, pts4d, sorted4d);
    else                    // AtomicBase, AtomicPacked
        PCT_LAUNCH(k_scatter, dim3(grid_1d(n, kBlock, 0)), dim3(kBlock), 0, ctx->stream, p.src, (const int*)ctx->cell_of.p,
                   (const int*)ctx->cell_cnt.p, (const int*)ctx->cell_own.p, (const int*)ctx->own_start.p, (const int*)ctx->cell_fill.p, n,
                   s.g_begin, (float4*)ctx->sorted4.p, (int*)ctx->row_of.p, (int*)ctx->owned_pos.p, pts4d, sorted4d);
    PCT_HIP(ctx, hipGetLastError());
    return PCT_OK;
}

// PCT_GRID_DEBUG: the work list a bin pass planned (debugging only: waits for the stream)
static int debug_bin_plan(pct_ctx* ctx, const GridPass& p) {
    int pw[3] = {0, 0, 0};
    PCT_HIP(ctx, hipMemcpyAsync(pw, p.bin.plan, sizeof(pw), hipMemcpyDeviceToHost, ctx->stream));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    fprintf(stderr, "[grid] bin build: %d buckets of %d cells, %d tiles of %d rows, %d work items of up to %d records, %d of them in %d shared buckets\n",
            p.bs.nb, 1 << p.bs.shift, p.bs.ntiles, p.bs.tile_rows, pw[0], p.bs.chunk, pw[1], pw[2]);
    return PCT_OK;
}

// ---- bookkeeping of an accepted build ------------------------------------------------------------------------------
static int commit_grid(pct_ctx* ctx, const GridPoints& s, pct_grid g, const EdgeSearch& es, int iters, double m_last, int4 tot,
                       int64_t n_owned, bool plain, bool sub_box) {          // plain: no pass of the chained sweep
    const bool level_pass = es.level_edge > 0;
    const int64_t n = s.n;
    // faces of the culling box become limits of what the grid can vouch for (cell units from the origin)
    for (int ax = 0; ax < 3; ++ax) {
        const double o = ax == 0 ? g.ox : ax == 1 ? g.oy : g.oz;
        g.lim_lo[ax] = ctx->culled ? ((double)s.kept_box.lo[ax] - o) * g.inv_cell : -INFINITY;
        g.lim_hi[ax] = ctx->culled ? ((double)s.kept_box.hi[ax] - o) * g.inv_cell : INFINITY;
    }
    if (pct_getenv("PCT_GRID_DEBUG"))
        fprintf(stderr, "[grid] box [%g %g %g]-[%g %g %g] edge %g dims %d x %d x %d = %lld cells, %d passes, occupancy %.1f, items %d\n", s.bbox[0],
                s.bbox[1], s.bbox[2], s.bbox[3], s.bbox[4], s.bbox[5], g.cell, g.nx, g.ny, g.nz, (long long)g.ncell, iters, m_last, tot.y);
    ctx->grid = g;
    ctx->tm.grid_iters += iters;
    ctx->tm.cells = g.ncell;
    ctx->tm.cell_size = g.cell;
    ctx->tm.grid_points = n;
    ctx->tm.occupancy = m_last;
    if (s.src != GridSource::CulledPack && plain) {       // remember the box for the next similar cloud
        for (int a = 0; a < 6; ++a) ctx->spec_bbox[a] = s.bbox[a];
        if (s.red.cnt > 0)                // raw bounding box of this cloud (before trimming)
            for (int a = 0; a < 6; ++a) ctx->spec_raw[a] = order_float(s.red.bb[a]);
        ctx->spec_n = ctx->n;
        ctx->spec_valid = true;
    }
    if (m_last > 0 && !level_pass) {        // the warm start of the next build
        ctx->hint_edge = es.hint_after(g.cell, m_last);
        ctx->hint_guess = es.first_guess;
        ctx->hint_target = es.target;
    }
    if ((tot.x != n && !sub_box) || tot.x > n || tot.z != n_owned)
        return pct_fail(ctx, PCT_ERR_INVALID, "cell scan totals %d/%d != %lld/%lld", tot.x, tot.z, (long long)n, (long long)n_owned);
    // A uniform cell list cannot resolve every cloud (tight clusters very far apart exhaust the cell budget):
    // refuse when the sweep would degenerate into an all-pairs scan of hours rather than run it.
    if (!level_pass && m_last > 64.0 * es.target && m_last * 27.0 * (double)n_owned > 1e12)
        return pct_fail(ctx, PCT_ERR_INVALID,
                        "the cell list cannot resolve this cloud: a point shares its cell with %.0f others on average at the "
                        "smallest usable cell edge %.3g (%lld cells); thin it out or split it into compact pieces",
                        m_last, g.cell, (long long)g.ncell);
    ctx->n_items = tot.y;
    ctx->nonempty_cells = tot.w;
    ctx->n_occ = tot.y;
    ctx->tm.occupied_cells = tot.y;
    ctx->grid_valid = true;
    // what pct_query_points_algo may send caller-supplied queries through: every point filed, every point owned
    ctx->grid_whole = plain && !sub_box && !ctx->culled && n == ctx->n && ctx->q_begin == 0 && ctx->q_end == ctx->n &&
                      ctx->slab_parts == 0;
    return PCT_OK;
}

// Chooses the cell edge so that a point shares its cell with about
// factor*(k+1) points, then counting-sorts the cloud.  With that occupancy the
// 27-cell stencil (guaranteed radius = one cell edge) contains the k+1 nearest
// points for nearly every query of a surface-like cloud; the sweep kernel
// widens ring by ring for the rest.
int pct_build_grid(pct_ctx* ctx, int32_t k, double eps, bool may_give_up, GridVerdict* out, pct_call_clock* clock, LevelPass* pass) {
    *out = GridVerdict::Built;
    ctx->grid_valid = false;       // (the lists are being rewritten: valid again once a build is committed)
    // measured optima on surface clouds (tools/tune_factor.py): larger cells cost candidates, smaller ones cost
    // trips to the exact sweep; the LDS staging capacity caps the large side
    const double factor = ctx->occupancy_factor > 0 ? ctx->occupancy_factor : pct_default_factor(k);
    const double target = factor * (k + 1);
    // (the first pass of a chained sweep only has to be roughly right: the later passes adapt)
    // cell budget: 2^27 cells (1.6 GB of counters and starts) serve surfaces of up to a few million points; beyond,
    // 32 cells per point up to 2^30 (a 60 M-point torus wants 3.3e8 cells: capped at 2^27 its cells held 51 points
    // instead of 29.5, the staging area overflowed and the sweep took 235 ms instead of ~40)
    int64_t cell_cap = (int64_t)1 << 27;
    if (pass) cell_cap = (int64_t)1 << 24;
    else if (32 * ctx->n > cell_cap) cell_cap = 32 * ctx->n < ((int64_t)1 << 30) ? 32 * ctx->n : (int64_t)1 << 30;
    const bool by_want = pass && pass->want;          // level passes: ownership by wanted-edge band
    const bool slab = ctx->slab_parts >= 1 && !by_want;
    const float* sub_box = pass && pass->edge > 0 ? pass->box : nullptr;
    const bool bin_allowed = !by_want && !sub_box && !slab && !pct_getenv("PCT_GRID_ATOMIC");
    // queries per work item: 16 - 20 measured best for k_knn_pair and k_knn_duo (one staged stencil serves more queries; a
    // cell of ~28 points is one or two items; 1 M torus, k = 50: sweep 0.376 | 0.366 | 0.363 | 0.364 | 0.370 ms at 12 | 14 | 18 |
    // 20 | 24; the reference's lattice torus 0.510 | 0.489 | 0.500 at 12 | 16 | 18; k = 80: 0.597 | 0.574 | 0.583 --
    // tools/items_q_probe.py, tools/lattice_probe.py)
    int items_q = 16;
    if (const char* e = pct_getenv("PCT_ITEMS_Q")) { const int v = atoi(e); if (v >= 1 && v <= 64) items_q = v; }   // tuning aid

    // A restart first rules itself out on the handle (select_source: no culling; below: no speculation), so a build
    // starts over twice at the most; everything else a restarted build finds in ctx is what any build finds.
    for (int attempt = 0; attempt < 3; ++attempt) {
        ctx->tm.grid_iters = 0;
        if (slab) PCT_TRY(slab_split(ctx));                // (sets the owned count: q_begin = 0, q_end = this slab's population)
        const int64_t n_owned = pct_call_rows(ctx, pass);
        const bool sharded = by_want || ctx->q_begin > 0 || ctx->q_end < ctx->n || slab;   // some points are candidates only
        GridPoints s;
        bool restart = false;
        PCT_TRY(select_source(ctx, k, target, slab, n_owned, sharded, pass, &s, &restart, clock));
        if (restart) continue;
        const int64_t n = s.n;
        ctx->items_q = items_q;
        PCT_TRY(reserve_lists(ctx, n, n_owned, by_want));
        EdgeSearch es = edge_search(ctx, s, target, eps, pass);
        double a = es.first();
        GridPass p = {};
        p.src = s.from_base ? pass->base : (const float4*)ctx->pts4.p;
        p.n_owned = n_owned; p.level = pass; p.sharded = sharded; p.sub_box = sub_box != nullptr; p.items_q = items_q;
        int iters = 0;
        int4 tot = make_int4(0, 0, 0, 0);
        double m_last = 0;
        // Every pass runs the whole build (histogram, scan, scatter) and only then reads back the occupancy statistic
        // together with the scan totals: the first cell size is accepted in the common case, which then costs ONE host
        // synchronisation instead of two; a rejected size costs a speculative scatter.
        for (int it = 0; it < es.max_iter; ++it) {
            a = es.clamp_eps(a);
            size_grid(sub_box, s.bbox, a, &p.g);
            // PCT_KNN_AUTO: a surface wants about a third of a cell per point; an edge that asks for 16 cells per point was
            // steered there by a dense minority (the size-biased occupancy) -- a 1/r^2 scan wants 130 per point, 1.6 ms of
            // counters and scans that the hierarchical list does not need.  Nothing was built: the caller goes there.
            if (!by_want && !(es.level_edge > 0) && p.g.ncell > 16 * n && p.g.ncell > ((int64_t)1 << 20)) {
                if (it == 0 && es.hinted) {
                    // ... unless the edge is the PREVIOUS cloud's (same size, similar box, another density -- a torus after
                    // a 1/r^2 scan inherited its 130 cells per point): this cloud's own first guess, then
                    a = es.fallback_first();
                    size_grid(sub_box, s.bbox, a, &p.g);
                } else if (may_give_up) {
                    *out = GridVerdict::GaveUp;
                    ctx->grid_valid = false;
                    return PCT_OK;
                }
            }
            bool hit_cap = false;            // the cell budget, not the occupancy target, set this edge
            while (p.g.ncell > cell_cap) {
                a *= cbrt((double)p.g.ncell / (double)cell_cap) * 1.01;
                size_grid(sub_box, s.bbox, a, &p.g);
                hit_cap = true;
            }
            const pct_grid& g = p.g;
            p.bs = bin_allowed ? bin_shape(n, g.ncell, sharded) : BinShape{};
            p.build = choose_build(bin_allowed, p.bs, s);
            const bool bin = p.build == GridBuild::Bin;
            p.occ_cap = (n_owned < g.ncell ? n_owned : g.ncell) + n_owned / items_q + 16;
            PCT_TRY(launch_count(ctx, s, p, clock));
            const int nblk = (int)((g.ncell + kScanTile - 1) / kScanTile);
            if (pct_getenv("PCT_GRID_DEBUG"))
                fprintf(stderr, "[grid] pass %d: n %lld owned %lld edge %g dims %d x %d x %d = %lld cells (%d scan tiles), box [%g %g %g]-[%g %g %g]\n", it,
                        (long long)n, (long long)n_owned, a, g.nx, g.ny, g.nz, (long long)g.ncell, nblk, s.bbox[0], s.bbox[1], s.bbox[2], s.bbox[3], s.bbox[4], s.bbox[5]);
            PCT_TRY(launch_scan(ctx, p, nblk));
            PCT_TRY(launch_place(ctx, s, p));
            PCT_HIP(ctx, hipEventSynchronize(ctx->ev[PCT_EV_SCAN_TOTALS]));
            if (s.deferred_box) {
                const BoxCheck box = check_deferred_box(ctx, &s);
                if (box == BoxCheck::NonFinite) return pct_fail(ctx, PCT_ERR_NONFINITE, "Non-finite values in input points");
                if (box == BoxCheck::Restart) {          // a different cloud: start over the regular way
                    ctx->spec_valid = false;
                    restart = true;
                    break;
                }
            }
            if (bin && pct_getenv("PCT_GRID_DEBUG")) PCT_TRY(debug_bin_plan(ctx, p));
            tot = pin_totals(ctx)->tot;
            m_last = (double)pin_totals(ctx)->sumsq / (double)(n_owned > 0 ? n_owned : 1);
            ++iters;
            if (es.accept(m_last, a, g.ncell, cell_cap, hit_cap, it)) break;
            a = es.next(m_last, a);
        }
        if (restart) continue;
        PCT_TRY(commit_grid(ctx, s, p.g, es, iters, m_last, tot, n_owned, pass == nullptr, p.sub_box));
        if (pass && !by_want) memcpy(pass->base_box, s.bbox, sizeof(s.bbox));     // first pass of a chain: its (trimmed) box serves the later ones
        return PCT_OK;
    }
    return pct_fail(ctx, PCT_ERR_INVALID, "cell-list build: restarted more than twice");
}

// Every reader of ctx->row_of calls this first (pct_get_fit's gather, the row export, the neighbour study).
int pct_ensure_row_of(pct_ctx* ctx) {
    if (ctx->row_of_valid) return PCT_OK;
    const int64_t rows = ctx->row_of_rows;
    if (rows > 0) {
        PCT_LAUNCH(k_bin_row_of, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, ctx->stream, (const float4*)ctx->sorted4.p,
                   (const int*)ctx->owned_pos.p, rows, ctx->row_of_begin, (int*)ctx->row_of.p);
        PCT_HIP(ctx, hipGetLastError());
    }
    ctx->row_of_valid = true;
    return PCT_OK;
}

int pct_launch_gather_int(pct_ctx* ctx, const int* d_map, int* d_inout, int64_t n) {
    PCT_LAUNCH(k_gather_int, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_map, d_inout, n);
    PCT_HIP(ctx, hipGetLastError());
    return PCT_OK;
}

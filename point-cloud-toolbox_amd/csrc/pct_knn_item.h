// The start of a work item of the fast sweeps, written once for k_knn_fast (pct_knn_fast.hip), k_knn_pair
// (pct_knn_pair.hip) and k_knn_duo (pct_knn_duo.hip): the exclusive prefix of the run lengths, the overflow test, the
// hand-off of an overflowing item to the redo list and the set-up of the keys; and, for the two scalar-lean kernels, the
// item's decode (tree form and uniform form) with its stencil runs and the prefetch of its queries.  The staging loop that
// follows stays in each kernel: it records the run index of a slot in the kernel's own way.  Also here: the kernel
// argument of the lean kernels (PairArgs) and the host helpers every family's launch uses.
#pragma once
#include "pct_knn_net.h"

namespace {

typedef float float2v __attribute__((ext_vector_type(2)));      // two candidates per packed float32 instruction

struct PairArgs {
    const float4* pts;        // cell-sorted candidate records {x, y, z, public index}
    const double4* ptsd;      // Q64: the native float64 coordinates in the same order (queries; the candidates stay float32, pct:74)
    const int* cell_start;
    const int* cell_own;
    const int* own_start;
    const int2* items;        // work items {cell, chunk of items_q queries}
    int* nbr_pos;
    float* nbr_dist;          // unused when DIST = false
    int* nbr_cnt;             // EPS only
    int* redo;
    int* redo_count;
    pct_sweep_words* counters;
    int n_items, items_q;
    int items_per_xcd;        // blocks are dealt to the 8 XCDs in turn: block b takes item (b % 8) * items_per_xcd + b / 8, so that
                              // the items one XCD's L2 serves at a time are neighbours in cell order (they share most of their stencils)
    int k, pitch;
    int stats;
    int seed;                 // KnnArgs::redo_seed: an item whose stencil overflows the staging area runs on its first CAP slots
    int adopt;                // KnnArgs::redo_adopt: a redo row whose list is the proven set of the 27 cells is marked (kRedoTrusted)
    unsigned magic_x, magic_xy;      // cell -> (cx, cy, cz) by multiplication: q = (x * magic) >> shift, exact for x < 2^30
    int shift_x, shift_xy;
    double eps2;
    pct_grid g;
    // TREE (the hierarchical cell list, pct_tree.hip): an item is a run of queries of one segment; g = the finest level's grid
    const int4* tree_seg;     // per segment {level, cx, cy, cz}
    const int2* tree_runs;    // per segment 27 x {first position, points}, centre cell first
    int tree_bits;
    unsigned long long* stamp;       // a call timed by the device clock: the sweep's entry (pct_stamp.h), else null
};

PairArgs make_pair_args(const pct_ctx* ctx, const KnnArgs& a, bool tree, int* redo, int* redo_count) {
    PairArgs pa = {};
    pa.pts = a.pts; pa.ptsd = a.ptsd; pa.cell_start = a.cell_start;
    pa.items = (const int2*)ctx->occ.p;
    pa.nbr_pos = a.nbr_pos; pa.nbr_dist = a.nbr_dist; pa.nbr_cnt = a.nbr_cnt;
    pa.redo = redo; pa.redo_count = redo_count; pa.counters = a.counters;
    pa.n_items = (int)ctx->n_items; pa.items_q = ctx->items_q;
    pa.k = a.k; pa.pitch = a.pitch; pa.stats = a.stats; pa.eps2 = a.eps2; pa.g = a.g;
    pa.seed = a.redo_seed;
    pa.adopt = a.redo_adopt;
    pa.stamp = a.stamp_sweep;
    pa.items_per_xcd = pct_getenv("PCT_NO_XCD_MAP") ? 0 : (int)((ctx->n_items + 7) / 8);
    if (tree) {
        pa.tree_seg = a.tree_seg; pa.tree_runs = a.tree_runs; pa.tree_bits = a.tree_bits;
        return pa;
    }
    pa.cell_own = a.cell_own; pa.own_start = a.own_start;
    // x / d = (x * magic) >> shift for every x < 2^30 (cell ids): shift = 30 + ceil(log2 d), magic = ceil(2^shift / d) < 2^32
    const auto magic = [](unsigned d, unsigned* mg, int* sh) {
        int l = 0;
        while ((1ull << l) < d) ++l;
        *sh = 30 + l;
        *mg = (unsigned)(((1ull << *sh) + d - 1) / d);
    };
    magic((unsigned)a.g.nx, &pa.magic_x, &pa.shift_x);
    magic((unsigned)a.g.nx * (unsigned)a.g.ny, &pa.magic_xy, &pa.shift_xy);
    return pa;
}

// Runtime values -> template arguments: f(std::bool_constant...) for the bools given, f(std::integral_constant<int, i>) for i < N
template <class F, class... Rest>
void with_bools(F&& f, bool b, Rest... rest) {
    if constexpr (sizeof...(rest) == 0) {
        if (b) f(std::true_type{}); else f(std::false_type{});
    } else {
        if (b) with_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
        else with_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
    }
}
template <int N, class F>
void with_index(int i, F&& f) {
    if constexpr (N > 0) {
        if (i == N - 1) f(std::integral_constant<int, N - 1>{}); else with_index<N - 1>(i, f);
    }
}

// ---------------------------------------------------------------------------
// One work item: a cell and <= items_q of its owned queries (uniform cell list), or a run of queries of one octree
// segment (TREE, the hierarchical cell list of pct_tree.hip).  load_item_head serves the two lean kernels; k_knn_fast
// keeps its own copy of the decode (see there) and shares everything after it.
// ---------------------------------------------------------------------------
template <bool TREE>
struct ItemHead {
    int cx, cy, cz;           // the item's cell (TREE: in the grid of its level)
    int qs, nq, row0;         // first query (sorted position), queries, neighbour-table row of the first query
    int run_len, run_s;       // per lane: the range of the cloud lane t < NRUNS stages (9 x-runs of the 27-cell stencil | TREE: 27 cells)
    pct_grid g_lvl;           // TREE: the grid of the item's level
};

// cell id -> (cx, cy, cz) by two multiplications (PairArgs::magic_*; k_knn_fast divides): no integer division on a
// kernel whose scalar unit is as busy as its vector units
__device__ __forceinline__ void split_cell(const PairArgs& a, int cell, int& cx, int& cy, int& cz) {
    cz = (int)(((unsigned long long)(unsigned)cell * a.magic_xy) >> a.shift_xy);
    const int rem = cell - cz * (a.g.nx * a.g.ny);
    cy = (int)(((unsigned long long)(unsigned)rem * a.magic_x) >> a.shift_x);
    cx = rem - cy * a.g.nx;
}

// A tree item whose segment is negative belongs to a segment that was split (pct_tree.hip: k_tree_refine): nothing to do.
// (The kernels test this themselves, before load_item_head: an exit taken through the helper's return value costs
// k_knn_duo<EPS, TREE> four architectural registers.)
template <bool TREE>
__device__ __forceinline__ bool item_of_split_segment(const int2 it2) {
    if constexpr (TREE) return __builtin_amdgcn_readfirstlane(it2.y) < 0;
    return false;
}

template <bool TREE>
__device__ __forceinline__ void load_item_head(const PairArgs& a, const int2 it2, const int lane, ItemHead<TREE>& h) {
    h.run_s = 0;
    h.run_len = 0;
    if constexpr (TREE) {
        // item = {first query (Morton position = table row) | (queries - 1) << 26, segment >= 0}
        const int seg = __builtin_amdgcn_readfirstlane(it2.y);
        const unsigned packed = (unsigned)__builtin_amdgcn_readfirstlane(it2.x);
        h.qs = (int)(packed & 0x3ffffffu);
        h.nq = (int)(packed >> 26) + 1;
        h.row0 = h.qs;
        const int4 hd = a.tree_seg[seg];
        const int level = __builtin_amdgcn_readfirstlane(hd.x);
        h.cx = __builtin_amdgcn_readfirstlane(hd.y);
        h.cy = __builtin_amdgcn_readfirstlane(hd.z);
        h.cz = __builtin_amdgcn_readfirstlane(hd.w);
        // the grid of this level: edges scale by exact powers of two, so (x - o) * inv_cell - cx lies in [0, 1) for
        // every point the Morton code put into the cell
        h.g_lvl = a.g;
        h.g_lvl.cell = __builtin_ldexp(a.g.cell, level);
        h.g_lvl.inv_cell = __builtin_ldexp(a.g.inv_cell, -level);
        h.g_lvl.nx = h.g_lvl.ny = h.g_lvl.nz = 1 << (a.tree_bits - level);
        if (lane < 27) {
            const int2 r = a.tree_runs[(int64_t)seg * 27 + lane];
            h.run_s = r.x;
            h.run_len = r.y;
        }
    } else {
        const int* __restrict__ cs = a.cell_start;
        const int cell = __builtin_amdgcn_readfirstlane(it2.x);
        const int chunk = __builtin_amdgcn_readfirstlane(it2.y);
        const int nx = a.g.nx, ny = a.g.ny, nz = a.g.nz;
        split_cell(a, cell, h.cx, h.cy, h.cz);
        const int c0 = cs[cell];
        h.qs = c0 + chunk * a.items_q;                              // owned points sit first in the cell
        h.nq = min(c0 + a.cell_own[cell], h.qs + a.items_q) - h.qs;
        h.row0 = a.own_start[cell] + chunk * a.items_q;             // neighbour-table row of query qs

        // ---- bounds of the 9 x-runs of the 27-cell stencil, fetched in parallel by lanes 0..8 (centre row first);
        // at the rim of the grid a run is clamped to the row, rows outside the grid stay empty
        if (lane < 9) {
            const int z = h.cz + kRowOrder[lane][0], y = h.cy + kRowOrder[lane][1];
            if (z >= 0 && z < nz && y >= 0 && y < ny) {
                const int row = (z * ny + y) * nx;
                h.run_s = cs[row + max(h.cx - 1, 0)];
                h.run_len = cs[row + min(h.cx + 1, nx - 1) + 1] - h.run_s;
            }
        }
    }
}

// exclusive prefix of the run lengths over lanes 0 .. NRUNS - 1 = first flat slot of every run; m = staged candidates
template <int NRUNS>
__device__ __forceinline__ void run_prefix(const int run_len, const int lane, int& my_pre, int& m) {
    my_pre = 0;
    int acc = 0;
#pragma unroll
    for (int t = 0; t < NRUNS; ++t) {
        my_pre = lane == t ? acc : my_pre;
        acc += __builtin_amdgcn_readlane(run_len, t);
    }
    m = acc;
}

// The stencil does not fit the staging area (dense cluster), or -- tree items -- it is crowded: a slot's run index has
// four bits, 16 non-empty ranges.  A surface meets about ten of its 27 stencil cells; more is a volume, where these
// items pay as little as uniform cells do.
template <bool TREE, int NRUNS>
__device__ __forceinline__ bool item_overflows(const int m, const int cap, const int run_len, const int lane) {
    const bool crowded = TREE && __popcll(__builtin_amdgcn_ballot_w64(lane < NRUNS && run_len > 0)) > 16;
    return m > cap || crowded;
}

// The exact sweep takes the whole item: its rows are appended to the redo list with ONE counter increment (an increment
// per query serialises at the memory side).  overflow: the item counts as a staging overflow in the statistics.
// No query of the item has run: every row gets -1 in its first column, so that whoever reads a redo row for the list the
// fast sweep left there (k_knn_exact, Sweep::seed) never takes what an earlier call wrote for one.
__device__ __forceinline__ void hand_item_to_redo(int* __restrict__ redo, int* __restrict__ redo_count, pct_sweep_words* counters,
                                                  const int stats, const int row0, const int nq, const int lane, const bool overflow,
                                                  int* __restrict__ nbr_pos, const int pitch) {
    int base = 0;
    if (lane == 0) base = atomicAdd(redo_count, nq);
    base = __builtin_amdgcn_readfirstlane(base);
    if (lane < nq) {
        redo[base + lane] = row0 + lane;
        nbr_pos[(int64_t)(row0 + lane) * pitch] = -1;
    }
    if (stats && lane == 0) {
        if (overflow) atomicAdd(&counters->lds_overflows, 1ull);
        atomicAdd(&counters->redone_queries, (unsigned long long)nq);
    }
}

// The item's own queries (<= items_q <= 64 consecutive sorted positions), one per lane: the float32 record and -- Q64, a
// float64 cloud -- the native coordinates and my_eq, the distance between the float64 query and its float32 rounding,
// rounded up (the float32 pre-selection measures from the rounded query: every bound taken from it moves by my_eq).
template <bool Q64>
__device__ __forceinline__ void load_queries(const float4* pts, const double4* ptsd, const int qs, const int nq,
                                             const int lane, float4& my_q, double& my_qx, double& my_qy, double& my_qz, float& my_eq) {
    my_q = make_float4(0.f, 0.f, 0.f, 0.f);
    my_qx = 0.; my_qy = 0.; my_qz = 0.;
    my_eq = 0.f;
    if (lane < nq) {
        my_q = pts[qs + lane];
        if constexpr (Q64) {
            const double4 qd = ptsd[qs + lane];
            my_qx = qd.x; my_qy = qd.y; my_qz = qd.z;
        }
    }
    if constexpr (Q64) {
        const double ex = my_qx - (double)my_q.x, ey = my_qy - (double)my_q.y, ez = my_qz - (double)my_q.z;
        my_eq = (float)sqrt((ex * ex + ey * ey) + ez * ez) * (1.0f + 0x1p-22f);
        if (!(my_eq >= 0.f)) my_eq = INFINITY;        // NaN cannot happen with finite inputs; be safe
    }
}

// ---------------------------------------------------------------------------
// Keys: key = floor(d2 * scale), KEY_BITS wide.
// Key range: the cube of 27 cells vouches for at most 1.5 cell edges around a query (min(gx + 1, 2 - gx) <= 1.5 per
// axis, guaranteed_r2), so no accepted list holds a squared distance beyond 2.25 cell^2: candidates farther out
// (the stencil reaches 12 cell^2) may share the saturated key -- if the (k+1)-th is among them the query was
// beyond the guarantee anyway.  (Until round 2 the range was the stencil's 12.1 cell^2: keys 5x coarser, equal
// keys 5x as frequent.  Queries at the rim of the grid, whose guarantee is unbounded on a side, can lose a
// provable answer to the saturation check: exact sweep.)
// ---------------------------------------------------------------------------
constexpr double kKeyRange = 2.3;

template <int KEY_BITS>
struct KeySetup {
    static constexpr unsigned key_max = (1u << KEY_BITS) - 1u;
    double scale;
    unsigned my_gkey;         // per query (lane l = query l): the largest key the stencil vouches for
    unsigned eps_key;         // ceil(eps^2 * scale): the whole eps ball must be inside the guaranteed radius too
    float cell2f;             // one cell edge squared: the first guess of the float32 threshold
    float eps2a;              // eps^2 rounded up generously in float32: everything inside the eps ball passes the pre-selection, the exact test follows on the survivors
    double eps1;              // eps itself, rounded up
};

// G: the item's grid; this lane's query as the exact keys measure from it: the float32 record widened, or (native) the
// float64 coordinates
template <int KEY_BITS, bool EPS>
__device__ __forceinline__ KeySetup<KEY_BITS> make_key_setup(const pct_grid& G, const int cx, const int cy, const int cz, const float4& my_q,
                                                             const bool native, const double my_qx, const double my_qy, const double my_qz,
                                                             const double eps2) {
    KeySetup<KEY_BITS> s;
    const double edge = G.cell;
    s.scale = (double)(1u << KEY_BITS) / (kKeyRange * edge * edge);
    const double lqx = native ? my_qx : (double)my_q.x, lqy = native ? my_qy : (double)my_q.y, lqz = native ? my_qz : (double)my_q.z;
    // Per query, the largest key the stencil can vouch for: lane l evaluates query l once per item (the radius
    // guaranteed by the 27-cell cube depends on where the query sits inside its cell).  floor() keeps it conservative.
    const double gx = (lqx - G.ox) * G.inv_cell - cx;
    const double gy = (lqy - G.oy) * G.inv_cell - cy;
    const double gz = (lqz - G.oz) * G.inv_cell - cz;
    // 0xFFFFFFFF only when nothing bounds the answer (the cube covers the grid and no points were left out):
    // that alone vouches for "fewer than k+1 points exist".  A query clamped into a boundary cell from far
    // outside the grid box can have a finite guarantee beyond the key range: keep it below the sentinel.
    const double g2 = fmin(guaranteed_r2(G, cx, cy, cz, gx, gy, gz, 1), limit_r2(G, cx, cy, cz, gx, gy, gz));
    s.my_gkey = g2 == INFINITY ? 0xFFFFFFFFu : (unsigned)fmin(g2 * s.scale, 4294967294.0);
    s.eps_key = EPS && eps2 < 1e300 ? (unsigned)fmin(ceil(eps2 * s.scale), 4294967295.0) : 0xFFFFFFFFu;
    s.cell2f = (float)(edge * edge);
    s.eps2a = EPS ? (float)fmin(eps2 * (1.0 + 0x1p-18), 3.0e38) : INFINITY;
    s.eps1 = EPS ? sqrt(eps2) * (1.0 + 0x1p-50) : 0.0;
    return s;
}

}  // namespace

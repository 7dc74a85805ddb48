// k_knn_fast: the fast sweep in every form -- level passes, owned subsets, clouds outside the float32 window, the A/B
// switches -- with its launcher and the entry that picks the instantiation a plan names (pct_knn.hip: launch_sweep).
#include "pct_knn_item.h"

namespace {

// ---------------------------------------------------------------------------
// Fast sweep: wave = work item (one cell, <= items_q consecutive queries).
//
// Elements of the wave-wide network are single 32-bit integers
//     key << SLOT_BITS | payload
// payload = LDS slot of a staged stencil candidate (or, on the pre-selection path, the candidate's place in the
// compacted list of survivors, from which the slot is looked up afterwards); key = floor(d2 * scale) with the
// exact fp64 squared distance d2 and scale = 2^KEY_BITS / (2.3 cell^2), just above the largest squared distance the
// 27-cell stencil can VOUCH for (beyond it keys saturate).  The quantisation is a monotone map of the exact value, so
// wherever two keys differ the order is the exact order.  Equal keys among the first k+2 of the sorted selection are
// put in the exact order in place (order_equal_keys); a saturated (k+1)-th key, every query whose answer is
// not guaranteed to lie inside the stencil or inside what the float32 pre-selection kept, and whole items whose
// stencil does not fit the LDS staging area are appended to the redo list and done by k_knn_exact.  Unflagged
// results are therefore bit-identical to the exact path: the stored distance is recomputed in fp64 from the
// coordinates.  (DESIGN.md 4.2 walks through the steps.)
// ---------------------------------------------------------------------------

// waves per block of the fast sweep: chosen so that whole blocks fill the 160 KiB of LDS (waves are independent;
// R = 1: 6 blocks x 4 waves x 6.25 KiB, R = 2: 4 blocks x 4 waves x 9.5 KiB)
#ifndef PCT_FAST_WAVES
#define PCT_FAST_WAVES 4
#endif
template <int R> constexpr int kFastWaves = PCT_FAST_WAVES;

// EPS = the hybrid eps-ball query is on (candidates beyond eps do not count); without it every staged slot is a
// candidate and the per-batch eps compares and candidate counts drop out.
// PRE = float32 pre-selection (clouds whose query coordinates are the float32 tree coordinates): the threshold
// that cuts the staged candidates down to <= 64 R is searched on squared distances computed in packed float32
// (two candidates per instruction), and only the survivors get the exact fp64 distance and a key.  A float32
// squared distance of float32 points is within 5 * 2^-24 relative of the exact one (the difference of two
// floats is rounded once, then one product and two fused multiply-adds), so a candidate that was cut has an
// exact squared distance >= T (1 - 2^-20): the query is accepted only if its (k+1)-th exact key lies below that.

// Level passes (pct_levels.hip) want to know WHY a row was not answered: 1 = the stencil cannot vouch for the answer
// (cells too small for this query), 2 = the stencil overflowed the staging area (cells too large), 3 = anything else;
// they get it, with the stencil population, in the row's slot of redo_m.  Plain sweeps append the bare row to the list.

// PAIR (with PRE, R = 1): two queries of the item per loop trip, their instruction streams side by side in the same
// basic blocks -- they share the LDS reads of the candidates, and each hides the other's dependency stalls.
template <int R, bool EPS, bool PRE, bool PAIR = false, bool Q64 = false, bool TREE = false>
__global__ __launch_bounds__(64 * kFastWaves<R>, (TREE ? (R == 1 ? (PCT_TREE_CAP <= 512 ? 6 : PCT_TREE_CAP <= 768 ? 4 : 3) : (PCT_TREE_CAP2 <= 768 ? 4 : 3)) : R == 1 ? (Q64 ? 5 : 6) : 4)) void k_knn_fast(KnnArgs a, const int2* __restrict__ items, int64_t n_items,
                                                                  int items_q, int* __restrict__ redo,
                                                                  int* __restrict__ redo_count) {
    // (tree items: an octree level changes the population fourfold on a surface; segments whose stencil exceeds the
    // staging area are split further at build time (k_tree_refine), so the capacity trades refinement and trips to
    // the exact sweep against occupancy: 768 slots / 4 blocks per CU measured best -- 1/r^2 scan, 1 M points: fast
    // sweep 0.51 | 0.65 | 0.83 ms at 512 | 768 | 1024 slots, whole call 2.30 | 1.57 | 1.65 ms)
    constexpr int CAP = TREE ? (R == 1 ? PCT_TREE_CAP : PCT_TREE_CAP2) : R == 1 ? kStageCap : PCT_STAGE_CAP2;   // staged stencil candidates per wave
    // low bits of a network element: the staged slot of the candidate, or -- pre-selection -- its place in the
    // compacted list of survivors (6 / 7 bits; the slot is looked up in that list afterwards), which leaves three
    // more bits for the key and cuts key collisions eightfold
    constexpr int SLOT_BITS = PRE ? (R == 1 ? 6 : 7) : (R == 1 ? 9 : 10);
    constexpr int KEY_BITS = 32 - SLOT_BITS;
    constexpr int CAP_POW2 = 1024;          // slots < CAP <= 1024: masks a garbage list entry read for a padding element
    static_assert(CAP <= CAP_POW2, "staging capacity");
    static_assert(PRE || CAP <= (1 << SLOT_BITS), "slot field too narrow");
    __shared__ float s_cx[kFastWaves<R>][CAP];        // staged stencil, structure of arrays:
    __shared__ float s_cy[kFastWaves<R>][CAP];        // 12 B per candidate
    __shared__ float s_cz[kFastWaves<R>][CAP];
    __shared__ unsigned s_pend[kFastWaves<R>][64 * R];
    __shared__ unsigned short s_pend2[kFastWaves<R>][PAIR ? 64 * R : 2];    // survivors of the second query of a pair (16 bits: R = 2 stays at 4 blocks per CU)
    __shared__ int s_offc[kFastWaves<R>][16];          // sorted position - flat slot, per non-empty run

    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const int64_t item = (int64_t)blockIdx.x * kFastWaves<R> + w;
    if (item >= n_items) return;
    const SortLanes sort_dir = make_sort_lanes();

    // ---- the work item and its stencil runs.  (Written out here and not through load_item_head of pct_knn_item.h, which
    // the two lean kernels share: with it the four one-query forms <1, EPS, PRE, false> of this kernel need four more
    // architectural registers.  The tree form, the rim clamp and the row order must agree with it.)
    pct_grid g = a.g;
    const int* __restrict__ cs = a.cell_start;
    const int2 it2 = items[item];
    int cx, cy, cz, qs, nq, row0;
    constexpr int NRUNS = TREE ? 27 : 9;           // ranges of the cloud the stencil is staged from
    int run_s = 0, run_len = 0;
    float* cand_x = s_cx[w];
    float* cand_y = s_cy[w];
    float* cand_z = s_cz[w];
    unsigned* pend = s_pend[w];
    int* offc = s_offc[w];
    if constexpr (TREE) {
        // item = {first query (Morton position = table row) | (queries - 1) << 26, segment}
        const int seg = __builtin_amdgcn_readfirstlane(it2.y);
        if (seg < 0) return;                       // an item of a segment that was split (pct_tree.hip: k_tree_refine)
        const unsigned packed = (unsigned)__builtin_amdgcn_readfirstlane(it2.x);
        qs = (int)(packed & 0x3ffffffu);
        nq = (int)(packed >> 26) + 1;
        row0 = qs;
        const int4 hd = a.tree_seg[seg];
        const int level = __builtin_amdgcn_readfirstlane(hd.x);
        cx = __builtin_amdgcn_readfirstlane(hd.y);
        cy = __builtin_amdgcn_readfirstlane(hd.z);
        cz = __builtin_amdgcn_readfirstlane(hd.w);
        // the grid of this level: edges scale by exact powers of two, so (x - o) * inv_cell - cx lies in [0, 1) for
        // every point the Morton code put into the cell
        g.cell = __builtin_ldexp(a.g.cell, level);
        g.inv_cell = __builtin_ldexp(a.g.inv_cell, -level);
        g.nx = g.ny = g.nz = 1 << (a.tree_bits - level);
        if (lane < 27) {
            const int2 r = a.tree_runs[(int64_t)seg * 27 + lane];
            run_s = r.x;
            run_len = r.y;
        }
    } else {
        const int cell = __builtin_amdgcn_readfirstlane(it2.x);
        const int chunk = __builtin_amdgcn_readfirstlane(it2.y);
        cx = cell % g.nx;
        cy = (cell / g.nx) % g.ny;
        cz = cell / (g.nx * g.ny);
        qs = cs[cell] + chunk * items_q;                       // owned points sit first in the cell
        const int qe = min(cs[cell] + a.cell_own[cell], qs + items_q);
        nq = qe - qs;
        row0 = a.own_start[cell] + chunk * items_q;            // neighbour-table row of query qs

        // ---- bounds of the 9 x-runs of the 27-cell stencil, fetched in parallel by lanes 0..8 (centre row first)
        if (lane < 9) {
            const int z = cz + kRowOrder[lane][0], y = cy + kRowOrder[lane][1];
            if (z >= 0 && z < g.nz && y >= 0 && y < g.ny) {
                const int row = (z * g.ny + y) * g.nx;
                run_s = cs[row + max(cx - 1, 0)];
                run_len = cs[row + min(cx + 1, g.nx - 1) + 1] - run_s;
            }
        }
    }
    // the item's own queries (<= items_q <= 64 consecutive sorted positions), one per lane
    float4 my_q = make_float4(0.f, 0.f, 0.f, 0.f);
    double4 my_qd = make_double4(0., 0., 0., 0.);
    if (lane < nq) {
        my_q = a.pts[qs + lane];
        if (a.ptsd) my_qd = a.ptsd[qs + lane];
    }
    float my_eq = 0.f;       // Q64: distance between the float64 query and its float32 rounding, rounded up
    if constexpr (Q64) {
        const double ex = my_qd.x - (double)my_q.x, ey = my_qd.y - (double)my_q.y, ez = my_qd.z - (double)my_q.z;
        my_eq = (float)sqrt((ex * ex + ey * ey) + ez * ez) * (1.0f + 0x1p-22f);
        if (!(my_eq >= 0.f)) my_eq = INFINITY;        // NaN cannot happen with finite inputs; be safe
    }
    int my_pre, m;
    run_prefix<NRUNS>(run_len, lane, my_pre, m);
    pct_stamp(a.stamp_sweep);      // (behind the prologue's loads; block 0 takes neither return above on a uniform list: pct_stamp.h)
    unsigned long long n_flush = 0, n_step = 0, n_redo = 0;
    // rows of this item that go to the redo list: collected here (bit = query of the item, two bits of reason) and
    // appended with ONE counter increment when the item is done -- a counter increment per query serialises at the
    // memory side (~88 per us on one address: 10^5 failing queries of a cloud of uneven density cost a millisecond)
    unsigned long long redo_mask = 0ull, redo_why_lo = 0ull, redo_why_hi = 0ull;
    const auto note_redo = [&](int row, int why) {
        const int q = row - row0;
        redo_mask |= 1ull << q;
        redo_why_lo |= (unsigned long long)(why & 1) << q;
        redo_why_hi |= (unsigned long long)((why >> 1) & 1) << q;
    };

    // (a pass of the density-adaptive sweep, no eps bound: a stencil that does not even hold k+1 points cannot answer
    // any of the item's queries -- every point is binned somewhere -- so the item is classified "cells too small"
    // without being swept)
    const bool hopeless = !EPS && a.row_done != nullptr && m < a.k + 1;
    if (item_overflows<TREE, NRUNS>(m, CAP, run_len, lane) || hopeless) {
        // stencil does not fit the staging area (dense cluster): the exact sweep takes the whole item
        if (a.row_done) {
            // passes of the density-adaptive sweep keep no list: reason and stencil population go to the row's own
            // slot (a cloud of very uneven density fails hundreds of thousands of one-query items per pass, and as
            // many increments of ONE counter serialise for milliseconds)
            if (lane < nq) a.redo_m[row0 + lane] = ((hopeless ? 1 : 2) << 29) | min(m, (1 << 29) - 1);
            return;
        }
        hand_item_to_redo(redo, redo_count, a.counters, a.stats, row0, nq, lane, !hopeless, a.nbr_pos, a.pitch);
        return;
    }

    // ---- copy the runs as one flat range: all global loads of the item are in flight together.
    // Flat slot j belongs to the u-th non-empty run, u = (number of run starts <= j) - 1.  The run starts are
    // marked in a CAP-bit string in LDS (the list area is free here), so that a batch of 64 slots gets its u
    // from one 64-bit word and a masked bit count instead of eight compares; offc[u] = sorted position - flat
    // slot of run u.  u is also remembered in 4 bits per staged slot (run_code: this lane's slots lane,
    // 64 + lane, ...) for the store phase, which turns a slot back into a sorted position with one cross-lane
    // read and one LDS read.
    unsigned run_code[(CAP / 64 + 7) / 8];
#pragma unroll
    for (int i = 0; i < (CAP / 64 + 7) / 8; ++i) run_code[i] = 0u;
    {
        unsigned* bits = pend;
        static_assert(CAP / 32 <= 64 * R, "bit string does not fit the list area");
        if (lane < CAP / 32) bits[lane] = 0u;
        wave_lds_sync();
        const bool nonempty = lane < NRUNS && run_len > 0;
        const unsigned long long ne = __builtin_amdgcn_ballot_w64(nonempty);
        if (nonempty) {
            atomicOr(&bits[my_pre >> 5], 1u << (my_pre & 31));
            offc[__builtin_amdgcn_mbcnt_lo((unsigned)ne, 0)] = run_s - my_pre;     // lanes 0..26: low word only
        }
        wave_lds_sync();
        float4 tmp[CAP / 64];
        int ubase = -1;
#pragma unroll
        for (int b = 0; b < CAP / 64; ++b) {
            tmp[b] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (b * 64 < m) {
                const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)bits[2 * b]);
                const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)bits[2 * b + 1]);
                const unsigned long long B = ((unsigned long long)hi << 32) | lo;
                const unsigned long long S = B >> 1;               // starts <= lane  =  starts of (B >> 1) below lane, + bit 0
                const int c0 = ubase + (int)(lo & 1u);
                const int u = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(S >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)S, (unsigned)c0));
                ubase += (int)__popcll(B);
                const int j = b * 64 + lane;
                run_code[b >> 3] |= (unsigned)u << (4 * (b & 7));
                if (j < m) tmp[b] = a.pts[j + offc[u]];
            }
        }
        wave_lds_sync();                      // the bit string is dead: the list area goes back to the queries
#pragma unroll
        for (int b = 0; b < CAP / 64; ++b) {
            const int j = b * 64 + lane;
            if (j < m) {
                cand_x[j] = tmp[b].x; cand_y[j] = tmp[b].y; cand_z[j] = tmp[b].z;
            } else if (PRE && (b & ~1) * 64 < m) {
                // the pre-selection works on pairs of batches: unused slots sit at +inf and never pass a threshold
                cand_x[j] = INFINITY; cand_y[j] = 0.f; cand_z[j] = 0.f;
            }
        }
    }
    wave_lds_sync();
    const int k = a.k;
    const double eps2 = EPS ? a.eps2 : (double)INFINITY;
    // (lane l evaluates query l once per item)
    const KeySetup<KEY_BITS> keys = make_key_setup<KEY_BITS, EPS>(g, cx, cy, cz, my_q, a.ptsd != nullptr, my_qd.x, my_qd.y, my_qd.z, eps2);
    const double scale = keys.scale;
    const unsigned key_max = KeySetup<KEY_BITS>::key_max;
    const unsigned my_gkey = keys.my_gkey;
    // (without EPS these three are constants of the kernel, and spelled as such: the per-query code folds them away)
    const unsigned eps_key = EPS ? keys.eps_key : 0xFFFFFFFFu;

    constexpr int NB = CAP / 64;             // candidate registers per lane: slot = b * 64 + lane
    constexpr int LIST = 64 * R;             // capacity of the sorted list
    unsigned t_prev = 0;                     // threshold of the previous query of this item (0 = none yet)
    float t_prev_f = 0.f;                    // same for the float32 pre-selection
    const float cell2f = keys.cell2f, eps2a = EPS ? keys.eps2a : INFINITY;
    const double eps1 = EPS ? keys.eps1 : 0.0;

    if constexpr (PRE && PAIR) {
        unsigned short* pend_b = s_pend2[w];
        const auto push_redo = [&](int row, int why) { note_redo(row, why); };
        // smallest exact key a candidate cut by the float32 threshold T can have: its float32 d'^2 >= T means the
        // exact d'^2 >= T (1 - 2^-20) (arithmetic error of the packed evaluation); for a float64 query the exact
        // distance to the true query is at least d' - eq
        const auto cut_key = [&](float T, double eq) {
            double lo2 = (double)T * (1.0 - 0x1p-20);
            if constexpr (Q64) {
                // (sqrt(L) - eq)^2 >= L - 2 eq sqrt(L); an upper bound of the root is enough: float32 root, rounded up
                const double root_up = (double)__builtin_sqrtf(T) * (1.0 + 0x1p-21);
                lo2 = fmax(lo2 - 2.0 * eq * root_up, 0.0);
            }
            return (unsigned)fmin(lo2 * scale, 4294967294.0);
        };
        // The per-query body is compiled once per number of staged batch PAIRS in use (NBP: 128 slots each): the loops
        // over the batches are then straight code -- the "is this batch in use" tests were a scalar compare and a
        // branch per batch, per loop, per query, on a kernel whose scalar unit is as busy as its vector units.  The
        // smallest variant also serves the items with fewer pairs and keeps the tests (GUARD).
        const auto pair_loop = [&](auto NBP_, auto GUARD_) {
            constexpr int NBP = decltype(NBP_)::value, NBU = 2 * NBP;
            constexpr bool GUARD = decltype(GUARD_)::value;
            for (int qi = 0; qi < nq; qi += 2) {
                const bool live_b = qi + 1 < nq;             // an odd tail runs its last query twice, the copy is discarded
                const int qj = live_b ? qi + 1 : qi;
                const int row_a = row0 + qi, row_b = row0 + qj;
                float ax, ay, az, bx, by, bz;
                if constexpr (!Q64) {
                    ax = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_q.x), qi));
                    ay = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_q.y), qi));
                    az = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_q.z), qi));
                    bx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_q.x), qj));
                    by = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_q.y), qj));
                    bz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_q.z), qj));
                }
                // Float64 cloud (Q64): the candidates are the float32-rounded points (the reference's tree data, pct:74) and
                // my_q is the query ROUNDED to float32, so the pre-selection measures distances to a point that lies
                // eq = |q64 - q32| away from the true query: every bound taken from it moves by eq (triangle inequality).
                double qax, qay, qaz, qbx, qby, qbz, eq_a = 0.0, eq_b = 0.0;
                if constexpr (Q64) {
                    const auto rl = [&](double v, int l) {
                        return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
                    };
                    qax = rl(my_qd.x, qi); qay = rl(my_qd.y, qi); qaz = rl(my_qd.z, qi);
                    qbx = rl(my_qd.x, qj); qby = rl(my_qd.y, qj); qbz = rl(my_qd.z, qj);
                    ax = (float)qax; ay = (float)qay; az = (float)qaz;         // == the float32 record of the point (k_pack_f64)
                    bx = (float)qbx; by = (float)qby; bz = (float)qbz;
                    eq_a = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_eq), qi));
                    eq_b = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_eq), qj));
                } else {
                    qax = (double)ax; qay = (double)ay; qaz = (double)az; qbx = (double)bx; qby = (double)by; qbz = (double)bz;
                }
                // ---- float32 squared distances of ALL staged candidates to both queries (one set of LDS reads) --------
                float ap_a[NBU], ap_b[NBU];
#pragma unroll
                for (int p2 = 0; p2 < NBP; ++p2) {
                    ap_a[2 * p2] = ap_a[2 * p2 + 1] = INFINITY;
                    ap_b[2 * p2] = ap_b[2 * p2 + 1] = INFINITY;
                    if (!GUARD || p2 * 128 < m) {
                        const int sa = p2 * 128 + lane, sb = sa + 64;
                        const float2v vx = {cand_x[sa], cand_x[sb]}, vy = {cand_y[sa], cand_y[sb]}, vz = {cand_z[sa], cand_z[sb]};
                        {
                            const float2v dx = vx - ax, dy = vy - ay, dz = vz - az;
                            float2v d = dx * dx;
                            d = __builtin_elementwise_fma(dy, dy, d);
                            d = __builtin_elementwise_fma(dz, dz, d);
                            ap_a[2 * p2] = d.x;
                            ap_a[2 * p2 + 1] = d.y;
                        }
                        {
                            const float2v dx = vx - bx, dy = vy - by, dz = vz - bz;
                            float2v d = dx * dx;
                            d = __builtin_elementwise_fma(dy, dy, d);
                            d = __builtin_elementwise_fma(dz, dz, d);
                            ap_b[2 * p2] = d.x;
                            ap_b[2 * p2 + 1] = d.y;
                        }
                        n_step += 4;
                    }
                }
                // ---- thresholds: k+1 <= #(d < T) <= LIST for each query, never beyond the eps ball ----------------------
                float T_a = EPS ? eps2a : INFINITY, T_b = T_a;
                if constexpr (EPS && Q64) {          // exact d < eps  =>  d' < eps + eq
                    const double ea = eps1 + eq_a, eb = eps1 + eq_b;
                    T_a = (float)fmin(ea * ea * (1.0 + 0x1p-18), 3.0e38);
                    T_b = (float)fmin(eb * eb * (1.0 + 0x1p-18), 3.0e38);
                }
                int tot_a = m, tot_b = m;
                if constexpr (EPS) {
                    tot_a = tot_b = 0;
#pragma unroll
                    for (int b = 0; b < NBU; ++b)
                        if (!GUARD || (b & ~1) * 64 < m) {
                            tot_a += (int)__popcll(__builtin_amdgcn_ballot_w64(ap_a[b] < T_a));
                            tot_b += (int)__popcll(__builtin_amdgcn_ballot_w64(ap_b[b] < T_b));
                        }
                }
                int cnt_a = tot_a, cnt_b = tot_b;
                bool ok_a = true, ok_b = live_b;              // still on the fast path
                unsigned bkey_a = 0xFFFFFFFFu, bkey_b = 0xFFFFFFFFu;
                const bool need_a = tot_a > LIST, need_b = live_b && tot_b > LIST;
                if (need_a || need_b) {
                    const float target = 0.5f * (float)(k + 1 + LIST);
                    float t0 = t_prev_f > 0.f ? t_prev_f : cell2f;
                    if (!(t0 < T_a)) t0 = 0.5f * T_a;
                    float lo_a = 0.f, hi_a = T_a, t_a = t0, lo_b = 0.f, hi_b = T_b, t_b = t0;
                    bool go_a = need_a, go_b = need_b, found_a = !need_a, found_b = !need_b;
#pragma unroll 1
                    for (int trial = 0; trial < 16 && (go_a || go_b); ++trial) {
                        int c_a = 0, c_b = 0;
#pragma unroll
                        for (int b = 0; b < NBU; ++b)
                            if (!GUARD || (b & ~1) * 64 < m) {
                                c_a += (int)__popcll(__builtin_amdgcn_ballot_w64(ap_a[b] < t_a));
                                c_b += (int)__popcll(__builtin_amdgcn_ballot_w64(ap_b[b] < t_b));
                            }
                        if (go_a) {
                            if (c_a >= k + 1 && c_a <= LIST) { T_a = t_a; cnt_a = c_a; found_a = true; go_a = false; }
                            else {
                                if (c_a < k + 1) lo_a = t_a; else hi_a = t_a;
                                float nt = c_a > 0 ? t_a * target * __builtin_amdgcn_rcpf((float)c_a) : 4.f * t_a;
                                if (!(nt > lo_a && nt < hi_a)) nt = hi_a < INFINITY ? 0.5f * (lo_a + hi_a) : 2.f * lo_a;
                                nt = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(nt)));
                                if (!(nt > lo_a && nt < hi_a)) go_a = false; else t_a = nt;   // no float left between
                            }
                        }
                        if (go_b) {
                            if (c_b >= k + 1 && c_b <= LIST) { T_b = t_b; cnt_b = c_b; found_b = true; go_b = false; }
                            else {
                                if (c_b < k + 1) lo_b = t_b; else hi_b = t_b;
                                float nt = c_b > 0 ? t_b * target * __builtin_amdgcn_rcpf((float)c_b) : 4.f * t_b;
                                if (!(nt > lo_b && nt < hi_b)) nt = hi_b < INFINITY ? 0.5f * (lo_b + hi_b) : 2.f * lo_b;
                                nt = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(nt)));
                                if (!(nt > lo_b && nt < hi_b)) go_b = false; else t_b = nt;
                            }
                        }
                    }
                    if (need_a) {
                        ok_a = found_a && T_a >= 1e-30f;
                        if (ok_a) { t_prev_f = T_a; bkey_a = cut_key(T_a, eq_a); }
                    }
                    if (need_b) {
                        ok_b = ok_b && found_b && T_b >= 1e-30f;
                        if (ok_b) { t_prev_f = T_b; bkey_b = cut_key(T_b, eq_b); }
                    }
                    if (!ok_a) { push_redo(row_a, 3); T_a = 0.f; cnt_a = 0; }        // nothing passes, nothing is stored
                    if (!ok_b) { if (live_b) push_redo(row_b, 3); T_b = 0.f; cnt_b = 0; }
                    if (!ok_a && !ok_b) continue;
                }
                if (!live_b) { T_b = 0.f; cnt_b = 0; }
                // ---- compact the slots of the survivors of both queries, then exact keys for them only ------------------
                FastK<2 * R> both;                 // set 0 = query a (registers 0 .. R-1), set 1 = query b
                float out_d[2 * R];                // float32 distance / sorted position of survivor lane + 64 r of each set
                int out_p[2 * R];
                const auto slot_to_pos = [&](int j) {
                    unsigned code = (unsigned)__builtin_amdgcn_ds_bpermute((j & 63) << 2, (int)run_code[0]);
                    if constexpr ((CAP / 64 + 7) / 8 > 1) {
                        const unsigned hi = (unsigned)__builtin_amdgcn_ds_bpermute((j & 63) << 2, (int)run_code[1]);
                        code = (j >> 9) ? hi : code;
                    }
                    return j + offc[(code >> ((((unsigned)j >> 6) & 7u) << 2)) & 15u];
                };
                {
                    int base_a = 0, base_b = 0;
                    wave_lds_sync();
#pragma unroll
                    for (int b = 0; b < NBU; ++b) {
                        if (!GUARD || (b & ~1) * 64 < m) {
                            const bool pa = ap_a[b] < T_a, pb = ap_b[b] < T_b;
                            const unsigned long long ma = __builtin_amdgcn_ballot_w64(pa), mb = __builtin_amdgcn_ballot_w64(pb);
                            if (pa) pend[base_a + __builtin_amdgcn_mbcnt_hi((unsigned)(ma >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ma, 0))] = (unsigned)(b * 64 + lane);
                            if (pb) pend_b[base_b + __builtin_amdgcn_mbcnt_hi((unsigned)(mb >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mb, 0))] = (unsigned short)(b * 64 + lane);
                            base_a += (int)__popcll(ma);
                            base_b += (int)__popcll(mb);
                        }
                    }
                    wave_lds_sync();
                    // Survivor i's exact distance and sorted position are worked out here, by the lane that holds its
                    // coordinates anyway, and parked in that lane (out_d / out_p); after the sort the lane that ends up
                    // with list entry i fetches them with one cross-lane read each instead of recomputing them.
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int i = lane + 64 * r;
                        unsigned e_a = kPadElem, e_b = kPadElem;
                        const int ja = (int)pend[i] & (CAP_POW2 - 1), jb = (int)pend_b[i] & (CAP_POW2 - 1);   // stale beyond cnt: masked, unused
                        out_p[r] = slot_to_pos(ja);           // cross-lane reads inside: every lane active here
                        out_p[R + r] = slot_to_pos(jb);
                        out_d[r] = out_d[R + r] = INFINITY;
                        if (i < cnt_a) {
                            const double dx = (double)cand_x[ja] - qax, dy = (double)cand_y[ja] - qay, dz = (double)cand_z[ja] - qaz;
                            const double d2 = (dx * dx + dy * dy) + dz * dz;
                            out_d[r] = (float)sqrt(d2);
                            if (!EPS || d2 < eps2) e_a = (min((unsigned)(d2 * scale), key_max - 1u) << SLOT_BITS) | (unsigned)i;
                        }
                        if (i < cnt_b) {
                            const double dx = (double)cand_x[jb] - qbx, dy = (double)cand_y[jb] - qby, dz = (double)cand_z[jb] - qbz;
                            const double d2 = (dx * dx + dy * dy) + dz * dz;
                            out_d[R + r] = (float)sqrt(d2);
                            if (!EPS || d2 < eps2) e_b = (min((unsigned)(d2 * scale), key_max - 1u) << SLOT_BITS) | (unsigned)i;
                        }
                        both.e[r] = e_a;
                        both.e[R + r] = e_b;
                    }
                    wave_lds_sync();
                    fast_sort_sets<R, 2, 2>(both, sort_dir);
                    n_flush += 2;
                }
                // ---- proof obligations per query (see the single-query path below) -----------------------------------------
                bool amb_a = false, amb_b = false, sparse_a = false, sparse_b = false;
                bool col_a = false, col_b = false;        // equal keys among the first k+2 entries
                {
                    unsigned tau_a, tau_b;         // element k of each list = the (k+1)-th nearest (padding if fewer exist)
                    {
                        const int sl = k >> 6, src = k & 63;
                        unsigned va = both.e[0], vb = both.e[R];
#pragma unroll
                        for (int r = 1; r < R; ++r)
                            if (sl == r) { va = both.e[r]; vb = both.e[R + r]; }
                        tau_a = (unsigned)__builtin_amdgcn_readlane((int)va, src);
                        tau_b = (unsigned)__builtin_amdgcn_readlane((int)vb, src);
                    }
                    const unsigned g_a = (unsigned)__builtin_amdgcn_readlane((int)my_gkey, qi);
                    const unsigned g_b = (unsigned)__builtin_amdgcn_readlane((int)my_gkey, qj);
                    const unsigned tk_a = tau_a >> SLOT_BITS, tk_b = tau_b >> SLOT_BITS;
                    const unsigned need_ka = min(tau_a == kPadElem ? 0xFFFFFFFFu : tk_a + 1u, eps_key);
                    const unsigned need_kb = min(tau_b == kPadElem ? 0xFFFFFFFFu : tk_b + 1u, eps_key);
                    sparse_a = need_ka > g_a;
                    sparse_b = need_kb > g_b;
                    amb_a |= need_ka > min(g_a, bkey_a);
                    amb_b |= need_kb > min(g_b, bkey_b);
                    amb_a |= tau_a != kPadElem && tk_a >= key_max - 1u;
                    amb_b |= tau_b != kPadElem && tk_b >= key_max - 1u;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        unsigned up_a = __shfl_down(both.e[r], 1), up_b = __shfl_down(both.e[R + r], 1);     // element i+1
                        if (r + 1 < R) {
                            const unsigned na = (unsigned)__builtin_amdgcn_readlane((int)both.e[r + 1 < R ? r + 1 : r], 0);
                            const unsigned nb = (unsigned)__builtin_amdgcn_readlane((int)both.e[R + (r + 1 < R ? r + 1 : r)], 0);
                            if (lane == 63) { up_a = na; up_b = nb; }
                        } else if (lane == 63) {
                            up_a = kPadElem;
                            up_b = kPadElem;
                        }
                        const int i = lane + 64 * r;
                        col_a |= i <= k && both.e[r] != kPadElem && up_a != kPadElem && ((both.e[r] ^ up_a) >> SLOT_BITS) == 0u;
                        col_b |= i <= k && both.e[R + r] != kPadElem && up_b != kPadElem && ((both.e[R + r] ^ up_b) >> SLOT_BITS) == 0u;
                    }
                }
                if (ok_a && __ballot(amb_a) != 0ull) { push_redo(row_a, sparse_a ? 1 : 3); ok_a = false; }
                if (ok_b && __ballot(amb_b) != 0ull) { push_redo(row_b, sparse_b ? 1 : 3); ok_b = false; }
                // equal keys: ordered here by the exact values (order_equal_keys), not by the exact sweep
                const auto pos_of_set = [&](unsigned at, int set) {
                    int p = __builtin_amdgcn_ds_bpermute((int)(at & 63u) << 2, out_p[set * R]);
#pragma unroll
                    for (int r2 = 1; r2 < R; ++r2) {
                        const int p2 = __builtin_amdgcn_ds_bpermute((int)(at & 63u) << 2, out_p[set * R + r2]);
                        if ((int)(at >> 6) == r2) p = p2;
                    }
                    return p;
                };
                // (the query is fetched from its lane again: keeping the six coordinates of the pair alive across the sort
                // for this rare branch would cost the common path scalar registers it does not have)
                const auto query_of = [&](int ql, double& x, double& y, double& z) {
                    if constexpr (Q64) {
                        x = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(my_qd.x), ql), __builtin_amdgcn_readlane(__double2loint(my_qd.x), ql));
                        y = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(my_qd.y), ql), __builtin_amdgcn_readlane(__double2loint(my_qd.y), ql));
                        z = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(my_qd.z), ql), __builtin_amdgcn_readlane(__double2loint(my_qd.z), ql));
                    } else {
                        x = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_q.x), ql));
                        y = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_q.y), ql));
                        z = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_q.z), ql));
                    }
                };
                if (ok_a && __ballot(col_a) != 0ull) {
                    double ux, uy, uz;
                    query_of(qi, ux, uy, uz);
                    const bool done = order_equal_keys<R, SLOT_BITS>(&both.e[0], a.pts,
                        [&](unsigned at) {
                            const int j = (int)pend[at] & (CAP_POW2 - 1);
                            const double dx = (double)cand_x[j] - ux, dy = (double)cand_y[j] - uy, dz = (double)cand_z[j] - uz;
                            return (dx * dx + dy * dy) + dz * dz;
                        },
                        [&](unsigned at) { return pos_of_set(at, 0); });
                    if (!done) { push_redo(row_a, 3); ok_a = false; }
                }
                if (ok_b && __ballot(col_b) != 0ull) {
                    double ux, uy, uz;
                    query_of(qj, ux, uy, uz);
                    const bool done = order_equal_keys<R, SLOT_BITS>(&both.e[R], a.pts,
                        [&](unsigned at) {
                            const int j = (int)pend_b[at] & (CAP_POW2 - 1);
                            const double dx = (double)cand_x[j] - ux, dy = (double)cand_y[j] - uy, dz = (double)cand_z[j] - uz;
                            return (dx * dx + dy * dy) + dz * dz;
                        },
                        [&](unsigned at) { return pos_of_set(at, 1); });
                    if (!done) { push_redo(row_b, 3); ok_b = false; }
                }
                // ---- store: slot -> sorted position (cross-lane reads with every lane active), exact distance ----------------
#pragma unroll
                for (int set = 0; set < 2; ++set) {
                    const bool ok = set == 0 ? ok_a : ok_b;
                    const int row = set == 0 ? row_a : row_b;
                    int found = 0;
                    char* const prow = (char*)(a.nbr_pos + (int64_t)row * a.pitch);      // uniform: scalar base + lane offset
                    char* const drow = (char*)(a.nbr_dist + (int64_t)row * a.pitch);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int i = lane + 64 * r;
                        const unsigned e = both.e[set * R + r];
                        const bool real = e != kPadElem;
                        const unsigned at = e & ((1u << SLOT_BITS) - 1u);       // survivor index: lane at & 63, register at >> 6
                        float dist = __int_as_float(__builtin_amdgcn_ds_bpermute((int)(at & 63u) << 2, __float_as_int(out_d[set * R])));
                        int pos = __builtin_amdgcn_ds_bpermute((int)(at & 63u) << 2, out_p[set * R]);
#pragma unroll
                        for (int r2 = 1; r2 < R; ++r2) {
                            const float d2nd = __int_as_float(__builtin_amdgcn_ds_bpermute((int)(at & 63u) << 2, __float_as_int(out_d[set * R + r2])));
                            const int p2nd = __builtin_amdgcn_ds_bpermute((int)(at & 63u) << 2, out_p[set * R + r2]);
                            if ((int)(at >> 6) == r2) { dist = d2nd; pos = p2nd; }
                        }
                        if (ok && i >= 1 && i <= k) {
                            const unsigned off = (unsigned)(i - 1) * 4u;
                            *(int*)(prow + off) = real ? pos : -1;
                            *(float*)(drow + off) = real ? dist : INFINITY;
                            found += real;
                        }
                    }
                    if (ok) {
                        if (a.nbr_cnt) {
                            for (int o = 32; o > 0; o >>= 1) found += __shfl_xor(found, o);
                            if (lane == 0) a.nbr_cnt[row] = found;
                        }
                        if (a.row_done && lane == 0) a.row_done[row] = 1;
                    }
                }
            }
        };
        {
            using std::integral_constant;
            constexpr int PAIRS = NB / 2, LOW = PAIRS / 2;          // R = 1: 4 pairs, variants 2 | 3 | 4; R = 2: 6 pairs, 3 | 4 | 5 | 6
            const int nbp = (m + 127) >> 7;
#ifdef PCT_NO_NBP                                                   // tuning aid: one guarded body as before
            if (nbp >= 0) pair_loop(integral_constant<int, PAIRS>{}, integral_constant<bool, true>{});
            else
#endif
            if (nbp <= LOW) pair_loop(integral_constant<int, LOW>{}, integral_constant<bool, true>{});
            else if (nbp == LOW + 1) pair_loop(integral_constant<int, LOW + 1>{}, integral_constant<bool, false>{});
            else if (PAIRS > LOW + 2 && nbp == LOW + 2) pair_loop(integral_constant<int, (PAIRS > LOW + 2 ? LOW + 2 : PAIRS)>{}, integral_constant<bool, false>{});
            // (PAIRS > LOW + 3 -- the 1024-slot staging area of the tree items: the last variant also serves counts it is
            // not cut for, so it keeps the "is this batch in use" tests; unused batches are not initialised)
            else pair_loop(integral_constant<int, PAIRS>{}, integral_constant<bool, (PAIRS > LOW + 3)>{});
        }
    } else
    for (int qi = 0; qi < nq; ++qi) {
        const int row = row0 + qi;
        double qx, qy, qz;
        if (a.ptsd) {
            qx = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(my_qd.x), qi), __builtin_amdgcn_readlane(__double2loint(my_qd.x), qi));
            qy = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(my_qd.y), qi), __builtin_amdgcn_readlane(__double2loint(my_qd.y), qi));
            qz = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(my_qd.z), qi), __builtin_amdgcn_readlane(__double2loint(my_qd.z), qi));
        } else {
            qx = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_q.x), qi));
            qy = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_q.y), qi));
            qz = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_q.z), qi));
        }

        FastK<R> best;
        bool amb = false;                    // per-lane: something this kernel cannot prove exact
        bool col = false;                    // per-lane: equal keys among the first k+2 entries
        unsigned bkey = 0xFFFFFFFFu;         // exact keys of the candidates the pre-selection cut are >= bkey
        if constexpr (PRE) {
            const float fqx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_q.x), qi));
            const float fqy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_q.y), qi));
            const float fqz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_q.z), qi));
            // ---- float32 squared distances of ALL staged candidates, two batches per packed instruction ---------
            float appr[NB];
#pragma unroll
            for (int p2 = 0; p2 < NB / 2; ++p2) {
                appr[2 * p2] = INFINITY;
                appr[2 * p2 + 1] = INFINITY;
                if (p2 * 128 < m) {
                    const int sa = p2 * 128 + lane, sb = sa + 64;
                    const float2v vx = {cand_x[sa], cand_x[sb]}, vy = {cand_y[sa], cand_y[sb]}, vz = {cand_z[sa], cand_z[sb]};
                    const float2v dx = vx - fqx, dy = vy - fqy, dz = vz - fqz;
                    float2v d = dx * dx;
                    d = __builtin_elementwise_fma(dy, dy, d);
                    d = __builtin_elementwise_fma(dz, dz, d);
                    appr[2 * p2] = d.x;
                    appr[2 * p2 + 1] = d.y;
                    n_step += 2;
                }
            }
            // ---- threshold T with k+1 <= #(appr < T) <= LIST; never beyond the eps ball -----------------------------
            float T = EPS ? eps2a : INFINITY;
            int total = m;
            if constexpr (EPS) {
                total = 0;
#pragma unroll
                for (int b = 0; b < NB; ++b)
                    if ((b & ~1) * 64 < m) total += (int)__popcll(__builtin_amdgcn_ballot_w64(appr[b] < T));
            }
            int cnt = total;
            if (total > LIST) {
                float lo = 0.f, hi = T;                        // count(lo) < k+1 ; count(hi) > LIST
                float t = t_prev_f > 0.f ? t_prev_f : cell2f;  // first guess: one cell edge
                if (!(t < hi)) t = 0.5f * hi;
                const float target = 0.5f * (float)(k + 1 + LIST);
                bool found = false;
#pragma unroll 1
                for (int trial = 0; trial < 16; ++trial) {
                    int c = 0;
#pragma unroll
                    for (int b = 0; b < NB; ++b)
                        if ((b & ~1) * 64 < m) c += (int)__popcll(__builtin_amdgcn_ballot_w64(appr[b] < t));
                    if (c >= k + 1 && c <= LIST) { T = t; cnt = c; found = true; break; }
                    if (c < k + 1) lo = t; else hi = t;
                    float nt = c > 0 ? t * target * __builtin_amdgcn_rcpf((float)c) : 4.f * t;
                    if (!(nt > lo && nt < hi)) nt = hi < INFINITY ? 0.5f * (lo + hi) : 2.f * lo;
                    nt = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(nt)));   // uniform by construction
                    if (!(nt > lo && nt < hi)) break;          // no float left between: a pile of equal distances
                    t = nt;
                }
                if (!found || !(T >= 1e-30f)) {                // no usable threshold: the exact sweep takes the query
                    note_redo(row, 3);
                    continue;
                }
                t_prev_f = T;
                bkey = (unsigned)fmin((double)T * (1.0 - 0x1p-20) * scale, 4294967294.0);
            }
            // ---- compact the slots of the survivors, then exact keys for them only ---------------------------------
            {
                int base = 0;
                wave_lds_sync();
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    if ((b & ~1) * 64 < m) {
                        const bool pass = appr[b] < T;
                        const unsigned long long mask = __builtin_amdgcn_ballot_w64(pass);
                        if (pass) {
                            const int at = base + __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
                            pend[at] = (unsigned)(b * 64 + lane);                       // at < cnt <= LIST
                        }
                        base += (int)__popcll(mask);
                    }
                }
                wave_lds_sync();
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int i = lane + 64 * r;
                    unsigned e = kPadElem;
                    if (i < cnt) {
                        const int j = (int)pend[i];
                        const double dx = (double)cand_x[j] - qx, dy = (double)cand_y[j] - qy, dz = (double)cand_z[j] - qz;
                        const double d2 = (dx * dx + dy * dy) + dz * dz;
                        if (!EPS || d2 < eps2) e = (min((unsigned)(d2 * scale), key_max - 1u) << SLOT_BITS) | (unsigned)i;
                    }
                    best.e[r] = e;
                }
                wave_lds_sync();
                fast_sort_from<R, 2>(best, sort_dir);          // ascending
                ++n_flush;
            }
        } else {
            // ---- keys of ALL staged candidates, in registers (0xFFFFFFFF = not a candidate) ----------------------
            unsigned key[NB];
            int total = EPS ? 0 : m;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                key[b] = 0xFFFFFFFFu;
                if (b * 64 < m) {
                    const int slot = b * 64 + lane;
                    if (slot < m) {
                        const double dx = (double)cand_x[slot] - qx, dy = (double)cand_y[slot] - qy, dz = (double)cand_z[slot] - qz;
                        const double d2 = (dx * dx + dy * dy) + dz * dz;
                        if (!EPS || d2 < eps2) key[b] = min((unsigned)(d2 * scale), key_max - 1u);   // key_max itself: padding only
                    }
                    if constexpr (EPS) total += (int)__popcll(__builtin_amdgcn_ballot_w64(key[b] != 0xFFFFFFFFu));
                    ++n_step;
                }
            }

            // ---- threshold T with k+1 <= #(key < T) <= LIST: a few ballot-count trials.  Counts grow about linearly in
            // d^2 (= in the key) on a surface, so a secant step from the previous query's threshold usually lands at once.
            unsigned T = key_max + 1u;           // "everything"
            int cnt = total;
            if (total > LIST) {
                unsigned lo = 0u, hi = key_max + 1u;          // count(lo) < k+1 ; count(hi) > LIST
                unsigned t = t_prev ? t_prev : (unsigned)((double)(1u << KEY_BITS) / kKeyRange);   // first guess: one cell edge
                const float target = 0.5f * (float)(k + 1 + LIST);
                bool found = false;
#pragma unroll 1
                for (int trial = 0; trial < 16; ++trial) {
                    int c = 0;
#pragma unroll
                    for (int b = 0; b < NB; ++b)
                        if (b * 64 < m) c += (int)__popcll(__builtin_amdgcn_ballot_w64(key[b] < t));
                    if (c >= k + 1 && c <= LIST) { T = t; cnt = c; found = true; break; }
                    if (c < k + 1) lo = t; else hi = t;
                    if (hi - lo <= 1u) break;                  // a pile of equal keys straddles the window
                    const float guess = (float)t * target * __builtin_amdgcn_rcpf((float)(c > 0 ? c : 1));   // a guess: 1 ulp is plenty
                    unsigned nt = guess >= 4294967040.f ? hi : (unsigned)guess;
                    if (c == 0) nt = t * 4u > t ? t * 4u : hi;
                    if (nt <= lo || nt >= hi) nt = lo + (hi - lo) / 2u;
                    t = nt;
                }
                if (!found) {                                   // no usable threshold: the exact sweep takes the query
                    note_redo(row, 3);
                    continue;
                }
            }
            t_prev = T <= key_max ? T : t_prev;

            // ---- compact the selected candidates (all of them when there are <= LIST) and sort them ONCE ----------
            {
                int base = 0;
                wave_lds_sync();
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    if (b * 64 < m) {
                        const bool pass = key[b] < T;
                        const unsigned long long mask = __builtin_amdgcn_ballot_w64(pass);
                        if (pass) {
                            const int at = base + __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
                            pend[at] = (key[b] << SLOT_BITS) | (unsigned)(b * 64 + lane);      // at < cnt <= LIST
                        }
                        base += (int)__popcll(mask);
                    }
                }
                wave_lds_sync();
                const int have = cnt < LIST ? cnt : LIST;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int i = lane + 64 * r;
                    best.e[r] = i < have ? pend[i] : kPadElem;
                }
                wave_lds_sync();
                fast_sort_from<R, 2>(best, sort_dir);          // ascending
                ++n_flush;
            }
        }
        unsigned tau;                        // element k of the list = the (k+1)-th nearest (padding if fewer exist)
        {
            const int sl = k >> 6, src = k & 63;
            unsigned v = best.e[0];
#pragma unroll
            for (int r = 1; r < R; ++r)
                if (sl == r) v = best.e[r];
            tau = (unsigned)__builtin_amdgcn_readlane((int)v, src);
        }

        // ---- is every point closer than the (k+1)-th best inside the stencil?  (key rounded up; all in key units)
        bool sparse = false;
        {
            const unsigned gkey = (unsigned)__builtin_amdgcn_readlane((int)my_gkey, qi);
            const unsigned tkey = tau >> SLOT_BITS;
            const unsigned need = min(tau == kPadElem ? 0xFFFFFFFFu : tkey + 1u, eps_key);
            sparse = need > gkey;
            amb |= need > min(gkey, bkey);
            // a saturated key (a point clamped into a boundary cell from outside the grid box) says nothing
            // about the true distance
            amb |= tau != kPadElem && tkey >= key_max - 1u;
        }
        // ---- neighbours with equal keys inside the first k+2 entries: order not proven
        {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                unsigned up = __shfl_down(best.e[r], 1);                     // element i+1 for lanes 0..62
                if (r + 1 < R) {
                    const unsigned first_next = (unsigned)__builtin_amdgcn_readlane((int)best.e[r + 1 < R ? r + 1 : r], 0);
                    if (lane == 63) up = first_next;
                } else if (lane == 63) {
                    up = kPadElem;
                }
                const int i = lane + 64 * r;
                col |= i <= k && best.e[r] != kPadElem && up != kPadElem && ((best.e[r] ^ up) >> SLOT_BITS) == 0u;
            }
        }
        if (__ballot(amb) != 0ull) {
            note_redo(row, sparse ? 1 : 3);
            continue;
        }
        // sorted position of staged slot j = j + offset of its run (cross-lane reads: every lane active)
        const auto slot_pos = [&](int j) {
            unsigned code = (unsigned)__builtin_amdgcn_ds_bpermute((j & 63) << 2, (int)run_code[0]);
            if constexpr ((CAP / 64 + 7) / 8 > 1) {
                const unsigned hi = (unsigned)__builtin_amdgcn_ds_bpermute((j & 63) << 2, (int)run_code[1]);
                code = (j >> 9) ? hi : code;
            }
            return j + offc[(code >> ((((unsigned)j >> 6) & 7u) << 2)) & 15u];
        };
        if (__ballot(col) != 0ull) {      // equal keys: ordered here by the exact values, not by the exact sweep
            const auto slot_of = [&](unsigned at) {
                int j = (int)at;
                if constexpr (PRE) j = (int)pend[j] & (CAP_POW2 - 1);
                return j;
            };
            const bool done = order_equal_keys<R, SLOT_BITS>(&best.e[0], a.pts,
                [&](unsigned at) {
                    const int j = slot_of(at);
                    const double dx = (double)cand_x[j] - qx, dy = (double)cand_y[j] - qy, dz = (double)cand_z[j] - qz;
                    return (dx * dx + dy * dy) + dz * dz;
                },
                [&](unsigned at) { return slot_pos(slot_of(at) & (CAP_POW2 - 1)); });
            if (!done) {
                note_redo(row, 3);
                continue;
            }
        }

        // ---- store: exact fp64 distance re-derived from the coordinates -------
        int found = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = lane + 64 * r;
            const unsigned e = best.e[r];
            const bool real = e != kPadElem;
            int j = (int)(e & ((1u << SLOT_BITS) - 1u));             // staged slot (anything for padding)
            if constexpr (PRE) j = (int)pend[j] & (CAP_POW2 - 1);        // ... via the survivors' list (still intact)
            // sorted position of slot j = j + offset of its run.  The cross-lane reads need every lane active:
            // they stay outside the divergent part.
            unsigned code = (unsigned)__builtin_amdgcn_ds_bpermute((j & 63) << 2, (int)run_code[0]);
            if constexpr ((CAP / 64 + 7) / 8 > 1) {
                const unsigned hi = (unsigned)__builtin_amdgcn_ds_bpermute((j & 63) << 2, (int)run_code[1]);
                code = (j >> 9) ? hi : code;
            }
            const unsigned t = (code >> ((((unsigned)j >> 6) & 7u) << 2)) & 15u;       // index of the slot's run
            const int pos_real = j + offc[t];
            if (i >= 1 && i <= k) {
                int pos = -1;
                float dist = INFINITY;
                if (real) {
                    const double dx = (double)cand_x[j] - qx, dy = (double)cand_y[j] - qy, dz = (double)cand_z[j] - qz;
                    dist = (float)sqrt((dx * dx + dy * dy) + dz * dz);
                    pos = pos_real;
                }
                a.nbr_pos[(int64_t)row * a.pitch + (i - 1)] = pos;
                a.nbr_dist[(int64_t)row * a.pitch + (i - 1)] = dist;
                found += real;
            }
        }
        if (a.nbr_cnt) {
            for (int o = 32; o > 0; o >>= 1) found += __shfl_xor(found, o);
            if (lane == 0) a.nbr_cnt[row] = found;
        }
        if (a.row_done && lane == 0) a.row_done[row] = 1;
    }
    if (redo_mask) {
        const int cnt = (int)__popcll(redo_mask);
        if (a.row_done) {
            if ((redo_mask >> lane) & 1ull) {
                const int why = (int)((redo_why_lo >> lane) & 1ull) | ((int)((redo_why_hi >> lane) & 1ull) << 1);
                a.redo_m[row0 + lane] = (why << 29) | min(m, (1 << 29) - 1);
            }
        } else {
            int base = 0;
            if (lane == 0) base = atomicAdd(redo_count, cnt);
            base = __builtin_amdgcn_readfirstlane(base);
            if ((redo_mask >> lane) & 1ull) redo[base + (int)__popcll(redo_mask & ((1ull << lane) - 1ull))] = row0 + lane;
        }
        n_redo += (unsigned long long)cnt;
    }
    // statistics are opt-in: ~10^5 waves adding to the same words serialise at the memory side
    if (a.stats && lane == 0) {
        atomicAdd(&a.counters->flushes, n_flush);
        atomicAdd(&a.counters->candidate_steps, n_step);
        if (n_redo) atomicAdd(&a.counters->redone_queries, n_redo);
    }
}

// The one launch site of each family (PCT_LAUNCH_T: the abort trace names the instantiation by its argument values).
template <int R, bool EPS, bool PRE, bool PAIR, bool Q64, bool TREE>
void launch_fast(pct_ctx* ctx, const KnnArgs& a, int* redo, int* redo_count) {
    const dim3 grid((unsigned)((ctx->n_items + kFastWaves<R> - 1) / kFastWaves<R>)), block(64 * kFastWaves<R>);
    PCT_LAUNCH_T((k_knn_fast<R, EPS, PRE, PAIR, Q64, TREE>), grid, block, 0, ctx->stream, a, (const int2*)ctx->occ.p, ctx->n_items,
                 ctx->items_q, redo, redo_count);
}

}  // namespace

void pct_launch_sweep_fast(pct_ctx* ctx, const SweepPlan& p, const KnnArgs& a, int* redo, int* redo_count) {
    with_bools([&](auto r2, auto e) {
        with_index<kFastForms>(p.form, [&](auto form) {
            constexpr FastFlags f = kFastFlags[form];
            launch_fast<(r2 ? 2 : 1), e, f.pre, f.pair, f.q64, f.tree>(ctx, a, redo, redo_count);
        });
    }, p.R == 2, p.eps);
}

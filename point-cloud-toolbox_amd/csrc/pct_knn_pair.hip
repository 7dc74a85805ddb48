// k_knn_pair: the fast sweep of the headline case (one list register, a plain sweep), with its launcher and entry.
#include "pct_knn_item.h"

namespace {

// ---------------------------------------------------------------------------
// k_knn_pair: the fast sweep for the case the headline workload is -- one list register (k + 1 <= 64), a float32 cloud,
// the uniform cell list, a plain sweep (no level pass) -- written for the SCALAR unit as much as for the vector units.
// Same algorithm, same proofs and bit-identical rows as k_knn_fast<1, EPS, true, true>; what differs:
//   * the kernel argument holds only what this kernel reads, the work item's cell coordinates come from two
//     multiplications (host-side magic numbers) instead of three integer divisions, per-item bases replace the
//     per-query 64-bit row arithmetic, and the opt-in statistics do not live in the loop: no scalar register spills
//     (k_knn_fast: 31 at the 106-register cap);
//   * the threshold search of the two queries of a pair runs in lanes 0 and 1 of the same vector instructions
//     (one secant step serves both) and leaves the loop with one ballot;
//   * the compaction of the survivors has no divergent region: a lane without a survivor writes to a spare slot
//     (k_knn_fast: s_and_saveexec / s_or exec and a branch per batch and query);
//   * exact keys, distances and positions of both queries are worked out for all 64 lanes in one basic block (the two
//     fp64 chains interleave; lanes beyond the survivor count are set to padding afterwards);
//   * the two sorting networks are ONE hand-scheduled assembly block (pct_sort_pair.inc, tools/gen_sort_asm.py): the
//     sets alternate instruction by instruction, so the wait states of every DPP read are the other set's work
//     (10 s_nop per pair instead of 40, 82 VALU instead of 99, both ds_bpermute of a flip in flight together);
//   * DIST = false (the fused curvature call, whose fit never reads distances) leaves out the correctly rounded
//     float32(sqrt(fp64)) and the second table: pct_get_neighbors derives the same bits from the positions on demand.
// Staged batches are used in pairs (128 slots); the body is compiled per number of pairs in use, without guards
// (1 | 2 | 3 | 4): slots of a staged pair beyond the stencil's population sit at +inf.
// ---------------------------------------------------------------------------
constexpr int kPairCap = kStageCap;
static_assert((kPairCap & (kPairCap - 1)) == 0 && kPairCap % 128 == 0 && kPairCap <= 512, "staging capacity of k_knn_pair");
static_assert(PCT_TREE_CAP % 128 == 0 && PCT_TREE_CAP <= 1024, "staging capacity of k_knn_pair on the hierarchical cell list");
template <int CAP>
struct PairLdsT {
    float cx[CAP], cy[CAP], cz[CAP];                     // staged stencil, 12 B per candidate
    unsigned pend[64 + 4];                               // staged slots of the survivors of query a; [64]: the spare slot
    unsigned short pend_b[64 + 8];                       // ... of query b
    int offc[16];                                        // sorted position - flat slot, per non-empty run
};
using PairLds = PairLdsT<kPairCap>;

#ifndef PCT_PAIR_WAVES
#define PCT_PAIR_WAVES 1
#endif
// waves (= work items) per block; they share nothing but the launch.  One: a finished wave's slot and LDS go to the
// next block at once (items differ in queries and in staged batches: with four waves per block the fastest three
// waited for the slowest, 4.6 of 6 wave slots per SIMD filled; 0.392 -> 0.379 ms)
constexpr int kPairWaves = PCT_PAIR_WAVES;

// Q64: a float64 cloud -- the candidates are the float32-rounded points (the reference's tree data, pct:74), a query is the
// native float64 point (pct:83): the float32 pre-selection measures from the query ROUNDED to float32, a point
// eq = |q64 - q32| away from the true one, and every bound taken from it moves by eq (see k_knn_fast); exact keys and
// distances use the float64 query.
// TREE: the work items of the hierarchical cell list (round 3; k_knn_fast<1, .., TREE> until then) -- an item is a run of
// queries of one octree segment, its stencil the 27 ranges of the Morton-ordered cloud the build recorded, its grid the
// segment's level; 768 staged slots (what the build refines segments for), slot ids of 10 + 4 bits.
template <bool EPS, bool DIST, bool Q64 = false, bool TREE = false>
__global__ __launch_bounds__(64 * kPairWaves, (TREE ? 4 : Q64 ? 5 : 6)) void k_knn_pair(PairArgs a) {
    constexpr int CAP = TREE ? PCT_TREE_CAP : kPairCap, LIST = 64, SLOT_BITS = 6, KEY_BITS = 32 - SLOT_BITS;
    constexpr int SB = TREE ? 10 : 9;                    // bits of a staged slot inside a slot id (the run index sits above)
    constexpr unsigned kIdMask = (1u << (SB + 4)) - 1u;
    __shared__ PairLdsT<CAP> s_lds[kPairWaves];
    const int w = kPairWaves == 1 ? 0 : __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const int blk = (int)blockIdx.x * kPairWaves + w;
    const int item = a.items_per_xcd ? (blk & 7) * a.items_per_xcd + (blk >> 3) : blk;
    if (item >= a.n_items || (a.items_per_xcd && (blk >> 3) >= a.items_per_xcd)) return;
    PairLdsT<CAP>& L = s_lds[w];
    const SortLanes sort_dir = make_sort_lanes();
    // ---- the work item, its stencil runs and its queries (pct_knn_item.h) ----------------------------------------------
    constexpr int NRUNS = TREE ? 27 : 9;                          // ranges of the cloud the stencil is staged from
    const int2 it2 = a.items[item];
    if (item_of_split_segment<TREE>(it2)) return;
    ItemHead<TREE> head;
    load_item_head<TREE>(a, it2, lane, head);
    const int cx = head.cx, cy = head.cy, cz = head.cz, qs = head.qs, nq = head.nq, row0 = head.row0;
    const int run_s = head.run_s, run_len = head.run_len;
    const pct_grid& G = TREE ? head.g_lvl : a.g;
    float4 my_q;
    double my_qx, my_qy, my_qz;
    float my_eq;
    load_queries<Q64>(a.pts, a.ptsd, qs, nq, lane, my_q, my_qx, my_qy, my_qz, my_eq);
    int my_pre, m;
    run_prefix<NRUNS>(run_len, lane, my_pre, m);
    pct_stamp(a.stamp);            // (behind the prologue's loads; block 0 takes neither return above on a uniform list: pct_stamp.h)
    unsigned long long redo_mask = 0ull;                  // queries of this item the exact sweep has to take
    // Per query (lane l = query l, as my_gkey): 1 = the query's list is the proven set of its 27 cells and only the cube
    // cannot vouch for it -- its redo entry carries kRedoTrusted and the exact sweep starts from the list (Sweep::adopt);
    // 2 = never, whatever the proofs say.  Written in the redo branches only.
    unsigned my_trust = 0u;
    if (item_overflows<TREE, NRUNS>(m, CAP, run_len, lane)) {
        if (TREE || !a.seed) {
            hand_item_to_redo(a.redo, a.redo_count, a.counters, a.stats, row0, nq, lane, true, a.nbr_pos, a.pitch);
            return;
        }
        // The item runs on the first CAP flat slots of its stencil: every list it stores is k real candidates, which is
        // all the exact sweep asks of a redo row (Sweep::seed) -- the proofs below assume the whole stencil, so every
        // query of the item is on the redo list from here on, whatever they say.
        redo_mask = nq >= 64 ? ~0ull : (1ull << nq) - 1ull;
        my_trust = 2u;                                    // (a list of a truncated stencil is the set of nothing)
        if (a.stats && lane == 0) atomicAdd(&a.counters->lds_overflows, 1ull);
        m = CAP;
    }

    // ---- copy the runs as one flat range (see k_knn_fast): run starts as a bit string in the list area; the run index
    // u of this lane's slot of batch b rides in the slot id itself (slotx[b] = slot | u << 9: what the compaction
    // writes into the survivors' lists), offc[u] = sorted position - flat slot of run u
    unsigned slotx[CAP / 64];
    {
        unsigned* bits = L.pend;
        if (lane < CAP / 32) bits[lane] = 0u;
        wave_lds_sync();
        const bool nonempty = lane < NRUNS && run_len > 0 && my_pre < CAP;      // (a truncated item: the runs that begin inside)
        const unsigned long long ne = __builtin_amdgcn_ballot_w64(nonempty);
        if (nonempty) {
            atomicOr(&bits[my_pre >> 5], 1u << (my_pre & 31));
            L.offc[__builtin_amdgcn_mbcnt_lo((unsigned)ne, 0)] = run_s - my_pre;
        }
        wave_lds_sync();
        float4 tmp[CAP / 64];
        int ubase = -1;
#pragma unroll
        for (int b = 0; b < CAP / 64; ++b) {
            tmp[b] = make_float4(0.f, 0.f, 0.f, 0.f);
            slotx[b] = (unsigned)(b * 64 + lane);
            if (b * 64 < m) {
                const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)bits[2 * b]);
                const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)bits[2 * b + 1]);
                const unsigned long long B = ((unsigned long long)hi << 32) | lo;
                const unsigned long long S = B >> 1;               // starts <= lane  =  starts of (B >> 1) below lane, + bit 0
                const int s0 = ubase + (int)(lo & 1u);
                const int u = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(S >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)S, (unsigned)s0));
                ubase += (int)__popcll(B);
                const int j = b * 64 + lane;
                slotx[b] |= (unsigned)u << SB;
                if (j < m) tmp[b] = a.pts[j + L.offc[u]];
            }
        }
        wave_lds_sync();                      // the bit string is dead: the list area goes back to the queries
#pragma unroll
        for (int b = 0; b < CAP / 64; ++b) {
            const int j = b * 64 + lane;
            if (j < m) {
                L.cx[j] = tmp[b].x; L.cy[j] = tmp[b].y; L.cz[j] = tmp[b].z;
            } else if ((b & ~1) * 64 < m) {
                L.cx[j] = INFINITY; L.cy[j] = 0.f; L.cz[j] = 0.f;     // unused slot of a staged pair: passes no threshold
            }
        }
    }
    wave_lds_sync();

    const int k = a.k;
    const double eps2 = EPS ? a.eps2 : (double)INFINITY;
    const KeySetup<KEY_BITS> keys = make_key_setup<KEY_BITS, EPS>(G, cx, cy, cz, my_q, Q64, my_qx, my_qy, my_qz, eps2);
    const double scale = keys.scale;
    constexpr unsigned key_max = KeySetup<KEY_BITS>::key_max;
    const unsigned my_gkey = keys.my_gkey;
    const float cell2f = keys.cell2f;
    // (without EPS these are constants of the kernel, and spelled as such: the per-query code folds them away)
    const unsigned eps_key = EPS ? keys.eps_key : 0xFFFFFFFFu;
    const float eps2a = EPS ? keys.eps2a : INFINITY;
    const double eps1 = EPS ? keys.eps1 : 0.0;
    float t_prev_f = 0.f;                                 // threshold of the previous query of this item (0 = none yet)

    // table rows of this item: one 64-bit base per item, 32-bit offsets per query and lane (list entry i -> column i - 1)
    char* const pos_item = (char*)(a.nbr_pos + (int64_t)row0 * a.pitch);
    char* const dist_item = DIST ? (char*)(a.nbr_dist + (int64_t)row0 * a.pitch) : nullptr;
    const unsigned lane_off = (unsigned)(lane - 1) * 4u;
    const unsigned pitch4 = (unsigned)a.pitch * 4u;
    const bool col_lane = lane >= 1 && lane <= k;         // lanes whose list entry is a table column
    const unsigned long long first_k1 = (2ull << k) - 1ull;          // lanes 0 .. k: the entries whose order matters

    static_assert(CAP <= (1 << SB) && SB + 4 <= 16, "slot ids: SB bits of slot, 4 bits of run index, 16-bit survivor list of query b");
    const auto slot_of = [](unsigned id) { return TREE ? min((int)(id & ((1u << SB) - 1u)), CAP - 1) : (int)(id & (unsigned)(CAP - 1)); };

    const auto pair_loop = [&](auto NBP_) {
        constexpr int NBP = decltype(NBP_)::value, NBU = 2 * NBP;
        for (int qi = 0; qi < nq; qi += 2) {
            const bool live_b = qi + 1 < nq;             // an odd tail runs its last query twice, the copy is discarded
            const int qj = live_b ? qi + 1 : qi;
            const float ax = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_q.x), qi));
            const float ay = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_q.y), qi));
            const float az = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_q.z), qi));
            const float bx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_q.x), qj));
            const float by = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_q.y), qj));
            const float bz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_q.z), qj));
            // the queries the exact keys measure from: the float32 record widened, or (Q64) the native coordinates
            const auto rl64 = [&](double v, int l) {
                return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
            };
            const double qax = Q64 ? rl64(my_qx, qi) : (double)ax, qay = Q64 ? rl64(my_qy, qi) : (double)ay, qaz = Q64 ? rl64(my_qz, qi) : (double)az;
            const double qbx = Q64 ? rl64(my_qx, qj) : (double)bx, qby = Q64 ? rl64(my_qy, qj) : (double)by, qbz = Q64 ? rl64(my_qz, qj) : (double)bz;
            // ---- float32 squared distances of ALL staged candidates to both queries (one set of LDS reads) --------
            float ap_a[NBU], ap_b[NBU];
#pragma unroll
            for (int p2 = 0; p2 < NBP; ++p2) {
                const int sa = p2 * 128 + lane, sb = sa + 64;
                const float2v vx = {L.cx[sa], L.cx[sb]}, vy = {L.cy[sa], L.cy[sb]}, vz = {L.cz[sa], L.cz[sb]};
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
            }
            // ---- thresholds: k+1 <= #(d < T) <= LIST for each query, never beyond the eps ball.  Lane 0 searches for
            // query a, lane 1 for query b: the counts are wave-wide ballots, the secant arithmetic is per lane.
            // +inf without eps; Q64: exact d < eps  =>  d' < eps + eq, per query (lane 0: a, lanes >= 1: b)
            float T_init = eps2a;
            float Ti_a = eps2a, Ti_b = eps2a;
            const float eq_a = Q64 ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_eq), qi)) : 0.f;
            const float eq_b = Q64 ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_eq), qj)) : 0.f;
            const float v_eq = lane == 0 ? eq_a : eq_b;
            if constexpr (EPS && Q64) {
                const double ee = eps1 + (double)v_eq;
                T_init = (float)fmin(ee * ee * (1.0 + 0x1p-18), 3.0e38);
                Ti_a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(T_init), 0));
                Ti_b = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(T_init), 1));
            }
            int tot_a = m, tot_b = m;
            if constexpr (EPS) {
                tot_a = tot_b = 0;
#pragma unroll
                for (int b = 0; b < NBU; ++b) {
                    tot_a += (int)__popcll(__builtin_amdgcn_ballot_w64(ap_a[b] < Ti_a));
                    tot_b += (int)__popcll(__builtin_amdgcn_ballot_w64(ap_b[b] < Ti_b));
                }
            }
            const bool need_a = tot_a > LIST, need_b = live_b && tot_b > LIST;
            float T_a = Ti_a, T_b = Ti_b;
            int cnt_a = tot_a, cnt_b = tot_b;
            bool ok_a = true, ok_b = live_b;
            unsigned bkey_a = 0xFFFFFFFFu, bkey_b = 0xFFFFFFFFu;     // exact keys of the candidates the pre-selection cut are >= bkey
#ifdef PCT_ABL_NO_TRIAL
            T_a = T_b = 0.33f * cell2f; cnt_a = cnt_b = 57;
            if (false)
#endif
            if (need_a || need_b) {
                const float target = 0.5f * (float)(k + 1 + LIST);
                float t0 = t_prev_f > 0.f ? t_prev_f : cell2f;
                if (!(t0 < T_init)) t0 = 0.5f * T_init;
                const bool mine = lane == 0 ? need_a : need_b;         // (lanes >= 2 mirror lane 1; nobody reads them)
                float v_t = t0, v_lo = 0.f, v_hi = T_init, v_T = T_init;
                int v_cnt = lane == 0 ? tot_a : tot_b;
                bool go = mine, found = !mine;
#pragma unroll 1
                for (int trial = 0; trial < 16; ++trial) {
                    const float ta = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v_t), 0));
                    const float tb = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v_t), 1));
                    int c_a = 0, c_b = 0;
#pragma unroll
                    for (int b = 0; b < NBU; ++b) {
                        c_a += (int)__popcll(__builtin_amdgcn_ballot_w64(ap_a[b] < ta));
                        c_b += (int)__popcll(__builtin_amdgcn_ballot_w64(ap_b[b] < tb));
                    }
                    const int c = lane == 0 ? c_a : c_b;
                    const bool in = go && (unsigned)(c - (k + 1)) <= (unsigned)(LIST - (k + 1));
                    v_T = in ? v_t : v_T;
                    v_cnt = in ? c : v_cnt;
                    found = found || in;
                    go = go && !in;
                    if ((__builtin_amdgcn_ballot_w64(go) & 3ull) == 0ull) break;      // both thresholds found: no secant step
                    // secant step for the lanes still searching (count ~ linear in d^2 on a surface); c = 0 gives +inf,
                    // which the interval test below turns into a doubling / a bisection
                    const bool below = c < k + 1;
                    v_lo = go && below ? v_t : v_lo;
                    v_hi = go && !below ? v_t : v_hi;
                    float nt = v_t * target * __builtin_amdgcn_rcpf((float)c);
                    if (!(nt > v_lo && nt < v_hi)) nt = v_hi < INFINITY ? 0.5f * (v_lo + v_hi) : 2.f * v_lo;
                    go = go && nt > v_lo && nt < v_hi;         // no float left between: a pile of equal distances
                    v_t = go ? nt : v_t;
                    if ((__builtin_amdgcn_ballot_w64(go) & 3ull) == 0ull) break;
                }
                const unsigned fm = (unsigned)__builtin_amdgcn_ballot_w64(found);
                T_a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v_T), 0));
                T_b = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v_T), 1));
                cnt_a = __builtin_amdgcn_readlane(v_cnt, 0);
                cnt_b = __builtin_amdgcn_readlane(v_cnt, 1);
                // smallest exact key a candidate cut by the float32 threshold T can have: its float32 d^2 >= T means the
                // exact d^2 >= T (1 - 2^-20) (arithmetic error of the packed evaluation)
                double lo2 = (double)v_T * (1.0 - 0x1p-20);
                if constexpr (Q64) {
                    // (sqrt(L) - eq)^2 >= L - 2 eq sqrt(L); an upper bound of the root is enough: float32 root, rounded up
                    const double root_up = (double)__builtin_sqrtf(v_T) * (1.0 + 0x1p-21);
                    lo2 = fmax(lo2 - 2.0 * (double)v_eq * root_up, 0.0);
                }
                const unsigned v_bkey = (unsigned)fmin(lo2 * scale, 4294967294.0);
                ok_a = (fm & 1u) != 0u && (!need_a || T_a >= 1e-30f);
                ok_b = live_b && (fm & 2u) != 0u && (!need_b || T_b >= 1e-30f);
                if (need_a && ok_a) { t_prev_f = T_a; bkey_a = (unsigned)__builtin_amdgcn_readlane((int)v_bkey, 0); }
                if (need_b && ok_b) { t_prev_f = T_b; bkey_b = (unsigned)__builtin_amdgcn_readlane((int)v_bkey, 1); }
                // no threshold: nothing passes, the list is all padding and the row stored below starts with -1 -- the mark
                // of a redo row without candidates (Sweep::seed)
                if (!ok_a) { redo_mask |= 1ull << qi; T_a = 0.f; cnt_a = 0; }
                if (!ok_b) { if (live_b) redo_mask |= 1ull << qj; T_b = 0.f; cnt_b = 0; }
            }
            if (!live_b) { T_b = 0.f; cnt_b = 0; }
            // ---- compact the slots of the survivors of both queries.  Per batch and query: one compare (the pass mask
            // goes to a scalar pair), two v_mbcnt for the rank among the survivors, one v_lshl_add for the LDS address --
            // four vector instructions -- and the write under exec = mask; the running list address and exec are
            // scalar work (the scalar unit has the room: the kernel is bound by vector issue, 4 cycles per instruction).
            // Hand-placed: on gfx940-class parts a VALU read of an SGPR needs two wait states after the VALU write of
            // it; the two queries' instructions fill each other's.
            {
                unsigned wr_a = (unsigned)(uintptr_t)&L.pend[0], wr_b = (unsigned)(uintptr_t)&L.pend_b[0];
                const unsigned long long all = __builtin_amdgcn_read_exec();
                wave_lds_sync();
#ifndef PCT_ABL_NO_COMPACT
#pragma unroll
                for (int b = 0; b < NBU; ++b) {
                    unsigned ra, rb, ca, cb;
                    const unsigned slot = slotx[b];
                    asm volatile(
                        "v_cmp_gt_f32 vcc, %[ta], %[apa]\n"
                        "v_cmp_gt_f32 s[96:97], %[tb], %[apb]\n"
                        "s_bcnt1_i32_b64 %[ca], vcc\n"
                        "v_mbcnt_lo_u32_b32 %[ra], vcc_lo, 0\n"
                        "s_bcnt1_i32_b64 %[cb], s[96:97]\n"
                        "v_mbcnt_lo_u32_b32 %[rb], s96, 0\n"
                        "v_mbcnt_hi_u32_b32 %[ra], vcc_hi, %[ra]\n"
                        "v_mbcnt_hi_u32_b32 %[rb], s97, %[rb]\n"
                        "v_lshl_add_u32 %[ra], %[ra], 2, %[wra]\n"
                        "v_lshl_add_u32 %[rb], %[rb], 1, %[wrb]\n"
                        "s_mov_b64 exec, vcc\n"
                        "ds_write_b32 %[ra], %[slot]\n"
                        "s_mov_b64 exec, s[96:97]\n"
                        "ds_write_b16 %[rb], %[slot]\n"
                        "s_mov_b64 exec, %[all]\n"
                        "s_lshl2_add_u32 %[wra], %[ca], %[wra]\n"
                        "s_lshl1_add_u32 %[wrb], %[cb], %[wrb]\n"
                        : [ra] "=&v"(ra), [rb] "=&v"(rb), [ca] "=&s"(ca), [cb] "=&s"(cb), [wra] "+s"(wr_a), [wrb] "+s"(wr_b)
                        : [ta] "v"(T_a), [tb] "v"(T_b), [apa] "v"(ap_a[b]), [apb] "v"(ap_b[b]), [slot] "v"(slot), [all] "s"(all)
                        : "vcc", "scc", "s96", "s97", "memory");
                }
#endif
                wave_lds_sync();
            }
            // ---- exact keys for the survivors only.  Survivor `lane` of each query: staged slot -> coordinates -> fp64
            // ((dx^2 + dy^2) + dz^2) (no FMA: SciPy's value) -> key, distance, sorted position; worked out by every lane
            // (a stale list entry is masked into the staging area and gives a garbage value nobody uses).
            const unsigned sxa = L.pend[lane] & kIdMask, sxb = (unsigned)L.pend_b[lane] & kIdMask;      // slot | run << SB
            const int ja = slot_of(sxa), jb = slot_of(sxb);
            const int out_pa = ja + L.offc[sxa >> SB], out_pb = jb + L.offc[sxb >> SB];                 // sorted positions
            float out_da = 0.f, out_db = 0.f;
            unsigned e_a, e_b;
#ifdef PCT_ABL_NO_KEYS
            e_a = ((unsigned)ja << 6) | (unsigned)lane; e_b = ((unsigned)jb << 6) | (unsigned)lane;
            if (false)
#endif
            {
                const double dxa = (double)L.cx[ja] - qax, dya = (double)L.cy[ja] - qay, dza = (double)L.cz[ja] - qaz;
                const double dxb = (double)L.cx[jb] - qbx, dyb = (double)L.cy[jb] - qby, dzb = (double)L.cz[jb] - qbz;
                const double d2a = (dxa * dxa + dya * dya) + dza * dza;
                const double d2b = (dxb * dxb + dyb * dyb) + dzb * dzb;
                if constexpr (DIST) {
                    out_da = (float)sqrt(d2a);
                    out_db = (float)sqrt(d2b);
                }
                const unsigned ka = (min((unsigned)(d2a * scale), key_max - 1u) << SLOT_BITS) | (unsigned)lane;
                const unsigned kb = (min((unsigned)(d2b * scale), key_max - 1u) << SLOT_BITS) | (unsigned)lane;
                e_a = lane < cnt_a && (!EPS || d2a < eps2) ? ka : kPadElem;
                e_b = lane < cnt_b && (!EPS || d2b < eps2) ? kb : kPadElem;
            }
            wave_lds_sync();
#ifndef PCT_ABL_NO_SORT
            sort_pair_asm(e_a, e_b, sort_dir);
#endif
            // ---- proof obligations per query (all in key units, see k_knn_fast) ------------------------------------
            const unsigned tau_a = (unsigned)__builtin_amdgcn_readlane((int)e_a, k);      // the (k+1)-th nearest (padding if fewer exist)
            const unsigned tau_b = (unsigned)__builtin_amdgcn_readlane((int)e_b, k);
            const unsigned g_a = (unsigned)__builtin_amdgcn_readlane((int)my_gkey, qi);
            const unsigned g_b = (unsigned)__builtin_amdgcn_readlane((int)my_gkey, qj);
            const unsigned tk_a = tau_a >> SLOT_BITS, tk_b = tau_b >> SLOT_BITS;
            const unsigned need_ka = min(tau_a == kPadElem ? 0xFFFFFFFFu : tk_a + 1u, eps_key);
            const unsigned need_kb = min(tau_b == kPadElem ? 0xFFFFFFFFu : tk_b + 1u, eps_key);
            const bool amb_a = need_ka > min(g_a, bkey_a) || (tau_a != kPadElem && tk_a >= key_max - 1u);
            const bool amb_b = need_kb > min(g_b, bkey_b) || (tau_b != kPadElem && tk_b >= key_max - 1u);
            // element i ^ element i+1 (one v_xor with a wave_shl:1 operand per set) below 64 <=> same key
            unsigned xa, xb;
            asm("v_xor_b32_dpp %0, %2, %2 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n"
                "v_xor_b32_dpp %1, %3, %3 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n"
                "s_nop 0"
                : "=&v"(xa), "=&v"(xb) : "v"(e_a), "v"(e_b));
#ifndef PCT_ABL_NO_CHECK
            // A query that goes to the redo list is `trusted` when its set is proven all the same: the (k+1)-th entry
            // exists, its key is below every key the pre-selection cut (bkey) and below the saturated one, and entry k+1
            // does not share it (equal keys are not put in order on a redo row: at the boundary the wrong one of the two
            // could be inside).  Entries 0 .. k are then every candidate of the stencil with a key up to entry k's -- what
            // failed is g alone, the cube's guarantee and the sharding limits, and that the exact sweep can mend from
            // ring 2 on (Sweep::adopt).  The eps key is not asked: a list of k+1 real entries lies inside the eps ball.
            const auto trusted = [&](unsigned tau, unsigned tk, unsigned bkey, unsigned x) {
                const bool tie = ((__builtin_amdgcn_ballot_w64(x < 64u) >> k) & 1ull) != 0ull;
                return a.adopt && tau != kPadElem && tk + 1u <= bkey && tk < key_max - 1u && !tie;
            };
            if (ok_a && amb_a) {
                redo_mask |= 1ull << qi; ok_a = false;
                const bool t = trusted(tau_a, tk_a, bkey_a, xa);
                if (lane == qi && t) my_trust |= 1u;
            }
            if (ok_b && amb_b) {
                redo_mask |= 1ull << qj; ok_b = false;
                const bool t = trusted(tau_b, tk_b, bkey_b, xb);
                if (lane == qj && t) my_trust |= 1u;
            }
#endif
            // equal keys among the first k+2 entries: ordered here by the exact values (order_equal_keys)
            {
#ifdef PCT_ABL_NO_CHECK
                const unsigned long long cm_any = 0ull;
#else
                const unsigned long long cm_any = __builtin_amdgcn_ballot_w64(min(xa, xb) < 64u) & first_k1;
#endif
                unsigned long long cm_a = 0ull, cm_b = 0ull;
                if (__builtin_expect(cm_any != 0ull, 0)) {
                    cm_a = __builtin_amdgcn_ballot_w64(xa < 64u && e_a != kPadElem) & first_k1;
                    cm_b = __builtin_amdgcn_ballot_w64(xb < 64u && e_b != kPadElem) & first_k1;
                }
                if (__builtin_expect((cm_a | cm_b) != 0ull, 0)) {
                    if (ok_a && cm_a != 0ull) {
                        const double ux = qax, uy = qay, uz = qaz;
                        const bool done = order_equal_keys<1, SLOT_BITS>(&e_a, a.pts,
                            [&](unsigned at) {
                                const int j = slot_of(L.pend[at]);
                                const double dx = (double)L.cx[j] - ux, dy = (double)L.cy[j] - uy, dz = (double)L.cz[j] - uz;
                                return (dx * dx + dy * dy) + dz * dz;
                            },
                            [&](unsigned at) { return __builtin_amdgcn_ds_bpermute((int)(at & 63u) << 2, out_pa); });
                        if (!done) { redo_mask |= 1ull << qi; ok_a = false; }
                    }
                    if (ok_b && cm_b != 0ull) {
                        const double ux = qbx, uy = qby, uz = qbz;
                        const bool done = order_equal_keys<1, SLOT_BITS>(&e_b, a.pts,
                            [&](unsigned at) {
                                const int j = slot_of((unsigned)L.pend_b[at]);
                                const double dx = (double)L.cx[j] - ux, dy = (double)L.cy[j] - uy, dz = (double)L.cz[j] - uz;
                                return (dx * dx + dy * dy) + dz * dz;
                            },
                            [&](unsigned at) { return __builtin_amdgcn_ds_bpermute((int)(at & 63u) << 2, out_pb); });
                        if (!done) { redo_mask |= 1ull << qj; ok_b = false; }
                    }
                }
            }
            // ---- store: the lane that holds list entry i fetches position (and distance) of survivor e & 63.  A query whose
            // proof failed stores its row like any other (ordered or not, these are k real candidates: the exact sweep
            // starts from the distance of the farthest, Sweep::seed) and is on the redo list all the same.
            {
                const unsigned off_a = lane_off + (unsigned)qi * pitch4, off_b = lane_off + (unsigned)qj * pitch4;
                const bool real_a = e_a != kPadElem, real_b = e_b != kPadElem;
                const int at_a = (int)(e_a << 2), at_b = (int)(e_b << 2);        // ds_bpermute reads lane (address >> 2) & 63: the survivor index
                const int pos_a = __builtin_amdgcn_ds_bpermute(at_a, out_pa), pos_b = __builtin_amdgcn_ds_bpermute(at_b, out_pb);
                float dist_a = 0.f, dist_b = 0.f;
                if constexpr (DIST) {
                    dist_a = __int_as_float(__builtin_amdgcn_ds_bpermute(at_a, __float_as_int(out_da)));
                    dist_b = __int_as_float(__builtin_amdgcn_ds_bpermute(at_b, __float_as_int(out_db)));
                }
#ifdef PCT_ABL_NO_STORE
                if (pos_a == 0x7fffffff && pos_b == 0x7ffffff1)
#endif
                if (col_lane) {
                    *(int*)(pos_item + off_a) = real_a ? pos_a : -1;
                    if constexpr (DIST) *(float*)(dist_item + off_a) = real_a ? dist_a : INFINITY;
                }
#ifdef PCT_ABL_NO_STORE
                if (pos_a == 0x7fffffff && pos_b == 0x7ffffff1)
#endif
                if (live_b && col_lane) {
                    *(int*)(pos_item + off_b) = real_b ? pos_b : -1;
                    if constexpr (DIST) *(float*)(dist_item + off_b) = real_b ? dist_b : INFINITY;
                }
                if constexpr (EPS) {
                    const int f_a = (int)__popcll(__builtin_amdgcn_ballot_w64(real_a && col_lane));
                    const int f_b = (int)__popcll(__builtin_amdgcn_ballot_w64(real_b && col_lane));
                    if (lane == 0) {
                        if (ok_a) a.nbr_cnt[row0 + qi] = f_a;
                        if (ok_b) a.nbr_cnt[row0 + qj] = f_b;
                    }
                }
            }
        }
    };
    {
        using std::integral_constant;
        const int nbp = (m + 127) >> 7;
        if (nbp <= 1) pair_loop(integral_constant<int, 1>{});
        else if (nbp == 2) pair_loop(integral_constant<int, 2>{});
        else if (nbp == 3) pair_loop(integral_constant<int, (CAP >= 384 ? 3 : 1)>{});
        else if (nbp == 4) pair_loop(integral_constant<int, (CAP >= 512 ? 4 : 1)>{});
        else if (nbp == 5) pair_loop(integral_constant<int, (CAP >= 640 ? 5 : 1)>{});
        else pair_loop(integral_constant<int, (CAP >= 768 ? 6 : 1)>{});
    }
#if defined(PCT_ABL_NO_SORT) || defined(PCT_ABL_NO_COMPACT) || defined(PCT_ABL_NO_KEYS) || defined(PCT_ABL_NO_TRIAL) || defined(PCT_ABL_NO_STORE) || defined(PCT_ABL_NO_CHECK)
    redo_mask = 0ull;          // timing experiments: nothing goes to the exact sweep
#endif
    if (redo_mask) {
        const int cnt = (int)__popcll(redo_mask);
        int base = 0;
        if (lane == 0) base = atomicAdd(a.redo_count, cnt);
        base = __builtin_amdgcn_readfirstlane(base);
        if ((redo_mask >> lane) & 1ull)
            a.redo[base + (int)__popcll(redo_mask & ((1ull << lane) - 1ull))] = (int)((unsigned)(row0 + lane) | (my_trust == 1u ? kRedoTrusted : 0u));
        if (a.stats && lane == 0) atomicAdd(&a.counters->redone_queries, (unsigned long long)cnt);
    }
}

// (blocks are dealt to the 8 XCDs in turn, PairArgs::items_per_xcd; PCT_NO_XCD_MAP: one block per item in order)
template <bool EPS, bool DIST, bool Q64, bool TREE>
void launch_pair(pct_ctx* ctx, const PairArgs& pa) {
    const int64_t n_blk = pa.items_per_xcd ? (int64_t)pa.items_per_xcd * 8 : ctx->n_items;
    PCT_LAUNCH_T((k_knn_pair<EPS, DIST, Q64, TREE>), dim3((unsigned)((n_blk + kPairWaves - 1) / kPairWaves)), dim3(64 * kPairWaves), 0,
                 ctx->stream, pa);
}

}  // namespace

void pct_launch_sweep_pair(pct_ctx* ctx, const SweepPlan& p, const KnnArgs& a, int* redo, int* redo_count) {
    const PairArgs pa = make_pair_args(ctx, a, p.tree, redo, redo_count);
    with_bools([&](auto e, auto d, auto q, auto t) { launch_pair<e, d, q, t>(ctx, pa); }, p.eps, p.dist, p.q64, p.tree);
}

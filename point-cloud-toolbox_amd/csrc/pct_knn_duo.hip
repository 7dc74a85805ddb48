// k_knn_duo: k_knn_pair's scheme for rows of 65 .. 128 entries, with its launcher and entry.
#include "pct_knn_item.h"

namespace {

// ---------------------------------------------------------------------------
// k_knn_duo: k_knn_pair's scheme for rows of 65 .. 128 entries (k = 64 .. 127; BASELINE configs[4] asks for k = 80) --
// a float32 cloud, the uniform cell list, a plain sweep.  ONE query per loop trip; its list is two registers per lane
// (element = lane + 64 * register), and the two registers take the roles the two queries of a pair play in
// k_knn_pair: the compaction handles two staged batches per block of instructions, the exact keys of survivors
// `lane` and `lane + 64` are two interleaved fp64 chains, and the sorting network (pct_sort_duo.inc, the same
// generator) sorts the two halves side by side and then merges them (element i against 127 - i, strides 32 .. 1).
// Same proofs, same bit-identical rows as k_knn_fast<2, EPS, true, true>: what could not be proven goes to
// the redo list.  Positions (and distances) of the survivors wait in LDS for the sorted order.
// ---------------------------------------------------------------------------
// Staging capacity: cells are sized for 0.35 (k + 1) points, a surface's 27-cell stencil then holds 12 - 14 cells' worth --
// 400 - 470 candidates at k = 64 .. 80: 512 slots sent 8 % of the items (k = 64) to 30 % (k = 80) to the exact sweep,
// 768 slots (4 waves per SIMD with the 16-bit survivor list) send a handful.
#ifndef PCT_DUO_CAP
#define PCT_DUO_CAP 768
#endif
constexpr int kDuoCap = PCT_DUO_CAP;
template <bool DIST, int CAP>
struct DuoLds {
    float cx[CAP], cy[CAP], cz[CAP];                     // staged stencil, 12 B per candidate
    unsigned short pend[128 + 8];                        // staged slot (| run << 10) of survivor s; (first: the run-start bit string)
    int pay_p[128];                                      // sorted position of survivor s
    float pay_d[DIST ? 128 : 1];                         // its float32 distance
    int offc[16];                                        // sorted position - flat slot, per non-empty run
};

// Q64: a float64 cloud, as in k_knn_pair -- float32-rounded candidates, native float64 queries, every bound taken from the
// float32 pre-selection widened by eq = |q64 - q32|.
// TREE: the items of the hierarchical cell list (as in k_knn_pair), 1024 staged slots -- what pct_tree.hip refines
// segments for when two list registers are in use.
template <bool EPS, bool DIST, bool Q64 = false, bool TREE = false>
__global__ __launch_bounds__(64, ((TREE ? PCT_TREE_CAP2 : PCT_DUO_CAP) <= 768 ? 4 : 3)) void k_knn_duo(PairArgs a) {
    constexpr int CAP = TREE ? PCT_TREE_CAP2 : kDuoCap, LIST = 128, SLOT_BITS = 7, KEY_BITS = 32 - SLOT_BITS;
    static_assert(CAP % 128 == 0 && CAP <= 1024, "slot ids: 10 bits of slot, 4 bits of run index");
    __shared__ DuoLds<DIST, CAP> L;
    const int lane = lane_id();
    const int item = a.items_per_xcd ? ((int)blockIdx.x & 7) * a.items_per_xcd + ((int)blockIdx.x >> 3) : (int)blockIdx.x;
    if (item >= a.n_items) return;
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
    unsigned long long redo_mask = 0ull;
    unsigned my_trust = 0u;        // per query (lane l = query l): 1 = its redo entry carries kRedoTrusted, 2 = never (k_knn_pair)
    if (item_overflows<TREE, NRUNS>(m, CAP, run_len, lane)) {
        if (TREE || !a.seed) {
            hand_item_to_redo(a.redo, a.redo_count, a.counters, a.stats, row0, nq, lane, true, a.nbr_pos, a.pitch);
            return;
        }
        // the item runs on the first CAP flat slots of its stencil and all its queries go to the redo list (k_knn_pair)
        redo_mask = nq >= 64 ? ~0ull : (1ull << nq) - 1ull;
        my_trust = 2u;
        if (a.stats && lane == 0) atomicAdd(&a.counters->lds_overflows, 1ull);
        m = CAP;
    }
    unsigned slotx[CAP / 64];
    {
        unsigned* bits = (unsigned*)L.pend;
        static_assert(sizeof(L.pend) >= CAP / 8, "the run-start bit string lives in the survivor list");
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
                const unsigned long long S = B >> 1;
                const int s0 = ubase + (int)(lo & 1u);
                const int u = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(S >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)S, (unsigned)s0));
                ubase += (int)__popcll(B);
                const int j = b * 64 + lane;
                slotx[b] |= (unsigned)u << 10;
                if (j < m) tmp[b] = a.pts[j + L.offc[u]];
            }
        }
        wave_lds_sync();
#pragma unroll
        for (int b = 0; b < CAP / 64; ++b) {
            const int j = b * 64 + lane;
            if (j < m) {
                L.cx[j] = tmp[b].x; L.cy[j] = tmp[b].y; L.cz[j] = tmp[b].z;
            } else if ((b & ~1) * 64 < m) {
                L.cx[j] = INFINITY; L.cy[j] = 0.f; L.cz[j] = 0.f;
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
    float t_prev_f = 0.f;

    char* const pos_item = (char*)(a.nbr_pos + (int64_t)row0 * a.pitch);
    char* const dist_item = DIST ? (char*)(a.nbr_dist + (int64_t)row0 * a.pitch) : nullptr;
    const unsigned pitch4 = (unsigned)a.pitch * 4u;
    // list entry i = lane + 64 r  ->  table column i - 1
    const unsigned lane_off0 = (unsigned)(lane - 1) * 4u, lane_off1 = (unsigned)(lane + 63) * 4u;
    const bool col0 = lane >= 1 && lane <= k, col1 = lane + 64 <= k;
    // entries 0 .. k are the ones whose order matters: lanes 0 .. k of register 0, lanes 0 .. k - 64 of register 1
    const unsigned long long order_lo = k >= 63 ? ~0ull : (2ull << k) - 1ull;
    const unsigned long long order_hi = k < 64 ? 0ull : k - 64 >= 63 ? ~0ull : (2ull << (k - 64)) - 1ull;
    const unsigned short* pend_hi = &L.pend[64];

    const auto query_loop = [&](auto NBP_) {
        constexpr int NBP = decltype(NBP_)::value, NBU = 2 * NBP;
        for (int qi = 0; qi < nq; ++qi) {
            const float ax = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_q.x), qi));
            const float ay = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_q.y), qi));
            const float az = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_q.z), qi));
            // the query the exact keys measure from: the float32 record widened, or (Q64) the native coordinates
            const auto rl64 = [&](double v, int l) {
                return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
            };
            const double qx = Q64 ? rl64(my_qx, qi) : (double)ax, qy = Q64 ? rl64(my_qy, qi) : (double)ay, qz = Q64 ? rl64(my_qz, qi) : (double)az;
            const float eq = Q64 ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_eq), qi)) : 0.f;
            // ---- float32 squared distances of all staged candidates (packed: two batches per instruction) ----------
            float ap[NBU];
#pragma unroll
            for (int p2 = 0; p2 < NBP; ++p2) {
                const int sa = p2 * 128 + lane, sb = sa + 64;
                const float2v vx = {L.cx[sa], L.cx[sb]}, vy = {L.cy[sa], L.cy[sb]}, vz = {L.cz[sa], L.cz[sb]};
                const float2v dx = vx - ax, dy = vy - ay, dz = vz - az;
                float2v d = dx * dx;
                d = __builtin_elementwise_fma(dy, dy, d);
                d = __builtin_elementwise_fma(dz, dz, d);
                ap[2 * p2] = d.x;
                ap[2 * p2 + 1] = d.y;
            }
            // ---- threshold: k+1 <= #(d < T) <= LIST, never beyond the eps ball (wave-uniform search) -----------------
            // +inf without eps; Q64: exact d < eps  =>  d' < eps + eq
            float T_init = eps2a;
            if constexpr (EPS && Q64) {
                const double ee = eps1 + (double)eq;
                T_init = (float)fmin(ee * ee * (1.0 + 0x1p-18), 3.0e38);
            }
            int tot = m;
            if constexpr (EPS) {
                tot = 0;
#pragma unroll
                for (int b = 0; b < NBU; ++b) tot += (int)__popcll(__builtin_amdgcn_ballot_w64(ap[b] < T_init));
            }
            const bool need = tot > LIST;
            float T = T_init;
            int cnt = tot;
            unsigned bkey = 0xFFFFFFFFu;          // exact keys of the candidates the pre-selection cut are >= bkey
            if (need) {
                const float target = 0.5f * (float)(k + 1 + LIST);
                float t = t_prev_f > 0.f ? t_prev_f : cell2f;
                if (!(t < T_init)) t = 0.5f * T_init;
                float lo = 0.f, hi = T_init;
                bool found = false;
#pragma unroll 1
                for (int trial = 0; trial < 16; ++trial) {
                    int c = 0;
#pragma unroll
                    for (int b = 0; b < NBU; ++b) c += (int)__popcll(__builtin_amdgcn_ballot_w64(ap[b] < t));
                    if ((unsigned)(c - (k + 1)) <= (unsigned)(LIST - (k + 1))) { T = t; cnt = c; found = true; break; }
                    const bool below = c < k + 1;
                    lo = below ? t : lo;
                    hi = below ? hi : t;
                    float nt = t * target * __builtin_amdgcn_rcpf((float)c);
                    if (!(nt > lo && nt < hi)) nt = hi < INFINITY ? 0.5f * (lo + hi) : 2.f * lo;
                    if (__builtin_amdgcn_ballot_w64(!(nt > lo && nt < hi)) != 0ull) break;      // no float left between: a pile of equal distances
                    t = nt;
                }
                if (!found || __builtin_amdgcn_ballot_w64(!(T >= 1e-30f)) != 0ull) {
                    // no threshold: nothing passes, the list is all padding and the row stored below starts with -1 -- the
                    // mark of a redo row without candidates (Sweep::seed)
                    redo_mask |= 1ull << qi;
                    T = 0.f;
                    cnt = 0;
                } else {
                    t_prev_f = T;
                    // smallest exact key a candidate cut by the float32 threshold can have (k_knn_pair)
                    double lo2 = (double)T * (1.0 - 0x1p-20);
                    if constexpr (Q64) {
                        // (sqrt(L) - eq)^2 >= L - 2 eq sqrt(L); an upper bound of the root is enough: float32 root, rounded up
                        const double root_up = (double)__builtin_sqrtf(T) * (1.0 + 0x1p-21);
                        lo2 = fmax(lo2 - 2.0 * (double)eq * root_up, 0.0);
                    }
                    bkey = (unsigned)fmin(lo2 * scale, 4294967294.0);
                }
            }
            // ---- compact the staged slots of the survivors, two batches per block of instructions (k_knn_pair's
            // hand-placed sequence; here both batches append to the same list)
            {
                unsigned wr = (unsigned)(uintptr_t)&L.pend[0], wr1;
                const unsigned long long all = __builtin_amdgcn_read_exec();
                wave_lds_sync();
#pragma unroll
                for (int b = 0; b < NBU; b += 2) {
                    unsigned r0, r1, n0, n1;
                    asm volatile(
                        "v_cmp_gt_f32 vcc, %[t], %[ap0]\n"
                        "v_cmp_gt_f32 s[96:97], %[t], %[ap1]\n"
                        "s_bcnt1_i32_b64 %[n0], vcc\n"
                        "v_mbcnt_lo_u32_b32 %[r0], vcc_lo, 0\n"
                        "s_bcnt1_i32_b64 %[n1], s[96:97]\n"
                        "v_mbcnt_lo_u32_b32 %[r1], s96, 0\n"
                        "v_mbcnt_hi_u32_b32 %[r0], vcc_hi, %[r0]\n"
                        "v_mbcnt_hi_u32_b32 %[r1], s97, %[r1]\n"
                        "s_lshl1_add_u32 %[wr1], %[n0], %[wr]\n"
                        "v_lshl_add_u32 %[r0], %[r0], 1, %[wr]\n"
                        "v_lshl_add_u32 %[r1], %[r1], 1, %[wr1]\n"
                        "s_mov_b64 exec, vcc\n"
                        "ds_write_b16 %[r0], %[slot0]\n"
                        "s_mov_b64 exec, s[96:97]\n"
                        "ds_write_b16 %[r1], %[slot1]\n"
                        "s_mov_b64 exec, %[all]\n"
                        "s_lshl1_add_u32 %[wr], %[n1], %[wr1]\n"
                        : [r0] "=&v"(r0), [r1] "=&v"(r1), [n0] "=&s"(n0), [n1] "=&s"(n1), [wr] "+s"(wr), [wr1] "=&s"(wr1)
                        : [t] "v"(T), [ap0] "v"(ap[b]), [ap1] "v"(ap[b + 1]), [slot0] "v"(slotx[b]), [slot1] "v"(slotx[b + 1]), [all] "s"(all)
                        : "vcc", "scc", "s96", "s97", "memory");
                }
                wave_lds_sync();
            }
            // ---- exact keys of survivors `lane` and `lane + 64` (two interleaved fp64 chains); a stale list entry is
            // masked into the staging area and gives a garbage value nobody uses
            const unsigned sx0 = (unsigned)L.pend[lane] & 0x3FFFu, sx1 = (unsigned)pend_hi[lane] & 0x3FFFu;      // slot | run << 10
            const int j0 = min((int)(sx0 & 1023u), CAP - 1), j1 = min((int)(sx1 & 1023u), CAP - 1);
            unsigned e[2];
            {
                const double dx0 = (double)L.cx[j0] - qx, dy0 = (double)L.cy[j0] - qy, dz0 = (double)L.cz[j0] - qz;
                const double dx1 = (double)L.cx[j1] - qx, dy1 = (double)L.cy[j1] - qy, dz1 = (double)L.cz[j1] - qz;
                const double d20 = (dx0 * dx0 + dy0 * dy0) + dz0 * dz0;
                const double d21 = (dx1 * dx1 + dy1 * dy1) + dz1 * dz1;
                L.pay_p[lane] = j0 + L.offc[sx0 >> 10];
                L.pay_p[lane + 64] = j1 + L.offc[sx1 >> 10];
                if constexpr (DIST) {
                    L.pay_d[lane] = (float)sqrt(d20);
                    L.pay_d[lane + 64] = (float)sqrt(d21);
                }
                const unsigned k0 = (min((unsigned)(d20 * scale), key_max - 1u) << SLOT_BITS) | (unsigned)lane;
                const unsigned k1 = (min((unsigned)(d21 * scale), key_max - 1u) << SLOT_BITS) | (unsigned)(lane + 64);
                e[0] = lane < cnt && (!EPS || d20 < eps2) ? k0 : kPadElem;
                e[1] = lane + 64 < cnt && (!EPS || d21 < eps2) ? k1 : kPadElem;
            }
            wave_lds_sync();
            sort_duo_asm(e[0], e[1], sort_dir);
            // ---- proof obligations (key units, see k_knn_fast) ----------------------------------------------------
            const unsigned tau = (unsigned)__builtin_amdgcn_readlane((int)(k < 64 ? e[0] : e[1]), k & 63);     // the (k+1)-th nearest (padding if fewer exist)
            const unsigned gk = (unsigned)__builtin_amdgcn_readlane((int)my_gkey, qi);
            const unsigned tk = tau >> SLOT_BITS;
            const unsigned need_k = min(tau == kPadElem ? 0xFFFFFFFFu : tk + 1u, eps_key);
            // equal keys: element i ^ element i + 1 below 2^SLOT_BITS <=> same key
            unsigned n0, n1;
            asm("s_nop 1\n"
                "v_mov_b32_dpp %0, %2 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n"
                "v_mov_b32_dpp %1, %3 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n"
                "s_nop 0"
                : "=&v"(n0), "=&v"(n1) : "v"(e[0]), "v"(e[1]));
            n0 = lane == 63 ? (unsigned)__builtin_amdgcn_readlane((int)e[1], 0) : n0;        // entry 64 follows entry 63
            const bool same0 = ((e[0] ^ n0) >> SLOT_BITS) == 0u && e[0] != kPadElem && n0 != kPadElem;
            const bool same1 = ((e[1] ^ n1) >> SLOT_BITS) == 0u && e[1] != kPadElem && n1 != kPadElem && lane < 63;
            // (a query whose proof fails stores its row like any other -- ordered or not, these are k real candidates: the
            // exact sweep starts from the distance of the farthest, Sweep::seed -- and is on the redo list all the same)
            if (need_k > min(gk, bkey) || (tau != kPadElem && tk >= key_max - 1u)) {
                redo_mask |= 1ull << qi;
                // trusted (k_knn_pair): the set is proven -- the (k+1)-th entry exists below bkey and the saturated key, and
                // entry k+1 does not share its key -- so what failed is g alone; never after a failed threshold search
                // (the list is padding: tau is)
                const bool tie = ((__builtin_amdgcn_ballot_w64(k < 64 ? same0 : same1) >> (k & 63)) & 1ull) != 0ull;
                const bool t = a.adopt && tau != kPadElem && tk + 1u <= bkey && tk < key_max - 1u && !tie;
                if (lane == qi && t) my_trust |= 1u;
            }
            // equal keys among the first k + 2 entries: ordered here by the exact values (order_equal_keys)
            {
                const unsigned long long cm = (__builtin_amdgcn_ballot_w64(same0) & order_lo) | (__builtin_amdgcn_ballot_w64(same1) & order_hi);
                if (__builtin_expect(cm != 0ull && ((redo_mask >> qi) & 1ull) == 0ull, 0)) {
                    const bool done = order_equal_keys<2, SLOT_BITS>(e, a.pts,
                        [&](unsigned at) {
                            const int j = min((int)L.pend[at] & 1023, CAP - 1);
                            const double dx = (double)L.cx[j] - qx, dy = (double)L.cy[j] - qy, dz = (double)L.cz[j] - qz;
                            return (dx * dx + dy * dy) + dz * dz;
                        },
                        [&](unsigned at) { return L.pay_p[at]; });
                    if (!done) redo_mask |= 1ull << qi;
                }
            }
            // ---- store: the lane that holds list entry i looks up position (and distance) of survivor e & 127 --------
            {
                const unsigned off0 = lane_off0 + (unsigned)qi * pitch4, off1 = lane_off1 + (unsigned)qi * pitch4;
                const bool real0 = e[0] != kPadElem, real1 = e[1] != kPadElem;
                const int s0 = (int)(e[0] & 127u), s1 = (int)(e[1] & 127u);
                const int pos0 = L.pay_p[s0], pos1 = L.pay_p[s1];
                if (col0) *(int*)(pos_item + off0) = real0 ? pos0 : -1;
                if (col1) *(int*)(pos_item + off1) = real1 ? pos1 : -1;
                if constexpr (DIST) {
                    const float d0 = L.pay_d[s0], d1 = L.pay_d[s1];
                    if (col0) *(float*)(dist_item + off0) = real0 ? d0 : INFINITY;
                    if (col1) *(float*)(dist_item + off1) = real1 ? d1 : INFINITY;
                }
                if constexpr (EPS) {
                    const int f = (int)__popcll(__builtin_amdgcn_ballot_w64(real0 && col0)) + (int)__popcll(__builtin_amdgcn_ballot_w64(real1 && col1));
                    if (lane == 0) a.nbr_cnt[row0 + qi] = f;
                }
            }
            wave_lds_sync();          // the payload arrays are free for the next query
        }
    };
    {
        using std::integral_constant;
        const int nbp = (m + 127) >> 7;
        if (nbp <= 1) query_loop(integral_constant<int, 1>{});
        else if (nbp == 2) query_loop(integral_constant<int, 2>{});
        else if (nbp == 3) query_loop(integral_constant<int, 3>{});
        else if (nbp == 4) query_loop(integral_constant<int, 4>{});
        else if (nbp == 5) query_loop(integral_constant<int, 5>{});
        else if (nbp == 6) query_loop(integral_constant<int, 6>{});
        else if (nbp == 7) query_loop(integral_constant<int, (CAP >= 896 ? 7 : 1)>{});
        else query_loop(integral_constant<int, (CAP >= 1024 ? 8 : 1)>{});
    }
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

template <bool EPS, bool DIST, bool Q64, bool TREE>
void launch_duo(pct_ctx* ctx, const PairArgs& pa) {
    const int64_t n_blk = pa.items_per_xcd ? (int64_t)pa.items_per_xcd * 8 : ctx->n_items;
    PCT_LAUNCH_T((k_knn_duo<EPS, DIST, Q64, TREE>), dim3((unsigned)n_blk), dim3(64), 0, ctx->stream, pa);
}

}  // namespace

void pct_launch_sweep_duo(pct_ctx* ctx, const SweepPlan& p, const KnnArgs& a, int* redo, int* redo_count) {
    const PairArgs pa = make_pair_args(ctx, a, p.tree, redo, redo_count);
    with_bools([&](auto e, auto d, auto q, auto t) { launch_duo<e, d, q, t>(ctx, pa); }, p.eps, p.dist, p.q64, p.tree);
}

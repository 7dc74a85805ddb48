// The sorting network of the fast sweeps (k_knn_fast, k_knn_pair, k_knn_duo) and the in-place repair of equal keys.
#pragma once
#include "pct_knn_sweep.h"

namespace {

constexpr unsigned kPadElem = 0xFFFFFFFFu;

template <int R>
struct FastK {
    unsigned e[R];
};

// ---------------------------------------------------------------------------
// Sorting network of the fast sweep: bitonic merges in the "flip" form -- a merge of two ascending runs of
// SIZE/2 first compares element i with element i ^ (SIZE - 1), then runs the half-cleaners of strides
// SIZE/4 .. 1 -- in which EVERY compare-exchange leaves the smaller element at the lower index.  Which of the two
// a lane keeps therefore depends only on one bit of its lane id: six lane-constant words sel[j] = -(bit j of
// lane) serve all 21 (28) levels, and a level is  partner move + v_med3_u32  (med3(a, b, 0) = min,
// med3(a, b, ~0) = max) with no per-level mask in scalar registers.  Partner moves: DPP for xor 1, 2, 3, 7, 8, 15,
// two DPP moves for xor 4, v_permlane16/32_swap for xor 16 / 32 (the pair of results holds {own, partner} in
// lane-dependent order -- as a set that is all a compare-exchange needs), ds_bpermute for the two wide flips.
// ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned umed3(unsigned a, unsigned b, unsigned c) {
    unsigned r;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

struct SortLanes {
    unsigned sel[6];     // sel[j] = all ones if bit j of the lane id is set
    int a31, a63;        // byte addresses of lanes lane ^ 31, lane ^ 63 for ds_bpermute
};

__device__ __forceinline__ SortLanes make_sort_lanes() {
    SortLanes c;
    const int lane = lane_id();
#pragma unroll
    for (int j = 0; j < 6; ++j) c.sel[j] = (unsigned)__builtin_amdgcn_sbfe(lane, j, 1);
    c.a31 = (lane ^ 31) << 2;
    c.a63 = (lane ^ 63) << 2;
    return c;
}

constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v / 2); }

// compare-exchange with the element STRIDE lanes away (STRIDE < 64), smaller one to the lower lane
template <int R, int STRIDE>
__device__ __forceinline__ void fast_stride(FastK<R>& t, const SortLanes& c) {
    const unsigned sel = c.sel[ilog2(STRIDE)];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if constexpr (STRIDE == 16) {
            const auto p = __builtin_amdgcn_permlane16_swap(t.e[r], t.e[r], false, false);
            t.e[r] = umed3(p[0], p[1], sel);
        } else if constexpr (STRIDE == 32) {
            const auto p = __builtin_amdgcn_permlane32_swap(t.e[r], t.e[r], false, false);
            t.e[r] = umed3(p[0], p[1], sel);
        } else {
            t.e[r] = umed3(t.e[r], (unsigned)lane_xor<STRIDE>((int)t.e[r]), sel);
        }
    }
}

// first step of a merge of SIZE elements: element i against element i ^ (SIZE - 1)
template <int R, int SIZE>
__device__ __forceinline__ void fast_flip(FastK<R>& t, const SortLanes& c) {
    if constexpr (SIZE <= 64) {
        const unsigned sel = c.sel[ilog2(SIZE) - 1];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            unsigned pk;
            if constexpr (SIZE == 2) pk = (unsigned)__builtin_amdgcn_mov_dpp((int)t.e[r], 0xB1, 0xF, 0xF, true);        // quad_perm [1,0,3,2]
            else if constexpr (SIZE == 4) pk = (unsigned)__builtin_amdgcn_mov_dpp((int)t.e[r], 0x1B, 0xF, 0xF, true);   // quad_perm [3,2,1,0]
            else if constexpr (SIZE == 8) pk = (unsigned)__builtin_amdgcn_mov_dpp((int)t.e[r], 0x141, 0xF, 0xF, true);  // row_half_mirror
            else if constexpr (SIZE == 16) pk = (unsigned)__builtin_amdgcn_mov_dpp((int)t.e[r], 0x140, 0xF, 0xF, true); // row_mirror
            else if constexpr (SIZE == 32) pk = (unsigned)__builtin_amdgcn_ds_bpermute(c.a31, (int)t.e[r]);
            else pk = (unsigned)__builtin_amdgcn_ds_bpermute(c.a63, (int)t.e[r]);
            t.e[r] = umed3(t.e[r], pk, sel);
        }
    } else {
        static_assert(SIZE == 128 && R == 2, "two registers per lane at most");
        const unsigned lo_rev = (unsigned)__builtin_amdgcn_ds_bpermute(c.a63, (int)t.e[0]);
        const unsigned hi_rev = (unsigned)__builtin_amdgcn_ds_bpermute(c.a63, (int)t.e[1]);
        t.e[0] = min(t.e[0], hi_rev);
        t.e[1] = max(t.e[1], lo_rev);
    }
}

template <int R, int STRIDE>
__device__ __forceinline__ void fast_strides(FastK<R>& t, const SortLanes& c) {
    if constexpr (STRIDE >= 1) {
        fast_stride<R, STRIDE>(t, c);
        fast_strides<R, STRIDE / 2>(t, c);
    }
}

// ascending sort of 64 R elements (element index = lane + 64 * register), starting from sorted runs of SIZE / 2
template <int R, int SIZE>
__device__ __forceinline__ void fast_sort_from(FastK<R>& t, const SortLanes& c) {
    fast_flip<R, SIZE>(t, c);
    fast_strides<R, SIZE / 4>(t, c);
    if constexpr (SIZE < 64 * R) fast_sort_from<R, SIZE * 2>(t, c);
}

// NSETS independent ascending sorts of 64 R elements each (set s = registers s R .. s R + R - 1), level by level side
// by side: the lane-level steps treat all NSETS R registers alike, only the 128-wide flip pairs registers per set
template <int R, int NSETS, int SIZE>
__device__ __forceinline__ void fast_sort_sets(FastK<NSETS * R>& t, const SortLanes& c) {
    if constexpr (SIZE <= 64) {
        fast_flip<NSETS * R, SIZE>(t, c);
    } else {
        static_assert(SIZE == 128 && R == 2, "two registers per set at most");
#pragma unroll
        for (int s = 0; s < NSETS; ++s) {
            const unsigned lo_rev = (unsigned)__builtin_amdgcn_ds_bpermute(c.a63, (int)t.e[2 * s]);
            const unsigned hi_rev = (unsigned)__builtin_amdgcn_ds_bpermute(c.a63, (int)t.e[2 * s + 1]);
            t.e[2 * s] = min(t.e[2 * s], hi_rev);
            t.e[2 * s + 1] = max(t.e[2 * s + 1], lo_rev);
        }
    }
    fast_strides<NSETS * R, (SIZE / 4 < 32 ? SIZE / 4 : 32)>(t, c);
    if constexpr (SIZE < 64 * R) fast_sort_sets<R, NSETS, SIZE * 2>(t, c);
}

// ---------------------------------------------------------------------------
// The same network as hand-scheduled assembly blocks (tools/gen_sort_asm.py): two independent lists of 64, one register
// each (k_knn_pair), and one list of 128 in two registers, element = lane + 64 * register (k_knn_duo).  The blocks
// assume that the caller's VALU code wrote ea / eb immediately before them (their leading s_nop 1).  They live here, not
// beside their kernels, so that the self-test (pct_knn.hip: k_selftest_sort) runs the very code the sweeps run.
// ---------------------------------------------------------------------------
#ifndef PCT_SORT_INC
#define PCT_SORT_INC "pct_sort_pair.inc"
#endif
#include PCT_SORT_INC
#include "pct_sort_duo.inc"

__device__ __forceinline__ void sort_pair_asm(unsigned& ea, unsigned& eb, const SortLanes& c) {
    unsigned ta, tb;
    asm volatile(PCT_SORT_PAIR_ASM
                 : [ea] "+v"(ea), [eb] "+v"(eb), [ta] "=&v"(ta), [tb] "=&v"(tb)
                 : [sel0] "v"(c.sel[0]), [sel1] "v"(c.sel[1]), [sel2] "v"(c.sel[2]), [sel3] "v"(c.sel[3]), [sel4] "v"(c.sel[4]),
                   [sel5] "v"(c.sel[5]), [a31] "v"(c.a31), [a63] "v"(c.a63));
    ea = PCT_SORT_PAIR_RESULT_A;
    eb = PCT_SORT_PAIR_RESULT_B;
}

__device__ __forceinline__ void sort_duo_asm(unsigned& ea, unsigned& eb, const SortLanes& c) {
    unsigned ta, tb;
    asm volatile(PCT_SORT_DUO_ASM
                 : [ea] "+v"(ea), [eb] "+v"(eb), [ta] "=&v"(ta), [tb] "=&v"(tb)
                 : [sel0] "v"(c.sel[0]), [sel1] "v"(c.sel[1]), [sel2] "v"(c.sel[2]), [sel3] "v"(c.sel[3]), [sel4] "v"(c.sel[4]),
                   [sel5] "v"(c.sel[5]), [a31] "v"(c.a31), [a63] "v"(c.a63));
    const unsigned lo = PCT_SORT_DUO_RESULT_A, hi = PCT_SORT_DUO_RESULT_B;
    ea = lo;
    eb = hi;
}

// ---------------------------------------------------------------------------
// Equal keys inside the sorted list: the quantised key cannot order those elements, the exact values can.
// On the reference's own generator output (theta x phi lattices, utils.py:883-914) every point has symmetric partners
// whose squared distances differ by float32 rounding noise only -- most queries meet at least one pair of equal keys
// among their first k+2 entries, and handing each of them to the wave-per-query exact sweep costs 10-50x the fast
// path.  Instead the list is repaired in place: an odd-even transposition over the sorted list in which two
// neighbours are compared -- by exact fp64 d2, then by public index, the total order of k_knn_exact -- ONLY when
// their keys are equal.  Elements with different keys never move, so every run of equal keys ends up in the exact
// order and everything proven on keys (the (k+1)-th key against the stencil radius, the pre-selection cut, eps)
// stays proven.  Runs are short (2, 4 or 8 symmetric partners): two or three passes and a quiet round.
//   exact_d2(payload)  fp64 squared distance of the element with that payload (LDS reads only; real elements only)
//   pos_of(payload)    its sorted position; may use cross-lane reads: called with every lane active
// Returns false when the list is still not in order after kOrderPasses (a long pile of equal keys): redo list.
// ---------------------------------------------------------------------------
constexpr int kOrderPasses = 36;

template <int R, int SLOT_BITS, class ExactD2, class PosOf>
__device__ __forceinline__ bool order_equal_keys(unsigned* e, const float4* __restrict__ pts, const ExactD2& exact_d2,
                                                 const PosOf& pos_of) {
    const int lane = lane_id();
    constexpr unsigned PAYLOAD = (1u << SLOT_BITS) - 1u;
    double d[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        d[r] = INFINITY;
        if (e[r] != kPadElem) d[r] = exact_d2(e[r] & PAYLOAD);
    }
    int quiet = 0;
#pragma unroll 1
    for (int pass = 0; pass < kOrderPasses; ++pass) {
        const int par = pass & 1;
        const int pl = ((lane - par) ^ 1) + par;      // partner lane: -1 / 64 = last / first lane of the neighbouring register
        const int addr = (pl & 63) << 2;
        const int dr = pl >> 6;                       // -1, 0, +1: register of the partner relative to mine
        unsigned be[R];
        int blo[R], bhi[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            be[r] = (unsigned)__builtin_amdgcn_ds_bpermute(addr, (int)e[r]);
            blo[r] = __builtin_amdgcn_ds_bpermute(addr, __double2loint(d[r]));
            bhi[r] = __builtin_amdgcn_ds_bpermute(addr, __double2hiint(d[r]));
        }
        bool any = false;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int pr = r + dr;
            unsigned pe = kPadElem;
            double pd = INFINITY;
#pragma unroll
            for (int r2 = 0; r2 < R; ++r2)
                if (pr == r2) { pe = be[r2]; pd = __hiloint2double(bhi[r2], blo[r2]); }
            const bool same = pr >= 0 && pr < R && e[r] != kPadElem && pe != kPadElem && ((e[r] ^ pe) >> SLOT_BITS) == 0u;
            bool p_lt_m = pd < d[r], m_lt_p = d[r] < pd;
            const bool tie = same && pd == d[r];
            if (__builtin_amdgcn_ballot_w64(tie) != 0ull) {       // exact tie somewhere: public indices decide
                const int my_pos = pos_of(e[r] & PAYLOAD), p_pos = pos_of(pe & PAYLOAD);
                if (tie) {
                    const int mp = pub_index(pts, my_pos), pp = pub_index(pts, p_pos);
                    p_lt_m = pp < mp;
                    m_lt_p = mp < pp;
                }
            }
            const bool take = same && (pl > lane ? p_lt_m : m_lt_p);     // the lower position keeps the smaller one
            if (take) { e[r] = pe; d[r] = pd; }
            any |= take;
        }
        if (__builtin_amdgcn_ballot_w64(any) != 0ull) quiet = 0;
        else if (++quiet == 2) return true;
    }
    return false;
}

}  // namespace

// How a row's fan is stored (pct_fan.hip writes it, pct_fan.hip and pct_hole.hip read it), and the block-wide partial sums
// both files' statistics go through.  The codes' meaning is at the head of pct_fan.hip.
#pragma once

#include "pct_area_row.h"

namespace {

__device__ __forceinline__ const int* fan_codes(const int2* __restrict__ head, const int* __restrict__ fast, const int* __restrict__ wide,
                                                int wpitch, int64_t i, int& n) {
    const int2 h = head[i];
    n = h.x;
    return h.y < 0 ? fast + i * kAreaCap : wide + (int64_t)h.y * wpitch;
}
__device__ __forceinline__ int code_record(int c) { return c >= 0 ? c : -2 - c; }          // (-1 stays -1)

// a block's share of one statistic into its slot (blocks of 256 threads; no same-address atomics: a last kernel adds the
// slots up)
__device__ __forceinline__ void block_partial(unsigned long long v, bool is_max, unsigned long long* __restrict__ slot) {
    __shared__ unsigned long long sh[4];
    for (int s = 32; s > 0; s >>= 1) {
        const unsigned long long other = __shfl_xor(v, s);
        v = is_max ? (other > v ? other : v) : v + other;
    }
    __syncthreads();                              // (the slot array is used once per statistic)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long r = sh[0];
        for (int w = 1; w < 4; ++w) r = is_max ? (sh[w] > r ? sh[w] : r) : r + sh[w];
        *slot = r;
    }
}

}  // namespace

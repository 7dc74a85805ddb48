// Stage times from device clock stamps.  A call whose route is certain before its first launch (an explicit PCT_KNN_GRID /
// PCT_KNN_GRID_EXACT request that cannot give the uniform list up) records no timing event: every event record is a
// marker packet between two kernels that depend on each other anyway.  Instead the first kernel of every stage stores
// the device's wall clock at its entry -- a marker, too, is processed when the previous kernel has retired -- and the
// last block out of the step's last kernel stores the end.  This header holds the layout of a call's stamps, the device
// helpers (HIP compilations only) and the host's arithmetic on a stamp block, which tests/host/ compiles on its own.
// Which calls take stamps, who hands the words to the kernels and who reads them back is the call clock's business
// (pct_clock.h): the host functions below are called from there and from nowhere else in the library.
#pragma once

#include <stdint.h>

enum pct_stamp_id {
    PCT_ST_CALL_BEGIN,         // entry of the first kernel the cell-list build launches (k_pack | k_bin_count)
    PCT_ST_GRID_END,           // entry of the first kernel of pct_launch_knn_grid: the fast sweep, or the exact kernel when there is none
    PCT_ST_FAST_END,           // entry of the exact kernel (== PCT_ST_GRID_END when no fast sweep ran)
    PCT_ST_SWEEP_END,          // entry of k_fit (a sweep on its own: of k_stamp_end)
    PCT_ST_CALL_END,           // the last block out of k_fit_svd (a sweep on its own: k_stamp_end); non-zero = the call has finished
    PCT_ST_COUNT
};
// The stamps of one call: 64 bytes.  One block per parity of the fused call in device memory (pct_dev_words::stamps, written
// by the stage kernels) and one in pinned memory (pct_pinned::stamps, mirrored whole by the writer of PCT_ST_CALL_END, that
// word last).
struct pct_stamp_block {
    unsigned long long t[8];   // pct_stamp_id; three spare words
};

struct pct_stage_ms { float grid, knn, knn_fast, fit, total; };

// Which calls are timed by stamps: the route must be certain before the first launch -- an explicit request for the uniform
// cell list (PCT_KNN_GRID, PCT_KNN_GRID_EXACT: auto_req false, so the list is neither given up nor examined), no slab
// ownership (its build starts with the split), at least one owned row (no rows, no fit kernels to end the call) -- and the
// clock rate known.  events_forced: PCT_TIME_EVENTS.
inline bool pct_stamps_apply(bool auto_req, bool uniform_list, bool slab, int64_t owned_rows, int rate_khz, bool events_forced) {
    return !auto_req && uniform_list && !slab && owned_rows > 0 && rate_khz > 0 && !events_forced;
}
// The parity of the next fused call's stamp block (and of its other pinned slots): the other one while a call is pending.
inline int pct_next_parity(bool pending, int pending_par) { return pending ? pending_par ^ 1 : 0; }

// Ticks of the device's wall clock between two stamps as milliseconds; rate_khz = hipDeviceAttributeWallClockRate.
// 0 for an unknown rate and for stamps that do not advance (a missing stamp, a clock that is not one clock).
inline float pct_ticks_ms(unsigned long long from, unsigned long long to, int rate_khz) {
    if (rate_khz <= 0 || to <= from) return 0.f;
    return (float)((double)(to - from) / (double)rate_khz);
}

// The pending call has finished when its end stamp -- cleared by the host before the call was enqueued, stored last by the
// device -- is non-zero.  (A volatile read: the device writes the word while the host polls it.)
inline bool pct_stamps_finished(const pct_stamp_block* b) {
    return ((const volatile unsigned long long*)b->t)[PCT_ST_CALL_END] != 0ull;
}

// The stage times of a finished call (a sweep on its own ends where its sweep does: fit = 0).  total is the sum of the stages' ticks, so grid + knn + fit == total to float rounding.
inline pct_stage_ms pct_stamps_ms(const pct_stamp_block* b, int rate_khz) {
    const unsigned long long* t = b->t;
    pct_stage_ms m;
    m.grid = pct_ticks_ms(t[PCT_ST_CALL_BEGIN], t[PCT_ST_GRID_END], rate_khz);
    m.knn = pct_ticks_ms(t[PCT_ST_GRID_END], t[PCT_ST_SWEEP_END], rate_khz);
    m.knn_fast = pct_ticks_ms(t[PCT_ST_GRID_END], t[PCT_ST_FAST_END], rate_khz);
    m.fit = pct_ticks_ms(t[PCT_ST_SWEEP_END], t[PCT_ST_CALL_END], rate_khz);
    m.total = pct_ticks_ms(t[PCT_ST_CALL_BEGIN], t[PCT_ST_CALL_END], rate_khz);
    return m;
}

#if defined(__HIPCC__)
// The first thread of block 0 stores the wall clock to `slot` (and to `also`: one reading for two boundaries that coincide).
// Null = the call is timed by events.  The block test comes first and alone: a scalar branch on a register the block
// starts with, so every other block skips the rest without waiting for the kernel argument that holds `slot`.
// Where it is called: at the kernel's entry in the build, exact and fit kernels.  In the three fast sweeps it stands BEHIND
// the item prologue, once, in front of the overflow hand-over and the loop.  At their entry -- and likewise in front of
// the two returns that precede the prologue's end -- it made the compiler load the work item, its cell's bounds and its
// first row with vector loads where it had used scalar loads, for every block and whether or not a stamp was asked for:
// k_knn_duo 1.1 % and k_knn_pair 0.5 - 1 % slower (profiles/r08_a_stage_stamps_ab.txt, block 3).  Behind the prologue the
// kernels keep the loads and registers the parent's had; the grid's end gets its stamp two or three dependent load latencies
// into block 0.  Block 0 never takes either of the two earlier returns in a call timed by stamps: it holds work item 0, which is
// out of range only when there are no items (no owned rows: pct_stamps_apply), and split segments exist on the hierarchical
// list alone, which is timed by events.
__device__ __forceinline__ void pct_stamp(unsigned long long* slot, unsigned long long* also = nullptr) {
    if (__builtin_expect(blockIdx.x != 0, 1)) return;
    if (threadIdx.x == 0 && slot) {
        const unsigned long long now = wall_clock64();
        *slot = now;
        if (also) *also = now;
    }
}

// At the END of the step's last kernel, called by every thread of every block: the blocks take a ticket and the last one
// out mirrors the call's device stamps to pinned memory, the end stamp last, and leaves the tickets at zero for the next
// launch.  Returns true in that one thread (it may have more to mirror: before the end stamp is what `pin` must hold then).
//
// Two levels of tickets, each on a 128-byte line of its own: block b counts on line 1 + b % 32, the last of a line on line
// 0.  All blocks of a launch whose list is empty end within a microsecond of each other, and 1024 returning atomics on one
// address are served one after the other at the memory side: measured, they and a system-scope fence per block made the
// fit stage of the 1 M-point step 15 us longer (profiles/r08_a_stage_stamps_ab.txt); two levels are 32 + 32 deep.
// No fence in the other blocks: what they store is device memory that the next kernel or the next synchronisation reads,
// as without stamps.  The ONE thread that ends the call stores the end stamp with a system-scope release, so a host that
// sees it sees the words mirrored in front of it (one cache write-back per launch, not the 1024 measured above).
constexpr int kStampTicketLines = 33, kStampTicketStride = 32;         // unsigned words per 128-byte line
__device__ __forceinline__ bool pct_stamp_last_out(const unsigned long long* dev, unsigned long long* pin, unsigned* tickets,
                                                   long long* pin_word = nullptr, long long word = 0) {
    if (!dev) return false;
    __syncthreads();
    if (threadIdx.x != 0) return false;
    const unsigned groups = gridDim.x < 32u ? gridDim.x : 32u, g = blockIdx.x & 31u;
    const unsigned in_group = (gridDim.x - g + 31u) >> 5;
    unsigned* mine = tickets + (1 + g) * kStampTicketStride;
    if (atomicAdd(mine, 1u) != in_group - 1u) return false;
    atomicExch(mine, 0u);
    if (atomicAdd(tickets, 1u) != groups - 1u) return false;
    atomicExch(tickets, 0u);
    for (int i = 0; i < PCT_ST_CALL_END; ++i) pin[i] = dev[i];
    if (pin_word) *pin_word = word;
    __hip_atomic_store(&pin[PCT_ST_CALL_END], (unsigned long long)wall_clock64(), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    return true;
}
#endif

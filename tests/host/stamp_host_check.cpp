// The host's arithmetic on a call's device clock stamps (csrc/pct_stamp.h), checked without a GPU and without Python:
// ticks to milliseconds, "the pending call has finished", which calls are timed by stamps, the parity of the next call.
// Stand-alone: compile with the host compiler and -fsanitize=address,undefined, run directly; exit status 0 = all held.
//   c++ -std=c++17 -fsanitize=address,undefined -I point-cloud-toolbox_amd/csrc tests/host/stamp_host_check.cpp -o stamp_host_check
#include "pct_stamp.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int g_failed = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond);      \
            ++g_failed;                                                   \
        }                                                                 \
    } while (0)

static bool near(float got, double want) { return fabs((double)got - want) <= 1e-6 * fabs(want); }

int main() {
    static_assert(sizeof(pct_stamp_block) == 64, "eight 64-bit words");
    static_assert(PCT_ST_COUNT <= 8, "a call's stamps fit one block");
    static_assert(PCT_ST_CALL_END == PCT_ST_COUNT - 1, "the end stamp is stored last");

    // ---- ticks -> milliseconds: rate in kHz = ticks per millisecond
    CHECK(pct_ticks_ms(0, 100000, 100000) == 1.0f);                        // 100 MHz: 100 000 ticks are one millisecond
    CHECK(near(pct_ticks_ms(1000, 67600, 100000), 0.666));
    CHECK(pct_ticks_ms(5, 6, 100000) == 1e-5f);                            // one tick of 10 ns
    CHECK(pct_ticks_ms(0, 25000, 25000) == 1.0f);                          // another clock
    // stamps far into the counter's range: the difference is taken in integers, before any rounding
    const unsigned long long far = 0xfffffff000000000ull;
    CHECK(pct_ticks_ms(far, far + 100000, 100000) == 1.0f);
    // unknown rate, missing stamp, stamps that do not advance: 0, never negative, never a division by zero
    CHECK(pct_ticks_ms(0, 100000, 0) == 0.f);
    CHECK(pct_ticks_ms(0, 100000, -1) == 0.f);
    CHECK(pct_ticks_ms(7, 7, 100000) == 0.f);
    CHECK(pct_ticks_ms(8, 7, 100000) == 0.f);

    // ---- finished: the end stamp, cleared by the host before the call, is non-zero
    pct_stamp_block* b = (pct_stamp_block*)calloc(2, sizeof(pct_stamp_block));     // (heap: the sanitizer watches the bounds)
    if (!b) return 2;
    CHECK(!pct_stamps_finished(&b[0]) && !pct_stamps_finished(&b[1]));
    b[0].t[PCT_ST_CALL_BEGIN] = 1000; b[0].t[PCT_ST_GRID_END] = 10000; b[0].t[PCT_ST_FAST_END] = 46000; b[0].t[PCT_ST_SWEEP_END] = 49100;
    CHECK(!pct_stamps_finished(&b[0]));                                    // every stage stamped, the end not yet
    b[0].t[PCT_ST_CALL_END] = 67600;
    CHECK(pct_stamps_finished(&b[0]) && !pct_stamps_finished(&b[1]));      // ... and the other parity's block is its own
    b[1].t[PCT_ST_CALL_END] = 1;                                           // any non-zero word, the smallest included
    CHECK(pct_stamps_finished(&b[1]));

    // ---- the stages of a finished fused call add up to its total
    pct_stage_ms m = pct_stamps_ms(&b[0], 100000);
    CHECK(near(m.grid, 0.09) && near(m.knn, 0.391) && near(m.knn_fast, 0.36) && near(m.fit, 0.185) && near(m.total, 0.666));
    CHECK(fabs((double)m.grid + m.knn + m.fit - m.total) <= 4 * 5.96e-8 * m.total);
    // no fast sweep: the exact kernel stamps both boundaries with one reading
    b[0].t[PCT_ST_FAST_END] = b[0].t[PCT_ST_GRID_END];
    CHECK(pct_stamps_ms(&b[0], 100000).knn_fast == 0.f);
    // a sweep on its own ends where the sweep does
    b[0].t[PCT_ST_CALL_END] = b[0].t[PCT_ST_SWEEP_END];
    m = pct_stamps_ms(&b[0], 100000);
    CHECK(m.fit == 0.f && near(m.total, 0.481) && fabs((double)m.grid + m.knn - m.total) <= 4 * 5.96e-8 * m.total);
    // rate 0: every time reads 0
    m = pct_stamps_ms(&b[0], 0);
    CHECK(m.grid == 0.f && m.knn == 0.f && m.knn_fast == 0.f && m.fit == 0.f && m.total == 0.f);
    // counters that are not one clock (a later stage stamped earlier): that stage reads 0, nothing is negative
    b[1].t[PCT_ST_CALL_BEGIN] = 500; b[1].t[PCT_ST_GRID_END] = 400; b[1].t[PCT_ST_FAST_END] = 450; b[1].t[PCT_ST_SWEEP_END] = 900; b[1].t[PCT_ST_CALL_END] = 1000;
    m = pct_stamps_ms(&b[1], 100000);
    CHECK(m.grid == 0.f && m.knn > 0.f && m.fit > 0.f && m.total > 0.f);

    // ---- the host clears the end stamp of the parity it is about to enqueue: the block of a call two steps back reads
    // "not finished" again, the pending call's block is untouched (wrapped parity: 0, 1, 0, 1, ...)
    int par = pct_next_parity(false, 0);
    CHECK(par == 0);
    bool pending = false;
    int pend_par = 0;
    memset(b, 0, 2 * sizeof(pct_stamp_block));
    for (int call = 0; call < 5; ++call) {
        par = pct_next_parity(pending, pend_par);
        CHECK(par == (call & 1));
        b[par].t[PCT_ST_CALL_END] = 0;                                     // host, before enqueueing
        CHECK(!pct_stamps_finished(&b[par]));
        if (pending) CHECK(pct_stamps_finished(&b[pend_par]));             // (the device finished it meanwhile, below)
        b[par].t[PCT_ST_CALL_END] = 1000ull * (call + 1);                  // device, at the end of the call
        pending = true;
        pend_par = par;
    }
    CHECK(pct_next_parity(true, 1) == 0 && pct_next_parity(true, 0) == 1 && pct_next_parity(false, 1) == 0);
    free(b);

    // ---- which calls are timed by stamps (auto_req, uniform_list, slab, owned_rows, rate_khz, events_forced)
    CHECK(pct_stamps_apply(false, true, false, 1, 100000, false));
    CHECK(!pct_stamps_apply(true, true, false, 1, 100000, false));         // PCT_KNN_AUTO: the route is open
    CHECK(!pct_stamps_apply(false, false, false, 1, 100000, false));       // the tree, the chain, brute force
    CHECK(!pct_stamps_apply(false, true, true, 1, 100000, false));         // slab ownership
    CHECK(!pct_stamps_apply(false, true, false, 0, 100000, false));        // no owned row: no fit kernel ends the call
    CHECK(!pct_stamps_apply(false, true, false, 1, 0, false));             // unknown clock rate
    CHECK(!pct_stamps_apply(false, true, false, 1, 100000, true));         // PCT_TIME_EVENTS

    if (g_failed) printf("%d checks failed\n", g_failed);
    else printf("stamp_host_check ok\n");
    return g_failed ? 1 : 0;
}

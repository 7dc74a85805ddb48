// The call clock: the stage timing of ONE sweep or fused call, and the only code that knows which source times it -- the
// device clock stamps of pct_stamp.h (a call whose route is certain before its first launch: no marker between its
// kernels) or five events, one per stage boundary.  The step's chain (run_knn, the cell-list build, the sweep launchers,
// the fit launch) receives the clock as an argument and tells it where the boundaries are; none of it asks which source is
// in use.  One clock per parity of the call on the handle (pct_ctx::clock), like the pinned slots of that parity: the
// pending call of an asynchronous stream keeps its clock while the next call runs on the other one.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/pct_hip.h"
#include "pct_stamp.h"

struct pct_ctx;

// FUSED: cell list | sweep | fit, the call ends behind its fit.  SWEEP: a sweep on its own, the call ends where its sweep
// does (fit_ms = 0).  SWEEP_HEAD: a sweep in front of kernels its caller times itself -- always on events, and read()
// leaves fit_ms and total_ms alone.
enum pct_call_kind { PCT_CALL_FUSED, PCT_CALL_SWEEP, PCT_CALL_SWEEP_HEAD };

// milliseconds between two events that have been recorded and passed (0 where the runtime cannot tell); the handle's
// stopwatch pairs (pct_event) are read with it too
inline float pct_event_ms(hipEvent_t from, hipEvent_t to) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, from, to) != hipSuccess) ms = 0.f;
    return ms;
}

struct pct_call_clock {
    // set by pct_create, which also creates the events (pct_destroy destroys them)
    hipEvent_t ev[PCT_ST_COUNT] = {};      // by pct_stamp_id: the boundary's marker in a call timed by events
    int par = 0;                           // which of the handle's two
    pct_stamp_block* pin = nullptr;        // the pinned stamp block of this parity, whose end word says "finished"
    int rate_khz = 0;                      // hipDeviceAttributeWallClockRate: ticks of a stamp per millisecond (0: unknown, every call is timed by events)
    // the call in progress or last made
    pct_stamp_block* dev = nullptr;        // the device stamp block of this parity, written by the stage kernels (set by a call that opens on stamps)
    unsigned* tickets = nullptr;           // the handle's ticket lines (pct_stamp_last_out)
    bool stamped = false, begun = false;   // its source; its begin has been taken, as a stamp word or as an event
    pct_call_kind kind = PCT_CALL_SWEEP;

    // Before the call's first launch.  Stamps where pct_stamps_apply says so: the device words and the ticket lines are
    // reserved (the tickets zeroed once per allocation) and the pinned end word is cleared.  Records nothing.
    int open(pct_ctx* ctx, bool auto_req, bool uniform_list, pct_call_kind call_kind);
    // Where the call starts on the stream: a clock on events records its begin; one on stamps leaves it to the build.
    hipError_t start(hipStream_t stream) { return stamped ? hipSuccess : begin_event(stream); }
    // The cell-list build's first launch, once per call (later passes and restarted attempts get null / nothing): a kernel
    // with a stamp argument takes begin_word(); in front of any other first launch begin_event() records the begin, and the
    // clock is on events for the rest of the call.
    unsigned long long* begin_word();
    hipError_t begin_event(hipStream_t stream);
    // A stage boundary lies here on the stream: recorded on events, nothing on stamps ...
    hipError_t boundary(pct_stamp_id id, hipStream_t stream) { return stamped ? hipSuccess : hipEventRecord(ev[id], stream); }
    // ... where the stage's first kernel stamps word(id) instead; null on events.
    unsigned long long* word(pct_stamp_id id) const { return stamped ? &dev->t[id] : nullptr; }
    // The end of the call.  A fused call on stamps hands end_words() to its fit launch: k_fit stamps the end of the sweep
    // and the last block out of k_fit_svd ends the call (all null on events).  end() stands behind the call's last launch:
    // a fused call on events records its end, a sweep on its own on stamps launches k_stamp_end, and a sweep on events has
    // ended at its sweep-end boundary.
    void end_words(unsigned long long** stamps, unsigned long long** stamps_pin, unsigned** ticket) const;
    hipError_t end(hipStream_t stream);
    // The pending call of an asynchronous stream
    bool finished() const { return stamped ? pct_stamps_finished(pin) : hipEventQuery(ev[PCT_ST_CALL_END]) == hipSuccess; }
    hipError_t wait(hipStream_t stream) const { return stamped ? hipStreamSynchronize(stream) : hipEventSynchronize(ev[PCT_ST_CALL_END]); }
    // The stage times of the finished call; sorted: its table is in a sorted space, so knn_fast_ms applies
    void read(bool sorted, pct_timings* t) const;
    // PCT_CALL_SWEEP_HEAD: milliseconds from the call's begin to an event of the caller's
    float since_begin(hipEvent_t to) const { return pct_event_ms(ev[PCT_ST_CALL_BEGIN], to); }
};

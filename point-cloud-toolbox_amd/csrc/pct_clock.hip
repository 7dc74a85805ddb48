// The call clock (pct_clock.h): the host side of a call's stage timing, for both of its sources.
#include "pct_internal.h"

// A sweep on its own, timed by stamps, has no fit kernel behind it to end the call: one thread, whose start is the end of the sweep.
extern "C" __global__ void k_stamp_end(const unsigned long long* __restrict__ dev, unsigned long long* __restrict__ pin) {
    const unsigned long long now = wall_clock64();
    for (int i = 0; i < PCT_ST_SWEEP_END; ++i) pin[i] = dev[i];
    pin[PCT_ST_SWEEP_END] = now;
    __hip_atomic_store(&pin[PCT_ST_CALL_END], now, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

int pct_call_clock::open(pct_ctx* ctx, bool auto_req, bool uniform_list, pct_call_kind call_kind) {
    kind = call_kind;
    begun = false;
    stamped = kind != PCT_CALL_SWEEP_HEAD && pct_stamps_apply(auto_req, uniform_list, ctx->slab_parts >= 1, ctx->q_end - ctx->q_begin, rate_khz,
                                                              pct_getenv("PCT_TIME_EVENTS") != nullptr);
    if (!stamped) return PCT_OK;
    const size_t ticket_bytes = (size_t)kStampTicketLines * kStampTicketStride * sizeof(unsigned);
    PCT_TRY(pct_reserve(ctx, &ctx->counters, sizeof(pct_dev_words)));
    const bool fresh = ctx->stamp_tickets.p == nullptr;        // (one size for the handle's life: allocated once)
    PCT_TRY(pct_reserve(ctx, &ctx->stamp_tickets, ticket_bytes));
    if (fresh) PCT_HIP(ctx, hipMemsetAsync(ctx->stamp_tickets.p, 0, ticket_bytes, ctx->stream));      // (once: the last block out leaves the tickets at zero)
    dev = &pct_dev(ctx)->stamps[par];
    tickets = (unsigned*)ctx->stamp_tickets.p;
    pin->t[PCT_ST_CALL_END] = 0ull;        // "finished" is this word non-zero
    return PCT_OK;
}

unsigned long long* pct_call_clock::begin_word() {
    if (begun) return nullptr;
    begun = true;
    return &dev->t[PCT_ST_CALL_BEGIN];
}

hipError_t pct_call_clock::begin_event(hipStream_t stream) {
    if (begun) return hipSuccess;
    begun = true;
    stamped = false;
    return hipEventRecord(ev[PCT_ST_CALL_BEGIN], stream);
}

void pct_call_clock::end_words(unsigned long long** stamps, unsigned long long** stamps_pin, unsigned** ticket) const {
    *stamps = stamped ? dev->t : nullptr;
    *stamps_pin = stamped ? pin->t : nullptr;
    *ticket = stamped ? tickets : nullptr;
}

hipError_t pct_call_clock::end(hipStream_t stream) {
    if (kind == PCT_CALL_FUSED) return boundary(PCT_ST_CALL_END, stream);
    if (!stamped) return hipSuccess;
    PCT_LAUNCH(k_stamp_end, dim3(1), dim3(1), 0, stream, (const unsigned long long*)dev->t, pin->t);
    return hipGetLastError();
}

void pct_call_clock::read(bool sorted, pct_timings* t) const {
    const bool fused = kind == PCT_CALL_FUSED;
    pct_stage_ms m = {};
    if (stamped) m = pct_stamps_ms(pin, rate_khz);
    else {                 // the same differences between the events; a sweep on its own ends at its sweep-end boundary
        const hipEvent_t last = ev[fused ? PCT_ST_CALL_END : PCT_ST_SWEEP_END];
        m.grid = pct_event_ms(ev[PCT_ST_CALL_BEGIN], ev[PCT_ST_GRID_END]);
        m.knn = pct_event_ms(ev[PCT_ST_GRID_END], ev[PCT_ST_SWEEP_END]);
        if (sorted) m.knn_fast = pct_event_ms(ev[PCT_ST_GRID_END], ev[PCT_ST_FAST_END]);
        if (fused) m.fit = pct_event_ms(ev[PCT_ST_SWEEP_END], last);
        if (kind != PCT_CALL_SWEEP_HEAD) m.total = pct_event_ms(ev[PCT_ST_CALL_BEGIN], last);
    }
    t->grid_ms = m.grid;
    t->knn_ms = m.knn;
    t->knn_fast_ms = sorted ? m.knn_fast : 0.f;
    if (kind == PCT_CALL_SWEEP_HEAD) return;       // (its caller times what follows the sweep)
    t->fit_ms = fused ? m.fit : 0.f;
    t->total_ms = m.total;
}

// C ABI of the curvature path (include/pct_hip.h).  Host-side orchestration
// only: buffer ownership, launch order, hipEvent timing, status mapping.
#include "pct_internal.h"
#include "pct_auto_route.h"
#include "pct_query_plan.h"
#include "pct_ball_plan.h"

#include <execinfo.h>
#include <math.h>
#include <mutex>
#include <signal.h>
#include <stdarg.h>
#include <stdlib.h>
#include <sys/prctl.h>
#include <unistd.h>
#include <vector>

int pct_fail(pct_ctx* ctx, int code, const char* fmt, ...) {
    if (ctx) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(ctx->err, sizeof(ctx->err), fmt, ap);
        va_end(ap);
    }
    return code;
}

extern char** environ;
const char* pct_getenv(const char* name) {
    struct Entry { const char* name; const char* value; };
    static std::mutex m;
    static Entry cache[48];
    static int used = 0;
    static uintptr_t fp = 0;
    std::lock_guard<std::mutex> g(m);
    uintptr_t now = 1469598103934665603ull;
    for (char** e = environ; e && *e; ++e) now = (now ^ (uintptr_t)*e) * 1099511628211ull;     // setenv allocates a new string
    if (now != fp) { fp = now; used = 0; }
    for (int i = 0; i < used; ++i)
        if (cache[i].name == name) return cache[i].value;
    const char* v = getenv(name);
    if (used < 48) cache[used++] = Entry{name, v};
    return v;
}

void pct_release(pct_buf* b) {
    if (b->p) (void)hipFree(b->p);
    b->p = nullptr;
    b->cap = 0;
}

int pct_reserve(pct_ctx* ctx, pct_buf* b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b->cap >= bytes) return PCT_OK;
    if (b->p) {
        PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        pct_release(b);
    }
    size_t want = bytes + bytes / 8 + 256;   // a little head-room for repeated calls with growing sizes
    // (debugging: exact sizes -- every growing request moves the buffer, so code that keeps a pointer across a
    // reserve, or counts on the spare bytes behind a buffer, shows)
    if (pct_getenv("PCT_NO_HEADROOM")) want = bytes;
    hipError_t e = hipMalloc(&b->p, want);
    if (e != hipSuccess) {
        b->p = nullptr;
        return pct_fail(ctx, PCT_ERR_OOM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    }
    b->cap = want;
    return PCT_OK;
}

int pct_claim_bytes(pct_ctx* ctx, size_t bytes, void** out, const char* who) {
    if (ctx->stage_top >= kPctStageSlots)
        return pct_fail(ctx, PCT_ERR_INVALID, "%s: every one of the %d staging slots is claimed", who, kPctStageSlots);
    pct_buf* slot = &ctx->stage[ctx->stage_top];
    PCT_TRY(pct_reserve(ctx, slot, bytes));
    ++ctx->stage_top;
    *out = slot->p;
    return PCT_OK;
}

int pct_reserve_fit(pct_ctx* ctx, int64_t rows) {
    PCT_TRY(pct_reserve(ctx, &ctx->coefs, (size_t)rows * 6 * sizeof(float)));
    PCT_TRY(pct_reserve(ctx, &ctx->K, (size_t)rows * sizeof(float)));
    PCT_TRY(pct_reserve(ctx, &ctx->H, (size_t)rows * sizeof(float)));
    PCT_TRY(pct_reserve(ctx, &ctx->H2, (size_t)rows * sizeof(float)));
    return PCT_OK;
}

// the statistics a sweep left, as the timings report them
static void read_sweep_stats(const pct_sweep_words& w, pct_timings* t) {
    t->ring_fallbacks = (int64_t)w.ring_fallbacks;
    t->lds_overflows = (int64_t)w.lds_overflows;
    t->flushes = (int64_t)w.flushes;
    t->candidate_steps = (int64_t)w.candidate_steps;
    t->redone_queries = (int64_t)w.redone_queries;
    t->redo_adopted = (int32_t)w.redo_adopted;
}

// bookkeeping of the pending fused call, whose kernels have finished: timings from its clock, statistics
static void finish_pending(pct_ctx* ctx) {
    const int par = ctx->pend.par;
    pct_timings t = ctx->pend.tm;
    read_sweep_stats(ctx->pin->stats[par], &t);
    ctx->clock[par].read(ctx->pend.sorted, &t);
    t.fit_svd_rows = ctx->pin->svd_rows[par];
    ctx->tm_done = t;
    ctx->pend.on = false;
}

// every entry point but an asynchronous pct_curvature: wait for the pending call and do its bookkeeping first
static int drain(pct_ctx* ctx) {
    if (!ctx->pend.on) return PCT_OK;
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    finish_pending(ctx);
    ctx->tm = ctx->tm_done;
    PCT_HIP(ctx, e);
    return PCT_OK;
}

int pct_begin_call(pct_ctx* ctx, bool wait_for_pending) {
    if (!ctx) return PCT_ERR_INVALID;
    ctx->err[0] = 0;
    ctx->stage_top = 0;            // (an error return of the call before left its claims standing: nothing to clean up)
    PCT_HIP(ctx, hipSetDevice(ctx->device));
    if (wait_for_pending) PCT_TRY(drain(ctx));
    return PCT_OK;
}

int pct_begin_row_call(pct_ctx* ctx, const char* what) {
    PCT_TRY(pct_begin_call(ctx));
    if (ctx->slab_parts >= 1)
        return pct_fail(ctx, PCT_ERR_INVALID, "%s: this handle owns a slab, not an index range (pct_slab_records / pct_scatter_records)", what);
    return PCT_OK;
}

// ---- what the row getters share, those of the surface stages included ----------------------------------------------------
// the range error of a row getter: rows [begin, end) within the rows r covers, which start at base; what: "the owned range", ...
int pct_check_owned_span(pct_ctx* ctx, const char* what, pct_resident r, int64_t begin, int64_t end, int64_t base) {
    if (begin < base || end > base + ctx->res.rows_of(r) || begin > end)
        return pct_fail(ctx, PCT_ERR_INVALID, "rows [%lld,%lld) outside %s", (long long)begin, (long long)end, what);
    return PCT_OK;
}

// rows [first, first + rows) of r's columns to the caller: through row_of where r is stored in table-row order (row_of
// outlives the table, PCT_TABLE_LOST: whatever rewrites the cell order drops r, and query_state keeps a query's build away)
int pct_get_rows(pct_ctx* ctx, pct_resident r, const pct_column* cols, int ncol, int64_t first, int64_t rows) {
    if (rows == 0) return PCT_OK;
    const int* map = nullptr;
    if (ctx->res.in_row_order(r)) {
        PCT_TRY(pct_ensure_row_of(ctx));
        map = (const int*)ctx->row_of.p;
    }
    return pct_download_columns(ctx, cols, ncol, first, rows, map);
}

extern "C" {

const char* pct_version(void) { return "pct_hip 0.1 (gfx950)"; }

int pct_device_count(int* count) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    if (count) *count = n;
    return e == hipSuccess ? PCT_OK : PCT_ERR_NO_DEVICE;
}

// PCT_ABORT_TRACE=1: a SIGABRT anywhere in the process first writes the NATIVE backtrace and the name of the thread
// that raised it to stderr, then goes on to whoever handled the signal before (Python's fault handler, the default
// action).  Twice in two rounds a GPU test run died with nothing but "Fatal Python error: Aborted" in its log -- no
// GPU fault line, no glibc diagnostic: the raiser is some library's bare abort(), possibly on a runtime
// helper thread that a Python traceback cannot show.  Tests, bench.py and smoke() switch this on.
extern "C++" {
const char* pct_last_launch = "(none)";
const char* pct_launch_name(const char* where, const char* instantiation) {
    const size_t len = strlen(where) + 2 + strlen(instantiation) + 1;
    char* s = (char*)malloc(len);
    if (!s) return where;
    snprintf(s, len, "%s  %s", where, instantiation);
    return s;
}
}
static struct sigaction g_prev_abrt;
static int g_abrt_fd = 2;       // PCT_ABORT_TRACE=<fd>: a descriptor of the REAL stderr (a test runner that captures fd 2
                                // -- pytest -- would swallow the trace with the dying process; tests/conftest.py dups it
                                // before capturing starts)
// Best effort only: backtrace() and backtrace_symbols_fd() are not async-signal-safe (an abort raised from inside
// malloc or the unwinder can hang here instead of dying) -- the hook is OPT-IN (PCT_ABORT_TRACE: tests, bench.py and
// smoke() set it; a host application that loads the library does not get its SIGABRT disposition touched).
static volatile sig_atomic_t g_in_abort_trace = 0;
static void abort_trace(int) {
    if (g_in_abort_trace) {                    // a second abort while tracing the first: give up tracing
        sigaction(SIGABRT, &g_prev_abrt, nullptr);
        raise(SIGABRT);
        return;
    }
    g_in_abort_trace = 1;
    static const char head[] = "\n[pct] SIGABRT -- native backtrace of the raising thread";
    const int fd = g_abrt_fd;
    (void)!write(fd, head, sizeof(head) - 1);
    char name[32] = {0};
    if (prctl(PR_GET_NAME, name, 0, 0, 0) == 0) {
        (void)!write(fd, " (", 2);
        (void)!write(fd, name, strnlen(name, sizeof(name)));
        (void)!write(fd, ")", 1);
    }
    (void)!write(fd, ":\n", 2);
    static const char last[] = "[pct] last kernel launched by the library: ";
    (void)!write(fd, last, sizeof(last) - 1);
    const char* ll = __atomic_load_n(&pct_last_launch, __ATOMIC_RELAXED);
    (void)!write(fd, ll, strlen(ll));
    (void)!write(fd, "\n", 1);
    void* frames[64];
    const int n = backtrace(frames, 64);
    backtrace_symbols_fd(frames, n, fd);
    sigaction(SIGABRT, &g_prev_abrt, nullptr);
    raise(SIGABRT);
}
static void install_abort_trace() {
    static std::once_flag once;
    std::call_once(once, [] {
        const char* e = getenv("PCT_ABORT_TRACE");
        if (!e) return;
        const int fd = atoi(e);
        if (fd > 2) g_abrt_fd = fd;
        void* warm[4];
        (void)backtrace(warm, 4);                 // loads the unwinder now, not inside the handler
        struct sigaction sa;
        memset(&sa, 0, sizeof(sa));
        sa.sa_handler = abort_trace;
        sigemptyset(&sa.sa_mask);
        sa.sa_flags = 0;
        sigaction(SIGABRT, &sa, &g_prev_abrt);
    });
}

int pct_create(int device, pct_ctx** out) {
    if (!out) return PCT_ERR_INVALID;
    *out = nullptr;
    install_abort_trace();
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return PCT_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return PCT_ERR_NO_DEVICE;
    pct_ctx* ctx = new pct_ctx();
    ctx->device = device;
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return PCT_ERR_HIP;
    }
    bool events = true;           // the handle's stopwatch pairs and the boundaries of its two call clocks
    for (auto& e : ctx->ev) events = events && hipEventCreate(&e) == hipSuccess;
    for (auto& c : ctx->clock)
        for (auto& e : c.ev) events = events && hipEventCreate(&e) == hipSuccess;
    if (!events) {
        delete ctx;
        return PCT_ERR_HIP;
    }
    if (hipHostMalloc((void**)&ctx->pin, 4096, hipHostMallocMapped) != hipSuccess) {
        delete ctx;
        return PCT_ERR_OOM;
    }
    memset(ctx->pin, 0, 4096);
    // the call clocks' pinned stamps, by parity, and the ticks of the device's wall clock per millisecond (unknown: every call keeps its events)
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || khz < 0) khz = 0;
    (void)hipGetLastError();
    for (int par = 0; par < 2; ++par) {
        ctx->clock[par].par = par;
        ctx->clock[par].pin = &ctx->pin->stamps[par];
        ctx->clock[par].rate_khz = khz;
    }
    *out = ctx;
    return PCT_OK;
}

void pct_destroy(pct_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    pct_comm_release(ctx);
    // the buffers free themselves when the handle is deleted: what is destroyed after them is taken out of it first
    pct_pinned* const pin = ctx->pin;
    const hipStream_t stream = ctx->stream;
    std::vector<hipEvent_t> events(ctx->ev, ctx->ev + PCT_EV_COUNT);
    for (auto& c : ctx->clock) events.insert(events.end(), c.ev, c.ev + sizeof(c.ev) / sizeof(c.ev[0]));
    delete ctx;
    if (pin) (void)hipHostFree(pin);
    for (hipEvent_t e : events)
        if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
}

const char* pct_last_error(const pct_ctx* ctx) { return ctx ? ctx->err : "null context"; }

// a change of ownership -- rows [begin, end), or (parts >= 1) a slab, whose rows the build cuts: the cell order depends on it
static void own_rows(pct_ctx* ctx, int64_t begin, int64_t end, int32_t part, int32_t parts) {
    ctx->q_begin = begin;
    ctx->q_end = end;
    ctx->slab_parts = parts;
    ctx->slab_part = part;
    ctx->slab_split_valid = ctx->grid_valid = false;
    ctx->res.drop(PCT_OWNERSHIP);
    ctx->no_cull = false;
    ctx->retries = 0;
}

static int new_cloud(pct_ctx* ctx, int64_t n) {
    if (n <= 0 || n > (int64_t)INT32_MAX - 1024) return pct_fail(ctx, PCT_ERR_INVALID, "cloud size %lld out of range", (long long)n);
    ctx->n = n;
    own_rows(ctx, 0, n, 0, 0);
    ctx->res.drop(PCT_NEW_CLOUD);
    ctx->pts4_valid = ctx->qpts4_valid = false;
    ctx->has_f64 = ctx->culled = false;
    ctx->tm = pct_timings{};
    return PCT_OK;
}

int pct_set_points_f32(pct_ctx* ctx, const float* xyz, int64_t n) {
    PCT_TRY(pct_begin_call(ctx));
    if (!xyz) return pct_fail(ctx, PCT_ERR_INVALID, "null coordinates");
    PCT_TRY(new_cloud(ctx, n));
    PCT_TRY(pct_reserve(ctx, &ctx->xyz, (size_t)n * 3 * sizeof(float)));
    PCT_HIP(ctx, hipEventRecord(ctx->ev[PCT_EV_IO_BEGIN], ctx->stream));
    PCT_HIP(ctx, hipMemcpyAsync(ctx->xyz.p, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    ctx->xyz_view = (const float*)ctx->xyz.p;
    PCT_HIP(ctx, hipEventRecord(ctx->ev[PCT_EV_IO_END], ctx->stream));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->tm.upload_ms = pct_ev_ms(ctx, PCT_EV_IO_BEGIN, PCT_EV_IO_END);
    return PCT_OK;
}

int pct_set_points_f64(pct_ctx* ctx, const double* xyz, int64_t n) {
    PCT_TRY(pct_begin_call(ctx));
    if (!xyz) return pct_fail(ctx, PCT_ERR_INVALID, "null coordinates");
    PCT_TRY(new_cloud(ctx, n));
    PCT_HIP(ctx, hipEventRecord(ctx->ev[PCT_EV_IO_BEGIN], ctx->stream));
    double* d_xyz = nullptr;
    PCT_TRY(pct_claim_upload(ctx, xyz, (size_t)n * 3, &d_xyz));
    PCT_TRY(pct_pack_points_f64(ctx, d_xyz));
    PCT_HIP(ctx, hipEventRecord(ctx->ev[PCT_EV_IO_END], ctx->stream));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->has_f64 = true;
    ctx->tm.upload_ms = pct_ev_ms(ctx, PCT_EV_IO_BEGIN, PCT_EV_IO_END);
    return PCT_OK;
}

int pct_set_points_device_f32(pct_ctx* ctx, const void* dev_xyz, int64_t n) {
    PCT_TRY(pct_begin_call(ctx));
    if (!dev_xyz) return pct_fail(ctx, PCT_ERR_INVALID, "null coordinates");
    PCT_TRY(new_cloud(ctx, n));
    PCT_TRY(pct_reserve(ctx, &ctx->xyz, (size_t)n * 3 * sizeof(float)));
    PCT_HIP(ctx, hipMemcpyAsync(ctx->xyz.p, dev_xyz, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->xyz_view = (const float*)ctx->xyz.p;
    return PCT_OK;
}

int pct_use_points_device_f32(pct_ctx* ctx, const void* dev_xyz, int64_t n) {
    PCT_TRY(pct_begin_call(ctx));
    if (!dev_xyz) return pct_fail(ctx, PCT_ERR_INVALID, "null coordinates");
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, dev_xyz) != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != ctx->device) {
        (void)hipGetLastError();
        return pct_fail(ctx, PCT_ERR_INVALID, "pct_use_points_device_f32: not a device pointer of device %d", ctx->device);
    }
    PCT_TRY(new_cloud(ctx, n));
    ctx->xyz_view = (const float*)dev_xyz;
    return PCT_OK;
}

int pct_set_query_range(pct_ctx* ctx, int64_t begin, int64_t end) {
    PCT_TRY(pct_begin_call(ctx));
    if (ctx->n <= 0) return pct_fail(ctx, PCT_ERR_INVALID, "no cloud loaded");
    if (begin < 0 || end > ctx->n || begin > end) return pct_fail(ctx, PCT_ERR_INVALID, "bad query range [%lld,%lld)", (long long)begin, (long long)end);
    own_rows(ctx, begin, end, 0, 0);
    return PCT_OK;
}

int pct_set_query_slab(pct_ctx* ctx, int32_t part, int32_t parts) {
    PCT_TRY(pct_begin_call(ctx));
    if (ctx->n <= 0) return pct_fail(ctx, PCT_ERR_INVALID, "no cloud loaded");
    if (parts > PCT_SLAB_PARTS_MAX || (parts >= 1 && (part < 0 || part >= parts)))
        return pct_fail(ctx, PCT_ERR_INVALID, "bad slab %d of %d (at most %d parts)", part, parts, PCT_SLAB_PARTS_MAX);
    if (parts >= 1 && (ctx->has_f64 || ctx->n < 4096))
        return pct_fail(ctx, PCT_ERR_INVALID, "slab ownership serves float32 clouds of at least 4096 points (use index ranges)");
    // the whole cloud until the build has cut it (one part: the whole cloud as one slab -- the same code path, for a world of one rank)
    own_rows(ctx, 0, ctx->n, parts >= 1 ? part : 0, parts >= 1 ? parts : 0);
    return PCT_OK;
}

int pct_slab_counts(pct_ctx* ctx, int64_t* counts, int32_t parts) {
    PCT_TRY(pct_begin_call(ctx));
    if (ctx->slab_parts < 1 || !ctx->slab_split_valid || !ctx->res.has(PCT_R_FIT))
        return pct_fail(ctx, PCT_ERR_INVALID, "pct_slab_counts: no slab pass on this handle (pct_set_query_slab, pct_curvature)");
    if (!counts || parts != ctx->slab_parts) return pct_fail(ctx, PCT_ERR_INVALID, "pct_slab_counts: %d parts asked, the cloud was cut into %d", parts, ctx->slab_parts);
    for (int p = 0; p < parts; ++p) counts[p] = ctx->slab_counts[p];
    return PCT_OK;
}

namespace {
// rows of the slab in table (cell) order -> (public index, K, H)
__global__ __launch_bounds__(256) void k_slab_records(const float4* __restrict__ sorted4, const int* __restrict__ owned_pos,
                                                      const float* __restrict__ K, const float* __restrict__ H, int64_t rows,
                                                      float* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    out[3 * r + 0] = sorted4[owned_pos[r]].w;          // (the public index as int32 bits)
    out[3 * r + 1] = K[r];
    out[3 * r + 2] = H[r];
}

__global__ __launch_bounds__(256) void k_scatter_records(const float* __restrict__ rec, int64_t n_rec, int64_t begin, int64_t end,
                                                         float* __restrict__ K, float* __restrict__ H, unsigned long long* __restrict__ hits) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool hit = false;
    if (i < n_rec) {
        const int64_t pub = (int64_t)__float_as_int(rec[3 * i + 0]);
        hit = pub >= begin && pub < end;
        if (hit) {
            K[pub - begin] = rec[3 * i + 1];
            H[pub - begin] = rec[3 * i + 2];
        }
    }
    const unsigned long long m = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(hits, (unsigned long long)__popcll(m));
}
}  // namespace

int pct_slab_records(pct_ctx* ctx, float* dev_records, int64_t capacity_rows, int64_t* rows_out) {
    PCT_TRY(pct_begin_call(ctx));
    if (ctx->slab_parts < 1 || !ctx->slab_split_valid || !ctx->res.has(PCT_R_FIT) || !ctx->knn_sorted_space || !ctx->res.in_row_order(PCT_R_FIT))
        return pct_fail(ctx, PCT_ERR_INVALID, "pct_slab_records: no slab pass on this handle (pct_set_query_slab, pct_curvature)");
    const int64_t rows = ctx->q_end - ctx->q_begin;
    if (rows_out) *rows_out = rows;
    if (rows > capacity_rows || (rows > 0 && !dev_records))
        return pct_fail(ctx, PCT_ERR_INVALID, "pct_slab_records: %lld rows, room for %lld", (long long)rows, (long long)capacity_rows);
    if (rows == 0) return PCT_OK;
    PCT_LAUNCH(k_slab_records, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, ctx->stream, (const float4*)ctx->sorted4.p,
               (const int*)ctx->owned_pos.p, (const float*)ctx->K.p, (const float*)ctx->H.p, rows, dev_records);
    PCT_HIP(ctx, hipGetLastError());
    return PCT_OK;
}

int pct_scatter_records(pct_ctx* ctx, const float* dev_records, int64_t n_records, int64_t begin, int64_t end, float* dev_K, float* dev_H) {
    PCT_TRY(pct_begin_call(ctx));
    if (n_records < 0 || begin < 0 || end < begin || (n_records > 0 && !dev_records) || (end > begin && (!dev_K || !dev_H)))
        return pct_fail(ctx, PCT_ERR_INVALID, "pct_scatter_records: bad arguments");
    PCT_TRY(pct_reserve(ctx, &ctx->counters, sizeof(pct_dev_words)));
    unsigned long long* d_hits = &pct_dev(ctx)->scatter_hits;
    PCT_HIP(ctx, hipMemsetAsync(d_hits, 0, sizeof(unsigned long long), ctx->stream));
    if (n_records > 0)
        PCT_LAUNCH(k_scatter_records, dim3((unsigned)((n_records + 255) / 256)), dim3(256), 0, ctx->stream, dev_records, n_records, begin,
                   end, dev_K, dev_H, d_hits);
    PCT_HIP(ctx, hipGetLastError());
    unsigned long long* h = &ctx->pin->scatter_hits;
    PCT_HIP(ctx, hipMemcpyAsync(h, d_hits, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if ((int64_t)*h != end - begin)
        return pct_fail(ctx, PCT_ERR_INVALID, "pct_scatter_records: %llu of the %lld records fall into rows [%lld,%lld) -- the slabs do not partition the cloud",
                        *h, (long long)n_records, (long long)begin, (long long)end);
    return PCT_OK;
}

int pct_set_grid_param(pct_ctx* ctx, double occupancy_factor) {
    PCT_TRY(pct_begin_call(ctx));
    ctx->occupancy_factor = occupancy_factor > 0 ? occupancy_factor : 0.0;
    return PCT_OK;
}

int pct_set_stats(pct_ctx* ctx, int32_t enable) {
    PCT_TRY(pct_begin_call(ctx));
    ctx->collect_stats = enable != 0;
    return PCT_OK;
}

// ---- the sweep of a call: which structure serves it (the rules: pct_auto_route.h), built and swept ---------------------
struct SweepDone { bool rows_fitted = false; };     // the passes of a chained sweep fitted the rows they answered: no fit is left to launch

// a sweep has left its table; hier: from the hierarchical list or the chain of cell lists
static void table_left(pct_ctx* ctx, bool hier) {
    ctx->knn_hier = hier;
    ctx->res.leave(PCT_R_TABLE, ctx->knn_sorted_space, ctx->q_end - ctx->q_begin);
}
static bool tree_table_resident(const pct_ctx* ctx) { return ctx->res.has(PCT_R_TABLE) && ctx->knn_hier; }

// The chain of cell lists.  fuse_par: every pass fits its rows, into the pinned slots of this parity (null: no fits).
static int sweep_levels(pct_ctx* ctx, int32_t k, double eps, const int* fuse_par, pct_call_clock& clock, SweepDone* done) {
    ctx->tm.algo = PCT_KNN_GRID_LEVELS;
    PCT_HIP(ctx, clock.boundary(PCT_ST_GRID_END, ctx->stream));
    PCT_TRY(pct_knn_levels(ctx, k, eps, fuse_par, &clock));
    PCT_HIP(ctx, clock.boundary(PCT_ST_FAST_END, ctx->stream));
    PCT_HIP(ctx, clock.boundary(PCT_ST_SWEEP_END, ctx->stream));
    ctx->tm.knn_launches = ctx->tm.levels;
    table_left(ctx, true);
    done->rows_fitted = fuse_par != nullptr;
    return PCT_OK;
}

// The hierarchical cell list of a whole cloud.  *verdict: Built -- swept; Unusable (extents or eps outside what the float32
// pre-selection can square) -- the chain of cell lists swept instead; OtherCloud (expect_bbox: the box a remembered
// verdict was given for, null: any cloud) -- nothing built or swept, the caller goes on.
static int sweep_tree(pct_ctx* ctx, int32_t k, double eps, bool want_dist, const float* expect_bbox, const int* fuse_par, pct_call_clock& clock,
                      SweepDone* done, TreeVerdict* verdict) {
    ctx->tm.algo = PCT_KNN_TREE;
    PCT_TRY(pct_build_tree(ctx, k, eps, expect_bbox, verdict));
    if (*verdict == TreeVerdict::OtherCloud) return PCT_OK;
    if (*verdict == TreeVerdict::Unusable) return sweep_levels(ctx, k, eps, fuse_par, clock, done);
    PCT_HIP(ctx, clock.boundary(PCT_ST_GRID_END, ctx->stream));
    PCT_TRY(pct_launch_knn_tree(ctx, k, eps, want_dist, &clock));
    PCT_HIP(ctx, clock.boundary(PCT_ST_SWEEP_END, ctx->stream));
    ctx->tm.knn_launches = 1;
    table_left(ctx, true);
    return PCT_OK;
}

// The exhaustive sweep: no cell list, the packed cloud
static int sweep_brute(pct_ctx* ctx, int32_t k, double eps, pct_call_clock& clock) {
    float bbox[6];
    PCT_TRY(pct_pack_points(ctx, bbox));
    ctx->tm.grid_iters = 0;
    ctx->tm.cells = ctx->tm.occupied_cells = 0;
    ctx->tm.grid_points = ctx->n;
    ctx->tm.cell_size = 0;
    PCT_HIP(ctx, clock.boundary(PCT_ST_GRID_END, ctx->stream));
    PCT_TRY(pct_launch_knn_brute(ctx, k, eps));
    PCT_HIP(ctx, clock.boundary(PCT_ST_SWEEP_END, ctx->stream));
    ctx->tm.knn_launches = 1;
    table_left(ctx, false);
    return PCT_OK;
}

// PCT_KNN_AUTO behind a uniform list just built, past the skew gate: is one cell size enough?  *route: Stay, or the
// structure the census sends the call to instead (tree_reachable: the hierarchical list, else the chain of cell lists).
static int examine_uniform_list(pct_ctx* ctx, int32_t k, bool tree_reachable, Route* route) {
    const bool debug = pct_getenv("PCT_GRID_DEBUG") != nullptr;
    const double skew = cell_skew(ctx->tm.occupancy, ctx->nonempty_cells, ctx->n);
    if (debug) fprintf(stderr, "[auto] occupancy %.1f, %lld non-empty cells, skew %.2f\n", ctx->tm.occupancy, (long long)ctx->nonempty_cells, skew);
    *route = Route::Stay;
    if (!(skew > skew_min(tree_reachable))) return PCT_OK;
    unsigned long long c[4];
    PCT_TRY(pct_item_census(ctx, k, c));
    const CensusShares s = census_shares(c);
    if (debug) fprintf(stderr, "[auto] census: %llu queries, %llu overflow, %llu short, %.1f non-empty stencil cells\n", c[0], c[1], c[2], s.cells);
    *route = census_route(s, ctx->n, tree_reachable);
    return PCT_OK;
}

// Neighbour sweep without timing bookkeeping.  clock: the call's, opened here once the request is known and told where
// the call begins, where the cell list ends and where the sweep ends; whatever follows the sweep (fused_call, pct_knn)
// ends it.  kind == PCT_CALL_FUSED: the fit reads no distances, and the passes of a chained sweep fit their rows into
// the pinned slots of the clock's parity.
static int run_knn(pct_ctx* ctx, int32_t k, double eps, int32_t asked, pct_call_clock& clock, pct_call_kind kind, SweepDone* done = nullptr) {
    SweepDone unread;
    if (!done) done = &unread;
    *done = SweepDone{};
    const int* fuse_par = kind == PCT_CALL_FUSED ? &clock.par : nullptr;
    const bool want_dist = fuse_par == nullptr;
    // 1. the request
    if (ctx->n <= 0) return pct_fail(ctx, PCT_ERR_INVALID, "no cloud loaded");
    if (k < 1 || k > PCT_K_MAX) return pct_fail(ctx, PCT_ERR_INVALID, "k=%d outside [1,%d]", k, PCT_K_MAX);
    if ((int64_t)k + 1 > ctx->n) return pct_fail(ctx, PCT_ERR_K_TOO_LARGE, "k+1=%d exceeds the cloud size %lld", k + 1, (long long)ctx->n);
    if (!(eps >= 0) || isinf(eps)) eps = 0;
    const bool whole = ctx->q_begin == 0 && ctx->q_end == ctx->n;
    Request rq;
    switch (resolve_request(asked, k, ctx->n, whole, ctx->slab_parts >= 1, fuse_par != nullptr, &rq)) {
        case Refusal::UnknownAlgorithm: return pct_fail(ctx, PCT_ERR_INVALID, "unknown algorithm %d", rq.algo);
        case Refusal::SlabNeedsFusedGrid: return pct_fail(ctx, PCT_ERR_INVALID, "slab ownership: pct_curvature with PCT_KNN_AUTO / PCT_KNN_GRID only");
        case Refusal::None: break;
    }
    const int32_t algo = rq.algo;
    RouteSwitches sw = {false, false};             // (they matter to PCT_KNN_AUTO only)
    if (rq.auto_req) sw = RouteSwitches{pct_getenv("PCT_NO_TREE") != nullptr, pct_getenv("PCT_NO_AUTO_LEVELS") != nullptr};
    ctx->res.drop(PCT_PLANTING);       // the request is resolved: nothing refuses it from here on
    ctx->k = k;
    ctx->eps = eps;
    PCT_TRY(clock.open(ctx, rq.auto_req, algo == PCT_KNN_GRID || algo == PCT_KNN_GRID_EXACT, kind));
    PCT_HIP(ctx, clock.start(ctx->stream));
    ctx->tm.levels = 0;
    ctx->tm.sweep_variant = 0;         // (set by the fast sweep's launch, pct_knn.hip)
    ctx->tm.algo = algo;
    TreeVerdict tree;
    if (algo == PCT_KNN_TREE)
        return rq.tree_ok ? sweep_tree(ctx, k, eps, want_dist, nullptr, fuse_par, clock, done, &tree) : sweep_levels(ctx, k, eps, fuse_par, clock, done);
    // 2. the remembered hierarchical list
    if (remembered_applies(rq, ctx->n, ctx->auto_tree_n, &ctx->auto_tree_calls, sw)) {
        PCT_TRY(sweep_tree(ctx, k, eps, want_dist, ctx->auto_tree_bbox, fuse_par, clock, done, &tree));
        if (tree != TreeVerdict::OtherCloud) return PCT_OK;
        ctx->auto_tree_n = 0;
        ctx->tm.algo = algo;
    }
    if (algo == PCT_KNN_GRID_LEVELS) return sweep_levels(ctx, k, eps, fuse_par, clock, done);
    if (algo == PCT_KNN_BRUTE) return sweep_brute(ctx, k, eps, clock);
    // 3. the uniform list (PCT_KNN_GRID, PCT_KNN_GRID_EXACT) -- and whether PCT_KNN_AUTO keeps it
    const bool tree_reachable = may_give_up(rq, ctx->n, sw);
    GridVerdict built;
    PCT_TRY(pct_build_grid(ctx, k, eps, tree_reachable, &built, &clock, nullptr));
    Route route = built == GridVerdict::GaveUp ? Route::Tree : Route::Stay;      // (not built: far too many cells per point)
    if (built == GridVerdict::Built && skew_gate(rq, whole, ctx->n, ctx->nonempty_cells, sw)) {
        PCT_TRY(examine_uniform_list(ctx, k, tree_reachable, &route));
        if (route == Route::Stay) ctx->auto_tree_n = 0;
    }
    if (route == Route::Tree) {
        PCT_TRY(sweep_tree(ctx, k, eps, want_dist, nullptr, fuse_par, clock, done, &tree));
        if (tree == TreeVerdict::Built) {          // the next cloud of this size and box goes there directly
            ctx->auto_tree_n = ctx->n;
            memcpy(ctx->auto_tree_bbox, ctx->tree_bbox, sizeof(ctx->tree_bbox));
        }
        return PCT_OK;
    }
    if (route == Route::Levels) return sweep_levels(ctx, k, eps, fuse_par, clock, done);
    // 4. the sweep
    PCT_HIP(ctx, clock.boundary(PCT_ST_GRID_END, ctx->stream));
    PCT_TRY(pct_launch_knn_grid(ctx, k, eps, algo == PCT_KNN_GRID_EXACT, 0, want_dist, &clock, nullptr));
    PCT_HIP(ctx, clock.boundary(PCT_ST_SWEEP_END, ctx->stream));
    ctx->tm.knn_launches = 1;
    table_left(ctx, false);
    return PCT_OK;
}

// The fused call, enqueued: the sweep and its tail -- the fit (where the passes of a chained sweep have not fitted their
// rows), the call's end on its clock, and the sweep's statistics words into the pinned slot of the clock's parity,
// mirrored by the fit kernel, else copied.
// (the fit stage has no boundary of its own: it starts where the sweep ends)
// *fit_by_row: the order the fit results are stored in, for the caller's fit_left
static int fused_call(pct_ctx* ctx, int32_t k, double eps, int32_t algo, pct_call_clock& clock, bool* fit_by_row) {
    SweepDone swept;
    PCT_TRY(run_knn(ctx, k, eps, algo, clock, PCT_CALL_FUSED, &swept));
    bool mirrored = false;
    *fit_by_row = false;          // (the passes fitted their rows: public order)
    if (!swept.rows_fitted) PCT_TRY(pct_launch_fit_table(ctx, FitSlot{clock.par, true, &clock}, &mirrored, fit_by_row));
    PCT_HIP(ctx, clock.end(ctx->stream));
    if (!mirrored)                // (no fit kernel ran: the chained sweep fitted its passes itself, or there are no rows)
        PCT_HIP(ctx, hipMemcpyAsync(&ctx->pin->stats[clock.par],ctx->counters.p, sizeof(pct_sweep_words), hipMemcpyDeviceToHost, ctx->stream));
    return PCT_OK;
}

// words_enqueued: the fused tail has sent the statistics words to pinned slot 0 already
static int finish_knn_stats(pct_ctx* ctx, const pct_call_clock& clock, bool words_enqueued, bool* beyond_limits) {
    pct_sweep_words& w = ctx->pin->stats[0];                             // pinned: a plain DMA, no staging
    if (!words_enqueued) PCT_HIP(ctx, hipMemcpyAsync(&w, ctx->counters.p, sizeof(w), hipMemcpyDeviceToHost, ctx->stream));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    read_sweep_stats(w, &ctx->tm);
    if (pct_getenv("PCT_TREE_DEBUG") && ctx->collect_stats)
        fprintf(stderr, "[tree] redone %llu, up-levelled %llu, candidate steps %llu, costliest exact query: %llu steps (row %llu)\n", w.redone_queries,
                w.ring_fallbacks, w.candidate_steps, w.costliest >> 32, w.costliest & 0xffffffffull);
    clock.read(ctx->knn_sorted_space, &ctx->tm);
    // a sharded handle that left far points out of its grid met a query those points could matter to
    *beyond_limits = ctx->knn_sorted_space && ctx->culled && w.beyond_limits > 0;
    ctx->tm.limit_retries = ctx->retries;
    return PCT_OK;
}

// rare: a culled grid met a query the points it left out could matter to -- the caller repeats with every point in it
static void retry_without_cull(pct_ctx* ctx) {
    ctx->no_cull = true;
    ctx->retries = 1;
    ctx->cull_box_valid = false;   // the cached box was too small for this cloud: measure it again next time
}

int pct_knn(pct_ctx* ctx, int32_t k, double eps, int32_t algo) {
    PCT_TRY(pct_begin_call(ctx));
    bool again = false;
    for (int attempt = 0; attempt < 2; ++attempt) {
        PCT_TRY(run_knn(ctx, k, eps, algo, ctx->clock[0], PCT_CALL_SWEEP));
        PCT_HIP(ctx, ctx->clock[0].end(ctx->stream));
        PCT_TRY(finish_knn_stats(ctx, ctx->clock[0], false, &again));
        if (!again) break;
        retry_without_cull(ctx);
    }
    return PCT_OK;
}

// The end of every fit: results for `rows` rows -- cloud-aligned (rows [q_begin, q_end), by_row: as their launcher stored
// them) or the rows of the call in the call's order.  They replace the fit before them and whatever was made from it.
static int fit_left(pct_ctx* ctx, int64_t rows, bool cloud_aligned, bool by_row) {
    ctx->fit_cloud_aligned = cloud_aligned;
    ctx->res.leave(PCT_R_FIT, by_row, rows);
    return PCT_OK;
}

int pct_fit(pct_ctx* ctx) {
    PCT_TRY(pct_begin_row_call(ctx, "pct_fit"));
    if (!ctx->res.has(PCT_R_TABLE)) return pct_fail(ctx, PCT_ERR_NO_NEIGHBORS, "plant the neighbour table first (pct_knn)");
    PCT_HIP(ctx, hipEventRecord(ctx->ev[PCT_EV_FIT_BEGIN], ctx->stream));
    bool by_row = false;
    PCT_TRY(pct_launch_fit_table(ctx, FitSlot{0, false, nullptr}, nullptr, &by_row));
    PCT_HIP(ctx, hipEventRecord(ctx->ev[PCT_EV_FIT_END], ctx->stream));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->tm.fit_ms = pct_ev_ms(ctx, PCT_EV_FIT_BEGIN, PCT_EV_FIT_END);
    ctx->tm.fit_svd_rows = ctx->pin->svd_rows[0];
    return fit_left(ctx, ctx->q_end - ctx->q_begin, true, by_row);
}

int pct_set_async(pct_ctx* ctx, int32_t enable) {
    PCT_TRY(pct_begin_call(ctx));
    ctx->async_mode = enable != 0;
    return PCT_OK;
}

// pct_curvature of a stream of clouds (pct_set_async): enqueue and return.  The previous call's bookkeeping is done here,
// after the cell list's mid-build wait -- which lies behind all of that call's kernels on the stream --, without a wait
// of its own.
static int curvature_async(pct_ctx* ctx, int32_t k, double eps, int32_t algo) {
    const bool had = ctx->pend.on;
    const int par = pct_next_parity(had, ctx->pend.par);        // (the pending call keeps its clock and its pinned slots)
    pct_call_clock& clock = ctx->clock[par];
    ctx->retries = 0;
    bool fit_by_row = false;
    const int st = fused_call(ctx, k, eps, algo, clock, &fit_by_row);
    if (st != PCT_OK) {            // leave the handle in the plain state: nothing pending
        (void)hipStreamSynchronize(ctx->stream);
        if (had) finish_pending(ctx);
        return st;
    }
    if (had) {
        // its kernels lie in front of this call's mid-build wait on the stream: normally long finished (checked, not assumed)
        const pct_call_clock& prev = ctx->clock[ctx->pend.par];
        if (!prev.finished()) (void)prev.wait(ctx->stream);
        (void)hipGetLastError();
        finish_pending(ctx);
    }
    ctx->tm.limit_retries = 0;
    ctx->pend.tm = ctx->tm;
    ctx->pend.par = par;
    ctx->pend.sorted = ctx->knn_sorted_space;
    ctx->pend.on = true;
    return fit_left(ctx, ctx->q_end - ctx->q_begin, true, fit_by_row);
}

int pct_curvature(pct_ctx* ctx, int32_t k, double eps, int32_t algo) {
    // (asynchronous only where nothing of the sweep's verdict is needed before returning: a whole-cloud handle never
    // repeats a pass for points it left out, and statistics are off)
    const bool async = ctx && ctx->async_mode && ctx->n > 0 && ctx->q_begin == 0 && ctx->q_end == ctx->n && ctx->slab_parts == 0 &&
                       !ctx->collect_stats;
    PCT_TRY(pct_begin_call(ctx, !async));
    if (async) return curvature_async(ctx, k, eps, algo);
    bool fit_by_row = false;
    for (int attempt = 0; attempt < 2; ++attempt) {
        bool again = false;
        PCT_TRY(fused_call(ctx, k, eps, algo, ctx->clock[0], &fit_by_row));
        PCT_TRY(finish_knn_stats(ctx, ctx->clock[0], true, &again));
        if (!again) break;
        retry_without_cull(ctx);
    }
    ctx->tm.fit_svd_rows = ctx->pin->svd_rows[0];
    ctx->tm_done = ctx->tm;
    return fit_left(ctx, ctx->q_end - ctx->q_begin, true, fit_by_row);
}

int pct_get_neighbors(pct_ctx* ctx, int64_t begin, int64_t end, int32_t* idx, float* dist, int32_t* count) {
    PCT_TRY(pct_begin_row_call(ctx, "pct_get_neighbors"));
    if (!ctx->res.has(PCT_R_TABLE)) return pct_fail(ctx, PCT_ERR_NO_NEIGHBORS, "no neighbour table");
    if (begin < ctx->q_begin || end > ctx->q_end || begin > end)
        return pct_fail(ctx, PCT_ERR_INVALID, "rows [%lld,%lld) outside the owned range [%lld,%lld)", (long long)begin,
                        (long long)end, (long long)ctx->q_begin, (long long)ctx->q_end);
    const int64_t rows = end - begin;
    if (rows == 0) return PCT_OK;
    const size_t cells = (size_t)rows * ctx->k;
    int *d_idx = nullptr, *d_cnt = nullptr;
    float* d_dist = nullptr;
    if (idx) PCT_TRY(pct_claim(ctx, cells, &d_idx));
    if (dist) PCT_TRY(pct_claim(ctx, cells, &d_dist));
    if (count) PCT_TRY(pct_claim(ctx, (size_t)rows, &d_cnt));
    PCT_HIP(ctx, hipEventRecord(ctx->ev[PCT_EV_IO_BEGIN], ctx->stream));
    PCT_TRY(pct_launch_export_neighbors(ctx, begin, end, d_idx, d_dist, d_cnt));
    PCT_HIP(ctx, hipEventRecord(ctx->ev[PCT_EV_IO_END], ctx->stream));
    const pct_column cols[] = {{d_idx, ctx->k * (int)sizeof(int), idx}, {d_dist, ctx->k * (int)sizeof(float), dist}, {d_cnt, sizeof(int), count}};
    PCT_TRY(pct_download_columns(ctx, cols, 3, 0, rows, nullptr));
    ctx->tm.export_ms = pct_ev_ms(ctx, PCT_EV_IO_BEGIN, PCT_EV_IO_END);
    return PCT_OK;
}

int pct_get_neighbor_rows(pct_ctx* ctx, const int64_t* rows, int64_t n_rows, int32_t* idx, float* dist, int32_t* count) {
    PCT_TRY(pct_begin_row_call(ctx, "pct_get_neighbor_rows"));
    if (!ctx->res.has(PCT_R_TABLE)) return pct_fail(ctx, PCT_ERR_NO_NEIGHBORS, "no neighbour table");
    if (!rows || n_rows <= 0) return pct_fail(ctx, PCT_ERR_INVALID, "bad row list");
    for (int64_t i = 0; i < n_rows; ++i)
        if (rows[i] < ctx->q_begin || rows[i] >= ctx->q_end)
            return pct_fail(ctx, PCT_ERR_INVALID, "row %lld outside the owned range", (long long)rows[i]);
    const size_t cells = (size_t)n_rows * ctx->k;
    int64_t* d_rows = nullptr;
    int *d_idx = nullptr, *d_cnt = nullptr;
    float* d_dist = nullptr;
    PCT_TRY(pct_claim_upload(ctx, rows, (size_t)n_rows, &d_rows));
    if (idx) PCT_TRY(pct_claim(ctx, cells, &d_idx));
    if (dist) PCT_TRY(pct_claim(ctx, cells, &d_dist));
    if (count) PCT_TRY(pct_claim(ctx, (size_t)n_rows, &d_cnt));
    PCT_TRY(pct_launch_export_rows(ctx, d_rows, n_rows, d_idx, d_dist, d_cnt));
    const pct_column cols[] = {{d_idx, ctx->k * (int)sizeof(int), idx}, {d_dist, ctx->k * (int)sizeof(float), dist}, {d_cnt, sizeof(int), count}};
    return pct_download_columns(ctx, cols, 3, 0, n_rows, nullptr);
}

// validates host-supplied neighbour rows and stages them on the device, in claims that are the calling entry point's (no
// scope: they outlive this function): ids with a 16-byte row pitch, counts and query ids (null where the caller gave
// none); the public-order records are packed if they are not resident
struct StagedRows { int* idx; int* cnt; int64_t* query; int32_t pitch; };
static int stage_neighbour_rows(pct_ctx* ctx, const int32_t* idx, const int32_t* count, const int64_t* query, int64_t rows, int32_t k, StagedRows* out, bool need_pts4) {
    if (ctx->n <= 0) return pct_fail(ctx, PCT_ERR_INVALID, "no cloud loaded");
    if (!idx || rows <= 0 || k < 1 || k > 4096) return pct_fail(ctx, PCT_ERR_INVALID, "bad neighbour rows");
    // host-side validation: the reference raises IndexError on such rows (pct:640).  PCT_TRUST_ROWS=1 skips it (test
    // hook for the kernel's own guard: an entry outside the cloud is clamped there and the row reads NaN)
    const bool trust = pct_getenv("PCT_TRUST_ROWS") != nullptr;
    for (int64_t r = 0; r < rows && !trust; ++r) {
        const int m = count ? count[r] : k;
        if (m < 0 || m > k) return pct_fail(ctx, PCT_ERR_INVALID, "row %lld: count %d outside [0,%d]", (long long)r, m, k);
        if (query && (query[r] < 0 || query[r] >= ctx->n)) return pct_fail(ctx, PCT_ERR_INVALID, "row %lld: query index out of range", (long long)r);
        if (!query && r >= ctx->n) return pct_fail(ctx, PCT_ERR_INVALID, "more rows than points and no query list");
        const int32_t* p = idx + r * k;
        for (int j = 0; j < m; ++j)
            if (p[j] < 0 || p[j] >= ctx->n)
                return pct_fail(ctx, PCT_ERR_INVALID, "row %lld: neighbour index %d out of range (IndexError in the reference)", (long long)r, p[j]);
    }
    if (need_pts4 && !ctx->pts4_valid) {
        float bbox[6];
        PCT_TRY(pct_pack_points(ctx, bbox));
    }
    // device rows are 16-byte aligned: pitch = k rounded up to a multiple of 4
    const int32_t pitch = (k + 3) & ~3;
    *out = StagedRows{nullptr, nullptr, nullptr, pitch};
    PCT_TRY(pct_claim(ctx, (size_t)rows * pitch, &out->idx));
    PCT_HIP(ctx, hipMemcpy2DAsync(out->idx, (size_t)pitch * sizeof(int), idx, (size_t)k * sizeof(int),
                                  (size_t)k * sizeof(int), (size_t)rows, hipMemcpyHostToDevice, ctx->stream));
    if (count) PCT_TRY(pct_claim_upload(ctx, count, (size_t)rows, &out->cnt));
    if (query) PCT_TRY(pct_claim_upload(ctx, query, (size_t)rows, &out->query));
    return PCT_OK;
}

int pct_fit_indices(pct_ctx* ctx, const int32_t* idx, const int32_t* count, const int64_t* query, int64_t rows, int32_t k) {
    PCT_TRY(pct_begin_row_call(ctx, "pct_fit_indices"));
    StagedRows in;
    PCT_TRY(stage_neighbour_rows(ctx, idx, count, query, rows, k, &in, true));
    PCT_TRY(pct_reserve_fit(ctx, rows));
    PCT_HIP(ctx, hipEventRecord(ctx->ev[PCT_EV_FIT_BEGIN], ctx->stream));
    PCT_TRY(pct_launch_fit_rows(ctx, in.idx, in.cnt, in.query, rows, k, in.pitch, (float*)ctx->coefs.p,
                                (float*)ctx->K.p, (float*)ctx->H.p, (float*)ctx->H2.p, false));
    PCT_HIP(ctx, hipEventRecord(ctx->ev[PCT_EV_FIT_END], ctx->stream));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->tm.fit_ms = pct_ev_ms(ctx, PCT_EV_FIT_BEGIN, PCT_EV_FIT_END);
    ctx->tm.fit_svd_rows = ctx->pin->svd_rows[0];
    return fit_left(ctx, rows, false, false);         // (a resident neighbour table is untouched and stays valid)
}

int pct_fit_indices_f64(pct_ctx* ctx, const int32_t* idx, const int32_t* count, const int64_t* query, int64_t rows, int32_t k,
                        double* coefs, double* K, double* H) {
    PCT_TRY(pct_begin_call(ctx));
    if (!coefs || !K || !H) return pct_fail(ctx, PCT_ERR_INVALID, "output arrays missing");
    StagedRows in;
    PCT_TRY(stage_neighbour_rows(ctx, idx, count, query, rows, k, &in, false));
    double* d_c = nullptr;           // one claim: coefs (rows, 6) | K | H
    PCT_TRY(pct_claim(ctx, (size_t)rows * 8, &d_c));
    double* d_K = d_c + rows * 6;
    double* d_H = d_K + rows;
    PCT_TRY(pct_launch_fit_rows_f64(ctx, in.idx, in.cnt, in.query, rows, k, in.pitch, d_c, d_K, d_H));
    const pct_column cols[] = {{d_c, 6 * sizeof(double), coefs}, {d_K, sizeof(double), K}, {d_H, sizeof(double), H}};
    return pct_download_columns(ctx, cols, 3, 0, rows, nullptr);       // the resident float32 results and the neighbour table are untouched
}

// ---- queries of caller-supplied points: what pct_query_points, pct_query_points_algo and pct_query_ball share ----------------
// What query_route and ball_route (pct_query_plan.h, pct_ball_plan.h) are told of the handle.  The only place that reads
// these fields for routing: a wrong reroute is a rebuild that invalidates what is resident in the cell order -- which
// results those are is kept where they are left (pct_residents::leave), not listed here.
static QueryState query_state(const pct_ctx* ctx) {
    const pct_grid& g = ctx->grid;
    bool finite_limits = false;
    for (int a = 0; a < 3; ++a) finite_limits = finite_limits || isfinite(g.lim_lo[a]) || isfinite(g.lim_hi[a]);
    QueryState qs = {};
    qs.uniform_resident = ctx->grid_valid && ctx->grid_whole && !finite_limits;
    qs.tree_resident = tree_table_resident(ctx);
    qs.sorted_resident = ctx->res.any_in_cell_order();
    qs.sharded = ctx->q_begin != 0 || ctx->q_end != ctx->n;      // (a culled list in place: finite limits, not uniform_resident)
    qs.slab = ctx->slab_parts >= 1;
    return qs;
}

// The caller's arrays, in the two steps every entry takes them in: a cloud and the arrays themselves before the entry's
// own arguments (others: whatever else the entry needs besides the m queries is there) ...
static int check_query_arrays(pct_ctx* ctx, const double* q_xyz, int64_t m, bool others) {
    if (ctx->n <= 0 || !ctx->xyz_view) return pct_fail(ctx, PCT_ERR_INVALID, "no cloud loaded");
    if (m < 0 || !others || (m > 0 && !q_xyz)) return pct_fail(ctx, PCT_ERR_INVALID, "bad query arrays");
    return PCT_OK;
}
// ... and their values after them, once the call is known to read any
static int check_queries_finite(pct_ctx* ctx, const double* q_xyz, int64_t m) {
    for (int64_t i = 0; i < 3 * m; ++i)
        if (!isfinite(q_xyz[i])) return pct_fail(ctx, PCT_ERR_NONFINITE, "query point %lld is not finite", (long long)(i / 3));
    return PCT_OK;
}

// QueryRoute::GridBuild for the entry `who`: an ordinary resident cell list afterwards, sized as the cloud's own sweep
// would size it for rows of kb.  Nothing resident is disturbed: the route builds only where no table or result in place
// refers to the cell order, and the timings of the call that produced the table in place stay what they were.
static int build_query_grid(pct_ctx* ctx, int32_t kb, const char* who) {
    if ((int64_t)kb + 1 > ctx->n) kb = ctx->n > 1 ? (int32_t)ctx->n - 1 : 1;
    const pct_timings keep = ctx->tm;
    GridVerdict built;
    const int st = pct_build_grid(ctx, kb, 0.0, false, &built, nullptr, nullptr);
    ctx->tm = keep;
    ctx->counters_clean = false;       // (the words the build cleared belong to no sweep of this call)
    if (st != PCT_OK) return st;       // (every refusal of the build is the caller's to see: none is turned into another route)
    if (!(ctx->grid_valid && ctx->grid_whole))
        return pct_fail(ctx, PCT_ERR_INVALID, "%s: the cell list built is not one list over the whole cloud", who);
    return PCT_OK;
}

// The k nearest of m caller-supplied points.  algo names the path: the exhaustive sweep (pct_knn.hip) or the uniform cell
// list (pct_query.hip), by query_route's rule.  algo == nullptr is pct_query_points: the sweep whatever is resident, so
// never a list built, and query_stats stay those of the last pct_query_points_algo call.
static int query_points(pct_ctx* ctx, const char* who, const double* q_xyz, int64_t m, int32_t k, double eps, const int32_t* algo,
                        int32_t* idx, double* dist) {
    PCT_TRY(pct_begin_row_call(ctx, who));
    PCT_TRY(check_query_arrays(ctx, q_xyz, m, m == 0 || (idx && dist)));
    if (k < 1 || k > 128) return pct_fail(ctx, PCT_ERR_INVALID, "k=%d outside [1,128]", k);
    QueryRoute route = QueryRoute::Sweep;
    if (algo) {
        if (!query_route(*algo, ctx->n, m, k, query_state(ctx), &route)) return pct_fail(ctx, PCT_ERR_INVALID, "unknown query algorithm %d", *algo);
        for (int i = 0; i < 4; ++i) ctx->query_stats[i] = 0;
    }
    if (m == 0) return PCT_OK;
    PCT_TRY(check_queries_finite(ctx, q_xyz, m));
    if (!(eps >= 0) || isinf(eps)) eps = 0;
    // (two list registers at the most: the occupancy rule of longer rows is the exact-only sweep's)
    if (route == QueryRoute::GridBuild) PCT_TRY(build_query_grid(ctx, k < 127 ? k : 127, who));
    double *d_q = nullptr, *d_dist = nullptr;
    int32_t* d_idx = nullptr;
    PCT_TRY(pct_claim_upload(ctx, q_xyz, (size_t)m * 3, &d_q));
    PCT_TRY(pct_claim(ctx, (size_t)m * k, &d_idx));
    PCT_TRY(pct_claim(ctx, (size_t)m * k, &d_dist));
    if (route == QueryRoute::Sweep)
        PCT_TRY(pct_launch_query_points(ctx, d_q, m, k, eps, d_idx, d_dist));
    else
        PCT_TRY(pct_launch_query_grid(ctx, d_q, m, k, eps, d_idx, d_dist, ctx->query_words));
    PCT_TRY(pct_enqueue_download(ctx, idx, d_idx, (size_t)m * k));
    PCT_TRY(pct_enqueue_download(ctx, dist, d_dist, (size_t)m * k));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (algo) ctx->query_stats[0] = (int64_t)route;
    if (route != QueryRoute::Sweep) {
        const int64_t redone = ctx->query_words[1];
        ctx->query_stats[1] = m - redone;
        ctx->query_stats[2] = redone;
        ctx->query_stats[3] = ctx->query_words[2] > 1 ? ctx->query_words[2] : 1;     // (the 27 cells of stage 2 are ring 1)
    }
    return PCT_OK;
}

int pct_query_points(pct_ctx* ctx, const double* q_xyz, int64_t m, int32_t k, double eps, int32_t* idx, double* dist) {
    return query_points(ctx, "pct_query_points", q_xyz, m, k, eps, nullptr, idx, dist);
}

int pct_query_points_algo(pct_ctx* ctx, const double* q_xyz, int64_t m, int32_t k, double eps, int32_t algo, int32_t* idx, double* dist) {
    return query_points(ctx, "pct_query_points_algo", q_xyz, m, k, eps, &algo, idx, dist);
}

int pct_query_stats(pct_ctx* ctx, int64_t out[4]) {
    if (!ctx || !out) return PCT_ERR_INVALID;
    for (int i = 0; i < 4; ++i) out[i] = ctx->query_stats[i];
    return PCT_OK;
}

// Radius search (pct_ball.hip).  The route is ball_route's (pct_ball_plan.h), from the same state query_points reads.
int pct_query_ball(pct_ctx* ctx, const double* q_xyz, int64_t m, const double* r, int64_t n_r, int32_t flags, int32_t algo,
                   int64_t max_entries, int64_t* offsets) {
    PCT_TRY(pct_begin_row_call(ctx, "pct_query_ball"));
    PCT_TRY(check_query_arrays(ctx, q_xyz, m, offsets && (m == 0 || r)));
    if (m > 0 && n_r != 1 && n_r != m) return pct_fail(ctx, PCT_ERR_INVALID, "%lld radii for %lld queries (one, or one per query)", (long long)n_r, (long long)m);
    if (flags & ~(PCT_BALL_SORTED | PCT_BALL_DISTANCES | PCT_BALL_COUNT_ONLY)) return pct_fail(ctx, PCT_ERR_INVALID, "unknown flags %d", flags);
    QueryRoute route;
    if (!ball_route(algo, ctx->n, m, query_state(ctx), &route)) return pct_fail(ctx, PCT_ERR_INVALID, "unknown query algorithm %d", algo);
    PCT_TRY(check_queries_finite(ctx, q_xyz, m));
    if (m > 0 && route == QueryRoute::GridBuild) PCT_TRY(build_query_grid(ctx, 30, "pct_query_ball"));      // (rows of 30: the cloud's usual sweep)
    ctx->res.drop(pct_replacing(PCT_R_BALL));  // the request is accepted and its cell list stands: whatever was resident is the previous call's
    for (int i = 0; i < 4; ++i) ctx->ball_stats[i] = 0;
    offsets[0] = 0;
    if (m > 0) {
        double *d_q = nullptr, *d_r = nullptr;
        PCT_TRY(pct_claim_upload(ctx, q_xyz, (size_t)m * 3, &d_q));
        PCT_TRY(pct_claim_upload(ctx, r, (size_t)n_r, &d_r));
        ctx->ball_stats[0] = (int64_t)route;
        PCT_TRY(pct_launch_ball(ctx, route != QueryRoute::Sweep, d_q, m, d_r, n_r == m && m > 1 ? 1 : 0, flags, max_entries, offsets,
                                ctx->ball_stats + 1));
    }
    if (flags & PCT_BALL_COUNT_ONLY) return PCT_OK;        // (nothing is kept)
    ctx->ball_has_dist = (flags & PCT_BALL_DISTANCES) != 0;
    ctx->res.leave(PCT_R_BALL, false, m);
    return PCT_OK;
}

int pct_get_ball(pct_ctx* ctx, int64_t row_begin, int64_t row_end, int32_t* idx, double* dist) {
    PCT_TRY(pct_begin_call(ctx));
    if (!ctx->res.has(PCT_R_BALL)) return pct_fail(ctx, PCT_ERR_INVALID, "no ball rows on this handle (pct_query_ball)");
    const int64_t have = ctx->res.rows_of(PCT_R_BALL);
    if (row_begin < 0 || row_end > have || row_begin > row_end)
        return pct_fail(ctx, PCT_ERR_INVALID, "bad row range [%lld,%lld) of %lld", (long long)row_begin, (long long)row_end, (long long)have);
    if (dist && !ctx->ball_has_dist) return pct_fail(ctx, PCT_ERR_INVALID, "pct_get_ball: no distances were asked for (PCT_BALL_DISTANCES)");
    if (row_begin == row_end) return PCT_OK;
    int64_t ends[2] = {0, 0};
    const int64_t* d_off = (const int64_t*)ctx->ball_off.p;
    PCT_HIP(ctx, hipMemcpyAsync(&ends[0], d_off + row_begin, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    PCT_HIP(ctx, hipMemcpyAsync(&ends[1], d_off + row_end, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int64_t count = ends[1] - ends[0];
    if (count <= 0) return PCT_OK;
    if (!idx) return pct_fail(ctx, PCT_ERR_INVALID, "null output");
    PCT_HIP(ctx, hipMemcpyAsync(idx, (const int32_t*)ctx->ball_idx.p + ends[0], (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (dist) PCT_HIP(ctx, hipMemcpyAsync(dist, (const double*)ctx->ball_dist.p + ends[0], (size_t)count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PCT_OK;
}

// Fit of the resident ball rows about their centres (pct_fit_ball.hip).  Like pct_fit_indices it replaces the results of an
// earlier fit and nothing else: the rows, a resident neighbour table, PCA results and the cell list stay as they are.
int pct_fit_ball(pct_ctx* ctx, const int64_t* self_rows, int64_t m, int32_t* used) {
    PCT_TRY(pct_begin_row_call(ctx, "pct_fit_ball"));
    if (!ctx->res.has(PCT_R_BALL)) return pct_fail(ctx, PCT_ERR_NO_NEIGHBORS, "pct_fit_ball: no ball rows on this handle (pct_query_ball)");
    if (m != ctx->res.rows_of(PCT_R_BALL))
        return pct_fail(ctx, PCT_ERR_INVALID, "pct_fit_ball: %lld centres for the %lld rows of the last query", (long long)m, (long long)ctx->res.rows_of(PCT_R_BALL));
    if (m > 0 && !self_rows) return pct_fail(ctx, PCT_ERR_INVALID, "pct_fit_ball: null centres");
    for (int64_t i = 0; i < m; ++i)
        if (self_rows[i] < 0 || self_rows[i] >= ctx->n)
            return pct_fail(ctx, PCT_ERR_INVALID, "pct_fit_ball: row %lld: centre %lld outside the cloud", (long long)i, (long long)self_rows[i]);
    ctx->tm.fit_ms = 0;
    ctx->tm.fit_svd_rows = 0;
    if (m == 0) return fit_left(ctx, 0, false, false);
    ctx->res.drop(pct_replacing(PCT_R_FIT));   // accepted: the fit before this one is gone, the new one is there once the kernels have run
    PCT_TRY(pct_reserve_fit(ctx, m));
    int *d_self = nullptr, *d_used = nullptr;
    const std::vector<int> self32(self_rows, self_rows + m);
    PCT_TRY(pct_claim_upload(ctx, self32.data(), self32.size(), &d_self));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));               // (the copy is done before the temporary dies, whichever way)
    PCT_TRY(pct_claim(ctx, (size_t)m, &d_used));
    PCT_HIP(ctx, hipEventRecord(ctx->ev[PCT_EV_FIT_BEGIN], ctx->stream));
    PCT_TRY(pct_launch_fit_ball(ctx, d_self, m, d_used));
    PCT_HIP(ctx, hipEventRecord(ctx->ev[PCT_EV_FIT_END], ctx->stream));
    PCT_TRY(pct_enqueue_download(ctx, used, d_used, (size_t)m));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->tm.fit_ms = pct_ev_ms(ctx, PCT_EV_FIT_BEGIN, PCT_EV_FIT_END);
    ctx->tm.fit_svd_rows = ctx->pin->svd_rows[0];
    return fit_left(ctx, m, false, false);
}

int pct_ball_stats(pct_ctx* ctx, int64_t out[4]) {
    if (!ctx || !out) return PCT_ERR_INVALID;
    for (int i = 0; i < 4; ++i) out[i] = ctx->ball_stats[i];
    return PCT_OK;
}

int pct_get_fit(pct_ctx* ctx, int64_t begin, int64_t end, float* coefs, float* K, float* H, float* H2) {
    PCT_TRY(pct_begin_row_call(ctx, "pct_get_fit"));
    if (!ctx->res.has(PCT_R_FIT)) return pct_fail(ctx, PCT_ERR_INVALID, "no fit results");
    const int64_t base = ctx->fit_cloud_aligned ? ctx->q_begin : 0;   // cloud-aligned vs row-aligned results
    PCT_TRY(pct_check_owned_span(ctx, "the fitted range", PCT_R_FIT, begin, end, base));
    const pct_column cols[] = {{ctx->coefs.p, 6 * sizeof(float), coefs}, {ctx->K.p, sizeof(float), K}, {ctx->H.p, sizeof(float), H},
                               {ctx->H2.p, sizeof(float), H2}};
    return pct_get_rows(ctx, PCT_R_FIT, cols, 4, begin - base, end - begin);
}

int pct_curvatures_from_coefficients(pct_ctx* ctx, const float* coefs, int64_t rows, float* K, float* H, float* H2) {
    PCT_TRY(pct_begin_call(ctx));
    if (!coefs || rows <= 0) return pct_fail(ctx, PCT_ERR_INVALID, "bad coefficient rows");
    float *d_coefs = nullptr, *d_out = nullptr;
    PCT_TRY(pct_claim_upload(ctx, coefs, (size_t)rows * 6, &d_coefs));
    PCT_TRY(pct_claim(ctx, (size_t)rows * 3, &d_out));
    PCT_TRY(pct_launch_curvatures(ctx, d_coefs, rows, d_out, d_out + rows, d_out + 2 * rows));
    const pct_column cols[] = {{d_out, sizeof(float), K}, {d_out + rows, sizeof(float), H}, {d_out + 2 * rows, sizeof(float), H2}};
    return pct_download_columns(ctx, cols, 3, 0, rows, nullptr);
}

int pct_plane_rotate(pct_ctx* ctx, const void* nbrs, int32_t is_f64, int64_t batch, int32_t m, double* rotated) {
    PCT_TRY(pct_begin_call(ctx));
    if (!nbrs || !rotated || batch <= 0 || m < 2 || (double)batch * m > 2.0e9) return pct_fail(ctx, PCT_ERR_INVALID, "bad neighbourhood block");
    const size_t count = (size_t)batch * m * 3, esz = is_f64 ? sizeof(double) : sizeof(float);
    if (is_f64) { const double* p = (const double*)nbrs; for (size_t i = 0; i < count; ++i) if (!isfinite(p[i])) return pct_fail(ctx, PCT_ERR_NONFINITE, "Non-finite values in input points"); }
    else { const float* p = (const float*)nbrs; for (size_t i = 0; i < count; ++i) if (!isfinite(p[i])) return pct_fail(ctx, PCT_ERR_NONFINITE, "Non-finite values in input points"); }
    char* d_nbrs = nullptr;          // (bytes: float or double)
    double* d_rot = nullptr;
    PCT_TRY(pct_claim_upload(ctx, (const char*)nbrs, count * esz, &d_nbrs));
    PCT_TRY(pct_claim(ctx, count, &d_rot));
    PCT_TRY(pct_launch_plane_rotate(ctx, d_nbrs, is_f64 != 0, batch, m, d_rot));
    PCT_TRY(pct_enqueue_download(ctx, rotated, d_rot, count));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PCT_OK;
}

int pct_fit_quadric(pct_ctx* ctx, const float* pts, int64_t batch, int32_t m, float* coefs) {
    PCT_TRY(pct_begin_call(ctx));
    if (!pts || !coefs || batch <= 0 || m < 1 || (double)batch * m > 2.0e9) return pct_fail(ctx, PCT_ERR_INVALID, "bad point block");
    const size_t count = (size_t)batch * m * 3;
    for (size_t i = 0; i < count; ++i)
        if (!isfinite(pts[i])) return pct_fail(ctx, PCT_ERR_NONFINITE, "Input contains non-finite values.");
    float *d_pts = nullptr, *d_coefs = nullptr;
    PCT_TRY(pct_claim_upload(ctx, pts, count, &d_pts));
    PCT_TRY(pct_claim(ctx, (size_t)batch * 6, &d_coefs));
    PCT_TRY(pct_launch_quadric_rows(ctx, d_pts, batch, m, d_coefs));
    PCT_TRY(pct_enqueue_download(ctx, coefs, d_coefs, (size_t)batch * 6));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PCT_OK;
}

int pct_neighbor_study_curvatures(pct_ctx* ctx, const int64_t* sample_rows, int64_t n_samples, int32_t n_lo, int32_t n_hi,
                                   float* K_out) {
    PCT_TRY(pct_begin_row_call(ctx, "pct_neighbor_study_curvatures"));
    if (!ctx->res.has(PCT_R_TABLE)) return pct_fail(ctx, PCT_ERR_NO_NEIGHBORS, "plant the neighbour table first (pct_knn)");
    if (!sample_rows || !K_out || n_samples <= 0 || n_lo < 1 || n_hi < n_lo) return pct_fail(ctx, PCT_ERR_INVALID, "bad study arguments");
    if (n_hi > ctx->k) return pct_fail(ctx, PCT_ERR_INVALID, "the study needs %d neighbours per point, the table holds %d", n_hi, ctx->k);
    if (ctx->eps > 0) return pct_fail(ctx, PCT_ERR_INVALID, "the study needs a plain k-NN table (no eps bound)");
    const int nn = n_hi - n_lo + 1;
    const int64_t rows = n_samples * nn;
    if (rows > (int64_t)1 << 30) return pct_fail(ctx, PCT_ERR_INVALID, "study too large");
    // sample rows -> positions in the order the table is indexed by
    std::vector<int> h_pos((size_t)n_samples);
    for (int64_t i = 0; i < n_samples; ++i) {
        if (sample_rows[i] < ctx->q_begin || sample_rows[i] >= ctx->q_end)
            return pct_fail(ctx, PCT_ERR_INVALID, "sample row %lld outside the owned range", (long long)sample_rows[i]);
        h_pos[(size_t)i] = (int)(sample_rows[i] - ctx->q_begin);    // exhaustive table: that is the row; grid table: index into row_of
    }
    const int32_t pitch = (n_hi + 1 + 3) & ~3;
    int *d_spos = nullptr, *d_table = nullptr, *d_cnt = nullptr;
    int64_t* d_row_query = nullptr;
    PCT_TRY(pct_claim_upload(ctx, h_pos.data(), h_pos.size(), &d_spos));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));               // (the copy is done before the temporary dies, whichever way)
    PCT_TRY(pct_claim(ctx, (size_t)rows * pitch, &d_table));
    PCT_TRY(pct_claim(ctx, (size_t)rows * 10, &d_cnt));             // one claim: counts (rows) | coefs (rows, 6), K, H, H2 as float
    PCT_TRY(pct_claim(ctx, (size_t)rows, &d_row_query));
    if (ctx->knn_sorted_space) {      // public index -> neighbour-table row, on the device
        PCT_TRY(pct_ensure_row_of(ctx));
        PCT_TRY(pct_launch_gather_int(ctx, (const int*)ctx->row_of.p, d_spos, n_samples));
    }
    static_assert(sizeof(int) == sizeof(float), "the packed claim counts both as four-byte words");
    float* d_out = (float*)(d_cnt + rows);            // coefs (rows,6), K, H, H2
    PCT_TRY(pct_launch_prefix_rows(ctx, d_spos, n_samples, n_lo, n_hi, d_table, pitch, d_cnt, d_row_query));
    PCT_TRY(pct_launch_fit_rows(ctx, d_table, d_cnt, d_row_query, rows, n_hi + 1, pitch, d_out, d_out + rows * 6, d_out + rows * 7,
                                d_out + rows * 8, ctx->knn_sorted_space));
    PCT_TRY(pct_enqueue_download(ctx, K_out, (const float*)(d_out + rows * 6), (size_t)rows));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PCT_OK;
}

int pct_mesh_energies(pct_ctx* ctx, const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                      const void* gaussian, const void* mean, int32_t curvature_is_f64, double* out3) {
    PCT_TRY(pct_begin_call(ctx));
    if (!vertices || !triangles || !gaussian || !mean || !out3 || n_vertices <= 0 || n_triangles < 0 || curvature_is_f64 < 0 ||
        curvature_is_f64 > PCT_MESH_K32_H64)
        return pct_fail(ctx, PCT_ERR_INVALID, "bad mesh arguments");
    out3[0] = out3[1] = out3[2] = 0.0;
    if (n_triangles == 0) return PCT_OK;                               // utils.py:719-721: zeros
    for (int64_t i = 0; i < 3 * n_triangles; ++i)
        if (triangles[i] < 0 || triangles[i] >= n_vertices)
            return pct_fail(ctx, PCT_ERR_INVALID, "triangle %lld refers to vertex %d outside [0,%lld)", (long long)(i / 3), triangles[i], (long long)n_vertices);
    const bool k_f64 = curvature_is_f64 == PCT_MESH_F64 || curvature_is_f64 == PCT_MESH_K64_H32;
    const bool h_f64 = curvature_is_f64 == PCT_MESH_F64 || curvature_is_f64 == PCT_MESH_K32_H64;
    const size_t ksz = (size_t)n_vertices * (k_f64 ? sizeof(double) : sizeof(float));
    const size_t hsz = (size_t)n_vertices * (h_f64 ? sizeof(double) : sizeof(float));
    const size_t h_at = (size_t)n_vertices * sizeof(double);          // H behind room for a float64 K: aligned whatever K is
    const int nblk = (int)((n_triangles + 255) / 256 < 1024 ? (n_triangles + 255) / 256 : 1024);
    double *d_v = nullptr, *d_part = nullptr;
    int32_t* d_tri = nullptr;
    char* d_kh = nullptr;            // one claim: K | H at h_at
    PCT_TRY(pct_claim_upload(ctx, vertices, (size_t)n_vertices * 3, &d_v));
    PCT_TRY(pct_claim_upload(ctx, triangles, (size_t)n_triangles * 3, &d_tri));
    PCT_TRY(pct_claim(ctx, h_at + hsz, &d_kh));
    PCT_TRY(pct_claim(ctx, (size_t)nblk * 3 + 3, &d_part));
    PCT_HIP(ctx, hipMemcpyAsync(d_kh, gaussian, ksz, hipMemcpyHostToDevice, ctx->stream));
    PCT_HIP(ctx, hipMemcpyAsync(d_kh + h_at, mean, hsz, hipMemcpyHostToDevice, ctx->stream));
    PCT_TRY(pct_launch_mesh_energies(ctx, d_v, d_tri, n_triangles, d_kh, d_kh + h_at, k_f64, h_f64, d_part, nblk, d_part + (size_t)nblk * 3));
    PCT_TRY(pct_enqueue_download(ctx, out3, d_part + (size_t)nblk * 3, 3));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PCT_OK;
}

static int voxel_downsample(pct_ctx* ctx, const void* xyz, bool f64, int64_t n, double voxel_size, int64_t* indices, int64_t* count) {
    PCT_TRY(pct_begin_call(ctx));
    if (!xyz || !indices || !count || n <= 0 || n >= 0x7F000000 || !(voxel_size > 0) || (!f64 && !((float)voxel_size > 0.f)))
        return pct_fail(ctx, PCT_ERR_INVALID, "bad down-sampling arguments");
    for (int64_t i = 0; i < 3 * n; ++i) {
        const double v = f64 ? ((const double*)xyz)[i] : (double)((const float*)xyz)[i];
        if (!isfinite(v) || fabs(v / voxel_size) >= 2147483000.0)
            return pct_fail(ctx, PCT_ERR_INVALID, "coordinate %lld does not map to an int32 voxel index", (long long)(i / 3));
    }
    const size_t bytes = (size_t)n * 3 * (f64 ? sizeof(double) : sizeof(float));
    char* d_xyz = nullptr;           // (bytes: float or double)
    int64_t* d_kept = nullptr;
    PCT_TRY(pct_claim_upload(ctx, (const char*)xyz, bytes, &d_xyz));
    PCT_TRY(pct_claim(ctx, (size_t)n, &d_kept));
    PCT_TRY(pct_voxel_downsample_device(ctx, d_xyz, f64, n, voxel_size, d_kept, count));
    if (*count > 0) PCT_TRY(pct_enqueue_download(ctx, indices, d_kept, (size_t)*count));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PCT_OK;
}

int pct_voxel_downsample(pct_ctx* ctx, const double* xyz, int64_t n, double voxel_size, int64_t* indices, int64_t* count) {
    return voxel_downsample(ctx, xyz, true, n, voxel_size, indices, count);
}

int pct_voxel_downsample_f32(pct_ctx* ctx, const float* xyz, int64_t n, double voxel_size, int64_t* indices, int64_t* count) {
    return voxel_downsample(ctx, xyz, false, n, voxel_size, indices, count);
}

int pct_surface_variation(pct_ctx* ctx, int32_t k_total, float* out) {
    PCT_TRY(pct_begin_row_call(ctx, "pct_surface_variation"));
    if (!out || k_total < 2) return pct_fail(ctx, PCT_ERR_INVALID, "bad surface-variation arguments");
    const int64_t rows = ctx->q_end - ctx->q_begin;
    for (int attempt = 0; attempt < 2; ++attempt) {
        bool again = false;
        PCT_TRY(run_knn(ctx, k_total - 1, 0.0, PCT_KNN_AUTO, ctx->clock[0], PCT_CALL_SWEEP_HEAD));        // k-1 neighbours + the point itself (utils.py:812-814)
        PCT_TRY(pct_reserve(ctx, &ctx->K, (size_t)rows * sizeof(float)));
        PCT_TRY(pct_launch_surface_variation(ctx, (float*)ctx->K.p));
        PCT_HIP(ctx, hipMemcpyAsync(out, ctx->K.p, (size_t)rows * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        PCT_TRY(finish_knn_stats(ctx, ctx->clock[0], false, &again));
        if (!again) break;
        retry_without_cull(ctx);
    }
    return PCT_OK;                     // (no fit: the planting dropped it, ctx->K holds the variation)
}

int pct_pca_curvatures(pct_ctx* ctx, int32_t k, int32_t algo, int32_t keep_neighbors, int64_t* exact_rows) {
    PCT_TRY(pct_begin_row_call(ctx, "pct_pca_curvatures"));
    if (ctx->n <= 0) return pct_fail(ctx, PCT_ERR_INVALID, "no cloud loaded");
    if (ctx->q_begin != 0 || ctx->q_end != ctx->n)
        return pct_fail(ctx, PCT_ERR_INVALID, "pct_pca_curvatures answers whole clouds (query range [%lld,%lld) of %lld points)",
                        (long long)ctx->q_begin, (long long)ctx->q_end, (long long)ctx->n);
    const int64_t kk = k < ctx->n - 1 ? k : ctx->n - 1;      // pct:916: argsort(...)[1:k+1] of N entries holds min(k, N-1)
    if (kk > PCT_K_MAX)
        return pct_fail(ctx, PCT_ERR_INVALID, "k=%d: the PCA estimator takes at most %d neighbours (the sweep's range)", k, PCT_K_MAX);
    if (kk < 2)      // np.cov of fewer than two points is NaN, and scipy.linalg.eigh refuses it
        return pct_fail(ctx, PCT_ERR_INVALID, "k=%d on %lld points leaves %lld neighbours: array must not contain infs or NaNs",
                        k, (long long)ctx->n, (long long)kk);
    ctx->res.drop(pct_replacing(PCT_R_PCA));
    double R = 0.0, origin[3] = {0, 0, 0};
    bool bad = false;
    // float64 clouds: from here until pct_pca_restore the handle's cloud is the recentred one the sweep ranks
    int st = pct_pca_prep(ctx, &R, &bad, origin);
    if (st == PCT_OK && bad) st = pct_fail(ctx, PCT_ERR_NONFINITE, "array must not contain infs or NaNs");
    const int64_t room = (PCT_K_MAX < ctx->n - 1 ? PCT_K_MAX : ctx->n - 1) - kk;
    const int32_t kc = (int32_t)(kk + (room < PCT_PCA_EXTRA ? room : PCT_PCA_EXTRA));
    bool again = false;
    if (st == PCT_OK) st = run_knn(ctx, kc, 0.0, algo, ctx->clock[0], PCT_CALL_SWEEP_HEAD);      // (the PCA kernels follow)
    if (st == PCT_OK) st = finish_knn_stats(ctx, ctx->clock[0], false, &again);     // (whole clouds: nothing was left out of the cell list)
    const int rs = pct_pca_restore(ctx);
    PCT_TRY(st);
    PCT_TRY(rs);
    PCT_HIP(ctx, hipEventRecord(ctx->ev[PCT_EV_FIT_BEGIN], ctx->stream));
    int64_t exact = 0;
    st = pct_launch_pca(ctx, (int32_t)kk, 2.0 * R * (1.0 + 1e-9), origin, keep_neighbors != 0, &exact);
    if (ctx->has_f64) ctx->grid_valid = false;        // (the cell list holds the recentred float32 cloud)
    ctx->res.drop(PCT_TABLE_AND_FIT_LOST);            // (the table in place holds the over-fetched candidates)
    PCT_TRY(st);
    PCT_HIP(ctx, hipEventRecord(ctx->ev[PCT_EV_FIT_END], ctx->stream));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->tm.fit_ms = pct_ev_ms(ctx, PCT_EV_FIT_BEGIN, PCT_EV_FIT_END);
    ctx->tm.total_ms = ctx->clock[0].since_begin(ctx->ev[PCT_EV_FIT_END]);
    ctx->res.leave(PCT_R_PCA, false, ctx->n);
    ctx->pca_has_nbr = keep_neighbors != 0;
    ctx->pca_k = (int32_t)kk;
    if (exact_rows) *exact_rows = exact;
    return PCT_OK;
}

int pct_get_pca(pct_ctx* ctx, int64_t begin, int64_t end, double* l1, double* l2, double* dirs, double* K, double* H,
                int32_t* idx) {
    PCT_TRY(pct_begin_call(ctx));
    if (!ctx->res.has(PCT_R_PCA)) return pct_fail(ctx, PCT_ERR_INVALID, "no PCA frame on this handle (pct_pca_curvatures)");
    const int64_t n = ctx->res.rows_of(PCT_R_PCA), rows = end - begin;
    if (begin < 0 || end > n || begin > end)
        return pct_fail(ctx, PCT_ERR_INVALID, "bad row range [%lld,%lld) of %lld", (long long)begin, (long long)end, (long long)n);
    if (idx && !ctx->pca_has_nbr)
        return pct_fail(ctx, PCT_ERR_INVALID, "pct_get_pca: the neighbourhoods were not kept (pct_pca_curvatures keep_neighbors)");
    if (rows == 0) return PCT_OK;
    const double* o = (const double*)ctx->pca.p;
    const pct_column cols[] = {{o, sizeof(double), l1}, {o + n, sizeof(double), l2}, {o + 2 * n, sizeof(double), K}, {o + 3 * n, sizeof(double), H},
                               {o + 4 * n, 6 * sizeof(double), dirs}, {ctx->pca_nbr.p, ctx->pca_k * (int)sizeof(int32_t), idx}};
    PCT_HIP(ctx, hipEventRecord(ctx->ev[PCT_EV_IO_BEGIN], ctx->stream));
    PCT_TRY(pct_enqueue_columns(ctx, cols, 6, begin, rows, nullptr));
    PCT_HIP(ctx, hipEventRecord(ctx->ev[PCT_EV_IO_END], ctx->stream));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->tm.export_ms = pct_ev_ms(ctx, PCT_EV_IO_BEGIN, PCT_EV_IO_END);
    return PCT_OK;
}

int pct_timings_size(void) { return (int)sizeof(pct_timings); }

int pct_get_timings(const pct_ctx* ctx, pct_timings* out) {
    if (!ctx || !out) return PCT_ERR_INVALID;
    if (ctx->pend.on) {                    // (an asynchronous call: its times exist once its kernels have finished)
        pct_ctx* c = const_cast<pct_ctx*>(ctx);
        PCT_TRY(pct_begin_call(c));
    }
    *out = ctx->tm;
    return PCT_OK;
}

int pct_get_timings_done(const pct_ctx* ctx, pct_timings* out) {
    if (!ctx || !out) return PCT_ERR_INVALID;
    *out = ctx->pend.on ? ctx->tm_done : ctx->tm;
    return PCT_OK;
}

int pct_device_alloc(pct_ctx* ctx, int64_t bytes, void** dev_ptr) {
    PCT_TRY(pct_begin_call(ctx));
    if (!dev_ptr || bytes <= 0) return pct_fail(ctx, PCT_ERR_INVALID, "bad allocation request");
    hipError_t e = hipMalloc(dev_ptr, (size_t)bytes);
    if (e != hipSuccess) return pct_fail(ctx, PCT_ERR_OOM, "hipMalloc(%lld) failed: %s", (long long)bytes, hipGetErrorString(e));
    return PCT_OK;
}

int pct_device_free(pct_ctx* ctx, void* dev_ptr) {
    PCT_TRY(pct_begin_call(ctx));
    if (dev_ptr) PCT_HIP(ctx, hipFree(dev_ptr));
    return PCT_OK;
}

int pct_device_upload(pct_ctx* ctx, void* dev_dst, const void* host_src, int64_t bytes) {
    PCT_TRY(pct_begin_call(ctx));
    PCT_HIP(ctx, hipMemcpyAsync(dev_dst, host_src, (size_t)bytes, hipMemcpyHostToDevice, ctx->stream));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PCT_OK;
}

int pct_device_download(pct_ctx* ctx, void* host_dst, const void* dev_src, int64_t bytes) {
    PCT_TRY(pct_begin_call(ctx));
    PCT_HIP(ctx, hipMemcpyAsync(host_dst, dev_src, (size_t)bytes, hipMemcpyDeviceToHost, ctx->stream));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PCT_OK;
}

int pct_synchronize(pct_ctx* ctx) {
    PCT_TRY(pct_begin_call(ctx));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PCT_OK;
}

}  // extern "C"

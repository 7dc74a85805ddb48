// The self-test entry points of the C ABI (include/pct_hip.h: pct_selftest*): test scaffolding, not entry-point logic.  Host
// arrays in and out around the launchers the sweeps, the sorters and the chained sweep's planning run themselves.
#include "pct_internal.h"

#include <math.h>
#include <vector>

namespace {
// Device memory of a self-test's own, nothing of the handle's: exactly the sizes asked for, freed when the call returns,
// whichever way.  A host array handed to take() or downloaded to must outlive the call's wait for the stream.
struct DevScratch {
    pct_ctx* const ctx;
    std::vector<pct_buf> held;
    template <class T>                                 // count elements, filled from host where one is given
    int take(T** p, size_t count, const T* host = nullptr) {
        held.emplace_back();
        pct_buf& b = held.back();
        PCT_HIP(ctx, hipMalloc(&b.p, count * sizeof(T)));
        b.cap = count * sizeof(T);
        *p = (T*)b.p;
        if (host) PCT_HIP(ctx, hipMemcpyAsync(b.p, host, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        return PCT_OK;
    }
};
constexpr int64_t kSelftestMaxLists = 1 << 20;

// public indices as the records carry them: the .w word of a float4
std::vector<float4> pub_records(const int32_t* pub, int64_t n) {
    std::vector<float4> r((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        float w;
        memcpy(&w, &pub[i], 4);
        r[(size_t)i] = make_float4(0.f, 0.f, 0.f, w);
    }
    return r;
}
}  // namespace

extern "C" {

int pct_selftest(pct_ctx* ctx, int32_t* failures) {
    PCT_TRY(pct_begin_call(ctx));
    if (!failures) return pct_fail(ctx, PCT_ERR_INVALID, "null output");
    PCT_TRY(pct_reserve(ctx, &ctx->red, 64));
    PCT_HIP(ctx, hipMemsetAsync(ctx->red.p, 0, 64, ctx->stream));
    PCT_TRY(pct_launch_selftest(ctx, (int*)ctx->red.p));
    PCT_TRY(pct_enqueue_download(ctx, failures, (const int32_t*)ctx->red.p, 1));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PCT_OK;
}

// ---- self-tests of the sorters: host arrays in and out, device memory of their own, nothing of the handle's ---------------
int pct_selftest_sort(pct_ctx* ctx, int32_t network, const uint32_t* in, int64_t n_lists, uint32_t* out) {
    PCT_TRY(pct_begin_call(ctx));
    const int regs = pct_selftest_sort_regs(network);
    if (!regs) return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_sort: no network %d", (int)network);
    if (!in || !out) return pct_fail(ctx, PCT_ERR_INVALID, "null array");
    const bool two = network == PCT_NET_SETS1 || network == PCT_NET_SETS2 || network == PCT_NET_PAIR;
    if (n_lists < 1 || n_lists > kSelftestMaxLists || (two && (n_lists & 1)))
        return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_sort: n_lists = %lld (1 .. 2^20; even where a wave sorts two lists)", (long long)n_lists);
    const int n_waves = (int)(two ? n_lists / 2 : n_lists);
    const size_t count = (size_t)n_waves * 64 * regs;
    DevScratch mem{ctx};
    uint32_t *d_in, *d_out;
    PCT_TRY(mem.take(&d_in, count, in));
    PCT_TRY(mem.take(&d_out, count));
    PCT_TRY(pct_launch_selftest_sort(ctx, network, d_in, n_waves, d_out));
    PCT_TRY(pct_enqueue_download(ctx, out, d_out, count));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PCT_OK;
}

int pct_selftest_sort_exact(pct_ctx* ctx, int32_t regs, int32_t mode, const double* d2, const int32_t* pos, const double* batch_d2,
                            const int32_t* batch_pos, const int32_t* pub, int64_t n_pub, int64_t n_lists, double* out_d2, int32_t* out_pos) {
    PCT_TRY(pct_begin_call(ctx));
    if (regs != 1 && regs != 2 && regs != 4 && regs != 8) return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_sort_exact: list registers are 1, 2, 4 or 8, not %d", (int)regs);
    if (mode != PCT_EXACT_ASCENDING && mode != PCT_EXACT_DESCENDING && mode != PCT_EXACT_MERGE_MIN)
        return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_sort_exact: no mode %d", (int)mode);
    const bool merge = mode == PCT_EXACT_MERGE_MIN;
    if (!d2 || !pos || !pub || !out_d2 || !out_pos || (merge && (!batch_d2 || !batch_pos))) return pct_fail(ctx, PCT_ERR_INVALID, "null array");
    if (n_lists < 1 || n_lists > kSelftestMaxLists || n_pub < 1 || n_pub > (1 << 24)) return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_sort_exact: n_lists = %lld, n_pub = %lld", (long long)n_lists, (long long)n_pub);
    const size_t count = (size_t)n_lists * 64 * regs;
    // the kernels read pub[position] for tied elements: no position may point outside the table
    for (int pass = 0; pass < (merge ? 2 : 1); ++pass) {
        const int32_t* p = pass ? batch_pos : pos;
        for (size_t i = 0; i < count; ++i)
            if (p[i] != INT32_MAX && (p[i] < 0 || p[i] >= n_pub)) return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_sort_exact: position %d outside [0, n_pub)", (int)p[i]);
    }
    const std::vector<float4> rec = pub_records(pub, n_pub);
    DevScratch mem{ctx};
    double *d_d2, *d_bd2 = nullptr, *d_od2;
    int *d_pos, *d_bpos = nullptr, *d_opos;
    float4* d_pts;
    PCT_TRY(mem.take(&d_d2, count, d2));
    PCT_TRY(mem.take(&d_pos, count, pos));
    PCT_TRY(mem.take(&d_od2, count));
    PCT_TRY(mem.take(&d_opos, count));
    PCT_TRY(mem.take(&d_pts, rec.size(), rec.data()));
    if (merge) {
        PCT_TRY(mem.take(&d_bd2, count, batch_d2));
        PCT_TRY(mem.take(&d_bpos, count, batch_pos));
    }
    PCT_TRY(pct_launch_selftest_exact(ctx, regs, mode, d_d2, d_pos, d_bd2, d_bpos, d_pts, (int)n_lists, d_od2, d_opos));
    PCT_TRY(pct_enqueue_download(ctx, out_d2, d_od2, count));
    PCT_TRY(pct_enqueue_download(ctx, out_pos, d_opos, count));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));        // (rec and the scratch outlive every copy: waited for here)
    return PCT_OK;
}

int pct_selftest_order_keys(pct_ctx* ctx, int32_t regs, int32_t slot_bits, const uint32_t* elems, const double* d2, const int32_t* pub,
                            int64_t n_lists, uint32_t* out, int32_t* done) {
    PCT_TRY(pct_begin_call(ctx));
    if (!((regs == 1 && (slot_bits == 6 || slot_bits == 9)) || (regs == 2 && (slot_bits == 7 || slot_bits == 10))))
        return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_order_keys: (regs, slot_bits) is (1, 6), (1, 9), (2, 7) or (2, 10), not (%d, %d)", (int)regs, (int)slot_bits);
    if (!elems || !d2 || !pub || !out || !done) return pct_fail(ctx, PCT_ERR_INVALID, "null array");
    if (n_lists < 1 || n_lists > (1 << 16)) return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_order_keys: n_lists = %lld (1 .. 65536)", (long long)n_lists);
    const size_t count = (size_t)n_lists * 64 * regs, table = (size_t)n_lists << slot_bits;
    const std::vector<float4> rec = pub_records(pub, (int64_t)table);
    DevScratch mem{ctx};
    uint32_t *d_e, *d_out;
    double* d_d2;
    float4* d_pts;
    int* d_done;
    PCT_TRY(mem.take(&d_e, count, elems));
    PCT_TRY(mem.take(&d_out, count));
    PCT_TRY(mem.take(&d_d2, table, d2));
    PCT_TRY(mem.take(&d_pts, table, rec.data()));
    PCT_TRY(mem.take(&d_done, (size_t)n_lists));
    PCT_TRY(pct_launch_selftest_order(ctx, regs, slot_bits, d_e, d_d2, d_pts, (int)n_lists, d_out, d_done));
    PCT_TRY(pct_enqueue_download(ctx, out, d_out, count));
    PCT_TRY(pct_enqueue_download(ctx, done, d_done, (size_t)n_lists));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PCT_OK;
}

// ---- self-test of the planned fast sweep (tests/test_gpu_select.py): pct_knn's cell list, plan and one launch, no exact sweep ----
// Unlike the self-tests above this one works on the handle's cloud and in its buffers, its staging claims among them: the
// table it leaves is unfinished, so every resident result is dropped, as by a new cloud.
int pct_selftest_sweep(pct_ctx* ctx, int32_t k, double eps, int32_t algo, int32_t want_dist, int32_t* idx, float* dist, int32_t* count,
                       uint8_t* flags, double* info) {
    PCT_TRY(pct_begin_row_call(ctx, "pct_selftest_sweep"));
    if (!idx || !flags || !info) return pct_fail(ctx, PCT_ERR_INVALID, "null array");
    if (ctx->n <= 0) return pct_fail(ctx, PCT_ERR_INVALID, "no cloud loaded");
    if (algo != PCT_KNN_GRID) return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_sweep: PCT_KNN_GRID only, not algorithm %d", (int)algo);
    if (k < 1 || k > 127) return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_sweep: k=%d outside [1,127], the fast sweeps' rows", (int)k);
    if ((int64_t)k + 1 > ctx->n) return pct_fail(ctx, PCT_ERR_K_TOO_LARGE, "k+1=%d exceeds the cloud size %lld", k + 1, (long long)ctx->n);
    if (ctx->n > ((int64_t)1 << 24)) return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_sweep: at most 2^24 points");
    if (!(eps >= 0) || isinf(eps)) eps = 0;
    const int64_t rows = ctx->q_end - ctx->q_begin;
    if (rows <= 0) return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_sweep: no owned rows");
    ctx->res.drop(PCT_UNFINISHED_TABLE);
    ctx->k = k;
    ctx->eps = eps;
    pct_call_clock& clock = ctx->clock[0];
    PCT_TRY(clock.open(ctx, false, true, PCT_CALL_SWEEP_HEAD));
    PCT_HIP(ctx, clock.start(ctx->stream));
    ctx->tm.levels = 0;
    ctx->tm.sweep_variant = 0;
    ctx->tm.algo = algo;
    GridVerdict built;
    PCT_TRY(pct_build_grid(ctx, k, eps, false, &built, &clock, nullptr));
    if (built != GridVerdict::Built) return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_sweep: no cell list");
    PCT_HIP(ctx, clock.boundary(PCT_ST_GRID_END, ctx->stream));
    // the buffers the launcher reserves, reserved here at the same sizes and filled: a table of -1 (a row the sweep leaves
    // alone, or marks in its first column only, exports as empty) and a list of kNoEntry (what the sweep did not write shows)
    constexpr int kNoEntry = 0x7f7f7f7f;
    const size_t pitch = (size_t)((k + 3) & ~3), list_len = (size_t)rows + 16;
    PCT_TRY(pct_reserve(ctx, &ctx->nbr_pos, (size_t)rows * pitch * sizeof(int)));
    PCT_TRY(pct_reserve(ctx, &ctx->nbr_dist, (size_t)rows * pitch * sizeof(float)));
    PCT_TRY(pct_reserve(ctx, &ctx->nbr_cnt, (size_t)rows * sizeof(int)));
    PCT_TRY(pct_reserve(ctx, &ctx->redo, list_len * sizeof(int)));
    PCT_HIP(ctx, hipMemsetAsync(ctx->nbr_pos.p, 0xff, (size_t)rows * pitch * sizeof(int), ctx->stream));
    PCT_HIP(ctx, hipMemsetAsync(ctx->nbr_dist.p, 0xff, (size_t)rows * pitch * sizeof(float), ctx->stream));
    PCT_HIP(ctx, hipMemsetAsync(ctx->nbr_cnt.p, 0xff, (size_t)rows * sizeof(int), ctx->stream));
    PCT_HIP(ctx, hipMemsetAsync(ctx->redo.p, 0x7f, list_len * sizeof(int), ctx->stream));
    PCT_TRY(pct_launch_knn_grid(ctx, k, eps, false, 3, want_dist != 0, &clock, nullptr));
    PCT_HIP(ctx, clock.boundary(PCT_ST_SWEEP_END, ctx->stream));
    // the rows in public order, through the getter's own export
    const size_t cells = (size_t)rows * k;
    const bool dist_kept = ctx->dist_valid;
    PCT_TRY(pct_ensure_row_of(ctx));
    int *d_idx = nullptr, *d_cnt = nullptr;
    float* d_dist = nullptr;
    PCT_TRY(pct_claim(ctx, cells, &d_idx));
    if (dist && dist_kept) PCT_TRY(pct_claim(ctx, cells, &d_dist));
    if (count) PCT_TRY(pct_claim(ctx, (size_t)rows, &d_cnt));
    PCT_TRY(pct_launch_export_neighbors(ctx, ctx->q_begin, ctx->q_end, d_idx, d_dist, d_cnt));
    std::vector<int> list(list_len), row_of((size_t)rows);
    int redo_count = -1;
    PCT_TRY(pct_enqueue_download(ctx, idx, d_idx, cells));
    PCT_TRY(pct_enqueue_download(ctx, dist, d_dist, d_dist ? cells : 0));
    PCT_TRY(pct_enqueue_download(ctx, count, d_cnt, (size_t)rows));
    PCT_TRY(pct_enqueue_download(ctx, list.data(), (const int*)ctx->redo.p, list_len));
    PCT_TRY(pct_enqueue_download(ctx, row_of.data(), (const int*)ctx->row_of.p, (size_t)rows));
    PCT_TRY(pct_enqueue_download(ctx, &redo_count, &pct_dev(ctx)->sweep.redo_count, 1));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < cells; ++i)
        if (idx[i] >= ctx->n) idx[i] = -1;                 // (the export's "no neighbour" is n)
    // the redo list as it is: its entries are the leading ones, as many as the counter says, each row once
    size_t written = 0;
    for (size_t i = 0; i < list_len; ++i) written += list[i] != kNoEntry;
    if (redo_count < 0 || (int64_t)redo_count > rows || written != (size_t)redo_count)
        return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_sweep: the redo list holds %zu entries, redo_count says %d", written, redo_count);
    const unsigned trusted_bit = pct_redo_trusted_bit();
    std::vector<uint8_t> by_row((size_t)rows, 0);
    for (int i = 0; i < redo_count; ++i) {
        if (list[(size_t)i] == kNoEntry) return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_sweep: entry %d of %d of the redo list was not written", i, redo_count);
        const unsigned e = (unsigned)list[(size_t)i], row = e & ~trusted_bit;
        if ((int64_t)row >= rows) return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_sweep: redo entry %d names row %u of %lld", i, row, (long long)rows);
        if (by_row[row]) return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_sweep: row %u is on the redo list twice", row);
        by_row[row] = (uint8_t)(1 | ((e & trusted_bit) ? 2 : 0));
    }
    for (int64_t i = 0; i < rows; ++i) {
        if (row_of[(size_t)i] < 0 || row_of[(size_t)i] >= rows) return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_sweep: no table row for public index %lld", (long long)(ctx->q_begin + i));
        flags[i] = by_row[(size_t)row_of[(size_t)i]];
    }
    const pct_grid& g = ctx->grid;
    const double words[12] = {(double)ctx->tm.sweep_variant, (double)redo_count, g.cell, (double)g.nx, (double)g.ny, (double)g.nz, g.ox, g.oy, g.oz,
                              dist_kept ? 1.0 : 0.0, (double)ctx->items_q, (double)ctx->n_items};
    memcpy(info, words, sizeof(words));
    return PCT_OK;
}

// ---- self-tests of the chained sweep's planning kernels (pct_levels.hip): as the sorters', host arrays in and out --------------
int pct_selftest_levels_classify(pct_ctx* ctx, const int32_t* row_done, const uint32_t* redo_m, const int32_t* pub, int64_t n_rows,
                                 int64_t n_pub, float log_edge, float target, float* want, float* bracket) {
    PCT_TRY(pct_begin_call(ctx));
    if (!row_done || !redo_m || !pub || !want || !bracket) return pct_fail(ctx, PCT_ERR_INVALID, "null array");
    if (n_rows < 1 || n_rows > ((int64_t)1 << 22) || n_pub < n_rows || n_pub > ((int64_t)1 << 24))
        return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_levels_classify: n_rows = %lld (1 .. 2^22), n_pub = %lld (n_rows .. 2^24)", (long long)n_rows, (long long)n_pub);
    // the kernel writes want[pub] and bracket[pub] of every row: each public index inside the arrays, and once
    std::vector<char> seen((size_t)n_pub, 0);
    for (int64_t i = 0; i < n_rows; ++i) {
        if (pub[i] < 0 || pub[i] >= n_pub || seen[(size_t)pub[i]]) return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_levels_classify: public index %d outside [0, n_pub) or twice", (int)pub[i]);
        seen[(size_t)pub[i]] = 1;
    }
    // row i is the query at position n_rows - 1 - i of the cell order: neither lookup is the identity
    std::vector<float4> rec((size_t)n_rows);
    std::vector<int> owned((size_t)n_rows);
    for (int64_t i = 0; i < n_rows; ++i) {
        float w;
        memcpy(&w, &pub[i], 4);
        owned[(size_t)i] = (int)(n_rows - 1 - i);
        rec[(size_t)(n_rows - 1 - i)] = make_float4(0.f, 0.f, 0.f, w);
    }
    DevScratch mem{ctx};
    int *d_done, *d_redo, *d_owned;
    float4* d_rec;
    float *d_want, *d_br;
    PCT_TRY(mem.take(&d_done, (size_t)n_rows, row_done));
    PCT_TRY(mem.take(&d_redo, (size_t)n_rows, (const int*)redo_m));
    PCT_TRY(mem.take(&d_owned, (size_t)n_rows, owned.data()));
    PCT_TRY(mem.take(&d_rec, (size_t)n_rows, rec.data()));
    PCT_TRY(mem.take(&d_want, (size_t)n_pub, want));
    PCT_TRY(mem.take(&d_br, (size_t)n_pub * 2, bracket));
    PCT_TRY(pct_launch_selftest_levels_classify(ctx, d_done, d_redo, n_rows, d_rec, d_owned, log_edge, target, d_want, d_br));
    PCT_TRY(pct_enqueue_download(ctx, want, d_want, (size_t)n_pub));
    PCT_TRY(pct_enqueue_download(ctx, bracket, d_br, (size_t)n_pub * 2));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));        // (rec, owned and the scratch outlive every copy: waited for here)
    return PCT_OK;
}

int pct_selftest_levels_bands(pct_ctx* ctx, const float* want, const float* xyz, int64_t n, int64_t begin, int64_t end, float log_edge0,
                              int32_t window, float lo, float hi, uint32_t* hist, uint32_t* exact, float* bounds, float* box, uint32_t* count) {
    PCT_TRY(pct_begin_call(ctx));
    if (!want || !xyz || !hist || !exact || !bounds || !box || !count) return pct_fail(ctx, PCT_ERR_INVALID, "null array");
    if (n < 1 || n > ((int64_t)1 << 24) || begin < 0 || begin > end || end > n)
        return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_levels_bands: n = %lld (1 .. 2^24), [begin, end) = [%lld, %lld) inside it", (long long)n, (long long)begin, (long long)end);
    if (window < -1 || window > 156) return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_levels_bands: window = %d (-1: lo and hi as given; 0 .. 156)", (int)window);
    constexpr int kStatWords = 162, kBoxWords = 7;
    DevScratch mem{ctx};
    float *d_want, *d_xyz;
    unsigned* d_stats;
    int* d_box;
    PCT_TRY(mem.take(&d_want, (size_t)n, want));
    PCT_TRY(mem.take(&d_xyz, (size_t)n * 3, xyz));
    PCT_TRY(mem.take(&d_stats, (size_t)kStatWords));
    PCT_TRY(mem.take(&d_box, (size_t)kBoxWords));
    PCT_TRY(pct_launch_selftest_levels_bands(ctx, d_want, d_xyz, begin, end, log_edge0, window, lo, hi, d_stats, bounds, d_box));
    unsigned h_stats[kStatWords];
    int h_box[kBoxWords];
    PCT_TRY(pct_enqueue_download(ctx, h_stats, d_stats, (size_t)kStatWords));
    PCT_TRY(pct_enqueue_download(ctx, h_box, d_box, (size_t)kBoxWords));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(hist, h_stats, 160 * sizeof(uint32_t));
    *exact = h_stats[160];
    for (int a = 0; a < 6; ++a) box[a] = pct_levels_box_float(h_box[a]);
    *count = (uint32_t)h_box[6];
    return PCT_OK;
}

int pct_selftest_levels_merge(pct_ctx* ctx, const int32_t* pub, int64_t n_pos, const int32_t* owned_pos, int32_t q_begin, const int32_t* nbr_pos,
                              const float* nbr_dist, const int32_t* nbr_cnt, const int32_t* row_done, int64_t n_rows, int32_t k, int32_t pitch,
                              int64_t n_out, int32_t* pub_pos, float* pub_dist, int32_t* pub_cnt, float* want, int64_t n_want) {
    PCT_TRY(pct_begin_call(ctx));
    if (!pub || !owned_pos || !nbr_pos || !nbr_dist || !row_done || !pub_pos || !pub_dist || !want) return pct_fail(ctx, PCT_ERR_INVALID, "null array");
    if (n_pos < 1 || n_pos > ((int64_t)1 << 24) || n_rows < 1 || n_rows > ((int64_t)1 << 20) || k < 1 || pitch < k || pitch > 512 || n_out < 1 ||
        n_out > ((int64_t)1 << 22) || n_want < 1 || n_want > ((int64_t)1 << 24) || q_begin < 0)
        return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_levels_merge: n_pos = %lld, n_rows = %lld, k = %d, pitch = %d, n_out = %lld, n_want = %lld, q_begin = %d",
                        (long long)n_pos, (long long)n_rows, (int)k, (int)pitch, (long long)n_out, (long long)n_want, (int)q_begin);
    // every address the kernel forms from the caller's numbers lies inside the caller's arrays
    for (int64_t r = 0; r < n_rows; ++r) {
        if (owned_pos[r] < 0 || owned_pos[r] >= n_pos) return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_levels_merge: owned position %d outside [0, n_pos)", (int)owned_pos[r]);
        const int64_t p = pub[owned_pos[r]];
        if (p < q_begin || p - q_begin >= n_out || p >= n_want) return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_levels_merge: public index %lld outside the output rows or the wanted edges", (long long)p);
        for (int j = 0; j < k; ++j)
            if (nbr_pos[r * pitch + j] >= n_pos) return pct_fail(ctx, PCT_ERR_INVALID, "pct_selftest_levels_merge: neighbour position %d outside [0, n_pos)", (int)nbr_pos[r * pitch + j]);
    }
    const std::vector<float4> rec = pub_records(pub, n_pos);
    const size_t in_cells = (size_t)n_rows * pitch, out_cells = (size_t)n_out * pitch;
    DevScratch mem{ctx};
    float4* d_rec;
    int *d_owned, *d_npos, *d_ncnt = nullptr, *d_done, *d_ppos, *d_pcnt = nullptr;
    float *d_ndist, *d_pdist, *d_want;
    PCT_TRY(mem.take(&d_rec, rec.size(), rec.data()));
    PCT_TRY(mem.take(&d_owned, (size_t)n_rows, owned_pos));
    PCT_TRY(mem.take(&d_done, (size_t)n_rows, row_done));
    PCT_TRY(mem.take(&d_npos, in_cells, nbr_pos));
    PCT_TRY(mem.take(&d_ndist, in_cells, nbr_dist));
    PCT_TRY(mem.take(&d_ppos, out_cells, pub_pos));
    PCT_TRY(mem.take(&d_pdist, out_cells, pub_dist));
    PCT_TRY(mem.take(&d_want, (size_t)n_want, want));
    if (nbr_cnt) PCT_TRY(mem.take(&d_ncnt, (size_t)n_rows, nbr_cnt));
    if (pub_cnt) PCT_TRY(mem.take(&d_pcnt, (size_t)n_out, pub_cnt));
    PCT_TRY(pct_launch_selftest_levels_merge(ctx, d_rec, d_owned, q_begin, d_npos, d_ndist, d_ncnt, d_done, n_rows, k, pitch, d_ppos, d_pdist, d_pcnt, d_want));
    PCT_TRY(pct_enqueue_download(ctx, pub_pos, d_ppos, out_cells));
    PCT_TRY(pct_enqueue_download(ctx, pub_dist, d_pdist, out_cells));
    PCT_TRY(pct_enqueue_download(ctx, pub_cnt, d_pcnt, (size_t)n_out));
    PCT_TRY(pct_enqueue_download(ctx, want, d_want, (size_t)n_want));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PCT_OK;
}

}  // extern "C"

// Rows of a per-row result on their way to the host: the one download every row getter of pct_api.hip ends in, and the one
// gather kernel behind it for results stored in neighbour-table row order.  A cold path: a getter call, never a step.
#include "pct_internal.h"

namespace {

struct GatherCols {
    const char* src[kPctRowColumns];
    char* dst[kPctRowColumns];         // null: column not asked for
    int bytes[kPctRowColumns];         // per row
    int unit[kPctRowColumns];          // 8, 4 or 1: the widest word that divides the row and that both ends are aligned to
};

template <typename W>
__device__ inline void copy_row(char* __restrict__ dst, const char* __restrict__ src, int bytes) {
    const int words = bytes / (int)sizeof(W);
    for (int w = 0; w < words; ++w) ((W*)dst)[w] = ((const W*)src)[w];
}

// row i of every column <- row map[i]
__global__ __launch_bounds__(256) void k_gather_rows(const int* __restrict__ map, int64_t rows, GatherCols c) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const int64_t r = map[i];
#pragma unroll
    for (int j = 0; j < kPctRowColumns; ++j) {
        if (!c.dst[j]) continue;
        const int b = c.bytes[j];
        char* d = c.dst[j] + i * b;
        const char* s = c.src[j] + r * b;
        if (c.unit[j] == 8) copy_row<unsigned long long>(d, s, b);
        else if (c.unit[j] == 4) copy_row<unsigned>(d, s, b);
        else copy_row<unsigned char>(d, s, b);
    }
}

// rows d_map[i], i < rows, of the columns into d_out (null: column skipped)
int launch_gather_rows(pct_ctx* ctx, const pct_column* cols, int ncol, void* const* d_out, const int* d_map, int64_t rows) {
    if (ncol > kPctRowColumns) return pct_fail(ctx, PCT_ERR_INVALID, "gather of %d columns (at most %d)", ncol, kPctRowColumns);
    if (rows <= 0) return PCT_OK;
    GatherCols c = {};
    for (int j = 0; j < ncol; ++j) {
        c.src[j] = (const char*)cols[j].base;
        c.dst[j] = (char*)d_out[j];
        c.bytes[j] = cols[j].bytes;
        const uintptr_t ends = (uintptr_t)cols[j].base | (uintptr_t)d_out[j] | (uintptr_t)cols[j].bytes;
        c.unit[j] = ends % 8 == 0 ? 8 : ends % 4 == 0 ? 4 : 1;
    }
    PCT_LAUNCH(k_gather_rows, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, ctx->stream, d_map, rows, c);
    PCT_HIP(ctx, hipGetLastError());
    return PCT_OK;
}

}  // namespace

// Rows [first, first + rows) of the columns the caller asked for, enqueued: copied from where the rows lie -- or, with a map
// (rows map[first + i] of the stored order), from a staging claim, where one gather has packed the columns asked for back to back.
// Columns that lie back to back on the device and at the caller travel in one copy (K, H of a million points: 0.65 -> 0.4 ms).
int pct_enqueue_columns(pct_ctx* ctx, const pct_column* cols, int ncol, int64_t first, int64_t rows, const int* map) {
    constexpr int kMax = 8;
    if (ncol > (map ? kPctRowColumns : kMax)) return pct_fail(ctx, PCT_ERR_INVALID, "download of %d columns", ncol);
    if (rows <= 0) return PCT_OK;
    pct_stage_scope stage(ctx);
    const char* src[kMax] = {};
    for (int j = 0; j < ncol; ++j) src[j] = (const char*)cols[j].base + first * cols[j].bytes;
    if (map) {
        size_t at[kPctRowColumns] = {}, total = 0;
        for (int j = 0; j < ncol; ++j) {
            if (!cols[j].host) continue;
            const size_t unit = cols[j].bytes % 8 == 0 ? 8 : cols[j].bytes % 4 == 0 ? 4 : 1;
            at[j] = total = (total + unit - 1) / unit * unit;
            total += (size_t)rows * cols[j].bytes;
        }
        char* packed = nullptr;
        PCT_TRY(pct_claim(ctx, total, &packed));
        void* staged[kPctRowColumns] = {};
        for (int j = 0; j < ncol; ++j)
            if (cols[j].host) src[j] = (const char*)(staged[j] = packed + at[j]);
        PCT_TRY(launch_gather_rows(ctx, cols, ncol, staged, map + first, rows));
    }
    for (int j = 0; j < ncol;) {
        if (!cols[j].host) { ++j; continue; }
        size_t bytes = (size_t)rows * cols[j].bytes;
        int e = j + 1;
        for (; e < ncol && cols[e].host && src[e] == src[j] + bytes && (char*)cols[e].host == (char*)cols[j].host + bytes; ++e)
            bytes += (size_t)rows * cols[e].bytes;
        PCT_HIP(ctx, hipMemcpyAsync(cols[j].host, src[j], bytes, hipMemcpyDeviceToHost, ctx->stream));
        j = e;
    }
    return PCT_OK;
}

int pct_download_columns(pct_ctx* ctx, const pct_column* cols, int ncol, int64_t first, int64_t rows, const int* map) {
    PCT_TRY(pct_enqueue_columns(ctx, cols, ncol, first, rows, map));
    if (rows > 0) PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PCT_OK;
}

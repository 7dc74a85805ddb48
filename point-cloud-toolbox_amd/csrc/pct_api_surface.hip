// C ABI of the surface stages -- what is computed from the resident neighbour table: point areas and the energies over
// them, point frames, their orientation, fans and triangles, boundary loops and patches (include/pct_hip.h,
// pct_hip_surface.h, pct_hip_holes.h).  Host-side orchestration only, no kernel: every computing entry point checks its own
// arguments and preconditions and then goes through run_stage, every statistics getter through stage_numbers.
#include "pct_internal.h"

#include <math.h>

// r is in place for every owned row (the fit: the cloud-aligned one), else PCT_ERR_INVALID with `missing`
static int need_for_owned_rows(pct_ctx* ctx, pct_resident r, const char* missing) {
    if (ctx->res.covers(r, ctx->q_end - ctx->q_begin) && (r != PCT_R_FIT || ctx->fit_cloud_aligned)) return PCT_OK;
    return pct_fail(ctx, PCT_ERR_INVALID, "%s", missing);
}

// One call of a surface stage, behind every refusal of its entry point (a refused call leaves the result and the report of
// an earlier one).  launch(rep, &by_row) enqueues the stage; report (null: the launcher had every number on the host) reads
// its pinned words; mid: the launcher records PCT_EV_STAGE_MID.  The result is gone from the first line on and back, for
// `rows` rows, with the last: a failed launcher leaves none, and nothing of it in flight.
template <class Launch>
static int run_stage(pct_ctx* ctx, pct_stage stage, int64_t rows, bool mid, void (*report)(pct_ctx*, pct_stage_report*), Launch launch) {
    const pct_resident r = kPctStageResident[stage];
    ctx->res.drop(pct_replacing(r));
    PCT_HIP(ctx, hipEventRecord(ctx->ev[PCT_EV_STAGE_BEGIN], ctx->stream));
    pct_stage_report rep = {};
    bool by_row = false;
    const int status = launch(&rep, &by_row);
    if (status != PCT_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        return status;
    }
    PCT_HIP(ctx, hipEventRecord(ctx->ev[PCT_EV_STAGE_END], ctx->stream));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));              // the call's one wait of its own: results, statistics words, events
    if (report) report(ctx, &rep);
    rep.ms[0] = pct_ev_ms(ctx, PCT_EV_STAGE_BEGIN, PCT_EV_STAGE_END);
    if (mid) {
        rep.ms[1] = pct_ev_ms(ctx, PCT_EV_STAGE_BEGIN, PCT_EV_STAGE_MID);
        rep.ms[2] = pct_ev_ms(ctx, PCT_EV_STAGE_MID, PCT_EV_STAGE_END);
    }
    ctx->report[stage] = rep;
    ctx->res.leave(r, by_row, rows);
    return PCT_OK;
}

// What a statistics getter answers: the first n_stats counters and n_ms doubles from ms[ms_first] on of the stage's report
// while its result is in place, zeros otherwise.  required: the getter's output that must not be null; ms may be.
static int stage_numbers(pct_ctx* ctx, pct_stage stage, const void* required, int64_t* stats, int n_stats, double* ms, int ms_first, int n_ms) {
    if (!ctx || !required) return PCT_ERR_INVALID;
    const bool live = ctx->res.has(kPctStageResident[stage]);
    const pct_stage_report& rep = ctx->report[stage];
    for (int i = 0; i < n_stats; ++i) stats[i] = live ? rep.stats[i] : 0;
    for (int i = 0; ms && i < n_ms; ++i) ms[i] = live ? rep.ms[ms_first + i] : 0.0;
    return PCT_OK;
}

extern "C" {

// ---- per-point tangent-plane Voronoi areas and the energies over them (pct_area.hip) --------------------------------------
int pct_point_areas(pct_ctx* ctx) {
    PCT_TRY(pct_begin_row_call(ctx, "pct_point_areas"));
    if (!ctx->res.has(PCT_R_TABLE)) return pct_fail(ctx, PCT_ERR_NO_NEIGHBORS, "plant the neighbour table first (pct_knn)");
    return run_stage(ctx, PCT_STAGE_AREAS, ctx->q_end - ctx->q_begin, false, pct_area_report,
                     [&](pct_stage_report*, bool* by_row) { return pct_launch_point_areas(ctx, by_row); });
}

int pct_get_point_areas(pct_ctx* ctx, int64_t begin, int64_t end, double* area, uint8_t* closed, int32_t* nverts) {
    PCT_TRY(pct_begin_row_call(ctx, "pct_get_point_areas"));
    if (!ctx->res.has(PCT_R_AREAS)) return pct_fail(ctx, PCT_ERR_INVALID, "no point areas (pct_point_areas)");
    PCT_TRY(pct_check_owned_span(ctx, "the owned range", PCT_R_AREAS, begin, end, ctx->q_begin));
    const pct_column cols[] = {{ctx->area.p, sizeof(double), area}, {ctx->area_closed.p, 1, closed}, {ctx->area_nverts.p, sizeof(int), nverts}};
    return pct_get_rows(ctx, PCT_R_AREAS, cols, 3, begin - ctx->q_begin, end - begin);
}

int pct_point_area_stats(pct_ctx* ctx, int64_t out[4]) { return stage_numbers(ctx, PCT_STAGE_AREAS, out, out, 4, nullptr, 0, 0); }

// (the survivor count travels as the double behind the milliseconds)
int pct_point_area_profile(pct_ctx* ctx, double out[2]) { return stage_numbers(ctx, PCT_STAGE_AREAS, out, nullptr, 0, out, 0, 2); }

int pct_point_energies(pct_ctx* ctx, int32_t closed_only, double out[4]) {
    PCT_TRY(pct_begin_row_call(ctx, "pct_point_energies"));
    if (!out) return pct_fail(ctx, PCT_ERR_INVALID, "null result");
    PCT_TRY(need_for_owned_rows(ctx, PCT_R_FIT, "no fit results"));
    PCT_TRY(need_for_owned_rows(ctx, PCT_R_AREAS, "no point areas (pct_point_areas)"));
    const int nblk = 1024;
    double* d_part = nullptr;
    PCT_TRY(pct_claim(ctx, (size_t)nblk * 4 + 4, &d_part));
    PCT_TRY(pct_launch_point_energies(ctx, closed_only != 0, d_part, d_part + (size_t)nblk * 4));
    PCT_TRY(pct_enqueue_download(ctx, out, d_part + (size_t)nblk * 4, 4));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PCT_OK;
}

// ---- per-point surface frames from the resident fit (pct_frame.hip) ----------------------------------------------------
int pct_point_frames(pct_ctx* ctx, const double* viewpoint) {
    PCT_TRY(pct_begin_row_call(ctx, "pct_point_frames"));
    if (!ctx->res.has(PCT_R_TABLE)) return pct_fail(ctx, PCT_ERR_NO_NEIGHBORS, "plant the neighbour table first (pct_knn)");
    PCT_TRY(need_for_owned_rows(ctx, PCT_R_FIT, "no fit results"));
    if (viewpoint && !(isfinite(viewpoint[0]) && isfinite(viewpoint[1]) && isfinite(viewpoint[2])))
        return pct_fail(ctx, PCT_ERR_INVALID, "pct_point_frames: the viewpoint is not finite");
    return run_stage(ctx, PCT_STAGE_FRAMES, ctx->q_end - ctx->q_begin, false, pct_frame_report,
                     [&](pct_stage_report*, bool* by_row) { return pct_launch_point_frames(ctx, viewpoint, by_row); });
}

int pct_get_point_frames(pct_ctx* ctx, int64_t begin, int64_t end, double* normal, double* k12, double* dirs, uint8_t* flipped) {
    PCT_TRY(pct_begin_row_call(ctx, "pct_get_point_frames"));
    if (!ctx->res.has(PCT_R_FRAMES)) return pct_fail(ctx, PCT_ERR_INVALID, "no point frames (pct_point_frames)");
    PCT_TRY(pct_check_owned_span(ctx, "the owned range", PCT_R_FRAMES, begin, end, ctx->q_begin));
    const int64_t all = ctx->res.rows_of(PCT_R_FRAMES);
    const double* f = (const double*)ctx->frame.p;
    const pct_column cols[] = {{f, 3 * sizeof(double), normal}, {f + all * 3, 2 * sizeof(double), k12}, {f + all * 5, 6 * sizeof(double), dirs},
                               {(const unsigned char*)ctx->frame_flip.p + 64, 1, flipped}};
    return pct_get_rows(ctx, PCT_R_FRAMES, cols, 4, begin - ctx->q_begin, end - begin);
}

int pct_point_frame_stats(pct_ctx* ctx, int64_t out[4], double* ms) { return stage_numbers(ctx, PCT_STAGE_FRAMES, out, out, 4, ms, 0, 1); }

// ---- consistent orientation of the resident frames (pct_orient.hip) ------------------------------------------------------
// the orientation belongs to the frames it turned: whatever drops or replaces them drops it (pct_residents.h)
int pct_orient_frames(pct_ctx* ctx, int32_t anchor, const double* viewpoint, int32_t max_components) {
    PCT_TRY(pct_begin_row_call(ctx, "pct_orient_frames"));
    if (!ctx->res.has(PCT_R_FRAMES) || !ctx->res.has(PCT_R_TABLE)) return pct_fail(ctx, PCT_ERR_INVALID, "no point frames (pct_point_frames)");
    const int64_t rows = ctx->q_end - ctx->q_begin;
    if (ctx->q_begin != 0 || ctx->q_end != ctx->n || ctx->culled || !ctx->res.covers(PCT_R_FRAMES, rows))
        return pct_fail(ctx, PCT_ERR_INVALID, "pct_orient_frames: the handle owns rows [%lld,%lld) of %lld: the flood needs the whole cloud",
                        (long long)ctx->q_begin, (long long)ctx->q_end, (long long)ctx->n);
    if (anchor != PCT_ORIENT_SEED && anchor != PCT_ORIENT_TOP && anchor != PCT_ORIENT_VIEW)
        return pct_fail(ctx, PCT_ERR_INVALID, "pct_orient_frames: unknown anchor %d", anchor);
    if (anchor == PCT_ORIENT_VIEW && !(viewpoint && isfinite(viewpoint[0]) && isfinite(viewpoint[1]) && isfinite(viewpoint[2])))
        return pct_fail(ctx, PCT_ERR_INVALID, "pct_orient_frames: PCT_ORIENT_VIEW needs a finite viewpoint");
    const int max_comp = max_components <= 0 ? 65536 : max_components;
    return run_stage(ctx, PCT_STAGE_ORIENT, rows, false, pct_orient_report, [&](pct_stage_report* rep, bool*) {
        return pct_run_orient(ctx, anchor, anchor == PCT_ORIENT_VIEW ? viewpoint : nullptr, max_comp, rep);
    });
}

int pct_get_orientation(pct_ctx* ctx, int64_t begin, int64_t end, int32_t* component, int32_t* parent, int32_t* level, uint8_t* toggled) {
    PCT_TRY(pct_begin_row_call(ctx, "pct_get_orientation"));
    if (!ctx->res.has(PCT_R_ORIENT)) return pct_fail(ctx, PCT_ERR_INVALID, "no orientation (pct_orient_frames)");
    PCT_TRY(pct_check_owned_span(ctx, "the cloud", PCT_R_ORIENT, begin, end, 0));
    const pct_column cols[] = {{ctx->orient_comp, sizeof(int), component}, {ctx->orient_parent, sizeof(int), parent},
                               {ctx->orient_level, sizeof(int), level}, {ctx->orient_toggle, 1, toggled}};
    return pct_download_columns(ctx, cols, 4, begin, end - begin, nullptr);
}

int pct_orient_stats(pct_ctx* ctx, int64_t out[8], double* ms) { return stage_numbers(ctx, PCT_STAGE_ORIENT, out, out, 8, ms, 0, 1); }

// ---- faces from the tangent-plane Voronoi cells (pct_fan.hip, include/pct_hip_surface.h) -----------------------------------
int pct_point_triangles(pct_ctx* ctx, int32_t flags) {
    PCT_TRY(pct_begin_row_call(ctx, "pct_point_triangles"));
    if (!ctx->res.has(PCT_R_TABLE)) return pct_fail(ctx, PCT_ERR_NO_NEIGHBORS, "plant the neighbour table first (pct_knn)");
    if (ctx->q_begin != 0 || ctx->q_end != ctx->n || ctx->culled)
        return pct_fail(ctx, PCT_ERR_INVALID, "pct_point_triangles: the handle owns rows [%lld,%lld) of %lld: agreement needs the whole cloud",
                        (long long)ctx->q_begin, (long long)ctx->q_end, (long long)ctx->n);
    if (flags & ~PCT_TRI_WIND_FRAMES) return pct_fail(ctx, PCT_ERR_INVALID, "pct_point_triangles: unknown flags %d", flags);
    const bool wind = (flags & PCT_TRI_WIND_FRAMES) != 0;
    if (wind) PCT_TRY(need_for_owned_rows(ctx, PCT_R_FRAMES, "no point frames (pct_point_frames)"));
    return run_stage(ctx, PCT_STAGE_TRIANGLES, ctx->n, true, pct_fan_report,       // (kept by public index)
                     [&](pct_stage_report*, bool*) { return pct_launch_point_triangles(ctx, wind, ctx->ev[PCT_EV_STAGE_MID]); });
}

int pct_get_point_fans(pct_ctx* ctx, int64_t begin, int64_t end, int64_t* offsets, int32_t* nbr) {
    PCT_TRY(pct_begin_call(ctx));
    if (!ctx->res.has(PCT_R_TRIANGLES)) return pct_fail(ctx, PCT_ERR_INVALID, "no triangles (pct_point_triangles)");
    if (begin < 0 || end > ctx->res.rows_of(PCT_R_TRIANGLES) || begin > end || !offsets)
        return pct_fail(ctx, PCT_ERR_INVALID, "rows [%lld,%lld) outside the cloud", (long long)begin, (long long)end);
    const int64_t rows = end - begin;
    int64_t *d_count = nullptr, *d_off = nullptr;
    PCT_TRY(pct_claim(ctx, (size_t)(rows + 1), &d_count));
    PCT_TRY(pct_claim(ctx, (size_t)(rows + 1), &d_off));
    PCT_TRY(pct_launch_point_fans(ctx, begin, rows, d_count, d_off, nullptr));
    PCT_TRY(pct_enqueue_download(ctx, offsets, d_off, (size_t)(rows + 1)));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int64_t total = offsets[rows];
    if (!nbr || total == 0) return PCT_OK;
    int* d_nbr = nullptr;
    PCT_TRY(pct_claim(ctx, (size_t)total, &d_nbr));
    PCT_TRY(pct_launch_point_fans(ctx, begin, rows, d_count, d_off, d_nbr));
    PCT_TRY(pct_enqueue_download(ctx, nbr, d_nbr, (size_t)total));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PCT_OK;
}

// triangles [first, first + count) of an ascending (have, 3) array
static int download_triangles(pct_ctx* ctx, const pct_buf& src, int64_t have, int64_t first, int64_t count, int32_t* tri) {
    if (first < 0 || count < 0 || first + count > have || (count > 0 && !tri))
        return pct_fail(ctx, PCT_ERR_INVALID, "triangles [%lld,%lld) outside the %lld resident", (long long)first, (long long)(first + count), (long long)have);
    const pct_column col = {src.p, 3 * sizeof(int), tri};
    return pct_download_columns(ctx, &col, 1, first, count, nullptr);
}

int pct_get_triangles(pct_ctx* ctx, int64_t first, int64_t count, int32_t* tri) {
    PCT_TRY(pct_begin_call(ctx));
    if (!ctx->res.has(PCT_R_TRIANGLES)) return pct_fail(ctx, PCT_ERR_INVALID, "no triangles (pct_point_triangles)");
    return download_triangles(ctx, ctx->tri, ctx->tri_total, first, count, tri);
}

int pct_point_triangle_stats(pct_ctx* ctx, int64_t out[8], double* ms) { return stage_numbers(ctx, PCT_STAGE_TRIANGLES, out, out, 8, ms, 0, 1); }

int pct_point_triangle_profile(pct_ctx* ctx, double out[2]) { return stage_numbers(ctx, PCT_STAGE_TRIANGLES, out, nullptr, 0, out, 1, 2); }

// ---- boundary loops and small-hole filling (pct_hole.hip, include/pct_hip_holes.h): PCT_R_HOLES, made from the triangles ------
int pct_fill_holes(pct_ctx* ctx, int32_t max_vertices, double max_perimeter, int32_t flags) {
    PCT_TRY(pct_begin_row_call(ctx, "pct_fill_holes"));
    if (ctx->n > 0 && (ctx->q_begin != 0 || ctx->q_end != ctx->n || ctx->culled))
        return pct_fail(ctx, PCT_ERR_INVALID, "pct_fill_holes: the handle owns rows [%lld,%lld) of %lld: a loop may cross into other rows",
                        (long long)ctx->q_begin, (long long)ctx->q_end, (long long)ctx->n);
    if (!ctx->res.has(PCT_R_TRIANGLES)) return pct_fail(ctx, PCT_ERR_INVALID, "no triangles (pct_point_triangles)");
    if (max_vertices < 3 || max_vertices > PCT_HOLE_MAX_VERTICES)
        return pct_fail(ctx, PCT_ERR_INVALID, "pct_fill_holes: max_vertices=%d outside [3,%d]", max_vertices, PCT_HOLE_MAX_VERTICES);
    if (!(max_perimeter > 0.0)) return pct_fail(ctx, PCT_ERR_INVALID, "pct_fill_holes: max_perimeter must be positive (+inf: no cap)");
    if (flags != 0) return pct_fail(ctx, PCT_ERR_INVALID, "pct_fill_holes: unknown flags %d", flags);
    return run_stage(ctx, PCT_STAGE_HOLES, ctx->n, false, nullptr,
                     [&](pct_stage_report* rep, bool*) { return pct_launch_fill_holes(ctx, max_vertices, max_perimeter, rep); });
}

static int get_triangle_rows(pct_ctx* ctx, const pct_buf& src, int64_t have, int64_t first, int64_t count, int32_t* tri) {
    PCT_TRY(pct_begin_call(ctx));
    if (!ctx->res.has(PCT_R_HOLES)) return pct_fail(ctx, PCT_ERR_INVALID, "no hole results (pct_fill_holes)");
    return download_triangles(ctx, src, have, first, count, tri);
}

int pct_get_hole_triangles(pct_ctx* ctx, int64_t first, int64_t count, int32_t* tri) {
    if (!ctx) return PCT_ERR_INVALID;
    return get_triangle_rows(ctx, ctx->hole_tri, ctx->hole_patches, first, count, tri);
}

int pct_get_filled_triangles(pct_ctx* ctx, int64_t first, int64_t count, int32_t* tri) {
    if (!ctx) return PCT_ERR_INVALID;
    return get_triangle_rows(ctx, ctx->hole_filled, ctx->tri_total + ctx->hole_patches, first, count, tri);
}

int pct_get_boundary_loops(pct_ctx* ctx, int64_t* offsets, int32_t* vertices, uint8_t* status) {
    PCT_TRY(pct_begin_call(ctx));
    if (!ctx->res.has(PCT_R_HOLES)) return pct_fail(ctx, PCT_ERR_INVALID, "no hole results (pct_fill_holes)");
    if (!offsets) return pct_fail(ctx, PCT_ERR_INVALID, "null offsets");
    const int64_t loops = ctx->hole_loops, verts = ctx->hole_loop_verts;
    const char* base = (const char*)ctx->hole_loop.p;
    const size_t off_bytes = (size_t)(loops + 1) * sizeof(int64_t), vert_bytes = (size_t)verts * sizeof(int);
    PCT_HIP(ctx, hipMemcpyAsync(offsets, base, off_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (status && loops > 0) PCT_HIP(ctx, hipMemcpyAsync(status, base + off_bytes + vert_bytes, (size_t)loops, hipMemcpyDeviceToHost, ctx->stream));
    if (vertices && verts > 0) PCT_HIP(ctx, hipMemcpyAsync(vertices, base + off_bytes, vert_bytes, hipMemcpyDeviceToHost, ctx->stream));
    PCT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PCT_OK;
}

int pct_fill_hole_stats(pct_ctx* ctx, int64_t out[8], double* ms) { return stage_numbers(ctx, PCT_STAGE_HOLES, out, out, 8, ms, 0, 1); }

}  // extern "C"

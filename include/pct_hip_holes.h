/*
 * pct_hip_holes.h -- watertight faces: the boundary loops of the resident triangles and the filling of the small ones, on
 * the device.  Same handle, same status codes and same conventions as pct_hip.h and pct_hip_surface.h, which this header
 * includes; the ctypes shim binds its entry points from a table of their own (HOLE_SIGNATURES).
 *
 * pct_point_triangles leaves a surface that is manifold (no edge carries more than two faces) but not closed: where the
 * three corners of a triangle do not all propose it, a gap of a few faces stays.  The reference closes such gaps on the host
 * right after ball pivoting (detect_boundary_loops, utils:407-436; loops whose perimeter is under half the mean extent of the
 * bounding box are triangulated, utils:150-206).  Here the loops are read off the fans, and each small one gets the
 * triangulation of least total squared area.  tests/hole_exact.py states all of it again in NumPy.
 *
 * Inputs.  The resident fans and the resident triangles of pct_point_triangles, and the cloud's coordinates as float64
 * (a float32 cloud widens exactly).  The fan of a row is its natural neighbours in polygon order, taken cyclically.
 *   faces(u, v)   the number of resident triangles that hold both u and v;
 *   sector t      of row v with fan F (m >= 2 entries): the pair (F[t], F[t + 1 mod m]); it is filled when the triangle
 *                 {v, F[t], F[t + 1]} is resident.
 * Gaps.  A fan position t with faces(v, F[t]) == 1, sector t empty and sector t - 1 filled opens a gap.  s is the first
 * position forward of t, cyclically (t + 1, t + 2, ..., t itself last), with faces(v, F[s]) > 0.  If s != t,
 * faces(v, F[s]) == 1 and sector s is filled, row v has the gap {F[t], F[s]}; otherwise the position is an odd gap: counted,
 * part of no loop.  The gap is an unordered pair: a mirrored frame reverses the fan and gives the same gaps.  A pinch vertex,
 * where four boundary edges meet, has two gaps; the fan order pairs its edges.  A row has as many gaps as it has (count,
 * scan, fill), in fan order.
 * Loops.  One walk starts per gap {a, b} of row v0 (a = F[t], b = F[s]) and leaves v0 towards b.  Arriving at cur from prev
 * it goes on through the first gap of cur that holds prev, to that gap's other member.  It succeeds when it is back at v0
 * from a, with at least three vertices.  It is rejected when it meets a vertex with no such gap, meets a vertex twice (v0
 * from another side included), or would need more than max_vertices vertices.  A loop is owned by the walk that starts at
 * its lowest vertex v0; its canonical order is [v0, w, ...], w the smaller of v0's two neighbours on the loop.  The loops
 * are listed by (v0, fan position of the gap).
 * Perimeter.  The sum, in canonical order and with the closing edge last, of sqrt((dx dx + dy dy) + dz dz) over consecutive
 * vertices, float64, accumulated left to right.  A loop is filled only if perimeter < max_perimeter.
 * Triangulation.  The polygon q[0 .. L - 1] in canonical order gets the triangulation of least total squared area by the
 * interval dynamic programme: W[i][i + 1] = 0; W[i][j] = min over m = i + 1 .. j - 1, ascending, strict <, of
 * (W[i][m] + W[m][j]) + w(i, m, j); w = 0.25 ((cx cx + cy cy) + cz cz), c = (q[m] - q[i]) x (q[j] - q[i]), each component two
 * rounded products and a rounded difference; no fused multiply-add anywhere.  (The squared area: no square root enters the
 * choice, and on a nearly planar quad, where both diagonals give the same area, the squared sum prefers the even split.)
 * w is +inf when {q[i], q[m], q[j]} is a resident triangle (an isolated triangle's own three edges form a 3-loop), or when a
 * side of the triangle is a diagonal (x, y) of the polygon with faces(x, y) > 0 (the fill puts no third face on an edge).
 * A loop whose W[0][L - 1] is not finite is blocked: counted, left open.
 * Emission.  The triangle (q[i], q[m], q[j]), i < m < j, is turned so that its lowest index comes first, cyclic order kept.
 * Let f be the one resident face on the edge (v0, w).  If f runs v0 -> w, as the canonical order does, every triangle of the
 * loop is reversed, (t0, t2, t1); otherwise they stay.  On triangles wound by oriented frames (PCT_TRI_WIND_FRAMES) the
 * patches are then wound as their surroundings.
 * Arrays.  The patch triangles ascending by (v0, v1, v2); the filled array is the merge of the resident triangles and the
 * patches, ascending.  All of it is a pure function of cloud, fans, triangles, max_vertices and max_perimeter: no atomics
 * on the outputs, the same bytes on a second call, the same bytes behind a PCT_KNN_BRUTE and a PCT_KNN_GRID planting.
 *
 * State.  The hole results are an appendix of the triangles (pct_hip.h, "Triangles"), not a result of their own: they are
 * valid exactly while the triangles they were computed from are in place.  Whatever drops the triangles -- a new cloud, a
 * change of ownership, a planting -- drops them, and so does a new pct_point_triangles; a fit, pct_point_frames,
 * pct_orient_frames and pct_voxel_downsample drop neither.  pct_fill_holes touches nothing else on the handle: the
 * triangles, the fans and every other result keep their bytes, and so does pct_timings.  A refused call changes nothing:
 * the hole results of an earlier call stay.
 */
#ifndef PCT_HIP_HOLES_H
#define PCT_HIP_HOLES_H

#include "pct_hip_surface.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCT_HOLE_MAX_VERTICES 32
/* Boundary loops of the resident triangles, the loops of at most max_vertices vertices and a perimeter below max_perimeter
 * filled.  max_vertices in [3, PCT_HOLE_MAX_VERTICES]; max_perimeter > 0, +inf allowed; flags 0: PCT_ERR_INVALID otherwise
 * (a NaN included).  PCT_ERR_INVALID without triangles, as pct_get_triangles, and on a handle that owns a slab or a proper
 * sub-range (a loop may cross ranks: no distributed form). */
int pct_fill_holes(pct_ctx* ctx, int32_t max_vertices, double max_perimeter, int32_t flags);
/* Patch triangles [first, first + count): (count, 3) int32.  PCT_ERR_INVALID without hole results. */
int pct_get_hole_triangles(pct_ctx* ctx, int64_t first, int64_t count, int32_t* tri);
/* Triangles [first, first + count) of the filled array (resident triangles + patches of them).  PCT_ERR_INVALID without
 * hole results. */
int pct_get_filled_triangles(pct_ctx* ctx, int64_t first, int64_t count, int32_t* tri);
/* Every owned loop in canonical order as CSR: offsets (loops + 1, int64, from 0; loops: pct_fill_hole_stats), vertices
 * public indices, status (loops; may be NULL) 0 filled, 1 left for its perimeter, 2 blocked.  vertices == NULL: offsets and
 * status only -- the first of two calls, which sizes the second's array.  PCT_ERR_INVALID without hole results. */
int pct_get_boundary_loops(pct_ctx* ctx, int64_t* offsets, int32_t* vertices, uint8_t* status);
/* Of the last pct_fill_holes: out = {boundary edges before, gaps, odd gaps, loops, loops filled, left for their perimeter,
 * blocked, patch triangles}; *ms (may be NULL) the device milliseconds between two events around the call's work.  Zeros
 * without hole results. */
int pct_fill_hole_stats(pct_ctx* ctx, int64_t out[8], double* ms);

#ifdef __cplusplus
}
#endif

#endif /* PCT_HIP_HOLES_H */

/*
 * pct_hip_surface.h -- the connectivity of the surface: natural neighbours and triangles from the tangent-plane Voronoi
 * cells of the resident neighbour table.  Same handle, same status codes, same conventions and same state rules as
 * pct_hip.h, which this header includes; the ctypes shim binds both headers' entry points from one table.
 *
 * The reference's pipeline builds a triangle mesh on the host before anything else (ball pivoting, utils:92-96), writes
 * self.faces into its PLY (pct:710-715) and integrates its energies over triangles (load_mesh_compute_energies).  Here the
 * faces come from what pct_point_areas already cuts: the localized Delaunay reconstruction (Gopi et al.) on the device.
 */
#ifndef PCT_HIP_SURFACE_H
#define PCT_HIP_SURFACE_H

#include "pct_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pct_point_triangles: fans, corners and triangles of the resident table.  tests/fan_exact.py states it again in NumPy.
 * Row i of the table, count_i valid neighbours:
 *   cell     the polygon pct_point_areas cuts for the row -- the same block, the same rotation R, the square [-L, L]^2 cut
 *            by the same bisectors in the same row order, the same arithmetic -- with one label per vertex v: the label of
 *            the edge from v to v + 1.  The square's edges carry -1.  A cut by the neighbour of row slot j that removes the
 *            run s .. e and inserts I1, I2: the vertices that stay keep their labels, I1 takes j (the edge I1 -> I2 lies on
 *            j's bisector), I2 the label vertex e had (the edge it continues); the same for a wrapped run;
 *   fan      the natural neighbours of the row: the cloud records of the labels >= 0, in polygon order (counter-clockwise
 *            about +z of R);
 *   corner   vertex v is a proper corner when its arriving edge (the label of v - 1, cyclic) and its leaving edge both
 *            carry a neighbour and x^2 + y^2 < L^2 (the disc test of pct_point_areas' closed).  Corners inside the disc are
 *            vertices of the unbounded cell: they depend neither on how the square is turned in the plane nor on the sign
 *            of the normal.  The row's corners are the pairs (a, b) = (record of the arriving label, of the leaving label)
 *            over its proper corners, in polygon order; a corner with a == b is dropped;
 *   NaN rows of pct_point_areas (count_i < 2, a table entry outside the cloud, a frame or bound that is not finite) have
 *            no fan and no corners.
 * A corner (a, b) of row i proposes the triangle {i, a, b}.  It is agreed when row a has a corner whose unordered pair is
 * {b, i} and row b one whose pair is {i, a} (unordered: neighbouring frames may be mirror images of each other).  An edge
 * (i, a) gets triangles only from the two ends of a's edge in i's cell: no edge carries more than two faces.  Every agreed
 * triangle is emitted once, by its corner of lowest public index v0, as (v0, v1, v2) counter-clockwise about v0's normal:
 * +z of R, turned over where PCT_TRI_WIND_FRAMES is given and the resident frames say flipped for v0 (after
 * pct_orient_frames the faces are wound to one side per component).  The array is ascending by (v0, v1, v2): a pure
 * function of the cloud, the table and -- with the flag -- the flipped bits, whatever order the table stores its rows in
 * (PCT_KNN_BRUTE and PCT_KNN_GRID plantings give the same bytes), and two calls on the same state give the same bytes (no
 * atomics on the output).
 *
 * State: the rules are in pct_hip.h ("Triangles", and the paragraphs on refusals, new clouds, ownership and plantings) --
 * what the call needs, that it touches nothing else, what drops the triangles and what does not.  Without
 * PCT_TRI_WIND_FRAMES the winding follows the fit's own side.  eps counts and rows of up to 511 neighbours work as in
 * pct_point_areas. */
#define PCT_TRI_WIND_FRAMES 1
int pct_point_triangles(pct_ctx* ctx, int32_t flags);
/* The natural neighbours of cloud rows [begin, end) as CSR: offsets (end - begin + 1, int64, from 0), nbr public indices
 * in polygon order.  nbr == NULL: offsets only -- the first of two calls, which sizes the second's array.
 * PCT_ERR_INVALID without triangles. */
int pct_get_point_fans(pct_ctx* ctx, int64_t begin, int64_t end, int64_t* offsets, int32_t* nbr);
/* Triangles [first, first + count) of the array: (count, 3) int32 public indices.  PCT_ERR_INVALID without triangles. */
int pct_get_triangles(pct_ctx* ctx, int64_t first, int64_t count, int32_t* tri);
/* Of the last pct_point_triangles: out = {rows, rows with at least one corner, corners, triangles, rows whose cell outgrew
 * the fast kernel's vertex capacity and were finished with room for k + 4 vertices (the same code, the same result),
 * largest fan, boundary edges (edges with exactly one face), 0}; *ms (may be NULL) the device milliseconds between two
 * events around the call's work.  Zeros without triangles. */
int pct_point_triangle_stats(pct_ctx* ctx, int64_t out[8], double* ms);
/* ... and out = {device milliseconds of the fan kernels, of agreement and emission} (hipEvent). */
int pct_point_triangle_profile(pct_ctx* ctx, double out[2]);
/* pct_write_ply_ascii_normals plus "element face n_tri" / "property list uchar int vertex_indices" in the header and one
 * "3 a b c" line per triangle behind the vertices (host code).  tri (n_tri, 3) int32, every index in [0, n):
 * PCT_ERR_INVALID otherwise. */
int pct_write_ply_ascii_faces(const char* path, const float* xyz, const float* normals, const float* gaussian, const float* mean,
                              int64_t n, const int32_t* tri, int64_t n_tri);

#ifdef __cplusplus
}
#endif

#endif /* PCT_HIP_SURFACE_H */

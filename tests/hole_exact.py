"""Boundary loops and small-hole filling over the fans and triangles, the reference  --  TEST INFRASTRUCTURE ONLY (CPU, NumPy,
no import of the package).

``pct_fill_holes`` (include/pct_hip_holes.h) closes the gaps the localized-Delaunay agreement leaves in the faces of
``pct_point_triangles``.  This module states it again, on the fans (one list of natural neighbours per row, in polygon
order, cyclic) and the triangles ((T, 3) int32) of ``fan_exact`` or of the device:

  faces(u, v)  the resident triangles that hold both u and v
  sector t     of row v with fan F (m >= 2): the pair (F[t], F[t + 1 mod m]); filled when {v, F[t], F[t + 1]} is resident
  gap          fan position t with faces(v, F[t]) == 1, sector t empty and sector t - 1 filled; s: the first position
               forward of t (t + 1, t + 2, ... cyclically, t itself last) with faces(v, F[s]) > 0.  s != t,
               faces(v, F[s]) == 1 and sector s filled: the row has the gap {F[t], F[s]}; otherwise an odd gap, counted
  walk         one per gap {a, b} of row v0, leaving towards b; at cur, arrived from prev, on through the first gap of cur
               that holds prev to its other member; closed when it is back at v0 from a with at least three vertices;
               rejected when a vertex has no such gap, is met twice, or more than max_vertices would be needed
  loop         owned by the walk from its lowest vertex v0, in the order [v0, w, ...], w the smaller of v0's two loop
               neighbours; the loops are listed by (v0, fan position of the gap)
  perimeter    sqrt((dx dx + dy dy) + dz dz) of consecutive vertices, the closing edge last, float64, left to right;
               filled only if perimeter < max_perimeter (status 1 otherwise)
  patch        the triangulation of least total squared area by the interval dynamic programme; a triangle costs +inf when
               it is resident or one of its sides is a polygon diagonal with faces > 0; no finite total: blocked (status 2)
  emission     (q[i], q[m], q[j]), i < m < j, turned so that its lowest index comes first, every triangle of the loop
               reversed when the one resident face on the edge (v0, w) runs v0 -> w; patches ascending; the filled array
               the merge of the triangles and the patches
"""
import math

import numpy as np

FILLED, PERIMETER, BLOCKED = 0, 1, 2
STAT_NAMES = ("boundary_edges", "gaps", "odd_gaps", "loops", "filled", "perimeter", "blocked", "patch_triangles")


def default_max_perimeter(points):
    """Half the mean extent of the bounding box, in float64."""
    p = np.asarray(points, np.float64)
    ext = p.max(0) - p.min(0)
    return 0.5 * (((ext[0] + ext[1]) + ext[2]) / 3.0)


def edge_count(tri):
    faces = {}
    for a, b, c in np.asarray(tri).tolist():
        for p, q in ((a, b), (b, c), (a, c)):
            key = (p, q) if p < q else (q, p)
            faces[key] = faces.get(key, 0) + 1
    return faces


def boundary_edges(tri):
    return sum(1 for v in edge_count(tri).values() if v == 1)


def gaps_of(fans, tri):
    """([[(a, b)] per row, in fan order], odd gaps)."""
    faces = edge_count(tri)
    resident = {frozenset(t) for t in np.asarray(tri).tolist()}
    nf = lambda u, v: faces.get((u, v) if u < v else (v, u), 0)
    out, odd = [], 0
    for v, F in enumerate(fans):
        mine = []
        m = len(F)
        if m >= 2:
            filled = [frozenset((v, F[t], F[(t + 1) % m])) in resident for t in range(m)]
            for t in range(m):
                if not (nf(v, F[t]) == 1 and not filled[t] and filled[t - 1]):
                    continue
                s = t
                for step in range(1, m + 1):
                    s = (t + step) % m
                    if nf(v, F[s]) > 0:
                        break
                if s != t and nf(v, F[s]) == 1 and filled[s]:
                    mine.append((F[t], F[s]))
                else:
                    odd += 1
        out.append(mine)
    return out, odd


def walk(gaps, v0, a, b, max_vertices):
    """The vertices [v0, b, ...] of the closed walk, or None."""
    verts = [v0]
    prev, cur = v0, b
    for _ in range(max_vertices):
        if cur == v0:
            return verts if prev == a and len(verts) >= 3 else None
        if cur in verts or len(verts) == max_vertices:
            return None
        verts.append(cur)
        nxt = None
        for p, q in gaps[cur]:
            if p == prev or q == prev:
                nxt = q if p == prev else p
                break
        if nxt is None:
            return None
        prev, cur = cur, nxt
    return None


def perimeter_of(q):
    """q (L, 3) float64 in canonical order."""
    total = 0.0
    L = len(q)
    for i in range(L):
        d = q[(i + 1) % L] - q[i]
        total = total + math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    return total


def weight(q, i, m, j):
    u, v = q[m] - q[i], q[j] - q[i]
    cx = u[1] * v[2] - u[2] * v[1]
    cy = u[2] * v[0] - u[0] * v[2]
    cz = u[0] * v[1] - u[1] * v[0]
    return 0.25 * ((cx * cx + cy * cy) + cz * cz)


def forbidden(loop, faces, resident):
    """w(i, m, j) == +inf?"""
    L = len(loop)

    def diagonal_taken(x, y):
        if y - x == 1 or (x == 0 and y == L - 1):
            return False
        u, v = loop[x], loop[y]
        return faces.get((u, v) if u < v else (v, u), 0) > 0

    def bad(i, m, j):
        return frozenset((loop[i], loop[m], loop[j])) in resident or diagonal_taken(i, m) or diagonal_taken(m, j) or diagonal_taken(i, j)
    return bad


def triangulate(loop, q, bad):
    """(total, [(i, m, j)]) of the interval dynamic programme; total == inf: blocked, no triangles."""
    L = len(loop)
    W = [[0.0] * L for _ in range(L)]
    S = [[-1] * L for _ in range(L)]
    for d in range(2, L):
        for i in range(L - d):
            j = i + d
            best, at = math.inf, -1
            for m in range(i + 1, j):
                w = math.inf if bad(i, m, j) else float(weight(q, i, m, j))
                cand = (W[i][m] + W[m][j]) + w
                if cand < best:
                    best, at = cand, m
            W[i][j], S[i][j] = best, at
    if not math.isfinite(W[0][L - 1]):
        return math.inf, []
    out, stack = [], [(0, L - 1)]
    while stack:
        i, j = stack.pop()
        if j - i < 2:
            continue
        m = S[i][j]
        out.append((i, m, j))
        stack += [(i, m), (m, j)]
    return W[0][L - 1], out


def lowest_first(t):
    at = t.index(min(t))
    return t[at:] + t[:at]


def fill(points, fans, tri, max_vertices=32, max_perimeter=math.inf):
    """dict(patches (P, 3) int32 ascending, filled (T + P, 3) int32 ascending, loops: list of vertex lists in canonical
    order, status (loops,) uint8, perimeters (loops,) float64, totals: the dynamic programme's W[0][L - 1] per loop (nan
    where it was not run), stats: the eight figures of pct_fill_hole_stats by STAT_NAMES, rejected: walks rejected)."""
    p = np.asarray(points, np.float64)
    tri = np.asarray(tri, np.int32).reshape(-1, 3)
    faces = edge_count(tri)
    resident = {frozenset(t) for t in tri.tolist()}
    stored = {}
    for t in tri.tolist():
        for x, y in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            stored.setdefault((min(x, y), max(x, y)), []).append((x, y))
    gaps, odd = gaps_of(fans, tri)
    loops, status, perimeters, totals, patches = [], [], [], [], []
    rejected = 0
    for v0, mine in enumerate(gaps):
        for a, b in mine:
            verts = walk(gaps, v0, a, b, max_vertices)
            if verts is None:
                rejected += 1
                continue
            if min(verts) != v0:
                continue
            loop = verts if b < a else [v0] + verts[:0:-1]
            w = loop[1]
            q = p[loop]
            per = perimeter_of(q)
            loops.append(loop)
            perimeters.append(per)
            if not per < max_perimeter:
                status.append(PERIMETER)
                totals.append(math.nan)
                continue
            total, tris = triangulate(loop, q, forbidden(loop, faces, resident))
            totals.append(total)
            if not tris:
                status.append(BLOCKED)
                continue
            status.append(FILLED)
            along = stored.get((v0, w), [])                      # (v0 < w: the loop's lowest vertex)
            reverse = len(along) == 1 and along[0] == (v0, w)
            for i, m, j in tris:
                t = lowest_first([loop[i], loop[m], loop[j]])
                patches.append((t[0], t[2], t[1]) if reverse else tuple(t))
    patches.sort()
    patches = np.asarray(patches, np.int32).reshape(-1, 3)
    filled = sorted(tri.tolist() + patches.tolist())
    status = np.asarray(status, np.uint8)
    stats = dict(zip(STAT_NAMES, (boundary_edges(tri), sum(len(g) for g in gaps), odd, len(loops), int((status == FILLED).sum()),
                                  int((status == PERIMETER).sum()), int((status == BLOCKED).sum()), len(patches))))
    return dict(patches=patches, filled=np.asarray(filled, np.int32).reshape(-1, 3), loops=loops, status=status,
                perimeters=np.asarray(perimeters, np.float64), totals=np.asarray(totals, np.float64), stats=stats, rejected=rejected)


def loops_csr(loops):
    off = np.zeros(len(loops) + 1, np.int64)
    off[1:] = np.cumsum([len(l) for l in loops])
    return off, np.asarray([v for l in loops for v in l], np.int32)


def brute_force_minimum(q, bad):
    """The least total weight over every triangulation of the polygon q (small L), each one enumerated as a tree (apex m
    over the edge (i, j), a tree on either side) and summed in the tree's own order -- Catalan(L - 2) of them."""
    def trees(i, j):
        if j - i < 2:
            yield None
            return
        for m in range(i + 1, j):
            for left in trees(i, m):
                for right in trees(m, j):
                    yield (i, m, j, left, right)

    def total(t):
        if t is None:
            return 0.0
        i, m, j, left, right = t
        w = math.inf if bad(i, m, j) else float(weight(q, i, m, j))
        return (total(left) + total(right)) + w
    every = [total(t) for t in trees(0, len(q) - 1)]
    return min(every), len(every)


def mesh_area(points, tri):
    p = np.asarray(points, np.float64)
    a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    return float(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum())

"""Consistent normal orientation over the neighbour graph, the restatement  --  TEST INFRASTRUCTURE ONLY (CPU, NumPy, no import
of the package).

``pct_orient_frames`` (include/pct_hip.h) turns the normals ``pct_point_frames`` left so that neighbouring rows agree, by a
level-synchronous flood over the resident k-NN table.  Every choice is a keyed 64-bit maximum, so the result is a pure
function of the unoriented normals and the table; ``orient`` states it again, and the device is held to it bit for bit
(tests/test_gpu_orient.py).

  valid     a row whose normal holds no NaN.  Invalid rows are never labelled, never parents, and keep every output.
  entries   of row i: idx[i, j] for j < count_i with 0 <= idx[i, j] < n.  i ~ j when j is an entry of row i or i one of row j.
  claim     a labelled row p on an unlabelled valid row c:
              dot = (n_p0 n_c0 + n_p1 n_c1) + n_p2 n_c2          float64, each product and sum rounded on its own
              key = (uint64(bits of float32(|dot|)) << 32) | (0xFFFFFFFF - p)
            the largest key wins (the best aligned parent, the lowest index among equals); the child takes
            toggle[c] = toggle[p] ^ (dot < 0), parent p, level[p] + 1 and p's component
  flood     until no unlabelled valid row is left or ``max_components`` components exist:
              seed   the unlabelled valid row of lowest index: toggle 0, level 0, parent -1, the next component id
              push   every row labelled in the previous level claims the unlabelled valid entries of its own row; all
                     claims of a level are in before any is decided; until a level labels nothing
              pull   once: every unlabelled valid row claims for itself from the entries of its own row that carry this
                     component's id, the entry as parent.  Rows labelled: they are the next frontier, push again.
                     None: the component is complete.
  anchor    per component.  SEED: as flooded.  TOP: the row of largest float32 z (-0 = +0), lowest index among equals;
            its oriented normal has n_z < 0: the component's toggles are inverted.  VIEW: with the oriented normal,
            s = ((vx - px) n0 + (vy - py) n1) + (vz - pz) n2, p in the cloud's dtype; rows with s < 0 face away, rows with
            s > 0 face the viewpoint; more away than facing: inverted; a tie leaves it.
  apply     rows with toggle 1: n <- -n, (k1, k2) <- (-k2, -k1), (d1, d2) <- (d2, d1), flipped ^= 1
  outputs   component, parent, level (int32; -1 where unlabelled; the seed's parent is -1), toggled (uint8, after the anchor)
"""
import numpy as np

SEED, TOP, VIEW = 0, 1, 2
ANCHORS = {"seed": SEED, "top": TOP, "view": VIEW}
MAX_COMPONENTS = 65536
LOW = np.uint64(0xFFFFFFFF)


def dots(N, P, C):
    return (N[P, 0] * N[C, 0] + N[P, 1] * N[C, 1]) + N[P, 2] * N[C, 2]


def keys(N, P, C):
    bits = np.abs(dots(N, P, C)).astype(np.float32).view(np.uint32).astype(np.uint64)
    return (bits << np.uint64(32)) | (LOW - P.astype(np.uint64))


def entry_mask(idx, count, n):
    idx = np.asarray(idx)
    k = idx.shape[1]
    count = np.full(len(idx), k) if count is None else np.minimum(np.asarray(count), k)
    return (np.arange(k)[None, :] < count[:, None]) & (idx >= 0) & (idx < n)


def orient(normals, idx, count=None, anchor=TOP, points=None, viewpoint=None, max_components=None):
    """dict(component, parent, level int32 (n), toggled uint8 (n), stats dict(valid, components, unlabelled, toggled,
    levels, pulls)).  ``points``: the cloud in its own dtype (TOP reads its float32 z, VIEW its coordinates)."""
    N = np.asarray(normals, np.float64)
    idx = np.asarray(idx).astype(np.int64)
    n, k = idx.shape
    anchor = ANCHORS.get(anchor, anchor)
    cap = MAX_COMPONENTS if max_components is None or max_components <= 0 else int(max_components)
    ok = entry_mask(idx, count, n)
    valid = ~np.isnan(N).any(1)
    comp = np.full(n, -1, np.int32)
    parent = np.full(n, -1, np.int32)
    level = np.full(n, -1, np.int32)
    toggle = np.zeros(n, np.uint8)
    levels = pulls = 0

    def decide(P, C, cid):
        """Claims (parent P[i] on child C[i]) -> the children labelled."""
        if len(C) == 0:
            return C
        key = keys(N, P, C)
        order = np.lexsort((key, C))
        C, key = C[order], key[order]
        last = np.r_[C[1:] != C[:-1], True]
        c, p = C[last], (LOW - (key[last] & LOW)).astype(np.int64)
        toggle[c] = toggle[p] ^ (dots(N, p, c) < 0)
        comp[c], parent[c], level[c] = cid, p, level[p] + 1
        return c

    cid = 0
    while cid < cap:
        rest = np.flatnonzero(valid & (comp < 0))
        if len(rest) == 0:
            break
        seed = rest[0]
        comp[seed], level[seed], toggle[seed] = cid, 0, 0
        front = np.array([seed])
        while True:
            while len(front):
                m = ok[front]
                P, C = np.repeat(front, k)[m.ravel()], idx[front][m]
                take = valid[C] & (comp[C] < 0)
                front = decide(P[take], C[take], cid)
                levels += len(front) > 0
            U = np.flatnonzero(valid & (comp < 0))
            m = ok[U]
            C, P = np.repeat(U, k)[m.ravel()], idx[U][m]
            take = comp[P] == cid
            front = decide(P[take], C[take], cid)
            if len(front) == 0:
                break
            pulls += 1
        cid += 1

    # ---- the anchor ----------------------------------------------------------------------------------------------------
    invert = np.zeros(max(cid, 1), bool)
    labelled = comp >= 0
    if anchor == TOP:
        z = np.asarray(points)[:, 2].astype(np.float32) + np.float32(0.0)
        for c in range(cid):
            rows = np.flatnonzero(comp == c)
            top = rows[np.argmax(z[rows])]                        # (the first among equals: the lowest index)
            nz = -N[top, 2] if toggle[top] else N[top, 2]
            invert[c] = nz < 0
    elif anchor == VIEW:
        p = np.asarray(points)
        v = np.asarray(viewpoint, np.float64).reshape(3)
        sign = np.where(toggle.astype(bool), -1.0, 1.0)
        with np.errstate(invalid="ignore"):
            s = ((v[0] - p[:, 0].astype(np.float64)) * (sign * N[:, 0]) + (v[1] - p[:, 1].astype(np.float64)) * (sign * N[:, 1])) + \
                (v[2] - p[:, 2].astype(np.float64)) * (sign * N[:, 2])
        for c in range(cid):
            rows = comp == c
            invert[c] = int((s[rows] < 0).sum()) > int((s[rows] > 0).sum())
    elif anchor != SEED:
        raise ValueError("unknown anchor")
    toggled = toggle.copy()
    toggled[labelled] ^= invert[comp[labelled]].astype(np.uint8)
    stats = dict(valid=int(valid.sum()), components=cid, unlabelled=int((valid & ~labelled).sum()), toggled=int(toggled.sum()),
                 levels=int(levels), pulls=int(pulls))
    return dict(component=comp, parent=parent, level=level, toggled=toggled, stats=stats)


def apply(normal, k12, dirs, flipped, toggled):
    """The frames after the call: rows ``toggled`` turned as frame_exact.flip turns one."""
    t = np.asarray(toggled).astype(bool)
    normal, k12, dirs = normal.copy(), k12.copy(), dirs.copy()
    normal[t] = -normal[t]
    k12[t] = -k12[t][:, ::-1]
    dirs[t] = dirs[t][:, :, ::-1]
    return normal, k12, dirs, (np.asarray(flipped).astype(np.uint8) ^ t.astype(np.uint8))


def check_tree(res, normals, idx, count=None):
    """The invariants every result keeps; returns the number of labelled non-seed rows."""
    N = np.asarray(normals, np.float64)
    comp, parent, level, n = res["component"], res["parent"], res["level"], len(N)
    ok = entry_mask(idx, count, n)
    kids = np.flatnonzero(parent >= 0)
    p = parent[kids].astype(np.int64)
    assert (comp[kids] >= 0).all() and np.array_equal(comp[p], comp[kids]) and np.array_equal(level[p] + 1, level[kids])
    seeds = np.flatnonzero((comp >= 0) & (parent < 0))
    assert (level[seeds] == 0).all() and np.array_equal(np.sort(comp[seeds]), np.arange(res["stats"]["components"]))
    assert ((comp < 0) == (level < 0)).all() and (parent[comp < 0] < 0).all()
    # an edge of the graph joins the two: c is an entry of p's row or p one of c's
    idx = np.asarray(idx)
    joined = ((idx[p] == kids[:, None]) & ok[p]).any(1) | ((idx[kids] == p[:, None]) & ok[kids]).any(1)
    assert joined.all()
    return len(kids)


def seed_toggles(res, normals):
    """Toggles as flooded (the anchor's inversion taken out): toggle[c] == toggle[p] ^ (dot < 0) along every tree edge."""
    N = np.asarray(normals, np.float64)
    comp, parent, t = res["component"], res["parent"], res["toggled"].astype(bool)
    kids = np.flatnonzero(parent >= 0)
    p = parent[kids].astype(np.int64)
    return np.array_equal(t[kids], t[p] ^ (dots(N, p, kids) < 0))       # (an inversion of a whole component cancels)


# ======================================================================================================================
# the clouds of the closed-form table, and their analytic outward normals
# ======================================================================================================================
def _fibonacci(n):
    i = np.arange(n, dtype=np.float64) + 0.5
    phi = np.arccos(1.0 - 2.0 * i / n)
    theta = np.pi * (1.0 + 5.0 ** 0.5) * i
    return np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], 1)


TWO_N, TWO_GAP = (1000, 600), 3.0
OUTLIERS = np.array([[6.0, 0.25, 0.5], [6.0, 0.25, 0.625]])


def two_spheres():
    """Unit Fibonacci spheres of 1 000 and 600 points, centres 3 apart along x: two components at k = 16."""
    b = _fibonacci(TWO_N[1])
    b[:, 0] += TWO_GAP
    return np.concatenate([_fibonacci(TWO_N[0]), b]).astype(np.float32)


def two_spheres_outward(pts):
    c = np.zeros((len(pts), 3))
    c[TWO_N[0]:, 0] = TWO_GAP
    return pts.astype(np.float64) - c


def sphere_with_outliers(n=2000):
    """The Fibonacci sphere and two points far off it, which list sphere points while no sphere point lists them: only a
    pull round reaches them."""
    return np.concatenate([_fibonacci(n), OUTLIERS]).astype(np.float32)


def torus_outward(pts, R=1.0):
    p = pts.astype(np.float64)
    th = np.arctan2(p[:, 1], p[:, 0])
    return p - np.stack([R * np.cos(th), R * np.sin(th), np.zeros(len(p))], 1)


def against(normal, outward):
    """Rows whose normal does not point to the outward side: n . N <= 0 (NaN rows are not counted)."""
    with np.errstate(invalid="ignore"):
        return int(((normal * outward).sum(1) <= 0).sum())

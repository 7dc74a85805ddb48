"""Exact ground truth for the kernels around the path  --  TEST INFRASTRUCTURE ONLY (CPU, no GPU, no import of the package).

pct_mesh.hip (mesh energies) and the voxel half of pct_aux.hip were compared with the NumPy restatement at a few
comfortable sizes and one absolute tolerance.  This module supplies, as fit_exact.py and eig_exact.py do for the fit and
the eigen stages: the cases (goldens of a reference run, launch edges, slivers), a reference MORE precise than either
side, and bars derived from the arithmetic, with the derivation next to every constant.

Mesh energies (utils.py:702-765)
--------------------------------
    term_t = widen(mean_dtype(X[tri_t])) * area_t,    bending: X = H**2 (squared in H's dtype), stretching: X = K,
    area_t = 0.5 |(v1 - v0) x (v2 - v0)|,             sums: nansum, nansum, sum.

``face_means``   the means as the reference defines them: ((x0 + x1) + x2) / 3 in the array's OWN dtype (np.mean of three
                 elements of a float32 array adds and divides in float32), widened to float64.  K and H each in its dtype.
``exact_areas``  the area of the float64 vertices at face value: cross product over ``fractions``, root by ``mpmath``
                 (50 digits), rounded once to float64.
``exact_energies``  per-triangle terms f * A (NaN terms dropped, as nansum does AFTER the product), summed by math.fsum.
``fsum_energies``   the same with the vectorised float64 area, for launch-edge meshes too large for rational arithmetic.

The bar (``bars``), u = 2^-53.  Write a = v1 - v0, b = v2 - v0 (exact), c = a x b, A = |c| / 2.

  area of one triangle.  The two edge subtractions round each component once: a^ = a (1 + d), |d| <= u.  A cross
      component is fl(fl(a^y b^z) - fl(a^z b^y)): every product carries the two subtraction errors and its own, the
      difference one more -- (1 + u)^4 on each of the two products, so  |c^x - cx| <= 4u (|ay||bz| + |az||by|) =: 4u Mx,
      and the same for y, z.  This is in |a|, |b| componentwise, NOT in the area: on a sliver Mx is 1e12 times cx.
      ||c^| - |c|| <= |c^ - c| <= 4u |M|.
      The norm fl(sqrt(fl(fl(cx^2 + cy^2) + cz^2))): squares 1u, two additions 2u on the radicand, halved by the root
      (1.5u), the root itself at most one ulp = 2u (the device's and NumPy's are correctly rounded: 1u; the bar does not
      rely on it): 3.5u |c^|.  The final * 0.5 is exact.  First order:
          dA_t = u (2 |M_t| + 3.5 A_t)                                                         AREA_CROSS = 2, AREA_NORM = 3.5
  one term.  fl(f * A^):  |p^ - f A| <= |f| (dA + u A).                                         (f is the same float64
      number on both sides: the means are taken exactly as the reference defines them.)
  the sums.  A value that passes through at most ``depth`` additions of a summation tree picks up (1 + u)^depth:
          |S^ - sum p^| <= depth u sum |p^|.
      depth of k_mesh_energy + k_mesh_final (``kernel_depth``): iterations of the grid-stride loop per thread, 6 xor-shuffle
      levels, 4 waves added in order, nblk block partials added in order.
  the reference's own rounding.  Every exact term is rounded to float64 once (u |term|) and fsum rounds the exact sum
      once (u |S| <= u sum |term|):  2u sum |term|.                                             REF_ROUNDING = 2
      With the float64 area (``fsum_energies``) the reference's terms carry dA_t and the product's u as well: the area
      and product part of the bar is counted twice (``area_sides=2``).
  higher order.  Everything above is first order in u.  The neglected terms are at most depth u times the first-order
      ones -- depth <= 2^11 here, so 2^-42 -- and the bar's own float64 evaluation adds a few u: HIGHER = 1 + 2^-20 covers
      both by twenty binary orders and is invisible in any comparison.

Non-finite sums (an infinite curvature on a triangle of positive area) have no bar: they are compared as values
(inf, -inf, NaN) with the reference run.

Voxel down-sampling (convert_asc_to_ply.py:20-51)
-------------------------------------------------
``first_occurrence``  np.unique over the int32 voxel rows, first index of every voxel, sorted: a vectorised statement of
                 "the first point of every voxel in order of first occurrence" that shares no code with the dict loop of
                 oracle.voxel_downsample (tests/test_aux_exact.py holds the two against each other on the goldens).
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
AREA_CROSS = 2.0             # 0.5 * 4u |M|
AREA_NORM = 3.5              # (1.5 + 2) u |c| / 2, in units of A
REF_ROUNDING = 2.0
HIGHER = 1.0 + 2.0 ** -20

MESH_BLOCK = 256             # kMeshBlock, pct_mesh.hip
MESH_BLOCKS_MAX = 1024       # pct_mesh_energies caps the launch here: one pass of the grid-stride loop covers 262 144 triangles
MESH_STRIDE = MESH_BLOCK * MESH_BLOCKS_MAX

NAMES = ("bending", "stretching", "area")


# ======================================================================================================================
# launch geometry of k_mesh_energy
# ======================================================================================================================
def kernel_blocks(T):
    return min((T + MESH_BLOCK - 1) // MESH_BLOCK, MESH_BLOCKS_MAX)


def kernel_depth(T):
    """Most additions any term passes through: loop iterations of its thread + 6 shuffle levels + 4 waves + nblk."""
    nblk = max(kernel_blocks(T), 1)
    iters = (T + nblk * MESH_BLOCK - 1) // (nblk * MESH_BLOCK)
    return iters + 6 + 4 + nblk


# ======================================================================================================================
# the terms as the reference defines them
# ======================================================================================================================
def _mean3(x, tri):
    """np.mean(x[tri]) of three elements in x's own dtype -- ((x0 + x1) + x2) / 3 -- widened to float64."""
    x = np.asarray(x)
    if x.dtype not in (np.float32, np.float64):
        x = x.astype(np.float64)
    with np.errstate(all="ignore"):
        s = (x[tri[:, 0]] + x[tri[:, 1]]) + x[tri[:, 2]]
        return (s / x.dtype.type(3)).astype(np.float64)


def face_means(tri, K, H):
    """(mean(H**2), mean(K)) per triangle, each in its array's dtype, float64 out."""
    H = np.asarray(H)
    with np.errstate(all="ignore"):
        H2 = H * H                                                 # utils.py:743, in H's dtype
    return _mean3(H2, tri), _mean3(K, tri)


def edge_products(v, tri):
    """|M_t| of the derivation: the norm of (|ay||bz| + |az||by|, |az||bx| + |ax||bz|, |ax||by| + |ay||bx|)."""
    v = np.asarray(v, np.float64)
    a = np.abs(v[tri[:, 1]] - v[tri[:, 0]])
    b = np.abs(v[tri[:, 2]] - v[tri[:, 0]])
    M = np.stack([a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]], 1)
    return np.sqrt((M * M).sum(1))


def float64_areas(v, tri):
    """The vectorised float64 area (same formula, NumPy's rounding)."""
    v = np.asarray(v, np.float64)
    c = np.cross(v[tri[:, 1]] - v[tri[:, 0]], v[tri[:, 2]] - v[tri[:, 0]])
    return 0.5 * np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])


def exact_areas(v, tri):
    """0.5 |(v1 - v0) x (v2 - v0)| of the float64 vertices taken at face value, correctly rounded to float64."""
    import mpmath
    v = np.asarray(v, np.float64)
    fr = [[Fraction(float(x)) for x in row] for row in v]
    out = np.empty(len(tri), np.float64)
    with mpmath.workdps(50):
        for t, (i0, i1, i2) in enumerate(np.asarray(tri).tolist()):
            a = [fr[i1][j] - fr[i0][j] for j in range(3)]
            b = [fr[i2][j] - fr[i0][j] for j in range(3)]
            c = (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
            n2 = c[0] * c[0] + c[1] * c[1] + c[2] * c[2]
            out[t] = float(mpmath.sqrt(mpmath.mpf(n2.numerator) / mpmath.mpf(n2.denominator)) / 2) if n2 else 0.0
    return out


def _terms(f, areas):
    """f * A with nansum's rule: a NaN PRODUCT is dropped (a NaN mean; an infinite mean on a zero area)."""
    with np.errstate(all="ignore"):
        p = f * areas
    return np.where(np.isnan(p), 0.0, p)


def _energies(v, tri, K, H, areas):
    tri = np.asarray(tri).reshape(-1, 3)
    fh2, fk = face_means(tri, K, H)
    pb, ps = _terms(fh2, areas), _terms(fk, areas)
    facts = dict(areas=areas, fh2=fh2, fk=fk, pb=pb, ps=ps, M=edge_products(v, tri), T=len(tri))
    with np.errstate(all="ignore"):
        sums = tuple(math.fsum(x) if np.isfinite(x).all() else float(np.sum(x)) for x in (pb, ps, areas))
    return sums, facts


def exact_energies(v, tri, K, H):
    """((bending, stretching, area), facts) with rational areas -- meshes up to a few thousand triangles."""
    tri = np.asarray(tri).reshape(-1, 3)
    return _energies(v, tri, K, H, exact_areas(v, tri))


def fsum_energies(v, tri, K, H):
    """The same with the float64 area: hold it to ``bars(facts, area_sides=2)``."""
    tri = np.asarray(tri).reshape(-1, 3)
    return _energies(v, tri, K, H, float64_areas(v, tri))


def bars(facts, area_sides=1, depth=None):
    """(bar bending, bar stretching, bar area) for sums that are finite; see the module docstring."""
    A, M = facts["areas"], facts["M"]
    depth = kernel_depth(facts["T"]) if depth is None else depth
    dA = U * (AREA_CROSS * M + AREA_NORM * A)
    out = []
    for f, p in ((facts["fh2"], facts["pb"]), (facts["fk"], facts["ps"]), (None, A)):
        if f is None:
            per_term, mag = dA, A
        else:
            live = np.isfinite(f)
            w = np.where(live, np.abs(f), 0.0)
            per_term, mag = w * (dA + U * A), np.abs(p)
        s = math.fsum(mag)
        out.append(HIGHER * (area_sides * math.fsum(per_term) + (depth + REF_ROUNDING) * U * s))
    return tuple(out)


def shares(got, want, bar):
    """|got - want| / bar per sum (0 / 0 = 0: an exact zero against a zero bar is met)."""
    out = []
    for g, w, b in zip(got, want, bar):
        e = abs(float(g) - float(w))
        out.append(0.0 if e == 0 else (e / b if b > 0 else math.inf))
    return out


def same_values(got, want):
    """Non-finite sums: identical as values (inf, -inf, NaN), finite ones left to the bar."""
    return all((math.isnan(g) and math.isnan(w)) or g == w or (math.isfinite(g) and math.isfinite(w)) for g, w in zip(got, want))


# ======================================================================================================================
# the kernel's summation, restated in NumPy: used to show that the bars hold for its tree and that defects do not pass
# ======================================================================================================================
def emulate_kernel(v, tri, K, H, defect=None):
    """k_mesh_energy + k_mesh_final in float64 NumPy, same tree.  ``defect``:
    'mean64'      face means taken in float64 whatever the arrays' dtype
    'mean_sq'     (mean H)^2 instead of mean(H^2)
    'nan_first'   NaN means replaced by 0 BEFORE the product (inf * 0 then stays in the sum)
    'drop_tail'   the last, partial pass of the grid-stride loop is not run
    'drop_block'  the partial sums of one block (the middle one) are left out"""
    tri = np.asarray(tri).reshape(-1, 3)
    T = len(tri)
    if T == 0:
        return 0.0, 0.0, 0.0
    K, H = np.asarray(K), np.asarray(H)
    if defect == "mean64":
        K, H = K.astype(np.float64), H.astype(np.float64)
    A = float64_areas(v, tri)
    fh2, fk = face_means(tri, K, H)
    if defect == "mean_sq":
        with np.errstate(all="ignore"):
            fh2 = _mean3(H, tri) ** 2
    with np.errstate(all="ignore"):
        if defect == "nan_first":
            pb, ps = np.where(np.isnan(fh2), 0.0, fh2) * A, np.where(np.isnan(fk), 0.0, fk) * A
        else:
            pb, ps = _terms(fh2, A), _terms(fk, A)
    nblk = kernel_blocks(T)
    stride = nblk * MESH_BLOCK
    iters = (T + stride - 1) // stride
    if defect == "drop_tail" and T % stride:
        iters -= 1
    out = []
    with np.errstate(all="ignore"):
        for x in (pb, ps, A):
            pad = np.zeros(max(iters, 0) * stride)
            m = min(T, len(pad))
            pad[:m] = x[:m]
            acc = np.zeros(stride)
            for it in range(iters):                                   # the thread's loop, in order
                acc = acc + pad[it * stride:(it + 1) * stride]
            lanes = acc.reshape(nblk, MESH_BLOCK // 64, 64)
            for o in (32, 16, 8, 4, 2, 1):                            # __shfl_xor butterfly
                lanes = lanes + lanes[:, :, np.arange(64) ^ o]
            waves = lanes[:, :, 0]
            block = np.zeros(nblk)
            for w in range(MESH_BLOCK // 64):
                block = block + waves[:, w]
            s = 0.0
            for b in range(nblk):
                if defect == "drop_block" and b == nblk // 2:
                    continue
                s = s + block[b]
            out.append(float(s))
    return tuple(out)


DEFECTS = ("mean64", "mean_sq", "nan_first", "drop_tail", "drop_block")


# ======================================================================================================================
# meshes
# ======================================================================================================================
def icosphere(levels):
    t = (1 + 5 ** 0.5) / 2
    v = [np.array(p, float) for p in ([-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                                      [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1])]
    v = [p / np.linalg.norm(p) for p in v]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    for _ in range(levels):
        cache, nf = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = (v[a] + v[b]) / 2
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    return np.array(v), np.array(f, np.int32)


def random_mesh(seed, nv, nt, dtype=np.float64, nans=0):
    """Vertices ~ N(0, 1), index triples with repeats allowed, curvatures ~ N(0, 1) with ``nans`` NaNs in each."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(nv, 3))
    t = rng.integers(0, nv, size=(nt, 3)).astype(np.int32)
    K, H = rng.normal(size=nv).astype(dtype), rng.normal(size=nv).astype(dtype)
    if nans:
        K[rng.integers(0, nv, nans)] = np.nan
        H[rng.integers(0, nv, nans)] = np.nan
    return v, t, K, H


N_GUARDED = 8


def nonfinite_mesh(seed=12, nv=400, nt=1500):
    """random_mesh with NaN curvatures anywhere and +-inf curvatures on the last N_GUARDED vertices, which only triangles
    of exactly zero area touch ((i, i, j), (i, j, j), (i, j, i), (i, i, i): one edge is exactly zero or the two are the
    same vector, so every cross component is x y - y x = 0): inf * 0 = NaN, dropped by nansum AFTER the product.
    float64 curvatures; the float32 case is their rounding."""
    rng = np.random.default_rng(seed)
    live = nv - N_GUARDED
    v, t, K, H = random_mesh(seed, live, nt, nans=12)
    v = np.vstack([v, rng.normal(size=(N_GUARDED, 3))])
    K = np.concatenate([K, [np.inf, -np.inf, np.inf, 1.5, np.nan, -np.inf, np.inf, -2.0]])
    H = np.concatenate([H, [0.5, np.inf, -np.inf, np.inf, -np.inf, np.nan, 3.0, -np.inf]])
    extra = []
    for g in range(live, nv):
        j = int(rng.integers(0, live))
        extra += [[g, g, j], [g, j, j], [j, g, j], [g, g, g], [j, j, g]]
    t = np.vstack([t, np.array(extra, np.int32)])
    return v, t[rng.permutation(len(t))], K, H


def live_inf_mesh(seed=13):
    """Infinite curvatures on triangles of positive area: the sums themselves are inf / NaN (compared as values)."""
    v, t, K, H = random_mesh(seed, 60, 200)
    K[[3, 17]] = np.inf, -np.inf                                     # inf - inf: NaN stretching
    H[5] = -np.inf                                                    # H^2 = +inf: inf bending
    return v, t, K, H


def zero_area_mesh():
    """Every area exactly zero: collinear integer vertices and repeated indices (utils.py:731-733 returns 0, 0, 0)."""
    v = np.array([[i, 2.0 * i, -3.0 * i] for i in range(12)])
    t = np.array([[0, 1, 2], [3, 7, 11], [4, 4, 9], [5, 6, 5], [10, 2, 2], [1, 8, 3]], np.int32)
    K = np.linspace(-1, 1, 12).astype(np.float32)
    return v, t, K, (K * 2).astype(np.float32)


SLIVER_ASPECTS = tuple(10.0 ** e for e in range(0, 13))


def sliver_mesh(seed=14, per_aspect=8, offset=(0.0, 0.0, 0.0)):
    """Triangles (0, 0, 0), (1, 0, 0), (x, 1 / aspect, 0) in a random frame each, aspect 1 ... 1e12: the cross product
    cancels to 1 / aspect of its operands.  Curvatures float32, order one."""
    rng = np.random.default_rng(seed)
    vs, ts = [], []
    for aspect in SLIVER_ASPECTS:
        for _ in range(per_aspect):
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            local = np.array([[0, 0, 0], [1, 0, 0], [rng.uniform(0.2, 0.8), 1.0 / aspect, 0]])
            ts.append([len(vs) * 3, len(vs) * 3 + 1, len(vs) * 3 + 2])
            vs.append(local @ q.T * rng.uniform(0.5, 2.0) + rng.normal(size=3) + np.asarray(offset))
    v = np.vstack(vs)
    K = rng.normal(size=len(v)).astype(np.float32)
    H = rng.normal(size=len(v)).astype(np.float32)
    return v, np.array(ts, np.int32), K, H


# launch edges of k_mesh_energy: one thread, a partial wave, one block exactly, one more, the cap of the launch exactly
# (1024 blocks, one pass), one triangle into the second pass, and two full passes plus a partial third one
EDGE_T = (1, 255, 256, 257, MESH_STRIDE, MESH_STRIDE + 1, 2 * MESH_STRIDE + 300)
EXACT_T_MAX = 2000          # rational areas up to here, the float64 area with area_sides=2 above


def edge_mesh(T, dtype):
    """A closed-form mesh of T triangles for the launch edges: nv = min(T + 2, 3001) vertices."""
    v, t, K, H = random_mesh(1000 + T % 977, min(T + 2, 3001), T, dtype=dtype, nans=min(T // 64, 30))
    return v, t, K, H


def reference_energies(v, tri, K, H):
    """exact_energies where the mesh is small enough, else fsum_energies.  Returns (sums, facts, area_sides)."""
    if len(tri) <= EXACT_T_MAX:
        return exact_energies(v, tri, K, H) + (1,)
    return fsum_energies(v, tri, K, H) + (2,)


def numpy_energies(v, tri, K, H):
    """utils.py:723-760 vectorised (np.cross, np.linalg.norm, np.nansum, np.sum): the reference's arithmetic on meshes
    too large for its per-triangle loop."""
    v, tri = np.asarray(v), np.asarray(tri)
    areas = 0.5 * np.linalg.norm(np.cross(v[tri[:, 1]] - v[tri[:, 0]], v[tri[:, 2]] - v[tri[:, 0]]), axis=1)
    fh2, fk = face_means(tri, K, H)
    with np.errstate(all="ignore"):
        return float(np.nansum(fh2 * areas)), float(np.nansum(fk * areas)), float(np.sum(areas))


# ======================================================================================================================
# golden cases (oracle/make_goldens_energies.py writes them, the tests read them)
# ======================================================================================================================
GOLDEN = "g12_energies.npz"
GOLDEN_CASES = ("icosphere_f32", "random_f32", "random_f64", "mixed_K64_H32", "mixed_K32_H64", "no_curvatures", "zero_area",
                "slivers", "live_inf")


def golden_inputs():
    """{case: (vertices, triangles, K or None, H or None)} -- K is None where point_data carries no curvatures."""
    v, t = icosphere(2)
    rng = np.random.default_rng(11)
    cases = {"icosphere_f32": (v * 2.0, t, (0.25 + 0.01 * rng.normal(size=len(v))).astype(np.float32),
                               (0.5 + 0.01 * rng.normal(size=len(v))).astype(np.float32))}
    v, t, K, H = nonfinite_mesh()
    cases["random_f32"] = (v, t, K.astype(np.float32), H.astype(np.float32))
    cases["random_f64"] = (v, t, K, H)
    cases["mixed_K64_H32"] = (v, t, K, H.astype(np.float32))
    cases["mixed_K32_H64"] = (v, t, K.astype(np.float32), H)
    cases["no_curvatures"] = (v, t, None, None)
    cases["zero_area"] = zero_area_mesh()
    cases["slivers"] = sliver_mesh()
    cases["live_inf"] = live_inf_mesh()
    return cases


def golden_case(g, case):
    """(vertices, triangles, K, H, (bending, stretching, area) of the reference run) out of the loaded .npz."""
    mesh = str(g[f"{case}_mesh"]) if f"{case}_mesh" in g else case      # one mesh, several curvature dtypes: stored once
    v, t = g[f"{mesh}_v"], g[f"{mesh}_t"]
    if f"{case}_K" in g:
        K, H = g[f"{case}_K"], g[f"{case}_H"]
    else:
        K = H = None
    return v, t, K, H, tuple(float(x) for x in g[f"{case}_out"])


def curvatures_or_zeros(v, K, H):
    """utils.py:744-748: float64 zeros where point_data has no curvatures."""
    return (np.zeros(len(v)), np.zeros(len(v))) if K is None else (K, H)


# ======================================================================================================================
# voxel down-sampling
# ======================================================================================================================
def voxel_rows(coordinates, voxel_size):
    """convert_asc_to_ply.py:34, the definition of a point's voxel: the division in the array's dtype."""
    return np.floor(np.asarray(coordinates) / voxel_size).astype(np.int32)


def first_occurrence(coordinates, voxel_size):
    """Indices (int64, increasing) of the first point of every voxel."""
    _, first = np.unique(voxel_rows(coordinates, voxel_size), axis=0, return_index=True)
    return np.sort(first).astype(np.int64)


VOXEL_BLOCK = 256            # threads per block of the voxel kernels: one count per block goes into the scan
SCAN_PASS = 1024             # k_scan_int scans this many block counts per pass and carries into the next
N_THREE_PASSES = 2 * SCAN_PASS * VOXEL_BLOCK + VOXEL_BLOCK + 1        # 524 545 points: 2 050 block counts, passes of 1024, 1024, 2
VOXEL_SPAN_MAX = 1 << 21     # pct_voxel_downsample_device packs 21 bits per axis


def half_kept_cloud(dtype, n=N_THREE_PASSES, seed=31):
    """Uniform in the unit cube with the voxel edge at which about half the points are kept: a point is the first of its
    voxel with probability (1 - exp(-x)) / x, x = n * voxel^3 points per voxel; x = 1.594 gives 0.5."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, size=(n, 3)).astype(dtype), (1.594 / n) ** (1.0 / 3.0)


def one_voxel_cloud(dtype, n=N_THREE_PASSES, seed=32):
    rng = np.random.default_rng(seed)
    return (3.0 + rng.uniform(0.1, 0.9, size=(n, 3)) * 0.125).astype(dtype), 0.125       # all in voxel (24, 24, 24)


def lattice_cloud(dtype, n=N_THREE_PASSES, seed=33):
    """n points of a shuffled 81^3 lattice, voxel = the lattice constant (a power of two: the centres (i + 0.5) / 4 are
    exact in float32): every point its own voxel, the scan's total is n and its carry passes 2^18 after the first pass."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*(np.arange(-40, 41),) * 3, indexing="ij"), -1).reshape(-1, 3)
    assert len(g) >= n
    return ((g[rng.permutation(len(g))[:n]] + 0.5) * 0.25).astype(dtype), 0.25


def span_cloud(dtype, axis, span):
    """Three points, voxel 1: the first and the third share a voxel, the second lies ``span`` voxels further along
    ``axis`` (all coordinates exact in float32: below 2^22 with one binary digit behind the point)."""
    p = np.full((3, 3), 0.5)
    p[:, axis] = [-5.5, -6.0 + span + 0.5, -5.75]
    return p.astype(dtype), 1.0


def multiples_cloud(dtype, voxel):
    """Coordinates ON the voxel boundaries, both signs, and -0.0: the last bit of the quotient decides the voxel."""
    k = np.arange(-60, 61)
    ax = (k * dtype(voxel)).astype(dtype)
    g = np.stack(np.meshgrid(ax, ax[::7], np.array([-0.0, 0.0, -voxel, voxel], dtype), indexing="ij"), -1).reshape(-1, 3)
    return g[np.random.default_rng(34).permutation(len(g))].astype(dtype)


def offset_cloud(n=5000, seed=35):
    """float32, 1e5 from the origin, voxel 0.05: the coordinates' spacing is 2^-7 and the quotient (2e6) is spaced
    0.125 -- the float32 rounding of the division decides the voxel."""
    rng = np.random.default_rng(seed)
    return (1e5 + rng.uniform(0.0, 2.0, size=(n, 3))).astype(np.float32), 0.05

"""Goldens of the reference's PCA estimator, principal_curvatures_via_principal_component_analysis (pct:901-950).

TEST INFRASTRUCTURE, build container only:  MPLBACKEND=Agg python tools/make_goldens_pca.py   (~1 min)

Runs the UNMODIFIED reference method (imported by oracle/make_goldens.py::load_reference) and writes
tests/golden/g12_pca_<case>.npz: the input points, k, the five attributes it sets and `ambiguous` (N,) -- the k-th and
(k+1)-th distances of the row, computed as the reference computes them, lie within 4 float32 ulps (the k-th place is
then a near-tie that NumPy's unstable argsort decides).  Cases whose call raises store the exception's message instead.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from make_goldens import OUT, REF, load_reference, load_shapes  # noqa: E402

ATTRS = ("pca_principal_curvature_values_1", "pca_principal_curvature_values_2", "principal_curvature_directions",
         "pca_K_values", "pca_H_values")


def ambiguous(points, k):
    n = len(points)
    out = np.zeros(n, bool)
    if k + 1 >= n:
        return out
    for i in range(n):
        d = np.sort(np.linalg.norm(points - points[i], axis=1))           # as pct:914
        a, b = np.float32(d[k]), np.float32(d[k + 1])
        out[i] = abs(float(b) - float(a)) <= 4 * float(np.spacing(max(a, np.finfo(np.float32).tiny)))
    return out


def run(ref, name, k, points=None, file_rows=None):
    if file_rows is not None:
        path, rows = file_rows
        with open(path) as f:
            lines = [ln for ln in f if ln.strip()]
        with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as t:
            t.writelines(lines[i] for i in rows)
        pc = ref.PointCloud(t.name)                                       # the file constructor: float32 + max shift
        os.unlink(t.name)
    else:
        pc = ref.PointCloud(points=points, normals=np.zeros((len(points), 0)))
    rec = dict(points=np.asarray(pc.points), k=np.int32(k))
    try:
        pc.principal_curvatures_via_principal_component_analysis(k)
    except Exception as exc:                                              # k in {0, 1}: np.cov is NaN, eigh refuses it
        rec["error"] = np.array(f"{type(exc).__name__}: {exc}")
    else:
        for a in ATTRS:
            rec[a] = np.asarray(getattr(pc, a))
        rec["ambiguous"] = ambiguous(rec["points"], k)
    np.savez_compressed(os.path.join(OUT, f"g12_pca_{name}.npz"), **rec)
    print(name, "error" in rec and rec["error"] or int(rec["ambiguous"].sum()), flush=True)


def main():
    ref = load_reference()
    sh = load_shapes()
    run(ref, "sphere2k_k30", 30, sh.fibonacci_sphere(2000))
    run(ref, "torus4k_k50", 50, sh.torus_random(4000, seed=7))
    run(ref, "bunny4k_k20", 20, file_rows=(os.path.join(REF, "sample_scans", "bunny.txt"), range(4000)))
    run(ref, "torus3k_f64_k40", 40, sh.torus_random(3000, seed=11, dtype=np.float64) * 0.2 + 40.0)
    side = 316                                                            # egg_carton.txt: a 316 x 316 lattice, row-major
    block = [r * side + c for r in range(64) for c in range(64)]
    run(ref, "egg64_k30", 30, file_rows=(os.path.join(REF, "sample_scans", "egg_carton.txt"), block))
    rng = np.random.default_rng(12)
    dup = sh.torus_random(300, seed=13)
    dup = np.concatenate([dup, dup[rng.choice(300, 60, replace=False)]])[rng.permutation(360)]
    run(ref, "dups360_k12", 12, dup)
    run(ref, "n10_k15", 15, rng.normal(size=(10, 3)).astype(np.float32))
    run(ref, "torus500_k2", 2, sh.torus_random(500, seed=17))
    for k in (0, 1):
        run(ref, f"n10_k{k}", k, rng.normal(size=(10, 3)).astype(np.float32))


if __name__ == "__main__":
    main()

"""N3: mesh energy integrals, the consumer of the path's K/H (utils.py:702-765).

The restatement in oracle/pct_oracle.py is pinned by a run of the reference's own function body
(tests/golden/g12_energies.npz, tests/test_aux_exact.py) and, here, by the closed-form values the reference quotes for
its validation shapes (main_shape_validation.py:33-45: sphere bending 4*pi, stretching 4*pi).  The kernel's launch edges,
dtypes and bars: tests/test_gpu_aux.py.
"""
import types

import numpy as np
import pytest

import pct_oracle as oracle


def icosphere(levels=3):
    t = (1 + 5 ** 0.5) / 2
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], float)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
                  [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10],
                  [8, 6, 7], [9, 8, 1]])
    v /= np.linalg.norm(v, axis=1)[:, None]
    for _ in range(levels):
        cache, nf = {}, []
        v = list(v)

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = (np.asarray(v[a]) + np.asarray(v[b])) / 2
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        v, f = np.array(v), np.array(nf)
    return v, f


def test_oracle_sphere_known_answer():
    r = 2.0
    v, f = icosphere(4)
    K = np.full(len(v), 1 / r ** 2, np.float32)
    H = np.full(len(v), 1 / r, np.float32)
    bend, stretch, area = oracle.mesh_energies(v * r, f, K, H)
    assert abs(area - 4 * np.pi * r * r) / (4 * np.pi * r * r) < 3e-3          # inscribed polyhedron
    assert abs(bend - 4 * np.pi) / (4 * np.pi) < 3e-3                           # main_shape_validation.py:33-45
    assert abs(stretch - 4 * np.pi) / (4 * np.pi) < 3e-3


def _random_mesh(seed, nv=5000, nt=20000, dtype=np.float32):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(nv, 3))
    t = rng.integers(0, nv, size=(nt, 3)).astype(np.int32)
    K = rng.normal(size=nv).astype(dtype)
    H = rng.normal(size=nv).astype(dtype)
    K[rng.integers(0, nv, 40)] = np.nan                                         # nansum semantics (utils.py:755-756)
    H[rng.integers(0, nv, 40)] = np.nan
    return v, t, K, H


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_gpu_energies_match_oracle(gpu, dtype):
    from point_cloud_toolbox_amd.energies import mesh_energies
    v, t, K, H = _random_mesh(1, dtype=dtype)
    got = mesh_energies(v, t, K, H)
    ref = oracle.mesh_energies(v, t, K, H)
    for a, b in zip(got, ref):
        assert abs(a - b) <= 1e-11 * max(1.0, abs(b)), (got, ref)


@pytest.mark.gpu
def test_gpu_energies_sphere_and_wrapper(gpu):
    from point_cloud_toolbox_amd.energies import load_mesh_compute_energies
    v, f = icosphere(5)
    mesh = types.SimpleNamespace(points=v, faces=np.column_stack([np.full(len(f), 3), f]).ravel(),
                                 point_data={"gaussian_curvature": np.ones(len(v), np.float32),
                                             "mean_curvature": np.ones(len(v), np.float32)})
    bend, stretch, area = load_mesh_compute_energies(mesh)
    assert abs(bend - 4 * np.pi) < 0.02 and abs(stretch - 4 * np.pi) < 0.02 and abs(area - 4 * np.pi) < 0.02
    mesh.point_data = {}                                                         # utils.py:747-751: zeros
    bend, stretch, area = load_mesh_compute_energies(mesh)
    assert bend == 0 and stretch == 0 and abs(area - 4 * np.pi) < 0.02
    mesh.faces = np.zeros((0, 3), np.int32)
    assert load_mesh_compute_energies(mesh) == (0, 0, 0)                         # utils.py:711-713


@pytest.mark.gpu
def test_gpu_energies_reject_bad_triangles(gpu):
    from point_cloud_toolbox_amd.energies import mesh_energies
    v, t, K, H = _random_mesh(2, nv=100, nt=50)
    t[7, 1] = 100
    with pytest.raises(ValueError, match="outside"):
        mesh_energies(v, t, K, H)

"""Reference fixtures for the mesh energies, row N3 (build container only; TEST INFRASTRUCTURE).

utils.py does not import here (open3d / pyvista), so ONLY the definition of ``load_mesh_compute_energies``
(/root/reference/utils.py:702-765) is compiled out of the file -- located by name with ``ast``, source untouched, as
oracle/make_goldens_prep.py does -- and run on the meshes of tests/aux_exact.py::golden_inputs.  Its namespace gets
``np``, ``logging`` and our own stand-in for ``convert_pv_to_o3d``: an object with ``vertices``, ``triangles``,
``has_triangles()`` and ``compute_triangle_normals()`` (the function reads nothing else of the converted mesh).
Nothing but inputs and outputs is written to tests/golden/g12_energies.npz.  The function's loop is O(T^2): no mesh
here has more than 2 000 triangles.
Run from the repo root:  python oracle/make_goldens_energies.py
"""
import ast
import logging
import os
import sys
import types

import numpy as np

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import aux_exact as ax  # noqa: E402


class ConvertedMesh:
    """What convert_pv_to_o3d would hand over, as far as load_mesh_compute_energies looks at it."""

    def __init__(self, mesh):
        self.vertices = np.asarray(mesh.points, dtype=np.float64)           # o3d.utility.Vector3dVector: float64
        self.triangles = np.asarray(mesh.triangles, dtype=np.int32)         # o3d.utility.Vector3iVector: int32

    def has_triangles(self):
        return len(self.triangles) > 0

    def compute_triangle_normals(self):
        return self


def reference_function(path, name):
    src = open(path).read()
    tree = ast.parse(src)
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name)
    ns = {"np": np, "logging": logging, "convert_pv_to_o3d": ConvertedMesh}
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return ns[name], (node.lineno, node.end_lineno)


def main():
    fn, span = reference_function(os.path.join(REF, "utils.py"), "load_mesh_compute_energies")
    print("load_mesh_compute_energies at lines", span)
    out, stored = {}, {}
    for case, (v, t, K, H) in ax.golden_inputs().items():
        assert len(t) <= 2000
        pd = {} if K is None else {"gaussian_curvature": K, "mean_curvature": H}
        with np.errstate(all="ignore"):
            res = fn(types.SimpleNamespace(points=v, triangles=t, point_data=pd))
        shared = next((c for c, m in stored.items() if m[0] is v and m[1] is t), None)
        if shared is None:                                                # one mesh, several curvature dtypes: stored once
            out[f"{case}_v"], out[f"{case}_t"] = np.asarray(v, np.float64), np.asarray(t, np.int32)
            stored[case] = (v, t)
        else:
            out[f"{case}_mesh"] = np.array(shared)
        if K is not None:
            out[f"{case}_K"], out[f"{case}_H"] = K, H
        out[f"{case}_out"] = np.array(res, np.float64)
        print(case, len(t), "triangles", None if K is None else (K.dtype, H.dtype), "->", res)
    assert tuple(ax.GOLDEN_CASES) == tuple(ax.golden_inputs())
    path = os.path.join(OUT, ax.GOLDEN)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

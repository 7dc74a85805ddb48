"""ctypes binding of libpct_hip.so (C ABI: include/pct_hip.h).

There is no CPU fallback: if the shared library is missing or no gfx950
device is usable every entry point raises.  Build with
``python -c "import __graft_entry__ as g; g.build()"`` (drives hipcc).
"""
from __future__ import annotations

import ctypes as C
import atexit
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PCT_LIB") or os.path.join(_HERE, "libpct_hip.so")     # PCT_LIB: a developer's A/B build (tools/build_variant.py)

PCT_OK = 0
PCT_ERR_HIP = 1
PCT_ERR_NO_DEVICE = 2
PCT_ERR_INVALID = 3
PCT_ERR_NONFINITE = 4
PCT_ERR_K_TOO_LARGE = 5
PCT_ERR_OOM = 6
PCT_ERR_NO_NEIGHBORS = 7
PCT_ERR_LIMIT = 8

MESH_F32, MESH_F64, MESH_K64_H32, MESH_K32_H64 = 0, 1, 2, 3      # pct_mesh_energies' curvature_is_f64

KNN_AUTO, KNN_BRUTE, KNN_GRID, KNN_GRID_EXACT, KNN_GRID_LEVELS, KNN_TREE = 0, 1, 2, 3, 4, 5
ORIENT_SEED, ORIENT_TOP, ORIENT_VIEW = 0, 1, 2          # pct_orient_frames' anchors
TRI_WIND_FRAMES = 1                                     # pct_point_triangles' flag (include/pct_hip_surface.h)
ORIENT_ANCHORS = {"seed": ORIENT_SEED, "top": ORIENT_TOP, "view": ORIENT_VIEW}
QUERY_AUTO, QUERY_SWEEP, QUERY_GRID = 0, 1, 2                    # pct_query_points_algo, pct_query_ball
BALL_SORTED, BALL_DISTANCES, BALL_COUNT_ONLY = 1, 2, 4           # pct_query_ball's flags
NET_FAST1, NET_FAST2, NET_SETS1, NET_SETS2, NET_PAIR, NET_DUO = range(6)        # pct_selftest_sort's networks
NET_LIST = {NET_FAST1: 64, NET_FAST2: 128, NET_SETS1: 64, NET_SETS2: 128, NET_PAIR: 64, NET_DUO: 128}      # elements of a list
EXACT_ASCENDING, EXACT_DESCENDING, EXACT_MERGE_MIN = 0, 1, 2     # pct_selftest_sort_exact's modes


class Timings(C.Structure):
    _fields_ = [
        ("upload_ms", C.c_float), ("grid_ms", C.c_float), ("knn_ms", C.c_float), ("knn_fast_ms", C.c_float),
        ("fit_ms", C.c_float), ("export_ms", C.c_float), ("total_ms", C.c_float),
        ("knn_launches", C.c_int32), ("grid_iters", C.c_int32), ("redo_adopted", C.c_int32),
        ("cells", C.c_int64), ("occupied_cells", C.c_int64),
        ("ring_fallbacks", C.c_int64), ("lds_overflows", C.c_int64),
        ("flushes", C.c_int64), ("candidate_steps", C.c_int64), ("redone_queries", C.c_int64),
        ("cell_size", C.c_double),
        ("grid_points", C.c_int64), ("limit_retries", C.c_int32), ("levels", C.c_int32),
        ("occupancy", C.c_double),
        ("fit_svd_rows", C.c_int64),
        ("algo", C.c_int32), ("sweep_variant", C.c_int32),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


_p = C.c_void_p
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_f32p = C.POINTER(C.c_float)
_f64p = C.POINTER(C.c_double)
_u8p = C.POINTER(C.c_uint8)
_u32p = C.POINTER(C.c_uint32)

# name -> (restype, argtypes); every symbol declared in include/pct_hip.h and include/pct_hip_surface.h
SIGNATURES = {
    "pct_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "pct_create": (C.c_int, [C.c_int, C.POINTER(_p)]),
    "pct_destroy": (None, [_p]),
    "pct_last_error": (C.c_char_p, [_p]),
    "pct_version": (C.c_char_p, []),
    "pct_set_points_f32": (C.c_int, [_p, _f32p, C.c_int64]),
    "pct_set_points_f64": (C.c_int, [_p, _f64p, C.c_int64]),
    "pct_set_points_device_f32": (C.c_int, [_p, _p, C.c_int64]),
    "pct_use_points_device_f32": (C.c_int, [_p, _p, C.c_int64]),
    "pct_set_query_range": (C.c_int, [_p, C.c_int64, C.c_int64]),
    "pct_set_query_slab": (C.c_int, [_p, C.c_int32, C.c_int32]),
    "pct_slab_counts": (C.c_int, [_p, C.POINTER(C.c_int64), C.c_int32]),
    "pct_slab_records": (C.c_int, [_p, _p, C.c_int64, C.POINTER(C.c_int64)]),
    "pct_scatter_records": (C.c_int, [_p, _p, C.c_int64, C.c_int64, C.c_int64, _p, _p]),
    "pct_set_grid_param": (C.c_int, [_p, C.c_double]),
    "pct_set_async": (C.c_int, [_p, C.c_int32]),
    "pct_get_timings_done": (C.c_int, [_p, C.POINTER(Timings)]),
    "pct_set_stats": (C.c_int, [_p, C.c_int32]),
    "pct_knn": (C.c_int, [_p, C.c_int32, C.c_double, C.c_int32]),
    "pct_get_neighbors": (C.c_int, [_p, C.c_int64, C.c_int64, _i32p, _f32p, _i32p]),
    "pct_get_neighbor_rows": (C.c_int, [_p, _i64p, C.c_int64, _i32p, _f32p, _i32p]),
    "pct_fit": (C.c_int, [_p]),
    "pct_fit_indices": (C.c_int, [_p, _i32p, _i32p, _i64p, C.c_int64, C.c_int32]),
    "pct_curvature": (C.c_int, [_p, C.c_int32, C.c_double, C.c_int32]),
    "pct_get_fit": (C.c_int, [_p, C.c_int64, C.c_int64, _f32p, _f32p, _f32p, _f32p]),
    "pct_curvatures_from_coefficients": (C.c_int, [_p, _f32p, C.c_int64, _f32p, _f32p, _f32p]),
    "pct_neighbor_study_curvatures": (C.c_int, [_p, _i64p, C.c_int64, C.c_int32, C.c_int32, _f32p]),
    "pct_fit_indices_f64": (C.c_int, [_p, _i32p, _i32p, _i64p, C.c_int64, C.c_int32, _f64p, _f64p, _f64p]),
    "pct_plane_rotate": (C.c_int, [_p, _p, C.c_int32, C.c_int64, C.c_int32, _f64p]),
    "pct_fit_quadric": (C.c_int, [_p, _f32p, C.c_int64, C.c_int32, _f32p]),
    "pct_query_points": (C.c_int, [_p, _f64p, C.c_int64, C.c_int32, C.c_double, _i32p, _f64p]),
    "pct_query_points_algo": (C.c_int, [_p, _f64p, C.c_int64, C.c_int32, C.c_double, C.c_int32, _i32p, _f64p]),
    "pct_query_stats": (C.c_int, [_p, _i64p]),
    "pct_query_ball": (C.c_int, [_p, _f64p, C.c_int64, _f64p, C.c_int64, C.c_int32, C.c_int32, C.c_int64, _i64p]),
    "pct_get_ball": (C.c_int, [_p, C.c_int64, C.c_int64, _i32p, _f64p]),
    "pct_ball_stats": (C.c_int, [_p, _i64p]),
    "pct_fit_ball": (C.c_int, [_p, _i64p, C.c_int64, _i32p]),
    "pct_mesh_energies": (C.c_int, [_p, _f64p, C.c_int64, _i32p, C.c_int64, _p, _p, C.c_int32, _f64p]),
    "pct_point_areas": (C.c_int, [_p]),
    "pct_get_point_areas": (C.c_int, [_p, C.c_int64, C.c_int64, _f64p, _u8p, _i32p]),
    "pct_point_area_stats": (C.c_int, [_p, _i64p]),
    "pct_point_area_profile": (C.c_int, [_p, _f64p]),
    "pct_point_energies": (C.c_int, [_p, C.c_int32, _f64p]),
    "pct_point_frames": (C.c_int, [_p, _f64p]),
    "pct_get_point_frames": (C.c_int, [_p, C.c_int64, C.c_int64, _f64p, _f64p, _f64p, _u8p]),
    "pct_point_frame_stats": (C.c_int, [_p, _i64p, _f64p]),
    "pct_orient_frames": (C.c_int, [_p, C.c_int32, _f64p, C.c_int32]),
    "pct_get_orientation": (C.c_int, [_p, C.c_int64, C.c_int64, _i32p, _i32p, _i32p, _u8p]),
    "pct_orient_stats": (C.c_int, [_p, _i64p, _f64p]),
    "pct_voxel_downsample": (C.c_int, [_p, _f64p, C.c_int64, C.c_double, _i64p, _i64p]),
    "pct_voxel_downsample_f32": (C.c_int, [_p, _f32p, C.c_int64, C.c_double, _i64p, _i64p]),
    "pct_surface_variation": (C.c_int, [_p, C.c_int32, _f32p]),
    "pct_pca_curvatures": (C.c_int, [_p, C.c_int32, C.c_int32, C.c_int32, _i64p]),
    "pct_get_pca": (C.c_int, [_p, C.c_int64, C.c_int64, _f64p, _f64p, _f64p, _f64p, _f64p, _i32p]),
    "pct_text_shape": (C.c_int, [C.c_char_p, _i64p, _i32p]),
    "pct_text_load": (C.c_int, [C.c_char_p, C.c_int64, C.c_int32, _f64p]),
    "pct_format_float": (C.c_int, [C.c_double, C.c_char_p]),
    "pct_matrix_norms_f32": (C.c_int, [_f32p, C.c_int64, _f64p]),
    "pct_matrix_norms_f64": (C.c_int, [_f64p, C.c_int64, _f64p]),
    "pct_write_ply_ascii": (C.c_int, [C.c_char_p, _f32p, _f32p, _f32p, C.c_int64]),
    "pct_write_ply_ascii_normals": (C.c_int, [C.c_char_p, _f32p, _f32p, _f32p, _f32p, C.c_int64]),
    "pct_comm_unique_id": (C.c_int, [_p]),
    "pct_comm_init": (C.c_int, [_p, C.c_int32, C.c_int32, _p]),
    "pct_comm_destroy": (C.c_int, [_p]),
    "pct_comm_allgather_f32": (C.c_int, [_p, _p, _p, _i64p]),
    "pct_comm_counters": (C.c_int, [_p, _i64p]),
    "pct_comm_wait": (C.c_int, [_p]),
    "pct_comm_synchronize": (C.c_int, [_p]),
    "pct_comm_allreduce_f64": (C.c_int, [_p, _f64p, C.c_int32, C.c_int32]),
    "pct_get_timings": (C.c_int, [_p, C.POINTER(Timings)]),
    "pct_timings_size": (C.c_int, []),
    "pct_device_alloc": (C.c_int, [_p, C.c_int64, C.POINTER(_p)]),
    "pct_device_free": (C.c_int, [_p, _p]),
    "pct_device_upload": (C.c_int, [_p, _p, _p, C.c_int64]),
    "pct_device_download": (C.c_int, [_p, _p, _p, C.c_int64]),
    "pct_synchronize": (C.c_int, [_p]),
    "pct_selftest": (C.c_int, [_p, _i32p]),
    "pct_selftest_sort": (C.c_int, [_p, C.c_int32, _u32p, C.c_int64, _u32p]),
    "pct_selftest_sort_exact": (C.c_int, [_p, C.c_int32, C.c_int32, _f64p, _i32p, _f64p, _i32p, _i32p, C.c_int64, C.c_int64, _f64p, _i32p]),
    "pct_selftest_order_keys": (C.c_int, [_p, C.c_int32, C.c_int32, _u32p, _f64p, _i32p, C.c_int64, _u32p, _i32p]),
    "pct_selftest_sweep": (C.c_int, [_p, C.c_int32, C.c_double, C.c_int32, C.c_int32, _i32p, _f32p, _i32p, _u8p, _f64p]),
    "pct_selftest_levels_classify": (C.c_int, [_p, _i32p, _u32p, _i32p, C.c_int64, C.c_int64, C.c_float, C.c_float, _f32p, _f32p]),
    "pct_selftest_levels_bands": (C.c_int, [_p, _f32p, _f32p, C.c_int64, C.c_int64, C.c_int64, C.c_float, C.c_int32, C.c_float, C.c_float,
                                            _u32p, _u32p, _f32p, _f32p, _u32p]),
    "pct_selftest_levels_merge": (C.c_int, [_p, _i32p, C.c_int64, _i32p, C.c_int32, _i32p, _f32p, _i32p, _i32p, C.c_int64, C.c_int32, C.c_int32,
                                            C.c_int64, _i32p, _f32p, _i32p, _f32p, C.c_int64]),
    # include/pct_hip_surface.h
    "pct_point_triangles": (C.c_int, [_p, C.c_int32]),
    "pct_get_point_fans": (C.c_int, [_p, C.c_int64, C.c_int64, _i64p, _i32p]),
    "pct_get_triangles": (C.c_int, [_p, C.c_int64, C.c_int64, _i32p]),
    "pct_point_triangle_stats": (C.c_int, [_p, _i64p, _f64p]),
    "pct_point_triangle_profile": (C.c_int, [_p, _f64p]),
    "pct_write_ply_ascii_faces": (C.c_int, [C.c_char_p, _f32p, _f32p, _f32p, _f32p, C.c_int64, _i32p, C.c_int64]),
}

# include/pct_hip_holes.h: a table of its own -- SIGNATURES stays the boundary of pct_hip.h and pct_hip_surface.h
HOLE_SIGNATURES = {
    "pct_fill_holes": (C.c_int, [_p, C.c_int32, C.c_double, C.c_int32]),
    "pct_get_hole_triangles": (C.c_int, [_p, C.c_int64, C.c_int64, _i32p]),
    "pct_get_filled_triangles": (C.c_int, [_p, C.c_int64, C.c_int64, _i32p]),
    "pct_get_boundary_loops": (C.c_int, [_p, _i64p, _i32p, C.POINTER(C.c_uint8)]),
    "pct_fill_hole_stats": (C.c_int, [_p, _i64p, _f64p]),
}
HOLE_MAX_VERTICES = 32                                  # PCT_HOLE_MAX_VERTICES
HOLE_STATUS = ("filled", "perimeter", "blocked")        # pct_get_boundary_loops' status bytes

_lib = None


class HipExtensionError(RuntimeError):
    """The HIP extension is missing or unusable -- there is no CPU fallback."""


def load():
    """Load libpct_hip.so and attach prototypes.  Raises if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipExtensionError(
            f"{LIB_PATH} not found: the HIP extension has not been built "
            "(run __graft_entry__.build()); this package has no CPU fallback")
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as exc:  # pragma: no cover - depends on the machine
        raise HipExtensionError(f"cannot load {LIB_PATH}: {exc}") from exc
    for name, (res, args) in (*SIGNATURES.items(), *HOLE_SIGNATURES.items()):
        fn = getattr(lib, name)      # AttributeError if the ABI and these tables diverge
        fn.restype = res
        fn.argtypes = args
    if lib.pct_timings_size() != C.sizeof(Timings):
        raise HipExtensionError(f"{LIB_PATH}: pct_timings is {lib.pct_timings_size()} bytes, this binding expects "
                                f"{C.sizeof(Timings)} (library and package out of step: rebuild)")
    _lib = lib
    return lib


def load_text(path):
    """np.loadtxt(path) for whitespace-separated numeric scans, multi-threaded native parser (float64 out)."""
    lib = load()
    rows, cols = C.c_int64(0), C.c_int32(0)
    bpath = os.fsencode(path)
    if lib.pct_text_shape(bpath, C.byref(rows), C.byref(cols)) != PCT_OK:
        raise ValueError(f"cannot parse {path!r} as a rectangular table of numbers")
    out = np.empty((rows.value, cols.value), np.float64)
    if rows.value and lib.pct_text_load(bpath, rows.value, cols.value, _ptr(out, _f64p)) != PCT_OK:
        raise ValueError(f"cannot parse {path!r} as a rectangular table of numbers")
    return out


def matrix_norm_sums(points):
    """One native pass over a C-contiguous (N, 3) float32 / float64 array: (column sums of |.|, largest row sum of |.|,
    3 x 3 Gram matrix) -- what np.linalg.norm(points, 1 | inf | 2) are made of (host code, no device)."""
    p = np.asarray(points)
    out = np.empty(10, np.float64)
    if p.dtype == np.float32:
        st = load().pct_matrix_norms_f32(_ptr(p, _f32p), len(p), _ptr(out, _f64p))
    else:
        st = load().pct_matrix_norms_f64(_ptr(p, _f64p), len(p), _ptr(out, _f64p))
    if st != PCT_OK:
        raise ValueError("matrix norms: bad array")
    g = out[4:]
    gram = np.array([[g[0], g[1], g[2]], [g[1], g[3], g[4]], [g[2], g[4], g[5]]])
    return out[:3], out[3], gram


def format_float(x):
    """repr(float(x)) computed natively (the number format of the PLY writer)."""
    buf = C.create_string_buffer(40)
    n = load().pct_format_float(float(x), buf)
    return buf.raw[:n].decode()


def write_ply_ascii(path, points, gaussian, mean):
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    g = np.ascontiguousarray(gaussian, dtype=np.float32)
    m = np.ascontiguousarray(mean, dtype=np.float32)
    if len(g) != len(p) or len(m) != len(p):
        raise ValueError("one curvature value per point is required")
    if load().pct_write_ply_ascii(os.fsencode(path), _ptr(p, _f32p), _ptr(g, _f32p), _ptr(m, _f32p), len(p)) != PCT_OK:
        raise OSError(f"cannot write {path!r}")


def write_ply_ascii_normals(path, points, normals, gaussian, mean):
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    nr = np.ascontiguousarray(normals, dtype=np.float32)
    g = np.ascontiguousarray(gaussian, dtype=np.float32)
    m = np.ascontiguousarray(mean, dtype=np.float32)
    if nr.shape != p.shape:
        raise ValueError("one normal per point is required")
    if len(g) != len(p) or len(m) != len(p):
        raise ValueError("one curvature value per point is required")
    if load().pct_write_ply_ascii_normals(os.fsencode(path), _ptr(p, _f32p), _ptr(nr, _f32p), _ptr(g, _f32p), _ptr(m, _f32p), len(p)) != PCT_OK:
        raise OSError(f"cannot write {path!r}")


def write_ply_ascii_faces(path, points, normals, gaussian, mean, faces):
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    nr = np.ascontiguousarray(normals, dtype=np.float32)
    g = np.ascontiguousarray(gaussian, dtype=np.float32)
    m = np.ascontiguousarray(mean, dtype=np.float32)
    t = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    if nr.shape != p.shape:
        raise ValueError("one normal per point is required")
    if len(g) != len(p) or len(m) != len(p):
        raise ValueError("one curvature value per point is required")
    if load().pct_write_ply_ascii_faces(os.fsencode(path), _ptr(p, _f32p), _ptr(nr, _f32p), _ptr(g, _f32p), _ptr(m, _f32p), len(p),
                                        _ptr(t, _i32p), len(t)) != PCT_OK:
        raise OSError(f"cannot write {path!r}")


def device_count():
    n = C.c_int(0)
    load().pct_device_count(C.byref(n))
    return n.value


def comm_unique_id():
    """128 bytes identifying a new RCCL communicator (rank 0 calls this and hands the bytes to every rank)."""
    buf = C.create_string_buffer(128)
    if load().pct_comm_unique_id(C.cast(buf, _p)) != PCT_OK:
        raise HipExtensionError("pct_comm_unique_id failed: librccl.so cannot be opened or refused")
    return buf.raw


def _ptr(a, typ):
    return None if a is None else a.ctypes.data_as(typ)


def _queries(q, message):
    """Caller-supplied query points as a contiguous (m, 3) float64 array."""
    q = np.ascontiguousarray(q, dtype=np.float64)
    if q.ndim != 2 or q.shape[1] != 3:
        raise ValueError(message)
    return q


_handle_pool = {}          # device -> one idle Handle whose device buffers stay allocated (PointCloud.close puts it there)


def acquire_handle(device=0):
    """A device context for a PointCloud: the idle one of the pool if there is one (its buffers -- two dozen
    hipMallocs, ~4 ms for a million points -- are reused by the next cloud), else a new one."""
    h = _handle_pool.pop(int(device), None)
    if h is not None and getattr(h, "_h", None) and h._h.value:
        return h
    return Handle(device)


def release_handle(h):
    """Back to the pool (one idle handle per device is kept; a second one is closed).  PCT_NO_HANDLE_POOL=1 closes."""
    if h is None or not getattr(h, "_h", None) or not h._h.value:
        return
    if os.environ.get("PCT_NO_HANDLE_POOL") or h.device in _handle_pool:
        h.close()
        return
    try:
        h.set_stats(False)
        h.set_async(False)
        for attr in ("k", "eps"):
            if hasattr(h, attr):
                delattr(h, attr)
    except Exception:
        h.close()
        return
    _handle_pool[h.device] = h


atexit.register(lambda: drain_handle_pool())


def drain_handle_pool():
    """Close the idle handles (their device memory goes back to the runtime)."""
    while _handle_pool:
        _handle_pool.popitem()[1].close()


class Handle:
    """One device context (one HIP stream) -- thin, typed wrapper over pct_ctx."""

    def __init__(self, device=0):
        self._lib = load()
        self._h = _p()
        st = self._lib.pct_create(int(device), C.byref(self._h))
        if st != PCT_OK:
            self._h = _p()
            raise HipExtensionError(
                f"pct_create(device={device}) failed with status {st}: no usable MI355X (gfx950) device; "
                "this package has no CPU fallback")
        self.device = int(device)

    # -- plumbing ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.pct_destroy(self._h)
            self._h = _p()

    __del__ = close

    def _check(self, st):
        if st == PCT_OK:
            return
        msg = self._lib.pct_last_error(self._h).decode("utf-8", "replace")
        if st == PCT_ERR_NONFINITE:
            raise ValueError(msg or "Non-finite values in input points")     # pct:274
        if st == PCT_ERR_K_TOO_LARGE:
            raise IndexError(msg)                                            # reference: IndexError at pct:640
        if st == PCT_ERR_INVALID:
            raise ValueError(msg)
        if st == PCT_ERR_OOM:
            raise MemoryError(msg)
        if st == PCT_ERR_NO_NEIGHBORS:
            raise AttributeError(msg)                                        # reference: no self.neighbor_indices yet
        raise HipExtensionError(f"status {st}: {msg}")

    # -- cloud ------------------------------------------------------------
    def set_points(self, pts):
        pts = np.asarray(pts)
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise ValueError("points must have shape (N, 3)")
        if pts.dtype == np.float64:
            p = np.ascontiguousarray(pts)
            self._check(self._lib.pct_set_points_f64(self._h, _ptr(p, _f64p), len(p)))
        else:
            p = np.ascontiguousarray(pts, dtype=np.float32)
            self._check(self._lib.pct_set_points_f32(self._h, _ptr(p, _f32p), len(p)))
        self.n = self._rows = len(p)                 # (a new cloud is owned whole: new_cloud, pct_api.hip)

    def set_points_device(self, dev_ptr, n):
        self._check(self._lib.pct_set_points_device_f32(self._h, _p(int(dev_ptr)), int(n)))
        self.n = self._rows = int(n)

    def use_points_device(self, dev_ptr, n):
        """Zero-copy variant: the caller keeps the buffer alive and unchanged while the handle uses it."""
        self._check(self._lib.pct_use_points_device_f32(self._h, _p(int(dev_ptr)), int(n)))
        self.n = self._rows = int(n)

    def set_query_range(self, begin, end):
        self._check(self._lib.pct_set_query_range(self._h, int(begin), int(end)))
        self._rows = int(end) - int(begin)

    # -- ownership by slab (multi-GPU, clouds in no spatial order; include/pct_hip.h) --------------------------------
    def set_query_slab(self, part, parts):
        self._check(self._lib.pct_set_query_slab(self._h, int(part), int(parts)))
        self._rows = self.n                          # (index ranges are dropped: pct_set_query_slab)

    def slab_counts(self, parts):
        out = (C.c_int64 * int(parts))()
        self._check(self._lib.pct_slab_counts(self._h, out, int(parts)))
        return [int(v) for v in out]

    def slab_records(self, dev_ptr, capacity_rows):
        """(public index bits, K, H) of this slab's rows into the device buffer; returns the row count."""
        rows = C.c_int64(0)
        self._check(self._lib.pct_slab_records(self._h, _p(int(dev_ptr)), int(capacity_rows), C.byref(rows)))
        return rows.value

    def scatter_records(self, dev_records, n_records, begin, end, dev_K, dev_H):
        self._check(self._lib.pct_scatter_records(self._h, _p(int(dev_records)), int(n_records), int(begin), int(end),
                                                  _p(int(dev_K)), _p(int(dev_H))))

    def set_stats(self, enable=True):
        self._check(self._lib.pct_set_stats(self._h, int(bool(enable))))

    def set_grid_param(self, occupancy_factor):
        self._check(self._lib.pct_set_grid_param(self._h, float(occupancy_factor)))

    # -- path -------------------------------------------------------------
    def knn(self, k, eps=0.0, algo=KNN_AUTO):
        self._check(self._lib.pct_knn(self._h, int(k), float(eps or 0.0), int(algo)))
        self.k = int(k)

    def fit(self):
        self._check(self._lib.pct_fit(self._h))

    def curvature(self, k, eps=0.0, algo=KNN_AUTO):
        self._check(self._lib.pct_curvature(self._h, int(k), float(eps or 0.0), int(algo)))
        self.k = int(k)

    def get_neighbors(self, begin, end, want_idx=True, want_dist=True, want_count=False):
        rows = int(end) - int(begin)
        idx = np.empty((rows, self.k), np.int32) if want_idx else None
        dist = np.empty((rows, self.k), np.float32) if want_dist else None
        cnt = np.empty(rows, np.int32) if want_count else None
        self._check(self._lib.pct_get_neighbors(self._h, int(begin), int(end), _ptr(idx, _i32p),
                                                _ptr(dist, _f32p), _ptr(cnt, _i32p)))
        return idx, dist, cnt

    def query_points(self, q, k, eps=0.0, algo=QUERY_AUTO):
        """The reference tree's ``query`` for arbitrary points: (m,3) float64 -> idx (m,k) int32 (missing: N), dist (m,k) float64 (missing: inf).
        ``algo``: QUERY_AUTO (large query sets through the cell list), QUERY_SWEEP, QUERY_GRID -- the same rows either way."""
        q = _queries(q, "query points must have shape (m, 3)")
        idx = np.empty((len(q), int(k)), np.int32)
        dist = np.empty((len(q), int(k)), np.float64)
        self._check(self._lib.pct_query_points_algo(self._h, _ptr(q, _f64p), len(q), int(k), float(eps or 0.0), int(algo),
                                                    _ptr(idx, _i32p), _ptr(dist, _f64p)))
        return idx, dist

    def query_points_plain(self, q, k, eps=0.0):
        """``pct_query_points`` itself: the exhaustive sweep whatever is resident (``query_points`` names the path)."""
        q = _queries(q, "query points must have shape (m, 3)")
        idx = np.empty((len(q), int(k)), np.int32)
        dist = np.empty((len(q), int(k)), np.float64)
        self._check(self._lib.pct_query_points(self._h, _ptr(q, _f64p), len(q), int(k), float(eps or 0.0), _ptr(idx, _i32p), _ptr(dist, _f64p)))
        return idx, dist

    def query_ball(self, q, r, flags=BALL_SORTED, algo=QUERY_AUTO, max_entries=0):
        """``pct_query_ball``: every cloud point within ``r`` (one radius, or one per query; inclusive) of each (m,3)
        float64 query.  Returns ``(status, offsets)`` -- PCT_OK, or PCT_ERR_LIMIT when the rows hold more than
        ``max_entries`` entries (offsets valid, nothing resident); every other status raises.  The rows stay on the
        device for ``get_ball``."""
        q = _queries(q, "query points must have shape (m,3)")
        r = np.ascontiguousarray(np.atleast_1d(r), dtype=np.float64)
        if r.ndim != 1:
            raise ValueError("radii must be a scalar or have shape (m,)")
        offsets = np.zeros(len(q) + 1, np.int64)
        st = self._lib.pct_query_ball(self._h, _ptr(q, _f64p), len(q), _ptr(r, _f64p), len(r), int(flags), int(algo),
                                      int(max_entries), _ptr(offsets, _i64p))
        if st in (PCT_ERR_INVALID, PCT_ERR_NONFINITE):
            self._check(st)                   # refused before the library dropped anything: the rows of an earlier query stay, and their offsets here
        self._ball_offsets = offsets if st == PCT_OK and not flags & BALL_COUNT_ONLY else None
        if st != PCT_ERR_LIMIT:
            self._check(st)
        return st, offsets

    def get_ball(self, row_begin=0, row_end=None, want_dist=False):
        """Rows [row_begin, row_end) of the last ``query_ball``: indices int32 (and distances float64), concatenated."""
        off = getattr(self, "_ball_offsets", None)
        if off is None:                       # (the library says why: nothing resident)
            self._check(self._lib.pct_get_ball(self._h, int(row_begin), int(row_begin if row_end is None else row_end), None, None))
            raise ValueError("no ball rows on this handle")
        row_end = len(off) - 1 if row_end is None else int(row_end)
        if not 0 <= row_begin <= row_end <= len(off) - 1:
            raise ValueError(f"bad row range [{row_begin},{row_end}) of {len(off) - 1}")
        count = int(off[row_end] - off[row_begin])
        idx = np.empty(count, np.int32)
        dist = np.empty(count, np.float64) if want_dist else None
        self._check(self._lib.pct_get_ball(self._h, int(row_begin), row_end, _ptr(idx, _i32p), _ptr(dist, _f64p) if want_dist else None))
        return (idx, dist) if want_dist else idx

    def ball_stats(self):
        """Of the last ``query_ball``: {route (as query_stats), staged, streamed, max_ring}."""
        out = np.zeros(4, np.int64)
        self._check(self._lib.pct_ball_stats(self._h, _ptr(out, _i64p)))
        return {"route": int(out[0]), "staged": int(out[1]), "streamed": int(out[2]), "max_ring": int(out[3])}

    def fit_ball(self, self_rows):
        """``pct_fit_ball``: the quadric fit of the resident rows of the last ``query_ball``, row i about the cloud point
        ``self_rows[i]`` (its own index is no member of its row).  Returns ``used`` (m,) int32, the members fitted per row;
        coefficients and curvatures are row-aligned, read with ``get_fit(0, m)``."""
        rows = np.ascontiguousarray(self_rows, dtype=np.int64)
        if rows.ndim != 1:
            raise ValueError("centres must have shape (m,)")
        used = np.empty(len(rows), np.int32)
        self._check(self._lib.pct_fit_ball(self._h, _ptr(rows, _i64p), len(rows), _ptr(used, _i32p)))
        return used

    def query_stats(self):
        """Of the last ``query_points``: {route (0 sweep, 1 resident cell list, 2 cell list built), stencil, redone, max_ring}."""
        out = np.zeros(4, np.int64)
        self._check(self._lib.pct_query_stats(self._h, _ptr(out, _i64p)))
        return {"route": int(out[0]), "stencil": int(out[1]), "redone": int(out[2]), "max_ring": int(out[3])}

    def get_neighbor_rows(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        idx = np.empty((len(rows), self.k), np.int32)
        dist = np.empty((len(rows), self.k), np.float32)
        cnt = np.empty(len(rows), np.int32)
        self._check(self._lib.pct_get_neighbor_rows(self._h, _ptr(rows, _i64p), len(rows), _ptr(idx, _i32p),
                                                   _ptr(dist, _f32p), _ptr(cnt, _i32p)))
        return idx, dist, cnt

    def fit_indices(self, idx, count=None, query=None):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        if idx.ndim != 2:
            raise ValueError("neighbour indices must have shape (rows, k)")
        cnt = None if count is None else np.ascontiguousarray(count, dtype=np.int32)
        qry = None if query is None else np.ascontiguousarray(query, dtype=np.int64)
        self._check(self._lib.pct_fit_indices(self._h, _ptr(idx, _i32p), _ptr(cnt, _i32p), _ptr(qry, _i64p),
                                              idx.shape[0], idx.shape[1]))
        return idx.shape[0]

    def fit_indices_f64(self, idx, count=None, query=None):
        """Diagnostics: unrounded float64 coefficients (rows,6) and float64 K, H of the given neighbourhoods."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        if idx.ndim != 2:
            raise ValueError("neighbour indices must have shape (rows, k)")
        cnt = None if count is None else np.ascontiguousarray(count, dtype=np.int32)
        qry = None if query is None else np.ascontiguousarray(query, dtype=np.int64)
        rows = idx.shape[0]
        c, K, H = np.empty((rows, 6), np.float64), np.empty(rows, np.float64), np.empty(rows, np.float64)
        self._check(self._lib.pct_fit_indices_f64(self._h, _ptr(idx, _i32p), _ptr(cnt, _i32p), _ptr(qry, _i64p), rows, idx.shape[1],
                                                  _ptr(c, _f64p), _ptr(K, _f64p), _ptr(H, _f64p)))
        return c, K, H

    def get_fit(self, begin, end, coefs=True, K=True, H=True, H2=True):
        rows = int(end) - int(begin)
        c = np.empty((rows, 6), np.float32) if coefs else None
        # K, H, H^2 share one host block, back to back: the library moves what is adjacent on both sides in ONE copy
        # (two 4 MB copies cost two fixed set-ups: 0.65 -> 0.4 ms for a million points)
        want = [K, H, H2]
        block = np.empty((sum(want), rows), np.float32)
        it = iter(block)
        k, h, h2 = (next(it) if w else None for w in want)
        self._check(self._lib.pct_get_fit(self._h, int(begin), int(end), _ptr(c, _f32p), _ptr(k, _f32p),
                                          _ptr(h, _f32p), _ptr(h2, _f32p)))
        return c, k, h, h2

    def curvatures_from_coefficients(self, coefs):
        c = np.ascontiguousarray(coefs, dtype=np.float32).reshape(-1, 6)
        k = np.empty(len(c), np.float32)
        h = np.empty(len(c), np.float32)
        h2 = np.empty(len(c), np.float32)
        self._check(self._lib.pct_curvatures_from_coefficients(self._h, _ptr(c, _f32p), len(c), _ptr(k, _f32p),
                                                               _ptr(h, _f32p), _ptr(h2, _f32p)))
        return k, h, h2

    def plane_rotate(self, nbrs):
        """get_best_fit_plane_and_rotate for a block of neighbourhoods: (batch, m, 3) float32 / float64 -> float64."""
        a = np.asarray(nbrs)
        a = np.ascontiguousarray(a, dtype=np.float64 if a.dtype == np.float64 else np.float32)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("neighbourhoods must have shape (batch, m, 3)")
        out = np.empty(a.shape, np.float64)
        self._check(self._lib.pct_plane_rotate(self._h, a.ctypes.data_as(_p), int(a.dtype == np.float64), a.shape[0], a.shape[1],
                                               _ptr(out, _f64p)))
        return out

    def fit_quadric(self, pts):
        """fit_quadratic_surface for a block of rotated neighbourhoods: (batch, m, 3) float32 -> (batch, 6) float32."""
        a = np.ascontiguousarray(pts, dtype=np.float32)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("Input points must have shape (batch, N, 3)")
        out = np.empty((a.shape[0], 6), np.float32)
        self._check(self._lib.pct_fit_quadric(self._h, _ptr(a, _f32p), a.shape[0], a.shape[1], _ptr(out, _f32p)))
        return out

    def neighbor_study_curvatures(self, sample_rows, n_lo, n_hi):
        rows = np.ascontiguousarray(sample_rows, dtype=np.int64)
        out = np.empty((len(rows), int(n_hi) - int(n_lo) + 1), np.float32)
        self._check(self._lib.pct_neighbor_study_curvatures(self._h, _ptr(rows, _i64p), len(rows), int(n_lo), int(n_hi),
                                                           _ptr(out, _f32p)))
        return out

    def mesh_energies(self, vertices, triangles, gaussian, mean):
        v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
        t = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
        # each array in its own dtype, as np.mean takes it (utils.py:753-755): float64 stays float64 whatever the other is
        k64, h64 = np.asarray(gaussian).dtype == np.float64, np.asarray(mean).dtype == np.float64
        g = np.ascontiguousarray(gaussian, dtype=np.float64 if k64 else np.float32)
        m = np.ascontiguousarray(mean, dtype=np.float64 if h64 else np.float32)
        kind = MESH_F64 if k64 and h64 else MESH_K64_H32 if k64 else MESH_K32_H64 if h64 else MESH_F32
        if len(g) != len(v) or len(m) != len(v):
            raise ValueError("one curvature value per vertex is required")
        out = np.zeros(3, np.float64)
        self._check(self._lib.pct_mesh_energies(self._h, _ptr(v, _f64p), len(v), _ptr(t, _i32p), len(t), g.ctypes.data_as(_p),
                                               m.ctypes.data_as(_p), kind, _ptr(out, _f64p)))
        return float(out[0]), float(out[1]), float(out[2])

    # -- mesh-free energies: tangent-plane Voronoi areas of the resident table's rows (pct:650-655) ------------------
    def point_areas(self):
        """``pct_point_areas``: the area of every owned point's Voronoi cell in its own tangent plane, from the rows of
        the resident neighbour table; kept on the device (``get_point_areas``, ``point_energies``)."""
        self._check(self._lib.pct_point_areas(self._h))

    def get_point_areas(self, begin, end, area=True, closed=True, nverts=True):
        """(area float64, closed uint8, nverts int32) of cloud rows [begin, end); ``None`` for what was not asked for."""
        rows = int(end) - int(begin)
        a = np.empty(rows, np.float64) if area else None
        c = np.empty(rows, np.uint8) if closed else None
        n = np.empty(rows, np.int32) if nverts else None
        self._check(self._lib.pct_get_point_areas(self._h, int(begin), int(end), _ptr(a, _f64p), _ptr(c, _u8p), _ptr(n, _i32p)))
        return a, c, n

    def _stage_stats(self, call, counters, ms_names=("ms",)):
        """What a surface stage's statistics getters answer, as one dict: ``call(out, ms)`` fills an int64 and a float64
        array through them; ``counters`` names the leading words of the one, ``ms_names`` those of the other."""
        out, ms = np.zeros(8, np.int64), np.zeros(3, np.float64)
        call(out, ms)
        return {**{k: int(v) for k, v in zip(counters, out)}, **{k: float(v) for k, v in zip(ms_names, ms)}}

    def point_area_stats(self):
        """Of the last ``point_areas``: {rows, closed, nan, overflow (rows redone with room for k + 4 vertices), ms (device
        time of its kernels), survivors (neighbours that passed the rejection test, summed over the rows)}."""
        def call(out, ms):
            self._check(self._lib.pct_point_area_stats(self._h, _ptr(out, _i64p)))
            self._check(self._lib.pct_point_area_profile(self._h, _ptr(ms, _f64p)))
        d = self._stage_stats(call, ("rows", "closed", "nan", "overflow"), ("ms", "survivors"))
        d["survivors"] = int(d["survivors"])         # (a count that travels as a double)
        return d

    # -- surface frames from the resident fit: fitted normals, k1 / k2 and their directions ---------------------------
    def point_frames(self, viewpoint=None):
        """``pct_point_frames``: normal, k1 >= k2 and the principal directions of every owned row, from the resident table
        and its fit; with ``viewpoint`` (three numbers in the cloud's coordinates) every normal is turned to its side.
        Kept on the device (``get_point_frames``)."""
        v = None if viewpoint is None else np.ascontiguousarray(viewpoint, dtype=np.float64).reshape(3)
        self._check(self._lib.pct_point_frames(self._h, _ptr(v, _f64p)))

    def get_point_frames(self, begin, end, normal=True, k=True, dirs=True, flipped=True):
        """(normal (rows, 3), k (rows, 2) = [k1, k2], dirs (rows, 3, 2), flipped (rows,) uint8) of cloud rows [begin, end);
        ``None`` for what was not asked for."""
        rows = int(end) - int(begin)
        n = np.empty((rows, 3), np.float64) if normal else None
        kk = np.empty((rows, 2), np.float64) if k else None
        d = np.empty((rows, 3, 2), np.float64) if dirs else None
        f = np.empty(rows, np.uint8) if flipped else None
        self._check(self._lib.pct_get_point_frames(self._h, int(begin), int(end), _ptr(n, _f64p), _ptr(kk, _f64p), _ptr(d, _f64p), _ptr(f, _u8p)))
        return n, kk, d, f

    def point_frame_stats(self):
        """Of the last ``point_frames``: {rows, nan, flipped, umbilic, ms (device time of its kernel)}."""
        return self._stage_stats(lambda out, ms: self._check(self._lib.pct_point_frame_stats(self._h, _ptr(out, _i64p), _ptr(ms, _f64p))),
                                 ("rows", "nan", "flipped", "umbilic"))

    # -- consistent orientation of those frames: a flood over the resident table --------------------------------------------
    def orient_frames(self, anchor="top", viewpoint=None, max_components=None):
        """``pct_orient_frames``: turns the resident frames so that neighbouring rows agree.  ``anchor``: "seed", "top" or
        "view" (or the ORIENT_* value); "view" needs ``viewpoint``.  The frames stay on the device (``get_point_frames``
        serves them turned), and so do the component, parent, level and toggle of every row (``get_orientation``)."""
        a = ORIENT_ANCHORS.get(anchor, anchor)
        if not isinstance(a, (int, np.integer)):
            raise ValueError(f"unknown anchor {anchor!r}")
        v = None if viewpoint is None else np.ascontiguousarray(viewpoint, dtype=np.float64).reshape(3)
        self._check(self._lib.pct_orient_frames(self._h, int(a), _ptr(v, _f64p), int(max_components or 0)))

    def get_orientation(self, begin, end):
        """(component, parent, level int32, toggled uint8) of cloud rows [begin, end); -1 where a row was not labelled."""
        rows = int(end) - int(begin)
        comp, parent, level = (np.empty(rows, np.int32) for _ in range(3))
        toggled = np.empty(rows, np.uint8)
        self._check(self._lib.pct_get_orientation(self._h, int(begin), int(end), _ptr(comp, _i32p), _ptr(parent, _i32p),
                                                  _ptr(level, _i32p), _ptr(toggled, _u8p)))
        return comp, parent, level, toggled

    def orient_stats(self):
        """Of the last ``orient_frames``: {valid, components, unlabelled, toggled, levels, pulls, launches, waits, ms}."""
        return self._stage_stats(lambda out, ms: self._check(self._lib.pct_orient_stats(self._h, _ptr(out, _i64p), _ptr(ms, _f64p))),
                                 ("valid", "components", "unlabelled", "toggled", "levels", "pulls", "launches", "waits"))

    # -- faces from the tangent-plane Voronoi cells (include/pct_hip_surface.h) ----------------------------------------------
    def point_triangles(self, wind_frames=False, flags=0):
        """``pct_point_triangles``: fans, corners and triangles of the resident table of a whole-cloud handle;
        ``wind_frames``: wound about the resident frames' normals (PCT_TRI_WIND_FRAMES); ``flags``: further flag bits,
        passed as they are.  Kept on the device (``get_triangles``, ``get_point_fans``)."""
        self._check(self._lib.pct_point_triangles(self._h, (TRI_WIND_FRAMES if wind_frames else 0) | int(flags)))

    def get_point_fans(self, begin, end):
        """(offsets (rows + 1,) int64, indices int32): the natural neighbours of cloud rows [begin, end) as CSR, public
        indices in polygon order."""
        rows = int(end) - int(begin)
        off = np.zeros(max(rows, 0) + 1, np.int64)
        self._check(self._lib.pct_get_point_fans(self._h, int(begin), int(end), _ptr(off, _i64p), None))
        nbr = np.empty(int(off[-1]), np.int32)
        if len(nbr):
            self._check(self._lib.pct_get_point_fans(self._h, int(begin), int(end), _ptr(off, _i64p), _ptr(nbr, _i32p)))
        return off, nbr

    def point_triangle_stats(self):
        """Of the last ``point_triangles``: {rows, rows_with_corner, corners, triangles, wide_rows, largest_fan,
        boundary_edges, ms, fan_ms, agree_ms (device times: the call, its fan kernels, agreement and emission)}."""
        def call(out, ms):
            self._check(self._lib.pct_point_triangle_stats(self._h, _ptr(out, _i64p), _ptr(ms, _f64p)))
            self._check(self._lib.pct_point_triangle_profile(self._h, _ptr(ms[1:], _f64p)))
        return self._stage_stats(call, ("rows", "rows_with_corner", "corners", "triangles", "wide_rows", "largest_fan", "boundary_edges"),
                                 ("ms", "fan_ms", "agree_ms"))

    def get_triangles(self, first=0, count=None):
        """(count, 3) int32 public indices, ascending by (v0, v1, v2); by default all of them."""
        if count is None:
            count = self.point_triangle_stats()["triangles"] - int(first)
        tri = np.empty((max(int(count), 0), 3), np.int32)
        self._check(self._lib.pct_get_triangles(self._h, int(first), int(count), _ptr(tri, _i32p)))
        return tri

    # -- boundary loops and small-hole filling (include/pct_hip_holes.h) -----------------------------------------------------
    def fill_holes(self, max_vertices=HOLE_MAX_VERTICES, max_perimeter=float("inf"), flags=0):
        """``pct_fill_holes``: the boundary loops of the resident triangles, those of at most ``max_vertices`` vertices and
        a perimeter below ``max_perimeter`` filled.  Kept on the device beside the triangles (``get_hole_triangles``,
        ``get_filled_triangles``, ``get_boundary_loops``)."""
        self._check(self._lib.pct_fill_holes(self._h, int(max_vertices), float(max_perimeter), int(flags)))

    def fill_hole_stats(self):
        """Of the last ``fill_holes``: {boundary_edges (before), gaps, odd_gaps, loops, filled, perimeter, blocked,
        patch_triangles, ms (device time of the call)}."""
        return self._stage_stats(lambda out, ms: self._check(self._lib.pct_fill_hole_stats(self._h, _ptr(out, _i64p), _ptr(ms, _f64p))),
                                 ("boundary_edges", "gaps", "odd_gaps", "loops", "filled", "perimeter", "blocked", "patch_triangles"))

    def get_hole_triangles(self, first=0, count=None):
        """(count, 3) int32: the patch triangles, ascending; by default all of them."""
        if count is None:
            count = self.fill_hole_stats()["patch_triangles"] - int(first)
        tri = np.empty((max(int(count), 0), 3), np.int32)
        self._check(self._lib.pct_get_hole_triangles(self._h, int(first), int(count), _ptr(tri, _i32p)))
        return tri

    def get_filled_triangles(self, first=0, count=None):
        """(count, 3) int32: the resident triangles merged with the patches, ascending; by default all of them."""
        if count is None:
            count = self.point_triangle_stats()["triangles"] + self.fill_hole_stats()["patch_triangles"] - int(first)
        tri = np.empty((max(int(count), 0), 3), np.int32)
        self._check(self._lib.pct_get_filled_triangles(self._h, int(first), int(count), _ptr(tri, _i32p)))
        return tri

    def get_boundary_loops(self):
        """(offsets (loops + 1,) int64, vertices int32, status (loops,) uint8): every owned loop in canonical order; status
        0 filled, 1 left for its perimeter, 2 blocked."""
        loops = self.fill_hole_stats()["loops"]
        off = np.zeros(loops + 1, np.int64)
        status = np.zeros(loops, np.uint8)
        u8p = C.POINTER(C.c_uint8)
        self._check(self._lib.pct_get_boundary_loops(self._h, _ptr(off, _i64p), None, _ptr(status, u8p)))
        verts = np.empty(int(off[-1]), np.int32)
        if len(verts):
            self._check(self._lib.pct_get_boundary_loops(self._h, _ptr(off, _i64p), _ptr(verts, _i32p), _ptr(status, u8p)))
        return off, verts, status

    def point_energies(self, closed_only=False):
        """``pct_point_energies``: (bending, stretching, area, n_used) over the owned rows -- the closed ones only with
        ``closed_only``; needs the fit and the areas of the table in place."""
        out = np.zeros(4, np.float64)
        self._check(self._lib.pct_point_energies(self._h, int(bool(closed_only)), _ptr(out, _f64p)))
        return float(out[0]), float(out[1]), float(out[2]), int(out[3])

    def voxel_downsample(self, xyz, voxel_size):
        """Indices of the first point of every voxel.  float32 coordinates are binned in float32, everything else in
        float64 -- as ``np.floor(coordinates / voxel_size)`` evaluates (convert_asc_to_ply.py:34)."""
        xyz = np.asarray(xyz)
        f32 = xyz.dtype == np.float32
        p = np.ascontiguousarray(xyz, dtype=np.float32 if f32 else np.float64).reshape(-1, 3)
        idx = np.empty(len(p), np.int64)
        cnt = C.c_int64(0)
        if f32:
            self._check(self._lib.pct_voxel_downsample_f32(self._h, _ptr(p, _f32p), len(p), float(voxel_size), _ptr(idx, _i64p), C.byref(cnt)))
        else:
            self._check(self._lib.pct_voxel_downsample(self._h, _ptr(p, _f64p), len(p), float(voxel_size), _ptr(idx, _i64p), C.byref(cnt)))
        return idx[:cnt.value].copy()

    def surface_variation(self, k_total):
        """One value per OWNED row (the query range; the whole cloud unless ``set_query_range`` narrowed it)."""
        out = np.empty(self._rows, np.float32)
        self._check(self._lib.pct_surface_variation(self._h, int(k_total), _ptr(out, _f32p)))
        self.k = int(k_total) - 1
        return out

    def pca_curvatures(self, k, algo=KNN_AUTO, keep_neighbors=False):
        """principal_curvatures_via_principal_component_analysis (pct:901-950) of the loaded cloud, kept on the device
        (``get_pca``).  Returns the number of float64 rows that went through the exhaustive pass."""
        exact = C.c_int64(0)
        st = self._lib.pct_pca_curvatures(self._h, int(k), int(algo), int(bool(keep_neighbors)), C.byref(exact))
        if st == PCT_ERR_NONFINITE:
            raise ValueError("array must not contain infs or NaNs")              # what scipy.linalg.eigh says (pct:925)
        self._check(st)
        self.pca_k = min(int(k), self.n - 1)
        return exact.value

    def get_pca(self, begin, end, want_idx=False):
        """(l1, l2, dirs (rows, 3, 2), K, H[, idx (rows, k)]) of rows [begin, end), float64."""
        rows = int(end) - int(begin)
        l1, l2, K, H = (np.empty(rows, np.float64) for _ in range(4))
        dirs = np.empty((rows, 3, 2), np.float64)
        idx = np.empty((rows, self.pca_k), np.int32) if want_idx else None
        self._check(self._lib.pct_get_pca(self._h, int(begin), int(end), _ptr(l1, _f64p), _ptr(l2, _f64p), _ptr(dirs, _f64p),
                                          _ptr(K, _f64p), _ptr(H, _f64p), _ptr(idx, _i32p)))
        return (l1, l2, dirs, K, H) + ((idx,) if want_idx else ())

    def timings(self):
        t = Timings()
        self._lib.pct_get_timings(self._h, C.byref(t))
        return t.as_dict()

    def set_async(self, enable=True):
        """Streams of clouds: ``curvature`` on a whole-cloud handle returns once its kernels are enqueued; every other
        call first waits for it (include/pct_hip.h, pct_set_async)."""
        self._check(self._lib.pct_set_async(self._h, int(bool(enable))))

    def stage_times_done(self):
        """Timings of the most recent call whose kernels are known to have finished -- with ``set_async`` the call before
        the pending one; does not wait.  One struct kept on the handle, refilled and returned."""
        t = self.__dict__.get("_tm")
        if t is None:
            t = self._tm = Timings()
            self._tm_ref = C.byref(t)
        self._lib.pct_get_timings_done(self._h, self._tm_ref)
        return t

    def stage_times(self):
        """The same record as ``timings`` without building a dict: one struct kept on the handle, refilled and returned
        (read ``.grid_ms``, ``.knn_ms``, ...).  For loops that poll after every step while the GPU waits for the host."""
        t = self.__dict__.get("_tm")
        if t is None:
            t = self._tm = Timings()
            self._tm_ref = C.byref(t)
        self._lib.pct_get_timings(self._h, self._tm_ref)
        return t

    # -- multi-GPU exchange (RCCL behind the C ABI) ---------------------------
    def comm_init(self, rank, world, unique_id):
        if len(unique_id) != 128:
            raise ValueError("the RCCL unique id is 128 bytes")
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._check(self._lib.pct_comm_init(self._h, int(rank), int(world), C.cast(buf, _p)))
        self.rank, self.world = int(rank), int(world)

    def comm_destroy(self):
        self._check(self._lib.pct_comm_destroy(self._h))

    def comm_allgather(self, dev_send, dev_recv, counts):
        """Start the all-gather of float32 shards (counts[r] floats from rank r) on the exchange stream."""
        c = np.ascontiguousarray(counts, dtype=np.int64)
        self._check(self._lib.pct_comm_allgather_f32(self._h, _p(int(dev_send)), _p(int(dev_recv)), _ptr(c, _i64p)))

    def comm_counters(self):
        """Collectives issued by this handle: {allgather, padded_allgather, broadcast_groups, allreduce}."""
        c = np.zeros(4, np.int64)
        self._check(self._lib.pct_comm_counters(self._h, _ptr(c, _i64p)))
        return dict(zip(("allgather", "padded_allgather", "broadcast_groups", "allreduce"), (int(v) for v in c)))

    def comm_wait(self):
        self._check(self._lib.pct_comm_wait(self._h))

    def comm_synchronize(self):
        self._check(self._lib.pct_comm_synchronize(self._h))

    def comm_allreduce(self, values, op="sum"):
        v = np.ascontiguousarray(np.atleast_1d(values), dtype=np.float64).copy()
        self._check(self._lib.pct_comm_allreduce_f64(self._h, _ptr(v, _f64p), len(v), {"sum": 0, "max": 2, "min": 3}[op]))
        return v

    def comm_barrier(self):
        self._check(self._lib.pct_comm_allreduce_f64(self._h, None, 0, 0))

    # -- raw device memory (multi-GPU all-gather target) ---------------------
    def device_alloc(self, nbytes):
        out = _p()
        self._check(self._lib.pct_device_alloc(self._h, int(nbytes), C.byref(out)))
        return out.value

    def device_free(self, ptr):
        self._check(self._lib.pct_device_free(self._h, _p(int(ptr))))

    def device_upload(self, ptr, host):
        host = np.ascontiguousarray(host)
        self._check(self._lib.pct_device_upload(self._h, _p(int(ptr)), host.ctypes.data_as(_p), host.nbytes))

    def device_download(self, ptr, host):
        assert host.flags["C_CONTIGUOUS"]
        self._check(self._lib.pct_device_download(self._h, host.ctypes.data_as(_p), _p(int(ptr)), host.nbytes))

    def selftest(self):
        n = C.c_int32(-1)
        self._check(self._lib.pct_selftest(self._h, C.byref(n)))
        return n.value

    # -- the wave-level sorters on caller-supplied lists (tests/test_gpu_sort_net.py) ---------------------------------
    def selftest_sort(self, network, lists):
        """lists (n, 64 | 128) uint32 -> each list sorted by the network `network` (NET_*)."""
        x = np.ascontiguousarray(lists, dtype=np.uint32)
        assert x.ndim == 2 and x.shape[1] == NET_LIST[network]
        out = np.empty_like(x)
        self._check(self._lib.pct_selftest_sort(self._h, network, _ptr(x, _u32p), len(x), _ptr(out, _u32p)))
        return out

    def selftest_sort_exact(self, regs, mode, d2, pos, pub, batch=None):
        """lists (n, 64 regs) of (float64 d2, int32 position) through the exact sweep's sorter (EXACT_*); pub[position] is
        the public index; batch = (d2, pos) of the descending lists of EXACT_MERGE_MIN."""
        d2 = np.ascontiguousarray(d2, dtype=np.float64)
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        pub = np.ascontiguousarray(pub, dtype=np.int32)
        assert d2.shape == pos.shape == (len(d2), 64 * regs) and (batch is not None) == (mode == EXACT_MERGE_MIN)
        bd = bp = None
        if batch is not None:
            bd, bp = np.ascontiguousarray(batch[0], dtype=np.float64), np.ascontiguousarray(batch[1], dtype=np.int32)
            assert bd.shape == bp.shape == d2.shape
        od, op = np.empty_like(d2), np.empty_like(pos)
        self._check(self._lib.pct_selftest_sort_exact(self._h, regs, mode, _ptr(d2, _f64p), _ptr(pos, _i32p),
                                                      None if bd is None else _ptr(bd, _f64p), None if bp is None else _ptr(bp, _i32p),
                                                      _ptr(pub, _i32p), len(pub), len(d2), _ptr(od, _f64p), _ptr(op, _i32p)))
        return od, op

    def selftest_order_keys(self, regs, slot_bits, elems, d2, pub):
        """order_equal_keys<regs, slot_bits> on lists (n, 64 regs) uint32; d2, pub (n, 2^slot_bits) by payload.
        Returns (lists, flags)."""
        e = np.ascontiguousarray(elems, dtype=np.uint32)
        d2 = np.ascontiguousarray(d2, dtype=np.float64)
        pub = np.ascontiguousarray(pub, dtype=np.int32)
        assert e.shape == (len(e), 64 * regs) and d2.shape == pub.shape == (len(e), 1 << slot_bits)
        out, done = np.empty_like(e), np.empty(len(e), np.int32)
        self._check(self._lib.pct_selftest_order_keys(self._h, regs, slot_bits, _ptr(e, _u32p), _ptr(d2, _f64p), _ptr(pub, _i32p),
                                                      len(e), _ptr(out, _u32p), _ptr(done, _i32p)))
        return out, done != 0

    # -- the planned fast sweep alone, on the handle's cloud (tests/test_gpu_select.py) --------------------------------
    def selftest_sweep(self, k, eps=0.0, algo=KNN_GRID, want_dist=True):
        """pct_knn(k, eps, algo) up to and including the one launch of the planned fast sweep; no exact sweep.  Returns a
        dict for the owned rows in public order: idx (rows, k; -1: none), dist (rows, k) or None where the plan keeps no
        distances, count (rows), redo / trusted (rows, bool), and sweep_variant, redo_count, cell_size, dims, origin,
        items_q, items.  Drops every resident result."""
        rows = self._rows
        idx = np.empty((rows, int(k)), np.int32)
        dist = np.full((rows, int(k)), np.nan, np.float32)
        count = np.empty(rows, np.int32)
        flags = np.empty(rows, np.uint8)
        info = np.zeros(12, np.float64)
        self._check(self._lib.pct_selftest_sweep(self._h, int(k), float(eps), int(algo), 1 if want_dist else 0, _ptr(idx, _i32p), _ptr(dist, _f32p),
                                                 _ptr(count, _i32p), _ptr(flags, _u8p), _ptr(info, _f64p)))
        self.k = int(k)                              # (as knn: what a getter would size its arrays by, were it not refused)
        return {"idx": idx, "dist": dist if info[9] else None, "count": count, "redo": (flags & 1) != 0, "trusted": (flags & 2) != 0,
                "sweep_variant": int(info[0]), "redo_count": int(info[1]), "cell_size": float(info[2]),
                "dims": tuple(int(v) for v in info[3:6]), "origin": tuple(float(v) for v in info[6:9]), "items_q": int(info[10]), "items": int(info[11])}

    # -- the planning kernels of the chained sweep on caller-supplied arrays (tests/test_gpu_levels_exact.py) ----------
    def selftest_levels_classify(self, row_done, redo_m, pub, log_edge, target, want, bracket):
        """k_classify over rows (row_done, redo_m = why << 29 | pop, public index pub); want (n_pub) and bracket
        (n_pub, 2) by public index.  Returns the rewritten (want, bracket); the arguments are left alone."""
        done = np.ascontiguousarray(row_done, dtype=np.int32)
        redo = np.ascontiguousarray(redo_m, dtype=np.uint32)
        pub = np.ascontiguousarray(pub, dtype=np.int32)
        want = np.array(want, dtype=np.float32, order="C")
        bracket = np.array(bracket, dtype=np.float32, order="C")
        assert done.shape == redo.shape == pub.shape == (len(pub),) and bracket.shape == (len(want), 2)
        self._check(self._lib.pct_selftest_levels_classify(self._h, _ptr(done, _i32p), _ptr(redo, _u32p), _ptr(pub, _i32p), len(pub), len(want),
                                                           float(log_edge), float(target), _ptr(want, _f32p), _ptr(bracket, _f32p)))
        return want, bracket

    def selftest_levels_bands(self, want, xyz, begin, end, log_edge0, window=-1, lo=0.0, hi=0.0):
        """k_band_hist and k_band_box over want[begin:end], xyz (n, 3).  window >= 0: the chain's bounds of the window of
        bins that starts there, else [lo, hi).  Returns (hist (160), exact, (lo, hi) used, box (6), count)."""
        want = np.ascontiguousarray(want, dtype=np.float32)
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        assert xyz.shape == (len(want), 3)
        hist, exact, count = np.empty(160, np.uint32), C.c_uint32(0), C.c_uint32(0)
        bounds, box = np.empty(2, np.float32), np.empty(6, np.float32)
        self._check(self._lib.pct_selftest_levels_bands(self._h, _ptr(want, _f32p), _ptr(xyz, _f32p), len(want), int(begin), int(end),
                                                        np.float32(log_edge0).item(), int(window), np.float32(lo).item(), np.float32(hi).item(),
                                                        _ptr(hist, _u32p), C.byref(exact), _ptr(bounds, _f32p), _ptr(box, _f32p), C.byref(count)))
        return hist, exact.value, bounds, box, count.value

    def selftest_levels_merge(self, pub, owned_pos, q_begin, nbr_pos, nbr_dist, nbr_cnt, row_done, k, pub_pos, pub_dist, pub_cnt, want):
        """k_merge_rows: the done rows of the pass table (nbr_pos, nbr_dist (n_rows, pitch), nbr_cnt or None) into copies of
        the public table (pub_pos, pub_dist (n_out, pitch), pub_cnt or None) and of want.  Returns those copies."""
        pub = np.ascontiguousarray(pub, dtype=np.int32)
        owned = np.ascontiguousarray(owned_pos, dtype=np.int32)
        npos = np.ascontiguousarray(nbr_pos, dtype=np.int32)
        ndist = np.ascontiguousarray(nbr_dist, dtype=np.float32)
        ncnt = None if nbr_cnt is None else np.ascontiguousarray(nbr_cnt, dtype=np.int32)
        done = np.ascontiguousarray(row_done, dtype=np.int32)
        ppos = np.array(pub_pos, dtype=np.int32, order="C")
        pdist = np.array(pub_dist, dtype=np.float32, order="C")
        pcnt = None if pub_cnt is None else np.array(pub_cnt, dtype=np.int32, order="C")
        want = np.array(want, dtype=np.float32, order="C")
        pitch = npos.shape[1]
        assert npos.shape == ndist.shape == (len(owned), pitch) and ppos.shape == pdist.shape == (len(ppos), pitch) and done.shape == owned.shape
        assert (ncnt is None or ncnt.shape == owned.shape) and (pcnt is None or pcnt.shape == (len(ppos),))
        self._check(self._lib.pct_selftest_levels_merge(self._h, _ptr(pub, _i32p), len(pub), _ptr(owned, _i32p), int(q_begin), _ptr(npos, _i32p),
                                                        _ptr(ndist, _f32p), None if ncnt is None else _ptr(ncnt, _i32p), _ptr(done, _i32p),
                                                        len(owned), int(k), pitch, len(ppos), _ptr(ppos, _i32p), _ptr(pdist, _f32p),
                                                        None if pcnt is None else _ptr(pcnt, _i32p), _ptr(want, _f32p), len(want)))
        return ppos, pdist, pcnt, want

    def synchronize(self):
        self._check(self._lib.pct_synchronize(self._h))

"""MI355X-backed ``PointCloud``: the reference's class surface for the curvature path.

Mirrors /root/reference/pointCloudToolbox.py:24-1009 for the methods on the hot
path: same constructor signature, same attribute names,
same curvature-array outputs, same exception types and messages.  The work is
done by hand-written HIP kernels behind the C ABI of ``include/pct_hip.h``;
there is no CPU fallback -- without the shared library or a gfx950 device the
compute methods raise.

Deliberate, documented differences (none changes a value):
* ``neighbor_indices`` / ``dists`` stay on the device and are downloaded on first
  access (400 MB at 1 M points, k=50);
* ``quadratic_coefficients`` is an (N, 6) float32 array and ``K_quadratic`` /
  ``H_quadratic`` / ``K_H_sq_quadratic`` are (N,) float32 arrays instead of
  Python lists of the same float32 values (pct:637, pct:659-661); every use in
  the reference's callers (len, indexing, np.save, np.isnan, iteration) works
  on both.
"""
from __future__ import annotations

import atexit
import threading
import zlib

import numpy as np

from . import _capi

__all__ = ["PointCloud"]

_ALGORITHMS = {"auto": _capi.KNN_AUTO, "brute": _capi.KNN_BRUTE, "grid": _capi.KNN_GRID,
               "grid_exact": _capi.KNN_GRID_EXACT, "grid_levels": _capi.KNN_GRID_LEVELS, "tree": _capi.KNN_TREE}


def _matrix_norms(points):
    """``np.linalg.norm(points, ord)`` for ord = 1, 2, inf (pct:45-47; nothing in the reference reads them) from one
    transposed copy of the (N, 3) matrix instead of three strided passes and an SVD: column sums accumulated in
    float64, the spectral norm as the square root of the largest eigenvalue of the 3x3 Gram matrix, the row sums in
    numpy's own order.  Same values up to rounding (numpy's float32 column sums are themselves only good to ~1e-4),
    ~6x faster per million points; non-finite input raises the LinAlgError the SVD would raise."""
    p = np.asarray(points)
    if p.ndim != 2 or p.shape[0] == 0 or p.shape[1] != 3 or p.dtype.kind != "f":
        return np.linalg.norm(points, 1), np.linalg.norm(points, 2), np.linalg.norm(points, np.inf)
    if p.dtype in (np.float32, np.float64) and p.flags.c_contiguous:
        try:
            cols, row_max, gram = _capi.matrix_norm_sums(p)       # one native multi-threaded pass (12 -> ~1 ms per million points)
        except _capi.HipExtensionError:
            cols = None
        if cols is not None:
            if not np.isfinite(gram).all() or not np.isfinite(row_max):
                raise np.linalg.LinAlgError("SVD did not converge")
            l2 = np.sqrt(max(np.linalg.eigvalsh(gram)[-1], 0.0))
            return p.dtype.type(cols.max()), p.dtype.type(l2), p.dtype.type(row_max)
    pt = np.ascontiguousarray(p.T)
    a = np.abs(pt)
    l1 = a.sum(1, dtype=np.float64).max()
    linf = ((a[0] + a[1]) + a[2]).max()
    p64 = pt.astype(np.float64, copy=False)
    gram = p64 @ p64.T
    if not np.isfinite(gram).all():
        raise np.linalg.LinAlgError("SVD did not converge")
    l2 = np.sqrt(max(np.linalg.eigvalsh(gram)[-1], 0.0))
    return p.dtype.type(l1), p.dtype.type(l2), linf


def _vectors3(x):
    """SciPy's check of the points handed to a tree: float64, the last axis of length 3."""
    x = np.asarray(x, dtype=np.float64)
    if x.shape[-1:] != (3,):
        raise ValueError(f"x must consist of vectors of length 3 but has shape {x.shape}")
    return x


class _DeviceTree:
    """``self.kdtree`` of the reference (SciPy's k-d tree of the float32 cloud, pct:74) as far as its callers use it
    (pct:625, 759, 844): ``query(x, k)`` for arbitrary points, answered on the device (``pct_query_points_algo`` with
    ``PCT_QUERY_AUTO``: the exhaustive sweep for a few points, the cell list for the points of another cloud -- the same
    rows either way).  Same return convention as SciPy: distances float64 ascending and indices, shape
    ``x.shape[:-1] + (k,)`` (the ``k`` axis squeezed for ``k == 1``), missing entries ``inf`` / ``n``.
    ``query_ball_point(x, r)`` is SciPy's radius search (``pct_query_ball``: rows of any length, ``d <= r`` inclusive),
    ``query_ball_point_csr`` the same rows as offsets and one index array."""

    def __init__(self, cloud):
        self._cloud = cloud
        self.n = cloud.num_points
        self.m = 3

    @property
    def data(self):
        return np.asarray(self._cloud.points, dtype=np.float32).astype(np.float64)

    def query(self, x, k=1, eps=0, p=2, distance_upper_bound=np.inf, workers=1):
        if eps != 0 or p != 2:
            raise NotImplementedError("only exact Euclidean queries (eps=0, p=2) run on the device")
        x = _vectors3(x)
        if not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError("k must be an integer >= 1")
        flat = x.reshape(-1, 3)
        bound = float(distance_upper_bound)
        idx, dist = self._cloud._ctx().query_points(flat, int(k), 0.0 if not np.isfinite(bound) else bound)
        shape = x.shape[:-1] + ((int(k),) if k > 1 else ())
        return dist.reshape(shape), idx.astype(np.intp).reshape(shape)

    def _ball_csr(self, flat, radii, sorted, distances, max_entries):
        """CSR rows of (m,3) queries with (m,) radii; the queries are chunked where one call would hold more than
        ``max_entries`` entries (the capped call's count pass gives the offsets the chunks are cut by)."""
        h = self._cloud._ctx()
        flags = (_capi.BALL_SORTED if sorted else 0) | (_capi.BALL_DISTANCES if distances else 0)
        one = len(radii) > 0 and bool((radii == radii[0]).all())
        st, offsets = h.query_ball(flat, radii[:1] if one else radii, flags, _capi.QUERY_AUTO, max_entries)
        if st == _capi.PCT_OK:
            got = h.get_ball(0, len(flat), want_dist=distances)
            return (offsets,) + (got if distances else (got,))
        idx = np.empty(int(offsets[-1]), np.int32)
        dist = np.empty(int(offsets[-1]), np.float64) if distances else None
        begin = 0
        while begin < len(flat):
            # as many rows as the budget holds, one at the least (a single row longer than the budget goes alone, uncapped)
            end = max(int(np.searchsorted(offsets, offsets[begin] + max_entries, side="right")) - 1, begin + 1)
            st, part = h.query_ball(flat[begin:end], radii[:1] if one else radii[begin:end], flags, _capi.QUERY_AUTO, 0)
            assert np.array_equal(part, offsets[begin:end + 1] - offsets[begin])
            got = h.get_ball(0, end - begin, want_dist=distances)
            idx[offsets[begin]:offsets[end]] = got[0] if distances else got
            if distances:
                dist[offsets[begin]:offsets[end]] = got[1]
            begin = end
        return (offsets, idx, dist) if distances else (offsets, idx)

    def _ball_arguments(self, x, r):
        x = _vectors3(x)
        if not np.isfinite(x).all():
            raise ValueError("'x' must be finite, check for nan or inf values")
        radii = np.empty(x.shape[:-1], np.float64)
        radii[...] = r                                   # SciPy's broadcast, and its error for a shape that does not fit
        return x, np.ascontiguousarray(x.reshape(-1, 3)), radii.reshape(-1)

    def query_ball_point(self, x, r, p=2., eps=0, workers=1, return_sorted=None, return_length=False, max_entries=1 << 28):
        """SciPy's ``query_ball_point``: the indices of every cloud point within ``r`` of ``x`` (inclusive), on the
        device (``pct_query_ball``).  A single point gives a list (an int with ``return_length``), an array of points an
        object array of lists (an int64 array of lengths); ``return_sorted=None`` sorts for a single point only.
        ``max_entries``: entries one device call may hold before the queries are chunked."""
        if eps != 0 or p != 2:
            raise NotImplementedError("only exact Euclidean queries (eps=0, p=2) run on the device")
        if return_sorted and return_length:
            raise ValueError("return_sorted and return_length cannot both be asked for")
        x, flat, radii = self._ball_arguments(x, r)
        if return_length:
            _, offsets = self._cloud._ctx().query_ball(flat, radii, _capi.BALL_COUNT_ONLY, _capi.QUERY_AUTO, 0)
            lengths = np.diff(offsets).reshape(x.shape[:-1])
            return int(lengths) if x.ndim == 1 else lengths
        sort = bool(return_sorted) or (return_sorted is None and x.ndim == 1)
        offsets, idx = self._ball_csr(flat, radii, sort, False, int(max_entries))
        if x.ndim == 1:
            return idx.tolist()
        out = np.empty(len(flat), dtype=object)
        rows = idx.tolist()
        for i in range(len(flat)):
            out[i] = rows[offsets[i]:offsets[i + 1]]
        return out.reshape(x.shape[:-1])

    def query_ball_point_csr(self, x, r, sorted=True, distances=False, max_entries=1 << 28):
        """The same rows without the Python lists: ``(offsets int64 (m + 1), indices int32[, distances float64])`` for the
        ``x.reshape(-1, 3)`` queries; row i is ``indices[offsets[i]:offsets[i + 1]]``."""
        x, flat, radii = self._ball_arguments(x, r)
        return self._ball_csr(flat, radii, bool(sorted), bool(distances), int(max_entries))


class PointCloud:

    # pct:26 -- identical signature and defaults
    def __init__(self, file_path=None, points=None, normals=None, downsample=False, voxel_size=0,
                 k_neighbors=20, output_path='./output/', max_points_per_voxel=1, device=0):
        self.downsample = downsample
        self.k_neighbors = k_neighbors
        self.voxel_size = voxel_size
        self.max_points_per_voxel = max_points_per_voxel
        self.output_path = output_path
        self.random_indexes = []
        self._device = device
        self._handle = None
        self._cloud_on_device = False
        self._table_on_device = False   # the neighbour table of the last planting is resident (and not yet replaced)
        self._uploaded_fp = None        # fingerprint of the points array the device cloud was uploaded from
        self._n_dev = 0                 # rows of the device cloud
        self._nbr_cache = None
        self._ball_counts = None        # members per row of the last compute_curvature_ball, until the next planting
        self._user_neighbors = None
        self._fit_on_device = False
        self._coefs_cache = None
        self._user_coefs = None
        self._device_curv = None
        self._plant_token = 0
        self._fit_token = -1
        self._fit_serial = 0            # counts the fits of this object: frames belong to one of them
        self._area_token = -1           # the planting whose per-point areas are on the device
        self._area_cache = None
        self._frame_key = None          # (planting, fit, viewpoint) whose surface frames are on the device
        self._frame_cache = None
        self._faces_token = -1          # the planting whose faces are in ``faces`` / ``natural_neighbors``
        self.eps = None
        self.collect_stats = False      # sweep statistics in last_timings (costs atomics)

        if file_path:
            self.file_path = file_path
            self.read_from_file()
        elif points is not None and normals is not None:
            self.points = points
            self.normals = normals
        else:
            raise ValueError("Either file_path or points and normals must be provided")      # pct:41

        # pct:43-47
        self.num_points = len(self.points)
        self.num_features = len(self.points[0])
        self.l1_norm, self.l2_norm, self.infinity_norm = _matrix_norms(self.points)

    # pct:50-66
    def read_from_file(self):
        points = _capi.load_text(self.file_path)           # np.loadtxt semantics, native multi-threaded parser
        self.points = points[:, 0:3].astype(np.float32)
        self.normals = points[:, 3:6].astype(np.float32)
        self.points[:, 0] -= np.max(self.points[:, 0])
        self.points[:, 1] -= np.max(self.points[:, 1])
        if self.downsample:
            # pct:59-60 calls a method the reference has commented out (pct:159-193)
            raise AttributeError("'PointCloud' object has no attribute 'downsample_point_cloud_by_grid'")
        self.x_domain = [np.min(self.points[:, 0]), np.max(self.points[:, 0])]
        self.y_domain = [np.min(self.points[:, 1]), np.max(self.points[:, 1])]
        self.z_domain = [np.min(self.points[:, 2]), np.max(self.points[:, 2])]

    # ---------------------------------------------------------------- device
    def _fingerprint(self):
        """Cheap identity of ``self.points`` as it is NOW: the object, its buffer and layout, and a checksum of about a
        thousand rows spread over the array.  Assigning ``pc.points`` or rewriting the array in place changes it (an
        in-place edit of a few rows between the sample can escape; plant_kdtree does not rely on it)."""
        p = self.points
        a = np.asarray(p)
        step = max(1, len(a) // 1024)
        sample = np.ascontiguousarray(a[::step]) if a.ndim == 2 else a
        return (id(p), a.shape, a.dtype.str, a.__array_interface__["data"][0], a.strides, zlib.crc32(sample.tobytes()))

    def _upload(self):
        """The cloud as ``self.points`` holds it now -> device (the reference builds its tree from the array of the
        moment, pct:74, and gathers from the array of the moment, pct:640)."""
        if self._handle is None:
            self._handle = _capi.acquire_handle(self._device)      # raises without library / GPU
            self._handle.set_stats(self.collect_stats)
        pts = np.asarray(self.points)
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise ValueError("points must have shape (N, 3)")
        if pts.dtype != np.float64:
            pts = pts.astype(np.float32, copy=False)
        self._handle.set_points(pts)
        self._table_on_device = False                      # a new cloud drops the device table
        self._cloud_on_device = True
        self._uploaded_fp = self._fingerprint()
        self._n_dev = len(pts)
        return self._handle

    def _ctx(self):
        if self._handle is None or not self._cloud_on_device:
            self._upload()
        return self._handle

    def close(self):
        """Release the device handle (an extension: the reference holds no device state).  Fitted coefficients that
        still live on the device are brought to the host first (24 B/point), so ``quadratic_coefficients`` and a later
        ``calculate_curvatures_...`` keep working; the neighbour table is dropped unless it has been read already."""
        if self._handle is not None:
            if self._fit_on_device and self._user_coefs is None:
                self._user_coefs = self.quadratic_coefficients
            _capi.release_handle(self._handle)              # (an idle context keeps its buffers for the next cloud)
            self._handle = None
            self._table_on_device = False
            self._cloud_on_device = False
            self._fit_on_device = False
            self._device_curv = None

    # ------------------------------------------------------------------ A3
    def plant_kdtree(self, k_neighbors, eps=None, algorithm="auto"):
        """k-NN table for every point (pct:69-89), computed on the GPU.

        ``eps`` (extension, README.md:8 / SURVEY A11): hybrid query, at most k
        neighbours with distance < eps; ``neighbor_counts`` then holds the
        number of valid entries per row.
        """
        self.k_neighbors = k_neighbors                      # pct:71
        self.eps = eps
        algo = _ALGORITHMS[algorithm]
        if self._fit_on_device and self._user_coefs is None and self._handle is not None:
            # the reference keeps the fitted coefficients across a re-planting (utils.py:495-501):
            # bring them to the host before the device results are invalidated
            self._user_coefs = self.quadratic_coefficients
        # pct:74 builds a NEW tree from self.points as they are at every planting: so does this (12 B/point over PCIe;
        # a cloud that was assigned or edited since the last call must not be answered from the old upload)
        h = self._upload()
        h.knn(k_neighbors, eps or 0.0, algo)
        self._table_on_device = True
        self.kdtree = _DeviceTree(self)                     # pct:74-75: the tree object later methods query
        self._nbr_cache = None
        self._ball_counts = None
        self._user_neighbors = None
        self._fit_on_device = False
        self._plant_token += 1
        self.last_timings = h.timings()

    def _download_neighbors(self):
        if self._nbr_cache is None:
            if self._handle is None or not self._table_on_device:
                raise AttributeError("'PointCloud' object has no attribute 'neighbor_indices'")
            idx, dist, cnt = self._handle.get_neighbors(0, self._n_dev, True, True, True)
            self._nbr_cache = (idx, dist, cnt)
        return self._nbr_cache

    @property
    def neighbor_indices(self):
        """(N, k) int32, rows ascending by distance, self excluded (pct:79, 85)."""
        if self._user_neighbors is not None:
            return self._user_neighbors
        return self._download_neighbors()[0]

    @neighbor_indices.setter
    def neighbor_indices(self, value):
        self._user_neighbors = np.asarray(value)      # used by the next fit; what has been fitted already stays (pct:637)

    @property
    def dists(self):
        """(N, k) float32 (pct:78, 84)."""
        return self._download_neighbors()[1]

    @property
    def neighbor_counts(self):
        if self._ball_counts is not None:
            return self._ball_counts
        return self._download_neighbors()[2]

    # ------------------------------------------------------------------ A4
    def fit_explicit_quadratic_surfaces_to_neighborhoods(self):
        """Plane-align + quadric fit of every neighbourhood (pct:635-647)."""
        h = self._ctx()
        if self._fingerprint() != self._uploaded_fp:
            # self.points were assigned or rewritten after the upload: pct:640 gathers the CURRENT coordinates with the
            # table of the last planting -- the table comes to the host (indices, distances, counts: the reference keeps
            # them as attributes) before the new upload drops it, and goes back as rows for the new cloud
            if self._table_on_device:
                self._download_neighbors()
                if self._user_neighbors is None:
                    self._user_neighbors = self._nbr_cache[0]
            h = self._upload()
        if self._user_neighbors is not None:
            h.fit_indices(self._user_neighbors)
        else:
            h.fit()                                          # AttributeError if no table (pct:640)
        # results stay on the device: coefficients (24 B/point) are downloaded on first access, K/H/H^2 by
        # calculate_curvatures_of_explicit_quadratic_surfaces_for_all_points()
        self._coefs_cache = None
        self._user_coefs = None
        self._device_curv = None
        self._fit_on_device = True
        self._fit_token = self._plant_token
        self._fit_serial += 1
        self.last_timings = h.timings()

    @property
    def quadratic_coefficients(self):
        """(N, 6) float32 [A, B, C, D, E, F] per point (pct:637-647), fetched from the device on first access."""
        if self._user_coefs is not None:
            return self._user_coefs
        if not self._fit_on_device:
            raise AttributeError("'PointCloud' object has no attribute 'quadratic_coefficients'")
        if self._coefs_cache is None:
            self._coefs_cache = self._handle.get_fit(0, self._n_dev, K=False, H=False, H2=False)[0]
        return self._coefs_cache

    @quadratic_coefficients.setter
    def quadratic_coefficients(self, value):
        self._user_coefs = value

    # ------------------------------------------------------------------ A8
    def calculate_curvatures_of_explicit_quadratic_surfaces_for_all_points(self):
        """K, H, H^2 from the fitted coefficients (pct:657-674)."""
        if self._user_coefs is None and self._fit_on_device and self._handle is not None:
            if self._device_curv is None:                    # produced by the fused kernel, still on the device
                self._device_curv = self._handle.get_fit(0, self._n_dev, coefs=False)[1:]
            K, H, H2 = self._device_curv
        else:                                                # coefficients the caller supplied, or a re-planted table
            K, H, H2 = self._ctx().curvatures_from_coefficients(np.asarray(self.quadratic_coefficients))
        self.K_quadratic = K
        self.H_quadratic = H
        self.K_H_sq_quadratic = H2
        return self.K_quadratic, self.H_quadratic

    # ------------------------------------------------------------------ A9
    def compute_pointwise_explicit_quadratic_curvature(self):
        """pct:505-509."""
        self.fit_explicit_quadratic_surfaces_to_neighborhoods()
        K, H = self.calculate_curvatures_of_explicit_quadratic_surfaces_for_all_points()
        return np.array(K), np.array(H)

    # ------------------------------------------------ mesh-free energies: the voronoi_areas of pct:650-655
    def _planted_table(self):
        """The handle, where the table of the last ``plant_kdtree`` is resident and is the one a fit would read."""
        if self._handle is None or not self._table_on_device:
            raise AttributeError("'PointCloud' object has no attribute 'neighbor_indices'")      # plant_kdtree first
        if self._user_neighbors is not None:
            raise ValueError("per-point areas are taken from the planted neighbour table, not from assigned neighbor_indices")
        return self._handle

    def _areas_on_device(self):
        return self._handle is not None and self._table_on_device and getattr(self, "_area_token", -1) == self._plant_token

    def compute_voronoi_areas(self):
        """Per-point area weights without a mesh: the area of every point's Voronoi cell in its own tangent plane, from the
        neighbourhoods of the last ``plant_kdtree`` and the device cloud of that planting (``pct_point_areas``,
        include/pct_hip.h) -- the ``voronoi_areas`` the reference's ``calculate_energies`` (pct:650-655) takes and nothing
        in it produces.  Returns (N,) float64; NaN for rows of fewer than two neighbours.  ``cells_closed`` tells the
        cells that the neighbourhood bounds on every side from those it leaves open (the rim of an open surface, k too small)."""
        h = self._planted_table()
        h.point_areas()
        self._area_token = self._plant_token
        self._area_cache = None
        self.last_area_stats = h.point_area_stats()
        return self.voronoi_areas

    def _download_areas(self):
        if not self._areas_on_device():
            self.compute_voronoi_areas()
        if self._area_cache is None:
            self._area_cache = self._handle.get_point_areas(0, self._n_dev, nverts=False)[:2]
        return self._area_cache

    @property
    def voronoi_areas(self):
        """(N,) float64, computed on first access after a planting and kept until the next one."""
        return self._download_areas()[0]

    @property
    def cells_closed(self):
        """(N,) bool: the cell is bounded by the point's own neighbours."""
        return self._download_areas()[1].astype(bool)

    def compute_point_energies(self, closed_only=False):
        """``(bending, stretching, area)`` of the cloud without a mesh: sum (h ** 2) * area and sum k * area (pct:652-653)
        over the per-point areas, and their sum, in float64 on the device -- over the rows whose area, K and H are no NaN,
        the closed cells only with ``closed_only``.  Runs the fit and the areas where they are not resident for the
        planted table; three doubles come back."""
        h = self._planted_table()
        if not (self._fit_on_device and self._fit_token == self._plant_token and self._user_coefs is None):
            self.fit_explicit_quadratic_surfaces_to_neighborhoods()
            h = self._planted_table()
        if not self._areas_on_device():
            h.point_areas()
            self._area_token = self._plant_token
            self._area_cache = None
            self.last_area_stats = h.point_area_stats()
        bending, stretching, area, _ = h.point_energies(closed_only)
        return bending, stretching, area

    # ------------------------------------------------ surface frames: what the quadric fit knows beyond K and H
    def _frames_on_device(self, key):
        return self._handle is not None and self._table_on_device and self._fit_on_device and self._frame_key == key

    def compute_surface_frames(self, viewpoint=None):
        """Per-point frames of the fitted patches (``pct_point_frames``, include/pct_hip.h): the unit normal, the principal
        curvatures k1 >= k2 (what ``calculate_explicit_quadratic_curvatures`` returns per call, pct:425-431) and their
        directions.  ``viewpoint`` -- three numbers in the cloud's coordinates, a scanner position -- turns every normal
        to its side; H and k1, k2 are signed relative to the normal, so ``H_signed_quadratic`` then has one sign
        convention over the whole cloud, which ``H_quadratic`` (signed by each row's far-minus-near rule, pct:286-297)
        does not.  Without it the normals stay on the side the fit chose.  Runs the fit first where it is not resident for
        the planted table.  Returns ``(normals (N, 3), k1 (N,), k2 (N,), directions (N, 3, 2))``, float64, and sets
        ``normals``, ``k1_quadratic``, ``k2_quadratic``, ``principal_directions_quadratic``, ``normals_flipped``,
        ``H_signed_quadratic`` and ``last_frame_stats``."""
        h = self._planted_table()
        if not (self._fit_on_device and self._fit_token == self._plant_token and self._user_coefs is None):
            self.fit_explicit_quadratic_surfaces_to_neighborhoods()
            h = self._planted_table()
        view = None if viewpoint is None else tuple(float(x) for x in np.asarray(viewpoint, np.float64).reshape(3))
        key = (self._plant_token, self._fit_serial, view)
        if not self._frames_on_device(key) or self._frame_cache is None:
            h.point_frames(view)
            self._frame_key = key
            self.last_frame_stats = h.point_frame_stats()
            normal, k12, dirs, flipped = h.get_point_frames(0, self._n_dev)
            H = h.get_fit(0, self._n_dev, coefs=False, K=False, H2=False)[2]
            self._frame_cache = (normal, np.ascontiguousarray(k12[:, 0]), np.ascontiguousarray(k12[:, 1]), dirs,
                                 flipped.astype(bool), np.where(flipped.astype(bool), -H, H).astype(np.float32))
        normal, k1, k2, dirs, flipped, H_signed = self._frame_cache
        self.normals = normal
        self.k1_quadratic, self.k2_quadratic = k1, k2
        self.principal_directions_quadratic = dirs
        self.normals_flipped = flipped
        self.H_signed_quadratic = H_signed
        return normal, k1, k2, dirs

    def orient_normals_consistently(self, anchor="top", viewpoint=None, max_components=None):
        """Turns the normals of the fitted patches so that neighbouring points agree (``pct_orient_frames``,
        include/pct_hip.h): a flood over the planted neighbour table -- the step the reference's pipeline takes from Open3D
        (``orient_normals_consistent_tangent_plane``, utils:80) and its README promises as "consistency in curvature
        signs".  ``anchor`` decides the side of each connected component as a whole: "top" (the highest point's normal
        points up: outward on a closed surface), "view" (to the side of ``viewpoint``) or "seed" (as flooded).  Computes the
        frames first (``compute_surface_frames``) where none are cached.  Refreshes ``normals``, ``k1_quadratic``,
        ``k2_quadratic``, ``principal_directions_quadratic``, ``normals_flipped`` and ``H_signed_quadratic`` from the
        device, sets ``normal_components`` (int32, -1: not reached) and ``last_orientation_stats``, and returns the
        normals.  ``compute_surface_frames`` with the same arguments, ``compute_normals`` and the PLY export serve the
        oriented values until the next planting or fit."""
        if self._frame_key is None or self._frame_key[:2] != (self._plant_token, self._fit_serial) or \
                not self._frames_on_device(self._frame_key) or self._frame_cache is None:
            self.compute_surface_frames()
        h = self._planted_table()
        h.orient_frames(anchor, viewpoint, max_components)
        self.last_orientation_stats = h.orient_stats()
        normal, k12, dirs, flipped = h.get_point_frames(0, self._n_dev)
        H = h.get_fit(0, self._n_dev, coefs=False, K=False, H2=False)[2]
        self._frame_cache = (normal, np.ascontiguousarray(k12[:, 0]), np.ascontiguousarray(k12[:, 1]), dirs,
                             flipped.astype(bool), np.where(flipped.astype(bool), -H, H).astype(np.float32))
        self.normal_components = h.get_orientation(0, self._n_dev)[0]
        self.normals, self.k1_quadratic, self.k2_quadratic, self.principal_directions_quadratic, self.normals_flipped, \
            self.H_signed_quadratic = self._frame_cache
        return self.normals

    def compute_normals(self):
        """pct:691-697 -- there through PyVista and a Delaunay mesh; here the normals of the fitted patches
        (``compute_surface_frames`` without a viewpoint).  Sets ``self.normals``."""
        self.compute_surface_frames()

    # ------------------------------------------------ faces: triangles from the tangent-plane Voronoi cells
    def compute_surface_triangles(self, use_frames=None):
        """Triangles of the surface without leaving the device (``pct_point_triangles``, include/pct_hip_surface.h): every
        point's Voronoi cell in its own tangent plane gives its natural neighbours in order, two consecutive ones propose a
        triangle, and the triangles all three of their corners propose are kept -- the role ball pivoting plays in the
        reference's pipeline (utils:92-96).  ``use_frames``: wind every face counter-clockwise about the normal of its
        lowest corner as the resident frames hold it (after ``orient_normals_consistently``: one side per component);
        default: where frames of this planting and fit are resident.  Without them the winding follows the fit's own side.
        Sets ``faces`` (T, 3) int32 -- the attribute the reference's export reads (pct:711) --, ``natural_neighbors``
        ((N + 1,) int64 offsets, int32 indices) and ``last_triangle_stats``; returns ``faces``."""
        h = self._planted_table()
        resident = self._frame_key is not None and self._frame_key[:2] == (self._plant_token, self._fit_serial) and \
            self._frames_on_device(self._frame_key)
        if use_frames is None:
            use_frames = resident
        if use_frames and not resident:
            raise ValueError("no surface frames of this planting and fit on the device (compute_surface_frames)")
        h.point_triangles(bool(use_frames))
        self.last_triangle_stats = h.point_triangle_stats()
        self.faces = h.get_triangles(0, self.last_triangle_stats["triangles"])
        self.natural_neighbors = h.get_point_fans(0, self._n_dev)
        self._faces_token = self._plant_token
        return self.faces

    def fill_surface_holes(self, max_vertices=32, max_perimeter=None, update_faces=True):
        """Close the small gaps ``compute_surface_triangles`` leaves, without leaving the device (``pct_fill_holes``,
        include/pct_hip_holes.h): the boundary loops of the faces are read off the fans, and every loop of at most
        ``max_vertices`` (3 .. 32) vertices whose perimeter is below ``max_perimeter`` gets the triangulation of least total
        squared area -- the step behind ball pivoting in the reference's pipeline (utils:150-206).  ``max_perimeter=None``:
        half the mean extent of the bounding box (utils:173, utils:338-339); ``float("inf")``: no cap.  Computes the faces
        first where they are missing.  Sets ``hole_faces`` (P, 3) int32, ``boundary_loops`` ((loops + 1,) int64 offsets,
        int32 vertices in canonical order, uint8 status: 0 filled, 1 left for its perimeter, 2 blocked) and
        ``last_hole_stats``; with ``update_faces`` also ``faces``, to the filled array, which the PLY export and
        ``compute_mesh_energies`` then read.  A later ``compute_surface_triangles`` restores the unfilled faces.
        Returns the filled array."""
        h = self._planted_table()
        if getattr(self, "faces", None) is None or self._faces_token != self._plant_token or h.point_triangle_stats()["rows"] == 0:
            self.compute_surface_triangles()
        if max_perimeter is None:
            p = np.asarray(self.points, np.float64)
            ext = p.max(0) - p.min(0)
            max_perimeter = 0.5 * (((ext[0] + ext[1]) + ext[2]) / 3.0)
        h.fill_holes(max_vertices, max_perimeter)
        self.last_hole_stats = h.fill_hole_stats()
        self.hole_faces = h.get_hole_triangles(0, self.last_hole_stats["patch_triangles"])
        self.boundary_loops = h.get_boundary_loops()
        filled = h.get_filled_triangles(0, self.last_triangle_stats["triangles"] + self.last_hole_stats["patch_triangles"])
        if update_faces:
            self.faces = filled
        return filled

    def compute_mesh_energies(self):
        """``(bending, stretching, area)`` over ``faces`` (utils.py:702-765 on this cloud's own triangles): the cloud,
        ``faces``, ``K_quadratic`` and ``H_quadratic`` through ``pct_mesh_energies``.  Computes the faces and the
        curvatures of the planted table where they are missing."""
        if getattr(self, "faces", None) is None or self._faces_token != self._plant_token:
            self.compute_surface_triangles()
        if not hasattr(self, "K_quadratic"):
            self.compute_pointwise_explicit_quadratic_curvature()
        from . import energies
        return energies.mesh_energies(np.asarray(self.points), self.faces, self.K_quadratic, self.H_quadratic, self._device)

    def export_ply_with_curvature_and_normals(self, filename):
        """pct:699-726: ASCII PLY vertices ``x y z nx ny nz gaussian_curvature mean_curvature`` and, once ``faces`` has been
        computed (``compute_surface_triangles``; pct:711), the face element behind them.  Computes the normals first when
        ``self.normals`` is missing or is not one normal per point (pct:701-702)."""
        normals = getattr(self, "normals", None)
        if normals is None or np.shape(normals) != (len(self.points), 3):
            self.compute_normals()
        faces = getattr(self, "faces", None)
        if faces is not None and len(faces) > 0:
            _capi.write_ply_ascii_faces(filename, np.asarray(self.points), self.normals, self.K_quadratic, self.H_quadratic, faces)
        else:
            _capi.write_ply_ascii_normals(filename, np.asarray(self.points), self.normals, self.K_quadratic, self.H_quadratic)

    def export_ply_with_curvatures(self, filename='output_with_curvatures.ply'):
        """The ASCII PLY validate_shape writes after the curvature step (utils.py:538-551), same bytes."""
        _capi.write_ply_ascii(filename, np.asarray(self.points), self.K_quadratic, self.H_quadratic)

    # ----------------------------------------------------------------- A10
    def explicit_quadratic_neighbor_study(self, tol=1e-7, sample_size=500, lower_bound=3, upper_bound=99):
        """Neighbour count at which the Gaussian curvature stops changing (pct:732-800).

        Same draw (``np.random.randint`` on the global generator, pct:753), same per-point bisection
        (pct:772-789) and same return value ``int(mean) + 1`` (pct:800) as the reference.  The curvature
        K(n) of "the point itself plus its n nearest neighbours" (pct:759-761) is evaluated on the GPU for
        every n the bisection can ask for, from a k = upper_bound+1 neighbour table.
        """
        num_total = len(self.points)
        sample_size = min(sample_size, num_total)
        random_indexes = np.random.randint(0, num_total, sample_size)                  # pct:753
        if sample_size == 0:
            return 0                                                                   # pct:797-798
        need = upper_bound + 1
        h = self._ctx()
        own = self._table_on_device and getattr(h, "k", 0) >= need and not self.eps and self._user_neighbors is None
        if not own:      # keep the planted table untouched: a second context does the k=need sweep
            h = _capi.Handle(self._device)
            pts = np.asarray(self.points)
            h.set_points(pts if pts.dtype == np.float64 else pts.astype(np.float32, copy=False))
            h.knn(need)
        try:
            Kn = h.neighbor_study_curvatures(random_indexes, lower_bound, need)        # columns n = lower..upper+1
        finally:
            if not own:
                h.close()
        converged = []
        for row in Kn:
            lower, upper, best = lower_bound, upper_bound, None
            while lower <= upper:                                                      # pct:778-786
                mid = (lower + upper) // 2
                if abs(row[mid + 1 - lower_bound] - row[mid - lower_bound]) < tol:
                    best, upper = mid, mid - 1
                else:
                    lower = mid + 1
            converged.append(upper if best is None else best)                          # pct:787-788
        return int(np.mean(converged)) + 1                                             # pct:800

    # fused entry: k-NN -> fit -> curvature with nothing but K/H leaving the GPU
    def compute_curvature_fused(self, k_neighbors, eps=None, algorithm="auto"):
        self.k_neighbors = k_neighbors
        self.eps = eps
        algo = _ALGORITHMS[algorithm]
        h = self._upload()                                 # the cloud of the moment, as plant_kdtree (pct:74)
        h.curvature(k_neighbors, eps or 0.0, algo)
        self._table_on_device = True
        self._nbr_cache = None
        self._ball_counts = None
        self._user_neighbors = None
        _, K, H, H2 = h.get_fit(0, self._n_dev, coefs=False)
        self.K_quadratic, self.H_quadratic, self.K_H_sq_quadratic = K, H, H2
        self._plant_token += 1
        self._fit_token = self._plant_token
        self._fit_on_device, self._user_coefs, self._coefs_cache, self._device_curv = True, None, None, (K, H, H2)
        self.last_timings = h.timings()
        return K, H

    # curvature over radius neighbourhoods: every point within r of each centre (the usual scan-processing form; the
    # hybrid form "at most k within eps" is plant_kdtree(k, eps))
    def compute_curvature_ball(self, radius, rows=None, max_entries=1 << 28):
        """Quadric-fit curvature of the neighbourhoods ``{p : |p - points[c]| <= radius}`` (inclusive, ``c`` itself left
        out) of the centres ``c`` in ``rows`` (default: every point), on the device: ``pct_query_ball`` with the centres'
        own native-dtype coordinates as queries, then ``pct_fit_ball`` on the resident rows, at any row length.
        ``radius``: a scalar, or one radius per centre.  The centres are chunked where one query would hold more than
        ``max_entries`` entries (cut by the count pass's offsets).  Returns ``(K, H)`` float32 and sets ``K_quadratic``,
        ``H_quadratic``, ``K_H_sq_quadratic``, ``quadratic_coefficients`` and ``neighbor_counts`` for the given rows."""
        h = self._upload()                                 # the cloud of the moment, as plant_kdtree (pct:74)
        pts = np.asarray(self.points)
        centres = np.arange(len(pts), dtype=np.int64) if rows is None else np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        if len(centres) and (centres.min() < 0 or centres.max() >= len(pts)):
            raise ValueError("rows outside the cloud")
        radii = np.empty(len(centres), np.float64)
        radii[...] = radius                                # a scalar, or one per centre (NumPy's broadcast and its error)
        flat = np.ascontiguousarray(pts[centres], dtype=np.float64)     # float32 coordinates widened, float64 as they are
        one = len(radii) > 0 and bool((radii == radii[0]).all())
        max_entries = int(max_entries)
        m = len(centres)
        coefs, K, H, H2 = np.empty((m, 6), np.float32), np.empty(m, np.float32), np.empty(m, np.float32), np.empty(m, np.float32)
        used = np.empty(m, np.int32)

        def fit(begin, end):                               # the rows [begin, end) are resident
            used[begin:end] = h.fit_ball(centres[begin:end])
            coefs[begin:end], K[begin:end], H[begin:end], H2[begin:end] = h.get_fit(0, end - begin)

        st, offsets = h.query_ball(flat, radii[:1] if one else radii, 0, _capi.QUERY_AUTO, max_entries)
        if st == _capi.PCT_OK:
            fit(0, m)
        else:                                              # PCT_ERR_LIMIT: the same cut as _DeviceTree._ball_csr
            begin = 0
            while begin < m:
                end = max(int(np.searchsorted(offsets, offsets[begin] + max_entries, side="right")) - 1, begin + 1)
                h.query_ball(flat[begin:end], radii[:1] if one else radii[begin:end], 0, _capi.QUERY_AUTO, 0)
                fit(begin, end)
                begin = end
        # the fit results on the device are those of the last chunk, and the neighbour table (if any) went with the upload
        self._table_on_device = False
        self._fit_on_device = False
        self._device_curv = None
        self._coefs_cache = None
        self._user_coefs = coefs
        self._user_neighbors = None
        self._nbr_cache = None
        self._ball_counts = used
        self.K_quadratic, self.H_quadratic, self.K_H_sq_quadratic = K, H, H2
        self.last_timings = h.timings()
        return K, H

    # ------------------------------------------------------- PCA estimator
    def principal_curvatures_via_principal_component_analysis(self, k_neighbors, algorithm="auto"):
        """Eigenvalues of every neighbourhood's covariance as 'principal curvatures' (pct:901-950), on the GPU.

        Sets ``pca_principal_curvature_values_1`` / ``_2`` (the two largest eigenvalues), ``principal_curvature_directions``
        (N, 3, 2: their eigenvectors as columns), ``pca_K_values`` and ``pca_H_values``, all float64, and returns None.
        The neighbourhoods are the reference's: the k nearest points in the cloud's dtype, the point itself dropped.  The
        work runs on a device handle of its own: the planted table, the fit results and ``kdtree`` stay as they are.
        ``algorithm`` (extension, as ``plant_kdtree``) picks the sweep that fetches the candidates; the values do not
        depend on it.  Eigenvector signs: the component of largest magnitude is positive (the reference's are LAPACK's)."""
        pts = np.asarray(self.points)
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise ValueError("points must have shape (N, 3)")
        algo = _ALGORITHMS[algorithm]
        n = len(pts)
        if n == 0:                                           # the reference's loop runs zero times
            l1, l2, K, H, dirs = np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros((0, 3, 2))
        else:
            if min(int(k_neighbors), n - 1) < 2:             # np.cov of < 2 neighbours is NaN: eigh refuses it (pct:925)
                raise ValueError("array must not contain infs or NaNs")
            if pts.dtype != np.float64:
                pts = pts.astype(np.float32, copy=False)
            h = _capi.acquire_handle(self._device)
            try:
                h.set_points(pts)
                self.pca_exact_rows = h.pca_curvatures(int(k_neighbors), algo)
                l1, l2, dirs, K, H = h.get_pca(0, n)
                self.last_pca_timings = h.timings()
            finally:
                _capi.release_handle(h)
        self.pca_principal_curvature_values_1 = l1
        self.pca_principal_curvature_values_2 = l2
        self.principal_curvature_directions = dirs
        self.pca_K_values = K
        self.pca_H_values = H

    # --------------------------------------------------------- staticmethods
    # The reference calls these once per point in a Python loop (pct:644-647, 668): one device context serves all
    # calls of the process (created on first use, released at exit), under a lock -- a handle has ONE stream.
    @staticmethod
    def get_best_fit_plane_and_rotate(points):
        """pct:270-321 for one neighbourhood: (k, 3) -> (k, 3) float64 with the best-fit normal on +z."""
        pts = np.asarray(points)
        if not np.all(np.isfinite(pts)):
            raise ValueError("Non-finite values in input points")                      # pct:273-274
        if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] < 2:
            return _reference_small_case(pts)
        with _static_lock:
            rotated = _static_handle().plane_rotate(pts[None])[0]
        if not np.all(np.isfinite(rotated)):
            raise ValueError("Non-finite values after rotation")                       # pct:318-319
        return rotated

    @staticmethod
    def fit_quadratic_surface(points):
        """pct:331-360 for one neighbourhood: (N, 3) [a, b, z] -> float32 (6,) [A, B, C, D, E, F]."""
        points = np.array(points, dtype=np.float32)                                    # pct:350
        if points.ndim != 2 or points.shape[1] != 3:
            raise ValueError("Input points must have shape (N, 3)")                    # pct:351-352
        if not np.all(np.isfinite(points)):
            raise ValueError("Input contains non-finite values.")                      # pct:356-357
        if points.shape[0] == 0:
            raise np.linalg.LinAlgError("0-dimensional array given")                   # what lstsq says to an empty system
        with _static_lock:
            return _static_handle().fit_quadric(points[None])[0]

    @staticmethod
    def calculate_explicit_quadratic_curvatures(coefficients):
        """pct:398-431 for one coefficient vector (device evaluation)."""
        c = np.asarray(coefficients, dtype=np.float32).reshape(1, 6)
        with _static_lock:
            K, H, H2 = _static_handle().curvatures_from_coefficients(c)
        disc = max(H[0] ** 2 - K[0], 0)                      # pct:425
        root = np.sqrt(disc)
        return K[0], H[0], H[0] + root, H[0] - root, H2[0]


_static_lock = threading.Lock()
_static = {"handle": None}


def _static_handle():
    if _static["handle"] is None:
        _static["handle"] = _capi.Handle(0)                 # raises without library / GPU: no CPU fallback
        atexit.register(_close_static_handle)
    return _static["handle"]


def _close_static_handle():
    h, _static["handle"] = _static["handle"], None
    if h is not None:
        h.close()


def _reference_small_case(pts):
    """What pct:277-280 does with a block the device path does not take (measured with NumPy 2.2): one point or none --
    np.cov has nothing to average, the covariance is NaN and np.linalg.svd raises LinAlgError("SVD did not converge");
    a 1-D array -- np.cov returns a scalar and svd refuses it; (m, c != 3) -- svd works but the rotation of pct:315
    cannot be formed (ValueError from the matrix product)."""
    if pts.ndim == 1:
        raise np.linalg.LinAlgError("0-dimensional array given. Array must be at least two-dimensional")
    if pts.ndim == 2 and pts.shape[1] == 3:
        raise np.linalg.LinAlgError("SVD did not converge")
    raise ValueError("Input points must have shape (N, 3)")

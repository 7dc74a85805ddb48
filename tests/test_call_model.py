"""The call-sequence driver would notice (no GPU): tests/call_driver.py against a FakeHandle that IS the model.

The FakeHandle executes tests/call_model.py -- every call moves a `State` through `call_model.apply`, every getter returns
values hashed from the provenance of what it serves, so two fake handles agree exactly where the header says two real
ones must.  With it: the committed seeds run clean; every seeded defect (one per "drops" and per "untouched" clause the
header has) is caught by a committed seed within its committed steps; every modelled entry point is issued at least five
times and every (operation, precondition) pair of the model refused at least twice -- pct_orient_frames also while an orientation is
resident; and every name of `_capi.SIGNATURES` is modelled or excluded
with a reason."""
import os
import re
import zlib

import numpy as np
import pytest

import call_driver as D
import call_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_M1, _M2, _M3 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def _seed(*prov):
    return zlib.crc32(repr(prov).encode())


def _mix(seed, a, b=0):
    a, b = np.asarray(a).astype(np.uint64), np.asarray(b).astype(np.uint64)
    with np.errstate(over="ignore"):
        x = (a + np.uint64(1)) * _M1 + (b + np.uint64(1)) * _M3 + np.uint64(seed) * _M2
        x = (x ^ (x >> np.uint64(31))) * _M2
        return x ^ (x >> np.uint64(29))


def _f(x):
    return (x % np.uint64(1000003)).astype(np.float64) / 1000.0 - 500.0


def _crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


# what an operation makes anew: keeping the one before cannot show
_MAKES = {"knn": ("table",), "curvature": ("table", "fit"), "surface_variation": ("table",), "fit": ("fit",), "fit_indices": ("fit",), "fit_ball": ("fit",),
          "point_areas": ("areas",), "point_frames": ("frames",), "point_triangles": ("triangles",), "pca_curvatures": ("pca",), "query_ball": ("ball",)}
# one defect per operation and per result its "drops" clause names: defect -> (operations, residents wrongly kept).  (An
# orientation goes with its frames: kept alone it is probed where the frames are made anew, by pct_point_frames.)
EVERY_KEEP = {f"{op} keeps the {r}": ((op,), (r,)) for op, o in M.OPS.items() for r in o.drops
              if r in ("table", "fit", "areas", "frames", "pca", "ball") and r not in _MAKES.get(op, ())}
# the same by the header's clauses, as the issue lists them
KEEPS = {
    "a planting keeps the areas": (("knn", "curvature"), ("areas",)),
    "a planting keeps the frames": (("knn", "curvature"), ("frames",)),
    "a fit keeps the frames": (("fit", "fit_indices", "fit_ball"), ("frames",)),
    "pct_point_frames keeps the orientation": (("point_frames",), ("orient",)),
    "a range change keeps the fit": (("set_query_range",), ("fit",)),
    "a range change keeps the areas": (("set_query_range",), ("areas",)),
    "a new cloud keeps the ball rows": (D._CLOUD_OPS, ("ball",)),
    "a new cloud keeps the PCA results": (D._CLOUD_OPS, ("pca",)),
    "the table readable after voxel_downsample": (("voxel_downsample", "voxel_downsample_f32"), ("table",)),
    "surface_variation keeps the fit": (("surface_variation",), ("fit",)),
    "pct_pca_curvatures keeps the areas": (("pca_curvatures",), ("areas",)),
    "a planting keeps the triangles": (("knn", "curvature", "surface_variation", "pca_curvatures"), ("triangles",)),
    "a change of ownership keeps the triangles": (("set_query_range", "set_query_slab"), ("triangles",)),
    "a new cloud keeps the triangles": (D._CLOUD_OPS, ("triangles",)),
    "a new pct_point_triangles keeps the hole results": (("point_triangles",), ("holes",)),
    "a planting keeps the hole results": (("knn", "curvature", "surface_variation", "pca_curvatures"), ("holes",)),
    "a change of ownership keeps the hole results": (("set_query_range", "set_query_slab"), ("holes",)),
}
# defect -> (operations, residents the operation wrongly drops)
DROPS = {
    "voxel_downsample drops the areas": (("voxel_downsample", "voxel_downsample_f32"), ("areas",)),
    "voxel_downsample drops the frames": (("voxel_downsample", "voxel_downsample_f32"), ("frames", "orient")),
    "a range change drops the ball rows": (("set_query_range",), ("ball",)),
    "a planting drops the PCA results": (("knn", "curvature"), ("pca",)),
    "pct_fit_indices drops the areas": (("fit_indices",), ("areas",)),
    "pct_point_areas drops the frames": (("point_areas",), ("frames", "orient")),
    "a fit drops the triangles": (("fit", "fit_indices", "fit_ball"), ("triangles",)),
    "pct_point_frames drops the triangles": (("point_frames",), ("triangles",)),
    "pct_orient_frames drops the triangles": (("orient_frames",), ("triangles",)),
    "voxel_downsample drops the triangles": (("voxel_downsample", "voxel_downsample_f32"), ("triangles",)),
    "a fit drops the hole results": (("fit", "fit_indices", "fit_ball"), ("holes",)),
    "pct_point_frames drops the hole results": (("point_frames",), ("holes",)),
    "voxel_downsample drops the hole results": (("voxel_downsample", "voxel_downsample_f32"), ("holes",)),
}
SPECIAL = ["fit_indices results served as cloud-aligned", "PCA leaves its over-fetched table valid", "query_points through the cell list disturbs the table",
           "fit_ball disturbs the ball rows", "a refused call changes state", "an async read served before the pending call is folded in",
           "a refused pct_point_triangles drops the triangles", "triangles wound by the frames as they are now, not as the call found them"]
KEEPS.update(EVERY_KEEP)
DEFECTS = list(KEEPS) + list(DROPS) + SPECIAL


class FakeHandle:
    """`_capi.Handle`'s methods over a `call_model.State`; `defect` names one way of breaking the header's rules."""

    def __init__(self, defect=None):
        self.s, self.defect = M.State(), defect
        self.pts = None
        self.mem, self.next_ptr = {}, 4096
        self.plant_algo = D.KNN_BRUTE
        self.ball_q = None
        self.stale = None                  # (table, fit) as they were before a pending asynchronous call
        self.memo = {}

    def close(self):
        pass

    # -- the model, executed ----------------------------------------------------------------------------------------------
    def _call(self, name, args):
        old = self.s
        status, new = M.apply(old, name, args)
        d = self.defect
        if status == M.OK:
            ops, keep = KEEPS.get(d, ((), ()))
            if name in ops:
                for r in keep:
                    if getattr(new, r) is None: setattr(new, r, getattr(old, r))
            ops, drop = DROPS.get(d, ((), ()))
            if name in ops:
                for r in drop: setattr(new, r, None)
            if d == "PCA leaves its over-fetched table valid" and name == "pca_curvatures":
                new.table = {"k": min(new.pca["k"] + 8, new.n - 1), "eps": 0.0, "lo": 0, "hi": new.n}
            if d == "query_points through the cell list disturbs the table" and name == "query_points_algo" and args["algo"] == D.QUERY_GRID and new.table:
                new.table = dict(new.table, disturbed=True)
            if d == "fit_ball disturbs the ball rows" and name == "fit_ball":
                new.ball = dict(new.ball, disturbed=True)
        elif d == "a refused call changes state" and status != M.LIMIT:
            new.fit = new.orient = None
        elif d == "a refused pct_point_triangles drops the triangles" and name == "point_triangles":
            new.triangles = None
        if M.OPS[name].folds and not new.pending:
            if not (d == "an async read served before the pending call is folded in" and name in ("get_fit", "get_neighbors")): self.stale = None
        self.s = new
        if status not in (M.OK, M.LIMIT):
            raise M.RAISES[status](f"{name}: {M.check(old, name, args)[1]}")
        return status

    def _key(self):
        return self.s.cloud["key"]

    # -- clouds and settings ----------------------------------------------------------------------------------------------
    def _load(self, name, pts):
        pts = np.ascontiguousarray(pts)
        self._call(name, {"serial": 0, "n": len(pts), "key": D.cloud_key(pts), "pts": pts})
        self.pts, self.n, self._rows, self.stale = pts, len(pts), len(pts), None

    def set_points(self, pts):
        pts = np.asarray(pts)
        self._load("set_points_f64" if pts.dtype == np.float64 else "set_points_f32", pts if pts.dtype == np.float64 else pts.astype(np.float32))

    def device_alloc(self, nbytes):
        self.next_ptr += 4096
        self.mem[self.next_ptr] = bytearray(int(nbytes))
        return self.next_ptr

    def device_free(self, ptr): del self.mem[ptr]

    def device_upload(self, ptr, host):
        b = np.ascontiguousarray(host).tobytes()
        self.mem[ptr][:len(b)] = b

    def device_download(self, ptr, host):
        host[...] = np.frombuffer(bytes(self.mem[ptr][:host.nbytes]), host.dtype).reshape(host.shape)

    def set_points_device(self, ptr, n): self._load("set_points_device", np.frombuffer(bytes(self.mem[ptr][:n * 12]), np.float32).reshape(n, 3))
    def use_points_device(self, ptr, n): self._load("use_points_device", np.frombuffer(bytes(self.mem[ptr][:n * 12]), np.float32).reshape(n, 3))
    def set_query_range(self, b, e): self._call("set_query_range", {"lo": int(b), "hi": int(e)})
    def set_query_slab(self, part, parts): self._call("set_query_slab", {"part": part, "parts": parts})
    def set_stats(self, v=True): self._call("set_stats", {"value": bool(v)})
    def set_grid_param(self, v): self._call("set_grid_param", {"value": float(v)})
    def set_async(self, v=True): self._call("set_async", {"value": bool(v)})
    def timings(self): self._call("get_timings", {}); return {"algo": self.plant_algo}
    def stage_times_done(self): self._call("get_timings_done", {}); return None
    def synchronize(self): self._call("synchronize", {})

    # -- plantings and fits -----------------------------------------------------------------------------------------------
    def knn(self, k, eps=0.0, algo=0):
        self._call("knn", {"k": int(k), "eps": float(eps), "algo": algo}); self.plant_algo = algo

    def curvature(self, k, eps=0.0, algo=0):
        before = (self.s.table, self.s.fit)
        self._call("curvature", {"k": int(k), "eps": float(eps), "algo": algo}); self.plant_algo = algo
        if self.s.pending and self.stale is None: self.stale = before

    def fit(self): self._call("fit", {})

    def _table(self, t):
        """(idx, dist, cnt) of the whole cloud for a table's provenance."""
        n, k = self.s.n, t["k"]
        sd = _seed("table", self._key(), k, t["eps"], t.get("disturbed"))
        if ("table", sd) not in self.memo:
            if len(self.memo) > 6: self.memo.clear()
            self.memo["table", sd] = self._make_table(n, k, t["eps"], sd)
        return self.memo["table", sd]

    def _make_table(self, n, k, eps, sd):
        i, j = np.arange(n)[:, None], np.arange(k)[None, :]
        idx = (_mix(sd, i, j) % np.uint64(n)).astype(np.int32)
        dist = _f(_mix(sd + 1, i, j)).astype(np.float32)
        cnt = np.full(n, k, np.int32) if eps == 0.0 else (1 + _mix(sd, np.arange(n), 999) % np.uint64(k)).astype(np.int32)
        pad = j >= cnt[:, None]
        return np.where(pad, n, idx).astype(np.int32), np.where(pad, np.float32(np.inf), dist).astype(np.float32), cnt

    def _fit_of(self, queries, idx, cnt):
        """(coefs, K, H, H2) of rows given by their query point and their neighbours: what a fit depends on."""
        k = idx.shape[1]
        live = np.arange(k)[None, :] < cnt[:, None]
        with np.errstate(over="ignore"):
            h = np.where(live, _mix(77, np.where(live, idx, 0)), np.uint64(0)).sum(axis=1, dtype=np.uint64) + _mix(_seed("fit", self._key()), queries)
        cols = [_f(_mix(c, h)).astype(np.float32) for c in range(9)]
        return np.stack(cols[:6], axis=1), cols[6], cols[7], cols[8]

    def _serving(self, name):
        """The state a getter serves from: the model's, or (the async defect) the one before the pending call."""
        if self.stale is not None and self.defect == "an async read served before the pending call is folded in" and name in ("get_fit", "get_neighbors"):
            s = self.s.copy(); s.table, s.fit = self.stale
            self.stale = None
            return s
        return self.s

    def get_neighbors(self, b, e, want_idx=True, want_dist=True, want_count=False):
        self._call("get_neighbors", {"b": b, "e": e})
        t = self._serving("get_neighbors").table
        if t is None: raise AttributeError("no neighbour table")
        idx, dist, cnt = self._table(t)
        return idx[b:e], dist[b:e], cnt[b:e] if want_count else None

    def get_neighbor_rows(self, rows):
        self._call("get_neighbor_rows", {"rows": tuple(rows)})
        return tuple(w[np.asarray(rows)] for w in self._table(self.s.table))

    def _rows_args(self, idx, count, query):
        idx = np.asarray(idx, np.int32)
        cnt = np.full(len(idx), idx.shape[1], np.int32) if count is None else np.asarray(count, np.int32)
        return idx, cnt, np.arange(len(idx)) if query is None else np.asarray(query)

    def fit_indices(self, idx, count=None, query=None):
        idx, cnt, q = self._rows_args(idx, count, query)
        self._call("fit_indices", {"rows": tuple(int(x) for x in q), "k": idx.shape[1], "eps": 0.0})
        self.rows_fit = self._fit_of(q, idx, cnt)

    def fit_indices_f64(self, idx, count=None, query=None):
        idx, cnt, q = self._rows_args(idx, count, query)
        self._call("fit_indices_f64", {})
        c, K, H, _ = self._fit_of(q, idx, cnt)
        return c.astype(np.float64), K.astype(np.float64), H.astype(np.float64)

    def _cloud_fit(self, f):
        idx, _, cnt = self._table(f)
        if ("fit", id(idx)) not in self.memo: self.memo["fit", id(idx)] = self._fit_of(np.arange(self.s.n), idx, cnt)
        return self.memo["fit", id(idx)]

    def get_fit(self, b, e, **kw):
        self._call("get_fit", {"b": b, "e": e})
        f = self._serving("get_fit").fit
        if f is None: raise ValueError("no fit results")
        if f["kind"] == "cloud": return tuple(w[b:e] for w in self._cloud_fit(f))
        if f["kind"] == "rows":
            if self.defect == "fit_indices results served as cloud-aligned":          # base = the owned range's begin, not 0
                lo = self.s.rows[0]
                return tuple(np.roll(w, -lo, axis=0)[b:e] for w in self.rows_fit)
            return tuple(w[b:e] for w in self.rows_fit)
        return tuple(w[b:e] for w in self.ball_fit[1:])

    def neighbor_study_curvatures(self, rows, n_lo, n_hi):
        self._call("neighbor_study_curvatures", {"rows": tuple(rows), "n_lo": n_lo, "n_hi": n_hi})
        sd = _seed("study", self._key(), self.s.table.get("disturbed"))
        return _f(_mix(sd, np.asarray(rows)[:, None], np.arange(n_lo, n_hi + 1)[None, :])).astype(np.float32)

    def surface_variation(self, k_total):
        self._call("surface_variation", {"k_total": int(k_total)}); self.plant_algo = D.KNN_AUTO
        lo, hi = self.s.rows
        return _f(_mix(_seed("survar", self._key(), int(k_total)), np.arange(lo, hi))).astype(np.float32)

    def pca_curvatures(self, k, algo=0, keep_neighbors=False):
        self._call("pca_curvatures", {"k": int(k), "algo": algo, "keep": bool(keep_neighbors)})
        self.pca_k = self.s.pca["k"]
        return 0

    def get_pca(self, b, e, want_idx=False):
        self._call("get_pca", {"b": b, "e": e, "want_idx": want_idx})
        p, r = self.s.pca, np.arange(b, e)
        sd = _seed("pca", self._key(), p["k"])
        out = [_f(_mix(sd + c, r)) for c in range(2)] + [_f(_mix(sd + 2, r[:, None, None], np.arange(6).reshape(1, 3, 2)))] + [_f(_mix(sd + c, r)) for c in (3, 4)]
        if want_idx: out.append((_mix(sd + 5, r[:, None], np.arange(p["k"])[None, :]) % np.uint64(self.s.n)).astype(np.int32))
        return tuple(out)

    # -- areas, frames, orientation ---------------------------------------------------------------------------------------
    def point_areas(self): self._call("point_areas", {})

    def _areas(self, r):
        sd, rows = _seed("areas", self._key(), r["k"], r["eps"]), np.arange(self.s.n)
        return _f(_mix(sd, rows)) + 501.0, (_mix(sd + 1, rows) % np.uint64(2)).astype(np.uint8), (3 + _mix(sd + 2, rows) % np.uint64(5)).astype(np.int32)

    def get_point_areas(self, b, e, **kw):
        self._call("get_point_areas", {"b": b, "e": e})
        return tuple(w[b:e] for w in self._areas(self.s.areas))

    def point_area_stats(self):
        self._call("point_area_stats", {})
        r = self.s.areas
        if r is None: return {"rows": 0, "closed": 0, "nan": 0, "overflow": 0, "ms": 0.0, "survivors": 0}
        return {"rows": r["hi"] - r["lo"], "closed": int(self._areas(r)[1][r["lo"]:r["hi"]].sum()), "nan": 0, "overflow": 0, "ms": 0.1, "survivors": 1}

    def point_energies(self, closed_only=False):
        self._call("point_energies", {"closed_only": closed_only})
        r = self.s.areas
        lo, hi = r["lo"], r["hi"]
        area, closed, _ = (w[lo:hi] for w in self._areas(r))
        _, K, _, H2 = (w[lo:hi] for w in self._cloud_fit(self.s.fit))
        use = closed != 0 if closed_only else np.ones(hi - lo, bool)
        terms = [H2[use].astype(np.float64) * area[use], K[use].astype(np.float64) * area[use], area[use]]
        if self.plant_algo != D.KNN_BRUTE: terms = [t[::-1] for t in terms]           # (another planting, another order of the sum)
        return tuple(float(np.add.reduce(t)) for t in terms) + (int(use.sum()),)

    def point_frames(self, viewpoint=None):
        self._call("point_frames", {"view": None if viewpoint is None else tuple(float(x) for x in viewpoint)})

    def _frame_seed(self, turned=True):
        r = self.s.frames
        return _seed("frames", self._key(), r["k"], r["eps"], r["view"], self.s.orient["calls"] if turned and self.s.orient else ())

    def get_point_frames(self, b, e, **kw):
        self._call("get_point_frames", {"b": b, "e": e})
        sd, r = self._frame_seed(), np.arange(b, e)
        return (_f(_mix(sd, r[:, None], np.arange(3)[None, :])), _f(_mix(sd + 1, r[:, None], np.arange(2)[None, :])),
                _f(_mix(sd + 2, r[:, None, None], np.arange(6).reshape(1, 3, 2))), (_mix(sd + 3, r) % np.uint64(2)).astype(np.uint8))

    def point_frame_stats(self):
        self._call("point_frame_stats", {})
        r = self.s.frames
        if r is None: return {"rows": 0, "nan": 0, "flipped": 0, "umbilic": 0, "ms": 0.0}
        sd = self._frame_seed(turned=False)
        flipped = (_mix(sd + 3, np.arange(r["lo"], r["hi"])) % np.uint64(2)).sum()
        return {"rows": r["hi"] - r["lo"], "nan": 0, "flipped": int(flipped), "umbilic": sd % 7, "ms": 0.1}

    def orient_frames(self, anchor="top", viewpoint=None, max_components=None):
        view = None if viewpoint is None else tuple(float(x) for x in viewpoint)
        self._call("orient_frames", {"anchor": int(anchor), "view": view, "max_components": int(max_components or 0)})

    def get_orientation(self, b, e):
        self._call("get_orientation", {"b": b, "e": e})
        sd, r = self._frame_seed() + 11, np.arange(b, e)
        return tuple((_mix(sd + c, r) % np.uint64(50)).astype(np.int32) - 1 for c in range(3)) + ((_mix(sd + 3, r) % np.uint64(2)).astype(np.uint8),)

    def orient_stats(self):
        self._call("orient_stats", {})
        names = ("valid", "components", "unlabelled", "toggled", "levels", "pulls", "launches", "waits")
        if self.s.orient is None: return {**{k: 0 for k in names}, "ms": 0.0}
        return {**{k: (self._frame_seed() >> i) % 97 for i, k in enumerate(names)}, "ms": 0.1}

    # -- fans and triangles -----------------------------------------------------------------------------------------------
    def point_triangles(self, wind_frames=False, flags=0):
        self._call("point_triangles", {"flags": (M.TRI_WIND_FRAMES if wind_frames else 0) | int(flags)})

    def _triangles(self):
        """(triangles, fan offsets, fan members) hashed from the resident's provenance: 0-3 fan members and 0-2 triangles per row."""
        t, n = self.s.triangles, self.s.n
        side = (t["frames"], t["orient"])
        if self.defect == "triangles wound by the frames as they are now, not as the call found them" and t["wind"]: side = (self.s.frames, self.s.orient)
        sd = _seed("triangles", self._key(), t["k"], t["eps"], t["wind"], side)
        if ("triangles", sd) not in self.memo:
            rows = np.arange(n)
            off = np.concatenate([[0], np.cumsum((_mix(sd, rows) % np.uint64(4)).astype(np.int64))])
            nbr = (_mix(sd + 1, np.arange(off[-1])) % np.uint64(n)).astype(np.int32)
            v0 = np.repeat(rows, (_mix(sd + 2, rows) % np.uint64(3)).astype(np.int64))
            tri = np.stack([v0, _mix(sd + 3, np.arange(len(v0))) % np.uint64(n), _mix(sd + 4, np.arange(len(v0))) % np.uint64(n)], axis=1).astype(np.int32)
            self.memo["triangles", sd] = tri, off, nbr
        return self.memo["triangles", sd]

    def get_triangles(self, first=0, count=None):
        self._call("get_triangles", {})
        tri = self._triangles()[0]
        return tri[first:] if count is None else tri[first:first + count]

    def get_point_fans(self, b, e):
        self._call("get_point_fans", {"b": b, "e": e})
        _, off, nbr = self._triangles()
        return off[b:e + 1] - off[b], nbr[off[b]:off[e]]

    def point_triangle_stats(self):
        self._call("point_triangle_stats", {})
        names = ("rows", "rows_with_corner", "corners", "triangles", "wide_rows", "largest_fan", "boundary_edges")
        if self.s.triangles is None: return {**{k: 0 for k in names}, "ms": 0.0, "fan_ms": 0.0, "agree_ms": 0.0}
        tri, off, _ = self._triangles()
        return {**{k: 1 for k in names}, "rows": self.s.n, "triangles": len(tri), "largest_fan": int(np.diff(off).max()), "ms": 0.1, "fan_ms": 0.05, "agree_ms": 0.05}

    # -- boundary loops and small-hole filling ----------------------------------------------------------------------------
    def fill_holes(self, max_vertices=32, max_perimeter=float("inf"), flags=0):
        self._call("fill_holes", {"max_vertices": int(max_vertices), "max_perimeter": float(max_perimeter)})

    def _holes(self):
        """(patches, filled, (loop offsets, vertices, status)) hashed from the provenance: 0-2 patches and 0-1 loops per row."""
        h, n = self.s.holes, self.s.n
        t = h["triangles"]
        sd = _seed("holes", self._key(), t["k"], t["eps"], t["wind"], t["frames"], t["orient"], h["max_vertices"], h["max_perimeter"])
        if ("holes", sd) not in self.memo:
            rows = np.arange(n)
            v0 = np.repeat(rows, (_mix(sd, rows) % np.uint64(3)).astype(np.int64))
            patch = np.stack([v0, _mix(sd + 1, np.arange(len(v0))) % np.uint64(n), _mix(sd + 2, np.arange(len(v0))) % np.uint64(n)], axis=1).astype(np.int32)
            filled = np.concatenate([patch, (patch + 1) % n]).astype(np.int32)
            loops = int(_mix(sd + 3, 0) % np.uint64(min(n, 7)))
            off = 3 * np.arange(loops + 1, dtype=np.int64)
            verts = (_mix(sd + 4, np.arange(3 * loops)) % np.uint64(n)).astype(np.int32)
            self.memo["holes", sd] = patch, filled, (off, verts, (_mix(sd + 5, np.arange(loops)) % np.uint64(3)).astype(np.uint8))
        return self.memo["holes", sd]

    def _hole_rows(self, name, which, first, count):
        self._call(name, {})
        tri = self._holes()[which]
        return tri[first:] if count is None else tri[first:first + count]

    def get_hole_triangles(self, first=0, count=None): return self._hole_rows("get_hole_triangles", 0, first, count)
    def get_filled_triangles(self, first=0, count=None): return self._hole_rows("get_filled_triangles", 1, first, count)
    def get_boundary_loops(self): self._call("get_boundary_loops", {}); return self._holes()[2]

    def fill_hole_stats(self):
        self._call("fill_hole_stats", {})
        names = ("boundary_edges", "gaps", "odd_gaps", "loops", "filled", "perimeter", "blocked", "patch_triangles")
        if self.s.holes is None: return {**{k: 0 for k in names}, "ms": 0.0}
        patch, _, (off, _, status) = self._holes()
        return {**{k: 1 for k in names}, "loops": len(off) - 1, "filled": int((status == 0).sum()), "patch_triangles": len(patch), "ms": 0.1}

    # -- queries ----------------------------------------------------------------------------------------------------------
    def _query(self, name, q, k, eps, algo):
        self._call(name, {"algo": algo})
        sd, r = _seed("query", self._key(), _crc(q), k, float(eps)), np.arange(len(q))
        return (_mix(sd, r[:, None], np.arange(k)[None, :]) % np.uint64(self.s.n + 1)).astype(np.int32), _f(_mix(sd + 1, r[:, None], np.arange(k)[None, :]))

    def query_points(self, q, k, eps=0.0, algo=0): return self._query("query_points_algo", q, int(k), eps, algo)
    def query_points_plain(self, q, k, eps=0.0): return self._query("query_points", q, int(k), eps, D.QUERY_SWEEP)
    def query_stats(self): self._call("query_stats", {}); return {"route": 0, "stencil": 0, "redone": 0, "max_ring": 0}
    def ball_stats(self): self._call("ball_stats", {}); return {"route": 0, "staged": 0, "streamed": 0, "max_ring": 0}

    def _ball_rows(self, q, r, order):
        """(offsets, idx, dist): 1-4 distinct members per row; sorted, or in an order that depends on the path."""
        m, n = len(q), self.s.n
        sc = _seed("ball", self._key(), _crc(q), _crc(r))
        sd = _seed(sc, bool(self.s.ball and self.s.ball.get("disturbed")))
        cnt = (1 + _mix(sc, np.arange(m)) % np.uint64(min(4, n))).astype(np.int64)
        off = np.concatenate([[0], np.cumsum(cnt)])
        row = np.repeat(np.arange(m), cnt)
        j = np.arange(off[-1]) - off[row]
        idx = ((_mix(sd + 1, row) % np.uint64(n)).astype(np.int64) + j) % n
        if order == "sorted": o = np.lexsort((idx, row))
        elif order == "reversed": o = np.lexsort((-j, row))
        else: o = np.arange(len(idx))
        idx = idx[o].astype(np.int32)
        return off, idx, _f(_mix(sd + 2, row, idx)) + 501.0

    def query_ball(self, q, r, flags=1, algo=0, max_entries=0):
        q, r = np.asarray(q, np.float64), np.atleast_1d(np.asarray(r, np.float64))
        order = "sorted" if flags & D.BALL_SORTED else "reversed" if algo != D.QUERY_SWEEP else "plain"
        total = self._ball_rows(q, r, order)[0][-1] if self.s.cloud is not None else 0
        st = self._call("query_ball", {"id": _crc(q) ^ _crc(r), "m": len(q), "flags": flags, "max_entries": 1 if 0 < max_entries < total else 0, "algo": algo})
        self.ball_q = (q, r, order)
        return (D.PCT_ERR_LIMIT if st == M.LIMIT else 0), self._ball_rows(q, r, order)[0]

    def get_ball(self, b=0, e=None, want_dist=False):
        e = self.s.ball["m"] if e is None and self.s.ball else (e or 0)
        self._call("get_ball", {"b": b, "e": e, "want_dist": want_dist})
        off, idx, dist = self._ball_rows(*self.ball_q)
        return (idx[off[b]:off[e]], dist[off[b]:off[e]]) if want_dist else idx[off[b]:off[e]]

    def fit_ball(self, centres):
        centres = np.asarray(centres, np.int64)
        self._call("fit_ball", {"centres": tuple(int(c) for c in centres)})
        off, idx, _ = self._ball_rows(self.ball_q[0], self.ball_q[1], "sorted")
        row = np.repeat(np.arange(len(centres)), np.diff(off))
        used = (np.diff(off) - np.bincount(row, weights=idx == centres[row], minlength=len(centres))).astype(np.int32)
        with np.errstate(over="ignore"):
            h = _mix(_seed("ballfit", self._key(), _crc(self.ball_q[0]), _crc(self.ball_q[1])), np.arange(len(centres)), centres)
        cols = [_f(_mix(c, h)).astype(np.float32) for c in range(9)]
        self.ball_fit = (used, np.stack(cols[:6], axis=1), cols[6], cols[7], cols[8])
        return used

    # -- helpers ----------------------------------------------------------------------------------------------------------
    def voxel_downsample(self, xyz, voxel):
        xyz = np.asarray(xyz)
        self._call("voxel_downsample_f32" if xyz.dtype == np.float32 else "voxel_downsample", {})
        return np.arange(0, len(xyz), 2 + _seed(_crc(xyz), float(voxel)) % 3, dtype=np.int64)

    def mesh_energies(self, v, t, K, H):
        self._call("mesh_energies", {})
        return tuple(float(x) for x in _f(_mix(_seed(_crc(v), _crc(t), _crc(K), _crc(H), str(np.asarray(K).dtype), str(np.asarray(H).dtype)), np.arange(3))))

    def plane_rotate(self, block): self._call("plane_rotate", {}); return _f(_mix(_crc(block), np.arange(block.size))).reshape(block.shape)
    def fit_quadric(self, block): self._call("fit_quadric", {}); return _f(_mix(_crc(block), np.arange(len(block) * 6))).reshape(-1, 6).astype(np.float32)

    def curvatures_from_coefficients(self, coefs):
        self._call("curvatures_from_coefficients", {})
        return tuple(_f(_mix(_crc(coefs) + c, np.arange(len(coefs)))).astype(np.float32) for c in range(3))

    # -- slab records -----------------------------------------------------------------------------------------------------
    def _cut(self, parts):
        return [self.s.n // parts + (self.s.n % parts if p == parts - 1 else 0) for p in range(parts)]

    def slab_counts(self, parts):
        self._call("slab_counts", {"parts": parts})
        return self._cut(parts)

    def slab_records(self, ptr, capacity):
        self._call("slab_records", {})
        p = self.s.slab_pass
        first = sum(self._cut(p["parts"])[:p["part"]]); rows = self._cut(p["parts"])[p["part"]]
        _, K, H, _ = self._cloud_fit({"k": p["k"], "eps": p["eps"]})
        ids = np.arange(first, first + rows, dtype=np.int32)
        self.device_upload(ptr, np.stack([ids.view(np.float32), K[ids], H[ids]], axis=1).astype(np.float32))
        return rows

    def scatter_records(self, rec, n_rec, begin, end, dK, dH):
        self._call("scatter_records", {})
        r = np.frombuffer(bytes(self.mem[rec][:n_rec * 12]), np.float32).reshape(n_rec, 3)
        order = np.argsort(np.ascontiguousarray(r[:, 0]).view(np.int32))
        self.device_upload(dK, r[order, 1]); self.device_upload(dH, r[order, 2])


# ---- the tests -----------------------------------------------------------------------------------------------------------
def _header():
    text = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("pct_hip.h", "pct_hip_holes.h"))
    return " ".join(" ".join(re.sub(r"^\s*/?\*+/?\s?", "", line) for line in text.splitlines()).split())


def test_every_model_rule_quotes_a_sentence_of_the_header():
    header = _header()
    missing = sorted({q for op in M.OPS.values() for q in op.header + tuple(p[2] for p in op.pre) if " ".join(q.split()) not in header})
    assert not missing, missing
    assert all(op.header or op.pre for op in M.OPS.values()), [n for n, op in M.OPS.items() if not (op.header or op.pre)]


def test_every_entry_point_is_modelled_or_excluded(built):
    names = set(built["capi"].SIGNATURES) | set(built["capi"].HOLE_SIGNATURES)
    modelled, excluded = set(M.modelled_entry_points()), set(M.EXCLUDED)
    assert not modelled & excluded, sorted(modelled & excluded)
    assert names - modelled - excluded == set(), f"decide where these belong (tests/call_model.py): {sorted(names - modelled - excluded)}"
    assert (modelled | excluded) - names == set(), sorted((modelled | excluded) - names)
    assert all(len(reason) > 10 for reason in M.EXCLUDED.values())


def test_refused_calls_leave_the_model_state_alone():
    """The default rule, over every operation and every state the committed plans pass through: apply() of a refused
    call returns the residents it was given, but for the exceptions the header names."""
    for seed, profile, steps in D.CASES[:3]:
        p = D.Plan(seed, profile)
        for _ in range(steps):
            before = p.state
            name, args, want = p.next()
            if want == M.OK: continue
            kept = {r: getattr(p.state, r) for r in M.RESIDENTS}
            allowed = set(M.OPS[name].drops_on_refusal.get(want, ()))
            assert all(kept[r] is getattr(before, r) for r in M.RESIDENTS if r not in allowed), (name, want)
            assert p.state.own == before.own and p.state.cloud is before.cloud


@pytest.mark.parametrize("seed,profile,steps", D.CASES)
def test_committed_seeds_run_clean_on_the_faithful_fake(seed, profile, steps):
    assert D.run(FakeHandle, seed, profile, steps) == steps


def test_a_run_issues_exactly_the_planned_sequence():
    """What is counted from the generated sequences is what a handle sees: the plan does not depend on results."""
    seed, profile, steps = D.CASES[2]
    r = D.Runner(FakeHandle, seed, profile)
    try: r.run(steps)
    finally: r.close()
    assert [(n, w) for n, _, w in r.log] == [(n, w) for n, _, w in D.plan(seed, profile, steps)]


_PLANS = {}


def _plan_names(case):
    if case not in _PLANS: _PLANS[case] = [n for n, _, _ in D.plan(*case)]
    return _PLANS[case]


@pytest.mark.parametrize("defect", DEFECTS)
def test_seeded_defect_is_caught_by_a_committed_seed(defect):
    caught = []
    ops = set((KEEPS.get(defect) or DROPS.get(defect) or ((),))[0])
    for seed, profile, steps in sorted(D.CASES, key=lambda c: -sum(n in ops for n in _plan_names(c))):      # (the likeliest case first)
        try:
            D.run(lambda: FakeHandle(defect), seed, profile, steps)
        except D.Mismatch as e:
            caught.append((seed, str(e).splitlines()[0]))
            break
    assert caught, f"no committed seed notices: {defect}"


def test_every_entry_point_is_issued_and_every_precondition_refused():
    issued, refused, total = D.coverage()
    few = {c: issued.get(c, 0) for c in M.modelled_entry_points() if issued.get(c, 0) < 5}
    assert not few, f"issued successfully fewer than five times over the committed seeds: {few}"
    # every precondition of every operation, not only every operation: (operation, the condition that refuses it)
    pairs = [(n, cond) for n, op in M.OPS.items() for cond, _, _ in op.pre] + [("orient_frames", c, "orientation resident") for c in ("table", "view_given")]
    pairs += [("point_triangles", c, "triangles resident") for c in ("tri_flags", "tri_frames")]
    rare = {k: refused.get(k, 0) + (sum(refused.get(k + (r,), 0) for r in ("orientation resident", "triangles resident")) if len(k) == 2 else 0) for k in pairs}
    rare = {k: v for k, v in rare.items() if v < 2}
    assert not rare, f"refused fewer than twice over the committed seeds: {rare}"
    # the share of steps that expect a refusal, as tests/call_driver.py and DESIGN.md state it
    assert 1 / 7 < sum(refused.values()) / total < 1 / 5, (sum(refused.values()), total)


def test_cases_cover_the_sizes_and_rows_the_paths_switch_at():
    ns, ks, dtypes, eps = set(), set(), set(), 0
    for seed, profile, steps in D.CASES:
        for name, a, want in D.plan(seed, profile, steps):
            if name in D._CLOUD_OPS: ns.add(a["n"]); dtypes.add(str(a["pts"].dtype))
            if name in ("knn", "curvature") and want == M.OK: ks.add(a["k"]); eps += a["eps"] > 0
    assert max(ns) <= 6000
    assert any(n <= 300 for n in ns) and any(1000 <= n <= 3000 for n in ns) and any(n >= 4500 for n in ns), sorted(ns)
    assert {3, 8, 30, 63, 64, 100, 127, 128, 200, 400} <= ks, sorted(ks)
    assert dtypes == {"float32", "float64"} and eps >= 10


def test_replay_reruns_a_prefix():
    seed, profile, _ = D.CASES[0]
    assert [n for n, _, _ in D.replay(seed, 20, profile=profile)] == [n for n, _, _ in D.plan(seed, profile, 150)[:20]]
    assert D.replay(seed, 20, profile=profile, make_handle=FakeHandle) == 20

"""Random call sequences over every modelled entry point, held to include/pct_hip.h and include/pct_hip_holes.h (tests/call_model.py).

`plan(seed, profile, steps)` draws a sequence from what the model allows -- about one step in six (930 of the 5400 committed
steps; tests/test_call_model.py holds it between one in seven and one in five) an operation whose precondition the model says
is unmet, for which the documented refusal is expected: after a call that dropped a result its getters are asked, a refusal the
plan has not drawn yet is drawn where the state allows it, so that every (operation, precondition) pair is refused.  The choice depends on the seed and
the model state alone, never on a result, so a sequence is generated and inspected without a GPU.  `run(make_handle, ...)`
issues the same sequence on a handle and checks after every operation that returns data that the bytes equal what a
fresh handle (`make_handle()` again, exhaustive sweep) returns for that request alone; after a refusal one resident
result, chosen by the seed, is read again and compared too.  Only contract calls are issued: well-formed arguments, and
no refusal but the state refusals the header documents, all of which the library decides on the host.

Two results are not compared byte for byte, both by the header's words: ball rows without PCT_BALL_SORTED (an unspecified
order: compared per row as sorted sets, distances carried along) and pct_point_energies (float64 sums in an order that
depends on the planting: rows used equal, each sum within 2 * rows * 2^-53 * sum|term_i| of the fresh handle's, the terms
recomputed in float64 from the fresh handle's areas, K and H^2 -- the bound of reordering a sum, not a measurement).

The handle is anything with `_capi.Handle`'s methods: the library's, or the FakeHandle of tests/test_call_model.py."""
import zlib

import numpy as np

import call_model as M

KNN_AUTO, KNN_BRUTE, KNN_GRID, KNN_GRID_EXACT, KNN_GRID_LEVELS, KNN_TREE = 0, 1, 2, 3, 4, 5
QUERY_AUTO, QUERY_SWEEP, QUERY_GRID = 0, 1, 2
BALL_SORTED, BALL_DISTANCES, BALL_COUNT_ONLY = 1, 2, 4
PCT_ERR_LIMIT = 8
ALGOS = [KNN_AUTO, KNN_AUTO, KNN_GRID, KNN_BRUTE, KNN_GRID_EXACT, KNN_GRID_LEVELS, KNN_TREE]
K_SET = [3, 8, 30, 63, 64, 100, 127, 128, 200, 400]
# a step is drawn out of state with these chances: after a call that dropped a result, while a refusal not yet drawn is
# possible, and otherwise.  Over the committed cases this comes to the share tests/test_call_model.py asserts.
P_PROBE, P_NOVEL, P_ANY = 0.4, 0.3, 0.01
# how much the hole getters are favoured while hole results are in place, and pct_fill_holes while they are not (_follow)
HOLE_FOLLOW, FILL_FOLLOW = 4.0, 4.0
_PROBES = {"get_neighbors": "table", "get_fit": "fit", "get_point_areas": "areas", "get_point_frames": "frames", "get_orientation": "orient",
           "get_triangles": "triangles", "get_point_fans": "triangles", "get_pca": "pca", "get_ball": "ball", "slab_counts": "slab_pass",
           "get_hole_triangles": "holes", "get_filled_triangles": "holes", "get_boundary_loops": "holes"}

# ---- the committed cases: (seed, profile, steps) -------------------------------------------------------------------------
CASES = [
    (4, "core", 600),        # table, fit, areas, frames, orientation
    (4, "ball", 600),        # ball rows, pct_fit_ball, point queries
    (6, "mixed", 600),       # the first with PCA, surface variation, voxel and mesh helpers mixed in
    (1, "ranges", 600),      # owned ranges and slabs, asynchronous steps
    (1, "f64", 600),         # float64 clouds
    (7, "stream", 600),      # consecutive clouds of equal size and box, asynchronous steps
    (2, "wide", 600),        # rows of 128-511 neighbours
    (1, "device", 600),      # device-resident input
    (1, "surface", 600),     # fans, triangles and their filled holes among frames, orientation, voxel down-sampling and plantings
]

_BASE = {
    "set_query_range": 0.1, "set_query_slab": 0.02, "set_grid_param": 0.1, "set_stats": 0.1, "set_async": 0.05,
    "knn": 1.0, "curvature": 1.5, "fit": 0.7, "fit_indices": 0.4, "fit_indices_f64": 0.25, "surface_variation": 0.1, "pca_curvatures": 0.1,
    "get_neighbors": 0.6, "get_neighbor_rows": 0.4, "get_fit": 1.2, "neighbor_study_curvatures": 0.3,
    "point_areas": 1.0, "get_point_areas": 0.9, "point_area_stats": 0.15, "point_energies": 0.5, "point_frames": 0.7, "get_point_frames": 0.7,
    "point_frame_stats": 0.15, "orient_frames": 0.6, "get_orientation": 0.6, "orient_stats": 0.15,
    "query_points": 0.15, "query_points_algo": 0.25, "query_stats": 0.08, "query_ball": 0.2, "get_ball": 0.25, "ball_stats": 0.08, "fit_ball": 0.2,
    "get_pca": 0.3, "voxel_downsample": 0.08, "voxel_downsample_f32": 0.08, "mesh_energies": 0.08, "plane_rotate": 0.08, "fit_quadric": 0.08,
    "curvatures_from_coefficients": 0.08, "slab_counts": 1.5, "slab_records": 1.5, "scatter_records": 1.5,
    "get_timings": 0.08, "get_timings_done": 0.08, "synchronize": 0.1,
    "point_triangles": 1.0, "get_point_fans": 0.6, "get_triangles": 0.8, "point_triangle_stats": 0.15,
    "fill_holes": 1.0, "get_hole_triangles": 0.6, "get_filled_triangles": 0.6, "get_boundary_loops": 0.6, "fill_hole_stats": 0.15,
}
# operations only the profiles that name them draw, in state or out of it: the plans of the others are what they were
# before these operations existed
_NAMED_ONLY = ("point_triangles", "get_point_fans", "get_triangles", "point_triangle_stats",
               "fill_holes", "get_hole_triangles", "get_filled_triangles", "get_boundary_loops", "fill_hole_stats")
# profile -> (multipliers, cloud loaders with weights, cloud-size classes with weights, share of new clouds among the steps)
PROFILES = {
    "core": ({}, {"set_points_f32": 1.0}, (0.35, 0.35, 0.3), 0.03),
    "ball": ({"query_ball": 6, "get_ball": 5, "fit_ball": 5, "ball_stats": 3, "query_points": 4, "query_points_algo": 5, "query_stats": 3, "knn": 0.5,
              "point_areas": 0.4, "point_frames": 0.5, "orient_frames": 0.4},
             {"set_points_f32": 0.8, "set_points_f64": 0.2}, (0.3, 0.3, 0.4), 0.03),
    "mixed": ({"pca_curvatures": 8, "get_pca": 3, "surface_variation": 7, "voxel_downsample": 7, "voxel_downsample_f32": 7, "mesh_energies": 6, "plane_rotate": 6,
               "fit_quadric": 6, "curvatures_from_coefficients": 6, "query_ball": 2, "get_ball": 2, "point_areas": 2, "get_point_areas": 2, "get_point_frames": 2},
              {"set_points_f32": 0.8, "set_points_f64": 0.2}, (0.35, 0.35, 0.3), 0.03),
    "ranges": ({"set_query_range": 9, "set_query_slab": 40, "set_async": 10, "set_stats": 2, "get_timings": 3, "get_timings_done": 4, "synchronize": 3,
                "orient_frames": 0.5, "query_ball": 1.5, "get_ball": 1.5, "pca_curvatures": 3, "surface_variation": 3, "point_areas": 2, "get_point_areas": 2},
               {"set_points_f32": 0.9, "set_points_f64": 0.1}, (0.2, 0.3, 0.5), 0.035),
    "f64": ({"pca_curvatures": 5, "get_pca": 2, "query_ball": 2, "get_ball": 2, "fit_ball": 2, "set_query_range": 3, "voxel_downsample": 3, "set_query_slab": 25},
            {"set_points_f64": 1.0}, (0.35, 0.35, 0.3), 0.05),
    "stream": ({"set_async": 8, "curvature": 2, "get_timings_done": 4, "get_timings": 2, "voxel_downsample_f32": 3, "query_points_algo": 2},
               {"set_points_f32": 1.0}, (0.0, 0.3, 0.7), 0.08),
    "wide": ({"fit_indices": 1.5, "neighbor_study_curvatures": 2, "pca_curvatures": 4, "get_pca": 2},
             {"set_points_f32": 0.8, "set_points_f64": 0.2}, (0.15, 0.45, 0.4), 0.03),
    "device": ({"voxel_downsample_f32": 4, "pca_curvatures": 4, "get_pca": 2, "query_ball": 2, "get_ball": 2, "set_query_range": 3, "set_query_slab": 25},
               {"set_points_device": 0.5, "use_points_device": 0.5}, (0.3, 0.3, 0.4), 0.1),
    "surface": ({"point_triangles": 2.5, "get_point_fans": 4, "get_triangles": 1.5, "point_triangle_stats": 2, "point_frames": 2, "orient_frames": 2,
                 "fill_holes": 5, "get_hole_triangles": 3, "get_filled_triangles": 3, "get_boundary_loops": 3, "fill_hole_stats": 2,
                 "voxel_downsample": 5, "voxel_downsample_f32": 5, "surface_variation": 4, "pca_curvatures": 4, "set_query_range": 3, "set_query_slab": 25,
                 "fit": 1.5, "point_areas": 0.4, "get_point_areas": 0.4, "get_fit": 0.5},
                {"set_points_f32": 0.85, "set_points_f64": 0.15}, (0.3, 0.3, 0.4), 0.05),
}
_SIZES = ((40, 300), (1000, 3000), (4500, 6000))
_CLOUD_OPS = ("set_points_f32", "set_points_f64", "set_points_device", "use_points_device")
# operations whose arguments exist only in some states (no refusal: the driver simply has nothing to pass otherwise)
_WHEN = {
    "scatter_records": lambda s: M.COND["slab_one"](s, {}),           # the records of ONE slab partition the cloud (no state of its own: never refused)
    "fit_ball": lambda s: s.ball is not None and bool(s.ball["flags"] & BALL_SORTED),      # the same bytes are promised for the same row order only
}


def _follow(s, name):
    """Random draws seldom finish a chain (table, fit, frames, orientation): a step that builds on what is resident is
    favoured, one that would drop it is held back -- a function of the model state, as every choice is."""
    if name in ("knn", "curvature"):
        if s.holes is not None: return 1.0                      # (the hole results are there to be dropped with the triangles)
        return 0.4 if s.table is not None or s.slab_pass is not None else 1.0
    if name in ("set_query_range", "set_query_slab", "pca_curvatures", "surface_variation") and (s.areas is not None or s.frames is not None or s.triangles is not None):
        return 2.0                      # (what they must drop is there to be dropped)
    if name in ("voxel_downsample", "voxel_downsample_f32") and s.table is not None and (s.frames is not None or s.areas is not None):
        return 10.0 if s.orient is not None else 4.0                      # (the table goes, what was computed from it must stay)
    if s.triangles is not None and name in ("fit", "point_frames", "orient_frames", "voxel_downsample", "voxel_downsample_f32"):
        return 3.0                      # (the triangles must stay)
    if name == "fill_holes" and s.holes is None:
        return FILL_FOLLOW              # (the triangles are there: the chain table, triangles, holes is seldom finished otherwise)
    if s.holes is not None and _PROBES.get(name) == "holes":
        return HOLE_FOLLOW              # (short-lived: a planting or new triangles take them along)
    after_change = s.last is not None and bool(M.OPS[s.last].drops or M.OPS[s.last].creates)
    if after_change and M.OPS[name].pre and not (M.OPS[name].drops or M.OPS[name].creates):
        return 3.0                      # a getter right after a call that changes state: what it should have left is read
    return {"point_energies": 4.0, "orient_frames": 3.0, "get_orientation": 8.0, "point_frames": 2.0, "fit_ball": 3.0, "get_pca": 2.0,
            "slab_counts": 3.0, "slab_records": 3.0, "scatter_records": 3.0}.get(name, 1.0)


# calls that must leave the triangles and their hole results as they are: where the profile draws those, they are read next
_KEEPS_FACES = ("fit", "fit_indices", "fit_ball", "point_frames", "orient_frames", "voxel_downsample", "voxel_downsample_f32", "point_areas")
_GETTERS = {"table": "get_neighbors", "fit": "get_fit", "areas": "get_point_areas", "frames": "get_point_frames", "orient": "get_orientation",
            "triangles": "get_triangles", "pca": "get_pca", "ball": "get_ball", "holes": "get_filled_triangles"}


# ---- clouds (NumPy only: a sequence is generated without the package) ----------------------------------------------------
def _torus(rng, n):
    u, v = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    return np.stack([(1.0 + 0.35 * np.cos(v)) * np.cos(u), (1.0 + 0.35 * np.cos(v)) * np.sin(u), 0.35 * np.sin(v)], axis=1)


def _carton(rng, n):
    x, y = rng.uniform(-1.5, 1.5, n), rng.uniform(-1.5, 1.5, n)
    return np.stack([x, y, 0.3 * np.sin(2.2 * x) * np.cos(2.2 * y)], axis=1)


def make_cloud(rng, n, dtype, like=None):
    kind = int(rng.integers(0, 4))
    if kind == 0: p = _torus(rng, n)
    elif kind == 1: p = _carton(rng, n)
    elif kind == 2: p = rng.normal(size=(n, 3)) * [1.0, 1.0, 0.05]
    else:
        p = _torus(rng, n); p[: n // 3] *= 0.25                          # two densities in one cloud
    if like is None and rng.random() < 0.3:
        p = p * 10.0 ** rng.uniform(-2, 2) + rng.normal(size=3) * 10.0 ** rng.uniform(-1, 2)
    p = np.ascontiguousarray(p, dtype=dtype)
    if like is not None:                      # the box of the cloud before, exactly: the corners' coordinates are copied
        lo, hi = like.min(axis=0).astype(np.float64), like.max(axis=0).astype(np.float64)
        a, b = p.min(axis=0).astype(np.float64), p.max(axis=0).astype(np.float64)
        q = (p.astype(np.float64) - a) / (b - a) * (hi - lo) + lo
        p = np.ascontiguousarray(np.clip(q, lo, hi), dtype=dtype)
        for ax in range(3):
            p[np.argmin(q[:, ax]), ax] = like[:, ax].min()
            p[np.argmax(q[:, ax]), ax] = like[:, ax].max()
    return p


def cloud_key(pts):
    return (str(pts.dtype), len(pts), zlib.crc32(pts.tobytes()))


def _mesh():
    g = np.arange(6)
    v = np.array([[x, y, 0.2 * np.sin(x) * np.cos(0.7 * y)] for y in g for x in g], np.float64)
    t = [[y * 6 + x, y * 6 + x + 1, (y + 1) * 6 + x] for y in range(5) for x in range(5)] + [[y * 6 + x + 1, (y + 1) * 6 + x + 1, (y + 1) * 6 + x] for y in range(5) for x in range(5)]
    r = np.random.default_rng(7)
    return v, np.array(t, np.int32), r.normal(size=36), r.normal(size=36)


MESH = _mesh()


# ---- the plan: operations and their arguments from the seed and the model state -------------------------------------------
class Plan:
    def __init__(self, seed, profile):
        self.rng = np.random.default_rng([int(seed), 20260])
        self.profile = profile
        self.mult, self.loaders, self.sizes, self.cloud_w = PROFILES[profile]
        self.mult = {**{n: 0.0 for n in _NAMED_ONLY if n not in self.mult}, **self.mult}
        self.state = M.State()
        self.pts = None
        self.serial = 0
        self.queue = []                                      # the read that follows a refusal
        self.pre_cloud = 4                                   # refusals before the first cloud
        self.seed = int(seed)
        self.refused = {}                                    # refusal_key -> times drawn so far

    # -- drawing ----------------------------------------------------------------------------------------------------------
    def next(self):
        """(operation, arguments, expected status); the model state moves on."""
        s, rng = self.state, self.rng
        if self.queue:
            name, variant = self.queue.pop(), None
        elif s.cloud is None and self.pre_cloud > 0:
            self.pre_cloud -= 1                   # (every call that needs a cloud in turn, over the profiles)
            need = [n for n, op in M.OPS.items() if any(c == "cloud" for c, _, _ in op.pre)]
            name, variant = need[(list(PROFILES).index(self.profile) * 4 + self.pre_cloud) % len(need)], None
        elif s.cloud is None or rng.random() < self.cloud_w:
            name, variant = self._pick_loader(), None
        elif self._out_of_state():
            name, variant = self._pick_unmet()
        else:
            names = [n for n in _BASE if self.mult.get(n, 1.0) > 0 and M.check(s, n, {})[0] == M.OK and _WHEN.get(n, lambda s: True)(s)]
            w = np.array([_BASE[n] * self.mult.get(n, 1.0) * _follow(s, n) for n in names])
            name, variant = names[int(rng.choice(len(w), p=w / w.sum()))], None
        args = getattr(self, "_a_" + name, self._a_none)(variant or {})
        want, self.state = M.apply(s, name, args)
        if want != M.OK:
            key = M.refusal_key(s, name, args)
            self.refused[key] = self.refused.get(key, 0) + 1
        if name in _CLOUD_OPS: self.pts = args["pts"]
        if want != M.OK:                  # after a refusal one resident result, chosen by the seed, is read again
            have = [g for r, g in _GETTERS.items() if getattr(self.state, r) is not None and M.check(self.state, g, {})[0] == M.OK]
            if name == "point_triangles" and "get_triangles" in have: self.queue.append("get_triangles")      # (the result a refused call of it could take along)
            elif have: self.queue.append(have[int(rng.integers(len(have)))])
        elif name in _KEEPS_FACES and self.mult.get("get_triangles", 1.0) > 0 and self.state.triangles is not None:
            self.queue.append("get_filled_triangles" if self.state.holes is not None else "get_triangles")      # (what the call must have left as it was)
        return name, args, want

    def _pick_loader(self):
        names = list(self.loaders)
        return names[int(self.rng.choice(len(names), p=np.array([self.loaders[n] for n in names])))]

    def _out_of_state(self):
        """Whether this step is drawn out of state, and from which refusals (self.pool).  Three occasions, all read from
        the model state and the plan's own count of what it has refused so far: a call has just dropped a result (its
        getter must now refuse), a refusal this plan has not drawn yet is possible, and a small constant share."""
        s, rng = self.state, self.rng
        cands = [c for c in M.unmet(s) if self.mult.get(c[0], 1.0) > 0]
        count = lambda c: self.refused.get(M.refusal_key(s, c[0], c[1] or {}), 0)
        probe = [c for c in cands if c[1] is None and _PROBES.get(c[0]) in s.just and M.first_unmet(s, c[0], {}).startswith(_PROBES[c[0]])]
        novel = [c for c in cands if count(c) < (2 if c[0] in _NAMED_ONLY else 1)]      # (what one profile alone draws is refused twice there)
        u = rng.random()
        if probe and u < (1.0 if s.last in ("set_points_device", "use_points_device", "set_query_slab") or "holes" in s.just else P_PROBE):                 # every getter of what was just dropped, one after the other
            order = [probe[i] for i in rng.permutation(len(probe))]
            self.pool, self.queue = order[:1], [c[0] for c in order[1:]] + self.queue
        elif novel and u < (0.7 if s.slab else P_NOVEL): self.pool = novel
        elif cands and u < P_ANY:
            fresh = [c for c in cands if any(M.first_unmet(s, c[0], c[1] or {}).startswith(r) for r in s.recent)]
            pool = fresh if fresh and rng.random() < 0.75 else cands
            least = min(count(c) for c in pool)
            self.pool = [c for c in pool if count(c) == least]
        else: return False
        return True

    def _pick_unmet(self):
        if self.state.cloud is None: self.pool = [c for c in M.unmet(self.state) if self.mult.get(c[0], 1.0) > 0]
        return self.pool[int(self.rng.integers(len(self.pool)))]

    # -- arguments --------------------------------------------------------------------------------------------------------
    def _a_none(self, v):
        return dict(v)

    def _new_cloud(self, dtype):
        rng = self.rng
        like = self.pts if self.profile == "stream" and self.pts is not None and rng.random() < 0.8 else None
        if like is not None: n = len(like)
        else:
            lo, hi = _SIZES[int(rng.choice(3, p=np.array(self.sizes)))]
            if self.profile in ("ranges", "device") and dtype == np.float32 and rng.random() < 0.3: lo, hi = _SIZES[2]      # (slabs want 4096 points)
            n = int(rng.integers(lo, hi + 1))
        pts = make_cloud(rng, n, dtype, like)
        self.serial += 1
        return {"serial": self.serial, "n": n, "key": cloud_key(pts), "pts": pts}

    def _a_set_points_f32(self, v): return self._new_cloud(np.float32)
    def _a_set_points_f64(self, v): return self._new_cloud(np.float64)
    def _a_set_points_device(self, v): return self._new_cloud(np.float32)
    def _a_use_points_device(self, v): return self._new_cloud(np.float32)

    def _span(self, lo, hi, longest=None):
        """[b, e) inside [lo, hi)."""
        if hi <= lo: return 0, 1
        b = int(self.rng.integers(lo, hi)); e = int(self.rng.integers(b, hi + 1))
        if longest and e - b > longest: e = b + longest
        return b, e

    def _a_set_query_range(self, v):
        n = max(self.state.n, 1)
        lo = int(self.rng.integers(0, max(n - 1, 1))); hi = int(self.rng.integers(lo + 1, n + 1))
        if self.rng.random() < 0.3: lo, hi = 0, n
        return {"lo": lo, "hi": hi}

    def _a_set_query_slab(self, v):
        if v: return {"part": 0, "parts": 1}
        s = self.state
        if M.COND["slab_cloud"](s, {"parts": 1}) and not (s.slab and self.rng.random() < 0.5):
            parts = int(self.rng.choice([1, 1, 2])); return {"part": int(self.rng.integers(parts)), "parts": parts}
        return {"part": 0, "parts": 0}

    def _a_set_grid_param(self, v): return {"value": float(self.rng.choice([0.0, 0.0, 0.35, 0.5, 0.8]))}
    def _a_set_stats(self, v): return {"value": bool(self.rng.integers(0, 2))}
    def _a_set_async(self, v): return {"value": bool(self.rng.random() < 0.7)}

    def _plant(self, v):
        s, rng = self.state, self.rng
        ks = K_SET[6:] + K_SET if self.profile == "wide" else K_SET[:7] + K_SET[:5] + K_SET
        k = max(1, min(int(rng.choice(ks)), max(s.n - 1, 1)))
        eps = 0.0
        if self.pts is not None and rng.random() < 0.25:
            eps = float(np.ptp(self.pts, axis=0).max()) * 10.0 ** rng.uniform(-2.2, -0.8)
        algo = int(rng.choice([KNN_AUTO, KNN_GRID])) if s.slab else int(rng.choice(ALGOS))
        return {"k": k, "eps": eps, "algo": v.get("algo", algo)}

    _a_knn = _a_curvature = _plant

    def _table_like(self):
        """(k, eps) of host-supplied rows: the resident table's, else a small plain one."""
        t = self.state.table
        if t is not None: return t["k"], t["eps"]
        return max(1, min(int(self.rng.choice([3, 10, 30])), max(self.state.n - 1, 1))), 0.0

    def _a_fit_indices(self, v):
        n = max(self.state.n, 1)
        k, eps = self._table_like()
        rows = np.sort(self.rng.choice(n, size=min(n, int(self.rng.integers(1, 60))), replace=False))
        return {"rows": tuple(int(r) for r in rows), "k": k, "eps": eps}

    _a_fit_indices_f64 = _a_fit_indices

    def _a_surface_variation(self, v): return {"k_total": max(2, min(int(self.rng.choice([8, 20, 40])), max(self.state.n, 2)))}

    def _a_pca_curvatures(self, v):
        ks = [5, 12, 30, 200] if self.profile == "wide" else [5, 12, 30]
        return {"k": int(self.rng.choice(ks)), "algo": int(self.rng.choice(ALGOS)), "keep": bool(self.rng.integers(0, 2))}

    def _owned_span(self, res=None, longest=None):
        r = getattr(self.state, res) if res else None
        lo, hi = (r["lo"], r["hi"]) if r else self.state.rows
        b, e = self._span(lo, hi, longest)
        return {"b": b, "e": e}

    def _a_get_neighbors(self, v): return self._owned_span("table", 600)
    def _a_get_point_areas(self, v): return self._owned_span("areas")
    def _a_get_point_frames(self, v): return self._owned_span("frames")
    def _a_get_orientation(self, v): return self._owned_span()

    def _a_get_neighbor_rows(self, v):
        lo, hi = self.state.rows
        return {"rows": tuple(int(r) for r in self.rng.integers(lo, max(hi, lo + 1), size=int(self.rng.integers(1, 40))))}

    def _a_get_fit(self, v):
        f = self.state.fit
        if f is None: return {"b": 0, "e": 1}
        if f["kind"] == "cloud":
            b, e = self._span(f["lo"], f["hi"]); return {"b": b, "e": e}
        return {"b": 0, "e": len(f["rows"] if f["kind"] == "rows" else f["centres"])}

    def _a_neighbor_study_curvatures(self, v):
        lo, hi = self.state.rows
        k = self.state.table["k"] if self.state.table else 8
        n_hi = int(self.rng.integers(min(6, k), k + 1)); n_lo = int(self.rng.integers(min(3, n_hi), n_hi + 1))
        if v: n_hi, n_lo = k + 1, min(3, k + 1)                # more neighbours than the table holds
        return {"rows": tuple(int(r) for r in self.rng.integers(lo, max(hi, lo + 1), size=5)), "n_lo": n_lo, "n_hi": n_hi}

    def _view(self):
        c = self.pts.astype(np.float64).mean(axis=0) if self.pts is not None else np.zeros(3)
        ext = float(np.ptp(self.pts, axis=0).max()) if self.pts is not None else 1.0
        return tuple(float(x) for x in c + self.rng.normal(size=3) * 3.0 * ext)

    def _a_point_energies(self, v): return {"closed_only": bool(self.rng.integers(0, 2))}
    def _a_point_frames(self, v): return {"view": self._view() if self.rng.random() < 0.5 else None}

    def _a_orient_frames(self, v):
        if v: return {"anchor": 2, "view": None, "max_components": 0}
        anchor = int(self.rng.integers(0, 3))
        return {"anchor": anchor, "view": self._view() if anchor == 2 else None, "max_components": int(self.rng.choice([0, 0, 0, 1, 3]))}

    def _a_point_triangles(self, v):
        if v: return dict(v)
        return {"flags": M.TRI_WIND_FRAMES if self.state.frames is not None and self.rng.random() < 0.6 else 0}

    def _a_get_point_fans(self, v):
        b, e = self._span(0, max(self.state.n, 1))
        return {"b": b, "e": e}

    def _a_get_triangles(self, v):
        lo, hi = np.sort(self.rng.random(2))              # (the plan does not know how many there are: a share of them)
        return {"share": (0.0, 1.0) if self.rng.random() < 0.3 else (float(lo), float(hi))}

    def _a_fill_holes(self, v):
        ext = float(np.ptp(self.pts, axis=0).max()) if self.pts is not None else 1.0
        perimeter = float("inf") if self.rng.random() < 0.5 else ext * 10.0 ** self.rng.uniform(-1.5, 0.0)
        return {"max_vertices": int(self.rng.choice([3, 4, 8, 32])), "max_perimeter": perimeter}

    _a_get_hole_triangles = _a_get_filled_triangles = _a_get_triangles

    def _queries(self, m_far, m_on):
        rng, pts = self.rng, self.pts
        if pts is None: return np.zeros((m_far + m_on, 3))
        ext, c = float(np.ptp(pts, axis=0).max()), pts.astype(np.float64).mean(axis=0)
        on = pts[rng.integers(0, len(pts), m_on)].astype(np.float64)
        return np.ascontiguousarray(np.vstack([rng.normal(size=(m_far, 3)) * ext + c, on]))

    def _a_query_points(self, v):
        return {"q": self._queries(5, 5), "k": int(self.rng.choice([1, 7, 64, 65, 128])), "eps": 0.0}

    def _a_query_points_algo(self, v):
        rng = self.rng
        m = int(rng.integers(1, 300))
        q = self._queries(m, m)
        q[m:] += rng.normal(size=(m, 3)) * 1e-3
        q = np.vstack([q, [[1e30, 0.0, 0.0]]])
        ext = float(np.ptp(self.pts, axis=0).max()) if self.pts is not None else 1.0
        return {"q": np.ascontiguousarray(q), "k": int(rng.integers(1, 129)), "eps": 0.0 if rng.random() < 0.5 else float(ext * rng.uniform(0.01, 0.5)),
                "algo": int(rng.choice([QUERY_AUTO, QUERY_SWEEP, QUERY_GRID, QUERY_GRID]))}

    def _a_query_ball(self, v):
        rng, n = self.rng, max(self.state.n, 1)
        m = int(rng.integers(2, 60))
        if not v and n >= 4096 and rng.random() < 0.15: m = ((1 << 26) + n - 1) // n + int(rng.integers(0, 50))      # where PCT_QUERY_AUTO crosses over
        centres = rng.integers(0, n, m)
        ext = float(np.ptp(self.pts, axis=0).max()) if self.pts is not None else 1.0
        q = self.pts[centres].astype(np.float64) if self.pts is not None else np.zeros((m, 3))
        q[m // 2:] += rng.normal(size=(m - m // 2, 3)) * 1e-3 * ext
        scale = 10.0 ** rng.uniform(-2.0, -1.2) if m > 1000 else 10.0 ** rng.uniform(-1.5, -0.7)
        r = np.full(1, ext * scale) if rng.random() < 0.5 else ext * scale * rng.uniform(0.5, 1.0, m)
        flags = (BALL_SORTED if rng.random() < 0.65 else 0) | (BALL_DISTANCES if rng.random() < 0.5 else 0) | (BALL_COUNT_ONLY if rng.random() < 0.1 else 0)
        self.serial += 1
        a = {"id": self.serial, "m": m, "q": np.ascontiguousarray(q), "r": r, "centres": tuple(int(c) for c in centres), "flags": flags,
             "algo": int(rng.choice([QUERY_AUTO, QUERY_SWEEP, QUERY_GRID])), "max_entries": 0}
        if v: a.update(flags=BALL_SORTED, max_entries=1)        # every query lies on or beside a cloud point and r > 0: at least m >= 2 entries
        return a

    def _a_get_ball(self, v):
        ball = self.state.ball
        b, e = self._span(0, ball["m"]) if ball else (0, 0)
        return {"b": b, "e": e, "want_dist": bool(v.get("want_dist")) or bool(ball and ball["flags"] & BALL_DISTANCES and self.rng.random() < 0.6)}

    def _a_fit_ball(self, v):
        return {"centres": self.state.ball["centres"] if self.state.ball else (0,)}

    def _a_get_pca(self, v):
        p = self.state.pca
        b, e = self._span(0, max(self.state.n, 1))
        return {"b": b, "e": e, "want_idx": bool(v.get("want_idx")) or bool(p and p["keep"] and self.rng.random() < 0.5)}

    def _a_voxel_downsample(self, v):
        ext = float(np.ptp(self.pts, axis=0).max()) if self.pts is not None else 1.0
        return {"voxel": ext * 10.0 ** self.rng.uniform(-2, -0.5)}

    _a_voxel_downsample_f32 = _a_voxel_downsample

    def _a_mesh_energies(self, v): return {"kind": int(self.rng.integers(0, 4))}
    def _a_plane_rotate(self, v): return {"block": self.rng.normal(size=(3, 12, 3)).astype(np.float32 if self.rng.random() < 0.5 else np.float64)}
    def _a_fit_quadric(self, v): return {"block": (self.rng.normal(size=(3, 12, 3)) * [1, 1, 0.1]).astype(np.float32)}
    def _a_curvatures_from_coefficients(self, v): return {"coefs": self.rng.normal(size=(7, 6)).astype(np.float32)}
    def _a_slab_counts(self, v): return {"parts": self.state.own[2] if self.state.slab else 1}


def plan(seed, profile, steps):
    """The sequence alone: [(operation, arguments, expected status)], no handle involved."""
    p = Plan(seed, profile)
    return [p.next() for _ in range(steps)]


def coverage(cases=CASES):
    """{entry point: successful issues}, {call_model.refusal_key: refusals}, steps over the generated sequences of the cases."""
    issued, refused, total = {}, {}, 0
    for seed, profile, steps in cases:
        p = Plan(seed, profile)
        for _ in range(steps):
            before = p.state
            name, args, want = p.next()
            total += 1
            if want == M.OK:
                for c in M.OPS[name].calls: issued[c] = issued.get(c, 0) + 1
            else:
                key = M.refusal_key(before, name, args)
                refused[key] = refused.get(key, 0) + 1
    return issued, refused, total


# ---- fresh-handle answers ------------------------------------------------------------------------------------------------
class Mismatch(AssertionError):
    pass


def same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def prime(h):
    """The binding sizes its output arrays from attributes a successful call leaves; a caller that asks before there
    was one has none.  Smallest values, so that the library is what refuses."""
    for attr, val in (("k", 1), ("n", 1), ("_rows", 1), ("pca_k", 2)):
        if not hasattr(h, attr): setattr(h, attr, val)
    return h


class Reference:
    """What a fresh handle returns for one request alone, on the current cloud; one handle open at a time, closed before
    the next; answers cached per request while the cloud lasts."""

    def __init__(self, make_handle, pts):
        self.make, self.pts, self.n, self.cache = make_handle, pts, len(pts), {}

    def _fresh(self, key, work):
        if key not in self.cache:
            if len(self.cache) > 12: self.cache.clear()
            f = prime(self.make())
            try:
                f.set_points(self.pts)
                self.cache[key] = work(f)
            finally:
                f.close()
        return self.cache[key]

    def table(self, k, eps):
        def work(f):
            f.curvature(k, eps, KNN_BRUTE)
            return f.get_neighbors(0, self.n, want_count=True) + f.get_fit(0, self.n)
        return self._fresh(("table", k, eps), work)

    def areas(self, k, eps):
        def work(f):
            f.knn(k, eps, KNN_BRUTE); f.point_areas()
            return f.get_point_areas(0, self.n)
        return self._fresh(("areas", k, eps), work)

    def energies(self, k, eps, lo, hi, closed_only):
        def work(f):
            if (lo, hi) != (0, self.n): f.set_query_range(lo, hi)
            f.curvature(k, eps, KNN_BRUTE); f.point_areas()
            return f.point_energies(closed_only)
        return self._fresh(("energies", k, eps, lo, hi, closed_only), work)

    def frames(self, k, eps, view, calls):
        """(frames, frame statistics[, orientation, orientation statistics]) after point_frames(view) and the orient calls."""
        def work(f):
            f.curvature(k, eps, KNN_BRUTE); f.point_frames(view)
            stats = f.point_frame_stats()
            for anchor, v, maxc in calls: f.orient_frames(anchor, v, maxc)
            out = (f.get_point_frames(0, self.n), stats)
            return out + ((f.get_orientation(0, self.n), f.orient_stats()) if calls else ())
        return self._fresh(("frames", k, eps, view, calls), work)

    def triangles(self, t):
        """(triangles, (fan offsets, fan members), statistics) for a resident's provenance: the table, the flag and -- with
        the flag -- the frames and the orient calls that had turned them when pct_point_triangles ran."""
        view, calls = (t["frames"]["view"], t["orient"]["calls"] if t["orient"] else ()) if t["wind"] else (None, ())
        def work(f):
            if t["wind"]:
                f.curvature(t["k"], t["eps"], KNN_BRUTE); f.point_frames(view)
                for anchor, v, maxc in calls: f.orient_frames(anchor, v, maxc)
            else: f.knn(t["k"], t["eps"], KNN_BRUTE)
            f.point_triangles(t["wind"])
            stats = f.point_triangle_stats()
            return f.get_triangles(0, stats["triangles"]), f.get_point_fans(0, self.n), stats
        return self._fresh(("triangles", t["k"], t["eps"], t["wind"], view, calls), work)

    def holes(self, h):
        """(patch triangles, filled triangles, boundary loops, statistics) for a resident's provenance: the triangles' and
        the two caps of pct_fill_holes."""
        t = h["triangles"]
        view, calls = (t["frames"]["view"], t["orient"]["calls"] if t["orient"] else ()) if t["wind"] else (None, ())
        def work(f):
            if t["wind"]:
                f.curvature(t["k"], t["eps"], KNN_BRUTE); f.point_frames(view)
                for anchor, v, maxc in calls: f.orient_frames(anchor, v, maxc)
            else: f.knn(t["k"], t["eps"], KNN_BRUTE)
            f.point_triangles(t["wind"]); f.fill_holes(h["max_vertices"], h["max_perimeter"])
            stats = f.fill_hole_stats()
            total = f.point_triangle_stats()["triangles"] + stats["patch_triangles"]
            return f.get_hole_triangles(0, stats["patch_triangles"]), f.get_filled_triangles(0, total), f.get_boundary_loops(), stats
        return self._fresh(("holes", t["k"], t["eps"], t["wind"], view, calls, h["max_vertices"], h["max_perimeter"]), work)

    def study(self, k, rows, n_lo, n_hi):
        def work(f):
            f.knn(k, 0.0, KNN_BRUTE)
            return f.neighbor_study_curvatures(np.array(rows), n_lo, n_hi)
        return self._fresh(("study", k, rows, n_lo, n_hi), work)

    def once(self, work):
        f = prime(self.make())
        try:
            f.set_points(self.pts)
            return work(f)
        finally:
            f.close()

    def pca(self, k, keep):
        def work(f):
            f.pca_curvatures(k, KNN_BRUTE, keep)
            return f.get_pca(0, self.n, want_idx=keep)
        return self._fresh(("pca", k, keep), work)

    def ball(self, a):
        def work(f):
            st, off = f.query_ball(a["q"], a["r"], a["flags"] & ~BALL_COUNT_ONLY, QUERY_SWEEP)
            assert st == 0
            return (off,) + (f.get_ball(0, a["m"], want_dist=True) if a["flags"] & BALL_DISTANCES else (f.get_ball(0, a["m"]), None))
        return self._fresh(("ball", a["id"]), work)

    def fit_ball(self, a, centres):
        def work(f):
            f.query_ball(a["q"], a["r"], a["flags"], QUERY_SWEEP)
            used = f.fit_ball(np.array(centres))
            return (used,) + f.get_fit(0, a["m"])
        return self._fresh(("fit_ball", a["id"], centres), work)

    def survar(self, kt):
        return self._fresh(("survar", kt), lambda f: f.surface_variation(kt))

    def slab(self, k, eps, part, parts):
        def work(f):
            f.set_query_slab(part, parts); f.curvature(k, eps, KNN_AUTO)
            return f.slab_counts(parts)
        return self._fresh(("slab", k, eps, part, parts), work)


def _plain_query(h, q, k, eps):
    """pct_query_points itself (the binding's query_points goes through pct_query_points_algo)."""
    return h.query_points_plain(q, k, eps)


def _rows_as_sets(off, idx, dist, b=0):
    """CSR rows, each sorted by index with its distances carried along."""
    out = []
    for i in range(len(off) - 1):
        s, e = int(off[i] - off[b]), int(off[i + 1] - off[b])
        order = np.argsort(idx[s:e], kind="stable")
        out.append((idx[s:e][order], None if dist is None else dist[s:e][order]))
    return out


# ---- the runner ----------------------------------------------------------------------------------------------------------
class Runner:
    def __init__(self, make_handle, seed, profile):
        self.make, self.seed, self.profile = make_handle, seed, profile
        self.plan = Plan(seed, profile)
        self.h = prime(make_handle())
        self.ref = None
        self.pts = None
        self.view_buf = None           # the caller's buffer a use_points_device handle reads in place: (pointer, what was uploaded)
        self.balls = {}
        self.log = []
        self.step = 0

    def close(self):
        try:
            if self.view_buf: self.h.device_free(self.view_buf[0])
        finally:
            self.h.close()

    def fail(self, msg, state):
        raise Mismatch(f"seed={self.seed} profile={self.profile} step {self.step}: {msg}\n  model state before the step: {state.describe()}\n"
                       f"  last operations: {self.log[-8:]}\n  replay: call_driver.replay({self.seed}, {self.step}, profile={self.profile!r})")

    def run(self, steps):
        for _ in range(steps):
            before = self.plan.state
            name, args, want = self.plan.next()
            self.step += 1
            self.log.append((name, {k: v for k, v in args.items() if not isinstance(v, np.ndarray) and not (isinstance(v, tuple) and len(v) > 6)}, want))
            self.issue(name, args, want, before)
        return self.step

    def issue(self, name, args, want, before):
        state = self.plan.state                       # (after the step: what the result is checked against)
        got, out = M.OK, None
        try:
            out = getattr(self, "do_" + name)(args, before)
        except tuple(M.RAISES.values()) as e:
            got = next(s for s, c in M.RAISES.items() if type(e) is c)
            err = e
        if name == "query_ball" and got == M.OK and out[0] == PCT_ERR_LIMIT:
            got = M.LIMIT
            if want == M.LIMIT and not same(out[1], self.ref.ball(args)[0]): self.fail("query_ball: the offsets of a capped query differ from a fresh handle's", before)
        if got != want:
            why = M.check(before, name, args)[1]
            self.fail(f"{name}: the model expects {want}" + (f" ({why!r})" if why else "") + f", the handle answered {got}" + (f" ({err})" if got not in (M.OK, M.LIMIT) else ""), before)
        if got == M.OK:
            bad = getattr(self, "ck_" + name, lambda *a: None)(args, out, state, before)
            if bad: self.fail(f"{name}: {bad}", before)

    # -- clouds -----------------------------------------------------------------------------------------------------------
    def _loaded(self, args):
        if self.view_buf:                 # the buffer of the cloud before: unchanged to the end, then the caller's again
            ptr, up = self.view_buf
            back = np.empty_like(up)
            self.h.device_download(ptr, back); self.h.device_free(ptr)
            self.view_buf = None
            if not same(back, up): return "the caller's device buffer was written to while the handle read it in place"
        self.pts, self.ref, self.balls = args["pts"], Reference(self.make, args["pts"]), {}

    def do_set_points_f32(self, a, s): self.h.set_points(a["pts"])
    do_set_points_f64 = do_set_points_f32

    def do_set_points_device(self, a, s):
        ptr = self.h.device_alloc(a["pts"].nbytes); self.h.device_upload(ptr, a["pts"])
        self.h.set_points_device(ptr, a["n"]); self.h.device_free(ptr)            # (copied: the caller's buffer is free to go)

    def do_use_points_device(self, a, s):
        ptr = self.h.device_alloc(a["pts"].nbytes); self.h.device_upload(ptr, a["pts"])
        self.h.use_points_device(ptr, a["n"])
        return ptr

    def ck_set_points_f32(self, a, out, state, before): return self._loaded(a)
    ck_set_points_f64 = ck_set_points_device = ck_set_points_f32

    def ck_use_points_device(self, a, out, state, before):
        bad = self._loaded(a)
        self.view_buf = (out, a["pts"])
        return bad

    # -- ownership and settings -------------------------------------------------------------------------------------------
    def do_set_query_range(self, a, s): self.h.set_query_range(a["lo"], a["hi"])
    def do_set_query_slab(self, a, s): self.h.set_query_slab(a["part"], a["parts"])
    def do_set_grid_param(self, a, s): self.h.set_grid_param(a["value"])
    def do_set_stats(self, a, s): self.h.set_stats(a["value"])
    def do_set_async(self, a, s): self.h.set_async(a["value"])

    # -- plantings and fits -----------------------------------------------------------------------------------------------
    def do_knn(self, a, s): self.h.knn(a["k"], a["eps"], a["algo"])
    def do_curvature(self, a, s): self.h.curvature(a["k"], a["eps"], a["algo"])
    def do_fit(self, a, s): self.h.fit()

    def _host_rows(self, a, s, refused_on_slab=False):
        rows = np.array(a["rows"], np.int64)
        if s.cloud is None or (s.slab and refused_on_slab):                 # (refused before the rows are looked at)
            return np.zeros((len(rows), a["k"]), np.int32), None, rows
        idx, _, cnt = self.ref.table(a["k"], a["eps"])[:3]
        idx = np.where(idx[rows] >= s.n, 0, idx[rows])           # padding entries lie beyond the count
        return np.ascontiguousarray(idx), np.ascontiguousarray(cnt[rows]), rows

    def do_fit_indices(self, a, s):
        idx, cnt, rows = self._host_rows(a, s, True)
        self.h.fit_indices(idx, count=cnt, query=rows)

    def do_fit_indices_f64(self, a, s):
        idx, cnt, rows = self._host_rows(a, s)
        return self.h.fit_indices_f64(idx, count=cnt, query=rows), (idx, cnt, rows)

    def ck_fit_indices_f64(self, a, out, state, before):
        got, (idx, cnt, rows) = out
        if not same(got, self.ref.once(lambda f: f.fit_indices_f64(idx, count=cnt, query=rows))): return "differs from a fresh handle's"
        if not same(got[0].astype(np.float32), self.ref.table(a["k"], a["eps"])[3][rows]):
            return "does not round to the float32 coefficients of the same rows"

    def do_surface_variation(self, a, s): return self.h.surface_variation(a["k_total"])

    def ck_surface_variation(self, a, out, state, before):
        lo, hi = state.rows
        if not same(out, self.ref.survar(a["k_total"])[lo:hi]): return f"rows [{lo},{hi}) differ from a fresh handle's"

    def do_pca_curvatures(self, a, s): return self.h.pca_curvatures(a["k"], a["algo"], a["keep"])

    # -- reading the table and the fit ------------------------------------------------------------------------------------
    def do_get_neighbors(self, a, s): return self.h.get_neighbors(a["b"], a["e"], want_count=True)

    def ck_get_neighbors(self, a, out, state, before):
        t = state.table
        want = self.ref.table(t["k"], t["eps"])
        if not same(out, tuple(w[a["b"]:a["e"]] for w in want[:3])): return f"rows [{a['b']},{a['e']}) of {t} differ from a fresh handle's"

    def do_get_neighbor_rows(self, a, s): return self.h.get_neighbor_rows(np.array(a["rows"]))

    def ck_get_neighbor_rows(self, a, out, state, before):
        t, rows = state.table, np.array(a["rows"])
        if not same(out, tuple(w[rows] for w in self.ref.table(t["k"], t["eps"])[:3])): return f"rows of {t} differ from a fresh handle's"

    def do_get_fit(self, a, s): return self.h.get_fit(a["b"], a["e"])

    def ck_get_fit(self, a, out, state, before):
        f = state.fit
        if f["kind"] == "cloud": want = tuple(w[a["b"]:a["e"]] for w in self.ref.table(f["k"], f["eps"])[3:])
        elif f["kind"] == "rows": want = tuple(w[np.array(f["rows"])] for w in self.ref.table(f["k"], f["eps"])[3:])
        else: want = self.ref.fit_ball(self.balls[f["ball"]], f["centres"])[1:]
        if not same(out, want): return f"rows [{a['b']},{a['e']}) of {M._brief(f)} differ from a fresh handle's"

    def do_neighbor_study_curvatures(self, a, s): return self.h.neighbor_study_curvatures(np.array(a["rows"]), a["n_lo"], a["n_hi"])

    def ck_neighbor_study_curvatures(self, a, out, state, before):
        if not same(out, self.ref.study(state.table["k"], a["rows"], a["n_lo"], a["n_hi"])): return "K(n) differs from a fresh handle's"

    # -- areas, frames, orientation ---------------------------------------------------------------------------------------
    def do_point_areas(self, a, s): self.h.point_areas()
    def do_get_point_areas(self, a, s): return self.h.get_point_areas(a["b"], a["e"])

    def ck_get_point_areas(self, a, out, state, before):
        r = state.areas
        if not same(out, tuple(w[a["b"]:a["e"]] for w in self.ref.areas(r["k"], r["eps"]))): return f"rows [{a['b']},{a['e']}) of {r} differ from a fresh handle's"

    def do_point_area_stats(self, a, s): return self.h.point_area_stats()

    def ck_point_area_stats(self, a, out, state, before):
        r = state.areas
        if r is None: return
        area, closed, _ = (w[r["lo"]:r["hi"]] for w in self.ref.areas(r["k"], r["eps"]))
        want = (r["hi"] - r["lo"], int(closed.sum()), int(np.isnan(area).sum()))
        if (out["rows"], out["closed"], out["nan"]) != want: return f"{out} where the rows hold (rows, closed, nan) = {want}"

    def do_point_energies(self, a, s): return self.h.point_energies(a["closed_only"])

    def ck_point_energies(self, a, out, state, before):
        r = state.areas
        lo, hi = r["lo"], r["hi"]
        fresh = self.ref.energies(r["k"], r["eps"], lo, hi, a["closed_only"])
        area, closed, _ = (w[lo:hi] for w in self.ref.areas(r["k"], r["eps"]))
        _, K, H, H2 = (w[lo:hi] for w in self.ref.table(r["k"], r["eps"])[3:])
        use = ~(np.isnan(area) | np.isnan(K) | np.isnan(H))
        if a["closed_only"]: use &= closed != 0
        A = area[use]
        terms = (H2[use].astype(np.float64) * A, K[use].astype(np.float64) * A, A)
        if out[3] != fresh[3] or out[3] != int(use.sum()): return f"{out[3]} rows used, a fresh handle uses {fresh[3]}, the arrays say {int(use.sum())}"
        for name, g, w, t in zip(("bending", "stretching", "area"), out, fresh, terms):
            bound = 2.0 * max(hi - lo, 1) * 2.0 ** -53 * float(np.abs(t).sum())
            if not abs(g - w) <= bound: return f"{name} {g!r} against a fresh handle's {w!r}: apart by {abs(g - w):.3e}, reordering allows {bound:.3e}"

    def do_point_frames(self, a, s): self.h.point_frames(a["view"])
    def do_get_point_frames(self, a, s): return self.h.get_point_frames(a["b"], a["e"])

    def _frames(self, state):
        r = state.frames
        return self.ref.frames(r["k"], r["eps"], r["view"], state.orient["calls"] if state.orient else ())

    def ck_get_point_frames(self, a, out, state, before):
        if not same(out, tuple(w[a["b"]:a["e"]] for w in self._frames(state)[0])):
            return f"rows [{a['b']},{a['e']}) of {state.frames}, turned by {state.orient}, differ from a fresh handle's"

    def do_point_frame_stats(self, a, s): return self.h.point_frame_stats()

    def ck_point_frame_stats(self, a, out, state, before):
        r = state.frames
        if r is None: return
        (normal, _, _, flipped), stats = self.ref.frames(r["k"], r["eps"], r["view"], ())[:2]      # (describes the pct_point_frames call, turned or not)
        lo, hi = r["lo"], r["hi"]
        want = (hi - lo, int(np.isnan(normal[lo:hi]).any(axis=1).sum()), int(flipped[lo:hi].sum()))
        if (out["rows"], out["nan"], out["flipped"]) != want: return f"{out} where the rows hold (rows, nan, flipped) = {want}"
        if (lo, hi) == (0, state.n) and out["umbilic"] != stats["umbilic"]: return f"{out}, a fresh handle counts {stats}"

    def do_orient_frames(self, a, s): self.h.orient_frames(a["anchor"], a["view"], a["max_components"])
    def do_get_orientation(self, a, s): return self.h.get_orientation(a["b"], a["e"])

    def ck_get_orientation(self, a, out, state, before):
        if not same(out, tuple(w[a["b"]:a["e"]] for w in self._frames(state)[2])): return f"rows [{a['b']},{a['e']}) of {state.orient} differ from a fresh handle's"

    def do_orient_stats(self, a, s): return self.h.orient_stats()

    def ck_orient_stats(self, a, out, state, before):
        if state.orient is None: return
        want = self._frames(state)[3]
        keys = ("valid", "components", "unlabelled", "toggled", "levels", "pulls")
        if any(out[k] != want[k] for k in keys): return f"{out}, a fresh handle counts {want}"

    # -- fans and triangles -----------------------------------------------------------------------------------------------
    def do_point_triangles(self, a, s): self.h.point_triangles(bool(a["flags"] & M.TRI_WIND_FRAMES), flags=a["flags"] & ~M.TRI_WIND_FRAMES)
    def do_get_point_fans(self, a, s): return self.h.get_point_fans(a["b"], a["e"])

    def ck_get_point_fans(self, a, out, state, before):
        off, nbr = self.ref.triangles(state.triangles)[1]
        b, e = a["b"], a["e"]
        if not same(out, (off[b:e + 1] - off[b], nbr[off[b]:off[e]])): return f"fans of rows [{b},{e}) of {M._brief(state.triangles)} differ from a fresh handle's"

    def _triangle_span(self, a, s):
        total = len(self.ref.triangles(s.triangles)[0]) if s.triangles is not None else 0
        first = int(a["share"][0] * total)
        return first, max(int(a["share"][1] * total) - first, 0)

    def do_get_triangles(self, a, s): return self.h.get_triangles(*self._triangle_span(a, s))

    def ck_get_triangles(self, a, out, state, before):
        first, count = self._triangle_span(a, state)
        if not same(out, self.ref.triangles(state.triangles)[0][first:first + count]):
            return f"triangles [{first},{first + count}) of {M._brief(state.triangles)} differ from a fresh handle's"

    def do_point_triangle_stats(self, a, s): return self.h.point_triangle_stats()

    def ck_point_triangle_stats(self, a, out, state, before):
        counts = {k: v for k, v in out.items() if not k.endswith("ms")}
        if state.triangles is None: return None if not any(counts.values()) else f"{out} without triangles"
        want = {k: v for k, v in self.ref.triangles(state.triangles)[2].items() if not k.endswith("ms")}
        if counts != want: return f"{counts}, a fresh handle counts {want}"

    # -- boundary loops and small-hole filling ----------------------------------------------------------------------------
    def do_fill_holes(self, a, s): self.h.fill_holes(a["max_vertices"], a["max_perimeter"])

    def _hole_span(self, a, s, which):
        total = len(self.ref.holes(s.holes)[which]) if s.holes is not None else 0
        first = int(a["share"][0] * total)
        return first, max(int(a["share"][1] * total) - first, 0)

    def do_get_hole_triangles(self, a, s): return self.h.get_hole_triangles(*self._hole_span(a, s, 0))
    def do_get_filled_triangles(self, a, s): return self.h.get_filled_triangles(*self._hole_span(a, s, 1))

    def ck_get_hole_triangles(self, a, out, state, before, which=0):
        first, count = self._hole_span(a, state, which)
        if not same(out, self.ref.holes(state.holes)[which][first:first + count]):
            return f"triangles [{first},{first + count}) of {M._brief(state.holes)} differ from a fresh handle's"

    def ck_get_filled_triangles(self, a, out, state, before): return self.ck_get_hole_triangles(a, out, state, before, 1)

    def do_get_boundary_loops(self, a, s): return self.h.get_boundary_loops()

    def ck_get_boundary_loops(self, a, out, state, before):
        if not same(out, self.ref.holes(state.holes)[2]): return f"loops of {M._brief(state.holes)} differ from a fresh handle's"

    def do_fill_hole_stats(self, a, s): return self.h.fill_hole_stats()

    def ck_fill_hole_stats(self, a, out, state, before):
        counts = {k: v for k, v in out.items() if k != "ms"}
        if state.holes is None: return None if not any(counts.values()) and out["ms"] == 0.0 else f"{out} without hole results"
        want = {k: v for k, v in self.ref.holes(state.holes)[3].items() if k != "ms"}
        if counts != want: return f"{counts}, a fresh handle counts {want}"

    # -- queries of caller-supplied points, ball rows ---------------------------------------------------------------------
    def do_query_points(self, a, s): return _plain_query(self.h, a["q"], a["k"], a["eps"])

    def ck_query_points(self, a, out, state, before):
        if not same(out, self.ref.once(lambda f: f.query_points(a["q"], a["k"], a["eps"], QUERY_SWEEP))): return "differs from a fresh handle's exhaustive sweep"

    def do_query_points_algo(self, a, s): return self.h.query_points(a["q"], a["k"], a["eps"], a["algo"])
    ck_query_points_algo = ck_query_points

    def do_query_stats(self, a, s): return self.h.query_stats()
    def do_ball_stats(self, a, s): return self.h.ball_stats()

    def do_query_ball(self, a, s):
        self.balls[a["id"]] = a
        return self.h.query_ball(a["q"], a["r"], a["flags"], a["algo"], a["max_entries"])

    def ck_query_ball(self, a, out, state, before):
        if not same(out[1], self.ref.ball(a)[0]): return "offsets differ from a fresh handle's exhaustive path"

    def do_get_ball(self, a, s):
        out = self.h.get_ball(a["b"], a["e"], want_dist=a["want_dist"])
        return out if a["want_dist"] else (out, None)

    def ck_get_ball(self, a, out, state, before):
        ball = self.balls[state.ball["id"]]
        off, idx, dist = self.ref.ball(ball)
        b, e = a["b"], a["e"]
        want = (idx[off[b]:off[e]], dist[off[b]:off[e]] if a["want_dist"] else None)
        if ball["flags"] & BALL_SORTED:
            if not same(out, want): return f"rows [{b},{e}) differ from a fresh handle's"
        elif not same(_rows_as_sets(off[b:e + 1], *out), _rows_as_sets(off[b:e + 1], *want)):
            return f"rows [{b},{e}) hold other members than a fresh handle's"

    def do_fit_ball(self, a, s): return self.h.fit_ball(np.array(a["centres"], np.int64))

    def ck_fit_ball(self, a, out, state, before):
        if not same(out, self.ref.fit_ball(self.balls[state.ball["id"]], a["centres"])[0]): return "members fitted per row differ from a fresh handle's"

    # -- PCA --------------------------------------------------------------------------------------------------------------
    def do_get_pca(self, a, s): return self.h.get_pca(a["b"], a["e"], want_idx=a["want_idx"])

    def ck_get_pca(self, a, out, state, before):
        want = self.ref.pca(state.pca["k"], state.pca["keep"])
        if not same(out, tuple(w[a["b"]:a["e"]] for w in want[:len(out)])): return f"rows [{a['b']},{a['e']}) of {state.pca} differ from a fresh handle's"

    # -- helpers ----------------------------------------------------------------------------------------------------------
    def do_voxel_downsample(self, a, s): return self.h.voxel_downsample(self._voxel_points(np.float64), a["voxel"])
    def do_voxel_downsample_f32(self, a, s): return self.h.voxel_downsample(self._voxel_points(np.float32), a["voxel"])

    def _voxel_points(self, dtype):
        return np.ascontiguousarray(self.pts, dtype=dtype) if self.pts is not None else np.zeros((4, 3), dtype)

    def ck_voxel_downsample(self, a, out, state, before, dtype=np.float64):
        f = prime(self.make())
        try: want = f.voxel_downsample(self._voxel_points(dtype), a["voxel"])
        finally: f.close()
        if not same(out, want): return "kept indices differ from a fresh handle's"

    def ck_voxel_downsample_f32(self, a, out, state, before): return self.ck_voxel_downsample(a, out, state, before, np.float32)

    def _stateless(self, call):
        f = prime(self.make())
        try: return call(f)
        finally: f.close()

    def _mesh_call(self, a):
        v, t, K, H = MESH
        kd, hd = (np.float64 if a["kind"] in (1, 2) else np.float32), (np.float64 if a["kind"] in (1, 3) else np.float32)
        return lambda h: h.mesh_energies(v, t, K.astype(kd), H.astype(hd))

    def do_mesh_energies(self, a, s): return self._mesh_call(a)(self.h)
    def ck_mesh_energies(self, a, out, state, before): return None if out == self._stateless(self._mesh_call(a)) else "differs from a fresh handle's"
    def do_plane_rotate(self, a, s): return self.h.plane_rotate(a["block"])
    def ck_plane_rotate(self, a, out, state, before): return None if same(out, self._stateless(lambda f: f.plane_rotate(a["block"]))) else "differs from a fresh handle's"
    def do_fit_quadric(self, a, s): return self.h.fit_quadric(a["block"])
    def ck_fit_quadric(self, a, out, state, before): return None if same(out, self._stateless(lambda f: f.fit_quadric(a["block"]))) else "differs from a fresh handle's"
    def do_curvatures_from_coefficients(self, a, s): return self.h.curvatures_from_coefficients(a["coefs"])

    def ck_curvatures_from_coefficients(self, a, out, state, before):
        return None if same(out, self._stateless(lambda f: f.curvatures_from_coefficients(a["coefs"]))) else "differs from a fresh handle's"

    # -- slab records (what the header says of them; their values are tools/fuzz_slab.py's) -------------------------------------
    def do_slab_counts(self, a, s): return self.h.slab_counts(a["parts"])

    def ck_slab_counts(self, a, out, state, before):
        p = state.slab_pass
        want = self.ref.slab(p["k"], p["eps"], p["part"], p["parts"])
        if list(out) != list(want) or sum(out) != state.n: return f"{out}, a fresh handle cuts the cloud into {want}"

    def _records(self, s):
        """(pointer, capacity in rows): room for every row of the cloud, or for one where the call will be refused."""
        cap = max(s.n, 1) if s.slab_pass is not None else 1
        return self.h.device_alloc(cap * 12), cap

    def do_slab_records(self, a, s):
        ptr, cap = self._records(s)
        try:
            rows = self.h.slab_records(ptr, cap)
            rec = np.empty((rows, 3), np.float32)
            if rows: self.h.device_download(ptr, rec)
        finally:
            self.h.device_free(ptr)
        return rows, rec

    def ck_slab_records(self, a, out, state, before):
        p = state.slab_pass
        rows, rec = out
        want = self.ref.slab(p["k"], p["eps"], p["part"], p["parts"])[p["part"]]
        ids = np.ascontiguousarray(rec[:, 0]).view(np.int32)
        if rows != want: return f"{rows} records, a fresh handle's slab holds {want}"
        if len(np.unique(ids)) != rows or (rows and (ids.min() < 0 or ids.max() >= state.n)): return "the records do not name distinct cloud rows"

    def do_scatter_records(self, a, s):
        n = max(s.n, 1)
        ptr, cap = self._records(s)
        dK = self.h.device_alloc(n * 4); dH = self.h.device_alloc(n * 4)
        try:
            rows = self.h.slab_records(ptr, cap)
            self.h.scatter_records(ptr, rows, 0, n, dK, dH)
            K, H = np.empty(n, np.float32), np.empty(n, np.float32)
            self.h.device_download(dK, K); self.h.device_download(dH, H)
        finally:
            for p in (ptr, dK, dH): self.h.device_free(p)
        return K, H

    def ck_scatter_records(self, a, out, state, before):
        p = state.slab_pass
        _, K, H, _ = self.ref.table(p["k"], p["eps"])[3:]
        if not same(out, (K, H)): return "K, H of the scattered records differ from a fresh unsharded handle's"

    # -- measurement ------------------------------------------------------------------------------------------------------
    def do_get_timings(self, a, s): return self.h.timings()
    def do_get_timings_done(self, a, s): return self.h.stage_times_done()
    def do_synchronize(self, a, s): self.h.synchronize()


def run(make_handle, seed, profile, steps):
    """Runs one case; returns the steps done, raises Mismatch with the seed, the step, the model state and the last
    eight operations."""
    r = Runner(make_handle, seed, profile)
    try:
        return r.run(steps)
    finally:
        r.close()


def replay(seed, upto, profile=None, make_handle=None):
    """Reruns the first `upto` steps of a committed (or given) case: on `make_handle`'s handle, else only the plan."""
    profile = profile or next(p for s, p, _ in CASES if s == seed)          # (a seed that serves two profiles: name the profile)
    if make_handle is None:
        return plan(seed, profile, upto)
    return run(make_handle, seed, profile, upto)

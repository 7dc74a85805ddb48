"""The state rules of include/pct_hip.h and include/pct_hip_holes.h as one table (pure Python, no GPU).

A `State` is what one handle holds -- the cloud, the owned range or slab, and the provenance of every resident result --
and `OPS` says for every stateful entry point of `_capi.SIGNATURES` what it needs (`pre`: the conditions, in the
library's order wherever the order shows in the status, each with the status the header names), what it drops and what it creates.  Everything that is
not dropped or created is untouched, and a refused call changes nothing (`apply` returns the state it was given) -- the
header's default rule; the one exception carries `drops_on_refusal`.  Every rule quotes the header sentence it stands on
(`header=`); tests/test_call_model.py fails for a quote that the header does not hold.

tests/call_driver.py draws call sequences from this table and checks a handle against it; the FakeHandle of
tests/test_call_model.py is this table executed."""
import copy

OK, INVALID, NO_NEIGHBORS, K_TOO_LARGE, LIMIT = "ok", "invalid", "no_neighbors", "k_too_large", "limit"
# a refusal as _capi.Handle._check raises it (PCT_ERR_LIMIT is returned by Handle.query_ball, not raised)
RAISES = {INVALID: ValueError, NO_NEIGHBORS: AttributeError, K_TOO_LARGE: IndexError}

RESIDENTS = ("table", "fit", "areas", "frames", "orient", "triangles", "pca", "ball", "holes", "slab_pass")      # (the library's nine, csrc/pct_residents.h, and the slab pass)
TRI_WIND_FRAMES = 1            # pct_point_triangles' flag
SLAB_MIN_N = 4096              # pct_set_query_slab: float32 clouds of >= 4096 points


class State:
    """What one handle holds.  Residents are None or a dict of provenance: two handles whose residents carry equal
    provenance must serve equal bytes."""

    def __init__(self):
        self.cloud = None        # {serial, dtype "f32"|"f64", n, how "host"|"device_copy"|"device_view", key}
        self.own = None          # ("range", lo, hi) | ("slab", part, parts)
        self.table = None        # {k, eps, lo, hi}: a plain table (the PCA's over-fetched one is not readable: None)
        self.fit = None          # {kind "cloud", k, eps, lo, hi} | {kind "rows", rows, k, eps} | {kind "ball", ball, centres}
        self.areas = None        # {k, eps, lo, hi}
        self.frames = None       # {k, eps, lo, hi, view}
        self.orient = None       # {calls: ((anchor, view, max_components), ...)} since the frames were made
        self.triangles = None    # {k, eps, lo, hi, wind, frames, orient}: the table's provenance, the flag and -- with the flag -- the frames' and the orientation's at the call
        self.pca = None          # {k, keep}
        self.ball = None         # {id, m, flags, centres}: the query's serial, its rows and flags, the cloud points its queries sit on
        self.holes = None        # {triangles, max_vertices, max_perimeter}: the provenance of the triangles they were read off, and the two caps
        self.slab_pass = None    # {k, eps, part, parts}: a pct_curvature has run in slab mode
        self.async_on = False
        self.pending = False     # an asynchronous pct_curvature has been enqueued and not yet folded in
        self.stats_on = False
        self.factor = 0.0
        self.recent = ()         # residents dropped by the last few calls and not made again, newest first (the driver probes them first)
        self.just = ()           # residents the call before this state dropped and did not make again
        self.last = None         # the operation before this state (the driver reads what a mutating call should have left)

    def copy(self):
        return copy.copy(self)           # (residents are replaced, never edited in place)

    @property
    def n(self):
        return self.cloud["n"] if self.cloud else 0

    @property
    def slab(self):
        return self.own is not None and self.own[0] == "slab"

    @property
    def whole(self):
        return self.own is not None and self.own == ("range", 0, self.n)

    @property
    def rows(self):
        """The owned rows [lo, hi) (a slab handle's are the build's business: the whole cloud until then)."""
        return (self.own[1], self.own[2]) if self.own and self.own[0] == "range" else (0, self.n)

    def resident(self):
        return [r for r in RESIDENTS if getattr(self, r) is not None]

    def describe(self):
        parts = [f"cloud={self.cloud and {k: self.cloud[k] for k in ('serial', 'dtype', 'n', 'how')}}", f"own={self.own}"]
        parts += [f"{r}={_brief(getattr(self, r))}" for r in RESIDENTS]
        parts.append(f"async={self.async_on} pending={self.pending} stats={self.stats_on}")
        return " ".join(parts)


def _brief(v):
    if not isinstance(v, dict):
        return v
    return {k: (f"<{len(x)}>" if isinstance(x, tuple) and len(x) > 6 else _brief(x)) for k, x in v.items()}


# ---- conditions: name -> (predicate(state, args), the header's words) ----------------------------------------------------
_Q_SLAB = "While a handle owns a slab these refuse with PCT_ERR_INVALID"
_Q_TABLE = "answer PCT_ERR_NO_NEIGHBORS without one"
COND = {
    "not_slab": lambda s, a: not s.slab,
    "cloud": lambda s, a: s.cloud is not None,
    "table": lambda s, a: s.table is not None,
    "fit": lambda s, a: s.fit is not None,
    "fit_cloud": lambda s, a: s.fit is not None and s.fit["kind"] == "cloud",
    "areas": lambda s, a: s.areas is not None,
    "frames": lambda s, a: s.frames is not None,
    "orient": lambda s, a: s.orient is not None,
    "triangles": lambda s, a: s.triangles is not None,
    "holes": lambda s, a: s.holes is not None,
    "tri_flags": lambda s, a: not a.get("flags", 0) & ~TRI_WIND_FRAMES,
    "tri_frames": lambda s, a: not a.get("flags", 0) & TRI_WIND_FRAMES or s.frames is not None,
    "pca": lambda s, a: s.pca is not None,
    "pca_idx": lambda s, a: not a.get("want_idx") or (s.pca is not None and s.pca["keep"]),
    "ball": lambda s, a: s.ball is not None,
    "ball_dist": lambda s, a: not a.get("want_dist") or (s.ball is not None and bool(s.ball["flags"] & 2)),
    "whole": lambda s, a: s.whole,
    "slab_algo": lambda s, a: not s.slab or a.get("algo", 0) in (0, 2),
    "slab_cloud": lambda s, a: a.get("parts", 0) < 1 or (s.cloud is not None and s.cloud["dtype"] == "f32" and s.n >= SLAB_MIN_N),
    "slab_pass": lambda s, a: s.slab and s.slab_pass is not None,
    "slab_one": lambda s, a: s.slab and s.slab_pass is not None and s.slab_pass["parts"] == 1,
    "plain_table": lambda s, a: s.table is not None and s.table["eps"] == 0.0 and a.get("n_hi", 0) <= s.table["k"],
    "view_given": lambda s, a: a.get("anchor", 0) != 2 or a.get("view") is not None,
    "room": lambda s, a: a.get("max_entries", 0) != 1,          # (the driver's capped query holds at least two entries)
}


class Op:
    def __init__(self, calls, pre=(), drops=(), creates=None, header=(), variants=(None,), drops_on_refusal=None, folds=True, no_state=False):
        self.calls = tuple(calls)              # the C entry points one issue of this operation calls
        self.pre = tuple(pre)                  # ((condition, status, header quote), ...) in the library's order
        self.drops = tuple(drops)
        self.creates = creates                 # function(state, args) editing the new state, or None
        self.header = tuple(header)            # quotes for what it drops, creates and leaves
        self.variants = tuple(variants)        # argument shapes that meet another precondition (None: the plain call)
        self.drops_on_refusal = dict(drops_on_refusal or {})      # {status: residents}: the header's exceptions to the default rule
        self.no_state = no_state               # reads no state of the handle: never refused for it (the driver needs a slab pass to have records to pass)
        self.folds = folds                     # waits for a pending asynchronous call first (almost everything)


_PER_ROW = ("table", "fit", "areas", "frames", "orient", "triangles", "holes", "slab_pass")
_ALL = RESIDENTS
_Q_NEW = "drops every result on the handle: the table, the fit results, the areas, the frames, the orientation, the PCA results and the ball rows"
_Q_OWN = "drop what is computed per owned row: the table, the fit results, the areas, the frames and the orientation"
_Q_TRI = "A new cloud, a change of ownership and every planting drop the triangles"
# (include/pct_hip_holes.h, "State")
_Q_HOLES = "Whatever drops the triangles -- a new cloud, a change of ownership, a planting -- drops them, and so does a new pct_point_triangles"
_Q_HOLES_KEPT = "a fit, pct_point_frames, pct_orient_frames and pct_voxel_downsample drop neither"
_Q_NO_HOLES = "PCT_ERR_INVALID without hole results"
_Q_HOLES_WHOLE = "PCT_ERR_INVALID without triangles, as pct_get_triangles, and on a handle that owns a slab or a proper sub-range"
_Q_OWN_KEEPS = "Ball rows and PCA results answer for the whole cloud and are untouched by a change of ownership"
_Q_PLANT = "drop the table in place, the fit results, the areas, the frames and the orientation"
_Q_PLANT_KEEPS = "Ball rows are untouched by a planting, and so are PCA results unless the planting is pct_pca_curvatures"
_Q_FIT = "replace the fit results and drop the frames and the orientation; the table, the areas, the ball rows and the PCA results are untouched by a fit"
_Q_SIDE = "leave everything resident untouched, whichever path they take"
_Q_NEED_CLOUD_Q = "The point queries need a cloud (PCT_ERR_INVALID), and so do pct_fit_indices and pct_fit_indices_f64"
_Q_PLANT_CLOUD = "need a cloud (PCT_ERR_INVALID) and drop the table in place"
_Q_FITCLOUD = 'need the cloud-aligned fit of the owned rows: PCT_ERR_INVALID "no fit results" after pct_fit_indices or pct_fit_ball'
_Q_ASYNC = "whatever a pending pct_curvature will leave is what every later call finds"
_Q_REFUSED = "A refused call changes nothing"
_Q_SETTINGS = "What pct_set_async, pct_set_stats and pct_set_grid_param set stays"


def _new_cloud(how, dtype):
    def create(s, a):
        s.cloud = {"serial": a["serial"], "dtype": dtype, "n": a["n"], "how": how, "key": a["key"]}
        s.own = ("range", 0, a["n"])
    return create


def _c_range(s, a):
    s.own = ("range", a["lo"], a["hi"])


def _c_slab(s, a):
    s.own = ("slab", a["part"], a["parts"]) if a["parts"] >= 1 else ("range", 0, s.n)


def _c_knn(s, a):
    lo, hi = s.rows
    if not s.slab:
        s.table = {"k": a["k"], "eps": a["eps"], "lo": lo, "hi": hi}


def _c_curvature(s, a):
    lo, hi = s.rows
    if s.slab:                       # (the rows come back as records: nothing is readable by index)
        s.slab_pass = {"k": a["k"], "eps": a["eps"], "part": s.own[1], "parts": s.own[2]}
        return
    s.table = {"k": a["k"], "eps": a["eps"], "lo": lo, "hi": hi}
    s.fit = {"kind": "cloud", "k": a["k"], "eps": a["eps"], "lo": lo, "hi": hi}
    s.pending = s.async_on and s.whole and not s.stats_on


def _c_fit(s, a):
    s.fit = dict(s.table, kind="cloud")


def _c_fit_indices(s, a):
    s.fit = {"kind": "rows", "rows": tuple(a["rows"]), "k": a["k"], "eps": a["eps"]}


def _c_fit_ball(s, a):
    s.fit = {"kind": "ball", "ball": s.ball["id"], "centres": tuple(a["centres"])}


def _c_areas(s, a):
    s.areas = dict(s.table)


def _c_frames(s, a):
    s.frames = dict(s.table, view=a.get("view"))


def _c_orient(s, a):
    before = s.orient["calls"] if s.orient else ()
    s.orient = {"calls": before + ((a["anchor"], a.get("view"), a.get("max_components", 0)),)}


def _c_triangles(s, a):
    wind = bool(a.get("flags", 0) & TRI_WIND_FRAMES)            # (the winding is a snapshot of the flipped bits at the call)
    s.triangles = dict(s.table, wind=wind, frames=s.frames if wind else None, orient=s.orient if wind else None)


def _c_holes(s, a):
    s.holes = {"triangles": s.triangles, "max_vertices": a["max_vertices"], "max_perimeter": a["max_perimeter"]}


def _c_ball(s, a):
    if a.get("max_entries", 0) == 1 or a["flags"] & 4:      # capped, or PCT_BALL_COUNT_ONLY: nothing is kept
        return
    s.ball = {"id": a["id"], "m": a["m"], "flags": a["flags"], "centres": a.get("centres")}


def _c_survar(s, a):
    lo, hi = s.rows
    s.table = {"k": a["k_total"] - 1, "eps": 0.0, "lo": lo, "hi": hi}


def _c_pca(s, a):
    s.pca = {"k": min(a["k"], s.n - 1), "keep": bool(a.get("keep"))}


def _setting(name):
    def create(s, a):
        setattr(s, name, a["value"])
    return create


_slab = ("not_slab", INVALID, _Q_SLAB)
_cloud = ("cloud", INVALID, _Q_NEED_CLOUD_Q)
_getter = dict(header=(_Q_SIDE,))

OPS = {
    # ---- clouds --------------------------------------------------------------------------------------------------------
    "set_points_f32": Op(["pct_set_points_f32"], drops=_ALL, creates=_new_cloud("host", "f32"), header=(_Q_NEW, _Q_TRI, _Q_HOLES, "It ends slab mode and owns the whole cloud", _Q_SETTINGS)),
    "set_points_f64": Op(["pct_set_points_f64"], drops=_ALL, creates=_new_cloud("host", "f64"), header=(_Q_NEW,)),
    "set_points_device": Op(["pct_device_alloc", "pct_device_upload", "pct_set_points_device_f32", "pct_device_free"], drops=_ALL,
                            creates=_new_cloud("device_copy", "f32"), header=(_Q_NEW,)),
    "use_points_device": Op(["pct_device_alloc", "pct_device_upload", "pct_use_points_device_f32"], drops=_ALL,
                            creates=_new_cloud("device_view", "f32"),
                            header=(_Q_NEW, "The buffer must stay allocated and unchanged until the next pct_set_points_* / pct_use_points_* call")),
    # ---- ownership -----------------------------------------------------------------------------------------------------
    "set_query_range": Op(["pct_set_query_range"], pre=[("cloud", INVALID, "pct_set_query_range and pct_set_query_slab need a cloud (PCT_ERR_INVALID)")],
                          drops=_PER_ROW, creates=_c_range, header=(_Q_OWN, _Q_TRI, _Q_HOLES, _Q_OWN_KEEPS, "also where the range is the one already set",
                                                                    "ends with pct_set_query_range, a new cloud or pct_set_query_slab(parts <= 0)")),
    "set_query_slab": Op(["pct_set_query_slab"], pre=[("cloud", INVALID, "pct_set_query_range and pct_set_query_slab need a cloud (PCT_ERR_INVALID)"),
                                                      ("slab_cloud", INVALID, "float32 clouds of >= 4096 points")],
                         drops=_PER_ROW, creates=_c_slab, header=(_Q_OWN, _Q_OWN_KEEPS, "Slab mode begins with pct_set_query_slab(parts >= 1)"),
                         variants=(None, {"parts": 1})),
    "set_grid_param": Op(["pct_set_grid_param"], creates=_setting("factor"), header=(_Q_SETTINGS,)),
    "set_stats": Op(["pct_set_stats"], creates=_setting("stats_on"), header=(_Q_SETTINGS,)),
    "set_async": Op(["pct_set_async"], creates=_setting("async_on"), header=(_Q_SETTINGS, _Q_ASYNC)),
    # ---- plantings and fits --------------------------------------------------------------------------------------------
    "knn": Op(["pct_knn"], pre=[("cloud", INVALID, _Q_PLANT_CLOUD), _slab], drops=_PER_ROW, creates=_c_knn,
              header=(_Q_PLANT, _Q_TRI, _Q_HOLES, _Q_PLANT_KEEPS, "pct_knn leaves its table")),
    "curvature": Op(["pct_curvature"], pre=[("cloud", INVALID, _Q_PLANT_CLOUD), ("slab_algo", INVALID, "pct_curvature refuses every algo but PCT_KNN_AUTO and PCT_KNN_GRID")],
                    drops=_PER_ROW, creates=_c_curvature, header=(_Q_PLANT, _Q_PLANT_KEEPS, "pct_curvature leaves its table and the cloud-aligned fit of it", _Q_FIT, _Q_ASYNC),
                    variants=(None, {"algo": 1})),
    "fit": Op(["pct_fit"], pre=[_slab, ("table", NO_NEIGHBORS, _Q_TABLE)], drops=("fit", "frames", "orient"), creates=_c_fit,
              header=(_Q_FIT, "The results of pct_fit and pct_curvature are cloud-aligned")),
    "fit_indices": Op(["pct_fit_indices"], pre=[_slab, _cloud], drops=("fit", "frames", "orient"), creates=_c_fit_indices,
                      header=(_Q_FIT, "those of pct_fit_indices and pct_fit_ball are row-aligned")),
    "fit_indices_f64": Op(["pct_fit_indices_f64"], pre=[_cloud], header=(_Q_SIDE, "pct_fit_indices_f64, pct_voxel_downsample and the stateless helpers keep working on a slab handle")),
    "surface_variation": Op(["pct_surface_variation"], pre=[_slab, ("cloud", INVALID, _Q_PLANT_CLOUD)], drops=_PER_ROW, creates=_c_survar,
                            header=(_Q_PLANT, _Q_PLANT_KEEPS, "pct_surface_variation leaves a plain table of k_total - 1 neighbours and no fit")),
    "pca_curvatures": Op(["pct_pca_curvatures"], pre=[_slab, ("cloud", INVALID, _Q_PLANT_CLOUD), ("whole", INVALID, "For every point of the loaded (whole) cloud")],
                         drops=_PER_ROW + ("pca",), creates=_c_pca,
                         header=(_Q_PLANT, _Q_PLANT_KEEPS, "pct_pca_curvatures leaves no readable table", "until the next planting) and no fit")),
    # ---- reading the table and the fit ---------------------------------------------------------------------------------
    "get_neighbors": Op(["pct_get_neighbors"], pre=[_slab, ("table", NO_NEIGHBORS, _Q_TABLE)], **_getter),
    "get_neighbor_rows": Op(["pct_get_neighbor_rows"], pre=[_slab, ("table", NO_NEIGHBORS, _Q_TABLE)], **_getter),
    "get_fit": Op(["pct_get_fit"], pre=[_slab, ("fit", INVALID, "pct_get_fit PCT_ERR_INVALID without fit results")], **_getter),
    "neighbor_study_curvatures": Op(["pct_neighbor_study_curvatures"],
                                    pre=[_slab, ("table", NO_NEIGHBORS, _Q_TABLE), ("plain_table", INVALID, "Needs a resident plain k-NN table with k >= n_hi")],
                                    variants=(None, {"n_hi": 1 << 20}), **_getter),
    # ---- areas, frames, orientation -------------------------------------------------------------------------------------
    "point_areas": Op(["pct_point_areas"], pre=[_slab, ("table", NO_NEIGHBORS, _Q_TABLE)], drops=("areas",), creates=_c_areas,
                      header=("pct_point_areas replaces the areas and touches nothing else",)),
    "get_point_areas": Op(["pct_get_point_areas"], pre=[_slab, ("areas", INVALID, "pct_get_point_areas PCT_ERR_INVALID without areas")], **_getter),
    "point_area_stats": Op(["pct_point_area_stats", "pct_point_area_profile"], folds=False, **_getter),
    "point_energies": Op(["pct_point_energies"], pre=[_slab, ("fit_cloud", INVALID, _Q_FITCLOUD), ("areas", INVALID, 'PCT_ERR_INVALID "no fit results" / "no point areas" otherwise')],
                         **_getter),
    "point_frames": Op(["pct_point_frames"], pre=[_slab, ("table", NO_NEIGHBORS, _Q_TABLE), ("fit_cloud", INVALID, _Q_FITCLOUD)], drops=("frames", "orient"),
                       creates=_c_frames, header=("pct_point_frames replaces the frames, drops the orientation and touches nothing else",)),
    "get_point_frames": Op(["pct_get_point_frames"], pre=[_slab, ("frames", INVALID, "pct_get_point_frames and pct_orient_frames PCT_ERR_INVALID without frames")], **_getter),
    "point_frame_stats": Op(["pct_point_frame_stats"], folds=False, **_getter),
    "orient_frames": Op(["pct_orient_frames"],
                        pre=[_slab, ("frames", INVALID, "pct_get_point_frames and pct_orient_frames PCT_ERR_INVALID without frames"),
                             ("table", INVALID, "pct_orient_frames answers PCT_ERR_INVALID"), ("whole", INVALID, "PCT_ERR_INVALID for an owned range or slab handle"),
                             ("view_given", INVALID, "PCT_ORIENT_VIEW without a finite viewpoint")],
                        creates=_c_orient, variants=(None, {"anchor": 2, "view": None}),
                        header=("pct_orient_frames turns the frames in place -- a second call starts from the frames as the first left them -- and replaces the orientation",
                                "a refused pct_orient_frames does not", _Q_REFUSED)),
    "get_orientation": Op(["pct_get_orientation"], pre=[_slab, ("orient", INVALID, "pct_get_orientation PCT_ERR_INVALID without an orientation")], **_getter),
    "orient_stats": Op(["pct_orient_stats"], folds=False, **_getter),
    # ---- fans and triangles (include/pct_hip_surface.h) ----------------------------------------------------------------
    "point_triangles": Op(["pct_point_triangles"],
                          pre=[_slab, ("table", NO_NEIGHBORS, _Q_TABLE), ("whole", INVALID, "PCT_ERR_INVALID for an owned range, as pct_orient_frames"),
                               ("tri_flags", INVALID, "Unknown flag bits: PCT_ERR_INVALID"),
                               ("tri_frames", INVALID, 'PCT_TRI_WIND_FRAMES without resident frames: PCT_ERR_INVALID "no point frames"')],
                          drops=("triangles", "holes"), creates=_c_triangles, variants=(None, {"flags": 64}, {"flags": TRI_WIND_FRAMES}),
                          header=("pct_point_triangles replaces the fans and triangles and touches nothing else", _Q_TRI, _Q_HOLES,
                                  "a fit, pct_point_frames, pct_orient_frames and pct_voxel_downsample do not", "the winding is a snapshot of the flipped bits at the call", _Q_REFUSED)),
    "get_point_fans": Op(["pct_get_point_fans"], pre=[("triangles", INVALID, "pct_get_point_fans and pct_get_triangles PCT_ERR_INVALID without triangles")], **_getter),
    "get_triangles": Op(["pct_get_triangles"], pre=[("triangles", INVALID, "pct_get_point_fans and pct_get_triangles PCT_ERR_INVALID without triangles")], **_getter),
    "point_triangle_stats": Op(["pct_point_triangle_stats"], folds=False, **_getter),
    # ---- boundary loops and small-hole filling (include/pct_hip_holes.h): made from the triangles ----------------------------
    "fill_holes": Op(["pct_fill_holes"], pre=[("not_slab", INVALID, _Q_HOLES_WHOLE), ("whole", INVALID, _Q_HOLES_WHOLE), ("triangles", INVALID, _Q_HOLES_WHOLE)],
                     drops=("holes",), creates=_c_holes,
                     header=("pct_fill_holes touches nothing else on the handle", _Q_HOLES_KEPT, "A refused call changes nothing: the hole results of an earlier call stay")),
    "get_hole_triangles": Op(["pct_get_hole_triangles"], pre=[("holes", INVALID, _Q_NO_HOLES)], header=(_Q_HOLES,)),
    "get_filled_triangles": Op(["pct_get_filled_triangles"], pre=[("holes", INVALID, _Q_NO_HOLES)], header=(_Q_HOLES,)),
    "get_boundary_loops": Op(["pct_get_boundary_loops"], pre=[("holes", INVALID, _Q_NO_HOLES)], header=(_Q_HOLES,)),
    "fill_hole_stats": Op(["pct_fill_hole_stats"], folds=False, header=("Zeros without hole results",)),
    # ---- queries of caller-supplied points, ball rows ------------------------------------------------------------------
    "query_points": Op(["pct_query_points"], pre=[_slab, _cloud], **_getter),
    "query_points_algo": Op(["pct_query_points_algo"], pre=[_slab, _cloud],
                            header=(_Q_SIDE, "The resident neighbour table, fit results and PCA results are untouched")),
    "query_stats": Op(["pct_query_stats"], folds=False, **_getter),
    "query_ball": Op(["pct_query_ball"], pre=[_slab, _cloud, ("room", LIMIT, "returns PCT_ERR_LIMIT: no rows are resident")], drops=("ball",), creates=_c_ball,
                     drops_on_refusal={LIMIT: ("ball",)}, variants=(None, {"max_entries": 1}),
                     header=("They stay on the device until the next pct_query_ball or pct_set_points*", "PCT_BALL_COUNT_ONLY: offsets alone, nothing is filled or kept",
                             "once its arguments are accepted it drops the rows of the previous query", "a query refused for its arguments or for the state of the handle leaves them",
                             "resident neighbour table, fit results, PCA results and their timings are untouched")),
    "get_ball": Op(["pct_get_ball"], pre=[("ball", INVALID, "pct_get_ball PCT_ERR_INVALID and pct_fit_ball PCT_ERR_NO_NEIGHBORS without ball rows"),
                                          ("ball_dist", INVALID, "needs PCT_BALL_DISTANCES")],
                   variants=(None, {"want_dist": True}), header=(_Q_SIDE, "pct_get_ball, pct_get_pca")),
    "ball_stats": Op(["pct_ball_stats"], folds=False, **_getter),
    "fit_ball": Op(["pct_fit_ball"], pre=[_slab, ("ball", NO_NEIGHBORS, "pct_get_ball PCT_ERR_INVALID and pct_fit_ball PCT_ERR_NO_NEIGHBORS without ball rows")],
                   drops=("fit", "frames", "orient"), creates=_c_fit_ball,
                   header=(_Q_FIT, "The resident ball rows, the resident neighbour table, PCA results and the cell list are untouched")),
    # ---- PCA -----------------------------------------------------------------------------------------------------------
    "get_pca": Op(["pct_get_pca"], pre=[("pca", INVALID, "pct_get_pca PCT_ERR_INVALID without PCA results"), ("pca_idx", INVALID, "and for idx unless keep_neighbors was set")],
                  variants=(None, {"want_idx": True}), **_getter),
    # ---- helpers that share the staging buffers ------------------------------------------------------------------------
    "voxel_downsample": Op(["pct_voxel_downsample"], drops=("table",),
                           header=("drop the table and nothing else: fit results, areas, frames, the orientation, ball rows and PCA results computed before stay readable, whichever sweep planted the table",)),
    "voxel_downsample_f32": Op(["pct_voxel_downsample_f32"], drops=("table",), header=("pct_voxel_downsample and pct_voxel_downsample_f32 drop the table and nothing else",)),
    "mesh_energies": Op(["pct_mesh_energies"], **_getter),
    "plane_rotate": Op(["pct_plane_rotate"], **_getter),
    "fit_quadric": Op(["pct_fit_quadric"], **_getter),
    "curvatures_from_coefficients": Op(["pct_curvatures_from_coefficients"], **_getter),
    # ---- slab records (values: tools/fuzz_slab.py) ---------------------------------------------------------------------
    "slab_counts": Op(["pct_slab_counts"], pre=[("slab_pass", INVALID, "pct_slab_counts and pct_slab_records refuse with PCT_ERR_INVALID until a pct_curvature has run in slab mode")], **_getter),
    "slab_records": Op(["pct_device_alloc", "pct_slab_records", "pct_device_download", "pct_device_free"],
                       pre=[("slab_pass", INVALID, "pct_slab_counts and pct_slab_records refuse with PCT_ERR_INVALID until a pct_curvature has run in slab mode")], **_getter),
    "scatter_records": Op(["pct_device_alloc", "pct_slab_records", "pct_scatter_records", "pct_device_download", "pct_device_free"],
                          header=(_Q_SIDE, "fails unless exactly end - begin records fell into the range"), no_state=True),
    # ---- measurement ---------------------------------------------------------------------------------------------------
    "get_timings": Op(["pct_get_timings"], **_getter),
    "get_timings_done": Op(["pct_get_timings_done"], folds=False, header=("pct_get_timings_done does NOT wait",)),
    "synchronize": Op(["pct_synchronize"], **_getter),
}

# ---- what the model leaves out, and why ----------------------------------------------------------------------------------
EXCLUDED = {
    **{f"pct_comm_{s}": "multi-process exchange: needs a world of ranks (tests/test_dist_gloo.py, bench.py --gpus)"
       for s in ("unique_id", "init", "destroy", "allgather_f32", "counters", "wait", "synchronize", "allreduce_f64")},
    "pct_text_shape": "host text parser: no handle, no state (tests/test_io.py)",
    "pct_text_load": "host text parser: no handle, no state (tests/test_io.py)",
    "pct_write_ply_ascii": "host PLY writer: no handle, no state (tests/test_io.py)",
    "pct_write_ply_ascii_normals": "host PLY writer: no handle, no state (tests/test_io.py)",
    "pct_write_ply_ascii_faces": "host PLY writer: no handle, no state (tests/test_gpu_triangles.py)",
    "pct_point_triangle_profile": "two device times of the last pct_point_triangles: nothing the model can hold a value to (tests/test_gpu_triangles.py)",
    "pct_matrix_norms_f32": "host pass over an array: no handle, no state",
    "pct_matrix_norms_f64": "host pass over an array: no handle, no state",
    "pct_format_float": "pure host function",
    "pct_selftest": "hardware self-test: reads and writes no state of the path",
    "pct_selftest_sort": "sorter self-test on caller arrays, device memory of its own: no state of the path (tests/test_gpu_sort_net.py)",
    "pct_selftest_sort_exact": "sorter self-test on caller arrays, device memory of its own: no state of the path (tests/test_gpu_sort_net.py)",
    "pct_selftest_order_keys": "sorter self-test on caller arrays, device memory of its own: no state of the path (tests/test_gpu_sort_net.py)",
    "pct_selftest_sweep": "sweep self-test on the handle's cloud: drops every result, as a new cloud does, and leaves none -- pct_get_neighbors after it is refused (tests/test_gpu_select.py); not drawn into the random sequences",
    "pct_selftest_levels_classify": "planning-kernel self-test on caller arrays, device memory of its own: no state of the path (tests/test_gpu_levels_exact.py)",
    "pct_selftest_levels_bands": "planning-kernel self-test on caller arrays, device memory of its own: no state of the path (tests/test_gpu_levels_exact.py)",
    "pct_selftest_levels_merge": "planning-kernel self-test on caller arrays, device memory of its own: no state of the path (tests/test_gpu_levels_exact.py)",
    "pct_device_count": "takes no handle: no state to model",
    "pct_create": "lifetime: the driver creates the handle under test and every fresh reference handle with it",
    "pct_destroy": "lifetime: every fresh reference handle is closed with it before the next is opened",
    "pct_last_error": "read by Handle._check for every refusal the driver provokes; holds no state of its own",
    "pct_version": "a constant string",
    "pct_timings_size": "a constant, checked when the binding loads",
}


def modelled_entry_points():
    return sorted({c for op in OPS.values() for c in op.calls})


def check(state, name, args):
    """(status, header quote) of the first unmet precondition, in the library's order; (OK, None) if the call goes through."""
    for cond, status, quote in OPS[name].pre:
        if not COND[cond](state, args or {}):
            return status, quote
    return OK, None


def first_unmet(state, name, args):
    """The name of the first unmet precondition, or None."""
    return next((cond for cond, _, _ in OPS[name].pre if not COND[cond](state, args or {})), None)


def refusal_key(state, name, args):
    """What a refusal exercises: the operation and the precondition that refuses it -- for pct_orient_frames also whether
    an orientation is resident, for pct_point_triangles whether triangles are: the one result a refused call of either
    could take along."""
    key = (name, first_unmet(state, name, args))
    if name == "orient_frames" and state.orient is not None: return key + ("orientation resident",)
    return key + ("triangles resident",) if name == "point_triangles" and state.triangles is not None else key


def unmet(state):
    """Every (operation, variant) whose precondition the state does not meet: what an out-of-state step may draw."""
    out = []
    for name, op in OPS.items():
        for v in op.variants:
            st, _ = check(state, name, v or {})
            if st != OK and (v is None or check(state, name, {})[0] == OK):      # (a variant counts where IT is what is unmet)
                out.append((name, v))
    return out


def apply(state, name, args):
    """(status, state after).  A refused call returns the state it was given, but for `drops_on_refusal`."""
    op = OPS[name]
    status, _ = check(state, name, args)
    s = state.copy()
    if op.folds:
        s.pending = False
    dropped = []
    for r in (op.drops if status == OK else op.drops_on_refusal.get(status, ())):
        if getattr(s, r) is not None:
            dropped.append(r)
        setattr(s, r, None)
    if status == OK and op.creates:
        op.creates(s, args)
    s.recent = tuple(r for r in tuple(dropped) + state.recent if getattr(s, r) is None)[:4]
    s.just = tuple(r for r in dropped if getattr(s, r) is None)
    s.last = name
    return status, s

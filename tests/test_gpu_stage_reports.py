"""The statistics of the five surface stages (point areas, point frames, their orientation, triangles, hole filling) on ONE
handle: a stage's numbers -- its device milliseconds included -- survive the stages that run after it, a refused call leaves
all of them alone, and they turn to zeros exactly when the stage's result goes (``pct_replacing``, csrc/pct_residents.h).
The stages share one stopwatch and one record type on the handle (csrc/pct_api_surface.hip); the counts themselves are held
to a fresh handle by tests/test_gpu_call_sequences.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, K = 2000, 12
STAGES = ("point_area_stats", "point_frame_stats", "orient_stats", "point_triangle_stats", "fill_hole_stats")


def read_all(h):
    return {s: getattr(h, s)() for s in STAGES}


def all_zero(d):
    return all(v == 0 for v in d.values())


def test_reports_survive_later_stages_and_go_with_their_results(gpu):
    capi = gpu["capi"]
    pts = gpu["shapes"].torus_random(N, seed=7)
    assert pts.dtype == np.float32 and pts.shape == (N, 3)
    h = capi.Handle(0)
    try:
        h.set_points(pts)
        h.curvature(K)
        calls = {"point_area_stats": h.point_areas, "point_frame_stats": h.point_frames, "orient_stats": lambda: h.orient_frames("top"),
                 "point_triangle_stats": lambda: h.point_triangles(wind_frames=True), "fill_hole_stats": h.fill_holes}
        seen = {}
        for s in STAGES:
            calls[s]()
            seen[s] = getattr(h, s)()
            print(s, seen[s])

        # survival: every stage's numbers as they were read behind its own call, the doubles bit for bit
        assert read_all(h) == seen
        for s in STAGES:
            assert seen[s]["ms"] > 0, s
        assert seen["point_triangle_stats"]["fan_ms"] > 0 and seen["point_triangle_stats"]["agree_ms"] > 0
        # (the five stages did something on this cloud)
        assert seen["point_area_stats"]["rows"] == N and seen["point_area_stats"]["closed"] > 0 and seen["point_area_stats"]["survivors"] > 0
        assert seen["point_frame_stats"]["rows"] == N
        assert seen["orient_stats"]["valid"] > 0 and seen["orient_stats"]["components"] >= 1 and seen["orient_stats"]["launches"] > 0
        assert seen["point_triangle_stats"]["rows"] == N and seen["point_triangle_stats"]["triangles"] > 0

        # a refused call leaves every report alone
        refused = (lambda: h.point_frames(viewpoint=[float("nan"), 0, 0]), lambda: h.orient_frames("view", viewpoint=None),
                   lambda: h.point_triangles(flags=2), lambda: h.fill_holes(max_vertices=2))
        for call in refused:
            with pytest.raises(ValueError):        # PCT_ERR_INVALID
                call()
            assert read_all(h) == seen

        # replacement follows pct_replacing: new frames drop the orientation and nothing else
        h.point_frames()
        now = read_all(h)
        assert all_zero(now["orient_stats"]), now["orient_stats"]
        for s in ("point_area_stats", "point_triangle_stats", "fill_hole_stats"):
            assert now[s] == seen[s], s
        fresh = now["point_frame_stats"]
        assert fresh["ms"] > 0
        assert {k: v for k, v in fresh.items() if k != "ms"} == {k: v for k, v in seen["point_frame_stats"].items() if k != "ms"}

        # ... new triangles drop the hole results
        h.point_triangles()
        assert all_zero(h.fill_hole_stats())
        assert h.point_triangle_stats()["ms"] > 0 and h.point_area_stats() == seen["point_area_stats"]

        # ... and a new table drops them all
        h.knn(K)
        for s, d in read_all(h).items():
            assert all_zero(d), (s, d)
    finally:
        h.close()

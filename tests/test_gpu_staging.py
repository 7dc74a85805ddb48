"""Interleaved calls on ONE handle whose staging claims differ in number and size (csrc/pct_internal.h: pct_ctx::stage,
pct_claim): every array a call returns is compared bit for bit with the same call on a fresh handle that ran only that
call's prerequisites.

The cloud is a seeded torus above the 4 096-point exhaustive route, swept with PCT_KNN_GRID, so the fit is stored in
table-row order and the row getters gather through a map into a claim of their own.  The sequence runs at 6 000 points and
again at 9 000 with more queries -- every claim of the second round is larger than the slot it finds -- and both under
PCT_NO_HEADROOM=1, where every slot moves whenever a request grows, and without it.

Claims nested above an entry point's own: pct_launch_fit_ball's two above the centres and the member counts, and -- the
second ball query has one row of more than 1 024 members, which sends every row through the library's segmented sort --
pct_launch_ball's sort scratch above the queries and the radii, whose distances are computed from the queries afterwards."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K_FIT = 12
ROUNDS = ((6000, 300, 1000), (9000, 450, 1500))        # points, ball queries, point queries


def _inputs(shapes, n, m_ball, m_query):
    rng = np.random.default_rng(n)
    pts = shapes.torus_random(n, seed=n)
    spacing = np.sqrt(4.0 * np.pi ** 2 * shapes.TORUS_R * shapes.TORUS_r / n)
    centres = np.sort(rng.choice(n, m_ball, replace=False)).astype(np.int64)
    radii = spacing * rng.uniform(2.0, 4.0, m_ball)                        # some 12 to 50 members per ball
    long_radii = radii.copy()
    long_radii[m_ball // 2] = 1.0                                          # ... and one that holds a good part of the torus
    queries = pts[rng.choice(n, m_query, replace=False)].astype(np.float64) + rng.normal(0.0, 0.3 * spacing, (m_query, 3))
    samples = np.sort(rng.choice(n, 50, replace=False)).astype(np.int64)
    return dict(pts=pts, n=n, centres=centres, ball_q=pts[centres].astype(np.float64), radii=radii, long_radii=long_radii, queries=queries,
                samples=samples, inner=(n // 7, n // 7 + n // 3), fans=(n // 5, n // 5 + n // 4))


# The steps of the sequence: (name, the prerequisites a fresh handle runs behind set_points, the call).  Every call returns a
# tuple of arrays.
def _curvature(h, c):
    h.curvature(K_FIT, algo=h.capi.KNN_GRID)


def _nothing(h, c):
    pass


def _inner_fit(h, c):
    _curvature(h, c)
    return h.get_fit(*c["inner"])


def _ball(h, c, radii="radii"):
    st, off = h.query_ball(c["ball_q"], c[radii], h.capi.BALL_SORTED | h.capi.BALL_DISTANCES)
    assert st == h.capi.PCT_OK
    return (off,) + h.get_ball(want_dist=True)


def _long_ball(h, c):
    got = _ball(h, c, "long_radii")
    assert np.diff(got[0]).max() > 1024, "no row takes the library's segmented sort"
    return got


def _fit_ball(h, c):
    used = h.fit_ball(c["centres"])
    return (used,) + h.get_fit(0, len(c["centres"]))


def _study(h, c):
    _curvature(h, c)
    return (h.neighbor_study_curvatures(c["samples"], 6, K_FIT),)


def _faces(h, c):
    h.point_areas()
    h.point_triangles()
    return h.get_point_fans(*c["fans"]) + h.get_point_areas(*c["fans"])


STEPS = (
    ("curvature, fit of an inner range", _nothing, _inner_fit),
    ("ball query", _nothing, _ball),
    ("ball fit", _ball, _fit_ball),
    ("ball query with a row past the in-kernel sort", _nothing, _long_ball),
    ("curvature, study", _nothing, _study),
    ("areas, triangles, fans", _curvature, _faces),
    ("point queries", _nothing, lambda h, c: h.query_points(c["queries"], 8, algo=h.capi.QUERY_AUTO)),
    ("fit of the whole range", _curvature, lambda h, c: h.get_fit(0, c["n"])),
)


def _handle(capi):
    h = capi.Handle(0)
    h.capi = capi
    return h


@pytest.fixture(scope="module")
def reference(gpu):
    """Per round: the inputs and, per step, what the call returns on a fresh handle behind its prerequisites alone."""
    capi, out = gpu["capi"], []
    for n, m_ball, m_query in ROUNDS:
        c = _inputs(gpu["shapes"], n, m_ball, m_query)
        want = []
        for _, pre, call in STEPS:
            h = _handle(capi)
            try:
                h.set_points(c["pts"])
                pre(h, c)
                want.append(call(h, c))
            finally:
                h.close()
        for arrays in want:
            for a in arrays:
                a.setflags(write=False)
        out.append((c, want))
    return out


@pytest.mark.parametrize("no_headroom", [True, False], ids=["exact_sizes", "headroom"])
def test_interleaved_calls_on_one_handle_match_fresh_handles(gpu, reference, monkeypatch, no_headroom):
    if no_headroom:
        monkeypatch.setenv("PCT_NO_HEADROOM", "1")
    else:
        monkeypatch.delenv("PCT_NO_HEADROOM", raising=False)
    h = _handle(gpu["capi"])
    try:
        for c, want in reference:
            h.set_points(c["pts"])
            for (name, _, call), ref in zip(STEPS, want):
                got = call(h, c)
                assert len(got) == len(ref), (c["n"], name)
                for j, (a, b) in enumerate(zip(got, ref)):
                    assert a.dtype == b.dtype and a.shape == b.shape, (c["n"], name, j, a.dtype, a.shape, b.dtype, b.shape)
                    same = a.view(np.uint8).reshape(-1) == b.view(np.uint8).reshape(-1)
                    assert same.all(), (c["n"], name, j, f"{int((~same).sum())} bytes differ, first at {int(np.flatnonzero(~same)[0])}")
    finally:
        h.close()

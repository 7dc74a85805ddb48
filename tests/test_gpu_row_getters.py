"""The row getters of the fit, the areas and the frames (pct_get_fit, pct_get_point_areas, pct_get_point_frames) on sub-ranges
and column subsets: one download and one gather kernel (csrc/pct_rows.hip) serve all three.

The full-range values are held to the exact restatements elsewhere (test_gpu_parity.py, test_gpu_point_areas.py,
test_gpu_point_frames.py).  Here, per result and per way its rows are stored -- table-row order behind a cell list, public
order behind the exhaustive sweep, an owned range [n/3, 2n/3) -- a 12-row span is read with every subset of its columns left
out and a 19-row span whole, and both must be the bytes of the same rows of the full read: columns of 1, 4, 8, 16, 24 and 48
bytes per row, where a wrong stride or word width of the gather shows.  An empty span answers empty arrays; a span that
leaves the owned rows is refused."""
import itertools

import pytest

import voronoi_exact as ve

pytestmark = pytest.mark.gpu

N, K = 1500, 12
# result -> (getter, its column keywords in the order of the tuple it returns, bytes per row of each)
GETTERS = {
    "fit": ("get_fit", ("coefs", "K", "H", "H2"), (24, 4, 4, 4)),
    "areas": ("get_point_areas", ("area", "closed", "nverts"), (8, 1, 4)),
    "frames": ("get_point_frames", ("normal", "k", "dirs", "flipped"), (24, 16, 48, 1)),
}


@pytest.fixture(scope="module", params=["row_order", "public_order", "owned_range"])
def planted(gpu, request):
    """A handle with table, fit, areas and frames in place; (handle, first owned row, end of the owned rows, full reads)."""
    capi = gpu["capi"]
    pts = ve.table_clouds(n=N)[0]
    h = capi.Handle(0)
    h.set_points(pts)
    b, e = (N // 3, 2 * N // 3) if request.param == "owned_range" else (0, N)
    if request.param == "owned_range":
        h.set_query_range(b, e)
    h.knn(K, 0.0, capi.KNN_BRUTE if request.param == "public_order" else capi.KNN_GRID)
    h.fit()
    h.point_areas()
    h.point_frames((0.3, -0.2, 5.0))
    full = {name: getattr(h, g)(b, e) for name, (g, _, _) in GETTERS.items()}
    yield h, b, e, full
    h.close()


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", list(GETTERS))
def test_full_read_has_the_documented_widths(planted, name):
    _, b, e, full = planted
    for col, width in zip(full[name], GETTERS[name][2]):
        assert len(col) == e - b and col.nbytes == (e - b) * width


@pytest.mark.parametrize("name", list(GETTERS))
def test_every_column_subset_of_a_span_is_the_full_reads_rows(planted, name):
    h, b, e, full = planted
    getter, cols, _ = GETTERS[name]
    for want in itertools.product((False, True), repeat=len(cols)):
        got = getattr(h, getter)(b + 7, b + 19, **dict(zip(cols, want)))
        for col, asked, part, whole in zip(cols, want, got, full[name]):
            if not asked:
                assert part is None, (col, want)
            else:
                assert _same_bytes(part, whole[7:19]), (col, want)
    for col, part, whole in zip(cols, getattr(h, getter)(b + 3, b + 22), full[name]):
        assert _same_bytes(part, whole[3:22]), col
    for col, part, whole in zip(cols, getattr(h, getter)(e - 19, e), full[name]):          # (the last rows: nothing read past the end)
        assert _same_bytes(part, whole[e - b - 19:]), col


@pytest.mark.parametrize("name", list(GETTERS))
def test_an_empty_span_answers_empty_arrays(planted, name):
    h, b, e, full = planted
    for at in (b, b + 5, e):
        for part, whole in zip(getattr(h, GETTERS[name][0])(at, at), full[name]):
            assert part.shape == (0,) + whole.shape[1:] and part.dtype == whole.dtype


@pytest.mark.parametrize("name", list(GETTERS))
def test_a_span_that_leaves_the_owned_rows_is_refused(planted, name):
    h, b, e, full = planted
    for lo, hi in ((0, 10) if b else (e, e + 10), (e - 5, e + 5), (b - 1, b + 1), (b - 10, b)):
        with pytest.raises(ValueError, match="outside the"):
            getattr(h, GETTERS[name][0])(lo, hi)
    for col, part, whole in zip(GETTERS[name][1], getattr(h, GETTERS[name][0])(b + 7, b + 19), full[name]):      # (a refusal disturbs nothing)
        assert _same_bytes(part, whole[7:19]), col

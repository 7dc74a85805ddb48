"""tests/select_exact.py against brute force and itself, and the preconditions of every case of tests/test_gpu_select.py (no GPU).

A cloud that stops reaching the edge it was built for fails here, on the CPU: the shares of the classes, the piles, the
overflowing stencils, the owned counts of the cells, the eps balls and the offsets of the far clouds are functions of the
inputs alone."""
import numpy as np
import pytest

import grid_exact as ge
import select_exact as se
import test_gpu_select as T

UNDECIDED_MAX = 0.02


@pytest.fixture(scope="module")
def clouds(built):
    return T.make_clouds(built["shapes"])


def by_name(name):
    return next(c for c in T.CASES if c["name"] == name)


@pytest.mark.parametrize("c", T.CASES, ids=[c["name"] for c in T.CASES])
def test_classes_are_disjoint_and_few_rows_undecided(clouds, c):
    a = T.analysis(clouds, c)
    n = len(a["m"])
    assert not (a["must_redo"] & a["must_final"]).any()
    assert not (a["undecided"] & (a["must_redo"] | a["must_final"])).any()
    assert a["undecided"].sum() <= UNDECIDED_MAX * n, (c["name"], int(a["undecided"].sum()), n)
    assert not (a["by_guarantee"] & ~a["must_redo"]).any() and a["must_redo"][a["over"]].all()
    # a trusted set is k+1 distinct candidates led by the smallest key
    for row in np.flatnonzero(~a["tie"])[:200]:
        members, keys = a["set_k1"][row]
        assert len(set(members.tolist())) == c["k"] + 1 and (np.diff(keys.astype(np.int64)) >= 0).all() and row in se.stencil_members(a, row)


@pytest.mark.parametrize("name", ["thin-square-a", "thin-sphere-b", "piles-pair", "clump-duo", "far-under"])
def test_stencil_populations_are_the_census(clouds, name):
    c = by_name(name)
    a = T.analysis(clouds, c)
    b = a["b"]
    m, _ = b["cells_obj"].stencils()
    assert np.array_equal(a["m"], m[b["cells_obj"].of_point])
    over = m > a["cap"]
    assert ge.census(b, c["k"])[0][1] == int(b["cells_obj"].owned[over].sum()) == int(a["over"].sum())


@pytest.mark.parametrize("name", ["thin-square-a", "thin-sphere-a", "k127", "sphere-f64", "eps-duo"])
def test_rows_against_brute_force(clouds, name):
    """tk, the eps ball and the k+1-nearest set from every point of the cloud inside the guaranteed ball, and the guarantee
    itself: a point outside the 27 cells is never nearer than guaranteed_r2 (test_query_plan's property) -- so a row that is
    not must_redo by the guarantee has its k+1 nearest inside its stencil, and one that is could have a nearer point outside."""
    c = by_name(name)
    pts = T.points_of(clouds, c)
    a = T.analysis(clouds, c)
    k, b = c["k"], a["b"]
    rec = pts.astype(np.float32).astype(np.float64)
    qry = pts.astype(np.float64) if pts.dtype == np.float64 else rec
    eps2 = c["eps"] ** 2 if c["eps"] > 0 else np.inf
    rng = np.random.default_rng(7)
    for row in rng.choice(len(pts), 150, replace=False):
        d = rec - qry[row]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        inside = np.zeros(len(pts), bool)
        inside[se.stencil_members(a, row)] = True
        assert inside[row] and inside.sum() == a["m"][row]
        # the guarantee: nothing outside the stencil lies within it
        assert not (~inside & (d2 < a["g2"][row])).any(), (name, row)
        assert int((inside & (d2 < eps2)).sum()) == a["inball"][row]
        keys = se.key_of(d2, a["scale"], a["KEY_BITS"])
        order = np.lexsort((np.arange(len(pts)), d2))
        assert (np.diff(keys[order].astype(np.int64)) >= 0).all(), "the key of a distance is monotone in the distance"
        sten = np.sort(keys[inside & (d2 < eps2)])
        if len(sten) > k:
            assert a["tk"][row] == sten[k]
            if not a["must_redo"][row] and not a["undecided"][row]:
                # proven: every point of the cloud with a key up to tk is in the stencil
                assert not (~inside & (keys <= sten[k]) & (d2 < eps2)).any(), (name, row)
        else:
            assert a["tk"][row] == se.PAD
        if a["set_k1"][row] is not None:
            members = a["set_k1"][row][0]
            want = order[inside[order] & (d2[order] < eps2)][:k + 1]
            assert np.array_equal(members, want), (name, row)


def test_keys_are_monotone_and_saturate():
    for kb in (26, 25, 23, 22):
        scale = se.scale_of(0.37, kb)
        d2 = np.sort(np.concatenate([[0.0], np.geomspace(1e-12, 12.0 * 0.37 ** 2, 4000)]))
        keys = se.key_of(d2, scale, kb).astype(np.int64)
        assert (np.diff(keys) >= 0).all() and keys[0] == 0 and keys[-1] == (1 << kb) - 2
        assert keys[np.searchsorted(d2, 2.25 * 0.37 ** 2)] < (1 << kb) - 2          # the guaranteed range stays below the saturated key


def test_constants_are_the_kernels():
    assert se.constants(se.PAIR) == (64, 26) and se.constants(se.DUO, 2) == (128, 25)
    assert se.constants(se.FAST, 1) == (64, 26) and se.constants(se.FAST, 2) == (128, 25)
    assert se.constants(se.FAST, 1, pre=False) == (64, 23) and se.constants(se.FAST, 2, pre=False) == (128, 22)


# ---- the preconditions of the GPU cases ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["thin-square-a", "thin-square-b", "thin-sphere-a", "thin-sphere-b", "thin-square-duo"])
def test_thin_clouds_have_rows_on_both_sides_of_the_guarantee(clouds, name):
    a = T.analysis(clouds, by_name(name))
    share = a["by_guarantee"].mean()
    assert 0.2 <= share <= 0.8, (name, share)
    assert (~a["must_redo"] & ~a["undecided"]).sum() >= 0.15 * len(a["m"])
    assert sum(a["set_k1"][r] is not None for r in np.flatnonzero(a["by_guarantee"])) >= 100          # rows a lean kernel may trust


def test_rim_rows_have_an_unbounded_guarantee(clouds):
    a = T.analysis(clouds, by_name("rim"))
    assert tuple(a["b"]["dims"]) == (3, 3, 1)
    assert (a["gkey"] == se.PAD).sum() >= 10 and (a["gkey"] != se.PAD).sum() >= 100
    assert not a["must_redo"][a["gkey"] == se.PAD].any()


@pytest.mark.parametrize("name,k,LIST", [("piles-pair", 30, 64), ("piles-duo", 100, 128)])
def test_piles_reach_their_edges(clouds, name, k, LIST):
    c = by_name(name)
    pts = T.points_of(clouds, c)
    a = T.analysis(clouds, c)
    assert a["LIST"] == LIST
    _, label, size = np.unique(pts.view(np.uint32).reshape(len(pts), 3), axis=0, return_inverse=True, return_counts=True)
    size_of = size[label.ravel()]
    for s in T.pile_sizes(k, LIST):
        assert (size == s).sum() >= 2 or s in (34, 35, 36) and (size == s).sum() >= 2, (name, s)
    lone = (pts[:, 1] == -2.0) & (size_of == 1)
    assert lone.sum() == len(T.pile_sizes(k, LIST))
    # a pile larger than LIST leaves its own rows and its lone neighbour no threshold; one of LIST rows does
    assert a["no_threshold"][size_of == LIST + 1].all() and not a["no_threshold"][size_of == LIST].any()
    assert a["no_threshold"][lone].sum() >= 1
    # ties across k | k+1: a row of a pile of at least k+2 records is never trusted; runs on both sides of 34
    assert a["tie"][size_of == k + 2].all() and a["tie"][size_of == k - 1].all()
    assert a["long_run"][size_of == 35].all() and not a["long_run"][(size_of == 34) & (pts[:, 1] == -1.0)].any()
    # the isolated piles stand alone in their stencils
    alone = (pts[:, 1] == -1.0) & (size_of > 1)
    assert np.array_equal(a["m"][alone], size_of[alone])


@pytest.mark.parametrize("name", ["doubled-k49", "doubled-k50"])
def test_doubled_cloud_ties_at_the_boundary_of_k50_only(clouds, name):
    a = T.analysis(clouds, by_name(name))
    if name.endswith("50"):
        assert a["tie"].all()
    else:
        assert a["tie"].mean() < 0.05 and sum(a["set_k1"][r] is not None for r in np.flatnonzero(a["by_guarantee"])) >= 20


@pytest.mark.parametrize("name", ["clump-pair", "clump-duo"])
def test_clump_overflows_beside_stencils_within_the_capacity(clouds, name):
    a = T.analysis(clouds, by_name(name))
    assert a["over"].sum() >= 100 and (~a["over"]).sum() >= 1000
    assert a["m"].max() > a["cap"] and ((a["m"] <= a["cap"]) & (a["m"] > a["cap"] - 128)).any()


@pytest.mark.parametrize("family", [se.PAIR, se.DUO])
def test_cap_sizes_are_the_scan_of_the_disc(family):
    """The chosen disc populations, re-derived: a greedy cover of the capacity edges over the scanned sizes, and at each
    chosen size a query's stencil with exactly each population it is listed for."""
    k, targets = T.CAP_K[family], T.CAP_TARGETS[family]
    hits = {}
    for n_disc in range(1900, 2048):
        cells = ge.build(T.clump_sized(n_disc), k)["cells_obj"]
        m, _ = cells.stencils()
        m = set(m[cells.owned > 0].tolist())
        hits[n_disc] = {t for t in targets if t in m}
    left, chosen = set(targets), {}
    while left:
        best = max(hits, key=lambda s: len(hits[s] & left))          # (the first of the best: the scan's order)
        assert hits[best] & left, sorted(left)
        chosen[best] = tuple(sorted(hits[best] & left))
        left -= hits[best]
    assert chosen == (T.CAP_PAIR if family == se.PAIR else T.CAP_DUO)
    assert ge.stage_cap(k) == targets[-2]                              # the capacity itself is the last edge


@pytest.mark.parametrize("name", ["items-q1", "items-q64"])
def test_item_cases_hold_cells_of_every_owned_count(clouds, name):
    """1, 2, an odd number, 16, 17 and more than 32 owned points: the odd tail that runs its last query twice, one item and
    several per cell at the default, one query per item and (PCT_ITEMS_Q = 64) one item for cells of up to 64"""
    c = by_name(name)
    a = T.analysis(clouds, c)
    owned = a["b"]["cells_obj"].owned
    assert {1, 2, 16, 17} <= set(owned.tolist()) and (owned > 32).any() and ((owned % 2 == 1) & (owned > 2)).any(), name
    assert a["b"]["items_q"] == int(c["env"]["PCT_ITEMS_Q"])


def test_eps_cases_reach_their_edges(clouds):
    c = by_name("eps-exact")
    pts, a = T.points_of(clouds, c), T.analysis(clouds, c)
    rec = pts.astype(np.float64)
    d = rec[3000:3200] - rec[:200]
    assert np.array_equal((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], np.full(200, T.EPS_EXACT ** 2))     # exactly on the bound: outside
    assert a["b"]["cell_size"] < T.EPS_EXACT                  # (the twin is a candidate of the stencil or of none: either way not a neighbour)
    a = T.analysis(clouds, by_name("eps-list"))
    assert (a["ball"] <= a["LIST"]).sum() >= 300 and (a["ball"] > a["LIST"]).sum() >= 300 and a["must_final"].sum() >= 300
    a = T.analysis(clouds, by_name("eps-short"))
    short = (a["inball"] <= 30) & (a["eps_key"] > a["gkey"])
    assert short.sum() >= 50 and a["must_redo"][short].all()
    a = T.analysis(clouds, by_name("eps-duo"))
    assert (a["inball"] > 128).any() and a["must_final"].any() and a["must_redo"].any()


def test_far_clouds_straddle_the_bound_of_the_q64_forms(clouds):
    """plan_sweep: near = far * 2^-23 < cell * 2^-7, far the largest coordinate of the grid's box"""
    for name, side in (("far-under", True), ("far-over", False)):
        b = T.analysis(clouds, by_name(name))["b"]
        lo = b["lo"].astype(np.float64)
        far = max(max(abs(lo[i]), abs(lo[i] + b["dims"][i] * b["cell_size"])) for i in range(3))
        ratio = far * 2.0 ** -23 / (b["cell_size"] * 2.0 ** -7)
        assert (0.98 < ratio < 1.0) if side else (1.0 < ratio < 1.02), (name, ratio)
    b = T.analysis(clouds, by_name("far-f32"))["b"]
    assert float(b["lo"][1]) / b["cell_size"] >= 1e4

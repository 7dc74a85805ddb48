"""The fast sweeps' selection and proofs, row by row on the device (pct_selftest_sweep: the planned fast sweep alone).

A whole-cloud comparison sees the table after k_knn_exact has redone the flagged rows: a proof that is too weak, a wrong
trusted mark or a proof that is too strict hardly ever shows there.  Here every case runs the planned kernel once, reads which
rows it stored as final, which it flagged and which it marked trusted, and holds that to tests/select_exact.py (the classes
must_redo / must_final / undecided, none of which depends on the threshold T the device finds) and to the exhaustive sweep
of a second handle:

  1. sound: a row without the redo flag equals the exhaustive row bit for bit -- indices, float32 distances, eps count;
  2. must_redo rows are flagged; 3. must_final rows are not;
  4. a trusted row is flagged, not of an overflowing item, has k full columns that are k distinct members of the stencil's
     k+1-nearest set, the missing member has the smallest key of the set; no mark under PCT_REDO_ADOPT=0, PCT_REDO_SEED=0 or
     from k_knn_fast;
  5. a flagged row of a lean kernel under the seed holds nothing (column 0 is -1) or distinct real records of its own
     stencil in a prefix of its columns -- k of them where the eps ball of the stencil holds k+1, all of the ball otherwise;
  6. the kernel family and the Q64 bit are the ones the case names; redo_count is the number of flagged rows.

The preconditions of every case (the shares of the classes, the edges a cloud is built to reach, at most 2 % undecided rows)
are functions of the inputs: tests/test_select_exact.py asserts them on the CPU.  Flagged rows outside must_redo are printed
per case and asserted nowhere: they depend on T.

PCT_FAST_R1_MAX is read once per process: its case runs this file as a program in a process of its own.

That the cases bind: the library rebuilt with one proof weakened at a time in k_knn_pair and k_knn_duo (value-level edits on
scratch copies: no address, index or loop bound changes), this file alone against each, on an MI355X (48 cases):

  mutant                                             cases that failed
  `trusted` without its `!tie`                       doubled-k50 (marks across the tie of entries k and k+1)
  the eps test `d2 < eps2` -> `<=`                   eps-exact (final rows count the neighbour on the bound)
  the saturation test dropped                        16: thin-square-a, thin-square-b, thin-square-duo, k60, k61, k127,
                                                     k63-r1max, pair-no-dist, duo-no-dist, no-adopt, no-seed, piles-duo,
                                                     doubled-k49, doubled-k50, far-under, far-f32 (must_redo rows stored as final)
  `trusted` without `tk + 1 <= bkey`                 none
  `lo2 = v_T (1 + 2^-12)` for `(1 - 2^-20)`          none
  `tk + 1u` -> `tk` in need_k                        none
  my_gkey from ceil instead of the floor             none

The four that no case noticed are not caught for a reason, not for want of rows.  The last two move the proof by ONE key unit:
they change a row's fate only where need and gkey differ by exactly one, which is the class `undecided` by definition, so
only a row stored as final and wrong could show them -- a point outside the 27 cells, or a cut candidate, inside one key
unit (2^-26 of 2.3 cell^2) of the (k+1)-th entry and ahead of it in (d2, public index) order.  The two on bkey act on the
band between the float32 threshold T and its exact counterpart, and T is the device's own (the secant through v_rcp_f32):
a restatement cannot name a row whose cut candidate lies in that band.  A cloud that plants such a row for a cell edge the
build chooses is still missing."""
import os
import subprocess
import sys

import numpy as np
import pytest

import select_exact as se

FAST, PAIR, DUO = se.FAST, se.PAIR, se.DUO
Q64 = se.Q64_BIT
KNOBS = ("PCT_NO_PAIR", "PCT_NO_PAIR_KERNEL", "PCT_NO_DUO_KERNEL", "PCT_KEEP_DIST", "PCT_NO_XCD_MAP", "PCT_FAST_R1_MAX", "PCT_ITEMS_Q",
         "PCT_REDO_SEED", "PCT_REDO_ADOPT", "PCT_NO_CULL", "PCT_NO_SPEC")

EPS_EXACT = 0.125                                  # "eps-exact": 200 rows have a neighbour at exactly this distance
PILE_STEP = 0.5                                    # "piles": spacing of the planted piles, several cell edges


def pile_sizes(k, LIST):
    return (k - 1, k, k + 1, k + 2, 34, 35, 36, LIST - k - 1, LIST - k, LIST, LIST + 1)


def piles_cloud(rng, k, LIST):
    """The unit square, and below it two rows of piles of bit-identical points, PILE_STEP apart: the upper row's piles
    alone in their stencils, the lower row's each beside a lone point a hundredth of the step away."""
    square = np.zeros((2000, 3))
    square[:, :2] = rng.random((2000, 2))
    parts = [square]
    for j, size in enumerate(pile_sizes(k, LIST)):
        x = 0.25 + PILE_STEP * j
        parts.append(np.tile([[x, -1.0, 0.0]], (size, 1)))
        parts.append(np.tile([[x, -2.0, 0.0]], (size, 1)))
        parts.append(np.array([[x + 0.01 * PILE_STEP, -2.0, 0.0]]))
    pts = np.concatenate(parts)
    return pts[rng.permutation(len(pts))]


def clump_sized(n_disc):
    """The clump with the first n_disc points of its disc: the disc's population moves single stencils across a capacity."""
    rng = np.random.default_rng(20240611)
    sq = np.zeros((2000, 3))
    sq[:, :2] = rng.random((2000, 2))
    r = 0.03 * np.sqrt(rng.random(2048))
    phi = 2.0 * np.pi * rng.random(2048)
    disc = np.stack([0.5 + r * np.cos(phi), 0.5 + r * np.sin(phi), np.zeros(2048)], axis=1)[:n_disc]
    pts = np.concatenate([sq, disc])
    return pts[np.random.default_rng(n_disc).permutation(len(pts))].astype(np.float32)


# Disc populations (of 1900 .. 2047, scanned on the CPU: tests/test_select_exact.py re-derives them) at which some stencil
# holds exactly the named number of candidates: the staging capacity (512 | 768) and every multiple of 128 below it down to
# the fewest staged batch pairs the family compiles a body for, each with its two neighbours
CAP_PAIR = {1918: (383, 511, 512, 513), 1915: (257, 385), 1998: (255, 384), 1913: (256,)}
CAP_DUO = {1928: (639, 640, 641), 1941: (511, 767), 1989: (385, 512), 1900: (384,), 1901: (383,), 1918: (513,), 1937: (768,), 1982: (769,)}
CAP_K = {PAIR: 30, DUO: 80}
CAP_TARGETS = {PAIR: [128 * j + d for j in (2, 3, 4) for d in (-1, 0, 1)], DUO: [128 * j + d for j in (3, 4, 5, 6) for d in (-1, 0, 1)]}


def make_clouds(shapes):
    rng = np.random.default_rng(20250117)
    clouds = {f"clump-{n}": clump_sized(n) for n in sorted(set(CAP_PAIR) | set(CAP_DUO))}
    square = np.zeros((3000, 3))
    square[:, :2] = rng.random((3000, 2))          # z exactly 0: the rim of the grid is everywhere in z
    clouds["square"] = square.astype(np.float32)
    clouds["small"] = clouds["square"][:300]      # a grid of 3 x 3 x 1 cells: the cube of the centre cell covers it, gkey = 0xFFFFFFFF
    v = rng.standard_normal((3000, 3))
    clouds["sphere"] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    clouds["piles30"] = piles_cloud(rng, 30, 64).astype(np.float32)
    clouds["piles100"] = piles_cloud(rng, 100, 128).astype(np.float32)
    import test_gpu_redo_seed as rs
    seam = rs.two_density_torus(shapes, 12_000, seed=3)
    clouds["doubled"] = np.ascontiguousarray(np.concatenate([seam[:2000], seam[:2000]])[np.random.default_rng(5).permutation(4000)])
    # the clump of tests/test_gpu_sweep_prologue.py: stencils beyond the staging capacity next to stencils within it
    sq = np.zeros((2000, 3))
    sq[:, :2] = rng.random((2000, 2))
    r = 0.03 * np.sqrt(rng.random(2000))
    phi = 2.0 * np.pi * rng.random(2000)
    disc = np.stack([0.5 + r * np.cos(phi), 0.5 + r * np.sin(phi), np.zeros(2000)], axis=1)
    clouds["clump"] = np.concatenate([sq, disc])[rng.permutation(4000)].astype(np.float32)
    # 200 rows with a neighbour at exactly EPS_EXACT: both on a 2^-12 lattice, so the difference and its square are exact
    e = square.copy()
    snapped = np.round(e[:200, :2] * 4096.0) / 4096.0
    e[:200, :2] = snapped
    twins = np.zeros((200, 3))
    twins[:, 0], twins[:, 1] = snapped[:, 0] + EPS_EXACT, snapped[:, 1]
    clouds["eps-exact"] = np.concatenate([e, twins]).astype(np.float32)
    # float64 clouds far from the origin: the rounding distance of a query against the cell edge (plan_sweep's `near`)
    for name, far in (("far-under", FAR_UNDER), ("far-over", FAR_OVER)):
        f = square.copy()
        f[:, 0] += far
        clouds[name] = f
    f = square.copy()
    f[:, 1] += FAR_F32
    clouds["far-f32"] = f.astype(np.float32)
    return clouds


# Offsets of the far clouds (the cell edge of the square at k = 30 and factor 0.3 is 0.0536: tests/test_select_exact.py re-derives the bound):
# the largest coordinate * 2^-23 just under / just over cell * 2^-7, and 10^4 cell edges in float32
FAR_UNDER, FAR_OVER, FAR_F32 = 3500.0, 3540.0, 540.0


def case(name, cloud, k, family, eps=0.0, factor=0.0, q64=False, dist=True, **env):
    return dict(name=name, cloud=cloud, k=k, family=family, eps=eps, factor=factor, q64=q64, dist=dist, env=env)


CASES = [
    # thin: rows on both sides of need <= gkey, rows at the rim of the grid (gkey = 0xFFFFFFFF)
    case("thin-square-a", "square", 30, PAIR, factor=0.3),
    case("thin-square-b", "square", 30, PAIR, factor=0.22),
    case("thin-sphere-a", "sphere", 30, PAIR, factor=0.3),
    case("thin-sphere-b", "sphere", 30, PAIR, factor=0.22),
    case("thin-square-duo", "square", 100, DUO, factor=0.3),
    case("rim", "small", 30, PAIR, factor=1.3),
    # k and family
    case("k1", "square", 1, PAIR, factor=2.0),
    case("k5", "square", 5, PAIR, factor=1.0),
    case("k60", "square", 60, PAIR, factor=0.3),
    case("k61", "square", 61, DUO, factor=0.3),
    case("k127", "square", 127, DUO, factor=0.3),
    case("k63-r1max", "square", 63, PAIR, factor=0.3, PCT_FAST_R1_MAX="64"),
    case("fast-r1", "square", 30, FAST, factor=0.3, PCT_NO_PAIR_KERNEL="1"),
    case("fast-r2", "square", 100, FAST, factor=0.3, PCT_NO_DUO_KERNEL="1"),
    case("fast-one-query-k30", "square", 30, FAST, factor=0.3, PCT_NO_PAIR="1"),
    case("fast-one-query-k100", "square", 100, FAST, factor=0.3, PCT_NO_PAIR="1"),
    case("pair-no-dist", "square", 30, PAIR, factor=0.3, dist=False),
    case("duo-no-dist", "square", 100, DUO, factor=0.3, dist=False),
    case("no-adopt", "square", 30, PAIR, factor=0.3, PCT_REDO_ADOPT="0"),
    case("no-seed", "square", 30, PAIR, factor=0.3, PCT_REDO_SEED="0"),
    # piles: ties across k | k+1, equal-key runs on both sides of 34, no threshold, a threshold below 1e-30
    case("piles-pair", "piles30", 30, PAIR),
    case("piles-duo", "piles100", 100, DUO),
    case("doubled-k49", "doubled", 49, PAIR),
    case("doubled-k50", "doubled", 50, PAIR),
    # cap: overflowing items beside items within the staging capacity
    case("clump-pair", "clump", 30, PAIR),
    case("clump-duo", "clump", 80, DUO),
    # items: the odd tail, several items per cell
    case("items-q1", "clump", 30, PAIR, factor=0.5, PCT_ITEMS_Q="1"),
    case("items-q64", "clump", 30, PAIR, factor=0.5, PCT_ITEMS_Q="64"),
    # eps
    case("eps-exact", "eps-exact", 30, PAIR, eps=EPS_EXACT),
    case("eps-list", "square", 30, PAIR, eps=0.08),
    case("eps-short", "piles30", 30, PAIR, eps=0.3),
    case("eps-duo", "square", 100, DUO, eps=0.15),
    # coordinates
    case("far-under", "far-under", 30, PAIR, factor=0.3, q64=True),
    case("far-over", "far-over", 30, FAST, factor=0.3),
    case("far-f32", "far-f32", 30, PAIR, factor=0.3),
    case("sphere-f64", "sphere", 30, PAIR, factor=0.3, q64=True),
]
# cap: single stencils one below, at and one above the staging capacity and the multiples of 128 below it
CASES += [case(f"cap-pair-{n}", f"clump-{n}", CAP_K[PAIR], PAIR) for n in CAP_PAIR] + [case(f"cap-duo-{n}", f"clump-{n}", CAP_K[DUO], DUO) for n in CAP_DUO]


def points_of(clouds, c):
    p = clouds[c["cloud"]]
    return p.astype(np.float64) if c["q64"] or c["cloud"] in ("far-under", "far-over") else p


_ANALYSES = {}


def analysis(clouds, c):
    """select_exact.analyse of a case, once per session (tests/test_select_exact.py shares it)"""
    if c["name"] not in _ANALYSES:
        env = c["env"]
        fam = c["family"]
        regs = 2 if c["k"] + 1 > int(env.get("PCT_FAST_R1_MAX", 61)) else 1
        pre = c["cloud"] != "far-over"             # (k_knn_fast keys every candidate of a far float64 cloud in float64: no pre-selection)
        _ANALYSES[c["name"]] = se.analyse(points_of(clouds, c), c["k"], c["eps"], c["factor"], fam, regs, pre, items_q=int(env.get("PCT_ITEMS_Q", 16)),
                                          r1_max=int(env.get("PCT_FAST_R1_MAX", 61)))
    return _ANALYSES[c["name"]]


@pytest.fixture(scope="module")
def bench(gpu):
    ref = gpu["capi"].Handle(0)
    yield {"ref": ref, "capi": gpu["capi"], "clouds": make_clouds(gpu["shapes"]), "oracle": {}}
    ref.close()


def oracle_rows(bench, c, pts):
    """the exhaustive sweep of a handle of its own, once per (cloud, dtype, k, eps)"""
    key = (c["cloud"], str(pts.dtype), c["k"], c["eps"])
    if key not in bench["oracle"]:
        ref, capi = bench["ref"], bench["capi"]
        ref.set_points(pts)
        ref.knn(c["k"], c["eps"], capi.KNN_BRUTE)
        idx, dist, cnt = ref.get_neighbors(0, len(pts), want_count=True)
        assert ref.timings()["sweep_variant"] == 0
        bench["oracle"][key] = (np.where(idx >= len(pts), -1, idx), dist, cnt)
    return bench["oracle"][key]


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_rows_meet_their_fate(bench, c, monkeypatch):
    for v in KNOBS:
        monkeypatch.delenv(v, raising=False)
    for name, value in c["env"].items():
        monkeypatch.setenv(name, value)
    if "PCT_FAST_R1_MAX" in c["env"]:              # read once per process: the case runs in a process of its own
        if bench.get("broken"):
            pytest.fail("not run: the library raised in " + bench["broken"])
        done = subprocess.run([sys.executable, os.path.abspath(__file__), c["name"]], capture_output=True, text=True, timeout=300)
        print(done.stdout, done.stderr)
        assert done.returncode == 0, (c["name"], done.stdout[-2000:], done.stderr[-2000:])
        return
    check_case(bench, c)


def check_case(bench, c):
    capi = bench["capi"]
    pts = points_of(bench["clouds"], c)
    k, name = c["k"], c["name"]
    a = analysis(bench["clouds"], c)
    if bench.get("broken"):                        # nothing more is launched behind a call the library failed in
        pytest.fail("not run: the library raised in " + bench["broken"])
    bench["broken"] = name
    want_idx, want_dist, want_cnt = oracle_rows(bench, c, pts)

    h = capi.Handle(0)                            # a fresh handle: no warm start of the cell-size search, as the restatement's
    try:
        h.set_grid_param(c["factor"])
        h.set_points(pts)
        out = h.selftest_sweep(k, c["eps"], capi.KNN_GRID, want_dist=c["dist"])
        with pytest.raises(AttributeError, match="no neighbour table"):        # the table is unfinished: nothing is resident
            h.get_neighbors(0, 1)
    finally:
        h.close()
    bench["broken"] = None
    flagged, trusted, idx = out["redo"], out["trusted"], out["idx"]
    extra = int((flagged & ~a["must_redo"]).sum())
    print(name, "variant", bin(out["sweep_variant"]), "flagged", int(flagged.sum()), "of them outside must_redo", extra, "trusted", int(trusted.sum()),
          "must_redo", int(a["must_redo"].sum()), "must_final", int(a["must_final"].sum()), "undecided", int(a["undecided"].sum()))

    # the grid is the restated one: the classes speak about this launch
    b = a["b"]
    assert out["cell_size"] == b["cell_size"] and out["dims"] == tuple(b["dims"]), (name, out["cell_size"], out["dims"], b["cell_size"], b["dims"])
    assert np.array_equal(np.asarray(out["origin"]), b["lo"].astype(np.float64)), (name, out["origin"], b["lo"])
    assert out["items_q"] == int(c["env"].get("PCT_ITEMS_Q", 16)), (name, out["items_q"])
    # 6. family, Q64, the count
    assert out["sweep_variant"] & 3 == c["family"], (name, bin(out["sweep_variant"]))
    assert bool(out["sweep_variant"] & Q64) == c["q64"], (name, bin(out["sweep_variant"]))
    assert out["redo_count"] == int(flagged.sum()), (name, out["redo_count"], int(flagged.sum()))
    assert (out["dist"] is not None) == (c["dist"] or c["family"] == FAST), name
    # 1. sound
    final = ~flagged
    bad = final & (idx != want_idx).any(axis=1)
    assert not bad.any(), (name, "final rows whose indices differ from the exhaustive sweep", np.flatnonzero(bad)[:8])
    if out["dist"] is not None:
        bad = final & (out["dist"].view(np.uint32) != want_dist.view(np.uint32)).any(axis=1)
        assert not bad.any(), (name, "final rows whose distances differ", np.flatnonzero(bad)[:8])
    if c["eps"] > 0:
        bad = final & (out["count"] != want_cnt)
        assert not bad.any(), (name, "final rows whose eps count differs", np.flatnonzero(bad)[:8])
    # 2. and 3.
    bad = a["must_redo"] & ~flagged
    assert not bad.any(), (name, "must_redo rows stored as final", np.flatnonzero(bad)[:8])
    bad = a["must_final"] & flagged
    assert not bad.any(), (name, "must_final rows on the redo list", np.flatnonzero(bad)[:8])
    # 4. trusted
    lean = c["family"] in (PAIR, DUO)
    seed = lean and c["env"].get("PCT_REDO_SEED") != "0"
    adopt = seed and c["env"].get("PCT_REDO_ADOPT") != "0"
    if not adopt:
        assert not trusted.any(), (name, "marks without adoption", int(trusted.sum()))
    assert not (trusted & ~flagged).any(), name
    assert not (trusted & a["over"]).any(), name
    for row in np.flatnonzero(trusted):
        cols = idx[row]
        assert (cols >= 0).all() and len(set(cols.tolist())) == k, (name, row, "a trusted row holds k distinct records")
        assert a["set_k1"][row] is not None, (name, row, "trusted across a tie of entries k and k+1, or without a (k+1)-th entry")
        members, keys = a["set_k1"][row]
        missing = np.setdiff1d(members, cols)
        assert len(missing) == 1 and np.isin(cols, members).all(), (name, row, "the columns are not the stencil's k+1 nearest but one")
        assert keys[members == missing[0]][0] == keys.min(), (name, row, "the missing member has not the smallest key")
    # 5. what a lean kernel leaves in a flagged row under the seed
    if seed:
        for row in np.flatnonzero(flagged):
            cols = idx[row]
            real = int((cols >= 0).sum())
            if cols[0] < 0:
                assert real == 0, (name, row, "a row that starts with -1 holds something")
                continue
            assert (cols[:real] >= 0).all() and len(set(cols[:real].tolist())) == real, (name, row, "real columns are a prefix of distinct records")
            assert np.isin(cols[:real], se.stencil_members(a, row)).all(), (name, row, "records outside the row's own stencil")
            if not a["over"][row]:
                assert real == min(k, int(a["inball"][row]) - 1), (name, row, real, int(a["inball"][row]))
    assert flagged[a["over"]].all(), name


if __name__ == "__main__":                         # one case in a process of its own, under the switches its parent set
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as entry
    entry.build()
    from point_cloud_toolbox_amd import _capi, shapes
    case_ = next(c for c in CASES if c["name"] == sys.argv[1])
    reference = _capi.Handle(0)
    try:
        check_case({"ref": reference, "capi": _capi, "clouds": make_clouds(shapes), "oracle": {}}, case_)
    finally:
        reference.close()

"""The bars of tests/aux_exact.py on the CPU: the reference meets them, planted defects do not.

  * oracle.mesh_energies equals the run of the reference's own function body (tests/golden/g12_energies.npz) bit for bit;
  * the reference's per-triangle loop -- and NumPy's vectorised form of it on the launch-edge meshes -- meets every bar
    against the exact (rational area, fsum) reference, and so does a NumPy restatement of the kernel's summation tree;
  * each planted defect misses at least one bar on at least one case;
  * the vectorised first-occurrence reference of the voxel tests agrees with oracle.voxel_downsample on the goldens.
No GPU, no import of the package.
"""
import math

import numpy as np
import pytest

import aux_exact as ax
import pct_oracle as oracle

_REF = {}


def _case(g, case):
    """(v, t, K, H, golden) with float64 zeros where the case has no curvatures; the exact reference computed once."""
    v, t, K, H, out = ax.golden_case(g, case)
    K, H = ax.curvatures_or_zeros(v, K, H)
    if case not in _REF:
        _REF[case] = ax.exact_energies(v, t, K, H)
    return v, t, K, H, out, _REF[case]


def _edge(T, dtype):
    key = (T, np.dtype(dtype).name)
    if key not in _REF:
        m = ax.edge_mesh(T, dtype)
        _REF[key] = (m, ax.reference_energies(*m))
    return _REF[key]


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("case", ax.GOLDEN_CASES)
def test_oracle_mesh_energies_equal_the_reference_run(golden, case):
    v, t, K, H, out = ax.golden_case(golden(ax.GOLDEN), case)
    K, H = ax.curvatures_or_zeros(v, K, H)
    with np.errstate(all="ignore"):
        got = oracle.mesh_energies(v, t, K, H)
    assert np.array_equal(_bits(got), _bits(out)), (case, got, out)


def test_golden_cases_are_what_they_claim(golden):
    g = golden(ax.GOLDEN)
    assert all(len(ax.golden_case(g, c)[1]) <= 2000 for c in ax.GOLDEN_CASES)
    v, t, K, H, out = ax.golden_case(g, "random_f64")
    A = ax.exact_areas(v, t)
    fh2, fk = ax.face_means(t, K, H)
    dropped = (A == 0) & (np.isinf(fh2) | np.isinf(fk))
    assert dropped.sum() >= 8 and np.isnan(K).any() and np.isinf(K).any() and (K == -np.inf).any()      # inf * 0 is there
    assert not (np.isinf(fk) & (A > 0)).any() and not (np.isinf(fh2) & (A > 0)).any() and all(math.isfinite(x) for x in out)
    assert (np.asarray(t)[:, 0] == np.asarray(t)[:, 1]).any()                                        # repeats in a triple
    kinds = {c: tuple(a.dtype.name for a in ax.golden_case(g, c)[2:4]) for c in ("random_f32", "random_f64", "mixed_K64_H32", "mixed_K32_H64")}
    assert kinds == {"random_f32": ("float32", "float32"), "random_f64": ("float64", "float64"),
                     "mixed_K64_H32": ("float64", "float32"), "mixed_K32_H64": ("float32", "float64")}
    assert ax.golden_case(g, "no_curvatures")[2] is None
    assert ax.golden_case(g, "zero_area")[4] == (0.0, 0.0, 0.0) and not ax.exact_areas(*ax.golden_case(g, "zero_area")[:2]).any()
    v, t = ax.golden_case(g, "slivers")[:2]
    e = np.linalg.norm(v[t[:, 1]] - v[t[:, 0]], axis=1)
    aspect = e * e / (2 * ax.exact_areas(v, t))                       # base / height
    assert aspect.min() < 2 and aspect.max() > 5e11
    out = ax.golden_case(g, "live_inf")[4]
    assert out[0] == math.inf and math.isnan(out[1]) and math.isfinite(out[2])
    # the mixed pair at float64 accuracy in the float64 array: each sum of a mixed case is the pure case's of that dtype
    o = {c: ax.golden_case(g, c)[4] for c in kinds}
    assert o["mixed_K64_H32"] == (o["random_f32"][0], o["random_f64"][1], o["random_f64"][2])
    assert o["mixed_K32_H64"] == (o["random_f64"][0], o["random_f32"][1], o["random_f64"][2])
    assert o["random_f32"][0] != o["random_f64"][0] and o["random_f32"][1] != o["random_f64"][1]


# ------------------------------------------------------------------------------------------- the reference meets the bars
@pytest.mark.parametrize("case", ax.GOLDEN_CASES)
def test_reference_loop_meets_the_bars_on_the_goldens(golden, case):
    v, t, K, H, out, (want, facts) = _case(golden(ax.GOLDEN), case)
    if case == "zero_area":
        assert want == (0.0, 0.0, 0.0) == tuple(out) == ax.emulate_kernel(v, t, K, H)      # small integers: nothing rounds
    assert ax.same_values(out, want), (case, out, want)
    fin = [i for i in range(3) if math.isfinite(want[i])]
    bar = ax.bars(facts)
    sh = ax.shares(out, want, bar)
    emu = ax.shares(ax.emulate_kernel(v, t, K, H), want, bar)
    print(f"{case}: reference loop at {max([sh[i] for i in fin]):.3f} of the bar, the kernel's tree in NumPy at {max([emu[i] for i in fin]):.3f}")
    assert all(sh[i] <= 1 for i in fin) and all(emu[i] <= 1 for i in fin), (case, sh, emu)
    assert ax.same_values(ax.emulate_kernel(v, t, K, H), want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("T", ax.EDGE_T)
def test_reference_meets_the_bars_at_the_launch_edges(T, dtype):
    (v, t, K, H), (want, facts, sides) = _edge(T, dtype)
    assert sides == (1 if T <= ax.EXACT_T_MAX else 2) and all(math.isfinite(x) for x in want)
    bar = ax.bars(facts, sides)
    with np.errstate(all="ignore"):
        ref = oracle.mesh_energies(v, t, K, H) if T <= ax.EXACT_T_MAX else ax.numpy_energies(v, t, K, H)
    sh = ax.shares(ref, want, bar)
    emu = ax.shares(ax.emulate_kernel(v, t, K, H), want, bar)
    print(f"T={T} {np.dtype(dtype).name}: depth {ax.kernel_depth(T)}, reference at {max(sh):.3f} of the bar, the kernel's tree in NumPy at {max(emu):.3f}")
    assert max(sh) <= 1 and max(emu) <= 1, (T, sh, emu)


def test_kernel_depth_counts_the_launch():
    S = ax.MESH_STRIDE
    assert [ax.kernel_blocks(T) for T in (1, 256, 257, S, S + 1)] == [1, 1, 2, 1024, 1024]
    assert [ax.kernel_depth(T) for T in (1, 256, 257, S, S + 1, 2 * S + 300)] == [12, 12, 13, 1035, 1036, 1037]
    assert ax.EDGE_T == (1, 255, 256, 257, 262144, 262145, 524588)


def test_exact_area_is_exact():
    v = np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0], [1e-160, 0, 0], [0, 1e-160, 0], [1, 1, 1], [1 + 2.0 ** -52, 1, 1], [1, 1 + 2.0 ** -52, 1]])
    t = np.array([[0, 1, 2], [0, 3, 4], [5, 6, 7]])
    A = ax.exact_areas(v, t)
    assert A[0] == 6.0 and A[2] == 2.0 ** -105
    assert A[1] > 0                                                                                  # (no underflow in the rational product)
    assert ax.float64_areas(v, t)[1] == 0.0                                                          # ... where float64 has one


# -------------------------------------------------------------------------------------------------------- planted defects
def _misses(v, t, K, H, want, bar, defect):
    got = ax.emulate_kernel(v, t, K, H, defect)
    return (not ax.same_values(got, want)) or max(s for s, w in zip(ax.shares(got, want, bar), want) if math.isfinite(w)) > 1


@pytest.mark.parametrize("defect", ax.DEFECTS)
def test_planted_defects_miss_a_bar(golden, defect):
    g = golden(ax.GOLDEN)
    where = []
    for case in ("icosphere_f32", "random_f32", "random_f64", "slivers"):
        v, t, K, H, out, (want, facts) = _case(g, case)
        if _misses(v, t, K, H, want, ax.bars(facts), defect):
            where.append(case)
    for T in (257, ax.MESH_STRIDE + 1, 2 * ax.MESH_STRIDE + 300):
        (v, t, K, H), (want, facts, sides) = _edge(T, np.float32)
        if _misses(v, t, K, H, want, ax.bars(facts, sides), defect):
            where.append(T)
    print(f"{defect}: misses a bar on {where}")
    expected = {"mean64": {"icosphere_f32", "random_f32", "slivers", 257},            # float32 arrays only
                "mean_sq": {"icosphere_f32", "random_f32", "random_f64", "slivers", 257},
                "nan_first": {"random_f32", "random_f64"},                            # where inf * 0 occurs
                "drop_tail": {ax.MESH_STRIDE + 1, 2 * ax.MESH_STRIDE + 300},          # where the loop has a partial last pass beyond the first
                "drop_block": {"icosphere_f32", "random_f32", "random_f64", 257, ax.MESH_STRIDE + 1}}[defect]
    assert expected <= set(where), (defect, where)
    if defect == "mean64":
        assert "random_f64" not in where                                              # (the defect is none there)


# ------------------------------------------------------------------------------------------------------------ voxel cases
@pytest.mark.parametrize("tag", ["f64", "f32", "lattice_f32", "lattice_f32_v01", "tuples"])
def test_first_occurrence_agrees_with_the_restatement_and_the_reference_run(golden, tag):
    g = golden("g11_prep.npz")
    pts, voxel = g[f"ds_{tag}_in"], float(g[f"ds_{tag}_voxel"])
    idx = ax.first_occurrence(pts, voxel)
    assert idx.dtype == np.int64 and (np.diff(idx) > 0).all()
    assert np.array_equal(pts[idx], oracle.voxel_downsample(pts, voxel)) and np.array_equal(pts[idx], g[f"ds_{tag}_out"])


def test_first_occurrence_semantics():
    pts = np.array([[0.05, 0.05, 0.05], [0.06, 0.01, 0.09], [0.15, 0.0, 0.0], [-0.01, 0.0, 0.0], [0.19, 0.09, 0.01], [-0.0, 0.0, 0.0]])
    assert ax.first_occurrence(pts, 0.1).tolist() == [0, 2, 3]


def test_voxel_cases_are_what_they_claim():
    assert ax.N_THREE_PASSES == 524_545 and -(-ax.N_THREE_PASSES // ax.VOXEL_BLOCK) == 2 * ax.SCAN_PASS + 2
    for dtype in (np.float32, np.float64):
        for axis in range(3):
            for span in (ax.VOXEL_SPAN_MAX - 1, ax.VOXEL_SPAN_MAX):
                p, voxel = ax.span_cloud(dtype, axis, span)
                r = ax.voxel_rows(p, voxel)
                assert p.dtype == dtype and (r.max(0) - r.min(0)).tolist() == [span if a == axis else 0 for a in range(3)]
                assert ax.first_occurrence(p, voxel).tolist() == [0, 1]
        m = ax.multiples_cloud(dtype, 0.05)
        assert m.dtype == dtype and np.signbit(m[m == 0]).any() and (m < 0).any()
        idx = ax.first_occurrence(m, 0.05)
        assert np.array_equal(m[idx], oracle.voxel_downsample(m, 0.05))
    p, voxel = ax.offset_cloud()
    r32, r64 = ax.voxel_rows(p, voxel), ax.voxel_rows(p.astype(np.float64), voxel)
    assert p.dtype == np.float32 and (r32 != r64).any()                 # the float32 quotient decides
    assert np.array_equal(p[ax.first_occurrence(p, voxel)], oracle.voxel_downsample(p, voxel))

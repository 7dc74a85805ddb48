"""The CPU restatement of the reference's PCA estimator (pct:901-950) against goldens of the unmodified reference
(tests/golden/g12_pca_*.npz, tools/make_goldens_pca.py)."""
import glob
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pca_restatement as pr  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[len("g12_pca_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "g12_pca_*.npz")))


def golden_out(g):
    return dict(l1=g["pca_principal_curvature_values_1"], l2=g["pca_principal_curvature_values_2"],
                dirs=g["principal_curvature_directions"], K=g["pca_K_values"], H=g["pca_H_values"])


def test_goldens_are_present():
    assert {"sphere2k_k30", "torus4k_k50", "bunny4k_k20", "torus3k_f64_k40", "egg64_k30", "dups360_k12", "n10_k15",
            "torus500_k2", "n10_k0", "n10_k1"} <= set(CASES)


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_the_reference(golden, case):
    g = golden(f"g12_pca_{case}.npz")
    if "error" in g:
        assert str(g["error"]) == "ValueError: array must not contain infs or NaNs"
        return
    pts, k = g["points"], int(g["k"])
    ref = golden_out(g)
    n = len(pts)
    assert ref["l1"].shape == (n,) and ref["dirs"].shape == (n, 3, 2) and ref["K"].dtype == np.float64
    res = pr.restate(pts, k)
    assert np.array_equal(res["ambiguous"], g["ambiguous"])
    ok = pr.compare(res, ref, res["l3"], rows_mask=~g["ambiguous"])
    assert ok.all(), f"{(~ok).sum()} of {n} rows outside the bars"

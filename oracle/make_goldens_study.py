"""Generate tests/golden/g13_neighbor_study.npz from the UNMODIFIED reference (build container only).

TEST INFRASTRUCTURE.  Run from the repo root:  MPLBACKEND=Agg python oracle/make_goldens_study.py

G8 (oracle/make_goldens.py) records one whole-sample result at tol = 1e-7, where no |K(n + 1) - K(n)| of a curved cloud
is ever below the tolerance: every sample ends at the upper bound and the result says nothing about the values.  G13
records the reference where its bisection decides something.  explicit_quadratic_neighbor_study returns only
int(mean) + 1 (pct:800), so with sample_size = 1 under np.random.seed(s) one call yields one sample's converged count + 1;
the draw is repeated under the same seed (pct:753).

  cloud32   shapes.torus_random(3000, seed=5), float32
  cloud64   the same torus drawn in float64, x 0.2 + 40: the float32 rounding of a coordinate is a visible share of a
            neighbour distance (as tests/test_gpu_pca.py and wide_exact.f64)
  cases     (tol, lower, upper) = (0.03, 3, 99), (0.1, 3, 99), (0.03, 10, 40) on both clouds; on cloud64 also the same three
            with tol / 0.2^2 (K of a cloud scaled by s is K / s^2: the tolerance that asks the same question)
  per seed  48 seeds: the drawn index and count + 1 for every case
  whole     sample_size = 60 under seeds 100, 101, 102: the 60 indices and the result for every case

Points and integers only.  Nothing from the reference is written into this repository except these numbers.
"""
import os

import numpy as np

from make_goldens import OUT, load_reference, load_shapes

SEEDS = np.arange(48)
WHOLE_SEEDS = np.array([100, 101, 102])
CASES = ((0.03, 3, 99), (0.1, 3, 99), (0.03, 10, 40))
SCALE, OFFSET = 0.2, 40.0


def study(pc, seed, size, case):
    tol, lo, hi = case
    np.random.seed(int(seed))
    res = pc.explicit_quadratic_neighbor_study(tol=tol, sample_size=size, lower_bound=lo, upper_bound=hi)
    np.random.seed(int(seed))
    draw = np.random.randint(0, len(pc.points), size)                  # same draw as pct:753
    return draw, res


def record(ref, points, cases):
    pc = ref.PointCloud(points=points, normals=np.zeros((len(points), 0)))
    pc.plant_kdtree(100)                                               # the tree the study queries (pct:74, 759)
    draws = np.array([study(pc, s, 1, cases[0])[0][0] for s in SEEDS], np.int64)
    per_seed = np.array([[study(pc, s, 1, c)[1] for c in cases] for s in SEEDS], np.int32)
    whole_draws = np.array([study(pc, s, 60, cases[0])[0] for s in WHOLE_SEEDS], np.int64)
    whole = np.array([[study(pc, s, 60, c)[1] for c in cases] for s in WHOLE_SEEDS], np.int32)
    return draws, per_seed, whole_draws, whole


def main():
    ref = load_reference()
    sh = load_shapes()
    p32 = sh.torus_random(3000, seed=5)
    p64 = sh.torus_random(3000, seed=5, dtype=np.float64) * SCALE + OFFSET
    assert p32.dtype == np.float32 and p64.dtype == np.float64
    cases64 = CASES + tuple((t / (SCALE * SCALE), lo, hi) for t, lo, hi in CASES)
    out = dict(points32=p32, points64=p64, seeds=SEEDS, whole_seeds=WHOLE_SEEDS,
               cases32=np.array(CASES, np.float64), cases64=np.array(cases64, np.float64))
    for tag, pts, cases in (("32", p32, CASES), ("64", p64, cases64)):
        draws, per_seed, whole_draws, whole = record(ref, pts, cases)
        out.update({"draw" + tag: draws, "plus1_" + tag: per_seed, "whole_draw" + tag: whole_draws, "whole" + tag: whole})
    np.savez_compressed(os.path.join(OUT, "g13_neighbor_study.npz"), **out)
    print("g13 written:", {k: np.asarray(v).shape for k, v in out.items()})


if __name__ == "__main__":
    main()

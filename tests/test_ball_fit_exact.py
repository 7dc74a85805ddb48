"""What tests/test_gpu_fit_ball.py relies on, pinned on the CPU (no GPU, no import of the package).

The device is compared with ``ball_fit_exact.reference``: the oracle's reference-faithful loop on the ranked members of
every ball.  Here the oracle's two restatements -- ``curvature_loop`` (np.cov, LAPACK's SVD and gelsd per row) and
``curvature_batched`` (padded rows plus ``count``: eigh, normal equations) -- are held against each other on every case the
device tests use, under the project's contract (``curvature_tolerance_ok``, rtol 1e-5, floor 1e-2 x the curvature scale):
two independent statements of the same arithmetic agree on every row of at least four members, whatever the order of the
members between ``near`` and ``far``.

The only rows left out of value comparisons anywhere are those of fewer than four members: their covariance has rank at
most two in a way that leaves the normal to rounding ("decided by LAPACK's rounding").  The exemption is exactly
``members < 4`` -- ``ball_fit_exact.MIN_MEMBERS`` -- and is asserted to be no wider: every longer row must agree.  On the
ladder it covers the five lengths L = 0 ... 4 of every sample row, 3.5 % of its rows."""
import numpy as np
import pytest

import ball_exact as be
import ball_fit_exact as bfe
import pct_oracle as oracle
import wide_exact as we


def _agree(a, b, scales):
    okK = oracle.curvature_tolerance_ok(a[1], b[1], 1e-2 * scales[0])
    okH = oracle.curvature_tolerance_ok(a[2], b[2], 1e-2 * scales[1])
    return okK & okH


def _batched(points, centres, ranked, rows):
    """curvature_batched on the listed rows (each of at least two members), in chunks that keep the padded block small."""
    out = [np.full((len(ranked), 6), np.nan, np.float32)] + [np.full(len(ranked), np.nan, np.float32) for _ in range(3)]
    order = sorted(rows, key=lambda i: len(ranked[i]))           # rows of similar length share a padded block
    for s in range(0, len(order), 128):
        part = order[s:s + 128]
        idx, count = bfe.padded([ranked[i] for i in part])
        with np.errstate(invalid="ignore", divide="ignore"):
            got = oracle.curvature_batched(points, idx, np.asarray(centres)[part], count)
        for o, g in zip(out, got):
            o[part] = g
    return out


def _permuted(ranked, seed):
    """The members between near and far shuffled."""
    rng = np.random.default_rng(seed)
    out = []
    for x in ranked:
        y = x.copy()
        if len(y) > 3:
            y[1:-1] = y[1:-1][rng.permutation(len(y) - 2)]
        out.append(y)
    return out


def _check(name, points, centres, ranked, scales):
    used = np.array([len(x) for x in ranked])
    fitted = [int(i) for i in np.flatnonzero(used >= 2)]
    loop = bfe.reference(points, centres, ranked=ranked)
    bat = _batched(points, centres, ranked, fitted)
    ok = _agree(bat, loop, scales)
    bad = np.flatnonzero(~ok & (used >= 2))
    print(f"{name}: {len(fitted)} fitted rows, {len(bad)} disagree, their members {sorted(set(used[bad].tolist()))}")
    assert (used[bad] < bfe.MIN_MEMBERS).all(), (name, "rows of >= 4 members disagree", bad[used[bad] >= bfe.MIN_MEMBERS][:8], used[bad][:8])
    perm = bfe.reference(points, centres, ranked=_permuted(ranked, 7))
    long_rows = used >= bfe.MIN_MEMBERS
    assert _agree(perm, loop, scales)[long_rows].all(), (name, "the order of the members between near and far matters")
    return loop


def test_exemption_is_members_below_four():
    assert bfe.MIN_MEMBERS == 4
    members = bfe.ladder_members()
    share = (members < bfe.MIN_MEMBERS).mean()
    assert (members < bfe.MIN_MEMBERS).sum() == 5 * bfe.LADDER_SAMPLE_ROWS and abs(share - 5 / len(be.LADDER)) < 1e-12 and share < 0.036


def test_ladder_restatements_agree():
    pts, centres, q, r = bfe.ladder_case(we)
    ranked = bfe.ranked_rows(pts, centres, r, queries=q)
    assert np.array_equal([len(x) for x in ranked], bfe.ladder_members())
    _check("ladder", pts, centres, ranked, bfe.SCALES["torus"])


@pytest.mark.parametrize("name", sorted(bfe.cloud_cases(we)))
def test_cloud_restatements_agree(name):
    key, pts, centres, r = bfe.cloud_cases(we)[name]
    ranked = bfe.ranked_rows(pts, centres, r)
    used = np.array([len(x) for x in ranked])
    if key == "clump":
        assert used.max() > 2048, "the clump is here for rows past 2 048 members"
    if key == "twins":
        assert (used >= 599).any(), "rows of coinciding members"
    loop = _check(name, pts, centres, ranked, bfe.SCALES[key])
    if key in ("flat", "line"):
        long_rows = used >= bfe.MIN_MEMBERS
        assert (np.abs(loop[1][long_rows]) <= 1e-2).all() and (np.abs(loop[2][long_rows]) <= 1e-2).all(), "|K|, |H| within the floor"


@pytest.mark.parametrize("k", (30, 80))
def test_knn_radii_reproduce_the_knn_rows(k):
    pts = we.torus()
    ranking = we.ranked(pts, width=k + 2)
    assert not we.tie_at(ranking, k).any()
    r = bfe.knn_radii(we, pts, k, ranking)
    sample = bfe.seeded_centres(len(pts), 5)
    ranked = bfe.ranked_rows(pts, sample, r[sample])
    assert all(np.array_equal(x, ranking[0][c, 1:k + 1]) for x, c in zip(ranked, sample))

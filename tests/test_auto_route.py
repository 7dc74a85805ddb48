"""The rules of a sweep's route (csrc/pct_auto_route.h), on the CPU: what a request resolves to, when PCT_KNN_AUTO trusts
its remembered verdict, when the uniform list may be given up, the skew gate and the census verdict.

A stand-alone program that includes nothing but that header prints what the rules say; every expectation below is
written out from the rule (DESIGN 4.1 *Dispatch*, 4.4), each on both sides of its boundary, not recomputed from the
header."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "point-cloud-toolbox_amd", "csrc")

PROGRAM = r"""
#include "pct_auto_route.h"
#include <stdio.h>

static const RouteSwitches kOff = {false, false}, kNoTree = {true, false}, kNoLevels = {false, true};

// refusal algo auto_req tree_ok as one number: r * 1000 + algo * 100 + auto_req * 10 + tree_ok
static void resolve(const char* name, int asked, int k, int64_t n, bool whole, bool slab, bool fused) {
    Request r;
    const Refusal f = resolve_request(asked, k, n, whole, slab, fused, &r);
    printf("%s %d\n", name, (int)f * 1000 + r.algo * 100 + (int)r.auto_req * 10 + (int)r.tree_ok);
}
static Request req(int algo, bool auto_req, bool tree_ok) { return Request{algo, auto_req, tree_ok}; }

static void census(const char* name, unsigned long long q, unsigned long long over, unsigned long long shrt, unsigned long long cells, int64_t n, bool tree) {
    const unsigned long long c[4] = {q, over, shrt, cells};
    printf("%s %d\n", name, (int)census_route(census_shares(c), n, tree));
}

int main() {
    // ---- the request
    resolve("auto_4095", PCT_KNN_AUTO, 30, 4095, true, false, false);
    resolve("auto_4096", PCT_KNN_AUTO, 30, 4096, true, false, false);
    resolve("auto_k127", PCT_KNN_AUTO, 127, 5000, true, false, false);
    resolve("auto_k128", PCT_KNN_AUTO, 128, 5000, true, false, false);
    resolve("auto_small_k128", PCT_KNN_AUTO, 128, 4000, true, false, false);
    resolve("grid_k127", PCT_KNN_GRID, 127, 5000, true, false, false);
    resolve("grid_k128", PCT_KNN_GRID, 128, 5000, true, false, false);
    resolve("brute_k127", PCT_KNN_BRUTE, 127, 5000, true, false, false);
    resolve("brute_k128", PCT_KNN_BRUTE, 128, 5000, true, false, false);
    resolve("levels", PCT_KNN_GRID_LEVELS, 30, 5000, true, false, false);
    resolve("tree", PCT_KNN_TREE, 30, 5000, true, false, false);
    resolve("tree_k128", PCT_KNN_TREE, 128, 5000, true, false, false);
    resolve("unknown_6", 6, 30, 5000, true, false, false);
    resolve("unknown_neg", -1, 30, 5000, true, false, false);
    resolve("shard", PCT_KNN_GRID, 30, 5000, false, false, false);
    resolve("n_2p26_less", PCT_KNN_GRID, 30, ((int64_t)1 << 26) - 1, true, false, false);
    resolve("n_2p26", PCT_KNN_GRID, 30, (int64_t)1 << 26, true, false, false);
    resolve("slab_auto_fused", PCT_KNN_AUTO, 30, 5000, true, true, true);
    resolve("slab_grid_fused", PCT_KNN_GRID, 30, 5000, true, true, true);
    resolve("slab_exact_fused", PCT_KNN_GRID_EXACT, 30, 5000, true, true, true);
    resolve("slab_auto_k128_fused", PCT_KNN_AUTO, 128, 5000, true, true, true);
    resolve("slab_grid_stepwise", PCT_KNN_GRID, 30, 5000, true, true, false);
    resolve("slab_brute_fused", PCT_KNN_BRUTE, 30, 5000, true, true, true);
    resolve("slab_levels_fused", PCT_KNN_GRID_LEVELS, 30, 5000, true, true, true);
    resolve("slab_tree_fused", PCT_KNN_TREE, 30, 5000, true, true, true);

    // ---- the remembered verdict: calls 1..32 with a matching n
    const Request a = req(PCT_KNN_GRID, true, true);
    int32_t calls = 0;
    for (int i = 1; i <= 32; ++i) printf("cadence_%d %d\n", i, (int)remembered_applies(a, 20000, 20000, &calls, kOff));
    printf("cadence_calls %d\n", calls);
    // the counter moves only where auto_req, tree_ok and the size all hold (the switches are looked at after it)
    calls = 0;
    printf("other_n %d\n", (int)remembered_applies(a, 20000, 20001, &calls, kOff));
    printf("never_remembered %d\n", (int)remembered_applies(a, 20000, 0, &calls, kOff));
    printf("not_auto %d\n", (int)remembered_applies(req(PCT_KNN_GRID, false, true), 20000, 20000, &calls, kOff));
    printf("not_tree_ok %d\n", (int)remembered_applies(req(PCT_KNN_GRID, true, false), 20000, 20000, &calls, kOff));
    printf("still_calls %d\n", calls);
    printf("no_tree %d\n", (int)remembered_applies(a, 20000, 20000, &calls, kNoTree));
    printf("no_levels %d\n", (int)remembered_applies(a, 20000, 20000, &calls, kNoLevels));
    printf("switch_calls %d\n", calls);

    // ---- the box: extents 1, 2 and 4 from (10, 20, 30); 2 % of the extent per face (the values are exact in float32)
    const float box[6] = {10, 20, 30, 11, 22, 34};
    printf("box_same %d\n", (int)same_box(box, box));
    for (int f = 0; f < 6; ++f) {
        const float ext = (float)(1 << (f % 3));
        for (int side = -1; side <= 1; side += 2) {
            float at[6], beyond[6];
            for (int i = 0; i < 6; ++i) at[i] = beyond[i] = box[i];
            at[f] = box[f] + side * 0.015625f * ext;           // 1/64 = 1.5625 %: inside
            beyond[f] = box[f] + side * 0.03125f * ext;        // 1/32 = 3.125 %: outside
            printf("box_in_%d_%d %d\nbox_out_%d_%d %d\n", f, side + 1, (int)same_box(at, box), f, side + 1, (int)same_box(beyond, box));
        }
    }
    // exactly 2 % off, and one float32 step beyond: extent 100 from 0, tolerance 0.02f * 100
    const float wide[6] = {0, 0, 0, 100, 100, 100};
    float edge[6] = {0, 0, 0, 100, 100, 100}, past[6] = {0, 0, 0, 100, 100, 100};
    edge[0] = -(0.02f * 100.0f + 1e-30f);
    past[0] = nextafterf(edge[0], -1000.0f);
    printf("box_at_2pc %d\nbox_past_2pc %d\n", (int)same_box(edge, wide), (int)same_box(past, wide));
    // a degenerate box of zero extent: the tolerance is 1e-30
    const float dot[6] = {1, 1, 1, 1, 1, 1};
    float dot2[6] = {1, 1, 1, 1, 1, 1}, tiny0[6] = {0, 0, 0, 0, 0, 0}, tiny1[6] = {1e-30f, 0, 0, 0, 0, 0}, tiny2[6] = {2e-30f, 0, 0, 0, 0, 0};
    printf("dot_same %d\n", (int)same_box(dot2, dot));
    dot2[4] = nextafterf(1.0f, 2.0f);
    printf("dot_moved %d\n", (int)same_box(dot2, dot));
    printf("tiny_in %d\ntiny_out %d\n", (int)same_box(tiny1, tiny0), (int)same_box(tiny2, tiny0));

    // ---- the give-up
    printf("give_up_16383 %d\n", (int)may_give_up(a, 16383, kOff));
    printf("give_up_16384 %d\n", (int)may_give_up(a, 16384, kOff));
    printf("give_up_exact %d\n", (int)may_give_up(req(PCT_KNN_GRID_EXACT, true, true), 16384, kOff));
    printf("give_up_not_auto %d\n", (int)may_give_up(req(PCT_KNN_GRID, false, true), 16384, kOff));
    printf("give_up_not_tree_ok %d\n", (int)may_give_up(req(PCT_KNN_GRID, true, false), 16384, kOff));
    printf("give_up_no_tree %d\n", (int)may_give_up(a, 16384, kNoTree));
    printf("give_up_no_levels %d\n", (int)may_give_up(a, 16384, kNoLevels));

    // ---- the skew gate
    printf("gate_65535 %d\n", (int)skew_gate(a, true, 65535, 100, kOff));
    printf("gate_65536 %d\n", (int)skew_gate(a, true, 65536, 100, kOff));
    printf("gate_2p29_less %d\n", (int)skew_gate(a, true, ((int64_t)1 << 29) - 1, 100, kOff));
    printf("gate_2p29 %d\n", (int)skew_gate(a, true, (int64_t)1 << 29, 100, kOff));
    printf("gate_shard %d\n", (int)skew_gate(a, false, 65536, 100, kOff));
    printf("gate_no_cells %d\n", (int)skew_gate(a, true, 65536, 0, kOff));
    printf("gate_not_auto %d\n", (int)skew_gate(req(PCT_KNN_GRID, false, true), true, 65536, 100, kOff));
    printf("gate_exact %d\n", (int)skew_gate(req(PCT_KNN_GRID_EXACT, true, true), true, 65536, 100, kOff));
    printf("gate_tree_not_ok %d\n", (int)skew_gate(req(PCT_KNN_GRID, true, false), true, (int64_t)1 << 26, 100, kOff));
    printf("gate_no_tree %d\n", (int)skew_gate(a, true, 65536, 100, kNoTree));
    printf("gate_no_levels %d\n", (int)skew_gate(a, true, 65536, 100, kNoLevels));
    // skew = occupancy * non-empty cells / n: 40 * 2048 / 65536 = 1.25, 48 * 2048 / 65536 = 1.5 (exact)
    printf("skew_125 %.17g\nskew_15 %.17g\n", cell_skew(40.0, 2048, 65536), cell_skew(48.0, 2048, 65536));
    printf("skew_min_tree %.17g\nskew_min_chain %.17g\n", skew_min(true), skew_min(false));
    printf("passes_125_tree %d\npasses_125_up_tree %d\n", (int)(cell_skew(40.0, 2048, 65536) > skew_min(true)), (int)(cell_skew(40.0 + 1e-9, 2048, 65536) > skew_min(true)));
    printf("passes_15_chain %d\npasses_15_up_chain %d\n", (int)(cell_skew(48.0, 2048, 65536) > skew_min(false)), (int)(cell_skew(48.0 + 1e-9, 2048, 65536) > skew_min(false)));
    printf("passes_14_chain %d\n", (int)(cell_skew(45.0, 2048, 65536) > skew_min(false)));

    // ---- the census {queries, overflow, short, cells of the others}; 12 cells per fine query unless said otherwise
    // n = 100 000: fail_min = 37500 / n = 0.375 (1000 queries: 375 fail, 625 fine)
    census("tree_at_0375", 1000, 200, 175, 625 * 12, 100000, true);
    census("tree_past_0375", 1000, 200, 176, 624 * 12, 100000, true);
    // n = 468 750: 37500 / n = 0.08 exactly
    census("tree_at_008", 1000, 50, 30, 920 * 12, 468750, true);
    census("tree_past_008", 1000, 50, 31, 919 * 12, 468750, true);
    // n = 1 000 000: 37500 / n = 0.0375, 0.08 takes over
    census("tree_big_at_008", 1000, 80, 0, 920 * 12, 1000000, true);
    census("tree_big_past_008", 1000, 81, 0, 919 * 12, 1000000, true);
    census("tree_big_0079", 1000, 79, 0, 921 * 12, 1000000, true);
    // cells per fine query: 14.9 and 15 (1000 queries, 500 fine)
    census("tree_cells_149", 1000, 500, 0, 7450, 100000, true);
    census("tree_cells_15", 1000, 500, 0, 7500, 100000, true);
    census("chain_cells_149", 1000, 500, 0, 7450, 100000, false);
    census("chain_cells_15", 1000, 500, 0, 7500, 100000, false);
    // the chain: fail > 0.30 and fine > 0.02 q
    census("chain_at_030", 1000, 300, 0, 700 * 12, 100000, false);
    census("chain_past_030", 1000, 301, 0, 699 * 12, 100000, false);
    census("chain_fine_at_002", 1000, 980, 0, 20 * 12, 100000, false);
    census("chain_fine_past_002", 1000, 979, 0, 21 * 12, 100000, false);
    census("chain_short_counts", 1000, 0, 301, 699 * 12, 100000, false);
    // what sends a call to the tree does not send it down the chain, and the reverse
    census("chain_at_tree_share", 1000, 100, 0, 900 * 12, 1000000, false);
    census("tree_no_fine_left", 1000, 1000, 0, 0, 100000, true);
    census("empty_tree", 0, 0, 0, 0, 100000, true);
    census("empty_chain", 0, 0, 0, 0, 100000, false);
    const unsigned long long none[4] = {0, 0, 0, 0};
    const CensusShares s = census_shares(none);
    printf("empty_q %.17g\nempty_fail %.17g\nempty_fine %.17g\nempty_cells %.17g\n", s.q, s.fail, s.fine, s.cells);
    return 0;
}
"""

STAY, TREE, LEVELS = 0, 1, 2                     # Route
AUTO, BRUTE, GRID, GRID_EXACT, GRID_LEVELS, KNN_TREE = range(6)     # pct_knn_algo (include/pct_hip.h)
UNKNOWN, SLAB = 1, 2                             # Refusal


def resolved(algo, auto_req, tree_ok, refusal=0):
    return refusal * 1000 + algo * 100 + auto_req * 10 + tree_ok


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("auto_route")
    src, exe = d / "route.cpp", d / "route"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe), "-lm"], check=True)
    text = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {k: float(v) for k, v in (ln.split() for ln in text.splitlines())}


def test_header_includes_the_c_library_and_the_public_header_only():
    with open(os.path.join(CSRC, "pct_auto_route.h")) as f:
        includes = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert sorted(includes) == ['"../../include/pct_hip.h"', "<math.h>", "<stdint.h>"]
    with open(os.path.join(ROOT, "include", "pct_hip.h")) as f:
        assert [ln.split()[1] for ln in f if ln.startswith("#include")] == ["<stdint.h>"]


def test_auto_resolves_by_cloud_size(out):
    assert out["auto_4095"] == resolved(BRUTE, 1, 1) and out["auto_4096"] == resolved(GRID, 1, 1)


def test_long_rows_take_the_exact_sweep_and_end_auto(out):
    assert out["auto_k127"] == resolved(GRID, 1, 1) and out["auto_k128"] == resolved(GRID_EXACT, 0, 1)
    assert out["auto_small_k128"] == resolved(BRUTE, 0, 1)           # below 4096 points AUTO is the exhaustive sweep: it stays
    assert out["grid_k127"] == resolved(GRID, 0, 1) and out["grid_k128"] == resolved(GRID_EXACT, 0, 1)
    assert out["brute_k127"] == resolved(BRUTE, 0, 1) and out["brute_k128"] == resolved(BRUTE, 0, 1)
    assert out["tree_k128"] == resolved(GRID_EXACT, 0, 1)


def test_explicit_requests_and_unknown_ones(out):
    assert out["levels"] == resolved(GRID_LEVELS, 0, 1) and out["tree"] == resolved(KNN_TREE, 0, 1)
    assert out["unknown_6"] == resolved(6, 0, 1, UNKNOWN)
    assert out["unknown_neg"] == UNKNOWN * 1000 - 100 + 1


def test_tree_takes_whole_clouds_below_2_to_26(out):
    assert out["shard"] == resolved(GRID, 0, 0)
    assert out["n_2p26_less"] == resolved(GRID, 0, 1) and out["n_2p26"] == resolved(GRID, 0, 0)


def test_slab_allows_the_fused_cell_list_only(out):
    assert out["slab_auto_fused"] == resolved(GRID, 0, 1)             # (AUTO no longer chooses: one cell list over the slab)
    assert out["slab_grid_fused"] == resolved(GRID, 0, 1) and out["slab_exact_fused"] == resolved(GRID_EXACT, 0, 1)
    assert out["slab_auto_k128_fused"] == resolved(GRID_EXACT, 0, 1)
    assert out["slab_grid_stepwise"] == resolved(GRID, 0, 1, SLAB)
    assert out["slab_brute_fused"] == resolved(BRUTE, 0, 1, SLAB)
    assert out["slab_levels_fused"] == resolved(GRID_LEVELS, 0, 1, SLAB) and out["slab_tree_fused"] == resolved(KNN_TREE, 0, 1, SLAB)


def test_remembered_verdict_is_re_examined_every_16th_call(out):
    for i in range(1, 33):
        assert out[f"cadence_{i}"] == (0 if i in (16, 32) else 1), i
    assert out["cadence_calls"] == 32


def test_cadence_counts_only_calls_that_could_use_the_verdict(out):
    assert out["other_n"] == 0 and out["never_remembered"] == 0 and out["not_auto"] == 0 and out["not_tree_ok"] == 0
    assert out["still_calls"] == 0
    assert out["no_tree"] == 0 and out["no_levels"] == 0              # each switch ends it ...
    assert out["switch_calls"] == 2                                   # ... after the call was counted


def test_box_matches_within_2_percent_of_the_extent_per_face(out):
    assert out["box_same"] == 1
    for f in range(6):
        for side in (0, 2):
            assert out[f"box_in_{f}_{side}"] == 1 and out[f"box_out_{f}_{side}"] == 0, (f, side)
    assert out["box_at_2pc"] == 1 and out["box_past_2pc"] == 0


def test_box_of_zero_extent(out):
    assert out["dot_same"] == 1 and out["dot_moved"] == 0
    assert out["tiny_in"] == 1 and out["tiny_out"] == 0               # the 1e-30 of the tolerance


def test_give_up(out):
    assert out["give_up_16383"] == 0 and out["give_up_16384"] == 1
    assert out["give_up_exact"] == 0 and out["give_up_not_auto"] == 0 and out["give_up_not_tree_ok"] == 0
    assert out["give_up_no_tree"] == 0 and out["give_up_no_levels"] == 0


def test_skew_gate(out):
    assert out["gate_65535"] == 0 and out["gate_65536"] == 1
    assert out["gate_2p29_less"] == 1 and out["gate_2p29"] == 0
    assert out["gate_shard"] == 0 and out["gate_no_cells"] == 0 and out["gate_not_auto"] == 0 and out["gate_exact"] == 0
    assert out["gate_tree_not_ok"] == 1                               # (the chain of cell lists is still there to go to)
    assert out["gate_no_tree"] == 1 and out["gate_no_levels"] == 0    # PCT_NO_TREE leaves the chain reachable


def test_skew_thresholds_are_strict(out):
    assert out["skew_125"] == 1.25 and out["skew_15"] == 1.5
    assert out["skew_min_tree"] == 1.25 and out["skew_min_chain"] == 1.5
    assert out["passes_125_tree"] == 0 and out["passes_125_up_tree"] == 1
    assert out["passes_15_chain"] == 0 and out["passes_15_up_chain"] == 1 and out["passes_14_chain"] == 0


def test_census_sends_to_the_tree_above_the_predicted_share(out):
    assert out["tree_at_0375"] == STAY and out["tree_past_0375"] == TREE          # n = 100 000: 0.375
    assert out["tree_at_008"] == STAY and out["tree_past_008"] == TREE            # n = 468 750: 0.08 on both sides of the max
    assert out["tree_big_at_008"] == STAY and out["tree_big_past_008"] == TREE and out["tree_big_0079"] == STAY
    assert out["tree_cells_149"] == TREE and out["tree_cells_15"] == STAY


def test_census_sends_down_the_chain_by_its_own_thresholds(out):
    assert out["chain_cells_149"] == LEVELS and out["chain_cells_15"] == STAY
    assert out["chain_at_030"] == STAY and out["chain_past_030"] == LEVELS
    assert out["chain_fine_at_002"] == STAY and out["chain_fine_past_002"] == LEVELS
    assert out["chain_short_counts"] == LEVELS                                    # short stencils fail like overflowing ones
    assert out["chain_at_tree_share"] == STAY
    assert out["tree_no_fine_left"] == STAY                                       # no fine query: 27 cells assumed


def test_census_of_nothing_stays(out):
    assert out["empty_tree"] == STAY and out["empty_chain"] == STAY
    assert (out["empty_q"], out["empty_fail"], out["empty_fine"], out["empty_cells"]) == (1.0, 0.0, 0.0, 27.0)

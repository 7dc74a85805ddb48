"""The library's table of resident results (csrc/pct_residents.h) against the header's state rules and tests/call_model.py, on the CPU.

A stand-alone program that includes nothing but that header prints, for every event, the residents it drops; for every
`leave`, the residents it replaces (the one left and what was derived from it); three short histories of a handle; and the
rows and the order the table records for the fit through a fourth.
The expected sets are written out by hand from the sentences of include/pct_hip.h, and each is then held equal to the
`drops` of every operation of `call_model.OPS` that stands for it -- the mapping is written out below, one line per operation."""
import os
import shutil
import subprocess

import pytest

import call_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "point-cloud-toolbox_amd", "csrc")

PROGRAM = r"""
#include "pct_residents.h"
#include <stdio.h>

static void show(const char* what, uint32_t set) {
    printf("%s:", what);
    for (int b = 0; b < kPctResidents; ++b)
        if (set >> b & 1) printf(" %s", kPctResidentNames[b]);
    printf("\n");
}
static void show_handle(const char* what, const pct_residents& r) {
    show(what, r.live);
    printf("%s.cell_order: %d\n", what, (int)r.any_in_cell_order());
}

int main() {
    show("names", kPctEveryResident);
    show("drop new_cloud", PCT_NEW_CLOUD.set);
    show("drop ownership", PCT_OWNERSHIP.set);
    show("drop planting", PCT_PLANTING.set);
    show("drop table_lost", PCT_TABLE_LOST.set);
    show("drop table_and_fit_lost", PCT_TABLE_AND_FIT_LOST.set);
    show("drop unfinished_table", PCT_UNFINISHED_TABLE.set);
    for (int b = 0; b < kPctResidents; ++b) {          // a handle that holds everything: what is gone after leave(r), r itself made anew
        pct_residents all;
        all.live = kPctEveryResident;
        all.leave((pct_resident)(1u << b), false, 1);
        char what[64];
        snprintf(what, sizeof(what), "leave %s", kPctResidentNames[b]);
        show(what, (kPctEveryResident & ~all.live) | 1u << b);
        if (!all.has((pct_resident)(1u << b))) printf("leave %s does not leave it\n", kPctResidentNames[b]);
    }

    pct_residents h;                                   // pct_curvature, pct_point_frames, pct_orient_frames, then pct_fit
    h.leave(PCT_R_TABLE, true, 10);
    h.leave(PCT_R_FIT, true, 10);
    h.leave(PCT_R_FRAMES, true, 10);
    h.leave(PCT_R_ORIENT, false, 10);
    show_handle("oriented", h);
    h.leave(PCT_R_FIT, true, 10);
    show_handle("fit_again", h);

    pct_residents g;                                   // everything in place, then pct_point_frames again
    g.live = kPctEveryResident;
    g.leave(PCT_R_FRAMES, false, 10);
    show_handle("frames_again", g);

    pct_residents a;                                   // pct_knn through a cell list, pct_point_areas, pct_voxel_downsample, a new planting by the exhaustive sweep
    a.leave(PCT_R_TABLE, true, 10);
    a.leave(PCT_R_AREAS, true, 10);
    a.leave(PCT_R_BALL, false, 10);
    show_handle("areas_by_row", a);
    a.drop(PCT_TABLE_LOST);
    show_handle("table_lost", a);
    a.drop(PCT_PLANTING);
    show_handle("planted", a);
    a.leave(PCT_R_TABLE, false, 10);
    show_handle("brute_table", a);

    pct_residents f;                                   // a fit in table-row order, a planting, a fit of seven caller rows
    f.leave(PCT_R_FIT, true, 100);
    printf("fit_by_row: %lld %d\n", (long long)f.rows_of(PCT_R_FIT), (int)f.in_row_order(PCT_R_FIT));
    f.drop(PCT_PLANTING);
    printf("fit_dropped: %lld %d\n", (long long)f.rows_of(PCT_R_FIT), (int)f.in_row_order(PCT_R_FIT));
    f.leave(PCT_R_FIT, false, 7);
    printf("fit_public: %lld %d\n", (long long)f.rows_of(PCT_R_FIT), (int)f.in_row_order(PCT_R_FIT));
    return 0;
}
"""

ALL = {"table", "fit", "areas", "frames", "orient", "triangles", "pca", "ball", "holes"}
PER_ROW = {"table", "fit", "areas", "frames", "orient", "triangles", "holes"}
# by the header: "A new cloud ... drops every result on the handle"; "Ownership ... drop what is computed per owned row: the
# table, the fit results, the areas, the frames and the orientation, and the triangles"; "Plantings ... drop the table in
# place, the fit results, the areas, the frames and the orientation, and the triangles"; "pct_voxel_downsample ... drop the
# table and nothing else"; "pct_pca_curvatures leaves no readable table ... and no fit"; "pct_selftest_sweep drops every result on
# the handle, as a new cloud does" (an entry the model excludes: call_model.EXCLUDED)
DROPS = {"new_cloud": ALL, "ownership": PER_ROW, "planting": PER_ROW, "table_lost": {"table"}, "table_and_fit_lost": {"table", "fit"},
         "unfinished_table": ALL}
# "Fits ... replace the fit results and drop the frames and the orientation"; "pct_point_areas replaces the areas and touches
# nothing else"; "pct_point_frames replaces the frames, drops the orientation and touches nothing else"; "pct_orient_frames
# ... replaces the orientation"; "pct_point_triangles replaces the fans and triangles and touches nothing else"; and by
# include/pct_hip_holes.h: "Whatever drops the triangles ... drops them, and so does a new pct_point_triangles";
# "pct_fill_holes touches nothing else on the handle"
LEAVES = {"table": {"table"}, "fit": {"fit", "frames", "orient"}, "areas": {"areas"}, "frames": {"frames", "orient"}, "orient": {"orient"},
          "triangles": {"triangles", "holes"}, "pca": {"pca"}, "ball": {"ball"}, "holes": {"holes"}}
# operation of call_model.OPS -> the events and leaves one successful call of it goes through in the library
STANDS_FOR = {
    "set_points_f32": ("drop new_cloud",),
    "set_points_f64": ("drop new_cloud",),
    "set_points_device": ("drop new_cloud",),
    "use_points_device": ("drop new_cloud",),
    "set_query_range": ("drop ownership",),
    "set_query_slab": ("drop ownership",),
    "knn": ("drop planting", "leave table"),
    "curvature": ("drop planting", "leave table", "leave fit"),
    "surface_variation": ("drop planting", "leave table"),
    "pca_curvatures": ("leave pca", "drop planting", "leave table", "drop table_and_fit_lost"),
    "fit": ("leave fit",),
    "fit_indices": ("leave fit",),
    "fit_ball": ("leave fit",),
    "point_areas": ("leave areas",),
    "point_frames": ("leave frames",),
    "point_triangles": ("leave triangles",),
    "fill_holes": ("leave holes",),
    "query_ball": ("leave ball",),
    "voxel_downsample": ("drop table_lost",),
    "voxel_downsample_f32": ("drop table_lost",),
}


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("residents")
    src, exe = d / "residents.cpp", d / "residents"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    text = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {k: v.split() for k, v in (ln.split(":") for ln in text.splitlines())}


def test_header_includes_stdint_only():
    with open(os.path.join(CSRC, "pct_residents.h")) as f:
        assert [ln.split()[1] for ln in f if ln.startswith("#include")] == ["<stdint.h>"]


def test_residents_are_the_models_in_its_order(out):
    assert tuple(out["names"]) == tuple(r for r in M.RESIDENTS if r != "slab_pass")


def test_every_event_drops_what_the_header_says(out):
    assert {k[5:]: set(v) for k, v in out.items() if k.startswith("drop ")} == DROPS


def test_the_sweep_self_test_drops_what_a_new_cloud_drops(out):
    """pct_selftest_sweep leaves an unfinished table: the header says what it drops, the model excludes it with that reason"""
    assert out["drop unfinished_table"] == out["drop new_cloud"]
    with open(os.path.join(ROOT, "include", "pct_hip.h")) as f:
        header = " ".join(" ".join(ln.strip(" */") for ln in f).split())
    assert "pct_selftest_sweep drops every result on the handle, as a new cloud does" in header
    assert "drops every result" in M.EXCLUDED["pct_selftest_sweep"] and "pct_selftest_sweep" not in M.modelled_entry_points()


def test_every_leave_replaces_what_was_derived_from_it(out):
    assert {k[6:]: set(v) for k, v in out.items() if k.startswith("leave ")} == LEAVES


def test_the_model_drops_the_same_sets():
    """(by hand against the model: the same comparison the next test makes against the program's output)"""
    expected = {**{"drop " + k: v for k, v in DROPS.items()}, **{"leave " + k: v for k, v in LEAVES.items()}}
    for name, steps in STANDS_FOR.items():
        assert set(M.OPS[name].drops) - {"slab_pass"} == set().union(*(expected[s] for s in steps)), name


def test_every_operation_that_drops_stands_for_an_event(out):
    assert {n for n, op in M.OPS.items() if op.drops} == set(STANDS_FOR)
    for name, steps in STANDS_FOR.items():
        assert set(M.OPS[name].drops) - {"slab_pass"} == set().union(*(set(out[s]) for s in steps)), name
    # pct_orient_frames replaces the orientation alone: the model chains its calls and drops nothing
    assert M.OPS["orient_frames"].drops == () and out["leave orient"] == ["orient"]


def test_a_fit_over_frames_and_an_orientation_leaves_neither(out):
    assert set(out["oriented"]) == {"table", "fit", "frames", "orient"}
    assert set(out["fit_again"]) == {"table", "fit"}


def test_frames_again_drop_the_orientation_and_nothing_else(out):
    assert set(out["frames_again"]) == ALL - {"orient"}


def test_rows_and_order_leave_with_the_result(out):
    """What a flag beside the table allowed: the order of a dropped fit read as that of the next."""
    assert out["fit_by_row"] == ["100", "1"]
    assert out["fit_dropped"] == ["0", "0"]
    assert out["fit_public"] == ["7", "0"]


def test_nothing_is_in_cell_order_once_the_only_row_ordered_resident_is_dropped(out):
    assert set(out["areas_by_row"]) == {"table", "areas", "ball"} and out["areas_by_row.cell_order"] == ["1"]
    assert set(out["table_lost"]) == {"areas", "ball"} and out["table_lost.cell_order"] == ["1"]        # (the areas outlive the table)
    assert set(out["planted"]) == {"ball"} and out["planted.cell_order"] == ["0"]
    assert set(out["brute_table"]) == {"table", "ball"} and out["brute_table.cell_order"] == ["0"]
    assert out["oriented.cell_order"] == ["1"] and out["frames_again.cell_order"] == ["0"]

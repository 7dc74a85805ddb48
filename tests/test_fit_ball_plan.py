"""The rules of pct_fit_ball (csrc/pct_fit_ball_plan.h), on the CPU: the class of a row by its member count, the pitch of
the short rows' table, the refusal of a table past its byte budget and the PCT_FIT_BALL_ROUTE knob.  A stand-alone program
that includes nothing but that header (which includes nothing), compiled with -fsanitize=undefined as the other plan tests
are: the products rows x pitch x 4 at 2^31 - 1 members and 2^30 rows must not overflow."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "point-cloud-toolbox_amd", "csrc")

PROGRAM = r"""
#include "pct_fit_ball_plan.h"
#include <stdio.h>

int main() {
    const int S = kBallFitShortMax;
    printf("short_max %d\n", S);
    printf("budget %lld\n", kBallFitTableBudget);
    printf("table %d\nwave %d\n", (int)kBallFitTable, (int)kBallFitWave);
    const long long members[8] = {0, 1, S, S + 1, 511, 512, 2147483647ll, 2};
    for (int i = 0; i < 8; ++i) {
        printf("class_allowed_%d %d\n", i, ball_fit_class(members[i], S, true));
        printf("class_refused_%d %d\n", i, ball_fit_class(members[i], S, false));
    }
    const int pitches[6] = {1, 3, 4, 32, 63, 130};
    for (int i = 0; i < 6; ++i) printf("pitch_%d %d\n", pitches[i], ball_fit_pitch(pitches[i]));
    printf("pitch_default %d\n", ball_fit_pitch(S));
    const long long at = kBallFitTableBudget / (4ll * ball_fit_pitch(S));
    printf("rows_at_budget %lld\n", at);
    printf("bytes_at %lld\n", ball_fit_table_bytes(at, S));
    printf("allowed_at %d\nallowed_above %d\n", (int)ball_fit_table_allowed(at, S, kBallFitAuto), (int)ball_fit_table_allowed(at + 1, S, kBallFitAuto));
    printf("allowed_none %d\n", (int)ball_fit_table_allowed(0, S, kBallFitAuto));
    printf("allowed_huge %d\n", (int)ball_fit_table_allowed(1ll << 30, 255, kBallFitAuto));
    printf("bytes_huge %lld\n", ball_fit_table_bytes(1ll << 30, 255));
    printf("wave_small %d\n", (int)ball_fit_table_allowed(1, S, kBallFitWaveOnly));
    printf("table_above %d\n", (int)ball_fit_table_allowed(at + 1, S, kBallFitTableFirst));
    printf("table_none %d\n", (int)ball_fit_table_allowed(0, S, kBallFitTableFirst));
    const char* words[8] = {"wave", "table", "", "wav", "waves", "Table", "tabl", "auto"};
    for (int i = 0; i < 8; ++i) printf("knob_%d %d\n", i, ball_fit_knob(words[i]));
    printf("knob_null %d\n", ball_fit_knob((const char*)0));
    return 0;
}
"""

AUTO, WAVE_ONLY, TABLE_FIRST = 0, 1, 2


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("fit_ball_plan")
    src, exe = d / "fit_ball_plan.cpp", d / "fit_ball_plan"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                    str(src), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=0"))
    assert run.returncode == 0, run.stderr[-2000:]
    assert "runtime error" not in run.stderr, run.stderr[-2000:]
    return {k: int(v) for k, v in (ln.split() for ln in run.stdout.splitlines())}


def test_header_includes_nothing():
    with open(os.path.join(CSRC, "pct_fit_ball_plan.h")) as f:
        assert not [ln for ln in f if ln.lstrip().startswith("#include")]


def test_class_boundaries(plan):
    table, wave = plan["table"], plan["wave"]
    assert table != wave and plan["short_max"] == 64
    # members 0, 1 (no fit: with the wave kernel's list) | kBallFitShortMax | kBallFitShortMax + 1, 511, 512, 2^31 - 1 | 2
    assert [plan[f"class_allowed_{i}"] for i in range(8)] == [wave, wave, table, wave, wave, wave, wave, table]
    assert all(plan[f"class_refused_{i}"] == wave for i in range(8))          # no table: the wave kernel takes any length


def test_pitch(plan):
    assert [plan[f"pitch_{s}"] for s in (1, 3, 4, 32, 63, 130)] == [4, 4, 4, 32, 64, 132]
    assert plan["pitch_default"] == 64 and plan["pitch_default"] >= plan["short_max"] and plan["pitch_default"] % 4 == 0


def test_budget_refusal(plan):
    assert plan["budget"] == 256 << 20
    assert plan["rows_at_budget"] == 1 << 20 and plan["bytes_at"] == plan["budget"]
    assert plan["allowed_at"] == 1 and plan["allowed_above"] == 0              # bytes <= budget, inclusive
    assert plan["allowed_none"] == 0
    assert plan["bytes_huge"] == (1 << 30) * 256 * 4 and plan["allowed_huge"] == 0


def test_knob(plan):
    assert [plan[f"knob_{i}"] for i in range(8)] == [WAVE_ONLY, TABLE_FIRST, AUTO, AUTO, AUTO, AUTO, AUTO, AUTO]
    assert plan["knob_null"] == AUTO
    assert plan["wave_small"] == 0                    # `wave`: never a table
    assert plan["table_above"] == 1                   # `table`: the budget does not refuse
    assert plan["table_none"] == 0                    # ... but no rows, no table

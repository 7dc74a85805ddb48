// The pure rules of pct_fit_ball (pct_fit_ball.hip): which of the two fits takes a CSR row, the pitch of the short rows'
// table, and when that table is refused.  Nothing here knows a handle or a device, and nothing is included: the kernels
// evaluate the same functions, tests/test_fit_ball_plan.py compiles this header alone with the host compiler.
#pragma once

#if defined(__HIPCC__)
#define BFP_HD __host__ __device__
#else
#define BFP_HD
#endif

// ---- the two routes -------------------------------------------------------------------------------------------------------
// Wave:  k_fit_ball, one wave per row, any length -- 64 lanes stride the members, 27 fp64 sums cross the wave.
// Table: the members of a row copied into one row of a (rows, pitch) table (k_ball_table) and fitted by k_fit, one thread
//        per row: what a wave is mostly idle on.
// A row's class goes by its MEMBERS (the entries other than the centre's own index).  Rows of fewer than two members have
// no fit (NaN): they go with the wave kernel's list, from where the SVD kernel writes the NaN, so that
// pct_timings.fit_svd_rows counts every row that was not solved by the normal equations.
// kBallFitShortMax is measured (1 M-point torus, 262 144 rows, fit time): rows of ~18 members 0.768 | 0.702 |
// 0.735 ms at 32 | 64 | 128, rows of ~213 members 1.649 | 1.655 | 1.915 ms; the wave kernel alone 1.693 ms on the short rows.
constexpr int kBallFitShortMax = 64;

enum BallFitKnob { kBallFitAuto = 0, kBallFitWaveOnly = 1, kBallFitTableFirst = 2 };
enum BallFitClass { kBallFitTable = 0, kBallFitWave = 1 };

// PCT_FIT_BALL_ROUTE=wave|table (read per call, like PCT_FIT_JACOBI): `wave` sends every row to k_fit_ball; `table` sends
// every row within the pitch to the table even where the byte budget below would refuse it (A/B runs).  Anything else,
// unset included: the measured rule.
BFP_HD inline int ball_fit_knob(const char* e) {
    if (!e) return kBallFitAuto;
    const char* w = "wave";
    const char* t = "table";
    int i = 0;
    while (w[i] && e[i] == w[i]) ++i;
    if (!w[i] && !e[i]) return kBallFitWaveOnly;
    i = 0;
    while (t[i] && e[i] == t[i]) ++i;
    if (!t[i] && !e[i]) return kBallFitTableFirst;
    return kBallFitAuto;
}

// table row pitch in elements: rows are 16-byte aligned (k_fit stages them as int4)
BFP_HD inline int ball_fit_pitch(int short_max) { return (short_max + 3) & ~3; }

// ---- the refusal ----------------------------------------------------------------------------------------------------------
// The table holds a row for EVERY row of the query (rows that go to the wave kernel read count 0 there: k_fit's outputs are
// row-aligned and one launch covers them), so it costs rows x pitch x 4 bytes whatever the rows hold.  Beyond the budget no
// table is built and every row goes to the wave kernel, which takes any length: 256 MiB is 1 M rows at the default pitch.
constexpr long long kBallFitTableBudget = 256ll << 20;
BFP_HD inline long long ball_fit_table_bytes(long long rows, int short_max) { return rows * (long long)ball_fit_pitch(short_max) * 4ll; }
BFP_HD inline bool ball_fit_table_allowed(long long rows, int short_max, int knob) {
    if (knob == kBallFitWaveOnly || rows <= 0) return false;
    if (knob == kBallFitTableFirst) return true;
    return ball_fit_table_bytes(rows, short_max) <= kBallFitTableBudget;
}

// ---- the class of a row ---------------------------------------------------------------------------------------------------
// members: 0 .. 2^31 - 1 (a row never holds more entries than the cloud has points)
BFP_HD inline int ball_fit_class(long long members, int short_max, bool table_allowed) {
    return table_allowed && members >= 2 && members <= (long long)short_max ? kBallFitTable : kBallFitWave;
}

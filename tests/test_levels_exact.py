"""The pass planning of the chained sweep (csrc/pct_levels_plan.h) against its NumPy restatement (tests/levels_exact.py), on the CPU.

A stand-alone program that includes nothing but that header reads cases as bit patterns and prints what the header's
functions answer, again as bit patterns; everything is compared bit for bit, with one exception.  The population step
of classify goes through log2f, the one library function in the rule: the restatement takes the logarithm in float64 and
rounds it to float32, and the header's value must follow -- exactly, through the halving, the clamp and the float
addition -- from that float32 or one of its two neighbours (the 1 ulp HIP documents for log2f; the host's log2f is held
to the same).  Cases whose float64 step lies within 1e-4 of a clamp are left out by the generator, fewer than 1 % of them.

Values no pass can produce -- classify adds a bounded step to a finite log2 edge, halves a finite sum or answers
kWantExact -- are kept as documented behaviour: bin_of clamps them into bin 0 or bin 159 (the conversion of the scaled
offset to int is out of range for them; whatever it gives, the correcting loops walk to the clamped bin), and the strip
[0.4e30, 0.5e30) is counted in bin 159 and owned by no window.  The invariant `window members == hist[b .. b + 3]` is
asserted over the values a pass can produce, and the strip is asserted to be the only place it breaks."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import levels_exact as lx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "point-cloud-toolbox_amd", "csrc")
F = np.float32

PROGRAM = r"""
#include "pct_levels_plan.h"
#include <stdio.h>
#include <string.h>
#include <vector>

static float f_of(unsigned u) { float f; memcpy(&f, &u, 4); return f; }
static unsigned u_of(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
static unsigned long long u_of(double d) { unsigned long long u; memcpy(&u, &d, 8); return u; }

int main() {
    char cmd[8];
    while (scanf("%7s", cmd) == 1) {
        if (cmd[0] == 'K') {               // the constants
            printf("K %d %u %u %u %u %u %d %d\n", kBins, u_of(kBinLo), u_of(kWantExact), u_of(kStepMax), u_of(kStepMin), u_of(kBracketMin),
                   kMaxPasses, kWindowBins);
        } else if (cmd[0] == 'E') {        // enough(nq)
            long long nq;
            if (scanf("%lld", &nq) != 1) return 2;
            printf("E %lld\n", (long long)levels_enough(nq));
        } else if (cmd[0] == 'B') {        // log_edge0, n values: bounds, bin of every value, members of every window
            unsigned le, n;
            if (scanf("%u %u", &le, &n) != 2) return 2;
            const float le0 = f_of(le);
            std::vector<float> w(n);
            for (unsigned i = 0; i < n; ++i) { unsigned u; if (scanf("%u", &u) != 1) return 2; w[i] = f_of(u); }
            printf("B");
            for (int b = 0; b <= kBins; ++b) printf(" %u", u_of(bin_lo(le0, b)));
            printf("\nb");
            for (unsigned i = 0; i < n; ++i) printf(" %d", bin_of(w[i], le0));
            printf("\nw");
            for (int b = 0; b + kWindowBins <= kBins; ++b) {
                const float lo = window_lo(le0, b), hi = window_hi(le0, b);
                unsigned c = 0;
                for (unsigned i = 0; i < n; ++i) c += in_window(w[i], lo, hi);
                printf(" %u %u %u", u_of(lo), u_of(hi), c);
            }
            printf("\n");
        } else if (cmd[0] == 'C') {        // n cases of classify
            unsigned n;
            if (scanf("%u", &n) != 1) return 2;
            for (unsigned i = 0; i < n; ++i) {
                int why; unsigned pop, le, tg, bx, by;
                if (scanf("%d %u %u %u %u %u", &why, &pop, &le, &tg, &bx, &by) != 6) return 2;
                // the population as k_classify takes it out of the row's word
                const unsigned e = (unsigned)why << 29 | pop;
                const LevelWant r = classify((int)(e >> 29), (float)(e & 0x1FFFFFFFu), f_of(le), f_of(tg), LevelBracket{f_of(bx), f_of(by)});
                printf("C %u %u %u\n", u_of(r.want), u_of(r.bracket.x), u_of(r.bracket.y));
            }
        } else if (cmd[0] == 'N') {        // passes, nq, log_edge0, exact, 160 bins
            int passes; long long nq; unsigned le, exact, hist[kBins];
            if (scanf("%d %lld %u %u", &passes, &nq, &le, &exact) != 4) return 2;
            for (int b = 0; b < kBins; ++b) if (scanf("%u", &hist[b]) != 1) return 2;
            const NextPass p = next_pass(hist, exact, passes, nq, f_of(le));
            printf("N %lld %lld %d %lld %d %u %u %llu %llu\n", (long long)p.pending, (long long)p.banded, p.best, (long long)p.best_cnt, (int)p.stop,
                   u_of(p.lo), u_of(p.hi), u_of(p.edge), u_of(closing_edge(hist, f_of(le))));
        } else return 3;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("levels_plan")
    src, exe = d / "plan.cpp", d / "plan"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe), "-lm"], check=True)

    def run(text):
        out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout
        return [ln.split() for ln in out.splitlines()]
    return run


def u64_of(x):
    return int(np.float64(x).view(np.uint64))


def test_header_includes_the_c_library_only():
    with open(os.path.join(CSRC, "pct_levels_plan.h")) as f:
        includes = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert sorted(includes) == ["<math.h>", "<stdint.h>"]


def test_constants(program):
    (k,) = program("K\n")
    assert [int(x) for x in k[1:]] == [lx.K_BINS, *(int(lx.bits(v)) for v in (lx.K_BIN_LO, lx.K_WANT_EXACT, lx.K_STEP_MAX, lx.K_STEP_MIN, lx.K_BRACKET_MIN)),
                                       lx.K_MAX_PASSES, lx.K_WINDOW]
    assert (lx.K_BINS, float(lx.K_BIN_LO), lx.K_MAX_PASSES) == (160, -20.0, 14)
    nqs = [0, 1, 1024 * 256 - 1, 1024 * 256, 1024 * 256 + 255, 1025 * 256, 1 << 29]
    assert [int(r[1]) for r in program("".join(f"E {n}\n" for n in nqs))] == [1024, 1024, 1024, 1024, 1024, 1025, 1 << 21]
    assert [lx.enough(n) for n in nqs] == [1024, 1024, 1024, 1024, 1024, 1025, 1 << 21]


@pytest.fixture(scope="module")
def bins(program):
    """Per log_edge0: (values, the header's bounds, bins, windows [(lo, hi, members)])."""
    text, vals = "", []
    for le0 in lx.LOG_EDGE0:
        v = lx.boundary_values(le0)
        vals.append(v)
        text += f"B {int(lx.bits(le0))} {len(v)} " + " ".join(str(int(u)) for u in lx.bits(v)) + "\n"
    out = program(text)
    got = []
    for i, v in enumerate(vals):
        B, b, w = out[3 * i:3 * i + 3]
        assert (B[0], b[0], w[0]) == ("B", "b", "w")
        win = np.array(w[1:], dtype=np.uint64).reshape(-1, 3)
        got.append((v, np.array(B[1:], dtype=np.uint32), np.array(b[1:], dtype=np.int64), win))
    return got


def test_the_list_of_first_edges_rounds_and_does_not():
    """Some bounds of the list are inexact sums (they differ from the float64 sum), the dyadic ones are exact throughout."""
    inexact = [bool((lx.bounds(le0).astype(np.float64) != float(le0) - 20.0 + 0.25 * np.arange(161)).any()) for le0 in lx.LOG_EDGE0]
    # (log2(1e-20) - 20 stays inside one binade with its bounds below -64: exact; kept for its magnitude)
    assert inexact == [True, True, False, True, True] + [False] * 5
    for name in (0.0371, 1.0 / 3.0, 1e-20):
        assert F(np.log2(name)) in lx.LOG_EDGE0


def test_bin_lo_at_every_bound(bins):
    for le0, (_, B, _, _) in zip(lx.LOG_EDGE0, bins):
        assert np.array_equal(B, lx.bits(lx.bounds(le0))), le0


def test_bin_of_at_every_boundary(bins):
    """Each value's bin is the bin whose [bin_lo(b), bin_lo(b + 1)) holds it, the clamp outside; NaN -1, the exact class 160."""
    for le0, (v, _, b, _) in zip(lx.LOG_EDGE0, bins):
        assert np.array_equal(b, lx.bin_of(v, le0)), le0
        e = lx.bounds(le0)
        inner = (b >= 0) & (b < lx.K_BINS) & (v >= e[0]) & (v < e[lx.K_BINS])
        assert inner.sum() >= 3 * 159 and (e[b[inner]] <= v[inner]).all() and (v[inner] < e[b[inner] + 1]).all()
        # a bound is the first value of its bin, its lower neighbour the last of the bin before
        assert np.array_equal(b[1:3 * 160:3], np.arange(160)) and np.array_equal(b[3:3 * 161:3], np.arange(160))
        assert b[0] == 0 and b[3 * 160 + 1] == 159 and b[3 * 160 + 2] == 159        # the clamp on both sides
        far = dict(zip([int(u) for u in lx.bits(np.array(lx.FAR_VALUES))], b[3 * 161:]))
        look = lambda x: far[int(lx.bits(F(x)))]
        assert look(-np.inf) == look(-3.0e38) == look(-200.0) == 0 and look(200.0) == look(1.0e29) == look(0.45e30) == 159
        assert look(lx.WINDOW_TOP) == 159 and look(np.nextafter(lx.EXACT_FROM, F(0))) == 159
        assert look(lx.EXACT_FROM) == look(lx.K_WANT_EXACT) == look(np.inf) == 160 and b[-1] == -1 and np.isnan(v[-1])


def test_every_window_owns_what_the_histogram_counts(bins):
    """For every window start the values with lo <= w < hi are hist[b .. b + 3]: the invariant that once broke at a bin
    boundary.  Over the values a pass can produce it holds everywhere; over all values it breaks in the last window only,
    by exactly the values of the strip [0.4e30, 0.5e30)."""
    for le0, (v, _, _, win) in zip(lx.LOG_EDGE0, bins):
        ok = lx.reachable(v)
        assert ok.sum() >= 3 * 161 + 8 and (~ok).sum() >= 6
        hist_ok, _ = lx.histogram(v[ok], le0)
        hist_all, exact_all = lx.histogram(v, le0)
        strip = int(((v >= lx.WINDOW_TOP) & (v < lx.EXACT_FROM)).sum())
        assert strip == 4 and exact_all == 5          # (of FAR_VALUES)
        assert len(win) == 157
        for b, (lo_u, hi_u, members) in enumerate(win):
            lo, hi = lx.window(le0, b)
            assert (int(lo_u), int(hi_u)) == (int(lx.bits(lo)), int(lx.bits(hi))), (le0, b)
            assert int(members) == int(lx.members(v, lo, hi).sum()), (le0, b)
            assert int(lx.members(v[ok], lo, hi).sum()) == int(hist_ok[b:b + 4].sum()), (le0, b)
            assert int(members) == int(hist_all[b:b + 4].sum()) - (strip if b == 156 else 0), (le0, b)
        assert lx.window(le0, 0)[0] == -np.inf and lx.window(le0, 156)[1] == lx.WINDOW_TOP


@pytest.fixture(scope="module")
def classified(program):
    cases, generated, dropped = lx.classify_cases()
    text = f"C {len(cases['why'])}\n" + "".join(
        f"{w} {p} {le} {t} {x} {y}\n" for w, p, le, t, x, y in zip(cases["why"], cases["pop"], lx.bits(cases["log_edge"]), lx.bits(cases["target"]),
                                                                    lx.bits(cases["bx"]), lx.bits(cases["by"])))
    got = np.array([r[1:] for r in program(text)], dtype=np.uint32)
    return cases, generated, dropped, lx.from_bits(got[:, 0]), lx.from_bits(got[:, 1]), lx.from_bits(got[:, 2])


def test_the_generator_leaves_out_few_cases(classified):
    cases, generated, dropped, *_ = classified
    assert generated >= 20000 and dropped < 0.01 * generated, (generated, dropped)
    assert len(cases["why"]) == generated - dropped
    print(f"classify cases: {generated} generated, {dropped} within {lx.CLAMP_MARGIN} of a clamp left out")


def check_classify(cases, want, bx, by):
    """Asserts everything but the population step bit for bit, that step within the three-value allowance; returns
    (rows through the logarithm, rows of those that differ from the nearest value)."""
    ref = [lx.classify(cases["why"], cases["pop"], cases["log_edge"], cases["target"], cases["bx"], cases["by"], s) for s in (0, -1, 1)]
    w0, x0, y0, took_log = ref[0]
    assert np.array_equal(lx.bits(bx), lx.bits(x0)) and np.array_equal(lx.bits(by), lx.bits(y0))
    assert np.array_equal(lx.bits(want[~took_log]), lx.bits(w0[~took_log]))
    allowed = np.stack([lx.bits(r[0]) for r in ref])
    inside = (lx.bits(want)[None, :] == allowed).any(axis=0)
    assert inside[took_log].all(), [(k, v[took_log & ~inside][:5]) for k, v in cases.items()]
    return int(took_log.sum()), int((lx.bits(want) != allowed[0])[took_log].sum())


def test_classify_over_the_product(classified):
    cases, _, _, want, bx, by = classified
    n_log, off = check_classify(cases, want, bx, by)
    print(f"classify: {len(want)} cases, {n_log} through log2f, {off} of them not the nearest float32 of the float64 logarithm")
    assert n_log >= 3000


def test_classify_reaches_every_branch(classified):
    """The restatement's own census of the product: every branch of the rule, each clamp from inside and from far beyond."""
    cases, _, _, want, bx, by = classified
    w0, _, _, took_log = lx.classify(cases["why"], cases["pop"], cases["log_edge"], cases["target"], cases["bx"], cases["by"])
    exact = w0 == lx.K_WANT_EXACT
    for why in range(8):
        sel = cases["why"] == why
        assert sel.sum() >= 1000 and (exact[sel].all() if why not in (1, 2) else (~exact[sel]).any())
    unchanged = (lx.bits(bx) == lx.bits(cases["bx"])) & (lx.bits(by) == lx.bits(cases["by"]))
    assert unchanged[~np.isin(cases["why"], (1, 2))].all() and (~unchanged).sum() > 1000
    step = lx.step64(cases["pop"], cases["target"])
    moved = (w0 - cases["log_edge"]).astype(np.float64)
    for why, sign in ((1, 1.0), (2, -1.0)):
        t = took_log & (cases["why"] == why)
        s = sign * step[t]
        assert (s < 0).any() and ((s > 0) & (s < 0.75)).any() and ((s > 0.76) & (s < 2.9)).any() and (s > 4).any()
        assert (sign * moved[t] >= 0.75 - 2e-6).all() and (sign * moved[t] <= 3 + 2e-6).all()
    closed = ~took_log & ~exact
    width = (by - bx).astype(np.float64)
    assert closed.sum() > 500 and (width[closed] >= float(lx.K_BRACKET_MIN)).all()
    news = ((cases["why"] == 1) & (cases["log_edge"] > cases["bx"])) | ((cases["why"] == 2) & (cases["log_edge"] < cases["by"]))
    narrow = exact & news & np.isfinite(bx) & np.isfinite(by)
    assert ((width[narrow] > 0.5) & (width[narrow] < 0.6)).any() and (width[narrow] < 0).any()
    assert (width[closed] == float(lx.K_BRACKET_MIN)).any() and (bx[narrow] > by[narrow]).any()


def hist_of(**at):
    h = [0] * 160
    for b, c in at.items():
        h[int(b[1:])] = c
    return h


ENOUGH = 1024               # of nq <= 262 144 + 255
NEXT_CASES = {
    # name: (hist, exact, passes, nq); every one at log_edge0 = log2(0.0371) and at -5
    "all_empty": (hist_of(), 0, 1, 6000),
    "only_exact": (hist_of(), 4711, 1, 6000),
    "tie_lowest_start_wins": (hist_of(b10=2000, b11=1000, b20=3000, b90=3000), 0, 1, 6000),
    "tie_overlapping_windows": (hist_of(b40=5000), 0, 1, 6000),                         # windows 37 .. 40 tie: 37 wins
    "best_at_0": (hist_of(b0=3000, b3=100, b100=2000), 5, 1, 6000),
    "best_at_156": (hist_of(b156=10, b159=3000, b50=2000), 5, 1, 6000),
    "banded_at_enough": (hist_of(b30=ENOUGH), 7, 1, 6000),
    "banded_above_enough": (hist_of(b30=ENOUGH + 1), 7, 1, 6000),
    "best_cnt_at_an_eighth": (hist_of(**{f"b{8 * i}": ENOUGH // 8 for i in range(20)}), 0, 1, 6000),
    "best_cnt_above_an_eighth": (hist_of(**{f"b{8 * i}": ENOUGH // 8 for i in range(20)}, b1=1), 0, 1, 6000),
    "passes_13": (hist_of(b70=5000), 0, 13, 6000),
    "passes_14": (hist_of(b70=5000), 0, 14, 6000),
    # nq / 256 reaches 1024 at 262 144 and exceeds it from 262 400 on: enough stays 1024 across the first, 1025 banded go on ...
    "nq_262143": (hist_of(b70=1024, b75=1), 0, 2, 262143),
    "nq_262144": (hist_of(b70=1024, b75=1), 0, 2, 262144),
    "nq_262399": (hist_of(b70=1024, b75=1), 0, 2, 262399),
    "nq_262400": (hist_of(b70=1024, b75=1), 0, 2, 262400),                              # ... enough = 1025: the same histogram stops
    "median_first_bin": (hist_of(b0=600, b100=300, b159=299), 0, 14, 6000),
    "median_last_bin": (hist_of(b0=299, b100=300, b159=600), 0, 14, 6000),
    "median_exactly_half": (hist_of(b12=500, b80=500), 3, 14, 6000),                    # twice the running sum REACHES the total at bin 12
    "median_one_query": (hist_of(b133=1), 0, 14, 6000),
}
# name: (best, best_cnt, stop, bin of the closing edge or None), written out by hand from the rule
NEXT_EXPECTED = {
    "all_empty": (0, 0, True, None), "only_exact": (0, 0, True, None),
    "tie_lowest_start_wins": (8, 3000, False, 20), "tie_overlapping_windows": (37, 5000, False, 40),
    "best_at_0": (0, 3100, False, 0), "best_at_156": (156, 3010, False, 159),
    "banded_at_enough": (27, 1024, True, 30), "banded_above_enough": (27, 1025, False, 30),
    "best_cnt_at_an_eighth": (0, 128, True, 72), "best_cnt_above_an_eighth": (0, 129, False, 72),
    "passes_13": (67, 5000, False, 70), "passes_14": (67, 5000, True, 70),
    "nq_262143": (67, 1024, False, 70), "nq_262144": (67, 1024, False, 70), "nq_262399": (67, 1024, False, 70), "nq_262400": (67, 1024, True, 70),
    "median_first_bin": (0, 600, True, 0), "median_last_bin": (156, 600, True, 159),
    "median_exactly_half": (9, 500, True, 12), "median_one_query": (130, 1, True, 133),
}


def test_next_pass_and_closing_edge(program):
    assert sorted(NEXT_CASES) == sorted(NEXT_EXPECTED)
    edges = [lx.LOG_EDGE0[0], F(-5.0)]
    names = [(n, le0) for n in NEXT_CASES for le0 in edges]
    text = "".join(f"N {NEXT_CASES[n][2]} {NEXT_CASES[n][3]} {int(lx.bits(le0))} {NEXT_CASES[n][1]} " + " ".join(map(str, NEXT_CASES[n][0])) + "\n"
                   for n, le0 in names)
    for (name, le0), row in zip(names, program(text)):
        hist, exact, passes, nq = NEXT_CASES[name]
        ref = lx.next_pass(hist, exact, passes, nq, le0)
        got = [int(x) for x in row[1:]]
        assert got == [ref["pending"], ref["banded"], ref["best"], ref["best_cnt"], int(ref["stop"]), int(lx.bits(ref["lo"])), int(lx.bits(ref["hi"])),
                       u64_of(ref["edge"]), u64_of(lx.closing_edge(hist, le0))], (name, le0)
        # ... and the restatement against the rule by hand
        best, best_cnt, stop, med = NEXT_EXPECTED[name]
        assert (ref["best"], ref["best_cnt"], ref["stop"]) == (best, best_cnt, stop), name
        assert ref["pending"] == sum(hist) + exact and ref["banded"] == sum(hist)
        # (exp2 is the C library's on both sides; it lies within one ulp of the correctly rounded power of the hand-made argument)
        want_closing = float(le0) if med is None else float(le0) - 20.0 + 0.25 * (med + 0.5)
        for got_edge, arg in ((ref["edge"], float(le0) - 20.0 + 0.25 * (best + 2)), (lx.closing_edge(hist, le0), want_closing)):
            exact_edge = lx.exp2_exact(arg)
            assert np.nextafter(exact_edge, 0.0) <= got_edge <= np.nextafter(exact_edge, np.inf), (name, got_edge, exact_edge)
    # the special bounds
    first, last = lx.next_pass(*NEXT_CASES["best_at_0"], F(-5.0)), lx.next_pass(*NEXT_CASES["best_at_156"], F(-5.0))
    assert first["lo"] == -np.inf and first["hi"] == F(-24.0) and last["lo"] == F(14.0) and last["hi"] == F(0.4) * F(1.0e30)
    assert [lx.enough(n) for n in (262143, 262144, 262399, 262400)] == [1024, 1024, 1024, 1025]

// The pure rule of the density-adaptive sweep (pct_levels.hip): the edge a query wants after a pass that failed it, the
// quarter-octave bin of a wanted edge, the one-octave window the next pass owns, when the chain stops and the edge of the
// closing exact pass.  Nothing here knows a handle, a device or the environment; the kernels evaluate the very same inline
// functions (LP_HD) -- tests/test_levels_exact.py compiles this header alone with the host compiler and holds it to the
// NumPy restatement of tests/levels_exact.py, tests/test_gpu_levels_exact.py holds the kernels to the same restatement.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LP_HD __host__ __device__
#else
#define LP_HD
#endif

#ifndef PCT_LEVEL_STEP_MAX
#define PCT_LEVEL_STEP_MAX 3.f
#endif
constexpr float kStepMax = PCT_LEVEL_STEP_MAX;   // largest jump (octaves of cell edge) taken on the population estimate alone
constexpr float kStepMin = 0.75f;               // ... and the smallest: a failed pass moves its query by at least this
constexpr float kBracketMin = 0.6f;             // a bracket narrower than this (octaves) is not bisected further
constexpr float kWantExact = 1.0e30f;          // wanted-edge value of a query only the exact sweep can answer
constexpr int kBins = 160;                      // histogram of wanted log2 edges, quarter octaves
constexpr float kBinLo = -20.f;                 // relative to the first pass's log2 edge
constexpr int kWindowBins = 4;                  // a pass serves one octave of wanted edges
constexpr int kMaxPasses = 14;

// leftovers of this size go to the exact sweep
inline int64_t levels_enough(int64_t nq) { return nq / 256 > 1024 ? nq / 256 : 1024; }

// ---- the bins ------------------------------------------------------------------------------------------------------------
// lower bound of bin b (= upper bound of bin b - 1): the ONE expression behind the histogram, the window and the box
LP_HD inline float bin_lo(float log_edge0, int b) { return log_edge0 + kBinLo + 0.25f * b; }

// a pending query only the exact sweep can answer (classify's kWantExact)
LP_HD inline bool wants_exact(float w) { return w >= 0.5f * kWantExact; }

// bin of a wanted edge below the exact class: the bin whose float bounds -- the very expressions a window of bins is
// turned into [lo, hi) with -- hold w.  floor() of the scaled offset can land one bin off at a boundary, and a window
// that the histogram says holds 2313 queries then owned none (box [inf, -inf], a launch of no blocks)
LP_HD inline int banded_bin(float w, float log_edge0) {
    int bin = (int)floorf((w - log_edge0 - kBinLo) * 4.f);
    bin = bin < 0 ? 0 : bin >= kBins ? kBins - 1 : bin;
    while (bin > 0 && w < bin_lo(log_edge0, bin)) --bin;
    while (bin < kBins - 1 && w >= bin_lo(log_edge0, bin + 1)) ++bin;
    return bin;
}

// the histogram slot of a wanted edge (k_band_hist): -1 not pending (NaN), kBins the exact class, else its bin
LP_HD inline int bin_of(float w, float log_edge0) { return !(w == w) ? -1 : wants_exact(w) ? kBins : banded_bin(w, log_edge0); }

// [lo, hi) of the window of kWindowBins bins that starts at bin `best`: open below at the first bin, and at the last
// bin up to (not including) the exact class
LP_HD inline float window_lo(float log_edge0, int best) { return best == 0 ? -INFINITY : bin_lo(log_edge0, best); }
LP_HD inline float window_hi(float log_edge0, int best) {
    return best + kWindowBins >= kBins ? 0.4f * kWantExact : bin_lo(log_edge0, best + kWindowBins);
}
LP_HD inline bool in_window(float w, float lo, float hi) { return w >= lo && w < hi; }

// ---- the wanted edge of a row the pass left unanswered -------------------------------------------------------------------
struct LevelBracket { float x, y; };      // log2 of the largest edge known too small, of the smallest known too large
struct LevelWant { float want; LevelBracket bracket; };

// why: 1 these cells were too small for the query, 2 too large; pop: candidates the 27-cell stencil of its item held;
// log_edge: log2 of the pass's cell edge; target: the stencil population of a well-sized pass
LP_HD inline LevelWant classify(int why, float pop, float log_edge, float target, LevelBracket b) {
    float w = kWantExact;
    // a failure that tells nothing new (the pass edge lay outside the bracket already known) ends the search
    const bool news = why == 1 ? log_edge > b.x : why == 2 ? log_edge < b.y : false;
    if (why == 1) b.x = fmaxf(b.x, log_edge);          // these cells were too small for it
    else if (why == 2) b.y = fminf(b.y, log_edge);     // ... too large
    if (news) {
        if (b.x > -INFINITY && b.y < INFINITY) {
            // bisection (log scale); a pass serves a one-octave band, so a bracket much narrower than that cannot
            // be resolved further (volumes: the workable window between "too few" and "overflow" is ~0.2 octaves)
            w = b.y - b.x < kBracketMin ? kWantExact : 0.5f * (b.x + b.y);
        } else {
            // population ~ edge^2 on a surface, ~ edge^3 in a volume: the square root over-shoots in a volume,
            // the bracket then takes over
            const float step = 0.5f * log2f(fmaxf(target / fmaxf(pop, 0.5f), 1e-6f));
            w = why == 1 ? log_edge + fminf(fmaxf(step, kStepMin), kStepMax) : log_edge + fmaxf(fminf(step, -kStepMin), -kStepMax);
        }
    }
    return LevelWant{w, b};
}

// ---- the next pass -------------------------------------------------------------------------------------------------------
struct NextPass {
    int64_t pending, banded;       // queries without an answer; those of them with a wanted edge
    int best;                      // first bin of the one-octave window that holds the most queries (the lowest of equals)
    int64_t best_cnt;
    bool stop;                     // no further banded pass: the exact sweep takes what is pending
    float lo, hi;                  // the pass owns the queries with lo <= want < hi
    double edge;                   // its cell edge: the centre of the window
};

inline NextPass next_pass(const unsigned* hist, unsigned exact, int passes, int64_t nq, float log_edge0) {
    NextPass p = {};
    for (int b = 0; b < kBins; ++b) p.banded += hist[b];
    p.pending = p.banded + exact;
    p.best_cnt = -1;
    for (int b = 0; b + kWindowBins <= kBins; ++b) {
        const int64_t c = (int64_t)hist[b] + hist[b + 1] + hist[b + 2] + hist[b + 3];
        if (c > p.best_cnt) { p.best_cnt = c; p.best = b; }
    }
    const int64_t enough = levels_enough(nq);
    p.stop = p.banded <= enough || passes >= kMaxPasses || p.best_cnt <= enough / 8;
    p.lo = window_lo(log_edge0, p.best);
    p.hi = window_hi(log_edge0, p.best);
    p.edge = exp2((double)log_edge0 + kBinLo + 0.25 * (p.best + 2));
    return p;
}

// cells of the closing exact pass: sized for the median wanted edge of the banded leftovers (the exact sweep widens ring
// by ring), for the first pass's edge when nothing is banded
inline double closing_edge(const unsigned* hist, float log_edge0) {
    int64_t acc = 0, banded = 0;
    for (int b = 0; b < kBins; ++b) banded += hist[b];
    int med = kBins / 2;
    for (int b = 0; b < kBins; ++b) { acc += hist[b]; if (acc * 2 >= banded) { med = b; break; } }
    return banded > 0 ? exp2((double)log_edge0 + kBinLo + 0.25 * (med + 0.5)) : exp2((double)log_edge0);
}

// Consistent normal orientation: a level-synchronous flood over the resident neighbour table that turns the normals of
// pct_point_frames so that neighbouring rows agree (the contract: include/pct_hip.h; tests/orient_exact.py states it again
// in NumPy, and the device is held to it bit for bit).  Every choice is a keyed 64-bit maximum, so the result is a pure
// function of the unoriented normals and the table: no edge sort, no union-find, no dependence on launch or arrival order.
//
// Every per-point array is in PUBLIC order (a whole-cloud handle: public index = owned row), whatever order the table and
// the frames are stored in: k_orient_prep copies the unoriented normals there once and notes every point's table row, and a
// table entry (a position of the sorted space behind a cell list, a public index behind the exhaustive sweep) becomes a
// public index through its record's w.  All tie-breaks use public indices.
//
//   claim    parent p on child c: dot = (n_p0 n_c0 + n_p1 n_c1) + n_p2 n_c2 in float64 (-ffp-contract=off), key =
//            bits((float)|dot|) << 32 | (0xFFFFFFFF - p); atomicMax into claim[c].  0 is no key (p < 2^31), and the lane
//            that finds the word empty appends c to the next list: once per level, so a list never outgrows the row count,
//            and its order shows in no result -- k_orient_resolve decides every listed row from its own word alone.
//   lists    two frontier lists A and B, two lists of unlabelled rows, their lengths in the control words on the device.
//            Level kernels run on a fixed grid and stride over the list; one that finds its list empty returns at once.
//   group    what the host enqueues blind: compact + seed (both act only when a component is to be started), L push
//            levels in pairs A -> B -> A, one pull round (acts only when the pushes ran dry).  Several groups per host
//            wait; the control words come back through pinned memory.
//
// Plain vector code: no inline assembly, no LDS.  A table entry is dereferenced only after it was checked against the record
// count, a public index only after it was checked against the row count, a list slot only below the row count.
#include "pct_internal.h"

#include <math.h>

namespace {

enum OrientWord {                          // int words of the control block (OrientState::ctl), mirrored to pct_pinned::orient_words
    OW_CNT_A = 0, OW_CNT_B, OW_UCNT0, OW_UCNT1, OW_UPAR, OW_SEED_BEST, OW_NCOMP, OW_RUNNING, OW_FINISHED, OW_LEVELS,
    OW_PULLS, OW_LABELLED, OW_VALID, OW_TOGGLED, OW_PUSH_DONE, OW_COUNT
};
static_assert(OW_COUNT <= sizeof(pct_pinned::orient_words) / sizeof(int), "pct_pinned::orient_words");

constexpr int kOrientBlock = 256;
constexpr int kOrientGrid = 1024;          // blocks of a level kernel: 4096 waves stride over the frontier
constexpr int kLevelsDefault = 8;          // push levels per group (even: the pairs end on list A)
constexpr int kGroupsDefault = 4;          // groups per host wait (DESIGN 4.3j has what was measured)

struct OrientState {
    // the table and the cloud, as pct_launch_point_frames reads them
    const float4* pts;
    const double4* ptsd;
    const int* table;
    const int* cnt;                 // eps counts, or null
    const int* owned_pos;           // table row -> record (sorted space), or null: the row itself
    unsigned n_pts;
    int rows, k, pitch;
    int frame_by_row;               // frames stored in table-row order, else public order
    // the frames, turned in place by k_orient_apply
    double* normal;
    double* k12;
    double* dirs;
    unsigned char* flipped;
    // public order, (rows) each
    double* n0;                     // (rows, 3) the unoriented normals; NaN x 3: no valid row
    unsigned long long* claim;
    int* comp;
    int* parent;
    int* level;
    unsigned char* toggle;
    int* rowtab;                    // table row of the public index
    float* z32;
    int* list_a;
    int* list_b;
    int* ulist[2];
    // per component (max_comp)
    unsigned long long* topkey;
    int* away;
    int* toward;
    unsigned char* invert;
    int max_comp;
    int* ctl;
    double vx, vy, vz;
};

__device__ __forceinline__ int lane_of() { return (int)(threadIdx.x & 63u); }

// the slots of the lanes that want one, from one atomicAdd of the wave; every lane of the wave calls it
__device__ __forceinline__ int wave_append(bool want, int* counter) {
    const unsigned long long mask = __ballot(want);
    if (!mask) return -1;
    const int lane = lane_of(), leader = __ffsll((long long)mask) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(counter, (int)__popcll(mask));
    base = __shfl(base, leader);
    return want ? base + (int)__popcll(mask & ((1ull << lane) - 1ull)) : -1;
}

__device__ __forceinline__ int record_of_row(const OrientState& s, int row) { return s.owned_pos ? s.owned_pos[row] : row; }

__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ __forceinline__ unsigned long long claim_key(double dot, int p) {
    return ((unsigned long long)__float_as_uint((float)fabs(dot)) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)p);
}

// ---- one pass over the table rows: everything into public order ----------------------------------------------------------
__global__ __launch_bounds__(kOrientBlock) void k_orient_prep(OrientState s) {
    const int row = (int)(blockIdx.x * kOrientBlock + threadIdx.x);
    bool valid = false;
    int pub = -1;
    if (row < s.rows) {
        const int rec = record_of_row(s, row);
        if ((unsigned)rec < s.n_pts) {
            const float4 q = s.pts[rec];
            pub = __float_as_int(q.w);
            if ((unsigned)pub < (unsigned)s.rows) {
                const double* n = s.normal + (int64_t)(s.frame_by_row ? row : pub) * 3;
                const double a = n[0], b = n[1], c = n[2];
                valid = a == a && b == b && c == c;
                const double nan = (double)__int_as_float(0x7fc00000);
                double* o = s.n0 + (int64_t)pub * 3;
                o[0] = valid ? a : nan;
                o[1] = valid ? b : nan;
                o[2] = valid ? c : nan;
                s.claim[pub] = 0ull;
                s.comp[pub] = s.parent[pub] = s.level[pub] = -1;
                s.toggle[pub] = 0;
                s.rowtab[pub] = row;
                s.z32[pub] = q.z + 0.0f;                   // (-0 -> +0: equal heights, equal bits)
            } else {
                pub = -1;
            }
        }
    }
    const int slot = wave_append(valid, &s.ctl[OW_UCNT0]);
    if (valid && slot < s.rows) s.ulist[0][slot] = pub;
    const unsigned long long vm = __ballot(valid);
    if (lane_of() == 0 && vm) atomicAdd(&s.ctl[OW_VALID], (int)__popcll(vm));
}

// ---- a component is to be started: the rows still unlabelled, compacted, and the lowest of them ---------------------------
__global__ __launch_bounds__(kOrientBlock) void k_orient_compact(OrientState s) {
    if (s.ctl[OW_RUNNING] || s.ctl[OW_FINISHED]) return;
    const int par = s.ctl[OW_UPAR] & 1;
    const int total = min(s.ctl[par ? OW_UCNT1 : OW_UCNT0], s.rows);
    const int* src = s.ulist[par];
    int* dst = s.ulist[par ^ 1];
    int* dst_count = &s.ctl[par ? OW_UCNT0 : OW_UCNT1];
    const int stride = (int)gridDim.x * kOrientBlock;
    for (int base = (int)blockIdx.x * kOrientBlock; base < total; base += stride) {      // (block-uniform trip count)
        const int i = base + (int)threadIdx.x;
        int u = -1;
        bool want = false;
        if (i < total) {
            const int v = src[i];
            if ((unsigned)v < (unsigned)s.rows && s.comp[v] < 0) { want = true; u = v; }
        }
        const int slot = wave_append(want, dst_count);
        if (want && slot < s.rows) dst[slot] = u;
        int best = want ? 0x7fffffff - u : 0;              // the lowest index as a maximum: 0 is no row, what a cleared word holds
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) best = max(best, __shfl_xor(best, d));
        if (lane_of() == 0 && best) atomicMax(&s.ctl[OW_SEED_BEST], best);
    }
}

__global__ void k_orient_seed(OrientState s) {
    int* c = s.ctl;
    if (c[OW_RUNNING] || c[OW_FINISHED]) return;
    const int par = c[OW_UPAR] & 1;
    c[par ? OW_UCNT1 : OW_UCNT0] = 0;                      // the list just read: the next compaction's target
    c[OW_UPAR] = par ^ 1;
    const int seed = c[OW_SEED_BEST] ? 0x7fffffff - c[OW_SEED_BEST] : -1;
    c[OW_SEED_BEST] = 0;
    c[OW_PUSH_DONE] = 0;
    if ((unsigned)seed >= (unsigned)s.rows || c[OW_NCOMP] >= s.max_comp) {
        c[OW_FINISHED] = 1;
        return;
    }
    s.comp[seed] = c[OW_NCOMP]++;
    s.level[seed] = 0;
    s.parent[seed] = -1;
    s.toggle[seed] = 0;
    s.list_a[0] = seed;
    c[OW_CNT_A] = 1;
    c[OW_CNT_B] = 0;
    c[OW_LABELLED] += 1;
    c[OW_RUNNING] = 1;
}

// ---- claims.  PULL = false: the rows of `list` (labelled in the previous level) claim the unlabelled valid members of their
// own rows.  PULL = true, once the pushes ran dry: the rows of the compacted list of unlabelled rows (which of the two, the
// control words say) claim for themselves, from the members of their own rows that carry the running component's id.
// One wave per listed row, one lane per table entry.
template <bool PULL>
__global__ __launch_bounds__(kOrientBlock) void k_orient_claim(OrientState s, const int* __restrict__ list, int count_word,
                                                               int* __restrict__ out, int out_word) {
    const int* c = s.ctl;
    if (c[OW_FINISHED] || !c[OW_RUNNING]) return;
    if (PULL) {
        if (!c[OW_PUSH_DONE]) return;
        const int par = c[OW_UPAR] & 1;
        list = s.ulist[par];
        count_word = par ? OW_UCNT1 : OW_UCNT0;
    }
    const int total = min(c[count_word], s.rows);
    if (total <= 0) return;
    const int cid = c[OW_NCOMP] - 1;
    const int lane = lane_of();
    const int waves = (int)gridDim.x * (kOrientBlock / 64);
    for (int e = (int)blockIdx.x * (kOrientBlock / 64) + (int)(threadIdx.x >> 6); e < total; e += waves) {     // (wave-uniform)
        const int me = list[e];
        if ((unsigned)me >= (unsigned)s.rows) continue;
        if (PULL && s.comp[me] >= 0) continue;
        const int row = s.rowtab[me];
        int m = s.cnt ? s.cnt[row] : s.k;
        m = max(0, min(m, s.k));
        const double* nm = s.n0 + (int64_t)me * 3;
        const double mine[3] = {nm[0], nm[1], nm[2]};
        const int* entries = s.table + (int64_t)row * s.pitch;
        for (int j0 = 0; j0 < m; j0 += 64) {
            const int j = j0 + lane;
            bool fresh = false;
            int child = -1;
            if (j < m) {
                const int pos = entries[j];
                if ((unsigned)pos < s.n_pts) {
                    const int other = __float_as_int(s.pts[pos].w);
                    if ((unsigned)other < (unsigned)s.rows) {
                        const int oc = s.comp[other];
                        if (PULL ? oc == cid : oc < 0) {
                            const double* no = s.n0 + (int64_t)other * 3;
                            const double theirs[3] = {no[0], no[1], no[2]};
                            if (theirs[0] == theirs[0]) {                       // (a valid row: prep writes NaN x 3 or none)
                                const int p = PULL ? other : me;
                                child = PULL ? me : other;
                                const double dot = PULL ? dot3(theirs, mine) : dot3(mine, theirs);
                                fresh = atomicMax(&s.claim[child], claim_key(dot, p)) == 0ull;
                            }
                        }
                    }
                }
            }
            const int slot = wave_append(fresh, &s.ctl[out_word]);
            if (fresh && slot < s.rows) out[slot] = child;
        }
    }
}

// ---- every listed row takes its winner.  after_pull: the list is what the pull round labelled (or the pull did not run);
// its bookkeeping is k_orient_book's.  A push level's bookkeeping is done here by one thread: it writes words no thread of
// this launch reads.
__global__ __launch_bounds__(kOrientBlock) void k_orient_resolve(OrientState s, const int* __restrict__ list, int count_word,
                                                                 int other_word, int after_pull) {
    int* c = s.ctl;
    if (c[OW_FINISHED] || !c[OW_RUNNING]) return;
    if (after_pull && !c[OW_PUSH_DONE]) return;            // no pull round in this group: list A is the running frontier
    const int total = min(c[count_word], s.rows);
    const int stride = (int)gridDim.x * kOrientBlock;
    for (int i = (int)(blockIdx.x * kOrientBlock + threadIdx.x); i < total; i += stride) {
        const int child = list[i];
        if ((unsigned)child >= (unsigned)s.rows) continue;
        const unsigned long long key = s.claim[child];
        const int p = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
        if (key == 0ull || (unsigned)p >= (unsigned)s.rows) continue;
        const double* np_ = s.n0 + (int64_t)p * 3;
        const double* nc = s.n0 + (int64_t)child * 3;
        const double a[3] = {np_[0], np_[1], np_[2]}, b[3] = {nc[0], nc[1], nc[2]};
        s.toggle[child] = (unsigned char)(s.toggle[p] ^ (dot3(a, b) < 0.0 ? 1 : 0));
        s.comp[child] = s.comp[p];
        s.parent[child] = p;
        s.level[child] = s.level[p] + 1;
        s.claim[child] = 0ull;
    }
    if (!after_pull && blockIdx.x == 0 && threadIdx.x == 0) {
        if (total > 0) { c[OW_LEVELS] += 1; c[OW_LABELLED] += total; }
        c[other_word] = 0;                                 // the list this level read: the next level's target
        if (count_word == OW_CNT_A) c[OW_PUSH_DONE] = total == 0 ? 1 : 0;
    }
}

// the bookkeeping of a pull round, after its resolve: a launch of its own, since the resolve's threads read what it writes
__global__ void k_orient_book(OrientState s) {
    int* c = s.ctl;
    if (c[OW_FINISHED] || !c[OW_RUNNING] || !c[OW_PUSH_DONE]) return;
    const int total = min(c[OW_CNT_A], s.rows);
    c[OW_PUSH_DONE] = 0;
    if (total == 0) { c[OW_RUNNING] = 0; return; }         // the component is complete
    c[OW_PULLS] += 1;
    c[OW_LABELLED] += total;
}

// ---- the anchor ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned ordered_bits(float z) {
    const unsigned u = __float_as_uint(z);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <bool F64>
__global__ __launch_bounds__(kOrientBlock) void k_orient_anchor(OrientState s, int anchor) {
    const int i = (int)(blockIdx.x * kOrientBlock + threadIdx.x);
    const int cid = i < s.rows ? s.comp[i] : -1;
    const bool live = cid >= 0 && cid < s.max_comp;
    const int first = __shfl(cid, 0);
    const bool uniform = __ballot(cid == first) == __ballot(true) && first >= 0 && first < s.max_comp;
    if (anchor == PCT_ORIENT_TOP) {
        unsigned long long key = live ? ((unsigned long long)ordered_bits(s.z32[i]) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i) : 0ull;
        if (uniform) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const unsigned long long o = __shfl_xor(key, d);
                key = o > key ? o : key;
            }
            if (lane_of() == 0) atomicMax(&s.topkey[first], key);
        } else if (live) {
            atomicMax(&s.topkey[cid], key);
        }
        return;
    }
    bool is_away = false, is_toward = false;
    if (live) {
        const int rec = record_of_row(s, s.rowtab[i]);
        double px = 0, py = 0, pz = 0;
        if ((unsigned)rec < s.n_pts) {
            if (F64) { const double4 q = s.ptsd[rec]; px = q.x; py = q.y; pz = q.z; }
            else { const float4 q = s.pts[rec]; px = (double)q.x; py = (double)q.y; pz = (double)q.z; }
        }
        const double* n = s.n0 + (int64_t)i * 3;
        const double sg = s.toggle[i] ? -1.0 : 1.0;
        const double side = ((s.vx - px) * (sg * n[0]) + (s.vy - py) * (sg * n[1])) + (s.vz - pz) * (sg * n[2]);
        is_away = side < 0.0;
        is_toward = side > 0.0;
    }
    const unsigned long long am = __ballot(is_away), tm = __ballot(is_toward);
    if (uniform) {
        if (lane_of() == 0) {
            if (am) atomicAdd(&s.away[first], (int)__popcll(am));
            if (tm) atomicAdd(&s.toward[first], (int)__popcll(tm));
        }
    } else if (live) {
        if (is_away) atomicAdd(&s.away[cid], 1);
        if (is_toward) atomicAdd(&s.toward[cid], 1);
    }
}

__global__ __launch_bounds__(kOrientBlock) void k_orient_decide(OrientState s, int anchor) {
    const int cid = (int)(blockIdx.x * kOrientBlock + threadIdx.x);
    if (cid >= min(s.ctl[OW_NCOMP], s.max_comp)) return;
    bool inv = false;
    if (anchor == PCT_ORIENT_TOP) {
        const unsigned long long key = s.topkey[cid];
        const int top = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
        if (key != 0ull && (unsigned)top < (unsigned)s.rows) {
            const double nz = s.n0[(int64_t)top * 3 + 2];
            inv = (s.toggle[top] ? -nz : nz) < 0.0;
        }
    } else if (anchor == PCT_ORIENT_VIEW) {
        inv = s.away[cid] > s.toward[cid];
    }
    s.invert[cid] = inv ? 1 : 0;
}

// ---- k_frame's flip on every row whose toggle, after the anchor, is 1 ------------------------------------------------------
__global__ __launch_bounds__(kOrientBlock) void k_orient_apply(OrientState s) {
    const int row = (int)(blockIdx.x * kOrientBlock + threadIdx.x);
    bool turn = false;
    if (row < s.rows) {
        const int rec = record_of_row(s, row);
        const int pub = (unsigned)rec < s.n_pts ? __float_as_int(s.pts[rec].w) : -1;
        if ((unsigned)pub < (unsigned)s.rows) {
            const int cid = s.comp[pub];
            if (cid >= 0 && cid < s.max_comp) {
                turn = (s.toggle[pub] ^ s.invert[cid]) != 0;
                s.toggle[pub] = turn ? 1 : 0;
            }
            if (turn) {
                const int64_t at = s.frame_by_row ? row : pub;
                double* n = s.normal + at * 3;
                double* kk = s.k12 + at * 2;
                double* d = s.dirs + at * 6;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    n[i] = -n[i];
                    const double t = d[2 * i];
                    d[2 * i] = d[2 * i + 1];
                    d[2 * i + 1] = t;
                }
                const double k1 = kk[0];
                kk[0] = -kk[1];
                kk[1] = -k1;
                s.flipped[at] ^= 1;
            }
        }
    }
    const unsigned long long tm = __ballot(turn);
    if (lane_of() == 0 && tm) atomicAdd(&s.ctl[OW_TOGGLED], (int)__popcll(tm));
}

// PCT_ORIENT_LEVELS / PCT_ORIENT_GROUPS (read per call), clamped
int env_int(const char* v, int fallback, int lo, int hi) {
    if (!v || !*v) return fallback;
    const int x = atoi(v);
    return x < lo ? lo : x > hi ? hi : x;
}

}  // namespace

size_t pct_orient_bytes(int64_t rows, int max_comp) {
    const size_t r = (size_t)rows, c = (size_t)max_comp;
    return 256 + r * (3 * sizeof(double) + sizeof(unsigned long long) + 8 * sizeof(int) + sizeof(float)) + ((r + 63) & ~(size_t)63) +
           c * (sizeof(unsigned long long) + 2 * sizeof(int)) + ((c + 63) & ~(size_t)63) + 64;
}

// The flood, the anchor and the apply pass on the resident frames of a whole-cloud handle.  rep->stats = {valid rows,
// components, rows left unlabelled, toggled rows, levels, pull rounds, kernel launches, host waits}: the last two from
// here, the others from the control words (pct_orient_report), which are on their way to pinned memory on return.
int pct_run_orient(pct_ctx* ctx, int anchor, const double* viewpoint, int max_comp, pct_stage_report* rep) {
    const int64_t rows64 = ctx->q_end - ctx->q_begin;
    const int rows = (int)rows64;
    const bool sorted = ctx->knn_sorted_space;
    if (max_comp > rows) max_comp = rows;
    PCT_TRY(pct_reserve(ctx, &ctx->orient, pct_orient_bytes(rows64, max_comp)));
    OrientState s = {};
    s.pts = (const float4*)(sorted ? ctx->sorted4.p : ctx->pts4.p);
    s.ptsd = ctx->has_f64 ? (const double4*)(sorted ? ctx->sorted4d.p : ctx->pts4d.p) : nullptr;
    s.n_pts = (unsigned)(sorted ? ctx->n_grid : ctx->n);
    s.table = (const int*)ctx->nbr_pos.p;
    s.cnt = ctx->eps > 0 ? (const int*)ctx->nbr_cnt.p : nullptr;
    s.owned_pos = sorted ? (const int*)ctx->owned_pos.p : nullptr;
    s.rows = rows;
    s.k = ctx->k;
    s.pitch = ctx->nbr_pitch;
    s.frame_by_row = ctx->res.in_row_order(PCT_R_FRAMES) ? 1 : 0;
    s.normal = (double*)ctx->frame.p;
    s.k12 = s.normal + rows64 * 3;
    s.dirs = s.k12 + rows64 * 2;
    s.flipped = (unsigned char*)ctx->frame_flip.p + 64;
    // the carve-up of ctx->orient: 8-byte arrays first
    char* at = (char*)ctx->orient.p;
    s.ctl = (int*)at;                       at += 256;
    s.n0 = (double*)at;                     at += (size_t)rows * 3 * sizeof(double);
    s.claim = (unsigned long long*)at;      at += (size_t)rows * sizeof(unsigned long long);
    s.topkey = (unsigned long long*)at;     at += (size_t)max_comp * sizeof(unsigned long long);
    s.comp = (int*)at;                      at += (size_t)rows * sizeof(int);
    s.parent = (int*)at;                    at += (size_t)rows * sizeof(int);
    s.level = (int*)at;                     at += (size_t)rows * sizeof(int);
    s.rowtab = (int*)at;                    at += (size_t)rows * sizeof(int);
    s.list_a = (int*)at;                    at += (size_t)rows * sizeof(int);
    s.list_b = (int*)at;                    at += (size_t)rows * sizeof(int);
    s.ulist[0] = (int*)at;                  at += (size_t)rows * sizeof(int);
    s.ulist[1] = (int*)at;                  at += (size_t)rows * sizeof(int);
    s.z32 = (float*)at;                     at += (size_t)rows * sizeof(float);
    s.away = (int*)at;                      at += (size_t)max_comp * sizeof(int);
    s.toward = (int*)at;                    at += (size_t)max_comp * sizeof(int);
    s.toggle = (unsigned char*)at;          at += ((size_t)rows + 63) & ~(size_t)63;
    s.invert = (unsigned char*)at;
    s.max_comp = max_comp;
    if (viewpoint) { s.vx = viewpoint[0]; s.vy = viewpoint[1]; s.vz = viewpoint[2]; }
    ctx->orient_comp = s.comp;
    ctx->orient_parent = s.parent;
    ctx->orient_level = s.level;
    ctx->orient_toggle = s.toggle;

    const int levels = env_int(pct_getenv("PCT_ORIENT_LEVELS"), kLevelsDefault, 2, 64) & ~1;
    const int groups = env_int(pct_getenv("PCT_ORIENT_GROUPS"), kGroupsDefault, 1, 64);
    const hipStream_t st = ctx->stream;
    int64_t launches = 0, waits = 0;
    const int* pin = ctx->pin->orient_words;

    PCT_HIP(ctx, hipMemsetAsync(s.ctl, 0, 256, st));       // every word's cleared state is its initial state
    PCT_HIP(ctx, hipMemsetAsync(s.topkey, 0, (size_t)max_comp * sizeof(unsigned long long), st));
    PCT_HIP(ctx, hipMemsetAsync(s.away, 0, (size_t)max_comp * 2 * sizeof(int), st));
    PCT_HIP(ctx, hipMemsetAsync(s.invert, 0, (size_t)max_comp, st));
    const dim3 per_row((unsigned)((rows + kOrientBlock - 1) / kOrientBlock)), block(kOrientBlock), grid(kOrientGrid);
    PCT_LAUNCH(k_orient_prep, per_row, block, 0, st, s);
    ++launches;

    const auto level = [&](const int* from, int from_word, int* to, int to_word) {
        PCT_LAUNCH(k_orient_claim<false>, grid, block, 0, st, s, from, from_word, to, to_word);
        PCT_LAUNCH(k_orient_resolve, grid, block, 0, st, s, (const int*)to, to_word, from_word, 0);
        launches += 2;
    };
    // a batch that neither labels a row nor ends a component does not exist while the flood runs, so rows + components
    // batches end it whatever the table holds; the bound only keeps a broken device from holding the host for ever
    const int64_t max_batches = 2 * (int64_t)rows + 4;
    bool finished = false;
    for (int64_t batch = 0; batch < max_batches && !finished; ++batch) {
        for (int g = 0; g < groups; ++g) {
            PCT_LAUNCH(k_orient_compact, grid, block, 0, st, s);
            PCT_LAUNCH(k_orient_seed, dim3(1), dim3(1), 0, st, s);
            for (int l = 0; l < levels; l += 2) {
                level(s.list_a, OW_CNT_A, s.list_b, OW_CNT_B);
                level(s.list_b, OW_CNT_B, s.list_a, OW_CNT_A);
            }
            PCT_LAUNCH(k_orient_claim<true>, grid, block, 0, st, s, (const int*)nullptr, 0, s.list_a, OW_CNT_A);
            PCT_LAUNCH(k_orient_resolve, grid, block, 0, st, s, (const int*)s.list_a, OW_CNT_A, OW_CNT_B, 1);
            PCT_LAUNCH(k_orient_book, dim3(1), dim3(1), 0, st, s);
            launches += 5;
        }
        PCT_HIP(ctx, hipGetLastError());
        PCT_HIP(ctx, hipMemcpyAsync(ctx->pin->orient_words, s.ctl, 16 * sizeof(int), hipMemcpyDeviceToHost, st));
        PCT_HIP(ctx, hipStreamSynchronize(st));
        ++waits;
        finished = pin[OW_FINISHED] != 0;
    }
    if (!finished) return pct_fail(ctx, PCT_ERR_INVALID, "pct_orient_frames: the flood did not end");

    if (anchor != PCT_ORIENT_SEED) {
        if (ctx->has_f64) PCT_LAUNCH(k_orient_anchor<true>, per_row, block, 0, st, s, anchor);
        else PCT_LAUNCH(k_orient_anchor<false>, per_row, block, 0, st, s, anchor);
        PCT_LAUNCH(k_orient_decide, dim3((unsigned)((max_comp + kOrientBlock - 1) / kOrientBlock)), block, 0, st, s, anchor);
        launches += 2;
    }
    PCT_LAUNCH(k_orient_apply, per_row, block, 0, st, s);
    ++launches;
    PCT_HIP(ctx, hipGetLastError());
    PCT_HIP(ctx, hipMemcpyAsync(ctx->pin->orient_words, s.ctl, 16 * sizeof(int), hipMemcpyDeviceToHost, st));
    rep->stats[6] = launches;
    rep->stats[7] = waits + 1;                             // (the caller's wait for the apply pass and the events)
    return PCT_OK;
}

void pct_orient_report(pct_ctx* ctx, pct_stage_report* rep) {
    const int* w = ctx->pin->orient_words;
    const int64_t st[6] = {w[OW_VALID], w[OW_NCOMP], (int64_t)w[OW_VALID] - w[OW_LABELLED], w[OW_TOGGLED], w[OW_LEVELS], w[OW_PULLS]};
    for (int i = 0; i < 6; ++i) rep->stats[i] = st[i];
}

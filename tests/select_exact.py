"""What the fast neighbour sweeps (k_knn_pair, k_knn_duo, k_knn_fast) must do with every row -- store it as final, hand it to
the exact sweep, mark it as trusted -- restated from their proofs in NumPy.  Nothing here imports the package.

The grid, the cell of every point and the stencil populations are grid_exact.build's; the guarantee is
tree_exact.guaranteed_r2.  tests/test_gpu_select.py holds the device to the classes below (pct_selftest_sweep: the planned
sweep alone, no exact sweep behind it) and tests/test_select_exact.py holds this module to brute force and to itself.
The rules, quoted:

  candidates  "The 27-cell stencil is staged once into LDS": the float32 records of the up to 27 cells of the grid around the
              query's cell; "fp64 ((dx^2 + dy^2) + dz^2) (no FMA: SciPy's value)" from the query -- "the float32 record
              widened, or (Q64) the native coordinates".
  keys        pct_knn_item.h: "key = floor(d2 * scale), KEY_BITS wide"; scale = (double)(1u << KEY_BITS) / (kKeyRange * edge *
              edge), kKeyRange = 2.3; "min((unsigned)(d2a * scale), key_max - 1u)", key_max = (1u << KEY_BITS) - 1u; KEY_BITS =
              32 - SLOT_BITS, the slot bits of the kernel that runs (constants(), read from the kernels' sources).
  guarantee   make_key_setup: "g2 = fmin(guaranteed_r2(G, cx, cy, cz, gx, gy, gz, 1), limit_r2(...))" (limit_r2 = +inf for a
              handle that holds the whole cloud); "my_gkey = g2 == INFINITY ? 0xFFFFFFFFu : (unsigned)fmin(g2 * s.scale,
              4294967294.0)" -- "floor() keeps it conservative"; gx = (q - o) * inv_cell - cx with the query the keys measure
              from.
  eps         "eps_key = ... (unsigned)fmin(ceil(eps2 * s.scale), 4294967295.0)"; an element is real where "d2a < eps2"
              (strict), padding otherwise.
  proof       "tau = readlane(e, k): the (k+1)-th nearest (padding if fewer exist)"; "need_k = min(tau == kPadElem ?
              0xFFFFFFFFu : tk + 1u, eps_key)"; "amb = need_k > min(g, bkey) || (tau != kPadElem && tk >= key_max - 1u)": the
              row goes to the redo list.  bkey ("exact keys of the candidates the pre-selection cut are >= bkey") is
              0xFFFFFFFF where nothing was cut: "need = tot > LIST" -- with at most LIST candidates (inside the eps ball as the
              pre-selection bounds it, eps2 (1 + 2^-18) in float32) there is no threshold search.
  overflow    item_overflows: "m > cap" (grid_exact.stage_cap): every row of the item is on the redo list and none is trusted
              ("a list of a truncated stencil is the set of nothing").
  threshold   "k+1 <= #(d < T) <= LIST for each query"; "no float left between: a pile of equal distances" -- "no threshold:
              nothing passes, the list is all padding and the row stored below starts with -1".
  equal keys  "equal keys among the first k+2 entries: ordered here by the exact values (order_equal_keys)", which gives up
              on a run it cannot hold: runs of up to 34 equal keys are pinned to finish (tests/test_gpu_sort_net.py).
  trusted     "the (k+1)-th entry exists, its key is below every key the pre-selection cut (bkey) and below the saturated one,
              and entry k+1 does not share it": "Entries 0 .. k are then every candidate of the stencil with a key up to entry
              k's".

From these, per owned row, three classes that do not depend on the threshold T the device happens to find (its secant step
goes through v_rcp_f32 and starts from the previous query's T: a row can fall either way from run to run):

  must_redo   the item overflows; or need > gkey; or the (k+1)-th key is saturated; or no threshold exists -- decided only
              for piles of bit-identical records, whose members share one float32 distance whatever the arithmetic: fewer than
              k+1 candidates can lie below the pile and more than LIST lie at or below it.  The device's (k+1)-th key is
              taken among the survivors, a subset of the stencil: it is never below the stencil's, so each of these
              conditions on the stencil's list holds on the device's.
  must_final  not must_redo, not undecided, at most LIST candidates in the stencil (with eps: within eps^2 (1 + 2^-16), and
              for a float64 cloud within (eps + 2 eq)^2 of the native query, eq the query's rounding distance), and no run of
              equal keys that reaches into the first k+2 entries is longer than 34.
  undecided   need and gkey within one key unit of each other, or the guarantee within tree_exact.UNDECIDED_REL of a key
              boundary: left out of both.
"""
import os
import re

import numpy as np

import grid_exact as ge
import tree_exact as te

F32 = np.float32
KEY_RANGE = 2.3
PAD = 0xFFFFFFFF
RUN_MAX = 34                                 # equal-key runs order_equal_keys is pinned to finish (tests/test_gpu_sort_net.py)
FAST, PAIR, DUO = 1, 2, 3                    # pct_timings.sweep_variant, bits 0-1
Q64_BIT = 64

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "point-cloud-toolbox_amd", "csrc")


def constants(family, regs=1, pre=True):
    """(LIST, KEY_BITS) of the kernel a case runs, read from its source."""
    def text(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()
    if family in (PAIR, DUO):
        m = re.search(r"LIST = (\d+), SLOT_BITS = (\d+), KEY_BITS = 32 - SLOT_BITS;", text("pct_knn_pair.hip" if family == PAIR else "pct_knn_duo.hip"))
        assert m, "the kernel's constants moved"
        return int(m.group(1)), 32 - int(m.group(2))
    src = text("pct_knn_fast.hip")
    m = re.search(r"SLOT_BITS = PRE \? \(R == 1 \? (\d+) : (\d+)\) : \(R == 1 \? (\d+) : (\d+)\);", src)
    assert m and "constexpr int LIST = 64 * R;" in src and "KEY_BITS = 32 - SLOT_BITS;" in src, "the kernel's constants moved"
    slot = int(m.group((1 if pre else 3) + (regs - 1)))
    return 64 * regs, 32 - slot


def key_of(d2, scale, key_bits):
    """min(floor(d2 * scale), key_max - 1) as uint64"""
    key_max = (1 << key_bits) - 1
    return np.minimum(np.floor(np.asarray(d2, np.float64) * scale), float(key_max - 1)).astype(np.uint64)


def scale_of(cell, key_bits):
    return float(1 << key_bits) / (KEY_RANGE * cell * cell)


def analyse(pts, k, eps=0.0, factor=0.0, family=PAIR, regs=None, pre=True, items_q=16, r1_max=None):
    """Per owned row (the whole cloud, public order) of pct_knn(k, eps, PCT_KNN_GRID) on a fresh handle with occupancy factor
    `factor`: a dict of arrays -- m (stencil population), over, gkey, need, tk (PAD: fewer than k+1 in the ball), saturated,
    no_threshold, by_guarantee, must_redo, must_final, undecided, tie (entries k and k+1 share a key, or entry k is missing),
    set_k1 (list per row: (public indices, keys) of the stencil's k+1 nearest in (d2, public index) order, None where a tie
    leaves the set undefined), inball (candidates with d2 < eps^2), ball (candidates the pre-selection may count), long_run --
    and the build b, scale, eps_key, LIST, KEY_BITS, cap."""
    pts = np.asarray(pts)
    native = pts.dtype == np.float64
    regs = regs or (2 if family == DUO else 1)
    LIST, KB = constants(family, regs, pre)
    key_max = (1 << KB) - 1
    b = ge.Handle(factor).build(pts, k, eps, items_q=items_q)
    assert not b["trimmed"] and b["verdict"] == "built", "the restatement needs an untrimmed, built grid"
    cells = b["cells_obj"]
    n = len(pts)
    rec32 = np.ascontiguousarray(pts.astype(F32))
    rec = rec32.astype(np.float64)
    qry = pts.astype(np.float64) if native else rec
    cell, dims = b["cell_size"], b["dims"]
    scale = scale_of(cell, KB)
    cap = ge.STAGE_CAP if k + 1 <= (r1_max or ge.oe.FAST_R1_MAX) else ge.STAGE_CAP2
    eps2 = eps * eps if eps > 0 else np.inf
    eps_key = PAD if not eps > 0 else int(min(np.ceil(eps2 * scale), 4294967295.0))
    # the guarantee of ring 1
    c = cells.coord
    g = (qry - b["lo"].astype(np.float64)) * b["inv"] - c
    g2 = ge.guaranteed_r2(b, c, g, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        gk = np.where(np.isinf(g2), float(PAD), np.floor(np.minimum(g2 * scale, 4294967294.0)))
        frac = g2 * scale - np.floor(g2 * scale)
        near_edge = np.isfinite(g2) & ((frac <= te.UNDECIDED_REL * g2 * scale) | (1.0 - frac <= te.UNDECIDED_REL * g2 * scale))
    gkey = gk.astype(np.uint64)
    # rounding distance of a float64 query (load_queries), generously
    eq = np.sqrt(((qry - rec) ** 2).sum(1)) * (1.0 + 2.0 ** -20) if native else np.zeros(n)

    # the points of every occupied cell, and the stencil of each
    order = np.argsort(cells.of_point, kind="stable")
    starts = np.concatenate([[0], np.cumsum(cells.total)])
    members = [order[starts[i]:starts[i + 1]] for i in range(len(cells.ids))]
    nx, ny, nz = dims
    out = {name: np.zeros(n, dt) for name, dt in (("m", np.int64), ("need", np.uint64), ("tk", np.uint64), ("saturated", bool), ("no_threshold", bool),
                                                  ("tie", bool), ("ball", np.int64), ("inball", np.int64), ("long_run", bool))}
    set_k1 = [None] * n
    _, bits = np.unique(rec32.view(np.uint32).reshape(n, 3), axis=0, return_inverse=True)      # bit-identical records share a label
    bits = bits.ravel()
    for ci, cid in enumerate(cells.ids):
        cx, cy, cz = int(cid % nx), int((cid // nx) % ny), int(cid // (nx * ny))
        near = []
        for dx, dy, dz in ge._OFFSETS:
            x, y, z = cx + dx, cy + dy, cz + dz
            if 0 <= x < nx and 0 <= y < ny and 0 <= z < nz:
                j = np.searchsorted(cells.ids, (z * ny + y) * nx + x)
                if j < len(cells.ids) and cells.ids[j] == (z * ny + y) * nx + x:
                    near.append(members[j])
        cand = np.concatenate(near)
        q = members[ci]
        d = rec[cand][None, :, :] - qry[q][:, None, :]
        d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        keys = key_of(d2, scale, KB)
        out["m"][q] = len(cand)
        lab = bits[cand]
        big = np.unique(lab[np.bincount(lab)[lab] >= LIST - k])    # piles large enough to leave no threshold
        for r, row in enumerate(q):
            inside = d2[r] < eps2
            o = np.lexsort((cand[inside], d2[r][inside]))          # (d2, public index): the order the exact sweep stores
            kk, who = keys[r][inside][o], cand[inside][o]
            out["inball"][row] = len(kk)
            # the pre-selection's ball: what it may count below its first bound
            out["ball"][row] = int((d2[r] <= (eps + 2.0 * eq[row]) ** 2 * (1.0 + 2.0 ** -16)).sum()) if eps > 0 else len(cand)
            if len(kk) > k:
                tk = int(kk[k])
                out["tk"][row] = tk
                out["need"][row] = min(tk + 1, eps_key)
                out["saturated"][row] = tk >= key_max - 1
                out["tie"][row] = len(kk) > k + 1 and int(kk[k + 1]) == tk
                if not out["tie"][row]:
                    set_k1[row] = (who[:k + 1], kk[:k + 1])        # every candidate of the stencil with a key up to entry k's
            else:
                out["tk"][row] = PAD
                out["need"][row] = min(PAD, eps_key)
                out["tie"][row] = True                             # (no (k+1)-th entry: never trusted)
            # equal-key runs that reach into the first k+2 entries
            if len(kk):
                _, first, counts = np.unique(kk, return_index=True, return_counts=True)
                out["long_run"][row] = bool((counts[first < k + 2] > RUN_MAX).any())
            # no threshold: a pile of bit-identical records surely inside the pre-selection's ball, fewer than k+1 candidates
            # can lie below it and more than LIST lie at or below it for certain.  (A float64 query's float32 distances are
            # taken from its rounding: not decided here.)
            if native and eq[row] > 0:
                continue
            for pile in big:
                in_pile = lab == pile
                dp = float(d2[r][in_pile][0])
                if eps > 0 and not dp < eps2 * (1.0 - 2.0 ** -16):
                    continue
                maybe_below = int((~in_pile & (d2[r] <= dp * (1.0 + 2.0 ** -16))).sum())
                surely_below = int((~in_pile & (d2[r] < dp * (1.0 - 2.0 ** -16))).sum())
                if maybe_below < k + 1 and surely_below + int(in_pile.sum()) > LIST:
                    out["no_threshold"][row] = True
    over = out["m"] > cap
    need = out["need"]
    by_guarantee = need > gkey
    must_redo = over | by_guarantee | out["saturated"] | out["no_threshold"]
    one_unit = (np.abs(need.astype(np.float64) - gkey.astype(np.float64)) <= 1.0) & (need != PAD) & (gkey != PAD)
    undecided = (one_unit | near_edge) & ~over & ~out["saturated"] & ~out["no_threshold"]
    must_final = ~must_redo & ~undecided & (out["ball"] <= LIST) & ~out["long_run"]
    must_redo = must_redo & ~undecided
    out.update(over=over, gkey=gkey, g2=g2, by_guarantee=by_guarantee & ~undecided, must_redo=must_redo, must_final=must_final, undecided=undecided,
               set_k1=set_k1, b=b, scale=scale, eps_key=eps_key, LIST=LIST, KEY_BITS=KB, cap=cap, eq=eq, coord=c, members=members)
    return out


def stencil_members(a, row):
    """public indices of the candidates of `row`'s stencil"""
    b = a["b"]
    cells = b["cells_obj"]
    nx, ny, nz = b["dims"]
    cx, cy, cz = (int(v) for v in a["coord"][row])
    near = []
    for dx, dy, dz in ge._OFFSETS:
        x, y, z = cx + dx, cy + dy, cz + dz
        if 0 <= x < nx and 0 <= y < ny and 0 <= z < nz:
            cid = (z * ny + y) * nx + x
            j = np.searchsorted(cells.ids, cid)
            if j < len(cells.ids) and cells.ids[j] == cid:
                near.append(a["members"][j])
    return np.concatenate(near)

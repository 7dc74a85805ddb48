"""Exact restatement of the sweeps' wave-level sorters  --  TEST INFRASTRUCTURE ONLY (CPU, NumPy, no import of the package).

Every neighbour row passes through one of these (pct_knn_net.h, pct_knn_sweep.h, pct_sort_pair.inc, pct_sort_duo.inc):

``comparators``  the flip-form bitonic network of the fast sweeps as an explicit list of levels, built from the definition
                 in the header comment of pct_knn_net.h: a merge of SIZE compares element i with i ^ (SIZE - 1), then runs
                 the strides SIZE/4 .. 1, for SIZE = 2 .. n; every compare-exchange leaves the smaller element at the
                 lower index.  ``merges`` names the levels of each merge, ``apply`` runs levels on lists.
``zero_one_merge_inputs``  the inputs of the 0-1 proof of one merge: every pair of ascending 0-1 runs of SIZE/2 at every
                 aligned offset.  A merge that orders all of them merges any two ascending runs (0-1 principle); a network
                 whose merges of SIZE = 2 .. n all do is a sorter, by induction over SIZE.
``IncProgram``   a lane-level interpreter of the instruction text of the two generated assembly blocks: the ten instruction
                 forms they contain, 64 lanes, the named operands.  Anything else raises.  It checks the LOGIC of the text;
                 wait states are the device's business (tests/test_gpu_sort_net.py).
``repair``       order_equal_keys pass by pass: it predicts the list AND the returned flag.
``repair_statement``  what a finished repair has to leave, stated independently: elements of different keys where they
                 were, every run of equal keys in (d2, pub) order.
``exact_sort``, ``merge_min``  the exact sweep's total order (key_less): fp64 d2, then the public index of the position,
                 padding (+inf, INT_MAX) last; bitonic_merge_min as "the 64 R smallest of the union, ascending".

No tolerance anywhere: everything here is integers, or doubles that are only compared and moved.
"""
import re

import numpy as np

PAD = np.uint32(0xFFFFFFFF)          # kPadElem
INT_MAX = np.int32(0x7FFFFFFF)
ORDER_PASSES = 36                    # kOrderPasses (tests/test_net_exact.py holds it to the header)


# ---------------------------------------------------------------------------------------------------------------------------
# the network
# ---------------------------------------------------------------------------------------------------------------------------
def merge_levels(n, size):
    """The levels of the merge of `size` over n elements: lists of (low index, high index), smaller element to the low one."""
    assert size >= 2 and size & (size - 1) == 0 and n % size == 0
    levels = [[(i, i ^ (size - 1)) for i in range(n) if i < i ^ (size - 1)]]
    st = size // 4
    while st >= 1:
        levels.append([(i, i ^ st) for i in range(n) if i & st == 0])
        st //= 2
    return levels


def merges(n, sets=1):
    """[(SIZE, levels of that merge)] for SIZE = 2 .. n; `sets` independent lists side by side, set s at [s n, (s + 1) n)."""
    assert n in (64, 128)
    out = []
    size = 2
    while size <= n:
        one = merge_levels(n, size)
        out.append((size, [[(lo + s * n, hi + s * n) for s in range(sets) for lo, hi in lv] for lv in one]))
        size *= 2
    return out


def comparators(n, sets=1):
    """The whole network: 21 levels for n = 64, 28 for n = 128."""
    return [lv for _, lvs in merges(n, sets) for lv in lvs]


def apply(levels, lists):
    """Run compare-exchange levels on lists (..., N); returns a new array."""
    x = np.array(lists, copy=True)
    for lv in levels:
        lo = np.array([p[0] for p in lv])
        hi = np.array([p[1] for p in lv])
        a, b = x[..., lo], x[..., hi]
        x[..., lo], x[..., hi] = np.minimum(a, b), np.maximum(a, b)
    return x


def zero_one_merge_inputs(n, size, rng):
    """Every pair of ascending 0-1 runs of size/2, (size/2 + 1)^2 of them, at every aligned offset of an n-element list:
    (n / size) (size/2 + 1)^2 lists.  The blocks beside the one under test hold valid pairs of runs of their own (drawn
    from rng), so the whole output can be held to np.sort of every block."""
    h = size // 2
    run = (np.arange(h)[None, :] >= (h - np.arange(h + 1))[:, None]).astype(np.uint32)      # run[z]: h - z zeros, z ones
    pairs = np.concatenate([np.repeat(run, h + 1, axis=0), np.tile(run, (h + 1, 1))], axis=1)  # every (z0, z1)
    assert pairs.shape == ((h + 1) ** 2, size)
    nb = n // size
    out = []
    for off in range(nb):
        x = pairs[rng.integers(0, len(pairs), size=(len(pairs), nb))].reshape(len(pairs), n)
        x[:, off * size:(off + 1) * size] = pairs
        out.append(x)
    return np.concatenate(out)


def sorted_blocks(lists, size):
    """np.sort of every aligned block of `size`."""
    x = np.asarray(lists)
    return np.sort(x.reshape(x.shape[:-1] + (x.shape[-1] // size, size)), axis=-1).reshape(x.shape)


# ---------------------------------------------------------------------------------------------------------------------------
# the instruction text of pct_sort_pair.inc / pct_sort_duo.inc
# ---------------------------------------------------------------------------------------------------------------------------
_LANE = np.arange(64)
_DPP_FULL = "row_mask:0xf bank_mask:0xf bound_ctrl:1"


def _dpp_source(ctrl):
    """Source lane of every lane under a DPP control (all of them stay inside their row of 16: no lane reads nothing)."""
    row, i = _LANE & ~15, _LANE & 15
    m = re.fullmatch(r"quad_perm:\[(\d),(\d),(\d),(\d)\]", ctrl)
    if m:
        perm = np.array([int(g) for g in m.groups()])
        assert perm.max() < 4
        return (_LANE & ~3) | perm[_LANE & 3]
    if ctrl == "row_mirror":
        return row | (15 - i)
    if ctrl == "row_half_mirror":
        return (_LANE & ~7) | (7 - (_LANE & 7))
    m = re.fullmatch(r"row_ror:(\d+)", ctrl)
    if m and 1 <= int(m.group(1)) <= 15:
        return row | ((i - int(m.group(1))) & 15)          # rotate right: lane i takes the value n lanes below it
    raise ValueError("DPP control the interpreter does not know: %r" % ctrl)


class IncProgram:
    """One generated .inc file: its result registers and its instruction lines."""

    OPERANDS = ("ea", "eb", "ta", "tb", "sel0", "sel1", "sel2", "sel3", "sel4", "sel5", "a31", "a63")

    def __init__(self, text, name):
        self.result = tuple(re.search(r"#define PCT_SORT_%s_RESULT_%s (\w+)" % (name, s), text).group(1) for s in "AB")
        body = text.split("#define PCT_SORT_%s_ASM" % name)[1]
        self.lines = re.findall(r'^\s*"(.+?)\\n" \\$', body, flags=re.M)
        assert self.lines and body.count('\\n"') == len(self.lines), "a line of the block the parser did not take"

    @staticmethod
    def constants():
        regs = {"sel%d" % j: np.where((_LANE >> j) & 1, 0xFFFFFFFF, 0).astype(np.uint32) for j in range(6)}
        regs["a31"] = ((_LANE ^ 31) << 2).astype(np.uint32)
        regs["a63"] = ((_LANE ^ 63) << 2).astype(np.uint32)
        return regs

    @staticmethod
    def _ops(rest):
        names = re.findall(r"%\[(\w+)\]", rest)
        for nm in names:
            if nm not in IncProgram.OPERANDS:
                raise ValueError("unknown operand %r" % nm)
        return names

    def step(self, regs, line):
        """Execute one line on regs (name -> (B, 64) uint32).  Returns (kind, dst, data sources) for the level tracker:
        kind is 'level' for an instruction that completes a compare-exchange level of its set, else 'move' or 'none'."""
        mnem, _, rest = line.partition(" ")
        if mnem in ("s_nop", "s_waitcnt"):
            if not re.fullmatch(r"\d+|lgkmcnt\(\d+\)", rest):
                raise ValueError("operand of %s: %r" % (mnem, rest))
            return "none", None, ()
        ops = self._ops(rest)
        tail = re.sub(r"%\[\w+\],?\s*", "", rest).strip()                # what follows the registers: the modifiers
        if mnem == "v_mov_b32":
            if tail or len(ops) != 2:
                raise ValueError(line)
            regs[ops[0]] = regs[ops[1]].copy()
            return "move", ops[0], (ops[1],)
        if mnem == "v_mov_b32_dpp":
            if len(ops) != 2 or not tail.endswith(" " + _DPP_FULL):
                raise ValueError(line)
            regs[ops[0]] = regs[ops[1]][:, _dpp_source(tail[:-len(_DPP_FULL) - 1])]
            return "move", ops[0], (ops[1],)
        if mnem in ("v_min_u32_dpp", "v_max_u32_dpp"):
            m = re.fullmatch(r"(row_ror:\d+) row_mask:0xf bank_mask:0x([0-9a-f])", tail)
            if len(ops) != 3 or not m:
                raise ValueError(line)
            f = np.minimum if mnem == "v_min_u32_dpp" else np.maximum
            val = f(regs[ops[1]][:, _dpp_source(m.group(1))], regs[ops[2]])
            on = ((int(m.group(2), 16) >> ((_LANE & 15) >> 2)) & 1).astype(bool)      # bank = four lanes of a row
            regs[ops[0]] = np.where(on[None, :], val, regs[ops[0]])      # a masked-off bank keeps the destination's old value
            return ("level" if mnem == "v_max_u32_dpp" else "move"), ops[0], (ops[1], ops[2])
        if mnem in ("v_min_u32", "v_max_u32"):
            if tail or len(ops) != 3:
                raise ValueError(line)
            regs[ops[0]] = (np.minimum if mnem == "v_min_u32" else np.maximum)(regs[ops[1]], regs[ops[2]])
            return "level", ops[0], (ops[1], ops[2])
        if mnem == "v_med3_u32":
            if tail or len(ops) != 4:
                raise ValueError(line)
            regs[ops[0]] = np.sort(np.stack([regs[ops[1]], regs[ops[2]], np.broadcast_to(regs[ops[3]], regs[ops[1]].shape)]), axis=0)[1]
            return "level", ops[0], (ops[1], ops[2])
        if mnem in ("v_permlane16_swap_b32", "v_permlane32_swap_b32"):
            if tail or len(ops) != 2:
                raise ValueError(line)
            w = 16 if mnem == "v_permlane16_swap_b32" else 32
            d, s = regs[ops[0]].copy(), regs[ops[1]].copy()
            upper = (_LANE & w) != 0                                      # odd rows (16) / the upper half (32) of vdst ...
            d[:, upper], s[:, ~upper] = regs[ops[1]][:, ~upper], regs[ops[0]][:, upper]     # ... <-> even rows / lower half of vsrc
            regs[ops[0]], regs[ops[1]] = d, s
            return "move", ops[0], (ops[0], ops[1])
        if mnem == "ds_bpermute_b32":
            if tail or len(ops) != 3:
                raise ValueError(line)
            src = (regs[ops[1]] >> 2) & 63
            regs[ops[0]] = np.take_along_axis(regs[ops[2]], np.broadcast_to(src, regs[ops[2]].shape).astype(np.int64), axis=1)
            return "move", ops[0], (ops[2],)
        raise ValueError("instruction the interpreter does not know: %r" % line)

    def run(self, a, b, on_level=None, lines=None, start=("ea", "eb"), bounds=None):
        """Run `lines` (default: all) with set a / b (B, 64) in the registers `start`; every other data register starts as
        noise.  on_level(n_levels_done, list (B, 128) = set a then set b) is called whenever both sets have finished the
        same number of levels; bounds, if given, collects (lines consumed, registers of the sets) at those points.  Returns (registers, (register of set a, register of set b), levels done)."""
        rng = np.random.default_rng(7)
        regs = self.constants()
        regs = {k: np.broadcast_to(v, a.shape).copy() for k, v in regs.items()}
        for nm in ("ea", "eb", "ta", "tb"):
            regs[nm] = rng.integers(0, 2 ** 32, size=a.shape, dtype=np.uint64).astype(np.uint32)
        regs[start[0]], regs[start[1]] = a.astype(np.uint32).copy(), b.astype(np.uint32).copy()
        tag = {start[0]: "a", start[1]: "b"}                             # which set's data a register holds
        cur = {"a": start[0], "b": start[1]}
        done = {"a": 0, "b": 0}
        for at, line in enumerate(self.lines if lines is None else lines):
            kind, dst, srcs = self.step(regs, line)
            if kind == "none":
                continue
            tags = {tag.get(s) for s in srcs}
            if None in tags:
                raise ValueError("%r reads a register no set has written" % line)
            if len(tags) == 2:                                           # the 128-wide flip: min -> lower half, max -> upper
                if not line.startswith(("v_min_u32 ", "v_max_u32 ")):
                    raise ValueError("%r mixes the two sets" % line)
                t = "a" if line.startswith("v_min_u32 ") else "b"
            else:
                t = tags.pop()
            tag[dst] = t
            if kind == "level":
                cur[t] = dst
                done[t] += 1
                assert abs(done["a"] - done["b"]) <= 1
                if done["a"] == done["b"]:
                    if bounds is not None:
                        bounds.append((at + 1, (cur["a"], cur["b"])))
                    if on_level is not None:
                        on_level(done["a"], np.concatenate([regs[cur["a"]], regs[cur["b"]]], axis=1))
        return regs, (cur["a"], cur["b"]), done["a"]

    def segments(self):
        """The lines of every level (all lines from the point both sets have finished level L - 1 up to the point both
        have finished level L) and the registers that hold the two sets before it: [(lines, (reg a, reg b))]."""
        zero = np.zeros((1, 64), np.uint32)
        bounds = []
        self.run(zero, zero, bounds=bounds)
        out, first, start = [], 0, ("ea", "eb")
        for end, cur in bounds:
            out.append((self.lines[first:end], start))
            first, start = end, cur
        assert all(l.startswith(("s_nop", "s_waitcnt")) for l in self.lines[first:]), "instructions behind the last level"
        return out


# ---------------------------------------------------------------------------------------------------------------------------
# order_equal_keys
# ---------------------------------------------------------------------------------------------------------------------------
def repair(elems, d2, pub, slot_bits, regs):
    """order_equal_keys<regs, slot_bits> pass by pass.
    elems (L, 64 regs) uint32: key << slot_bits | payload, padding 0xFFFFFFFF;  d2, pub (L, 2^slot_bits): the exact value
    and the public index of the element with that payload.  Returns (lists, flags): pass p has parity p & 1 and compares
    the pairs (2i + parity, 2i + parity + 1); a pair is compared only when neither element is padding and both have the
    same key; the lower position keeps the smaller by (d2, pub).  True after two consecutive passes without an exchange
    anywhere in the list, False after ORDER_PASSES passes."""
    e = np.array(elems, dtype=np.uint32, copy=True).reshape(-1, 64 * regs)
    L, n = e.shape
    d2 = np.broadcast_to(np.asarray(d2, np.float64), (L, 1 << slot_bits))
    pub = np.broadcast_to(np.asarray(pub, np.int64), (L, 1 << slot_bits))
    mask = np.uint32((1 << slot_bits) - 1)
    rows = np.arange(L)[:, None]
    flag = np.zeros(L, bool)
    live = np.ones(L, bool)
    quiet = np.zeros(L, np.int64)
    for p in range(ORDER_PASSES):
        lo = np.arange(p & 1, n - 1, 2)
        a, b = e[:, lo], e[:, lo + 1]
        same = (a != PAD) & (b != PAD) & (((a ^ b) >> np.uint32(slot_bits)) == 0)
        pa, pb = (a & mask).astype(np.int64), (b & mask).astype(np.int64)
        da, db = d2[rows, pa], d2[rows, pb]
        b_less = (db < da) | ((db == da) & (pub[rows, pb] < pub[rows, pa]))
        swap = same & b_less & live[:, None]
        e[:, lo], e[:, lo + 1] = np.where(swap, b, a), np.where(swap, a, b)
        moved = swap.any(axis=1)
        quiet = np.where(moved, 0, quiet + 1)
        finished = live & (quiet == 2)
        flag |= finished
        live &= ~finished
        if not live.any():
            break
    return e, flag


def runs_of(elems, slot_bits):
    """Run id of every position: maximal stretches of adjacent real elements with one key; padding elements are runs of one."""
    e = np.asarray(elems, np.uint32)
    brk = np.ones(e.shape, bool)
    brk[..., 1:] = (e[..., 1:] == PAD) | (e[..., :-1] == PAD) | ((e[..., 1:] >> np.uint32(slot_bits)) != (e[..., :-1] >> np.uint32(slot_bits)))
    return np.cumsum(brk, axis=-1)


def repair_statement(elems, d2, pub, slot_bits):
    """What a finished repair leaves, stated without passes: every run of equal keys sorted by np.lexsort((pub, d2))."""
    e = np.array(elems, dtype=np.uint32, copy=True)
    out = e.copy()
    mask = np.uint32((1 << slot_bits) - 1)
    for l in range(e.shape[0]):
        run = runs_of(e[l], slot_bits)
        pay = (e[l] & mask).astype(np.int64)
        dl = np.broadcast_to(d2, (e.shape[0], 1 << slot_bits))[l][pay]
        pl = np.broadcast_to(pub, (e.shape[0], 1 << slot_bits))[l][pay]
        out[l] = e[l][np.lexsort((pl, dl, run))]          # run ids ascend along the list: positions of a run stay its own
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the exact sweep's order
# ---------------------------------------------------------------------------------------------------------------------------
def exact_sort(d2, pos, pub, descending=False):
    """bitonic_sort_from: lists (L, N) of (fp64 d2, int32 position) in key_less's total order -- d2, then the public index
    pub[position]; padding is (+inf, INT_MAX) and goes last (first when descending)."""
    d2 = np.asarray(d2, np.float64)
    pos = np.asarray(pos, np.int32)
    real = pos != INT_MAX
    key2 = np.where(real, np.asarray(pub, np.int64)[np.where(real, pos, 0)], np.int64(INT_MAX))
    assert np.all(np.isinf(d2[~real]) & (d2[~real] > 0)) and np.all(np.isfinite(d2[real])), "padding is (+inf, INT_MAX), real elements are finite"
    order = np.lexsort((key2, d2), axis=-1)
    if descending:
        order = order[..., ::-1]
    return np.take_along_axis(d2, order, axis=-1), np.take_along_axis(pos, order, axis=-1)


def merge_min(best_d2, best_pos, batch_d2, batch_pos, pub):
    """bitonic_merge_min: the N smallest of best U batch, ascending."""
    n = np.asarray(best_d2).shape[-1]
    d, p = exact_sort(np.concatenate([best_d2, batch_d2], axis=-1), np.concatenate([best_pos, batch_pos], axis=-1), pub)
    return d[..., :n], p[..., :n]

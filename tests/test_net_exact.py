"""What tests/test_gpu_sort_net.py leans on, proven on the CPU: the restated network is a sorter (per-merge 0-1 proof, no
case left out), the committed assembly blocks are what the generator emits and their instruction text is that network,
and the restated repair of equal keys has the bound the sweeps rely on."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import net_exact as ne

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "point-cloud-toolbox_amd", "csrc")
INC = {"PAIR": ("pct_sort_pair.inc", []), "DUO": ("pct_sort_duo.inc", ["duo"])}


def _program(name):
    with open(os.path.join(CSRC, INC[name][0])) as f:
        return ne.IncProgram(f.read(), name)


def _reference(name):
    """(merges, levels) of the restatement the block `name` has to be: two lists of 64 side by side, or one of 128."""
    ms = ne.merges(64, sets=2) if name == "PAIR" else ne.merges(128)
    return ms, [lv for _, lvs in ms for lv in lvs]


# ------------------------------------------------------------------------------------------------------------ the network
def test_level_counts():
    assert len(ne.comparators(64)) == 21 and len(ne.comparators(128)) == 28
    for n in (64, 128):
        for lv in ne.comparators(n):
            assert len(lv) == n // 2 and sorted(i for p in lv for i in p) == list(range(n)) and all(lo < hi for lo, hi in lv)


@pytest.mark.parametrize("n", [64, 128])
def test_restated_network_is_a_sorter(n):
    """Induction over merges: the merge of SIZE, alone, turns every pair of ascending 0-1 runs of SIZE/2, at every aligned
    offset, into an ascending run -- (SIZE/2 + 1)^2 inputs per offset, none skipped.  By the 0-1 principle it merges any
    two ascending runs; runs of 1 are ascending; so SIZE = 2 .. n in turn sort."""
    rng = np.random.default_rng(1)
    seen = []
    for size, levels in ne.merges(n):
        x = ne.zero_one_merge_inputs(n, size, rng)
        assert len(x) == (n // size) * (size // 2 + 1) ** 2
        assert np.array_equal(ne.apply(levels, x), ne.sorted_blocks(x, size)), size
        seen.append(size)
    assert seen == [2 << j for j in range(n.bit_length() - 1)]
    x = rng.integers(0, 2 ** 32, size=(512, n), dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(ne.apply(ne.comparators(n), x), np.sort(x, axis=1))


# -------------------------------------------------------------------------------------------------- the assembly blocks
@pytest.mark.parametrize("name", ["PAIR", "DUO"])
def test_inc_files_are_what_the_generator_emits(name):
    fn, args = INC[name]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_sort_asm.py")] + args, check=True, capture_output=True).stdout
    with open(os.path.join(CSRC, fn), "rb") as f:
        assert out == f.read()


@pytest.mark.parametrize("name", ["PAIR", "DUO"])
def test_inc_text_is_the_network_level_by_level(name):
    prog = _program(name)
    _, levels = _reference(name)
    rng = np.random.default_rng(2)
    x = np.stack([np.arange(128), np.arange(128)[::-1]] + [rng.permutation(128) for _ in range(254)]).astype(np.uint32)
    x[2::2] *= np.uint32(0x01F35A7D)                # odd multiplier: still distinct, every bit of the word in use
    state = {"x": x.copy(), "n": 0}

    def on_level(n_done, lists):
        assert n_done == state["n"] + 1
        state["x"] = ne.apply(levels[state["n"]:n_done], state["x"])
        state["n"] = n_done
        assert np.array_equal(lists, state["x"]), "level %d" % n_done

    regs, cur, done = prog.run(x[:, :64], x[:, 64:], on_level=on_level)
    assert done == state["n"] == len(levels)
    assert cur == prog.result, "the declared result registers are the ones the last level wrote"
    got = np.concatenate([regs[prog.result[0]], regs[prog.result[1]]], axis=1)
    want = np.sort(x, axis=1) if name == "DUO" else np.concatenate([np.sort(x[:, :64], axis=1), np.sort(x[:, 64:], axis=1)], axis=1)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", ["PAIR", "DUO"])
def test_inc_text_passes_the_zero_one_proof(name):
    """The same per-merge enumeration as for the restatement, on the instruction text: the lines of one merge, started
    from the registers that hold the sets there, everything else noise."""
    prog = _program(name)
    ms, _ = _reference(name)
    segs = prog.segments()
    assert len(segs) == sum(len(lvs) for _, lvs in ms)
    rng = np.random.default_rng(3)
    at = 0
    for size, lvs in ms:
        lines = [l for seg, _ in segs[at:at + len(lvs)] for l in seg]
        start = segs[at][1]
        at += len(lvs)
        if name == "DUO" or size == 128:
            n = 128
            x = ne.zero_one_merge_inputs(128, size, rng)
        else:                            # two lists of 64: every case goes through set a AND through set b
            n = 64
            x = ne.zero_one_merge_inputs(64, size, rng)
            x = np.concatenate([x, np.roll(x, 1, axis=0)], axis=1)
        assert len(x) == (n // size) * (size // 2 + 1) ** 2
        regs, cur, done = prog.run(x[:, :64], x[:, 64:], lines=lines, start=start)
        assert done == len(lvs)
        got = np.concatenate([regs[cur[0]], regs[cur[1]]], axis=1)
        assert np.array_equal(got, ne.sorted_blocks(x, size)), size


def test_interpreter_refuses_what_it_does_not_know():
    prog = _program("PAIR")
    regs = {k: np.zeros((1, 64), np.uint32) for k in ne.IncProgram.OPERANDS}
    for bad in ("v_add_u32 %[ea], %[ea], %[ta]",
                "v_mov_b32_dpp %[ta], %[ea] row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1",
                "v_mov_b32_dpp %[ta], %[ea] row_mirror row_mask:0xf bank_mask:0x5 bound_ctrl:1",
                "v_med3_u32 %[ea], %[ea], %[ta], %[sel6]",
                "v_min_u32_dpp %[ta], %[ea], %[ea] row_ror:12 row_mask:0x3 bank_mask:0x5"):
        with pytest.raises(ValueError):
            prog.step(regs, bad)


# ------------------------------------------------------------------------------------------------------------- the repair
def _run_list(regs, slot_bits, at, order, d2_of, pub_of):
    """One sorted list of 64 regs elements with distinct keys except a run of len(order) equal keys at position `at`, whose
    payloads at + order[j] carry (d2_of[j], pub_of[j]) in run order j."""
    n = 64 * regs
    keys = np.arange(n, dtype=np.uint32) + 10            # ascending, one key per position ...
    keys[at:at + len(order)] = at + 10                   # ... but for the run
    pay = np.arange(n, dtype=np.uint32)
    pay[at:at + len(order)] = at + np.asarray(order)
    d2 = np.arange(1 << slot_bits, dtype=np.float64)
    pub = np.arange(1 << slot_bits, dtype=np.int64)
    d2[at:at + len(order)] = d2_of
    pub[at:at + len(order)] = pub_of
    return (keys << np.uint32(slot_bits)) | pay, d2, pub


def _single_runs(regs, slot_bits, length, rng):
    """Runs of `length` at offsets of both parities, at the head, the tail and (two registers) across position 63/64:
    reversed and random orders; d2 all distinct, all equal with pub deciding."""
    n = 64 * regs
    ats = {0, 1, 6, 7, n - length, n - length - 1}
    if regs == 2:
        ats |= {64 - length // 2, 63 - length // 2, 63, 64 - length + 1}
    E, D, P = [], [], []
    for at in sorted(a for a in ats if 0 <= a and a + length <= n):
        for order in [np.arange(length)[::-1]] + [rng.permutation(length) for _ in range(3)]:
            for tie in (False, True):
                d2_of = np.full(length, 3.5) if tie else 100.0 + np.arange(length)
                e, d, p = _run_list(regs, slot_bits, at, order, d2_of, 1000 + np.arange(length))
                E.append(e), D.append(d), P.append(p)
    return np.array(E), np.array(D), np.array(P)


def test_order_passes_is_the_headers():
    with open(os.path.join(CSRC, "pct_knn_net.h")) as f:
        assert int(re.search(r"constexpr int kOrderPasses = (\d+);", f.read()).group(1)) == ne.ORDER_PASSES


@pytest.mark.parametrize("regs,slot_bits", [(1, 6), (2, 7)])
def test_repair_bound(regs, slot_bits):
    """The longest run a repair is certain to finish, derived from `repair` itself: every run of up to 34 equal keys ends
    in order with True, a reversed run of 35 returns False.  (An odd-even transposition orders L elements in L passes,
    whichever parity comes first; two quiet passes follow: L + 2 <= kOrderPasses.)"""
    rng = np.random.default_rng(4)
    bound = None
    for length in range(2, 64):
        e, d, p = _single_runs(regs, slot_bits, length, rng)
        out, flag = ne.repair(e, d, p, slot_bits, regs)
        assert np.array_equal(out[flag], ne.repair_statement(e, d, p, slot_bits)[flag]), length      # True: the exact order
        # True or False: every element is still inside its own run
        run = ne.runs_of(e, slot_bits).astype(np.int64) << 32
        assert np.array_equal(ne.runs_of(out, slot_bits).astype(np.int64) << 32, run)
        assert np.array_equal(np.sort(out + run, axis=1), np.sort(e + run, axis=1))
        if not flag.all():
            bound = length - 1
            break
    assert bound == ne.ORDER_PASSES - 2 == 34
    # the reversed run of 35 (lists 0 and 1 of every eight: by d2, and by pub alone), wherever it sits
    e, d, p = _single_runs(regs, slot_bits, 35, rng)
    _, flag = ne.repair(e, d, p, slot_bits, regs)
    assert not flag[0::8].any() and not flag[1::8].any()


def test_repair_leaves_a_list_without_equal_keys_alone():
    e = ((np.arange(128, dtype=np.uint32) + 3) << np.uint32(7)) | np.arange(128, dtype=np.uint32)[::-1]
    e[100:] = ne.PAD
    out, flag = ne.repair(e[None], np.zeros((1, 128)), np.zeros((1, 128), np.int64), 7, 2)
    assert flag.all() and np.array_equal(out[0], e)


def test_repair_adjacent_runs_and_padding():
    """Runs side by side never mix, a run that ends at the padding does not pull it in, and padding elements (whose key
    bits are all ones, equal among themselves) are never compared."""
    rng = np.random.default_rng(5)
    sb, n = 7, 128
    keys = np.repeat(np.array([4, 9, 9, 11], np.uint32), [20, 30, 0, 25])
    keys = np.concatenate([keys, np.full(n - len(keys), 0, np.uint32)])
    real = len(keys) - (n - 75)
    E = []
    for _ in range(64):
        e = (keys << np.uint32(sb)) | rng.permutation(n).astype(np.uint32)
        e[real:] = ne.PAD
        E.append(e)
    E = np.array(E)
    d2 = rng.integers(0, 6, size=(len(E), n)).astype(np.float64)              # many exact ties: pub decides
    pub = np.argsort(rng.random((len(E), n)), axis=1)
    out, flag = ne.repair(E, d2, pub, sb, 2)
    assert flag.all()
    assert np.array_equal(out, ne.repair_statement(E, d2, pub, sb))
    assert np.all(out[:, real:] == ne.PAD)


# -------------------------------------------------------------------------------------------------------- the exact order
def test_exact_sort_and_merge_min():
    rng = np.random.default_rng(6)
    pub = rng.permutation(500)
    d2 = rng.integers(0, 8, size=(32, 128)).astype(np.float64)
    pos = np.argsort(rng.random((32, 500)), axis=1)[:, :128].astype(np.int32)
    d2[:, 100:], pos[:, 100:] = np.inf, ne.INT_MAX
    sd, sp = ne.exact_sort(d2, pos, pub)
    for l in range(32):
        items = sorted((d2[l, i], pub[pos[l, i]], pos[l, i]) for i in range(100))
        assert [it[2] for it in items] == list(sp[l, :100]) and np.all(sp[l, 100:] == ne.INT_MAX) and np.all(np.isinf(sd[l, 100:]))
    dd, dp = ne.exact_sort(d2, pos, pub, descending=True)
    assert np.array_equal(dd[:, ::-1], sd) and np.array_equal(dp[:, ::-1], sp)
    md, mp = ne.merge_min(sd[:, :64], sp[:, :64], dd[:, :64], dp[:, :64], pub)
    assert np.array_equal(md, sd[:, :64]) and np.array_equal(mp, sp[:, :64])

"""The sweeps' wave-level sorters on the device, list by list against tests/net_exact.py: every list, element and flag is
compared, nothing is sampled and there is no tolerance.  What the expected values rest on is proven in
tests/test_net_exact.py; what only the device can say -- the DPP controls and bank masks as the hardware reads them, the
{own, partner} order out of v_permlane16/32_swap, the wait states the generator counted -- is what these runs add."""
import functools

import numpy as np
import pytest

import net_exact as ne

pytestmark = pytest.mark.gpu

PAD = 0xFFFFFFFF


@pytest.fixture(scope="module")
def handle(gpu):
    h = gpu["capi"].Handle(0)
    yield h
    h.close()


# ------------------------------------------------------------------------------------------------------------ the orders
def _bit_reversal(n):
    bits = n.bit_length() - 1
    return np.array([int(format(i, "0%db" % bits)[::-1], 2) for i in range(n)])


def orders(n):
    """Rank lists (values 0 .. n - 1): identity, reverse, every rotation, bit reversal, organ pipe, saw teeth."""
    i = np.arange(n)
    out = [i, i[::-1], _bit_reversal(n), np.concatenate([i[::2], i[::-2]]), np.concatenate([i[::-2], i[::2]])]
    out += [np.roll(i, s) for s in range(1, n)]
    out += [(i % m) * (n // m) + i // m for m in (2, 4, 8, 16, 32)]           # ascending teeth of length m
    return np.array(out)


def block_patterns(n, bounds=None):
    """Every 0-1 list with ones exactly in [i, j): n (n + 1) / 2 of them (bounds: the i and j to take, default all)."""
    b = np.arange(n + 1) if bounds is None else np.asarray(sorted(bounds))
    i, j = np.meshgrid(b, b, indexing="ij")
    i, j = i[i < j], j[i < j]
    pos = np.arange(n)[None, :]
    return ((pos >= i[:, None]) & (pos < j[:, None])).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def sorter_family(n):
    """The lists every selector sorts, with np.sort of them; read-only."""
    rng = np.random.default_rng(100 + n)
    slot_bits = 6 if n == 64 else 7
    fam = []
    blocks = block_patterns(n)
    assert len(blocks) == {64: 2080, 128: 8256}[n]
    real_key = np.uint32((0x2A5F3 << slot_bits) | 5)
    for lo, hi in ((0, 1), (0x7FFFFFFF, 0x80000000), (real_key, PAD), (0xFFFFFFFE, PAD)):
        fam.append(np.where(blocks == 1, np.uint32(hi), np.uint32(lo)))
    dens = np.linspace(0.01, 0.99, 4096)[:, None]                              # random 0-1 lists over a sweep of densities
    fam.append((rng.random((4096, n)) < dens).astype(np.uint32))
    o = orders(n).astype(np.uint32)
    fam += [o, o * np.uint32(0x01F35A7D)]                                      # (odd multiplier: distinct, all 32 bits in use)
    perms = np.argsort(rng.random((4096, n)), axis=1).astype(np.uint32)
    # every other one as distinct words all over the range (multiplication by an odd number is a bijection mod 2^32)
    perms[1::2] = perms[1::2] * np.uint32(0x9E3779B1) + rng.integers(0, 2 ** 32, size=(2048, 1), dtype=np.uint64).astype(np.uint32)
    fam.append(perms)
    # the shape the sweeps build: key << slot_bits | lane, few distinct keys, padding at the tail and in between
    keys = rng.integers(0, rng.integers(1, 9, size=(4096, 1)), size=(4096, n)).astype(np.uint32) * np.uint32(977) + np.uint32(3)
    shaped = (keys << np.uint32(slot_bits)) | (np.arange(n, dtype=np.uint32) & np.uint32((1 << slot_bits) - 1))
    tail = rng.integers(0, n + 1, size=(4096, 1))
    shaped[np.arange(n)[None, :] >= n - tail] = PAD
    shaped[rng.random((4096, n)) < rng.random((4096, 1)) * 0.3] = PAD
    fam.append(shaped)
    fam.append(np.array([np.full(n, 0x12345678), np.full(n, 0), np.full(n, PAD)], dtype=np.uint32))      # all equal; all padding
    x = np.concatenate(fam).astype(np.uint32)
    want = np.sort(x, axis=1)
    x.setflags(write=False), want.setflags(write=False)
    return x, want


def _interleave(a, b):
    out = np.empty((2 * len(a), a.shape[1]), np.uint32)
    out[0::2], out[1::2] = a, b
    return out


# ----------------------------------------------------------------------------------------------------------- the sorters
@pytest.mark.parametrize("net", ["FAST1", "FAST2", "DUO"])
def test_one_list_per_wave(handle, gpu, net):
    capi = gpu["capi"]
    code = getattr(capi, "NET_" + net)
    x, want = sorter_family(capi.NET_LIST[code])
    got = handle.selftest_sort(code, x)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "%s: %d lists differ from np.sort, first %d: %r -> %r" % (net, bad.size, bad[0], x[bad[0]], got[bad[0]])


@pytest.mark.parametrize("net", ["SETS1", "SETS2", "PAIR"])
def test_two_lists_per_wave(handle, gpu, net):
    """Both sets sorted, and set a's output byte-identical whether set b holds the same data, other data or padding --
    and the other way round."""
    capi = gpu["capi"]
    code = getattr(capi, "NET_" + net)
    x, want = sorter_family(capi.NET_LIST[code])
    other, pad = np.roll(x, 1, axis=0)[::-1], np.full_like(x, PAD)
    for label, a, b in (("same", x, x), ("other in b", x, other), ("padding in b", x, pad), ("other in a", other, x), ("padding in a", pad, x)):
        got = handle.selftest_sort(code, _interleave(a, b))
        mine = got[0::2] if a is x else got[1::2]
        bad = np.flatnonzero((mine != want).any(axis=1))
        assert bad.size == 0, "%s, %s: %d lists differ from np.sort, first %d: %r -> %r" % (net, label, bad.size, bad[0], x[bad[0]], mine[bad[0]])
        theirs, given = (got[1::2], b) if a is x else (got[0::2], a)
        assert np.array_equal(theirs, np.sort(given, axis=1)), (net, label)


def test_assembly_blocks_equal_the_cxx_network(handle, gpu):
    """PAIR = SETS1 and DUO = FAST2 on every input, byte for byte."""
    capi = gpu["capi"]
    x64, _ = sorter_family(64)
    pairs = _interleave(x64, np.roll(x64, 7, axis=0))
    assert np.array_equal(handle.selftest_sort(capi.NET_PAIR, pairs), handle.selftest_sort(capi.NET_SETS1, pairs))
    x128, _ = sorter_family(128)
    assert np.array_equal(handle.selftest_sort(capi.NET_DUO, x128), handle.selftest_sort(capi.NET_FAST2, x128))


def test_refusals(handle, gpu):
    """PCT_ERR_INVALID, and nothing launched: an odd count where a wave sorts two lists, a network, a list length, a mode
    or a (regs, slot_bits) pair no sweep instantiates, a position outside the public index table."""
    capi = gpu["capi"]
    lib, hp = handle._lib, handle._h
    x = np.zeros((4, 64), np.uint32)
    with pytest.raises(ValueError, match="n_lists"):
        handle.selftest_sort(capi.NET_PAIR, x[:3])
    with pytest.raises(ValueError, match="no network"):
        handle._check(lib.pct_selftest_sort(hp, 6, capi._ptr(x, capi._u32p), 4, capi._ptr(x.copy(), capi._u32p)))
    d2, pos, pub = np.zeros((1, 192)), np.zeros((1, 192), np.int32), np.zeros(8, np.int32)
    with pytest.raises(ValueError, match="1, 2, 4 or 8"):
        handle.selftest_sort_exact(3, capi.EXACT_ASCENDING, d2, pos, pub)
    with pytest.raises(ValueError, match="no mode"):
        handle.selftest_sort_exact(1, 3, d2[:, :64], pos[:, :64], pub)
    with pytest.raises(ValueError, match="outside"):
        handle.selftest_sort_exact(1, capi.EXACT_ASCENDING, d2[:, :64], pos[:, :64] + 8, pub)
    with pytest.raises(ValueError, match=r"\(1, 6\)"):
        handle.selftest_order_keys(1, 7, x[:1], np.zeros((1, 128)), np.zeros((1, 128), np.int32))


# ------------------------------------------------------------------------------------------------------ the exact sorters
N_PUB = 4096


def _positions(lists, n, rng):
    """n distinct positions in [0, N_PUB) per list, in random order (an odd multiplier is a bijection mod a power of two)."""
    j = rng.permuted(np.tile(np.arange(n), (lists, 1)), axis=1)
    return ((j * (2 * rng.integers(0, N_PUB // 2, size=(lists, 1)) + 1) + rng.integers(0, N_PUB, size=(lists, 1))) % N_PUB).astype(np.int32)


@functools.lru_cache(maxsize=None)
def exact_family(regs):
    """(d2, pos) lists of 64 regs for bitonic_sort_from, and the public index table.
    Orders: those of the 32-bit sorters (0-1 block patterns with both boundaries on multiples of `regs` or beside a
    register seam: all 2 080 for one register, the same density of cases for more), random permutations (4 096; 1 024 from
    four registers on).  d2 takes few values in the 0-1 lists -- exact fp64 ties by the hundred, pub decides -- and is
    distinct in the orders and permutations, where no lane ever sees a tie and key_less never looks pub up."""
    n = 64 * regs
    rng = np.random.default_rng(200 + regs)
    pub = rng.permutation(N_PUB).astype(np.int32)
    ranks = [orders(n)]
    ranks.append(np.argsort(rng.random((4096 if regs <= 2 else 1024, n)), axis=1))
    seams = {64 * m + s for m in range(1, regs) for s in (-1, 1)}
    ranks.append(block_patterns(n, set(range(0, n + 1, regs)) | seams))                     # two values of d2
    ranks.append(rng.integers(0, 5, size=(256, n)))                                        # a few values
    ranks.append(np.zeros((4, n), np.int64))                                               # one value: pub alone orders
    one_tie = np.argsort(rng.random((256, n)), axis=1)
    one_tie[one_tie == n - 1] = rng.integers(0, n - 1, size=256)                           # exactly one pair of equal d2 in the list
    ranks.append(one_tie)
    seam = (np.argsort(rng.random((128, n)), axis=1) + 1) // 2                             # sorted ranks 2j-1, 2j tie: 63|64, 127|128 ...
    ranks.append(seam)
    r = np.concatenate([np.asarray(x, np.int64) for x in ranks])
    d2 = (r + 1) * 1.0000000001e-3                                                         # monotone in the rank, both words of the double in use
    pos = _positions(len(r), n, rng)
    # +inf padding in every count from 0 to 64 regs, anywhere in the list
    pr = np.argsort(rng.random((n + 1, n)), axis=1)
    pd2 = (pr + 1) * 0.25
    ppos = _positions(n + 1, n, rng)
    padded = np.argsort(rng.random((n + 1, n)), axis=1) < np.arange(n + 1)[:, None]
    pd2[padded], ppos[padded] = np.inf, ne.INT_MAX
    d2, pos = np.concatenate([d2, pd2]), np.concatenate([pos, ppos])
    for a in (d2, pos, pub):
        a.setflags(write=False)
    return d2, pos, pub


@pytest.mark.parametrize("regs", [1, 2, 4, 8])
def test_exact_sort(handle, gpu, regs):
    capi = gpu["capi"]
    d2, pos, pub = exact_family(regs)
    for mode, desc in ((capi.EXACT_ASCENDING, False), (capi.EXACT_DESCENDING, True)):
        wd, wp = ne.exact_sort(d2, pos, pub, descending=desc)
        gd, gp = handle.selftest_sort_exact(regs, mode, d2, pos, pub)
        bad = np.flatnonzero((gp != wp).any(axis=1) | (gd != wd).any(axis=1))
        assert bad.size == 0, "R = %d, descending = %s: %d lists differ, first %d" % (regs, desc, bad.size, bad[0])


@pytest.mark.parametrize("regs", [1, 2, 4, 8])
def test_exact_merge_min(handle, gpu, regs):
    """best (ascending) and batch (descending) cut from one pool of 128 regs elements: batches that replace nothing,
    everything, every other element, random shares; ties across the two lists; padding in either in every count."""
    capi = gpu["capi"]
    n = 64 * regs
    rng = np.random.default_rng(300 + regs)
    pub = rng.permutation(N_PUB).astype(np.int32)
    cases = []                                                                             # (rank of the 2n pool elements, which go to best)
    ident = np.arange(2 * n)
    cases += [(ident, ident < n), (ident, ident >= n), (ident, ident % 2 == 0), (ident, ident % 2 == 1), (ident // 2, ident % 2 == 0), (ident // 4, ident % 2 == 0),
              (ident * 0, ident % 2 == 0)]
    for _ in range(256):
        share = np.zeros(2 * n, bool)
        share[rng.permutation(2 * n)[:n]] = True
        cases.append((ident if rng.random() < 0.5 else rng.integers(0, 2 * n, size=2 * n) // rng.integers(1, 9), share))
    B, C = [], []
    for r, share in cases:
        d2 = (np.asarray(r) + 1) * 0.37
        pos = rng.permutation(N_PUB)[:2 * n].astype(np.int32)
        B.append((d2[share], pos[share])), C.append((d2[~share], pos[~share]))
    for c in range(n + 1):                                                                 # padding: c in best, n - c and a random count in batch
        for cb in (n - c, int(rng.integers(0, n + 1))):
            d2 = (rng.integers(0, 2 * n, size=2 * n) + 1) * 0.37
            pos = rng.permutation(N_PUB)[:2 * n].astype(np.int32)
            bd, bp, cd, cp = d2[:n].copy(), pos[:n].copy(), d2[n:].copy(), pos[n:].copy()
            bd[:c], bp[:c], cd[:cb], cp[:cb] = np.inf, ne.INT_MAX, np.inf, ne.INT_MAX
            B.append((bd, bp)), C.append((cd, cp))
    best = ne.exact_sort(np.array([b[0] for b in B]), np.array([b[1] for b in B]), pub)
    batch = ne.exact_sort(np.array([c[0] for c in C]), np.array([c[1] for c in C]), pub, descending=True)
    wd, wp = ne.merge_min(best[0], best[1], batch[0], batch[1], pub)
    gd, gp = handle.selftest_sort_exact(regs, capi.EXACT_MERGE_MIN, best[0], best[1], pub, batch=batch)
    bad = np.flatnonzero((gp != wp).any(axis=1) | (gd != wd).any(axis=1))
    assert bad.size == 0, "R = %d: %d lists differ, first %d" % (regs, bad.size, bad[0])


# ------------------------------------------------------------------------------------------------------------ the repair
def _repair_list(regs, sb, runs, n_real, rng):
    """A list of 64 regs elements sorted by key, n_real of them real: one key per position except inside the runs
    [(start, length, order, d2 kind)] -- order 'reversed' | 'random' against the exact order, d2 'distinct' | 'equal' (pub
    decides) | 'mixed'.  Payloads are drawn from the whole range of slot_bits."""
    n = 64 * regs
    keys = 2 * np.arange(n, dtype=np.uint32) + 7
    pay = rng.permutation(1 << sb)[:n].astype(np.uint32)
    d2 = rng.random(1 << sb) * 4.0
    pub = rng.permutation(1 << sb).astype(np.int64)
    for start, length, order, kind in runs:
        sl = slice(start, start + length)
        keys[sl] = keys[start]
        p = pay[sl]
        d2[p] = {"distinct": rng.permutation(length) * 0.125 + 1.0, "equal": np.full(length, 2.5), "mixed": rng.integers(0, 3, size=length) * 0.5}[kind]
        exact = p[np.lexsort((pub[p], d2[p]))]
        pay[sl] = exact[::-1] if order == "reversed" else exact[rng.permutation(length)]
    e = (keys << np.uint32(sb)) | pay
    e[n_real:] = PAD
    return e, d2, pub


@functools.lru_cache(maxsize=None)
def repair_family(regs, sb):
    n = 64 * regs
    rng = np.random.default_rng(400 + 16 * regs + sb)
    L = []
    for length in range(2, 41):
        starts = {0, 1, 10, 11}                                                    # the head, both parities
        if regs == 2:
            starts |= {64 - length // 2, 63 - length // 2, 63, 65 - length}        # over position 63 | 64
        for start in sorted(s for s in starts if s >= 0 and s + length <= n):
            for order in ("reversed", "random"):
                for kind in ("distinct", "equal", "mixed"):
                    L.append(_repair_list(regs, sb, [(start, length, order, kind)], n, rng))
        for start in (3, 4):                                                       # the run ends where the padding begins
            L.append(_repair_list(regs, sb, [(start, length, "reversed", "distinct")], start + length, rng))
            L.append(_repair_list(regs, sb, [(start, length, "random", "mixed")], start + length, rng))
    for _ in range(96):                                                            # two and three adjacent runs of different keys
        lens = rng.integers(2, 21, size=int(rng.integers(2, 4)))
        start = int(rng.integers(0, n - lens.sum() + 1))
        runs, at = [], start
        for ln in lens:
            runs.append((at, int(ln), ("reversed", "random")[int(rng.integers(2))], ("distinct", "equal", "mixed")[int(rng.integers(3))]))
            at += int(ln)
        L.append(_repair_list(regs, sb, runs, int(rng.integers(at, n + 1)), rng))
    for n_real in (n, n - 1, n // 2, 1, 0):                                        # no equal keys at all
        L.append(_repair_list(regs, sb, [], n_real, rng))
    e, d2, pub = (np.array([l[j] for l in L]) for j in range(3))
    quiet = len(L) - 5
    for a in (e, d2, pub):
        a.setflags(write=False)
    return e, d2, pub, quiet


@pytest.mark.parametrize("regs,sb", [(1, 6), (1, 9), (2, 7), (2, 10)])
def test_order_equal_keys(handle, regs, sb):
    e, d2, pub, quiet = repair_family(regs, sb)
    want, want_flag = ne.repair(e, d2, pub, sb, regs)
    # the family reaches both answers, and part 1's theorem in its own terms: True for every run of at most 34
    run = ne.runs_of(e, sb)
    longest = np.array([np.bincount(r).max() for r in run])
    assert want_flag[longest <= ne.ORDER_PASSES - 2].all() and (~want_flag).any() and want_flag[quiet:].all()
    assert np.array_equal(want[quiet:], e[quiet:])
    got, flag = handle.selftest_order_keys(regs, sb, e, d2, pub)
    bad = np.flatnonzero((got != want).any(axis=1) | (flag != want_flag))
    assert bad.size == 0, "(%d, %d): %d lists differ from the restated repair, first %d: flag %s for %s" % (regs, sb, bad.size, bad[0], flag[bad[0]], want_flag[bad[0]])


# -------------------------------------------------------------------------------------------------------------- the state
def test_hooks_touch_nothing_resident(gpu):
    capi = gpu["capi"]
    h = capi.Handle(0)
    try:
        pts = gpu["shapes"].torus_random(4000, seed=11)
        h.set_points(pts)
        h.curvature(20)
        before = h.get_neighbors(0, len(pts)) + h.get_fit(0, len(pts))
        x = sorter_family(64)[0][:64]
        h.selftest_sort(capi.NET_PAIR, x)
        h.selftest_sort(capi.NET_DUO, sorter_family(128)[0][:64])
        d2, pos, pub = exact_family(2)
        h.selftest_sort_exact(2, capi.EXACT_ASCENDING, d2[:64], pos[:64], pub)
        e, t, p, _ = repair_family(2, 7)
        h.selftest_order_keys(2, 7, e[:64], t[:64], p[:64])
        after = h.get_neighbors(0, len(pts)) + h.get_fit(0, len(pts))
        for a, b in zip(before, after):
            assert (a is None and b is None) or a.tobytes() == b.tobytes()
    finally:
        h.close()

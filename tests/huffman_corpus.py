"""Adversarial byte histograms for the Huffman table builders, shared by tests/test_huffman_corpus_host.py (the serial host
statement: huf_build_pm, huf_write_tree of zstd_entropy.h) and tests/test_gpu_huffman_tables.py (the three wave-parallel
instantiations of region_plan / huf_build_wave / huf_write_tree_wave in zstd_encode.hip).  Pure numpy; the two searched families ask
the host statement (entropy_host) which histograms take the tree writer's side exits.

regions() returns Region tuples: a name, a family, the bytes, and the histogram they realise.  The bytes are a fixed-seed arrangement of
the multiset: a shuffle, and where one value holds more than a third of the region that value dealt into the gaps between the others at
most MAX_RUN to a gap -- the encoder's tokeniser turns every run of RMIN (12) or more EQUAL bytes into a sequence (zstd_encode.hip:
tokenise_runs; any value, not only zero), after which the literals are no longer the region.  `runs` says that an arrangement without such
runs does not exist (or, for the three zero-dominated regions, was not wanted): those are held to the round trip only.

Sizes: a region compared bit for bit stays below 32 KB or below 240 distinct values, so that the encoder's sampled histogram
(HIST_SAMPLE_FROM, HIST_SAMPLE_SEEN) is never used; the `sampled` regions (>= 32 KB, >= 240 values) get the weaker check.

What the searches found (20 000 random complete codes over up to 256 symbols, through entropy_host.weights_report): fse_normalize's
second method for 0.2 % of them, all above 180 symbols; a description that does not pay never above 128 symbols (the FSE-coded weights of
130 .. 170 symbols take 47 .. 65 bytes, just under half the alphabet) -- above 128 "no tree" is reached through the all-equal exit only
(256 symbols; a list of 129 weights or more cannot hold every value once), and "does not pay" below 128 falls to direct weights."""
import collections
import functools

import numpy as np

RMIN = 12        # vbz_kernels.h: the shortest run of equal bytes the encoder turns into a sequence
MAX_RUN = 8      # what the arrangements here aim for
SAMPLE_FROM, SAMPLE_SEEN = 32 << 10, 240   # zstd_encode.hip: HIST_SAMPLE_FROM, HIST_SAMPLE_SEEN

Region = collections.namedtuple("Region", "name family data counts runs sampled")


def longest_run(data):
    if len(data) == 0:
        return 0
    edges = np.flatnonzero(np.diff(data.astype(np.int16)) != 0)
    return int(np.diff(np.concatenate([[-1], edges, [len(data) - 1]])).max())


def arrange(counts, seed, plain=False):
    """the multiset `counts` as bytes in a fixed pseudo-random order, without a run of RMIN equal bytes if that can be had"""
    counts = np.asarray(counts, np.int64)
    data = np.repeat(np.arange(256, dtype=np.uint8), counts)
    top = int(np.argmax(counts))
    D, m = int(counts[top]), int(len(data) - counts[top])
    for attempt in range(32):
        rng = np.random.default_rng([seed, attempt])
        if plain or 3 * D <= len(data) or m == 0:
            out = rng.permutation(data)
        else:
            cap = MAX_RUN if D <= MAX_RUN * (m + 1) else RMIN - 1
            if D > cap * (m + 1):
                return rng.permutation(data)
            gaps = np.bincount(rng.choice(cap * (m + 1), D, replace=False) // cap, minlength=m + 1)
            vals = np.full(2 * m + 1, top, np.uint8)
            vals[1::2] = rng.permutation(data[data != top])
            reps = np.ones(2 * m + 1, np.int64)
            reps[0::2] = gaps
            out = np.repeat(vals, reps)
        if plain or longest_run(out) < RMIN:
            return out
    return out


def hist(symbols, counts):
    h = np.zeros(256, np.int64)
    h[np.asarray(symbols, np.int64)] = np.asarray(counts, np.int64)
    return h


def off_zero(h):
    """the histogram with byte 0's count swapped away if it is above a quarter: to the lightest value below the largest"""
    h = h.copy()
    if 4 * h[0] > h.sum():
        top = int(np.flatnonzero(h).max())
        k = 1 + int(np.argmin(h[1:top])) if top > 1 else top
        h[0], h[k] = h[k], h[0]
    return h


def fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def complete_code_lengths(rng, n, limit=11):
    """code lengths of a random complete prefix code over n symbols, none above `limit`"""
    lens = [1, 1]
    while len(lens) < n:
        i = int(rng.integers(0, len(lens)))
        if lens[i] < limit:
            l = lens.pop(i) + 1
            lens += [l, l]
    return lens


def plan_estimate(h, nblk=1):
    """region_plan's verdict for a region with the exact histogram h coded in nblk blocks: (mode, estimate) -- mode 'rle', 'raw' or
    'huffman', estimate = the bytes it expects of Huffman coding (None where it never gets that far).  The host statement's lengths and
    tree size; the same arithmetic as zstd_encode.hip: region_plan."""
    import entropy_host as E

    h = np.asarray(h, np.int64)
    S = int(h.sum())
    if h.max() == S:
        return "rle", None
    if S <= 63 or h.max() <= (S >> 7) + 4:
        return "raw", None
    tl, nb, tree = E.tree_description_counts(h, package_merge=True)
    if tree is None:
        return "raw", None
    est = (int((h * nb.astype(np.int64)).sum()) >> 3) + len(tree) + 14 * nblk
    return ("huffman" if est + (S >> 6) + 2 < S else "raw"), est


def _searched():
    """(name, histogram) of the families found by asking the host statement: complete codes whose weight lists make fse_normalize take
    its second method (realised by the dyadic histogram 2^(11 - length): the only optimal code for it is the one drawn), the same looked
    for among Dirichlet histograms, and the pair of 600-byte regions on either side of est + minGain < S"""
    import entropy_host as E

    out = []
    rng = np.random.default_rng(20261018)
    found = 0
    for _ in range(6000):
        if found == 4:
            break
        n = int(rng.integers(180, 257))
        lens = rng.permutation(complete_code_lengths(rng, n))
        syms = np.sort(rng.choice(np.arange(1, 256), n, replace=False)) if n < 256 else np.arange(256)
        nb = np.zeros(256, np.uint8)
        nb[syms] = lens
        if E.weights_report(nb, int(syms[-1]), int(lens.max()))[0] == 2:
            h = hist(syms, 4 << (11 - lens.astype(np.int64)))   # 8 192 bytes: the limit is 11 from 4 097 bytes on
            tl, nb2, tree = E.tree_description_counts(h, package_merge=True)
            assert (nb2 == nb).all() and tl == lens.max()
            out.append(("second_method_%d" % found, h))
            found += 1
    rng = np.random.default_rng(20261019)
    found = 0
    for _ in range(1500):   # (a bonus: one in some thousands; none is required)
        if found == 2:
            break
        n, S = int(rng.integers(150, 257)), int(rng.integers(4000, 32768))
        h = off_zero(hist(np.sort(rng.choice(256, n, replace=False)), 1 + rng.multinomial(S - n, rng.dirichlet(np.full(n, 1.0)))))
        tl, nb, tree = E.tree_description_counts(h, package_merge=True)
        if E.weights_report(nb, int(np.flatnonzero(h).max()), tl)[0] == 2:
            out.append(("second_method_dirichlet_%d" % found, h))
            found += 1
    # 600 bytes, one value twelve times (past the "probably not compressible" rule) and the rest spread evenly over ever fewer values:
    # the largest alphabet that pays and the next larger one, which is given up for its estimate
    prev = None
    for distinct in range(250, 20, -2):
        h = _small(600, distinct, 12, 600 + distinct)
        mode, est = plan_estimate(h)
        assert est is not None
        if mode == "huffman":
            if prev is not None:
                out.append(("small600_just_not_paying", prev))
            out.append(("small600_just_paying", h))
            break
        prev = h
    return out


def _small(S, distinct, max_count, seed):
    """S bytes over `distinct` values (anywhere but 0), one of them max_count times, the others as evenly as S allows"""
    rng = np.random.default_rng(seed)
    syms = np.sort(rng.choice(np.arange(1, 256), distinct, replace=False))
    rest = S - max_count
    c = np.full(distinct - 1, rest // (distinct - 1), np.int64)
    c[: rest % (distinct - 1)] += 1
    assert c.max() < max_count and c.min() >= 1
    return hist(syms, np.concatenate([[max_count], rng.permutation(c)]))


@functools.lru_cache(maxsize=1)
def regions():
    fam = []   # (family, name, histogram, plain shuffle)

    def add(family, name, h, plain=False):
        fam.append((family, name, np.asarray(h, np.int64), plain))

    # Fibonacci counts: the unlimited Huffman code is a comb of depth n - 1, far above the limit optimal_table_log gives (11 symbols and
    # more).  One size for each limit value 5 .. 11; the 21 counts also on the last symbols (an FSE-coded tree instead of a direct one)
    for n in (9, 11, 12, 13, 15, 16, 17, 21):
        add("fibonacci", "fibonacci_%d" % n, hist(np.arange(1, n + 1), fib(n)[::-1] if n % 2 else fib(n)))
    add("fibonacci", "fibonacci_21_high", hist(np.arange(235, 256), fib(21)))
    add("fibonacci", "fibonacci_21_high_descending", hist(np.arange(235, 256), fib(21)[::-1]))
    # powers of two, each twice: ties at every package weight
    p2 = [1 << (k // 2) for k in range(28)]
    add("powers", "powers_twice", hist(np.arange(3, 31), p2))
    add("powers", "powers_twice_descending_spread", hist(np.arange(255, 255 - 9 * 28, -9), p2))
    # all-equal counts.  Exactly equal counts never pass libzstd's "probably not compressible" rule from 128 symbols on
    # (maxCount <= (S >> 7) + 4); the `bump` variants give one symbol ten more, which leaves every code length where it was
    for n, c in ((64, 40), (128, 40), (65, 40), (129, 40), (200, 40), (255, 7), (256, 40)):
        add("equal", "equal_%d" % n, hist(np.arange(n), np.full(n, c)))
    for n, c in ((64, 20), (128, 20), (129, 20), (256, 20)):
        cc = np.full(n, c)
        cc[n // 2] += 10
        add("equal", "equal_%d_bump" % n, hist(np.arange(n), cc))
    add("equal", "equal_256_jitter", hist(np.arange(256), 30 + np.random.default_rng(10).integers(0, 20, 256)))
    # (256 symbols with words of one length have no description at all.  region_plan never gets that far: the largest count would have
    # to be above twice the mean for the "probably not compressible" rule and below twice the smallest for the equal lengths)
    # one dominant symbol and 254 / 255 singletons
    add("dominant", "dominant_first_254", hist(np.arange(1, 256), [1500] + [1] * 254))
    add("dominant", "dominant_last_254", hist(np.arange(1, 256), [1] * 254 + [1500]))
    add("dominant", "dominant_last_255", hist(np.arange(256), [1] * 255 + [1500]))
    add("dominant", "dominant_first_255", hist(np.arange(256), [80] + [1] * 255))   # (byte 0: at most a quarter)
    # counts 1 .. 255: the largest is 1 / 128 of the sum, which region_plan's "probably not compressible" rule stores raw -- the host
    # statement still codes them; 4 x (1 .. 127) is the same shape past that rule
    add("ramp", "ramp_ascending", hist(np.arange(1, 256), np.arange(1, 256)))
    add("ramp", "ramp_descending", hist(np.arange(1, 256), np.arange(255, 0, -1)))
    add("ramp", "ramp_127_ascending", hist(np.arange(129, 256), 4 * np.arange(1, 128)))
    add("ramp", "ramp_127_descending", hist(np.arange(1, 255, 2), 4 * np.arange(127, 0, -1)))
    # a stair: eight levels x 32 symbols
    add("stair", "stair", hist(np.arange(256), np.repeat(1 << np.arange(8), 32)))
    add("stair", "stair_interleaved", hist(np.arange(256), np.tile(1 << np.arange(8), 32)))
    # few symbols
    add("few", "two_0_255_equal", hist([0, 255], [2000, 2000]))
    add("few", "two_0_1_equal", hist([0, 1], [2000, 2000]))
    add("few", "two_0_255_unequal", hist([0, 255], [1000, 3000]))
    add("few", "two_0_1_unequal", hist([0, 1], [600, 2400]))
    add("few", "two_254_255_ten_to_one", hist([254, 255], [300, 3000]))
    add("few", "three", hist([0, 7, 255], [500, 1000, 2500]))
    add("few", "three_low", hist([0, 1, 2], [900, 1100, 2000]))
    add("few", "six_low", hist(np.arange(6), [500, 510, 520, 250, 120, 110]))   # its description does not pay: direct weights
    add("few", "one_symbol", hist([7], [3000]))
    # every weight once: 1, 2, 4 .. 512, 1 (x 8) on the symbols 0 .. 10 -- one of the two longest codes on the largest symbol, no symbol
    # absent below it, so that the weights written are all different: direct weights (above 128 symbols no list is that short)
    add("once", "weights_once_11", hist(np.arange(11), [8 << k for k in range(10)] + [8]))
    add("once", "weights_once_4", hist(np.arange(4), [100, 200, 400, 100]))
    # symbol placement: the lanes and register indices of the sort's key layout (symbol = 4 * lane + j)
    rng = np.random.default_rng(11)
    add("placement", "top_lanes", hist(np.arange(192, 256), rng.integers(1, 400, 64)))
    add("placement", "register_3", hist(np.arange(3, 256, 4), rng.integers(1, 400, 64)))
    add("placement", "register_0_ties", hist(np.arange(4, 256, 4), np.repeat([3, 9, 27, 81, 243, 300, 300], 9)))
    # small regions, on both sides of maxCount <= (S >> 7) + 4
    add("small", "small63", _small(63, 40, 6, 1))
    for S, distinct in ((64, 40), (65, 40), (300, 120), (600, 240)):
        t = (S >> 7) + 4
        add("small", "small%d_at_rule" % S, _small(S, distinct, t, S))
        add("small", "small%d_over_rule" % S, _small(S, distinct, t + 1, S + 1))
    add("small", "small_skewed_40",hist(np.arange(100, 140), np.maximum(1, (130 * 0.8 ** np.arange(40)).astype(np.int64))))
    for name, h in _searched():
        add("small" if name.startswith("small") else "searched", name, h)
    # random histograms
    rng = np.random.default_rng(12)
    for alpha in (0.02, 0.05, 0.3, 1.0, 5.0):
        for k in range(8):
            n = int(rng.integers(2, 257))
            S = int(rng.integers(max(64, n), 32768))
            c = 1 + rng.multinomial(S - n, rng.dirichlet(np.full(n, alpha)))
            add("random", "dirichlet_%g_%d" % (alpha, k), off_zero(hist(np.sort(rng.choice(256, n, replace=False)), c)))
    # sampled shapes: 32 KB and more with 240 values and more (the encoder may build their table from a quarter of the bytes)
    add("sampled", "sampled_squares", hist(np.arange(1, 256), 1 + np.arange(1, 256) ** 2 // 80))
    add("sampled", "sampled_stair_x8", hist(np.arange(256), 8 * np.repeat(1 << np.arange(8), 32)))
    add("sampled", "sampled_dirichlet", off_zero(hist(np.arange(256), 1 + rng.multinomial(120000 - 256, rng.dirichlet(np.full(256, 0.3))))))
    add("sampled", "sampled_bell", hist(np.arange(256), 1 + np.floor(50000 * np.exp(-0.5 * ((np.arange(256) - 128) / 30.0) ** 2) / 75.2)))
    # byte 0 dominates, plain shuffles: long zero runs become sequences -- round trip only
    add("zeros", "zeros_90", hist(np.arange(64), [9000] + [16] * 62 + [8]), plain=True)
    add("zeros", "zeros_99", hist([0, 1, 255], [20000, 100, 100]), plain=True)
    add("zeros", "zeros_60_all_values", hist(np.arange(256), [6000] + list(4 + np.arange(255) % 29)), plain=True)
    out = []
    for k, (family, name, h, plain) in enumerate(fam):
        data = arrange(h, 1000 + k, plain)
        assert (np.bincount(data, minlength=256) == h).all()
        out.append(Region(name, family, data, h, longest_run(data) >= RMIN, len(data) >= SAMPLE_FROM and np.count_nonzero(h) >= SAMPLE_SEEN))
    assert len(set(r.name for r in out)) == len(out)
    return tuple(out)

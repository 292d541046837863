"""The numpy statements of the four pile-up rules (include/vbz_gpu_pile.h: vbz_gpu_levels_pile_batch, vbz_gpu_squiggle_kmers_batch,
vbz_gpu_pile_kmers_batch, vbz_gpu_model_update_batch) and the catalogues of planted tables the tests run: test_pile_ref holds the
statements to plain Python loops, Python integers and Python floats and counts the catalogues, the tests on the MI355X hold the device to
the statements bit for bit -- the sums are integers, so every comparison is exact.

Tables are plain numpy.  A pile: uint64 [4, n_cells], the planes count word (kept + 2^32 skipped), n_samples, sum (two's complement),
sumsq; every add modulo 2^64.  The position pile has n_cells = G * target_stride and cell g * target_stride + j, the k-mer pile 4 ** k.
pairs / hit / n_levels / levels / target_len are squiggle_ref's; fit is uint32 [pairs, 4] (offset bits, scale bits, used, ok) or None."""
import numpy as np

import squiggle_ref as R

CLEAR, REQUIRE_OK, DIRECT = 1, 2, 4
MARK = 0xFFFFFFFF
U_MAX = float(1 << 24)
SKIP = np.uint64(1 << 32)
TILE = 4096    # a workgroup's positions in the k-mer kernel; which k keep their table in LDS is the kernel's to say: every k runs both forms


# ---- vbz_gpu_levels_pile_batch ----------------------------------------------------------------------------------------------------------
def fixed(w):
    """(keep bool, u int64) of float64 values w: kept when |w| <= 2^24 holds, u = rint(w)"""
    w = np.asarray(w, np.float64)
    with np.errstate(invalid="ignore"):
        keep = np.abs(w) <= U_MAX
    return keep, np.rint(np.where(keep, w, 0.0)).astype(np.int64)


def level_values(rec, o, s, fix, min_samples, max_entries):
    """(keep bool [W], u int64 [W], n_samples uint64 [W]) of the records uint32 [W, 8] under the pair's constants o, s (float32)"""
    ns, ne = rec[:, 2].astype(np.int64), rec[:, 3].astype(np.int64)
    total = np.ascontiguousarray(rec[:, 4:6]).view(np.int64)[:, 0]
    keep = ns >= max(int(min_samples), 1)
    if max_entries:
        keep &= ne <= int(max_entries)
    f = np.float64
    with np.errstate(over="ignore", invalid="ignore"):
        m = total.astype(f) / np.maximum(ns, 1).astype(f)
        v = (m + f(np.float32(o))) * f(np.float32(s))
        w = v * f(np.float32(fix))
    inside, u = fixed(w)
    keep &= inside
    return keep, np.where(keep, u, 0), ns.astype(np.uint64)


def levels_pile(pairs, hit, n_levels, levels, target_len, target_stride, n_reads, max_width, min_samples, max_entries, fix, fit=None, flags=0, pile=None):
    """-> pile uint64 [4, G * target_stride]; pile: what the arena held (None or CLEAR: zeros)"""
    n_cells = len(target_len) * target_stride
    out = np.zeros((4, n_cells), np.uint64) if pile is None or flags & CLEAR else np.array(pile, np.uint64).reshape(4, n_cells)
    for p in range(len(pairs)):
        W = int(n_levels[p])
        if not R.pair_valid(pairs[p], hit[p], W, target_len, target_stride, n_reads, max_width):
            continue
        o, s = np.float32(0), np.float32(1)
        if fit is not None:
            if flags & REQUIRE_OK and int(fit[p][3]) == 0:
                continue
            o, s = np.asarray(fit[p][:2], np.uint32).view(np.float32)
        keep, u, ns = level_values(levels[p, :W], o, s, fix, min_samples, max_entries)
        c0 = int(pairs[p][1]) * target_stride + int(hit[p][2])
        cells = slice(c0, c0 + W)   # (a pair's cells are distinct: plain adds)
        with np.errstate(over="ignore"):
            out[0, cells] += np.where(keep, np.uint64(1), SKIP)
            out[1, cells] += np.where(keep, ns, np.uint64(0))
            out[2, cells] += u.astype(np.uint64)
            out[3, cells] += (u * u).astype(np.uint64)
    return out


class PileCall:
    """one call of vbz_gpu_levels_pile_batch; add() plants a pair: its stretch of a target row, its level records and its fit record"""

    def __init__(self, name, target_len, target_stride, max_width, n_reads=None, min_samples=0, max_entries=0, fix=256.0, flags=0, use_fit=False, before=None):
        self.name, self.target_len, self.T, self.W = name, np.asarray(target_len, np.uint32), target_stride, max_width
        self.min_samples, self.max_entries, self.fix, self.flags, self.use_fit, self.n_reads = min_samples, max_entries, fix, flags, use_fit, n_reads
        self.before = before   # what the arena holds in front of the call: None zeros, else uint64 [4, n_cells]
        self.pairs, self.hit, self.n_levels, self.rec, self.fit = [], [], [], [], []

    @property
    def n_cells(self):
        return len(self.target_len) * self.T

    def add(self, ref, start, rec, read=None, end=None, W=None, fit=(0.0, 1.0, 1)):
        W = len(rec) if W is None else W
        self.pairs.append((len(self.pairs) if read is None else read, ref, 0, 0))
        self.hit.append((3, start + len(rec) if end is None else end, start, 9))
        self.n_levels.append(W)
        self.rec.append(rec)
        self.fit.append(fit)
        return self

    def arrays(self):
        P = len(self.pairs)
        levels = np.zeros((P, self.W, 8), np.uint32)
        levels[:, :, 6] = 0xABCDEF01   # rows behind n_levels: nobody reads them
        for p, rec in enumerate(self.rec):
            levels[p, :min(len(rec), self.W)] = rec[:self.W]
        fit = None
        if self.use_fit:
            fit = np.zeros((P, 4), np.uint32)
            for p, (o, s, ok) in enumerate(self.fit):
                fit[p] = np.array([o, s], np.float32).view(np.uint32).tolist() + [7, ok]
        n_reads = P if self.n_reads is None else self.n_reads
        return (np.asarray(self.pairs, np.uint32).reshape(P, 4), np.asarray(self.hit, np.uint32).reshape(P, 4), np.asarray(self.n_levels, np.uint32), levels,
                n_reads, fit)

    def expected(self):
        pairs, hit, n_levels, levels, n_reads, fit = self.arrays()
        return levels_pile(pairs, hit, n_levels, levels, self.target_len, self.T, n_reads, self.W, self.min_samples, self.max_entries, self.fix, fit, self.flags,
                           self.before)


def mean_records(rng, mean, ns=None, ne=None):
    """records whose sums are round(mean * ns)"""
    W = len(mean)
    ns = rng.integers(3, 40, W) if ns is None else np.asarray(ns)
    return R.records(ns, np.ones(W, np.int64) if ne is None else ne, np.rint(np.asarray(mean, np.float64) * ns).astype(np.int64))


def dirty(rng, n_cells):
    """an arena that holds something: every plane, both halves of the count word, sums near wrapping"""
    d = rng.integers(0, 1 << 40, (4, n_cells)).astype(np.uint64)
    d[2, ::3] = np.uint64((1 << 64) - 12345)   # a negative sum
    d[3, ::5] = np.uint64((1 << 64) - 1)       # a sumsq that wraps with the next add
    d[0, ::7] = np.uint64((1 << 32) - 1)       # a count whose low half carries into the high half
    return d


MAX_WIDTH = 136


def pile_cases():
    rng = np.random.default_rng(2801)
    cases = []
    T = 352
    lens3 = [340, 340, 333]
    # W = 1, 63, 64, 65, 129 and max_width; start at every residue of 4; G = 3; both signs of sum
    c = PileCall("widths and residues, G 3", lens3, T, MAX_WIDTH)
    for i, W in enumerate((1, 63, 64, 65, 129, MAX_WIDTH, 2, 7)):
        c.add(i % 3, i % 4 + 16 * (i % 5), mean_records(rng, rng.normal(0, 900, W)))
    c.add(2, 333 - 65, mean_records(rng, rng.normal(0, 900, 65)))   # ends at L_g exactly
    cases.append(c)
    # depth 1, 2, 64 and 300 pairs on one stretch, G = 1
    for depth in (1, 2, 64, 300):
        c = PileCall("depth %d on one stretch" % depth, [200], 208, MAX_WIDTH)
        for _ in range(depth):
            c.add(0, 37, mean_records(rng, rng.normal(0, 500, 130)))
        cases.append(c)
    # staggered overlaps: every pair one to three levels further, widths across a turn's seam
    c = PileCall("staggered overlaps", [340, 340], T, MAX_WIDTH)
    at = 0
    for i in range(90):
        W = int(rng.integers(50, 131))
        c.add(i % 2, at, mean_records(rng, rng.normal(0, 700, W)))
        at = (at + int(rng.integers(1, 4))) % (340 - 131)
    cases.append(c)
    # u at +-2^24 (kept) and beyond (skipped); means of both signs that round to ties
    c = PileCall("u at the bound", [64], 64, 8)
    ns = np.array([1, 4, 4, 4, 4, 2, 2, 8], np.int64)
    total = np.array([65536, 65536 * 4, -65536 * 4, 65536 * 4 + 1, -65536 * 4 - 1, 1, -1, 3], np.int64)
    c.add(0, 3, R.records(ns, np.ones(8, np.int64), total))
    c.add(0, 3, R.records(np.full(8, 512), np.ones(8, np.int64), np.array([1, -1, 3, -3, 5, -5, 7, -7])))   # w = +-0.5, 1.5, 2.5, 3.5: rint to even
    cases.append(c)
    # every skip condition alone, counted in the high half of the count word
    for name, kw, hurt in (("skip: n_samples < min_samples", {"min_samples": 5}, (2, 4)), ("skip: n_samples == 0", {}, (2, 0)),
                           ("skip: n_entries > max_entries", {"max_entries": 3}, (3, 4)), ("skip: |w| > 2^24", {}, (4, 1 << 30))):
        c = PileCall(name, [200], 208, MAX_WIDTH, **kw)
        for _ in range(3):
            rec = mean_records(rng, rng.normal(0, 300, 130), ns=np.full(130, 9))
            drop = [0, 63, 64, 129] + list(rng.integers(1, 129, 5))
            if hurt[0] == 4:
                rec[drop, 4:6] = np.array([hurt[1] * 9], np.int64).view(np.uint32)
            else:
                rec[drop, hurt[0]] = hurt[1]
            c.add(0, 11, rec)
        cases.append(c)
    # fit given: offsets and scales of every kind; REQUIRE_OK with ok = 0; a NaN and an infinite constant skip every level
    fits = [(0.0, 1.0, 1), (-12.5, 0.03125, 1), (700.0, 1.0 / 3.0, 0), (3.0, 2.0, 1), (float("nan"), 1.0, 1), (0.0, float("inf"), 0), (1e30, 1e-30, 1)]
    for name, flags in (("fit given", 0), ("fit given, REQUIRE_OK", REQUIRE_OK)):
        c = PileCall(name, [340, 340], T, MAX_WIDTH, flags=flags, use_fit=True)
        for i, f in enumerate(fits):
            c.add(i % 2, 5 * i, mean_records(rng, rng.normal(0, 800, 100)), fit=f)
        cases.append(c)
    c = PileCall("fit NULL: the records' constants are not read", [340, 340], T, MAX_WIDTH, use_fit=False)
    for i, f in enumerate(fits):
        c.add(i % 2, 5 * i, mean_records(rng, rng.normal(0, 800, 100)), fit=f)
    cases.append(c)
    # CLEAR over a dirty arena; adding to a dirty arena: wraps of sum and sumsq, the carry of the count word
    for name, flags in (("CLEAR over a dirty arena", CLEAR), ("added to a dirty arena", 0)):
        c = PileCall(name, [200, 150], 208, MAX_WIDTH, flags=flags, before=dirty(rng, 2 * 208))
        for i in range(6):
            c.add(i % 2, 9 * i, mean_records(rng, rng.normal(0, 500, 120)))
        cases.append(c)
    c = PileCall("no pairs, CLEAR", [200], 208, MAX_WIDTH, flags=CLEAR, before=dirty(rng, 208))
    cases.append(c)
    c = PileCall("no pairs", [200], 208, MAX_WIDTH, before=dirty(rng, 208))
    cases.append(c)
    # fix other than 256; wide sums as locate_levels may hand on
    c = PileCall("fix 1000.5, wrapped record sums", [200], 208, MAX_WIDTH, fix=1000.5)
    rec = mean_records(rng, rng.normal(0, 50, 64))
    rec[[2, 63], 4:6] = np.array([(1 << 63) - 5, -(1 << 63)], np.int64).view(np.uint32).reshape(2, 2)
    rec[7, 2] = 0xFFFFFFFF
    c.add(0, 10, rec)
    cases.append(c)
    return cases


def split_call(rng=None):
    """-> (whole, first, second): one call over the concatenated pairs, and the same pairs as two calls without CLEAR"""
    rng = rng or np.random.default_rng(2802)
    recs = [(i % 2, 7 * i, mean_records(rng, rng.normal(0, 600, int(rng.integers(20, 131))))) for i in range(24)]
    calls = []
    for name, part in (("whole", recs), ("first", recs[:10]), ("second", recs[10:])):
        c = PileCall("two calls: " + name, [340, 300], 352, MAX_WIDTH)
        for ref, start, rec in part:
            c.add(ref, start, rec)
        calls.append(c)
    return calls


def invalid_pair_calls():
    """every invalid-pair condition one at a time, in the middle of good pairs -> [(name, call)]: the bad pair touches nothing"""
    rng = np.random.default_rng(2803)
    out = []
    for name, kw, tl in (("read >= n_reads", {"read": 3}, None), ("read far out", {"read": 0xFFFFFFFF}, None), ("ref >= G", {"ref": 2}, None),
                         ("ref far out", {"ref": 0xFFFFFFFF}, None), ("W == 0", {"W": 0}, None), ("W > max_width", {"W": 41, "n_rec": 41}, None),
                         ("end - start != W", {"end": 61}, None), ("end < start", {"end": 10}, None), ("L_g == 0", {"ref": 1}, [120, 0]),
                         ("L_g > target_stride", {"ref": 1}, [120, 129]), ("L_g far out", {"ref": 1}, [120, 0xFFFFFFFF]), ("end > L_g", {"ref": 1}, [120, 59])):
        c = PileCall(name, tl or [120, 120], 128, 40, n_reads=3)
        c.add(0, 7, mean_records(rng, rng.normal(0, 100, 40)), read=0)
        n_rec = kw.pop("n_rec", 40)
        c.add(kw.pop("ref", 0), 20, mean_records(rng, rng.normal(0, 100, n_rec)), read=kw.get("read", 1), end=kw.get("end"), W=kw.get("W"))
        c.add(0, 50, mean_records(rng, rng.normal(0, 100, 40)), read=2)
        c.bad = 1
        out.append((name, c))
    return out


# ---- vbz_gpu_squiggle_kmers_batch -------------------------------------------------------------------------------------------------------
def squiggle_kmers(seq, seq_len, k, target_stride, flags):
    """-> (kmer uint32 [rows, target_stride], target_len uint32 [rows]): squiggle_ref.squiggle with the gather left out"""
    S, stride = seq.shape
    rows = 2 * S if flags & R.BOTH else S
    kmer, target_len = np.full((rows, target_stride), MARK, np.uint32), np.zeros(rows, np.uint32)
    for r in range(rows):
        s, rc = (r >> 1, bool(r & 1)) if flags & R.BOTH else (r, False)
        n = int(seq_len[s])
        if n > stride:
            continue
        L = n - k + 1 if k <= n else 0
        if L == 0 or L > target_stride:
            continue
        index, bad = R.kmers(R.strand(seq[s], n, rc), k)
        key = np.where(bad, MARK, index).astype(np.uint32)
        kmer[r, :L], target_len[r] = key[::-1] if flags & R.REVERSED else key, L
    return kmer, target_len


def kmers_cases():
    """squiggle_ref's catalogue, every k: the cases of k = 1, 2, 5, 6, 9 as they stand, and the seams again at k = 3, 4, 7, 8"""
    rng = np.random.default_rng(2804)
    cases = list(R.squiggle_cases())
    for k in (3, 4, 7, 8):
        seqs = [R.random_seq(rng, n) for n in R.seam_lengths(k)]
        base = R.random_seq(rng, R.WAVE + 40)
        hurt = [R.with_invalid(base, at) for at in list(range(0, 24)) + [R.LANE - 1 + i for i in range(k + 1)] + [R.WAVE - 1 + i for i in range(k + 1)]]
        for flags in (0, R.BOTH, R.REVERSED, R.BOTH | R.REVERSED):
            cases.append(R.SquiggleCall("k %d flags %d: every seam" % (k, flags), k, seqs, R.random_model(rng, k), flags))
            cases.append(R.SquiggleCall("k %d flags %d: invalid bases at every slot of a lane's bytes" % (k, flags), k, hurt, R.random_model(rng, k), flags))
    return cases


# ---- vbz_gpu_pile_kmers_batch -----------------------------------------------------------------------------------------------------------
def pile_kmers(pile, kmer, target_len, k, flags=0, kmer_pile=None):
    """pile uint64 [4, rows * target_stride], kmer uint32 [rows, target_stride] -> kmer_pile uint64 [4, 4 ** k]"""
    rows, T = kmer.shape
    cells = 4 ** k
    out = np.zeros((4, cells), np.uint64) if kmer_pile is None or flags & CLEAR else np.array(kmer_pile, np.uint64).reshape(4, cells)
    pile = np.asarray(pile, np.uint64).reshape(4, rows, T)
    for g in range(rows):
        L = int(target_len[g])
        if L > T:
            continue
        key = kmer[g, :L].astype(np.int64)
        live = key < cells
        for q in range(4):
            with np.errstate(over="ignore"):
                np.add.at(out[q], key[live], pile[q, g, :L][live])
    return out


class KmersPileCall:
    def __init__(self, name, k, kmer, target_len, pile, flags=0, before=None):
        self.name, self.k, self.kmer, self.target_len, self.pile, self.flags, self.before = name, k, kmer, np.asarray(target_len, np.uint32), pile, flags, before

    def expected(self):
        return pile_kmers(self.pile, self.kmer, self.target_len, self.k, self.flags, self.before)


def random_pile(rng, n_cells, zero_share=0.0):
    """a position pile as levels_pile leaves it: small counts, sums of both signs; a share of cells all zero"""
    p = np.zeros((4, n_cells), np.uint64)
    n, sk = rng.integers(0, 300, n_cells), rng.integers(0, 4, n_cells)
    p[0] = (n + (sk << 32)).astype(np.uint64)
    p[1] = rng.integers(0, 5000, n_cells).astype(np.uint64)
    p[2] = rng.integers(-(1 << 30), 1 << 30, n_cells).astype(np.int64).view(np.uint64)
    p[3] = rng.integers(0, 1 << 55, n_cells).astype(np.uint64)
    if zero_share:
        p[:, rng.random(n_cells) < zero_share] = 0
    return p


def pile_kmers_cases():
    rng = np.random.default_rng(2805)
    cases = []
    for k in range(1, 10):
        cells = 4 ** k
        for rows, L, T in ((1, 3000, 3008), (5, TILE + 300, TILE + 304)):   # (the second: more than one workgroup a row)
            kmer = rng.integers(0, cells, (rows, T)).astype(np.uint32)
            kmer[rng.random((rows, T)) < 0.02] = MARK
            lens = [L] + [int(v) for v in rng.integers(1, L, rows - 1)]
            cases.append(KmersPileCall("k %d rows %d" % (k, rows), k, kmer, lens, random_pile(rng, rows * T, 0.1)))
            cases.append(KmersPileCall("k %d rows %d DIRECT" % (k, rows), k, kmer, lens, random_pile(rng, rows * T, 0.1), flags=DIRECT))
    for k in (1, 5, 6, 9):
        cells, T = 4 ** k, 2 * TILE
        one = np.full((2, T), cells - 1, np.uint32)
        cases.append(KmersPileCall("k %d: every position on one k-mer" % k, k, one, [T, T - 5], random_pile(rng, 2 * T)))
        marks = np.full((2, T), MARK, np.uint32)
        marks[1, 7] = 0
        cases.append(KmersPileCall("k %d: marks, and keys at and beyond 4^k" % k, k, np.where(rng.random((2, T)) < 0.5, marks, np.uint32(cells)), [T, T],
                                   random_pile(rng, 2 * T)))
        kmer = rng.integers(0, cells, (3, 512)).astype(np.uint32)
        cases.append(KmersPileCall("k %d: target_len 0 and beyond the stride" % k, k, kmer, [0, 513, 0xFFFFFFFF], random_pile(rng, 3 * 512)))
        cases.append(KmersPileCall("k %d: target_len at the stride, CLEAR over a dirty arena" % k, k, kmer, [512, 1, 511], random_pile(rng, 3 * 512), flags=CLEAR,
                                   before=dirty(rng, cells)))
        cases.append(KmersPileCall("k %d: added to a dirty arena" % k, k, kmer, [512, 300, 511], random_pile(rng, 3 * 512), before=dirty(rng, cells)))
        cases.append(KmersPileCall("k %d: all-zero cells" % k, k, kmer, [512, 512, 512], np.zeros((4, 3 * 512), np.uint64), before=dirty(rng, cells)))
    return cases


# ---- vbz_gpu_model_update_batch ---------------------------------------------------------------------------------------------------------
def model_update(kmer_pile, prior, k, min_obs, fix):
    """kmer_pile uint64 [4, 4 ** k], prior uint32 [4 ** k] (bits) -> (model uint32 [4 ** k], sd uint32 [4 ** k]) (bits)"""
    f = np.float64
    kp = np.asarray(kmer_pile, np.uint64).reshape(4, 4 ** k)
    n = (kp[0] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    have = n >= max(int(min_obs), 1)
    nn = np.maximum(n, 1).astype(f)
    mean = kp[2].view(np.int64).astype(f) / nn
    var = kp[3].astype(f) / nn - mean * mean
    fx = f(np.float32(fix))
    with np.errstate(over="ignore"):
        m = (mean / fx).astype(np.float32)
        sd = (np.sqrt(np.maximum(var, 0.0)) / fx).astype(np.float32)
    return np.where(have, m.view(np.uint32), np.asarray(prior, np.uint32)), np.where(have, sd.view(np.uint32), np.uint32(0))


class UpdateCall:
    def __init__(self, name, k, kmer_pile, prior, min_obs=0, fix=256.0, use_sd=True, in_place=False):
        self.name, self.k, self.kmer_pile, self.prior = name, k, kmer_pile, np.asarray(prior, np.float32).view(np.uint32)
        self.min_obs, self.fix, self.use_sd, self.in_place = min_obs, fix, use_sd, in_place

    def expected(self):
        return model_update(self.kmer_pile, self.prior, self.k, self.min_obs, self.fix)


def observed_pile(rng, cells, n):
    """a k-mer pile of n[i] observations of u ~ N(mu_i, 40^2) each, skipped in the count word's high half"""
    p = np.zeros((4, cells), np.uint64)
    mu = rng.normal(0, 600, cells)
    for i in range(cells):
        u = np.rint(rng.normal(mu[i], 40, int(n[i]))).astype(np.int64)
        p[1, i], p[2, i], p[3, i] = int(n[i]) * 9, np.int64(u.sum()).view(np.uint64), int((u * u).sum())
    p[0] = (np.asarray(n, np.int64) + (rng.integers(0, 50, cells) << 32)).astype(np.uint64)
    return p


def update_cases():
    rng = np.random.default_rng(2806)
    cases = []
    special = R.special_model()   # k = 2: NaN with a payload, infinities, -0: the prior's 32 bits are kept
    n = np.array([0, 1, 7, 8, 9, 100, 0, 7, 8, 3000, 2, 1, 0, 8, 7, 9])
    for min_obs in (0, 1, 8):
        cases.append(UpdateCall("n on both sides of min_obs %d, a special prior" % min_obs, 2, observed_pile(rng, 16, n), special, min_obs=min_obs))
    # all observations equal: var rounds to a few ulp below or above zero; one observation: var 0
    p = np.zeros((4, 64), np.uint64)
    for i in range(64):
        u, cnt = int(rng.integers(-(1 << 24), (1 << 24) + 1)), int(rng.integers(1, 4000))
        p[0, i], p[2, i], p[3, i] = cnt, np.int64(u * cnt).view(np.uint64), u * u * cnt
    p[3, ::2] -= np.uint64(1)   # sumsq one short: var below zero by rounding AND by value
    cases.append(UpdateCall("equal observations: var at and below zero", 3, p, rng.normal(0, 2, 64)))
    for k in (1, 6, 9):
        cells = 4 ** k
        cnt = rng.integers(0, 30, cells)
        kp = observed_pile(rng, cells, cnt) if k < 9 else random_counts_pile(rng, cells)
        cases.append(UpdateCall("k %d" % k, k, kp, rng.normal(0, 2, cells), min_obs=10))
    cases.append(UpdateCall("sd NULL", 4, observed_pile(rng, 256, rng.integers(0, 30, 256)), rng.normal(0, 2, 256), min_obs=5, use_sd=False))
    cases.append(UpdateCall("prior in place", 4, observed_pile(rng, 256, rng.integers(0, 30, 256)), rng.normal(0, 2, 256), min_obs=5, in_place=True))
    cases.append(UpdateCall("fix 1000.5", 4, observed_pile(rng, 256, rng.integers(0, 30, 256)), rng.normal(0, 2, 256), min_obs=5, fix=1000.5))
    return cases


def random_counts_pile(rng, cells):
    """sums consistent with n observations of |u| <= 2^24, with no per-cell loop"""
    n = rng.integers(0, 30, cells)
    mu, spread = rng.normal(0, 600, cells), rng.uniform(0, 80, cells)
    total = np.rint(mu * n).astype(np.int64)
    p = np.zeros((4, cells), np.uint64)
    p[0] = (n + (rng.integers(0, 50, cells) << 32)).astype(np.uint64)
    p[1], p[2] = (n * 9).astype(np.uint64), total.view(np.uint64)
    p[3] = np.rint((mu * mu + spread * spread) * n).astype(np.uint64)
    return p

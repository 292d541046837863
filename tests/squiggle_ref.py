"""The numpy statements of the two pore-model rules (include/vbz_gpu.h: vbz_gpu_squiggle_batch, vbz_gpu_levels_fit_batch) and the
catalogues of planted tables the tests run: test_squiggle_ref holds the statements to plain Python loops, big integers and Python floats
and counts the catalogues, the tests on the MI355X hold the device to the statements bit for bit.

Tables are plain numpy.  A squiggle: seq uint8 [S, seq_stride], seq_len uint32 [S], model uint32 [4 ** k] (the floats' bits) -> target int8
[rows, target_stride], target_len uint32 [rows], masked uint32 [rows], level uint32 [rows, target_stride] (bits).  A fit: pairs / hit uint32
[pairs, 4], n_levels uint32 [pairs], levels uint32 [pairs, max_width, 8] (a record's eight words: first_sample, end_sample, n_samples,
n_entries, sum lo, sum hi, sumsq lo, sumsq hi), target int8 [G, target_stride], target_len uint32 [G], prior uint32 [n_reads, 2] (bits) or
None -> out uint32 [pairs, 4] (offset bits, scale bits, used, ok), sums int64 [pairs, 4]."""
import numpy as np

BOTH, REVERSED = 1, 2
INVALID = 4
CODE = np.full(256, INVALID, np.uint8)
for _letters, _code in (("Aa", 0), ("Cc", 1), ("Gg", 2), ("TtUu", 3)):
    for _ch in _letters:
        CODE[ord(_ch)] = _code
LANE, WAVE, BLOCK = 16, 1024, 4096   # the kernel's own cut: levels a lane, a wavefront, a workgroup


# ---- vbz_gpu_squiggle_batch -------------------------------------------------------------------------------------------------------------
def quantise(bits, quant):
    """the query's rule of the match calls over float32 bits -> int8"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(bits, np.uint32).view(np.float32) * np.float32(quant)
        r = np.clip(np.rint(v), np.float32(-127), np.float32(127))
    return np.where(np.isnan(v), np.float32(0), r).astype(np.int8)


def strand(row, n, rc):
    """the codes b_0 ... b_(n-1) of a strand: the row's first n bytes, or their reverse complement"""
    c = CODE[np.asarray(row[:n], np.uint8)]
    return np.where(c == INVALID, c, 3 - c)[::-1] if rc else c


def kmers(c, k):
    """(index int64 [L], bad bool [L]) of the k-mers of a strand of n >= k codes, L = n - k + 1"""
    L = len(c) - k + 1
    index, bad = np.zeros(L, np.int64), np.zeros(L, bool)
    for i in range(k):
        part = c[i:i + L]
        bad |= part == INVALID
        index = index * 4 + np.where(part == INVALID, 0, part)
    return index, bad


def squiggle(seq, seq_len, model, k, target_stride, quant, flags):
    """-> (target int8 [rows, target_stride], target_len uint32 [rows], masked uint32 [rows], level uint32 [rows, target_stride])"""
    S, stride = seq.shape
    rows = 2 * S if flags & BOTH else S
    target, level = np.zeros((rows, target_stride), np.int8), np.zeros((rows, target_stride), np.uint32)
    target_len, masked = np.zeros(rows, np.uint32), np.zeros(rows, np.uint32)
    model = np.asarray(model, np.uint32)
    for r in range(rows):
        s, rc = (r >> 1, bool(r & 1)) if flags & BOTH else (r, False)
        n = int(seq_len[s])
        if n > stride:
            continue
        L = n - k + 1 if k <= n else 0
        if L == 0 or L > target_stride:
            continue
        index, bad = kmers(strand(seq[s], n, rc), k)
        m = np.where(bad, np.uint32(0), model[index])
        q = np.where(bad, np.int8(0), quantise(m, quant))
        if flags & REVERSED:
            m, q = m[::-1], q[::-1]
        target[r, :L], level[r, :L], target_len[r], masked[r] = q, m, L, int(bad.sum())
    return target, target_len, masked, level


def revcomp(b):
    return bytes(b"ACGT"[3 - CODE[x]] for x in reversed(b))


class SquiggleCall:
    """one call of vbz_gpu_squiggle_batch: seqs are bytes objects; seq_len overrides the declared lengths"""

    def __init__(self, name, k, seqs, model, flags=0, quant=32.0, seq_stride=None, target_stride=None, seq_len=None, use_level=True, fill=0x4E):
        self.name, self.k, self.flags, self.quant, self.use_level = name, k, flags, quant, use_level
        longest = max(len(s) for s in seqs)
        self.seq_stride = seq_stride or (longest + 16) // 16 * 16
        self.target_stride = target_stride or (longest + 16) // 16 * 16
        self.seq = np.full((len(seqs), self.seq_stride), fill, np.uint8)   # behind a sequence: the caller's junk ('N' by default)
        for i, s in enumerate(seqs):
            self.seq[i, :min(len(s), self.seq_stride)] = np.frombuffer(s, np.uint8)[:self.seq_stride]
        self.seq_len = np.asarray(seq_len if seq_len is not None else [len(s) for s in seqs], np.uint32)
        self.model = np.asarray(model, np.float32).view(np.uint32)
        assert len(self.model) == 4 ** k
        self.rows = len(seqs) * (2 if flags & BOTH else 1)

    def expected(self):
        return squiggle(self.seq, self.seq_len, self.model, self.k, self.target_stride, self.quant, self.flags)


def random_seq(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n)) if n else b""


def random_model(rng, k, spread=3.0):
    """float32 levels of which a part lands past +-127 under quant 32"""
    return (rng.normal(0, spread, 4 ** k)).astype(np.float32)


def special_model():
    """k = 2: NaN, +-inf, -0, exact .5 ties under quant 32, values past +-127 and at them"""
    m = np.array([np.nan, np.inf, -np.inf, -0.0, 0.5 / 32, 1.5 / 32, 2.5 / 32, -0.5 / 32, -1.5 / 32, 126.5 / 32, 127.5 / 32, -127.5 / 32, 200.0, -200.0, 3.0,
                  1e-30], np.float32)
    m = m.view(np.uint32).copy()
    m[15] = 0x7FC12345   # a NaN with a payload: level keeps the 32 bits
    return m.view(np.float32)


def seam_lengths(k):
    """n with L = n - k + 1 on each side of every seam of the cut, and n at k - 1, k, k + 1"""
    Ls = [0, 1, 2, LANE - 1, LANE, LANE + 1, WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1]
    return sorted({L + k - 1 for L in Ls} | {0})


def with_invalid(s, at, byte=b"N"):
    return s[:at] + byte + s[at + 1:]


def squiggle_cases():
    rng = np.random.default_rng(2501)
    cases = []
    for k in (1, 2, 5, 6, 9):
        model = random_model(rng, k)
        seqs = [random_seq(rng, n) for n in seam_lengths(k)]
        for flags in (0, BOTH, REVERSED, BOTH | REVERSED):
            cases.append(SquiggleCall("k %d flags %d: every seam" % (k, flags), k, seqs, model, flags))
        # an invalid base at the first and the last position, and at each of the k positions of a k-mer that straddles a lane's and a tile's seam
        base = random_seq(rng, BLOCK + 40)
        hurt = [with_invalid(base, 0), with_invalid(base, len(base) - 1)]
        for seam in (LANE, WAVE, BLOCK):
            for i in range(k + 1):   # base seam - 1 + i masks the levels seam - k + i ... seam - 1 + i: each side of the seam, and both
                hurt.append(with_invalid(base, seam - 1 + i))
                hurt.append(with_invalid(base, len(base) - 1 - (seam - 1 + i)))   # (the same seen from the other end: the reverse strand, REVERSED)
        for flags in (BOTH, BOTH | REVERSED):
            cases.append(SquiggleCall("k %d flags %d: invalid bases at the seams" % (k, flags), k, hurt, model, flags))
    half = random_seq(rng, 700)
    pal = half + revcomp(half)
    cases.append(SquiggleCall("a palindrome: both rows equal", 5, [pal], random_model(rng, 5), BOTH))
    mixed = random_seq(rng, 3000)
    lower = bytes(rng.choice(np.frombuffer(b"ACGTacgtUu", np.uint8), 3000))
    cases.append(SquiggleCall("lower case and U", 6, [mixed, mixed.lower(), mixed.replace(b"T", b"U"), lower], random_model(rng, 6), BOTH))
    every = bytes(range(256)) * 3 + random_seq(rng, 100)
    for flags in (BOTH, REVERSED):
        cases.append(SquiggleCall("all 256 byte values, flags %d" % flags, 2, [every, bytes(rng.permutation(np.frombuffer(every, np.uint8)))], random_model(rng, 2), flags))
    some = [random_seq(rng, n) for n in (100, 64, 48, 200, 33)]
    # seq_len 0, above seq_stride (even 2^32 - 1), and L above target_stride; the junk behind a sequence is valid letters here
    cases.append(SquiggleCall("refused lengths", 5, some, random_model(rng, 5), BOTH | REVERSED, seq_stride=208, target_stride=64,
                              seq_len=[0, 209, 0xFFFFFFFF, 200, 68], fill=0x41))
    cases.append(SquiggleCall("L at target_stride", 5, some, random_model(rng, 5), BOTH, seq_stride=208, target_stride=64, seq_len=[68, 69, 4, 5, 208], fill=0x43))
    sp = random_seq(rng, 2000)
    for flags in (0, BOTH | REVERSED):
        cases.append(SquiggleCall("special values in the model, flags %d" % flags, 2, [sp, random_seq(rng, 17)], special_model(), flags))
    cases.append(SquiggleCall("no level arena", 6, [random_seq(rng, 5000), with_invalid(random_seq(rng, 1030), 500)], random_model(rng, 6), BOTH | REVERSED,
                              use_level=False))
    cases.append(SquiggleCall("quant 1.5", 5, [random_seq(rng, 1500)], random_model(rng, 5, 40.0), REVERSED, quant=1.5))
    long = bytearray(random_seq(rng, 70000))
    for at in rng.integers(0, 70000, 40):
        long[at] = 0x6E
    cases.append(SquiggleCall("70 000 bases at k 9", 9, [bytes(long)], random_model(rng, 9), BOTH))
    return cases


# ---- vbz_gpu_levels_fit_batch -----------------------------------------------------------------------------------------------------------
M_MAX = 32768.0


def pair_valid(pair, hit, W, target_len, target_stride, n_reads, max_width):
    read, ref = int(pair[0]), int(pair[1])
    end, start = int(hit[1]), int(hit[2])
    if read >= n_reads or ref >= len(target_len) or W == 0 or W > max_width or end <= start or end - start != W:
        return False
    Lg = int(target_len[ref])
    return Lg != 0 and Lg <= target_stride and end <= Lg


def kept_levels(rec, g, min_samples, max_entries):
    """(g int64 [K], q int64 [K]) of the levels a fit keeps; rec uint32 [W, 8]"""
    ns, ne = rec[:, 2].astype(np.int64), rec[:, 3].astype(np.int64)
    total = np.ascontiguousarray(rec[:, 4:6]).view(np.int64)[:, 0]
    keep = ns >= max(int(min_samples), 1)
    if max_entries:
        keep &= ne <= int(max_entries)
    m = total.astype(np.float64) / np.maximum(ns, 1).astype(np.float64)
    keep &= np.abs(m) <= M_MAX
    q = np.rint(np.where(keep, m, 0.0) * 64.0).astype(np.int64)
    return g.astype(np.int64)[keep], q[keep]


def integer_sums(g, q):
    return int(g.sum()), int((g * g).sum()), int(q.sum()), int((g * q).sum())


def line(K, sums, quant):
    """the float64 formula -> (offset, scale) as float32, or None without a good fit"""
    Sg, Sgg, Sq, Sgq = sums
    num, den = K * Sgq - Sg * Sq, K * Sgg - Sg * Sg
    if K < 2 or den <= 0 or num <= 0:
        return None
    f = np.float64
    A = f(num) / f(den)
    B = (f(Sq) - A * f(Sg)) / f(K)
    a, b = A / f(64), B / f(64)
    with np.errstate(over="ignore", divide="ignore"):
        scale, offset = np.float32(f(1.0) / (a * f(np.float32(quant)))), np.float32(-b)
    if not (np.isfinite(scale) and np.isfinite(offset) and scale > 0):
        return None
    return offset, scale


def prior_constants(prior, read, n_reads):
    """(offset, scale) float32 of a pair without a good fit; prior uint32 [n_reads, 2] bits or None"""
    if prior is None or read >= n_reads:
        return np.float32(0), np.float32(1)
    shift, scale = np.asarray(prior[read], np.uint32).view(np.float32)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        return np.float32(-shift), np.float32(np.float64(1) / np.float64(scale))


def levels_fit(pairs, hit, n_levels, levels, target, target_len, n_reads, max_width, min_samples, max_entries, quant, prior=None):
    """-> (out uint32 [pairs, 4], sums int64 [pairs, 4])"""
    P = len(pairs)
    out, sums = np.zeros((P, 4), np.uint32), np.zeros((P, 4), np.int64)
    for p in range(P):
        W, K, fit = int(n_levels[p]), 0, None
        if pair_valid(pairs[p], hit[p], W, target_len, target.shape[1], n_reads, max_width):
            start = int(hit[p][2])
            g, q = kept_levels(levels[p, :W], target[int(pairs[p][1]), start:start + W], min_samples, max_entries)
            K = len(g)
            sums[p] = integer_sums(g, q)
            fit = line(K, [int(v) for v in sums[p]], quant)
        offset, scale = fit if fit is not None else prior_constants(prior, int(pairs[p][0]), n_reads)
        out[p] = np.array([offset], np.float32).view(np.uint32)[0], np.array([scale], np.float32).view(np.uint32)[0], K, int(fit is not None)
    return out, sums


def records(ns, ne, total):
    """level records uint32 [W, 8] of (n_samples, n_entries, sum); first / end sample and sumsq carry patterns nobody reads"""
    W = len(ns)
    rec = np.zeros((W, 8), np.uint32)
    rec[:, 0], rec[:, 1] = np.arange(W) * 7, np.arange(W) * 7 + 5
    rec[:, 2], rec[:, 3] = ns, ne
    rec[:, 4:6] = np.asarray(total, np.int64).astype(np.int64).view(np.uint32).reshape(W, 2)
    rec[:, 6], rec[:, 7] = 0xDEADBEEF, 0x7FFFFFFF
    return rec


class FitCall:
    """one call of vbz_gpu_levels_fit_batch; add() plants a pair: its stretch of a target row and its level records"""

    def __init__(self, name, target, target_len, max_width, n_reads=None, min_samples=0, max_entries=0, quant=32.0, prior=None, use_sums=True):
        self.name, self.target, self.target_len = name, np.asarray(target, np.int8), np.asarray(target_len, np.uint32)
        self.W, self.min_samples, self.max_entries, self.quant, self.use_sums = max_width, min_samples, max_entries, quant, use_sums
        self.pairs, self.hit, self.n_levels, self.rec, self.n_reads, self.prior = [], [], [], [], n_reads, prior

    def add(self, ref, start, rec, read=None, end=None, W=None):
        W = len(rec) if W is None else W
        self.pairs.append((len(self.pairs) if read is None else read, ref, 0, 0))
        self.hit.append((3, start + len(rec) if end is None else end, start, 9))
        self.n_levels.append(W)
        self.rec.append(rec)
        return self

    def arrays(self):
        P = len(self.pairs)
        levels = np.zeros((P, self.W, 8), np.uint32)
        levels[:, :, 6] = 0xABCDEF01   # rows behind n_levels: nobody reads them
        for p, rec in enumerate(self.rec):
            levels[p, :min(len(rec), self.W)] = rec[:self.W]
        n_reads = P if self.n_reads is None else self.n_reads
        prior = None if self.prior is None else np.asarray(self.prior, np.float32).reshape(n_reads, 2).view(np.uint32)
        return np.asarray(self.pairs, np.uint32), np.asarray(self.hit, np.uint32), np.asarray(self.n_levels, np.uint32), levels, n_reads, prior

    def expected(self):
        pairs, hit, n_levels, levels, n_reads, prior = self.arrays()
        return levels_fit(pairs, hit, n_levels, levels, self.target, self.target_len, n_reads, self.W, self.min_samples, self.max_entries, self.quant, prior)


def line_records(rng, g, a, b, noise=0.0, ns=None, ne=None):
    """records whose means are a g + b (+ noise): sum = round(mean * ns)"""
    W = len(g)
    ns = rng.integers(3, 40, W) if ns is None else np.asarray(ns)
    mean = a * g.astype(np.float64) + b + (rng.normal(0, noise, W) if noise else 0.0)
    return records(ns, np.ones(W, np.int64) if ne is None else ne, np.rint(mean * ns).astype(np.int64))


def random_target(rng, G, L, stride):
    t = np.zeros((G, stride), np.int8)
    t[:, :L] = rng.integers(-127, 128, (G, L))
    return t


def extreme_call():
    """|g| = 128, |m| = 32768, K = 65 536: the stated bounds are reached and nothing leaves int64; one pair rising, one falling"""
    W = 65536
    t = np.zeros((2, W), np.int8)
    t[:, 0::2], t[:, 1::2] = -128, 127
    c = FitCall("the extreme case", t, [W, W], W)
    lo_hi = np.where(np.arange(W) % 2 == 0, -32768, 32768).astype(np.int64)
    ns = np.full(W, 4, np.int64)
    c.add(0, 0, records(ns, np.ones(W, np.int64), lo_hi * 4))
    c.add(1, 0, records(ns, np.ones(W, np.int64), -lo_hi * 4))
    return c


def fit_cases():
    rng = np.random.default_rng(2502)
    cases = []
    stride = 352
    target = random_target(rng, 3, 340, stride)
    prior = np.stack([rng.normal(0, 50, 12), rng.uniform(5, 40, 12)], axis=1).astype(np.float32)
    # W at 1, 2, 63, 64, 65, 128; start at every residue of a dword; the stretch ending at L_g exactly
    c = FitCall("widths and residues", target, [340, 340, 333], 128, prior=prior)
    for i, W in enumerate((1, 2, 63, 64, 65, 128, 7, 9, 100, 130 - 2, 5, 64)):
        start = [0, 1, 2, 3, 4, 5, 6, 7][i % 8] + 16 * (i % 3)
        if i >= 8:
            start = [340, 340, 333][i % 3] - W   # ends at L_g
        c.add(i % 3, start, line_records(rng, target[i % 3, start:start + W], 9.0 + i, -30.0 + 7 * i, noise=2.0))
    cases.append(c)
    # K at 0, 1, 2; all g equal; a negative and a zero slope
    flat = np.zeros((2, 64), np.int8)
    flat[0, :40] = 17
    flat[1, :40] = np.arange(40) - 20
    c = FitCall("few levels, flat targets, falling and level lines", flat, [40, 40], 64, min_samples=4, prior=prior[:8])
    g = flat[1, 0:30]
    few = np.full(30, 2, np.int64)
    for K in (0, 1, 2):
        ns = few.copy()
        ns[[3, 17][:K]] = 6
        c.add(1, 0, line_records(rng, g, 10.0, 5.0, ns=ns))
    c.add(0, 5, line_records(rng, flat[0, 5:35], 10.0, 5.0, noise=3.0, ns=np.full(30, 8)))     # all g equal: den 0
    c.add(1, 0, line_records(rng, g, -10.0, 5.0, ns=np.full(30, 8)))                           # a negative slope
    c.add(1, 0, line_records(rng, g, 0.0, 77.0, ns=np.full(30, 8)))                            # a zero slope: num 0
    c.add(1, 2, line_records(rng, flat[1, 2:32], 12.0, -800.0, noise=1.0, ns=np.full(30, 8)))  # a good one among them
    c.add(1, 0, line_records(rng, g, 1e-3, 0.0, ns=np.full(30, 64)))                           # q is 0 or +-1: a slope so small that scale is huge but finite
    cases.append(c)
    # min_samples and max_entries each dropping levels on both sides of a turn's seam
    wide = random_target(rng, 1, 200, 208)
    for name, kw in (("min_samples at the seams", {"min_samples": 5}), ("max_entries at the seams", {"max_entries": 3}),
                     ("both filters, no prior, no sums", {"min_samples": 5, "max_entries": 3, "use_sums": False})):
        c = FitCall(name, wide, [200], 136, prior=None if "no prior" in name else prior[:5], **kw)
        for drop in ([63], [64], [63, 64], [127, 128, 0], list(range(60, 70))):
            ns, ne = np.full(130, 9, np.int64), np.ones(130, np.int64)
            ns[drop], ne[drop] = 4, 4
            # the dropped levels are far off the line: a fit that keeps one is another fit
            rec = line_records(rng, wide[0, 3:133], 11.0, 40.0, ns=ns, ne=ne)
            bad = line_records(rng, wide[0, 3:133], -300.0, 9000.0, ns=ns, ne=ne)
            rec[drop] = bad[drop]
            c.add(0, 3, rec)
        cases.append(c)
    # |m| just inside and outside 32 768; wrapped sums as locate_levels may hand on
    c = FitCall("means at the bound, wrapped sums", wide, [200], 72, prior=prior[:6])
    g = wide[0, 10:74]
    base = line_records(rng, g, 200.0, 100.0, ns=np.full(64, 16))
    for total in (32768 * 16, -32768 * 16, 32768 * 16 + 1, -32768 * 16 - 1, 32768 * 16 - 1):
        rec = base.copy()
        rec[5, 4:6] = np.array([total], np.int64).view(np.uint32)
        c.add(0, 10, rec)
    rec = base.copy()
    rec[[2, 63], 4:6] = np.array([(1 << 63) - 5, -(1 << 63)], np.int64).view(np.uint32).reshape(2, 2)   # a sum that wrapped: far outside, left out
    rec[7, 2] = 0xFFFFFFFF                                                                              # ... and a wrapped n_samples: a mean near 0
    c.add(0, 10, rec)
    cases.append(c)
    cases.append(extreme_call())
    cases.append(exact_call())
    return cases


def exact_call():
    """level means are a g + b with integers a and b: offset = -b and scale = float32(1 / (a quant)) exactly"""
    rng = np.random.default_rng(2503)
    t = random_target(rng, 2, 500, 512)
    c = FitCall("exact recovery", t, [500, 500], 256, quant=32.0)
    c.planted = []
    for i, (a, b) in enumerate(((8, 0), (1, -5), (13, 700), (255, -32000 + 127 * 255), (3, 12345), (64, -64))):
        W = (256, 100, 65, 200, 2, 31)[i]
        start = 11 * i + i % 4
        c.add(i % 2, start, line_records(rng, t[i % 2, start:start + W], float(a), float(b)))
        c.planted.append((a, b))
    return c


def invalid_pair_calls():
    """every invalid-pair condition one at a time, in the middle of good pairs -> [(name, call, the bad pair)]"""
    rng = np.random.default_rng(2504)
    t = random_target(rng, 2, 120, 128)
    prior = np.stack([rng.normal(0, 50, 3), rng.uniform(5, 40, 3)], axis=1).astype(np.float32)
    out = []
    for name, kw, tl in (("read >= n_reads", {"read": 3}, None), ("read far out", {"read": 0xFFFFFFFF}, None), ("ref >= G", {"ref": 2}, None),
                         ("ref far out", {"ref": 0xFFFFFFFF}, None), ("W == 0", {"W": 0}, None), ("W > max_width", {"W": 41, "n_rec": 41}, None),
                         ("end - start != W", {"end": 61}, None), ("end < start", {"end": 10}, None), ("L_g == 0", {"ref": 1}, [120, 0]),
                         ("L_g > target_stride", {"ref": 1}, [120, 129]), ("L_g far out", {"ref": 1}, [120, 0xFFFFFFFF]), ("end > L_g", {"ref": 1}, [120, 59])):
        c = FitCall(name, t, tl or [120, 120], 40, n_reads=3, prior=prior)
        good = lambda ref, start: line_records(rng, t[ref, start:start + 40], 10.0, 3.0, noise=1.0)   # noqa: E731
        c.add(0, 7, good(0, 7), read=0)
        n_rec = kw.pop("n_rec", 40)
        ref = kw.pop("ref", 0)
        rec = line_records(rng, t[min(ref, 1), 20:20 + n_rec], 10.0, 3.0, noise=1.0)
        c.add(ref, 20, rec, read=kw.get("read", 1), end=kw.get("end"), W=kw.get("W"))
        c.add(0, 50, good(0, 50), read=2)
        out.append((name, c, 1))
    return out


# ---- the refit chain's conditions -----------------------------------------------------------------------------------------------------------
def fitted_tables(out):
    """(offset, scale) float32 tables of a fit's records"""
    return out[:, 0].copy().view(np.float32), out[:, 1].copy().view(np.float32)

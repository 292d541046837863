"""Reference for the signal-match calls (include/vbz_gpu.h: vbz_gpu_match), pure numpy: the quantisation, the subsequence DTW row by row,
and the catalogue of pairs the stage entry is held to on the device.

The DP.  Row i of D over a query k_0 ... k_{n-1}: c_j = |r_i - k_j|, a_j = min(D[i-1][j], D[i-1][j-1]) (row 0: a_j = 0, the free start;
D[i-1][-1] is +inf), and D[i][j] = c_j + min(a_j, D[i][j-1]).  Unrolled along the row that is D[i][j] = C_j + min_{j' <= j} (a_j' - C_{j'-1})
with C the row's cumulative cost (C_{-1} = 0): one cumulative sum and one running minimum per row, in int64.  A position only depends on
positions in front of it, so a batch of queries of different lengths n is walked as one [reads, N] array and read off below n."""
import functools

import numpy as np

EMPTY = (0xFFFFFFFF, 0)
FAR = np.int64(1) << 40
LENGTHS_M = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2047, 2048]
LENGTHS_N = [0, 1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 191, 192, 193, 1000]


def quantize(z, quant):
    """k = 0 for a NaN product, else clamp(rint(float32(z) * float32(quant)), -127, 127), rint to nearest even -> int8"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(z, dtype=np.float32) * np.float32(quant)
        k = np.clip(np.rint(v), np.float32(-127), np.float32(127))
    return np.where(np.isnan(v), np.float32(0), k).astype(np.int8)


def dtw_rows(ref, K):
    """the last row D[M-1][.] of every query row of K (int [reads, N]) against ref (int [M], M >= 1), int64 [reads, N]"""
    K = np.asarray(K, np.int64)
    prev = None
    for r in np.asarray(ref, np.int64):
        c = np.abs(r - K)
        C = np.cumsum(c, axis=1)
        if prev is None:
            a = np.zeros_like(c)
        else:
            a = prev.copy()
            a[:, 1:] = np.minimum(prev[:, 1:], prev[:, :-1])
        prev = C + np.minimum.accumulate(a - (C - c), axis=1)
    return prev


def dtw_batch(ref, K, n):
    """(cost, end) uint32 [reads] each: query i is K[i, :n[i]]; n[i] == 0 or an empty ref: the empty verdict"""
    K = np.asarray(K, np.int64)
    n = np.asarray(n, np.int64)
    cost = np.full(len(K), EMPTY[0], np.uint32)
    end = np.zeros(len(K), np.uint32)
    if len(ref) == 0 or K.shape[1] == 0:
        return cost, end
    last = dtw_rows(ref, K)
    last[np.arange(K.shape[1])[None, :] >= n[:, None]] = FAR
    ok = n > 0
    cost[ok] = last.min(axis=1)[ok]
    end[ok] = last.argmin(axis=1)[ok] + 1   # (argmin: the first position that attains it)
    return cost, end


def dtw(ref, k):
    """(cost, end) of one pair"""
    if len(k) == 0:
        return EMPTY
    cost, end = dtw_batch(ref, np.asarray(k, np.int64)[None, :], [len(k)])
    return int(cost[0]), int(end[0])


def dtw_matrix(ref, k):
    """the whole D by the defining triple loop (small pairs only)"""
    M, n = len(ref), len(k)
    D = np.zeros((M, n), np.int64)
    for i in range(M):
        for j in range(n):
            c = abs(int(ref[i]) - int(k[j]))
            if i == 0:
                D[i][j] = c
            elif j == 0:
                D[i][j] = c + D[i - 1][0]
            else:
                D[i][j] = c + min(D[i - 1][j - 1], D[i - 1][j], D[i][j - 1])
    return D


def dtw_brute(ref, k):
    if len(k) == 0 or len(ref) == 0:
        return EMPTY
    last = dtw_matrix(ref, k)[-1]
    return int(last.min()), int(np.argmin(last)) + 1


def hits(query, valid, quant, ref, ref_len):
    """what a match launch writes: uint32 [reads, R, 2].  query float32 [reads, N]; valid, ref_len: any integers 0 ... 2^32 - 1"""
    N = query.shape[1]
    K = quantize(query, quant)
    n = np.minimum(np.asarray(valid, np.uint64), N).astype(np.int64)
    out = np.zeros((len(query), len(ref), 2), np.uint32)
    out[:, :, 0] = EMPTY[0]
    for r, M in enumerate(np.asarray(ref_len, np.uint64).tolist()):
        if M == 0 or M > ref.shape[1]:
            continue
        out[:, r, 0], out[:, r, 1] = dtw_batch(ref[r, : int(M)], K, n)
    return out


# ---- the catalogue ------------------------------------------------------------------------------------------------------------------------
class Call:
    """one stage-entry call: queries (float32 [reads, N]) with their valid counts against reference rows (int8 [R, stride]) with their
    lengths; pairs: the (n, M) of every pair it checks; planted: {(read, ref): (cost, end)} known without running the DP"""

    def __init__(self, name, N, quant, stride):
        self.name, self.N, self.quant, self.stride = name, N, quant, stride
        self.rows, self.valid, self.refs, self.ref_len, self.planted = [], [], [], [], {}

    def read(self, levels=None, z=None, valid=None):
        """a query row from int levels (z = level / quant: exact for a power-of-two quant) or from floats as they are"""
        row = np.zeros(self.N, np.float32)
        if z is None:
            z = np.asarray(levels, np.float32) / np.float32(self.quant)
        row[: len(z)] = z
        self.rows.append(row)
        self.valid.append(len(z) if valid is None else valid)
        return len(self.rows) - 1

    def ref(self, levels, length=None):
        row = np.zeros(self.stride, np.int8)
        row[: len(levels)] = levels
        self.refs.append(row)
        self.ref_len.append(len(levels) if length is None else length)
        return len(self.refs) - 1

    def arrays(self):
        return (np.stack(self.rows), np.asarray(self.valid, np.uint64).astype(np.uint32), np.stack(self.refs),
                np.asarray(self.ref_len, np.uint64).astype(np.uint32))

    def pairs(self):
        return [(min(int(v), self.N), int(M)) for v in self.valid for M in self.ref_len if 0 < int(M) <= self.stride]


def _signal_levels(rng, n):
    """levels like MAD-normalised signal at 32 a unit: plateaus under noise"""
    steps = np.repeat(rng.integers(-70, 71, n // 6 + 1), 6)[:n]
    return np.clip(steps + rng.integers(-6, 7, n), -127, 127)


def _plant(bg, at, what):
    q = np.array(bg, np.int64)
    q[at : at + len(what)] = what
    return q


@functools.lru_cache(maxsize=None)
def catalogue():
    """the calls of tests/test_gpu_match.py: every M of LENGTHS_M against at least four n of LENGTHS_N and the other way round (not the
    cross product: the long references meet a handful of queries), the planted answers, the extremes, refused ref_len, valid above N"""
    rng = np.random.default_rng(2210)
    calls = []
    # short and middle references against every query length
    a = Call("lengths", 1024, 32.0, 272)
    for n in LENGTHS_N:
        a.read(_signal_levels(rng, n))
    for M in [m for m in LENGTHS_M if m <= 257]:
        a.ref(_signal_levels(rng, M))
    a.ref(_signal_levels(rng, 40), length=0)             # refused lengths beside good ones
    a.ref(_signal_levels(rng, 40), length=273)
    a.ref(_signal_levels(rng, 40), length=0xFFFFFFFF)
    a.ref(_signal_levels(rng, 100))
    a.read(_signal_levels(rng, 1024), valid=5000)        # valid above N is clamped to N
    a.read(_signal_levels(rng, 1024), valid=0xFFFFFFFF)
    calls.append(a)
    # long references against a handful of query lengths: each change of c, a lane's last row, the last lane
    b = Call("long", 1000, 32.0, 2048)
    for n in (0, 1, 8, 64, 65, 129, 193, 1000):
        b.read(_signal_levels(rng, n))
    for M in [m for m in LENGTHS_M if m >= 255]:
        b.ref(_signal_levels(rng, M))
    calls.append(b)
    # planted answers: cost 0 and a known end.  The reference's levels stay inside +-40, the background at 90 and above
    p = Call("planted", 448, 32.0, 144)
    for M in (17, 64, 129):
        ref = rng.integers(-40, 41, M)
        for i in range(1, M):   # (no level twice in a row: no alignment at cost 0 ends in front of the copy's end)
            if ref[i] == ref[i - 1]:
                ref[i] += 1 if ref[i] < 40 else -1
        ri = p.ref(ref)
        bg = rng.integers(90, 128, 448)
        for at in (0, 448 - M, 64 - M // 2, 192 - 1):   # its very start, its very end, across a load seam, one sample in front of one
            p.planted[(p.read(_plant(bg, at, ref)), ri)] = (0, at + M)
        p.planted[(p.read(_plant(bg, 30, np.repeat(ref, 2))), ri)] = (0, 30 + 2 * M - 1)   # every sample doubled: the first-j rule
        p.planted[(p.read(_plant(_plant(bg, 10, ref), 250, ref)), ri)] = (0, 10 + M)      # two equal plants: the first
    calls.append(p)
    # extremes
    e = Call("extremes", 64, 1.0, 2048)
    hi, lo = e.ref(np.full(2048, 127)), e.ref(np.full(300, -128))
    e.ref(rng.integers(-128, 128, 700))
    e.ref(rng.integers(-128, 128, 64))
    q_lo = e.read(np.full(64, -127))
    q_hi = e.read(np.full(9, 127))
    e.read(rng.integers(-127, 128, 64))
    e.read(rng.integers(-127, 128, 33))
    e.planted[(q_lo, hi)] = (254 * 2048, 1)
    e.planted[(q_hi, lo)] = (255 * 300, 1)
    # the quantisation inside a call: ties of both parities, the clamp, NaN, infinities, a quant that is no power of two below
    e.read(z=np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5, 127.5, 200.0, -127.5, -1e30, np.nan, np.inf, -np.inf, 3e38, 0.49999997], np.float32))
    calls.append(e)
    f = Call("floats", 200, 10.3, 64)
    for n in (200, 77):
        f.read(z=rng.normal(0, 4, n).astype(np.float32))
    for M in (5, 33, 64):
        f.ref(quantize(rng.normal(0, 4, M), 10.3))
    calls.append(f)
    return calls


@functools.lru_cache(maxsize=None)
def expected(index):
    """the hits of catalogue()[index], computed once"""
    c = catalogue()[index]
    query, valid, ref, ref_len = c.arrays()
    out = hits(query, valid, c.quant, ref, ref_len)
    out.setflags(write=False)
    return out

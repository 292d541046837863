"""Reference for the signal-match calls that also give the start of the aligned stretch (include/vbz_gpu.h: vbz_gpu_match_span), pure
numpy and python: the row-by-row statement, the defining triple loop, the enumeration of every path, and the catalogue of pairs the
stage entry is held to on the device.  match_ref is the statement of everything the two families share: quantisation, cost and end.

The DP is over pairs (cost, start) ordered lexicographically.  As one int64 key cost << 20 | start (a start is < 65 536 < 2^20) the
signed order of keys is that order, and match_ref's row form carries over: with c_j the row's costs, C their cumulative sum and
a_j = min(P[i-1][j], P[i-1][j-1]) (row 0: a_j = the key (0, j); P[i-1][-1] is far), P[i][j] = (c_j << 20) + min(a_j, P[i][j-1])
unrolls to (C_j << 20) + min_{j' <= j} (a_j' - (C_{j'-1} << 20)): subtracting C << 20 leaves the start bits alone and the signed order
stays lexicographic.  Row 0 needs no case of its own: P[0][j-1] beats the key (0, j) exactly when its cost is 0."""
import functools

import numpy as np

import match_ref as M

EMPTY = (0xFFFFFFFF, 0, 0, 0)
SHIFT = 20
FAR = np.int64(1) << 60


def span_rows(ref, K):
    """the last row of keys of every query row of K (int [reads, N]) against ref (int [M], M >= 1), int64 [reads, N]"""
    K = np.asarray(K, np.int64)
    prev = None
    for r in np.asarray(ref, np.int64):
        c = np.abs(r - K)
        C = np.cumsum(c, axis=1)
        if prev is None:
            a = np.broadcast_to(np.arange(K.shape[1], dtype=np.int64), K.shape).copy()
        else:
            a = prev.copy()
            a[:, 1:] = np.minimum(prev[:, 1:], prev[:, :-1])
        prev = (C << SHIFT) + np.minimum.accumulate(a - ((C - c) << SHIFT), axis=1)
    return prev


def span_batch(ref, K, n):
    """(cost, end, start) uint32 [reads] each: query i is K[i, :n[i]]; n[i] == 0 or an empty ref: the empty verdict.  The answer is the
    lexicographic minimum of the last row at its first column (the header's fact 1: that column is the first of the minimum cost)"""
    K = np.asarray(K, np.int64)
    n = np.asarray(n, np.int64)
    cost = np.full(len(K), EMPTY[0], np.uint32)
    end = np.zeros(len(K), np.uint32)
    start = np.zeros(len(K), np.uint32)
    if len(ref) == 0 or K.shape[1] == 0:
        return cost, end, start
    last = span_rows(ref, K)
    last[np.arange(K.shape[1])[None, :] >= n[:, None]] = FAR
    ok = n > 0
    best = last.min(axis=1)
    cost[ok] = (best >> SHIFT)[ok]
    start[ok] = (best & ((1 << SHIFT) - 1))[ok]
    end[ok] = last.argmin(axis=1)[ok] + 1   # (argmin: the first position that attains it)
    return cost, end, start


def spans(query, valid, quant, ref, ref_len):
    """what a span launch writes: uint32 [reads, R, 4] = (cost, end, start, 0).  Arguments as match_ref.hits"""
    N = query.shape[1]
    n = np.minimum(np.asarray(valid, np.uint64), N).astype(np.int64)
    K = M.quantize(query[:, : int(n.max(initial=0))], quant)   # (a position depends on positions in front of it alone)
    out = np.zeros((len(query), len(ref), 4), np.uint32)
    out[:, :, 0] = EMPTY[0]
    for r, m in enumerate(np.asarray(ref_len, np.uint64).tolist()):
        if m == 0 or m > ref.shape[1]:
            continue
        out[:, r, 0], out[:, r, 1], out[:, r, 2] = span_batch(ref[r, : int(m)], K, n)
    return out


def span_matrix(ref, k, sit=True):
    """the whole P by the defining triple loop: P[i][j] = (cost, start).  sit False: row 0 is (c(0, j), j) whatever stands left of it --
    the DP of paths that may not sit on row 0 (what moved when the two differ moved because of a sit at cost 0)"""
    ref, k = [int(v) for v in ref], [int(v) for v in k]
    P = [[None] * len(k) for _ in ref]
    for i, r in enumerate(ref):
        for j, q in enumerate(k):
            c = abs(r - q)
            if i == 0:
                P[0][j] = (c, P[0][j - 1][1] if sit and j > 0 and P[0][j - 1][0] == 0 else j)
            else:
                m = P[i - 1][j] if j == 0 else min(P[i - 1][j - 1], P[i - 1][j], P[i][j - 1])
                P[i][j] = (c + m[0], m[1])
    return P


def first_end(P):
    """(cost, end, start) read off a matrix by the cost-only rule: the FIRST column of the minimum cost, and its start"""
    last = P[-1]
    cost = min(p[0] for p in last)
    j = next(j for j, p in enumerate(last) if p[0] == cost)
    return cost, j + 1, last[j][1]


def span_brute(ref, k, sit=True):
    if len(k) == 0 or len(ref) == 0:
        return EMPTY[:3]
    return first_end(span_matrix(ref, k, sit))


def diagonal_first_start(ref, k, P, end):
    """the start an ordinary backtrace from (M - 1, end - 1) gives: diagonal before up before left, stopping where it reaches row 0"""
    i, j = len(ref) - 1, end - 1
    while i > 0:
        want = P[i][j][0] - abs(int(ref[i]) - int(k[j]))
        if j > 0 and P[i - 1][j - 1][0] == want:
            i, j = i - 1, j - 1
        elif P[i - 1][j][0] == want:
            i -= 1
        else:
            j -= 1
    return j


def span_paths(ref, k):
    """(cost, end, start) by walking EVERY warping path (pairs of at most 4 x 6): the minimum cost over all paths, the first column that
    a path of that cost ends at, the smallest start over the paths of that cost that end there"""
    rows, n = len(ref), len(k)
    assert rows <= 4 and n <= 6
    c = [[abs(int(r) - int(q)) for q in k] for r in ref]
    ends = []   # (cost, end column, start) of every path

    def walk(i, j, cost, s):
        cost += c[i][j]
        if i == rows - 1:
            ends.append((cost, j, s))
        if j + 1 < n:
            walk(i, j + 1, cost, s)
            if i + 1 < rows:
                walk(i + 1, j + 1, cost, s)
        if i + 1 < rows:
            walk(i + 1, j, cost, s)

    for s in range(n):
        walk(0, s, 0, s)
    cost = min(e[0] for e in ends)
    col = min(e[1] for e in ends if e[0] == cost)
    return cost, col + 1, min(e[2] for e in ends if e[0] == cost and e[1] == col)


# ---- the catalogue ------------------------------------------------------------------------------------------------------------------------
TIE_N = [63, 64, 65, 129]                          # around the 64-sample load seam
TIE_M = [64, 65, 128, 129, 257, 513, 1025]         # a lane's last row and each change of the rows per lane
TIE_SHORT = [3, 5, 9, 17, 33, 47]                  # ... and references shorter than the queries, where a stretch has room to move


def _distinct(rng, lo, hi, m):
    """m levels in lo ... hi, no level twice in a row: no alignment at cost 0 ends in front of a copy's end"""
    ref = rng.integers(lo, hi + 1, m)
    for i in range(1, m):
        if ref[i] == ref[i - 1]:
            ref[i] += 1 if ref[i] < hi else -1
    return ref


def _plant(bg, at, what):
    q = np.array(bg, np.int64)
    q[at : at + len(what)] = what
    return q


@functools.lru_cache(maxsize=None)
def span_catalogue():
    """the calls of tests/test_gpu_match_span.py beside match_ref.catalogue(), as match_ref.Calls; planted: {(read, ref): (cost, end, start)}.
    Names: tie calls start with "ties", the four calls of one data set on both sides of the host's rule with "rule"."""
    rng = np.random.default_rng(4220)
    calls = []
    # ties: small alphabets, where many paths cost the same
    for name, a in (("ties-3", 3), ("ties-1", 1)):
        t = M.Call(name, 136, 1.0, 1040)
        for n in TIE_N:
            t.read(rng.integers(-a, a + 1, n))
        for n in TIE_N:   # plateaus of four samples: a row has several samples to take at the same cost
            t.read(np.repeat(rng.integers(-a, a + 1, n // 4 + 1), 4)[:n])
        for m in TIE_M + TIE_SHORT:
            t.ref(rng.integers(-a, a + 1, m))
        calls.append(t)
    # planted answers at cost 0, n = N = 2^8.  The references stay inside +-40 with no level twice in a row, the background at 90 and above
    p = M.Call("ties-planted", 256, 1.0, 80)
    for m in (17, 64):
        ref = _distinct(rng, -40, 40, m)
        ri = p.ref(ref)
        bg = rng.integers(90, 128, 256)
        p.planted[(p.read(_plant(bg, 0, ref)), ri)] = (0, m, 0)                                  # a plant at sample 0
        p.planted[(p.read(_plant(bg, 256 - m, ref)), ri)] = (0, 256, 256 - m)                    # the query's last samples
        run = _plant(_plant(bg, 100, ref), 95, np.full(5, ref[0]))                               # its first level five times in front:
        p.planted[(p.read(run), ri)] = (0, 100 + m, 95)                                          # ... sitting on row 0 moves the start
        p.planted[(p.read(_plant(bg, 30, np.repeat(ref, 2))), ri)] = (0, 30 + 2 * m - 1, 30)     # doubled: the start stays, the end moves
    one = p.ref([7])
    p.planted[(p.read(_plant(rng.integers(90, 128, 256), 255, [7])), one)] = (0, 256, 255)       # the largest start of the field
    calls.append(p)
    # field extremes.  254 x 2048 = 520 192 is just under the far value of a 19-bit cost field (N = 4096: 12 bits of start)
    for name, N in (("extreme-packed", 4096), ("extreme-wide", 8192)):
        e = M.Call(name, N, 1.0, 2048)
        e.planted[(e.read(np.full(N, -127)), e.ref(np.full(2048, 127)))] = (254 * 2048, 1, 0)
        calls.append(e)
    bg = rng.integers(90, 128, 65536)
    ref = _distinct(rng, -40, 40, 128)
    for name, stride in (("long-packed", 128), ("long-wide", 144)):   # 16 bits of start: stride 128 is the packed kernel's last
        e = M.Call(name, 65536, 1.0, stride)
        ri, hi = e.ref(ref), e.ref(np.full(128, 127))
        e.ref(rng.integers(-128, 128, stride))
        at = 65536 - 150
        e.planted[(e.read(_plant(bg, at, ref), valid=65536), ri)] = (0, at + 128, at)
        e.planted[(e.read(np.full(65536, -127)), hi)] = (254 * 128, 1, 0)
        calls.append(e)
    # one data set on both sides of the host's rule: padded rows, the same valid counts
    reads = [M._signal_levels(rng, 4096), rng.integers(-3, 4, 1000), rng.integers(-1, 2, 65), M._signal_levels(rng, 4095)]
    refs = [M._signal_levels(rng, 257), rng.integers(-3, 4, 129), rng.integers(-1, 2, 64), M._signal_levels(rng, 17)]
    for N, stride in ((4096, 2048), (8192, 2048), (16384, 416), (32768, 416)):
        c = M.Call("rule-%d-%d" % (N, stride), N, 32.0, stride)
        for x in reads:
            c.read(x)
        for x in refs:
            c.ref(x)
        calls.append(c)
    return calls


@functools.lru_cache(maxsize=None)
def expected(index, base=False):
    """the spans of span_catalogue()[index] (base: of match_ref.catalogue()[index]), computed once"""
    c = (M.catalogue() if base else span_catalogue())[index]
    query, valid, ref, ref_len = c.arrays()
    out = spans(query, valid, c.quant, ref, ref_len)
    out.setflags(write=False)
    return out

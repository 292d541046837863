"""The numpy statements of the two event-space alignment rules (include/vbz_gpu.h: vbz_gpu_events_query_batch,
vbz_gpu_locate_levels_batch) and the catalogues of planted tables the tests run: test_eventalign_ref holds the statements to plain
Python loops and counts the catalogues, the tests on the MI355X hold the device to the statements bit for bit.

Tables are plain numpy: event_first uint64 [reads + 1], event_rows an integer (the DECLARED rows: a refused read may point far behind the
arrays), mean uint32 [rows] (the float's bits), n uint32 [rows], start uint32 [rows], moments uint64 [rows, 2] (S1 as its two's
complement), pairs / hit uint32 [pairs, 4], rows uint32 [pairs, N, 2], index uint32 [reads, N] or None.  A level record is its eight
32-bit words: first_sample, end_sample, n_samples, n_entries, sum lo, sum hi, sumsq lo, sumsq hi."""
import numpy as np

E_FIRST = 0xFFFFFFF8   # result[i] at or above it is an error verdict (vbz_gpu_query_valid_batch's test)
NONE = 0xFFFFFFFF
EMPTY_HIT = (0xFFFFFFFF, 0, 0, 0)
MAX_ROWS = (1 << 31) - 1


def read_rows(event_first, event_rows, i):
    """(c0, rows) of read i, or None for a bad event_first"""
    c0, c1 = int(event_first[i]), int(event_first[i + 1])
    if c0 > c1 or c1 > int(event_rows) or c1 - c0 > MAX_ROWS:
        return None
    return c0, c1 - c0


# ---- vbz_gpu_events_query_batch -------------------------------------------------------------------------------------------------------------
def events_query(event_first, event_rows, mean, n, N, min_n, result=None):
    """-> (query uint32 [reads, N], valid uint32 [reads], index uint32 [reads, N])"""
    reads = len(event_first) - 1
    query, index, valid = np.zeros((reads, N), np.uint32), np.zeros((reads, N), np.uint32), np.zeros(reads, np.uint32)
    for i in range(reads):
        own = read_rows(event_first, event_rows, i)
        if own is None or (result is not None and int(result[i]) >= E_FIRST):
            continue
        c0, rows = own
        kept = np.flatnonzero(np.asarray(n[c0:c0 + rows], np.uint32) >= np.uint32(min_n))[:N]
        valid[i] = len(kept)
        query[i, :len(kept)] = np.asarray(mean, np.uint32)[c0 + kept]
        index[i, :len(kept)] = kept
    return query, valid, index


# ---- vbz_gpu_locate_levels_batch ------------------------------------------------------------------------------------------------------------
def path_ok(rows, n, start, end):
    """the invariants of a path of n rows from level start to level end"""
    b, e = rows[:n, 0].astype(np.int64), rows[:n, 1].astype(np.int64)
    return bool(b[0] == start and e[-1] == end and (b < e).all() and ((b[1:] == e[:-1]) | (b[1:] == e[:-1] - 1)).all())


def _prefix(x):
    """exclusive prefix sums modulo 2^64, one entry more than x"""
    return np.concatenate([np.zeros(1, np.uint64), np.cumsum(np.asarray(x, np.uint64), dtype=np.uint64)])


def pair_levels(rows, n, start, end, c, ev_start, ev_n, moments, direct=False):
    """the records of levels start ... end - 1 of one checked pair -> uint32 [end - start, 8]; c: the event row of every entry.  The sums
    as differences of prefix sums, or (direct) added up entry by entry: the same modulo 2^32 and 2^64"""
    b, e = rows[:n, 0].astype(np.int64), rows[:n, 1].astype(np.int64)
    j = np.arange(start, end, dtype=np.int64)
    k0 = np.searchsorted(e, j, side="right")   # entries that end at or in front of j
    k1 = np.searchsorted(b, j, side="right")   # entries that begin at or in front of j
    assert (k0 < k1).all()
    s, m = np.asarray(ev_start, np.uint32)[c].astype(np.uint64), np.asarray(ev_n, np.uint32)[c].astype(np.uint64)
    s1, s2 = np.asarray(moments, np.uint64)[c, 0], np.asarray(moments, np.uint64)[c, 1]
    out = np.zeros((end - start, 4), np.uint64)
    out[:, 0] = s[k0]
    out[:, 1] = (s[k1 - 1] + m[k1 - 1]) & np.uint64(0xFFFFFFFF)
    out[:, 3] = k1 - k0
    sums = np.zeros((end - start, 2), np.uint64)
    if direct:
        with np.errstate(over="ignore"):
            for t in range(end - start):
                out[t, 2] = np.sum(m[k0[t]:k1[t]], dtype=np.uint64) & np.uint64(0xFFFFFFFF)
                sums[t] = np.sum(s1[k0[t]:k1[t]], dtype=np.uint64), np.sum(s2[k0[t]:k1[t]], dtype=np.uint64)
    else:
        pm, p1, p2 = _prefix(m), _prefix(s1), _prefix(s2)
        out[:, 2] = (pm[k1] - pm[k0]) & np.uint64(0xFFFFFFFF)
        sums[:, 0], sums[:, 1] = p1[k1] - p1[k0], p2[k1] - p2[k0]
    rec = np.zeros((end - start, 8), np.uint32)
    rec[:, :4] = out.astype(np.uint32)
    rec[:, 4:] = sums.view(np.uint32).reshape(-1, 4)   # (little endian: lo, hi, lo, hi)
    return rec


def pair_events(pair, hit, rows, index, event_first, event_rows, n_reads, N, W):
    """the event row of every entry of a pair, or None when the pair is refused"""
    read, (end, start, n) = int(pair[0]), (int(v) for v in hit[1:])
    if read >= n_reads or n == 0 or n > N or start >= end or end - start > W:
        return None
    own = read_rows(event_first, event_rows, read)
    if own is None or not path_ok(rows, n, start, end):
        return None
    idx = np.arange(n, dtype=np.int64) if index is None else index[read, :n].astype(np.int64)
    if (idx >= own[1]).any():
        return None
    return own[0] + idx


def levels(pairs, hit, rows, index, event_first, event_rows, ev_start, ev_n, moments, n_reads, N, W, direct=False):
    """-> (n_levels uint32 [pairs], levels uint32 [pairs, W, 8])"""
    P = len(pairs)
    n_levels, out = np.zeros(P, np.uint32), np.zeros((P, W, 8), np.uint32)
    for p in range(P):
        c = pair_events(pairs[p], hit[p], rows[p], index, event_first, event_rows, n_reads, N, W)
        if c is None:
            continue
        end, start, n = (int(v) for v in hit[p][1:])
        n_levels[p] = end - start
        out[p, :end - start] = pair_levels(rows[p], n, start, end, c, ev_start, ev_n, moments, direct)
    return n_levels, out


# ---- planted paths --------------------------------------------------------------------------------------------------------------------------
def path_of(start, advance, vertical):
    """rows [n, 2] of the path whose entry k ends advance[k] levels behind entry k - 1's end (entry 0: behind start + 1) and begins on the
    previous entry's last level (vertical[k], forced where advance[k] == 0) or just behind it; width = 1 + sum(advance)"""
    n = len(advance)
    rows = np.zeros((n, 2), np.int64)
    rows[0] = start, start + 1 + advance[0]
    for k in range(1, n):
        pe = rows[k - 1, 1]
        rows[k] = (pe - 1 if (vertical[k] or advance[k] == 0) else pe), pe + advance[k]
    return rows


def random_path(rng, n, width, start=0):
    """n entries over exactly `width` levels: a random composition of width - 1 into n advances, stalls where it gives 0"""
    cuts = np.sort(rng.integers(0, width, n - 1)) if n > 1 else np.zeros(0, np.int64)
    adv = np.diff(np.concatenate([[0], cuts, [width - 1]]))
    return path_of(start, adv, rng.integers(0, 2, n).astype(bool))


def shape_counts(rows):
    """(stalls, skips) of a path: levels that hold more than one entry, entries that span more than one level"""
    b, e = rows[:, 0], rows[:, 1]
    return int(((b[1:] == e[:-1] - 1)).sum()), int((e - b > 1).sum())


class LevelsCall:
    """one call of vbz_gpu_locate_levels_batch: read r has the events its paths need; pair p is (read, hit, rows)"""

    def __init__(self, name, N, W):
        self.name, self.N, self.W = name, N, W
        self.first, self.ev_start, self.ev_n, self.moments = [0], [], [], []
        self.index, self.pairs, self.hit, self.rows = [], [], [], []
        self.use_index = True
        self.event_rows = None   # (None: the arrays' own length)

    def add_read(self, rng, rows, entries, gaps=False, moments="small", dwell=30):
        """a read of `rows` events of which `entries` ascending ones are the query's -> the read's number"""
        pos = 0
        for _ in range(rows):
            d = int(rng.integers(0, dwell + 1))
            self.ev_start.append(pos)
            self.ev_n.append(d)
            pos += d
        if moments == "small":
            m = np.stack([rng.integers(-(1 << 20), 1 << 20, rows).astype(np.int64).view(np.uint64), rng.integers(0, 1 << 40, rows).astype(np.uint64)], 1)
        elif moments == "2^46":
            m = np.stack([np.where(rng.integers(0, 2, rows) == 1, 1 << 46, -(1 << 46)).astype(np.int64).view(np.uint64),
                          rng.integers(1 << 62, 1 << 63, rows).astype(np.uint64)], 1)
        else:   # running totals that pass 2^64
            m = rng.integers(1 << 62, (1 << 64) - 1, (rows, 2), dtype=np.uint64)
        self.moments.extend(m.tolist())
        idx = np.sort(rng.choice(rows, entries, replace=False)) if gaps else np.arange(entries)
        row = np.zeros(self.N, np.uint32)
        row[:entries] = idx
        self.index.append(row)
        self.first.append(self.first[-1] + rows)
        return len(self.first) - 2

    def add_pair(self, read, path, begin=None, cost=7):
        n, start, end = len(path), int(path[0, 0]), int(path[-1, 1])
        rows = np.zeros((self.N, 2), np.uint32)
        rows[:n] = path
        self.pairs.append((read, 0, start if begin is None else begin, end))
        self.hit.append((cost, end, start, n))
        self.rows.append(rows)
        return len(self.pairs) - 1

    def plant(self, rng, path, **kw):
        """a read of its own for one path"""
        gaps = kw.pop("gaps", False)
        rows = len(path) + (int(rng.integers(1, 9)) if gaps else 0)
        return self.add_pair(self.add_read(rng, rows, len(path), gaps=gaps, **kw), path)

    def arrays(self):
        """(pairs, hit, rows, index, event_first, event_rows, start, n, moments, n_reads)"""
        R = len(self.ev_start)
        return (np.asarray(self.pairs, np.uint64).astype(np.uint32).reshape(-1, 4), np.asarray(self.hit, np.uint64).astype(np.uint32).reshape(-1, 4),
                np.asarray(self.rows, np.uint32).reshape(-1, self.N, 2), np.asarray(self.index, np.uint32).reshape(-1, self.N) if self.use_index else None,
                np.asarray(self.first, np.uint64), R if self.event_rows is None else self.event_rows, np.asarray(self.ev_start, np.uint64).astype(np.uint32),
                np.asarray(self.ev_n, np.uint64).astype(np.uint32), np.asarray(self.moments, np.uint64).reshape(-1, 2), len(self.first) - 1)

    def expected(self, direct=False):
        pairs, hit, rows, index, first, event_rows, start, n, moments, n_reads = self.arrays()
        return levels(pairs, hit, rows, index, first, event_rows, start, n, moments, n_reads, self.N, self.W, direct)


def _up8(v):
    return max(8, (int(v) + 7) // 8 * 8)


def call_of(name, rng, paths, W=None, **kw):
    N = _up8(max(len(p) for p in paths))
    c = LevelsCall(name, N, _up8(max(int(p[-1, 1] - p[0, 0]) for p in paths)) if W is None else W)
    for p in paths:
        c.plant(rng, p, **kw)
    return c


def stall_path(lead, held, tail=3, start=5):
    """`lead` diagonal entries, then one level holding `held` entries, then `tail` diagonal entries"""
    adv = [0] + [1] * (lead + tail + held - 1)
    vert = [False] * (lead + tail + held)
    for k in range(lead + 1, lead + held):   # entries lead + 1 ... lead + held - 1 stay on entry lead's level
        adv[k], vert[k] = 0, True
    return path_of(start, adv, vert)


def skip_path(span, lead=5, tail=4, start=2, vertical=False):
    """diagonal entries around one entry that spans `span` levels"""
    adv = [0] + [1] * (lead + tail)
    adv[lead] = span if not vertical else span - 1
    vert = [False] * (lead + tail + 1)
    vert[lead] = vertical
    return path_of(start, adv, vert)


def levels_shapes():
    """the path shapes: every n, the widths, diagonals, long skips, long stalls at every residue of a turn"""
    rng = np.random.default_rng(2424)
    out = [call_of("n 1 ... 136", rng, [random_path(rng, n, int(rng.integers(1, 2 * n + 2)), int(rng.integers(0, 1000))) for n in range(1, 137)]),
           call_of("n 255 ... 257", rng, [random_path(rng, n, int(rng.integers(100, 400))) for n in (255, 256, 257)]),
           call_of("n 2047, 2048", rng, [random_path(rng, 2047, 1500, 9), random_path(rng, 2048, 2048, 1 << 29), random_path(rng, 2048, 700)])]
    widths = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257)
    out.append(call_of("widths", rng, [random_path(rng, int(rng.integers(1, 200)), w, int(rng.integers(0, 50))) for w in widths for _ in range(2)]))
    out.append(call_of("width 2048", rng, [random_path(rng, 300, 2048), random_path(rng, 2048, 2048, 77), random_path(rng, 1, 2048)]))
    out.append(call_of("diagonals", rng, [path_of(s, [0] + [1] * (n - 1), [False] * n) for n, s in ((1, 0), (2, 9), (63, 1), (64, 0), (65, 3), (129, 4), (700, 5))]))
    out.append(call_of("one entry over many levels", rng, [skip_path(s, vertical=v) for s in (1, 2, 8, 9, 10, 63, 64, 65, 73, 74, 300) for v in (False, True)]
                        + [skip_path(300, lead=0, tail=0), skip_path(65, lead=63), skip_path(300, lead=64, tail=70)]))
    out.append(call_of("one level holding many entries", rng, [stall_path(2, h) for h in (1, 2, 63, 64, 65, 130, 2048 - 5)] + [stall_path(0, 2048, tail=0)]))
    out.append(call_of("a stall at every residue of a turn", rng, [stall_path(lead, 65) for lead in range(64)] + [stall_path(lead, 130, tail=0) for lead in (0, 31, 63)]))
    return out


def levels_tables():
    """the tables: index with gaps and NULL, moments at the edges of their ranges, sums that wrap, start > begin of the pair"""
    rng = np.random.default_rng(4242)
    paths = [random_path(rng, n, w, s) for n, w, s in ((1, 1, 0), (40, 60, 3), (64, 64, 0), (65, 20, 8), (130, 130, 100), (200, 90, 0))] + [stall_path(3, 70)]
    out = [call_of("index with gaps", rng, paths, gaps=True)]
    c = call_of("index NULL", rng, paths)
    c.use_index = False
    out.append(c)
    out.append(call_of("moments at +-2^46", rng, paths, moments="2^46", gaps=True))
    out.append(call_of("running totals pass 2^64", rng, paths, moments="wrap"))
    out.append(call_of("n sums pass 2^32", rng, paths, dwell=(1 << 31)))
    c = LevelsCall("two pairs of one read, start > begin of the pair", 72, 96)
    r = c.add_read(rng, 80, 72, gaps=True)
    c.add_pair(r, random_path(rng, 72, 90, 40), begin=11)
    c.add_pair(r, random_path(rng, 50, 17, 1000), begin=0)
    c.add_pair(r, stall_path(1, 68, 1), begin=2)
    out.append(c)
    return out


def _good_pairs(c, rng):
    for n, w, s in ((30, 44, 6), (70, 33, 0), (64, 64, 19), (1, 5, 3)):
        c.plant(rng, random_path(rng, n, w, s), gaps=True)


BROKEN = ("read >= n_reads", "read far out", "the empty verdict", "the best call's none", "n == 0", "n > query_len", "n far out", "wider than max_width",
          "start == end", "start > end", "a wrapping width", "begin_0 != start", "end_last != end", "begin_k == end_k", "begin_k > end_k",
          "begin_k == end_k at a seam", "a gap between entries", "a step back", "a step back at a seam", "a row far out", "index at the row count",
          "index far out", "index bad at a seam", "event_first descending", "event_first behind event_rows", "a read of 2^31 rows")


def levels_broken(name, at):
    """good pairs with the one broken pair `name` at position `at` -> (call, the broken pair's number)"""
    rng = np.random.default_rng(999)
    c = LevelsCall(name, 80, 72)
    _good_pairs(c, rng)
    path = random_path(rng, 70, 50, 10)   # (entries 63 and 64 sit at a seam of the 64-entry turns)
    p = c.plant(rng, path, gaps=True)
    read, rows, hit, idx = c.pairs[p][0], c.rows[p], list(c.hit[p]), c.index[c.pairs[p][0]]
    rows_of_read = c.first[read + 1] - c.first[read]

    if name == "read >= n_reads":
        c.pairs[p] = (len(c.first) - 1,) + c.pairs[p][1:]
    elif name == "read far out":
        c.pairs[p] = (NONE,) + c.pairs[p][1:]
    elif name == "the empty verdict":
        hit = list(EMPTY_HIT)
    elif name == "the best call's none":
        c.pairs[p], hit = (read, NONE, 0, 0), list(EMPTY_HIT)
        rows[:] = 0
    elif name == "n == 0":
        hit[3] = 0
    elif name == "n > query_len":
        hit[3] = c.N + 1
    elif name == "n far out":
        hit[3] = NONE
    elif name == "wider than max_width":
        wide = random_path(rng, 70, c.W + 1, 10)
        rows[:70], hit[1] = wide, int(wide[-1, 1])
    elif name == "start == end":
        hit[2] = hit[1]
    elif name == "start > end":
        hit[2] = hit[1] + 1
    elif name == "a wrapping width":
        hit[1], hit[2] = 4, NONE - 3
    elif name == "begin_0 != start":
        hit[2] -= 1
    elif name == "end_last != end":
        hit[1] += 1
    elif name in ("begin_k == end_k", "begin_k > end_k", "begin_k == end_k at a seam"):
        k = 64 if "seam" in name else 20
        rows[k, 0] = rows[k, 1] + (1 if ">" in name else 0)
    elif name == "a gap between entries":
        shift = int(rows[29, 1]) + 1 - int(rows[30, 0])   # begin_30 = end_29 + 1, the path behind it moved along
        rows[30:70] += shift
        hit[1] += shift
    elif name in ("a step back", "a step back at a seam"):
        k = 64 if "seam" in name else 33
        rows[k, 0] = rows[k - 1, 1] - 2
    elif name == "a row far out":
        rows[69, 1] = NONE
        hit[1] = NONE
    elif name == "index at the row count":
        idx[69] = rows_of_read
    elif name == "index far out":
        idx[5] = NONE
    elif name == "index bad at a seam":
        idx[64] = rows_of_read + 1000
    elif name in ("event_first descending", "event_first behind event_rows", "a read of 2^31 rows"):
        # the broken read is the LAST one, so that every other read keeps its rows
        assert read == len(c.first) - 2
        if name == "event_first descending":
            c.first[-1] = c.first[-2] - 1
        elif name == "event_first behind event_rows":
            c.first[-1] = len(c.ev_start) + 1
        else:
            c.first[-1] = c.first[-2] + (1 << 31)
            c.event_rows = c.first[-1]
    else:
        raise KeyError(name)
    c.hit[p] = tuple(hit)
    # move the broken pair to position `at` among the good ones
    order = list(range(p))
    order.insert(at, p)
    c.pairs, c.hit, c.rows = [c.pairs[i] for i in order], [c.hit[i] for i in order], [c.rows[i] for i in order]
    return c, at


def levels_catalogue():
    return levels_shapes() + levels_tables()


# ---- planted event tables for the query call ------------------------------------------------------------------------------------------------
class QueryCall:
    def __init__(self, name, N, min_n, reads, result=None, use_index=True, event_first=None, event_rows=None):
        """reads: one (mean uint32 [rows], n uint32 [rows]) per read"""
        self.name, self.N, self.min_n, self.result, self.use_index = name, N, min_n, result, use_index
        self.mean = np.concatenate([np.asarray(m, np.uint32) for m, _ in reads] + [np.zeros(0, np.uint32)])
        self.n = np.concatenate([np.asarray(v, np.uint32) for _, v in reads] + [np.zeros(0, np.uint32)])
        own = np.concatenate([[0], np.cumsum([len(v) for _, v in reads])]).astype(np.uint64)
        self.first = own if event_first is None else np.asarray(event_first, np.uint64)
        self.event_rows = len(self.n) if event_rows is None else event_rows

    def expected(self):
        return events_query(self.first, self.event_rows, self.mean, self.n, self.N, self.min_n, self.result)


def _read(rng, rows, n=None):
    mean = rng.normal(0, 2, rows).astype(np.float32).view(np.uint32)
    return mean, (rng.integers(0, 5, rows) if n is None else np.asarray(n)).astype(np.uint32)


def _kept_read(rng, kept, dropped):
    """a read of kept + dropped rows, n 3 for the kept and 0 ... 2 for the dropped (min_n 3), shuffled"""
    n = np.concatenate([np.full(kept, 3), rng.integers(0, 3, dropped)])
    rng.shuffle(n)
    return _read(rng, kept + dropped, n)


ROWS = (0, 1, 63, 64, 65, 127, 128, 129, 200)


def query_counts():
    """rows per read x N x min_n over n in 0 ... 4, then kept counts around N"""
    rng = np.random.default_rng(1717)
    out = [QueryCall("rows %s N %u min_n %u" % (ROWS, N, m), N, m, [_read(rng, r) for r in ROWS]) for N in (8, 64, 72, 2048) for m in (0, 1, 3)]
    for N in (8, 64, 72, 2048):
        reads = [_kept_read(rng, N + d, drop) for d in (-1, 0, 1) for drop in (0, 5, 70)]
        reads.append(_read(rng, N, np.full(N, 3)))                       # N reached exactly at the read's end ...
        reads.append(_read(rng, N + 64, np.full(N + 64, 4)))             # ... at a turn's last row when N % 64 == 0, in the middle of one otherwise
        reads.append(_read(rng, 200, np.concatenate([np.full(36, 0), np.full(164, 3)])))   # the N-th kept row in the middle of a turn
        reads.append(_read(rng, 150, rng.integers(0, 3, 150)))           # every event dropped
        reads.append(_read(rng, 64, np.full(64, 2)))
        out.append(QueryCall("kept around N %u" % N, N, 3, reads))
    return out


def query_tables():
    rng = np.random.default_rng(7171)
    out = []
    n = np.full(200, 2)
    n[[61, 62, 63, 64, 65, 127, 128, 191]] = 0
    seam = _read(rng, 200, n)
    n2 = np.zeros(200)
    n2[[63, 64, 127, 128, 199]] = 1
    out.append(QueryCall("drops straddling a seam", 256, 1, [seam, _read(rng, 200, n2), _read(rng, 130, np.r_[np.zeros(64), np.ones(66)])]))
    special = np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FFFFFFF, 0x80000000, 0, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001] * 7, np.uint32)
    out.append(QueryCall("NaN and -0 means", 72, 0, [(special, np.ones(len(special))), (special[:5], np.zeros(5))]))
    reads = [_read(rng, r) for r in (70, 5, 130, 64)]
    out.append(QueryCall("an error verdict", 64, 1, reads, result=np.array([400, E_FIRST, 0xFFFFFFFF, 0], np.uint32)))
    out.append(QueryCall("result NULL", 64, 1, reads))
    out.append(QueryCall("index NULL", 64, 2, reads, use_index=False))
    own = [0, 70, 75, 205, 269]
    out.append(QueryCall("event_first descending", 64, 1, reads, event_first=[0, 70, 69, 205, 269]))
    out.append(QueryCall("event_first behind event_rows", 64, 1, reads, event_first=[0, 70, 75, 205, 270]))
    out.append(QueryCall("event_first far behind event_rows", 64, 1, reads, event_first=[0, 70, 75, 205, 1 << 63]))
    out.append(QueryCall("a read of 2^31 rows", 64, 1, reads, event_first=own[:4] + [205 + (1 << 31)], event_rows=205 + (1 << 31)))
    out.append(QueryCall("a read of 2^31 - 1 rows behind the arena is refused by event_rows", 64, 1, reads, event_first=own[:4] + [205 + MAX_ROWS]))
    out.append(QueryCall("3 000 one-row reads", 8, 1, [_read(rng, 1) for _ in range(3000)]))
    out.append(QueryCall("no rows at all", 16, 0, [_read(rng, 0) for _ in range(5)]))
    return out


def query_catalogue():
    return query_counts() + query_tables()

"""CPU tests of tests/locate_path_ref.py, the statement the locate path call is held to (include/vbz_gpu.h: vbz_gpu_locate_path_batch): it is
match_path_ref.path_pair with its arguments exchanged, so it is held to match_path_ref.all_paths with the roles swapped on EVERY tiny pair
over a 2-level alphabet, to locate_span_ref for (cost, start), to recost and the five invariants of the header; paths() -- the pair rules
and the batched walk -- to the statement pair by pair; query_valid to the clamps; and the catalogue is counted."""
import itertools

import numpy as np

import locate_path_ref as LP
import locate_span_ref as LS
import match_path_ref as P
import match_ref as M
from vbz_compression_amd import _lib


def check_invariants(levels, target, a, b, hit, rows):
    cost, end, start, n = hit
    assert (end, n) == (b, len(levels))
    assert rows[0][0] == start and rows[-1][1] == b and a <= start < b
    assert (rows[:, 0] < rows[:, 1]).all()
    for i in range(n - 1):
        assert rows[i + 1][0] in (rows[i][1] - 1, rows[i][1]), (i, rows[i].tolist(), rows[i + 1].tolist())
    assert P.recost(levels, target, rows) == cost


def test_every_tiny_pair_over_two_levels():
    """every query of 1 ... 4 levels against every target of 1 ... 6 levels, both over {0, 3}: the traced path is a warping path of the
    least cost to (n - 1, L - 1), its start the smallest among those, by all_paths with the query in the reference's place"""
    pairs = 0
    for n in range(1, 5):
        for L in range(1, 7):
            for levels in itertools.product((0, 3), repeat=n):
                for target in itertools.product((0, 3), repeat=L):
                    hit, rows = LP.path_pair(levels, target, 0, L)
                    every = P.all_paths(levels, target)
                    least = min(e[0] for e in every)
                    assert hit[0] == least and hit[2] == min(e[1] for e in every if e[0] == least)
                    cells = P.backtrace(P.key_matrix(levels, target))
                    assert (least, hit[2], cells) in every
                    for i in range(n):
                        assert sorted(j for r, j in cells if r == i) == list(range(int(rows[i][0]), int(rows[i][1])))
                    pairs += 1
    assert pairs == sum(2 ** n for n in range(1, 5)) * sum(2 ** L for L in range(1, 7))


def test_span_agreement_and_invariants_on_random_pairs():
    rng = np.random.default_rng(4310)
    for trial in range(600):
        alpha = int(rng.integers(1, 4))
        n, L = int(rng.integers(1, 12)), int(rng.integers(1, 40))
        levels, target = rng.integers(-alpha, alpha + 1, n), rng.integers(-alpha, alpha + 1, L)
        a = int(rng.integers(0, L))
        b = int(rng.integers(a + 1, L + 1))
        hit, rows = LP.path_pair(levels, target, a, b)
        assert (hit, rows.tolist()) == (lambda h, r: (h, r.tolist()))(*LP.path_pair(levels, target, a, b, brute=True))
        check_invariants(levels, target, a, b, hit, rows)
        cost, end, start = LS.span(levels, target)
        for a2 in {start, int(rng.integers(0, start + 1)), 0}:   # (a, b) the span, and any a' <= start with the same b
            h2, r2 = LP.path_pair(levels, target, a2, end)
            assert h2 == (cost, end, start, n), (levels.tolist(), target.tolist(), a2)
            check_invariants(levels, target, a2, end, h2, r2)


def test_paths_applies_the_pair_rules():
    query = np.zeros((3, 16), np.float32)
    query[0, :3] = [1, 2, 3]
    target = np.zeros((2, 32), np.int8)
    target[0, 4:10] = [1, 1, 2, 3, 3, 0]
    valid, lens = [3, 0, 0xFFFFFFFF], [20, 33]
    pairs = [(0, 0, 0, 8), (3, 0, 0, 8), (0, 2, 0, 8), (0, LP.NONE, 0, 0), (0, 0, 4, 4), (0, 0, 5, 4), (1, 0, 0, 8), (0, 1, 0, 8), (0, 0, 13, 21),
             (0, 0, 0, 17), (0, 0, 4, 20), (2, 0, 19, 20)]
    hit, rows = LP.paths(query, valid, 1.0, target, lens, pairs, 16)
    assert hit[0].tolist() == [0, 8, 4, 3] and rows[0, :3].tolist() == [[4, 6], [6, 7], [7, 8]] and not rows[0, 3:].any()
    assert (hit[1:10] == np.array(LP.EMPTY, np.uint32)).all() and not rows[1:10].any()
    assert hit[10].tolist() == list(LP.path_pair([1, 2, 3], target[0, :20], 4, 20)[0]) and hit[10][1] == 20   # max_width levels wide, b == L
    assert hit[11].tolist() == [0, 20, 19, 16] and rows[11].tolist() == [[19, 20]] * 16   # valid above N is clamped to N


def test_paths_is_the_statement_pair_by_pair():
    calls = LP.catalogue()
    for index in [i for i, c in enumerate(calls) if c.name in ("ties", "planted", "lowest", "bytes-residues")]:
        c = calls[index]
        query, valid, target, target_len = c.call.arrays()
        hit, rows = LP.expected(index)
        for p, (rd, tg, a, b) in enumerate(c.pairs):
            n, L = min(int(valid[rd]), c.call.N), int(target_len[tg])
            h, r = LP.path_pair(M.quantize(query[rd], c.call.quant)[:n], target[tg, :L], a, b)
            assert hit[p].tolist() == list(h) and rows[p, :n].tolist() == r.tolist() and not rows[p, n:].any(), (c.name, p)
            check_invariants(M.quantize(query[rd], c.call.quant)[:n], target[tg, :L].astype(np.int64), a, b, h, r)


def test_query_valid():
    E = LP.E_FIRST
    assert E == _lib.VBZ_DEVICE_ERROR and _lib.is_error(E) and not _lib.is_error(E - 1)
    res = [4 * 100, 4 * 5, 0, E, 0xFFFFFFFF, 4 * 3000, 4 * 100]
    assert LP.query_valid(res, 64).tolist() == [64, 5, 0, 0, 0, 64, 64]
    assert LP.query_valid(res, 64, begin=[90, 9, 0, 0, 0, 2990, 0xFFFFFFFF], end=[0xFFFFFFFF, 3, 7, 1, 1, 3001, 50]).tolist() == [10, 0, 0, 0, 0, 10, 0]


def tie_count(levels, target, a, b):
    """cells of the traced path at which all three predecessors hold the same pair"""
    K = P.key_matrix(levels, [int(v) for v in target[a:b]])
    return sum(1 for i, j in P.backtrace(K) if i > 0 and j > 0 and K[i - 1][j - 1] == K[i - 1][j] == K[i][j - 1])


def test_catalogue_count():
    calls = LP.catalogue()
    names = [c.name for c in calls]
    assert names == ["rows-small", "rows-large", "bytes-residues", "bytes-a0", "bytes-bL", "bytes-junk", "bytes-blocks", "ties", "planted", "lowest",
                     "keys-4096", "keys-4104", "beyond"]
    assert [len(c.pairs) for c in calls] == [136 * 18, 11 * 18, 64, 20, 20, 20, 48, 72, 10, 24, 4, 4, 1]
    for c in calls:
        assert c.max_width % 8 == 0 and 8 <= c.max_width <= 65536 and c.call.N % 8 == 0 and c.call.stride % 16 == 0, c.name
        assert all(0 <= a < b <= c.call.target_len[tg] and b - a <= c.max_width for _, tg, a, b in c.pairs), c.name
    small, large = calls[0], calls[1]
    assert sorted(set(small.call.valid)) == list(range(1, 137)) and sorted(set(large.call.valid)) == LP.ROWS_LARGE
    assert {b - a for _, _, a, b in small.pairs} == {b - a for _, _, a, b in large.pairs} == set(LP.WIDTHS)
    res = calls[2]
    assert {(rd, a % 4, b % 4) for rd, _, a, b in res.pairs} == {(rd, x, y) for rd in (0, 1) for x in range(4) for y in range(4)}
    assert all(L % 4 == 3 for L in calls[4].call.target_len) and all(b == 1003 for _, _, _, b in calls[4].pairs + calls[5].pairs)
    assert {b - a for _, _, a, b in calls[6].pairs} == {255, 256, 257, 511, 512, 513}
    # the planted answers are the statement's
    for index, c in enumerate(calls):
        for p, (hit, rows) in c.planted.items():
            ehit, erows = LP.expected(index)
            assert ehit[p].tolist() == list(hit), (c.name, p, ehit[p].tolist())
            assert erows[p, : hit[3]].tolist() == rows, (c.name, p)
    # sits on row 0, whole and cut by the window
    planted = calls[names.index("planted")]
    hit, rows = LP.expected(names.index("planted"))
    assert rows[0][0].tolist() == [695, 701] and planted.pairs[0][2] < 695, "a sit whole"
    assert rows[1][0].tolist() == [697, 701] and planted.pairs[1][2] == 697, "a sit cut by the window"
    # pairs where all three predecessors tie
    ties = calls[names.index("ties")]
    query, valid, target, target_len = ties.call.arrays()
    tied = [tie_count(M.quantize(query[rd], 1.0)[: valid[rd]], target[tg], a, b) for rd, tg, a, b in ties.pairs]
    assert sum(1 for t in tied if t > 0) >= len(tied) // 2, tied
    # both keys, by the host's rule; the window beyond the swapped route's reach
    assert [w for w in LP.KEY_WIDTHS] == [4096, 4104] and calls[10].pairs[0][2:] == (0, 4096) and calls[10].call.valid[0] == 2048
    assert calls[-1].pairs[0][2] > 65536 and calls[-1].call.stride == 70_016

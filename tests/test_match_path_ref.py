"""CPU tests of tests/match_path_ref.py, the statement the path calls are held to (include/vbz_gpu.h: vbz_gpu_match_path): the facts the
header lists, on random small-alphabet pairs and windows; the enumeration of every path of tiny pairs -- the traced path is one of minimum
cost to (M - 1, b - 1), its start the smallest over all such paths, and it is the one the tie order names; the agreement with
match_span_ref.span_brute; the vectorised matrix against the defining triple loop; the winners' table; a count of the catalogue."""
import numpy as np

import match_path_ref as P
import match_ref as M
import match_span_ref as S


def check_facts(ref, k, a, b, hit, rows):
    cost, end, start, m = hit
    assert (end, m) == (b, len(ref))
    assert rows[0][0] == start and rows[-1][1] == b and a <= start < b
    assert (rows[:, 0] < rows[:, 1]).all()
    for i in range(len(ref) - 1):
        assert rows[i + 1][0] in (rows[i][1] - 1, rows[i][1]), (i, rows[i].tolist(), rows[i + 1].tolist())
    assert P.recost(ref, k, rows) == cost


def test_facts_and_span_brute_on_random_pairs():
    rng = np.random.default_rng(7)
    for trial in range(1500):
        alpha = int(rng.integers(1, 4))
        m, n = int(rng.integers(1, 9)), int(rng.integers(1, 14))
        ref, k = rng.integers(-alpha, alpha + 1, m), rng.integers(-alpha, alpha + 1, n)
        a = int(rng.integers(0, n))
        b = int(rng.integers(a + 1, n + 1))
        hit, rows = P.path_pair(ref, k, a, b)
        assert (hit, rows.tolist()) == (lambda h, r: (h, r.tolist()))(*P.path_pair(ref, k, a, b, brute=True)), "the vectorised matrix"
        check_facts(ref, k, a, b, hit, rows)
        assert hit[2] == a + S.span_matrix(ref, k[a:b])[-1][-1][1], "start == P[M-1][b-1].start"
        # the span call's (start, end) as the window, and any a' <= start with the same end: its cost and start
        cost, end, start = S.span_brute(ref, k)
        for a2 in {start, int(rng.integers(0, start + 1)), 0}:
            h2, r2 = P.path_pair(ref, k, a2, end)
            assert (h2[0], h2[1], h2[2]) == (cost, end, start), (ref.tolist(), k.tolist(), a2)
            check_facts(ref, k, a2, end, h2, r2)


def rule_cells(ref, k):
    """the rule's backtrace written out on match_span_ref.span_matrix's pairs, not on keys"""
    Pm = S.span_matrix(ref, k)
    i, j = len(ref) - 1, len(k) - 1
    cells = [(i, j)]
    while True:
        if i == 0:
            if j > 0 and Pm[0][j - 1][0] == 0:
                j -= 1
            else:
                return cells
        elif j == 0:
            i -= 1
        else:
            three = [Pm[i - 1][j - 1], Pm[i - 1][j], Pm[i][j - 1]]
            i, j = [(i - 1, j - 1), (i - 1, j), (i, j - 1)][three.index(min(three))]
        cells.append((i, j))


def test_every_path_of_tiny_pairs():
    rng = np.random.default_rng(11)
    for trial in range(300):
        alpha = int(rng.integers(1, 3))
        m, n = int(rng.integers(1, 5)), int(rng.integers(1, 7))
        ref, k = rng.integers(-alpha, alpha + 1, m), rng.integers(-alpha, alpha + 1, n)
        hit, rows = P.path_pair(ref, k, 0, n)
        every = P.all_paths(ref, k)
        least = min(e[0] for e in every)
        assert hit[0] == least
        assert hit[2] == min(e[1] for e in every if e[0] == least)
        cells = P.backtrace(P.key_matrix(ref, k))
        assert cells == rule_cells(ref, k), "the path the tie order names"
        assert (least, hit[2], cells) in every, "the traced path is a warping path of the minimum cost"
        # rows are that path's cells, row by row
        for i in range(m):
            cols = sorted(j for r, j in cells if r == i)
            assert cols == list(range(int(rows[i][0]), int(rows[i][1])))


def test_sits_verticals_and_single_rows():
    # a sit of cost 0 on row 0, whole and cut by the window; M = 1; W = 1: all vertical
    ref, k = [5, 9], [1, 5, 5, 5, 9, 1]
    assert P.path_pair(ref, k, 0, 5)[0] == (0, 5, 1, 2) and P.path_pair(ref, k, 0, 5)[1].tolist() == [[1, 4], [4, 5]]
    assert P.path_pair(ref, k, 2, 5)[0] == (0, 5, 2, 2)
    assert P.path_pair([5], k, 0, 4)[0] == (0, 4, 1, 1) and P.path_pair([5], k, 0, 5)[0] == (4, 5, 1, 1)
    hit, rows = P.path_pair([1, 2, 3], k, 3, 4)
    assert hit == (4 + 3 + 2, 4, 3, 3) and rows.tolist() == [[3, 4]] * 3


def test_best():
    E = P.EMPTY[0]
    spans = np.array([[[5, 9, 2, 0], [3, 7, 1, 0], [3, 8, 4, 0]], [[E, 0, 0, 0]] * 3, [[E, 0, 0, 0], [9, 4, 2, 0], [E, 0, 0, 0]]], np.uint32)
    assert P.best(spans).tolist() == [[0, 1, 1, 7], [1, P.NONE, 0, 0], [2, 1, 2, 4]]
    assert P.best(spans, 3).tolist() == [[0, 1, 1, 7], [1, P.NONE, 0, 0], [2, P.NONE, 0, 0]]
    assert P.best(spans, 2).tolist() == [[0, P.NONE, 0, 0], [1, P.NONE, 0, 0], [2, P.NONE, 0, 0]]


def test_paths_empty_verdicts():
    query = np.zeros((2, 16), np.float32)
    ref = np.zeros((2, 16), np.int8)
    pairs = [(0, 0, 0, 8), (2, 0, 0, 8), (0, 2, 0, 8), (0, P.NONE, 0, 0), (0, 0, 4, 4), (0, 0, 5, 4), (0, 0, 0, 11), (0, 0, 0, 9), (1, 0, 0, 8), (0, 1, 0, 8)]
    hit, rows = P.paths(query, [10, 7], 1.0, ref, [3, 17], pairs, 8)
    assert hit[0].tolist() == [0, 8, 0, 3] and rows[0, :3].tolist() == [[0, 6], [6, 7], [7, 8]] and not rows[0, 3:].any()
    assert (hit[1:] == np.array(P.EMPTY, np.uint32)).all() and not rows[1:].any()
    assert P.paths(query, None, 1.0, ref, [3, 17], [(1, 0, 8, 16)], 8)[0].tolist() == [[0, 16, 8, 3]]


def test_catalogue_count():
    calls = P.catalogue()
    assert [c.name for c in calls] == ["lengths", "ties", "planted", "large", "rule-4096-2048", "rule-8192-2048", "rule-16384-416", "rule-32768-416"]
    lengths = calls[0]
    assert len(lengths.pairs) == len(M.LENGTHS_M) * len(P.WIDTHS) and {b - a for _, _, a, b in lengths.pairs} == set(P.WIDTHS)
    assert {1, 2, 7, 8, 9, 63, 64, 65, 129} <= set(P.WIDTHS)
    assert sorted(set(lengths.call.ref_len)) == M.LENGTHS_M
    assert calls[3].pairs == [(0, 0, 0, 4096)] and calls[3].call.ref_len == [2048]
    assert sum(len(c.pairs) for c in calls) == 342 + 112 + 11 + 1 + 4 * 16
    for c in calls:
        assert c.max_width % 8 == 0 and all(0 <= a < b <= c.call.N and b - a <= c.max_width for _, _, a, b in c.pairs), c.name
    # the planted answers
    hit, rows = P.expected(2)
    assert hit[0].tolist() == [0, 117, 95, 17] and hit[1].tolist() == [0, 117, 97, 17] and rows[0][0].tolist() == [95, 101]
    assert hit[5].tolist() == [0, 209, 200, 1] and hit[6][2] == 219 and hit[7].tolist() == [0, 205, 204, 1]
    assert hit[9].tolist() == [5, 8, 7, 5] and rows[9][:5].tolist() == [[7, 8]] * 5
    # both sides of the rule: one answer
    assert all((P.expected(i)[0] == P.expected(4)[0]).all() for i in (5, 6, 7))

"""CPU tests of the span reference (tests/match_span_ref.py; the rule: include/vbz_gpu.h, vbz_gpu_match_span): the row-by-row numpy
statement against the defining triple loop over the tie calls and against the enumeration of every path on tiny pairs, its (cost, end)
against match_ref everywhere, the header's fact 1 on random pairs, the planted answers, and the conditions the catalogue must meet to
test anything: pairs with more than one start among their minimum-cost paths, and a start moved by a zero-cost sit on row 0."""
import functools

import numpy as np

import match_ref as M
import match_span_ref as S


def pairs_of(call):
    """(read, ref, k, r) of every pair of a call with a query and a legal reference"""
    query, valid, ref, ref_len = call.arrays()
    K = M.quantize(query, call.quant)
    for i, v in enumerate(valid.tolist()):
        n = min(v, call.N)
        for j, m in enumerate(ref_len.tolist()):
            if n > 0 and 0 < m <= call.stride:
                yield i, j, K[i, :n], ref[j, :m]


def tie_calls():
    return [(i, c) for i, c in enumerate(S.span_catalogue()) if c.name.startswith("ties")]


@functools.lru_cache(maxsize=None)
def tie_matrices():
    """{(call index, read, ref): (k, r, P)} by the defining loop, once"""
    return {(ci, i, j): (k, r, S.span_matrix(r, k)) for ci, c in tie_calls() for i, j, k, r in pairs_of(c)}


def test_rows_equal_the_defining_loop_over_the_tie_calls():
    assert len(tie_matrices()) >= 3 * 28
    for (ci, i, j), (k, r, P) in tie_matrices().items():
        want = S.first_end(P)
        got = S.expected(ci)[i][j]
        assert tuple(int(v) for v in got) == want + (0,), (S.span_catalogue()[ci].name, i, j, got.tolist(), want)
        assert want[2] < want[1]


def test_rows_equal_every_path_on_tiny_pairs():
    rng = np.random.default_rng(77)
    checked = 0
    for t in range(2400):
        a = int(rng.integers(1, 4))
        m, n = int(rng.integers(1, 5)), int(rng.integers(1, 7))
        r, k = rng.integers(-a, a + 1, m), rng.integers(-a, a + 1, n)
        want = S.span_paths(r, k)
        assert S.span_brute(r, k) == want, (r.tolist(), k.tolist())
        cost, end, start = S.span_batch(r, k[None, :], [n])
        assert (int(cost[0]), int(end[0]), int(start[0])) == want, (r.tolist(), k.tolist())
        checked += 1
    assert checked >= 2000


def test_cost_and_end_are_match_refs_everywhere():
    for base, calls in ((True, M.catalogue()), (False, S.span_catalogue())):
        for index, c in enumerate(calls):
            got = S.expected(index, base)
            query, valid, ref, ref_len = c.arrays()
            used = max(1, min(int(valid.max()), c.N))   # (the padding behind the longest query is not walked twice)
            want = M.expected(index) if base else M.hits(query[:, :used], valid, c.quant, ref, ref_len)
            assert (got[:, :, :2] == want).all(), c.name
            assert (got[:, :, 3] == 0).all()
            empty = got[:, :, 0] == 0xFFFFFFFF
            assert (got[empty] == np.array(S.EMPTY, np.uint32)).all(), c.name
            assert (got[~empty][:, 2] < got[~empty][:, 1]).all(), c.name


def test_the_first_end_has_the_smallest_start():
    """fact 1: the lexicographic argmin of the last row is (the first column of the minimum cost, that column's start)"""
    rng = np.random.default_rng(78)
    for t in range(10_000):
        m, n = int(rng.integers(1, 9)), int(rng.integers(1, 13))
        r, k = rng.integers(-3, 4, m), rng.integers(-3, 4, n)
        last = S.span_matrix(r, k)[-1]
        lex = min(range(n), key=lambda j: (last[j], j))
        cost = min(p[0] for p in last)
        first = next(j for j in range(n) if last[j][0] == cost)
        assert lex == first and last[lex] == (cost, min(p[1] for p in last if p[0] == cost)), (r.tolist(), k.tolist())


def test_planted_answers():
    planted = 0
    for index, c in enumerate(S.span_catalogue()):
        for (read, ref), hit in c.planted.items():
            assert tuple(int(v) for v in S.expected(index)[read][ref]) == hit + (0,), (c.name, read, ref)
            planted += 1
    assert planted >= 15
    names = [c.name for c in S.span_catalogue()]
    e = S.expected(names.index("extreme-packed"))
    assert e[0][0].tolist() == [520_192, 1, 0, 0]
    assert S.expected(names.index("extreme-wide"))[0][0].tolist() == [520_192, 1, 0, 0]


def test_both_sides_of_the_rule_expect_identical_hits():
    rule = [i for i, c in enumerate(S.span_catalogue()) if c.name.startswith("rule")]
    assert [(S.span_catalogue()[i].N, S.span_catalogue()[i].stride) for i in rule] == [(4096, 2048), (8192, 2048), (16384, 416), (32768, 416)]
    for i in rule[1:]:
        assert (S.expected(i) == S.expected(rule[0])).all()


def test_the_catalogue_has_ties_and_a_sit_on_row_0():
    """asserted, not measured: at least 64 pairs whose smallest start is not the start of a diagonal-first backtrace -- more than one start
    among the minimum-cost paths to `end` -- and at least one pair whose start moved because a path sat on row 0 at cost 0"""
    several, sat = 0, 0
    for (ci, i, j), (k, r, P) in tie_matrices().items():
        cost, end, start = S.first_end(P)
        back = S.diagonal_first_start(r, k, P, end)
        assert start <= back
        several += start < back
        if len(r) <= 129:   # (the loop once more without the sit, on the shorter references)
            sat += S.span_brute(r, k, sit=False) != (cost, end, start)
    assert several >= 64, several
    assert sat >= 1, sat

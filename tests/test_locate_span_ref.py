"""CPU tests of the numpy statements of the locate-span rule (tests/locate_span_ref.py; include/vbz_gpu.h: vbz_gpu_locate_span_batch): the
row form against match_span_ref's triple loop and its enumeration of every path with the roles swapped, against match_span_ref.spans and
locate_ref.hits; the reversed anchored DP against the forward statement; the monotone column minima; the model of the device's two-step
front rule; the planted answers and a count of the catalogue."""
import collections
import itertools

import numpy as np

import locate_ref as LR
import locate_span_ref as LS
import match_ref as M
import match_span_ref as S


def random_pair(rng, run=False):
    """a small pair over a small alphabet (+-2 or +-3), -128 among the target's levels; run: long runs of the query's first level"""
    a = int(rng.integers(2, 4))
    n, L = int(rng.integers(1, 14)), int(rng.integers(1, 40))
    levels = rng.integers(-a, a + 1, n)
    target = rng.integers(-a, a + 1, L)
    if run:
        at = int(rng.integers(0, L))
        target[at : at + int(rng.integers(1, 20))] = levels[0]
    if rng.integers(0, 4) == 0:
        target[rng.integers(0, L)] = -128
    return levels, target


def test_row_form_against_the_triple_loop():
    rng = np.random.default_rng(4230)
    for x in range(400):
        levels, target = random_pair(rng, run=x % 2 == 1)
        # rows the query, columns the target: span_matrix's `ref` is the sequence aligned whole
        want = S.first_end(S.span_matrix(levels, target))
        assert LS.span(levels, target) == want == S.span_brute(levels, target), (levels.tolist(), target.tolist())
    assert LS.span([], [1, 2]) == LS.EMPTY[:3] and LS.span([1], []) == LS.EMPTY[:3]


def test_row_form_against_every_path():
    """every pair span_paths can enumerate (at most 4 rows x 6 columns) over the levels -1, 0, 1: all 3^3 queries of 3 levels against all
    targets of up to 4, and random ones up to 4 x 6"""
    seen = 0
    for n in (1, 2, 3):
        for levels in itertools.product((-1, 0, 1), repeat=n):
            for L in (1, 2, 3, 4):
                for target in itertools.product((-1, 0, 1), repeat=L):
                    assert LS.span(levels, target) == S.span_paths(levels, target), (levels, target)
                    seen += 1
    rng = np.random.default_rng(4231)
    for _ in range(150):
        levels, target = rng.integers(-2, 3, int(rng.integers(1, 5))), rng.integers(-2, 3, int(rng.integers(1, 7)))
        assert LS.span(levels, target) == S.span_paths(levels, target), (levels.tolist(), target.tolist())
    assert seen == (3 + 9 + 27) * (3 + 9 + 27 + 81)


def swap_arrays(rng):
    N, stride = 48, 96
    query = (rng.integers(-3, 4, (9, N)) / 32.0).astype(np.float32)
    query[3, 5] = np.nan
    valid = np.array([48, 1, 17, 48, 0, 33, 500, 0xFFFFFFFF, 2], np.uint64)
    target = rng.integers(-3, 4, (7, stride)).astype(np.int8)
    target_len = np.array([96, 1, 40, 0, 97, 0xFFFFFFFF, 64], np.uint64)
    return query, valid, target, target_len


def test_swap_identity_and_cost_end():
    """spans(query, valid, target, target_len)[i][g] == match_span_ref.spans(target as the query, target_len, levels as references, n)[g][i]
    for targets without -128, and (cost, end) == locate_ref.hits with -128 among them"""
    rng = np.random.default_rng(4232)
    query, valid, target, target_len = swap_arrays(rng)
    N, stride = query.shape[1], target.shape[1]
    got = LS.spans(query, valid, 32.0, target, target_len)
    levels = M.quantize(query, 32.0).astype(np.int8)
    n = np.minimum(valid, N)
    tvalid = np.where((target_len != 0) & (target_len <= stride), target_len, 0)
    want = S.spans(target.astype(np.float32) / np.float32(32.0), tvalid, 32.0, levels, n)
    assert (got == want.transpose(1, 0, 2)).all()
    empty = np.array(LS.EMPTY, np.uint32)
    assert (got[4] == empty).all() and (got[:, 3] == empty).all() and (got[:, 4] == empty).all() and (got[:, 5] == empty).all()
    assert got[0][0].tolist() != list(LS.EMPTY) and (got[:, :, 3] == 0).all()
    lowest = np.array(target)
    lowest[rng.integers(0, 2, lowest.shape) == 0] = -128
    got = LS.spans(query, valid, 32.0, lowest, target_len)
    assert (got[:, :, :2] == LR.hits(query, valid, 32.0, lowest, target_len)).all()
    ok = got[:, :, 0] != LS.EMPTY[0]
    assert (got[:, :, 2][ok] < got[:, :, 1][ok]).all()


def test_walk_back_is_the_forward_statement():
    """the reversed anchored DP gives the row form's start on some thousands of pairs, reading no further than the first column whose
    minimum exceeds cost; and column minima never decrease"""
    rng = np.random.default_rng(4233)
    stopped = 0
    for x in range(4000):
        levels, target = random_pair(rng, run=x % 2 == 1)
        cost, end, start = LS.span(levels, target)
        got, walked = LS.walk_back(levels, target, cost, end)
        assert got == start, (levels.tolist(), target.tolist(), (cost, end, start), got)
        stopped += walked < end
        mins = LS.back_matrix(levels, target, end).min(axis=0)
        assert (np.diff(mins) >= 0).all(), (levels.tolist(), target.tolist())
    assert stopped > 1000, stopped


def test_front_rule_never_stops_early():
    """the model of the device's rule at c = 1, 2, 4: its stop never comes before the step that computes the last cell of the tracked row
    that holds cost -- and it does stop before the target's first level on more than half of the pairs whose stretch leaves it room"""
    rng = np.random.default_rng(4234)
    pairs = stops = 0
    for x in range(3000):
        levels, target = random_pair(rng, run=x % 3 == 1)
        c = (1, 2, 4)[x % 3]
        cost, end, start = LS.span(levels, target)
        D = LS.back_matrix(levels, target, end)
        stop, last = LS.front_stop(D, cost, c)
        assert stop is None or stop >= last, (levels.tolist(), target.tolist(), c, stop, last)
        assert end - 1 - (last - (len(levels) - 1) // c) == start
        pairs += 1
        stops += stop is not None
    assert pairs == 3000 and stops > 1500, (pairs, stops)


def test_the_wavefront_restated():
    """the kernel's walk back, lane by lane in numpy, at c = 1, 2, 4: the statement's start, and exactly the steps the model of its rule
    counts -- on plants behind runs of the query's first level, where the walk is long, stops early, and end - 1 takes every residue"""
    rng = np.random.default_rng(4236)
    early, residues = 0, set()
    for x in range(45):
        c = (1, 2, 4)[x % 3]
        n, L = int(rng.integers(1, 64 * c + 1)), int(rng.integers(600, 2400))
        levels = rng.integers(-40, 41, n)
        target = rng.integers(60, 100, L)
        if x % 9 == 0:
            target[rng.integers(0, L)] = -128
        at = int(rng.integers(300, L - n)) if L - n > 300 else 0
        target[at : at + n] = levels
        run = int(rng.integers(0, min(at, 600) + 1))
        target[at - run : at] = levels[0]
        cost, end, start = LS.span(levels, target)
        got, steps = LS.wavefront_back(levels, target, cost, end, c)
        assert got == start, (x, c, n, L, (cost, end, start), got)
        assert steps == LS.steps_back(levels, target, cost, end, start, c), (x, c, n, L)
        early += steps < end + (n - 1) // c
        residues.add((end - 1) % 4)
    assert early > 30 and residues == {0, 1, 2, 3}, (early, residues)


def test_planted_answers():
    seen = collections.Counter()
    for call in LS.catalogue():
        if not isinstance(call, LS.Call):
            continue
        query, valid, target, target_len = call.arrays()
        for (read, tg), hit in call.planted.items():
            if call.name == "span-long":   # (the long call's numpy runs once, in the device test; here the walk back alone, from the known hit)
                levels = M.quantize(query[read : read + 1], call.quant)[0, : valid[read]]
                assert LS.walk_back(levels, target[tg, : target_len[tg]], hit[0], hit[1])[0] == hit[2]
            else:
                got = LS.spans(query[read : read + 1], valid[read : read + 1], call.quant, target[tg : tg + 1], target_len[tg : tg + 1])[0][0]
                assert tuple(int(v) for v in got) == hit + (0,), (call.name, read, tg, got.tolist(), hit)
            assert hit[2] < hit[1]
            seen[call.name] += 1
    per_n = 3 + 1 + 1 + 2 * len(LS.RUNS) + 1
    assert seen == {"span-planted-17": per_n, "span-planted-129": per_n, "span-planted-600": per_n, "span-edges": 9 + 1, "span-extremes": 4,
                    "span-long": 1}, seen
    long = LS.catalogue()[-1]
    assert list(long.planted.values()) == [(0, LR.LONG_END, LS.LONG_START)] and LR.LONG_END - LS.LONG_START > 50_000 and LR.LONG_END > 65536


def test_catalogue_counted():
    """all six rows-per-lane, every plant kind, the refusals"""
    by_c = collections.Counter()
    for call in LS.catalogue():
        assert call.N % 8 == 0 and 8 <= call.N <= 2048 and call.stride % 16 == 0
        for n, L in call.pairs():
            by_c[LR.rows_per_lane(n)] += 1
    assert sorted(by_c) == list(LR.ROWS) and all(by_c[c] >= 20 for c in LR.ROWS), by_c
    p = next(c for c in LS.catalogue() if c.name == "span-edges")
    assert 0 in p.valid and 5000 in p.valid and 0xFFFFFFFF in p.valid and {0, p.stride + 1, 0xFFFFFFFF} <= set(p.target_len)
    hits = list(p.planted.values())
    assert {(h[1] - 1) % 4 for h in hits} == {0, 1, 2, 3} and {255, 256, 257} <= {h[1] for h in hits} and (0, 1, 0) in hits
    for n in (17, 129, 600):
        p = next(c for c in LS.catalogue() if c.name == "span-planted-%d" % n)
        hits = list(p.planted.values())
        assert sum(1 for h in hits if h[2] == 0) == 1 + len(LS.RUNS)                 # the plant and the runs at the target's very start
        assert sum(1 for h in hits if h[1] == p.stride) == 1                         # ... at its very end
        assert {h[1] - h[2] for h in hits} >= {n + r for r in LS.RUNS} | {n, 3 * n - 2}

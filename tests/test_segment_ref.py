"""CPU tests of tests/segment_ref.py, the numpy statement of the segmentation rule (include/vbz_gpu.h: vbz_gpu_segmentation), against a
brute-force loop over positions and neighbours that follows the header's text line by line, and against the properties the header
states: the row bound, the spacing of boundaries, the shortest signals a detector sees, constants and steps, invariance under offset and
scale, and ties (of equal scores the first wins)."""
import numpy as np
import pytest

import segment_ref as S

PARAMS = [(3, 6, 4.0, 9.0, 2), (1, 0, 1.5, 1.0, 1), (32, 32, 2.0, 3.0, 32), (3, 6, 4.0, 9.0, 32), (5, 2, 0.75, 6.5, 4)]


def brute_scores(x, P):
    w1, w2, t1, t2, r = P
    x = [int(v) for v in x]
    T = len(x)
    s = [0.0] * (T + 1)
    for w, t in ((w1, t1), (w2, t2)):
        if w == 0:
            continue
        tt = np.float64(np.float32(t)) * np.float64(np.float32(t))
        for q in range(w, T - w + 1):
            a, b = x[q - w : q], x[q : q + w]
            A, B = sum(a), sum(b)
            A2, B2 = sum(v * v for v in a), sum(v * v for v in b)
            N = w * (A - B) ** 2
            D = max(w * (A2 + B2) - A * A - B * B, 1)
            assert N < 1 << 47 and D < 1 << 43
            s[q] = max(s[q], float((np.float64(N) / np.float64(D)) / tt))
    return s


def brute_starts(x, P):
    r = P[4]
    T = len(x)
    if T == 0:
        return []
    s = brute_scores(x, P)
    out = [0]
    for q in range(1, T):
        if s[q] >= 1 and all(s[q] > s[j] for j in range(max(q - r, 0), q)) and all(s[q] >= s[j] for j in range(q + 1, min(q + r, T) + 1)):
            out.append(q)
    return out


def steps(rng, T, lo=3, hi=30, noise=6.0):
    """a step signal of random dwell under Gaussian noise"""
    x, p = np.zeros(T), 0
    while p < T:
        d = int(rng.integers(lo, hi + 1))
        x[p : p + d] = rng.uniform(-600, 900)
        p += d
    return np.clip(x + rng.normal(0, noise, T), -32768, 32767).astype(np.int16)


def square(T, half, lo=100, hi=500, phase=0):
    return np.where(((np.arange(T) + phase) // half) % 2 == 0, lo, hi).astype(np.int16)


def check(x, P):
    got = S.starts(x, None, None, P)
    assert got.dtype == np.uint32
    assert got.tolist() == brute_starts(x, P), (len(x), P)
    T, r = len(x), P[4]
    assert len(got) <= S.max_rows(T, r) and (T == 0) == (len(got) == 0)
    assert (np.diff(got.astype(np.int64))[1:] > r).all()   # (two boundaries; row 0 is no boundary)
    return got


@pytest.mark.parametrize("P", PARAMS)
def test_random_and_built_signals_against_the_loop(P):
    rng = np.random.default_rng(P[0] * 100 + P[4])
    for T in (0, 1, 2, 5, 63, 64, 65, 300, 1000):
        check(steps(rng, T), P)
        check(rng.integers(-32768, 32768, T).astype(np.int16), P)
        check(rng.integers(0, 65536, T).astype(np.uint16), P)
        check(np.full(T, 17, np.int16), P)


@pytest.mark.parametrize("P", PARAMS)
def test_shortest_signals(P):
    w1, w2 = P[0], P[1]
    rng = np.random.default_rng(7)
    for T in sorted({0, 1, max(2 * w1 - 1, 0), 2 * w1, max(2 * w2 - 1, 0), 2 * w2, 2 * w1 + 1, 2 * w2 + 1}):
        x = np.concatenate([np.full(T // 2, -300), np.full(T - T // 2, 700)]).astype(np.int16)
        got = check(x, P)
        if T < 2 * w1 and (w2 == 0 or T < 2 * w2):
            assert got.tolist() == ([0] if T else []), (T, P)   # (no detector sees a position)
        check(steps(rng, T, 1, 3), P)


def test_a_constant_read_has_one_row_and_a_step_one_boundary_at_the_step():
    for P in PARAMS:
        assert S.starts(np.full(500, -4321, np.int16), None, None, P).tolist() == [0]
        for at in (P[0], max(P[0], P[1]), 250, 500 - max(P[0], P[1])):
            x = np.concatenate([np.full(at, 100), np.full(500 - at, 900)]).astype(np.int16)
            got = S.starts(x, None, None, P).tolist()
            assert got == [0, at], (P, at, got)
            assert got == brute_starts(x, P)


def test_invariance_under_offset_and_scale():
    rng = np.random.default_rng(3)
    x = steps(rng, 3000, noise=5.0).astype(np.int64)
    x = np.clip(x, -3000, 3000)
    base = S.starts(x.astype(np.int16), None, None, S.DEFAULT)
    assert len(base) > 50
    for a, c in ((1, 1234), (-1, 0), (3, -7000), (-5, 99), (10, 2000)):
        y = a * x + c
        assert y.min() >= -32768 and y.max() <= 32767
        assert S.starts(y.astype(np.int16), None, None, S.DEFAULT).tolist() == base.tolist(), (a, c)
    y = x + 32768   # (the same signal as uint16)
    assert S.starts(y.astype(np.uint16), None, None, S.DEFAULT).tolist() == base.tolist()


@pytest.mark.parametrize("r", [2, 4])
@pytest.mark.parametrize("half", [3, 4, 5])
def test_ties_the_first_wins(half, r):
    """noise-free square waves: equal scores >= 1 within r of each other occur, and the later one is suppressed.  (Half-period 3 with
    r = 2 is the one combination without such a tie, whatever the amplitude: the steps' equal scores lie 3 apart and the two positions
    between them score 0.75 / t1^2 = 0.1875 -- the quotient does not change under scale.  It runs all the same.)"""
    P = (3, 6, 2.0, 4.0, r)
    x = square(400, half)
    s = S.scores(x, P)
    ties = [(q, j) for q in range(1, 400) for j in range(q + 1, min(q + r, 400) + 1) if s[q] >= 1 and s[q] == s[j]]
    assert bool(ties) == ((half, r) != (3, 2)), (half, r, len(ties))
    got = check(x, P).tolist()
    assert len(got) > 1
    later = {j for q, j in ties}
    assert not (later & set(got)), sorted(later & set(got))[:4]   # (a later equal score within r of an earlier one is no boundary)


def test_ranges_and_tables():
    rng = np.random.default_rng(5)
    reads = [steps(rng, T) for T in (0, 50, 700, 9)]
    first, st = S.tables(reads, [3, 3, 101, 20], [0xFFFFFFFF, 40, 650, 5])
    assert first.dtype == np.int64 and first[0] == 0 and first.tolist() == np.concatenate([[0], np.cumsum([len(v) for v in st])]).tolist()
    assert st[0].tolist() == [] and st[3].tolist() == []   # (an empty read, an empty range)
    assert st[1].tolist() == brute_starts(reads[1][3:40], S.DEFAULT) and st[2].tolist() == brute_starts(reads[2][101:650], S.DEFAULT)

"""CPU tests of the span reference (tests/spans_ref.py): held to a brute-force per-sample loop over random signals and every parameter
corner, the bound with equality, the integer key bounds against the float64 comparison, and the catalogue the GPU tests use -- every
catalogue signal has the spans its test relies on, so no GPU test can pass on empty tables."""
import math

import numpy as np
import pytest

import spans_ref as S

CORNERS = [(d, D, m, p0) for d in (S.ABOVE, S.BELOW) for D in (0, 1, 9, 65535) for m in (1, 2, 7) for p0 in (0, 5, 10_000)]


def brute(x, begin, end, P, a, w):
    """the rule, one sample at a time"""
    direction, D, m, p0, f = P
    T = len(x)
    e = T if end is None else min(int(end), T)
    b = 0 if begin is None else min(int(begin), e)
    thr = float(np.float64(np.float32(a)) + np.float64(np.float32(f)) * np.float64(np.float32(w)))
    out, first, last = [], None, None
    for q in range(e - b):
        v = float(x[b + q])
        hit = q >= p0 and (v > thr if direction == S.ABOVE else v < thr)
        if not hit:
            continue
        if first is not None and q - last - 1 > D:
            if last + 1 - first >= m:
                out += [first, last + 1]
            first = None
        if first is None:
            first = q
        last = q
    if first is not None and last + 1 - first >= m:
        out += [first, last + 1]
    return out


@pytest.mark.parametrize("signed", [True, False])
def test_reference_against_the_loop(signed):
    rng = np.random.default_rng(3 + signed)
    n_spans = 0
    for k, (d, D, m, p0) in enumerate(CORNERS):
        T = int(rng.integers(0, 400))
        x = rng.integers(300, 500, T).astype(np.int16)
        for _ in range(int(rng.integers(0, 6))):   # planted runs of random length and level
            a = int(rng.integers(0, max(T, 1)))
            x[a : a + int(rng.integers(1, 20))] = 900 if d == S.ABOVE else -20
        if not signed:
            x = (x.astype(np.int32) + 40_000).astype(np.uint16)
        a, w, f = (450.0, 10.0, 2.5) if signed else (40_450.0, 10.0, 2.5)
        if d == S.BELOW:
            a -= 130.0
        for bg, en in ((None, None), (3, None), (None, max(T - 9, 0)), (11, 200), (500, 2)):
            P = (d, D if D < 65535 or k % 2 else 30, m, p0 if p0 < 10_000 or k % 2 else T // 2, f)
            got = S.edges(x, bg, en, P, a, w).tolist()
            assert got == brute(x, bg, en, P, a, w), (P, T, bg, en)
            n_spans += len(got) // 2
    assert n_spans > 200   # (the corners are not all empty)


def test_equal_to_the_threshold_is_not_in_and_nan_inf():
    x = np.array([5, 6, 7, 6, 5], np.int16)
    assert S.edges(x, None, None, (S.ABOVE, 0, 1, 0, 0.0), 6.0, 0.0).tolist() == [2, 3]
    assert S.edges(x, None, None, (S.BELOW, 0, 1, 0, 0.0), 6.0, 0.0).tolist() == [0, 1, 4, 5]
    assert S.edges(x, None, None, (S.ABOVE, 0, 1, 0, 1.0), 5.0, 1.0).tolist() == [2, 3]          # thr = 5 + 1 x 1
    for d in (S.ABOVE, S.BELOW):
        assert S.edges(x, None, None, (d, 0, 1, 0, 0.0), float("nan"), 0.0).tolist() == []
    assert S.edges(x, None, None, (S.ABOVE, 0, 1, 0, 0.0), float("-inf"), 0.0).tolist() == [0, 5]
    assert S.edges(x, None, None, (S.ABOVE, 0, 1, 0, 0.0), float("inf"), 0.0).tolist() == []
    assert S.edges(x, None, None, (S.BELOW, 0, 1, 2, 0.0), float("inf"), 0.0).tolist() == [2, 5]   # (everything in: one span [p0, T'))
    assert S.edges(x, None, None, (S.BELOW, 0, 1, 0, 0.0), float("-inf"), 0.0).tolist() == []


@pytest.mark.parametrize("D", [0, 1, 9, 300])
@pytest.mark.parametrize("m", [1, 2, 7])
def test_the_bound_holds_and_is_reached(D, m):
    rng = np.random.default_rng(D + m)
    period = m + D + 1
    for T in (0, 1, m, period - 1, period, 5 * period - D - 1, 5 * period, 5 * period + 1, 997):
        x = np.zeros(T, np.int16)
        x[np.arange(T) % period < m] = 10   # m in, D + 1 out, ...: every run is a span of its own
        k = len(S.spans(x, None, None, (S.ABOVE, D, m, 0, 0.0), 5.0, 0.0))
        assert k == S.bound(T, D, m), (T, D, m, k)   # equality: the last period needs its m in-positions only
        y = (rng.random(T) < 0.3).astype(np.int16) * 10
        assert len(S.spans(y, None, None, (S.ABOVE, D, m, 0, 0.0), 5.0, 0.0)) <= S.bound(T, D, m)


def thresholds():
    out = [-32768.5, 65535.5, float("inf"), float("-inf"), float("nan"), -32769.0, 65536.0, 1e300, -1e300]
    for c in (-32768.0, -1.0, 0.0, 1.0, 32767.0, 32768.0, 65535.0, 400.0):
        out += [c, float(np.nextafter(c, -np.inf)), float(np.nextafter(c, np.inf)), c - 0.5, c + 0.5]
    return out


@pytest.mark.parametrize("signed", [True, False])
def test_integer_key_bounds_equal_the_float64_comparison(signed):
    """for thr at, just below and just above integers, at -32768.5, 65535.5, +-inf and NaN: lo <= u < hi is exactly the comparison"""
    values = np.arange(-32768, 32768) if signed else np.arange(0, 65536)
    keys = values + (32768 if signed else 0)
    for thr in thresholds():
        for d in (S.ABOVE, S.BELOW):
            lo, hi = S.key_bounds(thr, d, signed)
            assert 0 <= lo <= 65536 and 0 <= hi <= 65536
            with np.errstate(invalid="ignore"):
                want = values.astype(np.float64) > thr if d == S.ABOVE else values.astype(np.float64) < thr
            got = (keys >= lo) & (keys < hi)
            assert np.array_equal(got, want), (thr, d, signed, lo, hi)
            if math.isnan(thr):
                assert not got.any()


# ---- the catalogue the GPU tests run (tests/test_gpu_spans.py imports these) ------------------------------------------------------------------
M = 3
LEVEL = (500.0, 0.0)   # between the baseline (400) and the runs (900)


@pytest.mark.parametrize("D", [0, 1, 9, 65535])
def test_catalogue_has_the_spans_its_tests_rely_on(D):
    cat = S.catalogue(D, M)
    P = (S.ABOVE, D, M, 0, 0.0)
    total = 0
    for name, x in cat:
        sp = S.spans(x, None, None, P, *LEVEL)
        total += len(sp)
        if name.startswith("pair"):
            gap, L = int(name.split("gap")[1].split()[0]), int(name.split("L")[1])
            s = int(name.split()[1][1:])
            if gap == D:      # the two runs merge into one span across the seam, kept whatever L
                assert len(sp) == 1 and sp[0][0] < s <= sp[0][1] and sp[0][1] - sp[0][0] == 2 * L + gap, (name, sp.tolist())
            elif L == M:      # a gap of D + 1: two spans of exactly m, one on either side of the seam
                assert len(sp) == 2 and (sp[:, 1] - sp[:, 0]).tolist() == [M, M] and sp[0][1] <= s <= sp[1][0], (name, sp.tolist())
            else:             # ... and two runs of m - 1: dropped
                assert len(sp) == 0, (name, sp.tolist())
        elif name == "short at both ends":
            # two runs of m - 1 samples: dropped -- unless the gap between them is at most D, when they merge into [0, T)
            assert sp.tolist() == ([[0, len(x)]] if len(x) - 2 * (M - 1) <= D else []), (name, sp.tolist())
        else:
            assert len(sp) == 1, (name, sp.tolist())
    assert total >= 18 if D < 65535 else total >= 12
    names = [n for n, _ in cat]
    for want in ("begins at 8", "begins at 15", "last at 7", "last at 15", "begins at 512", "last at 511", "begins at 2048", "last at 2047", "at 0", "at T - 1"):
        assert want in names, want
    by = dict(cat)
    assert S.spans(by["begins at 15"], None, None, P, *LEVEL)[0][0] == 15 and S.spans(by["last at 7"], None, None, P, *LEVEL)[0][1] == 8
    assert S.spans(by["at T - 1"], None, None, P, *LEVEL)[0][1] == len(by["at T - 1"])


def test_ignore_prefix_cases():
    """p0 inside a run, on its first position and behind the read's end"""
    x = S.baseline(300, [(100, 120)])
    for p0, want in ((110, [110, 120]), (100, [100, 120]), (99, [100, 120]), (120, []), (301, []), (0xFFFFFFFF, [])):
        assert S.edges(x, None, None, (S.ABOVE, 0, 1, p0, 0.0), *LEVEL).tolist() == want, p0
    assert S.edges(x, 50, None, (S.ABOVE, 0, 1, 60, 0.0), *LEVEL).tolist() == [60, 70]   # (positions count from the range's first sample)

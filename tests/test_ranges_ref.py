"""tests/ranges_ref.py held to a brute-force statement on tiny reads: every sample of the range placed on its own into every chunk that
holds it, every other position the pad value; the statistics from a sorted Python list."""
import math

import numpy as np

import norm_ref as R
import pod5_reads_ref as PR
import ranges_ref as G

TO_END = G.TO_END


def brute_range(T, begin, end):
    e = T if end is None else end
    e = e if e < T else T
    b = 0 if begin is None else begin
    b = b if b < e else e
    return b, e


def brute_chunks(x, b, e, L, S, mode, end_align, padb, bits):
    """place sample i (b <= i < e) at range position i - b"""
    Tp = e - b
    if Tp == 0:
        K = 0
    elif Tp <= L:
        K = 1
    else:
        K = (Tp - L + S - 1) // S + 1
    starts = [k * S for k in range(K)]
    if mode == "end" and K >= 2:
        starts[-1] = min(starts[-1], (Tp - L + end_align - 1) // end_align * end_align)
    out = [[padb] * L for _ in range(K)]
    for i in range(len(x)):
        if not (b <= i < e):
            continue
        p = i - b
        for k, s in enumerate(starts):
            if s <= p < s + L:
                out[k][p - s] = int(bits[i])
    return starts, out


RANGES = [(None, None), (0, None), (None, 0), (0, 0), (1, None), (3, 3), (3, 4), (5, 2), (7, TO_END), (8, 20), (9, 1000), (TO_END, TO_END), (1000, 2000),
          (None, 17), (16, 33), (2, 31)]


def test_clamp_and_range_samples():
    for T in (0, 1, 7, 8, 9, 33):
        for bg, en in RANGES:
            assert G.clamp(T, bg, en) == brute_range(T, bg, en), (T, bg, en)
            b, e = G.clamp(T, bg, en)
            assert 0 <= b <= e <= T
    assert G.range_samples([10, 0x80000000, 0xFFFFFFFC, 5], [2, 0, 0, 9], [TO_END, 5, 5, 3]) == [8, 0x80000000, 0xFFFFFFFC, 0]
    assert G.range_samples([10, 4]) == [10, 4]
    assert G.range_samples([10, 4], None, [3, 9]) == [3, 4]


def test_chunks_against_per_sample_placement():
    rng = np.random.default_rng(3)
    for T in (0, 1, 7, 8, 9, 33):
        x = rng.integers(-2000, 2000, T).astype(np.int16)
        for dtype in ("f32", "f16", "bf16"):
            bits = PR.typed_bits(x, 12.5, 0.37, dtype)
            padb = int(PR.pad_bits(-7.0, dtype))
            for L, S, mode, ea in ((8, 8, "pad", 0), (16, 8, "pad", 0), (16, 8, "end", 1), (16, 8, "end", 6), (8, 8, "end", 8), (24, 16, "end", 3)):
                for bg, en in RANGES:
                    b, e = brute_range(T, bg, en)
                    starts, want = brute_chunks(x, b, e, L, S, mode, ea, padb, bits)
                    got_starts, got = G.chunk_rows(x, bg, en, L, S, mode, ea, 12.5, 0.37, -7.0, dtype)
                    assert list(got_starts) == starts, (T, bg, en, L, S, mode, ea)
                    assert got.shape == (len(starts), L) and got.tolist() == want, (T, bg, en, L, S, mode, ea, dtype)


def brute_stats(vals, norm):
    s = sorted(float(v) for v in vals)
    T = len(s)
    if T == 0:
        return 0.0, 0.0
    if norm[0] == R.MED_MAD:
        c = (s[(T - 1) // 2] + s[T // 2]) / 2.0
        d = sorted(abs(v - c) for v in s)
        return c, (d[(T - 1) // 2] + d[T // 2]) / 2.0

    def q(qv):
        h = float(np.float32(qv)) * (T - 1)
        j = math.floor(h)
        t = h - j
        a, bb = s[j], s[min(j + 1, T - 1)]
        return a + (bb - a) * t if t < 0.5 else bb - (bb - a) * (1.0 - t)

    return q(norm[1]) + q(norm[2]), q(norm[2]) - q(norm[1])


def test_statistics_of_the_range_and_of_the_read():
    rng = np.random.default_rng(5)
    for T in (0, 1, 2, 9, 33):
        x = rng.integers(-500, 500, T).astype(np.int16)
        x[: T // 3] += 3000
        for norm in (R.BONITO, R.DORADO):
            for bg, en in RANGES:
                b, e = brute_range(T, bg, en)
                for stats, vals in ((G.STATS_RANGE, x[b:e]), (G.STATS_READ, x)):
                    c, w = brute_stats(vals.tolist(), norm)
                    want = R.constants(c, w, norm)
                    got = G.shift_scale(x, bg, en, norm, stats)
                    assert [np.float32(v).view(np.uint32) for v in got] == [np.float32(v).view(np.uint32) for v in want], (T, bg, en, norm, stats)


def test_pod5_reads_are_their_concatenated_rows():
    rows = [np.arange(5, dtype=np.int16), np.zeros(0, np.int16), np.arange(100, 103, dtype=np.int16), np.arange(7, dtype=np.int16)]
    sig = G.pod5_signals(rows, [0, 3, 3])
    assert [s.tolist() for s in sig] == [[0, 1, 2, 3, 4, 100, 101, 102], [], [0, 1, 2, 3, 4, 5, 6]]
    starts, got = G.chunk_rows(sig[0], 4, 7, 8, 8, "pad", 0, 0.0, 1.0, -1.0, "f32")
    assert list(starts) == [0] and got.view(np.float32).tolist() == [[4.0, 100.0, 101.0, -1.0, -1.0, -1.0, -1.0, -1.0]]

"""CPU tests of tests/trim_ref.py, the numpy statement of the signal trim (include/vbz_gpu.h: vbz_gpu_trim): hand cases for every clause of
the rule, the statement against a plain-loop transcription on random reads, and the generator the GPU tests draw their reads from."""
import numpy as np

import norm_ref as R
import ranges_ref as G
import trim_ref as T

THR = 100.0


def read(n, high=()):
    """n samples at 0 with the given positions (or slices) at 200"""
    x = np.zeros(n, np.int16)
    for p in high:
        x[p] = 200
    return x


def tr(x, W=10, m=3, t0=5, M=1000, max_fraction=1.0, flags=0, thr=THR):
    return T.trim(x, thr, W, m, t0, M, max_fraction, flags)


def test_no_samples_and_fewer_than_min_trim():
    assert tr(read(0)) == 0
    assert tr(read(3)) == 3
    assert tr(read(5)) == 5
    assert tr(read(14)) == 5          # not one whole window behind min_trim
    assert tr(read(4, [slice(0, 4)])) == 4


def test_no_peak_gives_min_trim():
    assert tr(read(200)) == 5
    assert tr(read(200, [7, 30, 31, 90])) == 5   # high samples, never more than m in a window


def test_peak_then_a_quiet_window():
    x = read(200, [slice(25, 42)])    # windows [25, 35) and [35, 45) hold 10 and 7 high samples; [35, 45) ends low
    assert tr(x) == 45
    x = read(200, [slice(0, 35)])     # a plateau in front: windows [5, 15) ... [25, 35) end high, [35, 45) is quiet
    assert tr(x) == 45
    x = read(200, [slice(0, 34)])     # the last sample of [25, 35) is low: the peak ends there
    assert tr(x) == 35


def test_peak_to_the_end_of_the_prefix_gives_min_trim():
    assert tr(read(200, [slice(25, 200)])) == 5
    assert tr(read(200, [slice(25, 200)]), M=100) == 5
    assert tr(read(200, [slice(25, 110)]), M=100) == 5    # it comes down behind max_samples: not seen
    assert tr(read(200, [slice(25, 110)]), M=130) == 115


def test_exactly_min_elements_does_not_open_a_peak():
    x = read(200, [16, 17, 18])              # 3 high samples in [15, 25): not MORE than m = 3
    assert tr(x) == 5
    x = read(200, [16, 17, 18, 19])          # 4: the peak opens, and the window ends low
    assert tr(x) == 25
    assert tr(read(200, [16]), m=0) == 25    # m = 0: one high sample opens it


def test_a_window_whose_last_sample_is_high_continues_whatever_its_count():
    x = read(200, [16, 17, 18, 19, 24, 34, 44])   # [15, 25) opens and ends high; [25, 35) and [35, 45) hold ONE high sample, their last
    assert tr(x) == 55
    x = read(200, [24, 34, 44])                   # the same last samples without a peak in front of them
    assert tr(x) == 5


def test_a_sample_equal_to_the_threshold_is_not_high():
    x = np.zeros(200, np.int16)
    x[15:24] = 100
    assert tr(x) == 5
    x[15:24] = 101
    assert tr(x) == 25
    assert tr(x, thr=100.5) == 25
    assert tr(x, thr=101.0) == 5


def test_reject_at_end():
    x = read(200, [slice(25, 86)])      # the peak ends in the window [85, 95): e = 95
    assert tr(x, M=95) == 95            # N = 95 = e: kept without the flag
    assert tr(x, M=95, flags=T.REJECT_AT_END) == 5
    assert tr(x, M=96, flags=T.REJECT_AT_END) == 95          # e = N - 1
    assert tr(x[:95], flags=T.REJECT_AT_END) == 5            # N = T = 95
    assert tr(x[:96], flags=T.REJECT_AT_END) == 95


def test_max_fraction_on_both_sides_of_its_boundary():
    x = read(200, [slice(25, 42)])      # e = 45
    assert tr(x, max_fraction=0.25) == 45           # 45 <= 50
    assert tr(x, max_fraction=0.125) == 5           # 45 > 25
    assert tr(x[:180], max_fraction=0.25) == 45     # 45 <= 45.0: not beyond
    assert tr(x[:179], max_fraction=0.25) == 5      # 45 > 44.75


def test_shift_of_minus_infinity_makes_every_sample_high():
    thr = T.threshold(np.float32("-inf"), np.float32(3.0), 2.4)
    assert thr == float("-inf")
    assert tr(read(200), thr=thr) == 5                         # every window ends high: the peak never comes down
    x = np.full(200, -32768, np.int16)
    assert T.trim(x, thr, 10, 3, 5, 1000) == 5 and (x.astype(np.float64) > thr).all()


def test_threshold_is_a_multiply_then_an_add_in_float64():
    shift, scale, f = np.float32(401.3), np.float32(17.77), 2.4
    assert T.threshold(shift, scale, f) == float(np.float64(shift)) + float(np.float64(np.float32(f))) * float(np.float64(scale))
    assert T.threshold(shift, scale, f) != float(shift + np.float32(f) * scale)   # not float32 arithmetic


def test_unsigned_samples_and_the_window_limit():
    x = np.full(200, 40_000, np.uint16)
    x[25:42] = 40_200
    assert T.trim(x, 40_100.0, 10, 3, 5, 1000) == 45
    assert T.trim(x.view(np.int16), 40_100.0, 10, 3, 5, 1000) == 5    # the same bits as int16 lie below the threshold
    assert T.windows_ok((1, 3, 10, 10 + 4096, 2.4, 1.0, 0)) and not T.windows_ok((1, 3, 10, 10 + 4097, 2.4, 1.0, 0))
    assert T.windows_ok((40, 3, 10, 8000, 2.4, 1.0, 0)) and T.windows_ok((1, 0, 5000, 100, 2.4, 1.0, 0))


def loop_trim(x, thr, W, m, t0, M, max_fraction, flags):
    """the rule of include/vbz_gpu.h transcribed sample by sample"""
    n = len(x)
    N = min(M, n)
    nW = (N - t0) // W if N > t0 else 0
    seen = False
    for k in range(nW):
        start, e = t0 + k * W, t0 + (k + 1) * W
        count = 0
        for j in range(start, e):
            if float(x[j]) > thr:
                count += 1
        if count > m:
            seen = True
        if not seen:
            continue
        if float(x[e - 1]) > thr:
            continue
        if (flags & 1) and e >= N:
            return min(t0, n)
        if float(e) > float(np.float64(np.float32(max_fraction))) * float(n):
            return min(t0, n)
        return e
    return min(t0, n)


def test_statement_against_the_plain_loop_on_random_reads():
    rng = np.random.default_rng(3)
    moved = 0
    for i in range(200):
        n = int(rng.integers(0, 1500))
        kind = T.KINDS[i % len(T.KINDS)]
        x = T.make_read(rng, n, kind, 400 if i % 2 else 40_000)
        v = x if i % 2 else x.view(np.uint16)
        W = int(rng.choice([1, 3, 7, 40, 64, 300]))
        m = int(rng.integers(0, min(5, W)))   # (m >= W can never open a peak)
        t0 = int(rng.choice([0, 1, 10, 37, 37, 2000]))
        M = int(rng.choice([1, 400, 1000, 8000, 8000, 8000]))
        mf = float(rng.choice([1.0, 1.0, 0.6, 0.05]))
        flags = int(rng.integers(0, 4) == 0)
        norm = R.BONITO if i % 4 else R.DORADO   # (DORADO's q90 often lies inside the plateau: its threshold above it)
        shift, scale = R.shift_scale(v, norm)
        thr = T.threshold(shift, scale, 2.4)
        got = T.trim(v, thr, W, m, t0, M, mf, flags)
        assert got == loop_trim(v, thr, W, m, t0, M, mf, flags), (i, n, kind, W, m, t0, M, mf, flags)
        assert got == T.begin(v, norm, (W, m, t0, M, 2.4, mf, flags))
        moved += got not in (0, min(t0, n))
    assert moved >= 40, moved


def test_begin_takes_the_statistics_of_the_range_or_of_the_read():
    rng = np.random.default_rng(5)
    x = T.make_read(rng, 6000, "front")
    x[:3000] += 150           # half of the read up: the whole read's median sits between the two levels, the tail's on the baseline
    by_read = T.begin(x, R.BONITO, T.DEFAULT, 3000, None, G.STATS_READ)
    by_range = T.begin(x, R.BONITO, T.DEFAULT, 3000, None, G.STATS_RANGE)
    assert by_read == T.begin(x, R.BONITO) and by_range != by_read
    shift, scale, _, _ = G.shift_scale(x, 3000, None, R.BONITO, G.STATS_RANGE)
    assert by_range == T.trim(x, T.threshold(shift, scale, 2.4), *T.DEFAULT[:4], T.DEFAULT[5], T.DEFAULT[6])


def test_pod5_reads_are_their_concatenated_rows():
    rng = np.random.default_rng(6)
    x = T.make_read(rng, 5000, "front")
    y = T.make_read(rng, 900, "middle")
    rows = [x[:7], x[7:7], x[7:2000], x[2000:], y[:450], y[450:]]
    assert T.pod5_begins(rows, [0, 4, 6], R.BONITO) == [T.begin(x, R.BONITO), T.begin(y, R.BONITO), 0]
    assert T.pod5_begins(rows, [0, 4, 6], R.DORADO, T.DEFAULT, [100, 0, 0], [4000, 300, 0]) == [
        T.begin(x, R.DORADO, T.DEFAULT, 100, 4000), T.begin(y, R.DORADO, T.DEFAULT, 0, 300), 0]


def test_the_gpu_tests_generator_is_pinned():
    """the reads the GPU tests use: their sizes, seed and kinds, and that they exercise the rule -- at least half of the reads of 511
    samples and more get a trim of their own, and some fall back to min_trim"""
    assert T.GPU_SIZES == [0, 1, 9, 10, 11, 49, 50, 51, 511, 513, 2047, 2048, 2049, 4101, 7999, 8000, 8001, 8010, 8050, 20_000] and T.GPU_SEED == 7
    reads = T.gpu_reads()
    assert [len(x) for x in reads] == [n for n in T.GPU_SIZES for _ in T.KINDS]
    assert reads[-1].dtype == np.int16 and T.gpu_reads()[-1].tobytes() == reads[-1].tobytes()
    x = reads[T.GPU_SIZES.index(2049) * len(T.KINDS) + 2]    # a read without a plateau: the baseline and its spread
    assert abs(float(np.median(x)) - 400.0) <= 2.0 and 8.0 < float(np.std(x)) < 16.0
    big = [x for x in reads if len(x) >= 511]
    begins = [T.begin(x, R.BONITO) for x in big]
    moved = sum(b not in (0, T.DEFAULT[2]) for b in begins)
    print("reads of 511 samples and more:", len(big), "with a trim of their own:", moved, "at min_trim:", begins.count(T.DEFAULT[2]))
    assert 2 * moved >= len(big), (moved, len(big))
    assert begins.count(T.DEFAULT[2]) >= 1
    wide = T.gpu_reads(level=40_000)
    assert all(int(w.view(np.uint16).min()) > 32_767 for w in wide if len(w))
    moved_wide = sum(T.begin(w.view(np.uint16), R.BONITO) not in (0, T.DEFAULT[2]) for w in wide if len(w) >= 511)
    assert 2 * moved_wide >= len(big), moved_wide

"""The reference of POD5 reads of several rows (tests/pod5_reads_ref.py) held to hand-worked cases and to norm_ref on the concatenation."""
import numpy as np

import norm_ref as R
import pod5_reads_ref as PR


def test_read_signals_concatenate_rows_in_order():
    rows = [np.array([1, 2, 3], np.int16), np.zeros(0, np.int16), np.array([4], np.int16), np.array([5, 6], np.int16)]
    sig = PR.read_signals(rows, [0, 3, 3])
    assert [s.tolist() for s in sig] == [[1, 2, 3, 4], [], [5, 6]]
    assert PR.bounds([0, 3, 3], 4) == [0, 3, 3, 4]


def test_chunk_starts_by_hand():
    assert PR.chunk_starts(0, 8, 8, "pad", 0) == []
    assert PR.chunk_starts(8, 8, 8, "pad", 0) == [0]
    assert PR.chunk_starts(5, 8, 8, "end", 1) == [0]
    assert PR.chunk_starts(20, 8, 8, "pad", 0) == [0, 8, 16]
    assert PR.chunk_starts(20, 8, 8, "end", 1) == [0, 8, 12]
    assert PR.chunk_starts(20, 8, 8, "end", 8) == [0, 8, 16]
    assert PR.chunk_starts(20, 8, 8, "end", 6) == [0, 8, 12]
    assert PR.chunk_starts(2148, 1024, 1000, "end", 6) == [0, 1000, 1128]   # e = ceil(1124 / 6) * 6 = 1128 < 2000


def test_chunk_rows_pad_and_values():
    x = np.arange(1, 21, dtype=np.int16)
    starts, rows = PR.chunk_rows(x, 8, 8, "pad", 0, 1.0, 2.0, -7.0, "f32")
    assert starts == [0, 8, 16] and rows.shape == (3, 8)
    got = rows.view(np.float32)
    assert got[0].tolist() == [4.0, 6.0, 8.0, 10.0, 12.0, 14.0, 16.0, 18.0]
    assert got[2].tolist() == [36.0, 38.0, 40.0, 42.0, -7.0, -7.0, -7.0, -7.0]
    _, end = PR.chunk_rows(x, 8, 8, "end", 1, 0.0, 1.0, -7.0, "f16")
    assert end.view(np.float16)[2].tolist() == [13.0, 14.0, 15.0, 16.0, 17.0, 18.0, 19.0, 20.0]


def test_bf16_bits_round_to_nearest_even():
    # 257 = 0x43808000 lies halfway between two bfloat16 values: the even one (0x4380) wins; 259 = 0x43818000 rounds up to 0x4382
    assert PR.typed_bits(np.array([257, 259], np.int16), 0.0, 1.0, "bf16").tolist() == [0x4380, 0x4382]
    assert PR.pad_bits(-7.0, "f16") == np.float16(-7.0).view(np.uint16)


def test_statistics_are_norm_ref_on_the_concatenation():
    rng = np.random.default_rng(5)
    rows = [rng.integers(-500, 900, n).astype(np.int16) for n in (13, 7, 1, 2047, 2049)]
    x = PR.read_signals(rows, [0])[0]
    assert len(x) == 4117
    for p in (R.BONITO, R.DORADO):
        shift, scale, so, sc = PR.shift_scale(x, p)
        assert (shift, scale) == R.shift_scale(x, p)
        assert so == np.float32(-shift) and sc == np.float32(1.0 / np.float64(scale))
    s, k, _, _ = PR.shift_scale(np.array([-1, 1], np.int16), R.BONITO, signed=False)   # uint16: 65535 and 1 -> median 32768, MAD 32767
    assert (float(s), float(k)) == (32768.0, float(np.float32(R.f64(1.4826) * 32767.0)))   # (scale_mul is a float32 field)
    assert PR.shift_scale(np.zeros(0, np.int16), R.DORADO)[:2] == (np.float32(10.0), np.float32(1.0))

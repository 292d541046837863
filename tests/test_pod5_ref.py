"""CPU tests of tests/pod5_ref.py, the numpy statement of POD5's signal codec (svb16 + zstd) the GPU tests hold the library to: the known
answers of the format, and round trips through libzstd over ragged lengths and the real signal of tests/golden."""
import numpy as np
import pytest

import oracle_lib as O
import pod5_ref as P


def test_known_answers():
    assert P.svb16_encode(np.array([0, 1, -1, 300, 300], np.int16)).tobytes() == bytes.fromhex("08 00 02 03 5a 02 00")
    assert P.svb16_encode(np.array([-32768, 32767], np.int16)).tobytes() == bytes.fromhex("01 ff ff 01")
    assert P.svb16_encode(np.zeros(0, np.int16)).size == 0
    # unused key bits are ignored by the decoder
    s = bytearray(P.svb16_encode(np.array([0, 1, -1, 300, 300], np.int16)))
    s[0] |= 0xE0
    assert P.svb16_decode(np.frombuffer(bytes(s), np.uint8), 5).tolist() == [0, 1, -1, 300, 300]


def test_stream_length_rule():
    x = np.array([5, -200, 7000, 7000, -32768, 3, 2, 1, 0, 9], np.int16)
    s = P.svb16_encode(x)
    assert len(s) == P.key_len(10) + 10 + int((P.zigzag(x) > 0xFF).sum())
    assert P.svb16_decode(s, 10).tolist() == x.tolist()
    assert P.svb16_decode(s[:-1], 10) is None
    assert P.svb16_decode(np.concatenate([s, [0]]).astype(np.uint8), 10) is None
    assert len(s) <= P.svb16_max(10)


@pytest.mark.parametrize("seed", [0, 1])
def test_round_trip_ragged(seed):
    rng = np.random.default_rng(seed)
    lens = [0, 1, 2, 7, 8, 9, 15, 16, 17, 2047, 2048, 2049, 100003] + rng.integers(0, 100004, 12).tolist()
    for n in lens:
        kind = rng.integers(0, 3)
        if kind == 0:
            x = rng.integers(-32768, 32768, n).astype(np.int16)
        elif kind == 1:
            x = O.synth_signal(seed, n, n)
        else:
            x = (np.cumsum(rng.integers(-300, 301, n)) % 65536).astype(np.uint16).view(np.int16)
        s = P.svb16_encode(x)
        assert len(s) <= P.svb16_max(n)
        f = P.compress_row(x)
        assert len(f) <= P.max_compressed_size(n)
        assert O.zstd_content_size(f) == len(s)
        back = P.decompress_row(f, n)
        assert back is not None and back.tobytes() == x.tobytes(), n


def test_round_trip_golden_signal():
    rows, owner = P.golden_rows()
    assert len(rows) > 11 and max(len(r) for r in rows) == P.ROW
    for x in rows:
        f = P.compress_row(x)
        assert P.decompress_row(f, len(x)).tobytes() == x.tobytes()
    # a read's rows, concatenated, are the read
    reads = P.golden_reads()
    for k, x in enumerate(reads):
        assert np.concatenate([r for r, o in zip(rows, owner) if o == k]).tobytes() == x.tobytes()

"""CPU tests: the restated zstd decoder (oracle/zstd_restate.c, the serial mirror of the HIP decoder)
against the pinned dependency itself (libzstd, dlopen'd) on frames libzstd produced."""
import numpy as np
import pytest

import oracle_lib as O


def _gen(rng, kind, n):
    if kind == 0:
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == 1:
        return np.clip(rng.normal(128, 20, n), 0, 255).astype(np.uint8)
    if kind == 2:
        return (rng.integers(0, 100, n) < 4).astype(np.uint8)
    if kind == 3:
        words = [bytes(rng.integers(97, 123, rng.integers(2, 9), dtype=np.uint8)) for _ in range(200)]
        s = b" ".join(words[i] for i in rng.integers(0, 200, n // 4 + 1))
        return np.frombuffer(s[:n].ljust(n, b"x"), np.uint8).copy()
    if kind == 4:
        return np.zeros(n, np.uint8)
    if kind == 5:
        return (np.arange(n) % 251).astype(np.uint8)
    if kind == 6:
        a = rng.integers(0, 256, n, dtype=np.uint8)
        for _ in range(20):
            if n < 200:
                break
            i = int(rng.integers(0, n - 100))
            l = int(rng.integers(4, min(5000, n - i)))
            j = int(rng.integers(0, n - l))
            a[j : j + l] = a[i : i + l].copy()
        return a
    return np.minimum(rng.geometric(0.3, n), 255).astype(np.uint8)


SIZES = [0, 1, 2, 5, 17, 100, 255, 256, 257, 1000, 5000, 20000, 70000, 131072, 131073, 200000, 400000]


def test_restated_decoder_matches_libzstd():
    if O.lib().vbo_zstd_version() is None:
        pytest.skip("no libzstd.so.1 on this box")
    rng = np.random.default_rng(1)
    frames = 0
    for it in range(240):
        n = SIZES[it % len(SIZES)] if it % 3 else int(rng.integers(1, 300000))
        data = _gen(rng, it % 8, n)
        for level in (1, 3, int(rng.integers(-5, 20))):
            frame = O.zstd_compress(data, level)
            out = O.zstd_restate_decompress(frame, n)
            assert out is not None, (it, n, level)
            assert out.tobytes() == data.tobytes(), (it, n, level)
            frames += 1
    assert frames == 720


def test_restated_decoder_on_svb_streams():
    # the frames the VBZ path actually produces: svb streams of synthetic signal, levels 1 and 3
    for r in range(4):
        a = O.synth_signal(5, r, 60000 + 50000 * r)
        svb = O.svb_compress(a, 2, True, 0)
        for level in (1, 3):
            frame = O.zstd_compress(svb, level)
            out = O.zstd_restate_decompress(frame, len(svb))
            assert out is not None and out.tobytes() == svb.tobytes()
    u = O.synth_u32(5, 0, 300000)
    svb = O.svb_compress(u, 4, False, 0)
    frame = O.zstd_compress(svb, 3)
    out = O.zstd_restate_decompress(frame, len(svb))
    assert out is not None and out.tobytes() == svb.tobytes()


def test_restated_decoder_rejects_corruption_without_crashing():
    rng = np.random.default_rng(3)
    a = O.synth_signal(5, 9, 30000)
    svb = O.svb_compress(a, 2, True, 0)
    frame = O.zstd_compress(svb, 1)
    accepted = 0
    for _ in range(300):
        bad = frame.copy()
        for _ in range(int(rng.integers(1, 4))):
            bad[int(rng.integers(0, len(bad)))] ^= 1 << int(rng.integers(0, 8))
        mine = O.zstd_restate_decompress(bad, len(svb))
        ref = O.zstd_decompress(bad, len(svb))
        # The restatement follows RFC 8878 strictly (every Huffman/FSE bitstream must be consumed
        # exactly).  libzstd 1.4.8 is lenient in a few corner cases (double-symbol Huffman decoder's
        # last-symbol clamp, the superfluous final FSE state update), so it may accept a corrupted
        # frame the restatement rejects -- never the other way round, and never with different bytes.
        if mine is not None:
            accepted += 1
            assert ref is not None and ref.tobytes() == mine.tobytes()
    assert accepted < 300
    for cut in (0, 1, 4, 5, 8, 9, 12, len(frame) // 2, len(frame) - 1):
        assert O.zstd_restate_decompress(frame[:cut], len(svb)) is None or cut == 0


def test_weights_alphabet_ends_at_eleven():
    """A Huffman tree description whose FSE-coded weights LIST a symbol beyond 11 -- one no weight ever takes -- can still be a complete
    tree, and a frame built on it can decode consistently (every stream ends on its first bit): tools/soak_corrupt.py found one in
    round 5 (seed 73: one bit of the accuracy log flipped in the frame of a read with four distinct data bytes).  libzstd >= 1.4.7 refuses
    such a description (its workspace is sized for weights 0 .. HUF_TABLELOG_MAX - 1), so the restatement -- and the device decoders,
    which mirror it -- must too: they may be stricter than libzstd, never more lenient.  The fixture holds the frame before and after."""
    import os

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weights_alphabet_beyond_11.npz"))
    good, bad = z["original"], z["damaged"]
    assert np.count_nonzero(good != bad) == 1
    ref = O.zstd_decompress(good, 60000)
    assert ref is not None and len(ref) == 45000
    assert O.zstd_restate_decompress(good, 60000).tobytes() == ref.tobytes()
    assert O.zstd_decompress(bad, 60000) is None                     # libzstd 1.4.8: "Corrupted block detected"
    assert O.zstd_restate_decompress(bad, 60000) is None
    # ... and the hole is closed in general: bit flips in the description never make the restatement accept what libzstd refuses
    rng = np.random.default_rng(5)
    for _ in range(600):
        b = good.copy()
        for _ in range(int(rng.integers(1, 3))):
            b[int(rng.integers(23, 33))] ^= 1 << int(rng.integers(0, 8))
        mine = O.zstd_restate_decompress(b, 60000)
        if mine is not None:
            lz = O.zstd_decompress(b, 60000)
            assert lz is not None and lz.tobytes() == mine.tobytes()


# ---- frames of chosen block layouts (oracle_lib.zstd_compress_cuts: libzstd's streaming compressor, flushed at every cut) ----------------
def _svb(seed, n):
    return O.svb_compress(O.synth_signal(5, seed, n), 2, True, 1)


def test_flushed_frames_end_their_blocks_at_the_cuts():
    """A flush ends a block: the block ends libzstd's bufferless decoder reports are the cuts, the content size, and libzstd's own
    splits every 128 KiB of a stretch between cuts.  The restated decoder reads every such frame as libzstd does."""
    if O.lib().vbo_zstd_version() is None:
        pytest.skip("no libzstd.so.1 on this box")
    rng = np.random.default_rng(17)
    B = O.BLOCK_MAX
    layouts = [[125000], [110000], [B + 118000], [1, 17, 4096], [B, 2 * B], [5000, 5000 + B + 7], [B - 1, B + 1]]
    for it, cuts in enumerate(layouts + [sorted(set(int(x) for x in rng.integers(1, 390000, 3))) for _ in range(6)]):
        s = _svb(100 + it, 260000)
        cuts = [c for c in cuts if c < len(s)]
        for level, checksum in ((1, False), (3, True), (9, False)):
            f = O.zstd_compress_cuts(s, cuts, level=level, checksum=checksum)
            assert O.zstd_content_size(f) == len(s)
            assert O.zstd_frame_geometry(f)[3] == int(checksum)
            want, start = [], 0
            for end in cuts + [len(s)]:
                want += list(range(start + B, end, B)) + [end]
                start = end
            assert O.zstd_block_ends(f, len(s)) == want, (it, level, cuts)
            for dec in (O.zstd_decompress, O.zstd_restate_decompress):
                out = dec(f, len(s))
                assert out is not None and out.tobytes() == s.tobytes(), (it, level, dec.__name__)
    # cuts at k x 128 KiB give the one-shot frame's layout -- and, at level 1, its bytes
    s = _svb(7, 300000)
    one = O.zstd_compress(s, 1)
    f = O.zstd_compress_cuts(s, [B, 2 * B], level=1)
    assert O.zstd_block_ends(f, len(s)) == O.zstd_block_ends(one, len(s)) == [B, 2 * B, len(s)]
    for bad in ([0], [len(s)], [len(s) + 5], [B, B], [2 * B, B]):
        with pytest.raises(ValueError):
            O.zstd_compress_cuts(s, bad)


def test_small_windows_cut_blocks_of_the_window():
    """ZSTD_c_windowLog 10 .. 16: block_max is the window, every block but the last is that long (and the frame has a window descriptor
    that says so); 17 is the 128 KiB of a one-shot frame."""
    if O.lib().vbo_zstd_version() is None:
        pytest.skip("no libzstd.so.1 on this box")
    s = _svb(11, 200000)
    for wlog in (10, 12, 16, 17):
        for level, checksum in ((1, False), (3, True)):
            f = O.zstd_compress_cuts(s, (), level=level, window_log=wlog, checksum=checksum)
            _, fcs, bmax, ck = O.zstd_frame_geometry(f)
            assert (fcs, bmax, ck) == (len(s), min(1 << wlog, O.BLOCK_MAX), int(checksum))
            assert O.zstd_block_ends(f, len(s)) == list(range(bmax, len(s), bmax)) + [len(s)], wlog
            assert O.zstd_restate_decompress(f, len(s)).tobytes() == s.tobytes()
            assert O.zstd_decompress(f, len(s)).tobytes() == s.tobytes()


def test_flushed_layouts_have_overlapping_literal_ranges():
    """The device puts the literals of a non-last block's unit at a guessed block end (oracle_lib.ref_literal_units).  The layouts
    tests/test_gpu_block_layouts.py relies on must really hold units whose ranges overlap -- a short non-last block's wrong guess lands in a
    later unit's range --, else that test would pass without testing what it is for.  One-shot frames never do."""
    if O.lib().vbo_zstd_version() is None:
        pytest.skip("no libzstd.so.1 on this box")
    B = O.BLOCK_MAX
    # (the rows of the issue's table: the int16 svb stream of synth_signal(5, 3, samples), flushed once)
    for samples, n, cuts, pair in ((120000, 151364, [125000], (0, 1)), (120000, 151364, [110000], (0, 1)), (230000, 290131, [B + 118000], (1, 2))):
        s = O.svb_compress(O.synth_signal(5, 3, samples), 2, True, 0)
        assert len(s) == n
        f = O.zstd_compress_cuts(s, cuts)
        u = O.ref_literal_units(f)
        assert pair in O.overlapping_units(u), (n, cuts, u)
        wrong = u[pair[0]]
        assert not wrong["last"] and wrong["guess"] != O.zstd_block_ends(f, n)[wrong["ordinal"]], u
    # the test's own generator: the first block cut 2 .. 30 KiB short, a last block of 15 .. 60 KiB
    import test_gpu_block_layouts as T

    for cuts, _, s in T.short_first_blocks():
        assert O.overlapping_units(O.ref_literal_units(O.zstd_compress_cuts(s, cuts))), cuts
    for cuts, _, s in T.short_middle_blocks():
        assert O.overlapping_units(O.ref_literal_units(O.zstd_compress_cuts(s, cuts))), cuts
    for r in range(6):
        s = _svb(300 + r, 100000 + 60000 * r)
        assert not O.overlapping_units(O.ref_literal_units(O.zstd_compress(s, 1)))
        assert not O.overlapping_units(O.ref_literal_units(O.zstd_compress_cuts(s, [], window_log=16)))

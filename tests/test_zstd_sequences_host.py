"""oracle_lib.zstd_sequences (oracle/zstd_restate.c, vbo_zstd_restate_sequences): the restated decoder's listing of a frame's blocks and
sequences, held to the census of the same decoder and to the content itself over the 140 libzstd frames of tests/zstd_feature_corpus.py.

The listing is what tests/test_gpu_encoder_sequences.py compares the device encoder's frames with, so it is pinned here from two sides
that do not share its code: the census counts the same events with counters of its own, and the replay needs nothing but the decoded
content -- a sequence (position p, literal length ll, match length ml, offset off) says that content[p + ll : p + ll + ml] repeats what
stands off bytes in front of it, byte by byte (so also where off < ml: in the finished content "copied byte-serially" and "equal to the byte
off in front" are the same statement), and the sequences and tail literals of a block tile its range."""
import numpy as np

import oracle_lib as O
import zstd_feature_corpus as C


def per_block(blocks, seqs):
    """[(block, its sequences)]: the listing's sequences are in block order, nseq of them per block"""
    out, at = [], 0
    for b in blocks:
        out.append((b, seqs[at : at + int(b["nseq"])]))
        at += int(b["nseq"])
    assert at == len(seqs)
    return out


def test_counts_and_byte_sums_equal_the_census():
    frames = C.frames()
    assert len(frames) == 140
    for name, content, frame, _ in frames:
        cen = O.zstd_census(frame)
        blocks, seqs = O.zstd_sequences(frame)
        offs = ["off_new", "off_rep0", "off_rep1", "off_rep2", "off_ll0_rep1", "off_ll0_rep2", "off_ll0_rep0_minus_1"]
        assert len(seqs) == sum(cen[k] for k in offs) == int(blocks["nseq"].sum()), name
        assert int(seqs["ml"].sum()) == cen["match_bytes"], name
        assert int(blocks["literals"].sum()) == cen["literal_bytes"], name
        assert cen["match_bytes"] + cen["literal_bytes"] == len(content) == cen["content_size"], name
        assert int((seqs["ll_code"] == 35).sum()) == cen["ll_code_35"] and int((seqs["ml_code"] == 52).sum()) == cen["ml_code_52"], name
        # the kinds of offset, one by one, from the raw offset value and the literal length
        rep, ll0 = (seqs["ofv"] <= 3), (seqs["ll"] == 0)
        assert int((~rep).sum()) == cen["off_new"] and int((seqs["offset"][~rep] + 3 != seqs["ofv"][~rep]).sum()) == 0, name
        for v, a, b in ((1, "off_rep0", "off_ll0_rep1"), (2, "off_rep1", "off_ll0_rep2"), (3, "off_rep2", "off_ll0_rep0_minus_1")):
            assert int((rep & ~ll0 & (seqs["ofv"] == v)).sum()) == cen[a] and int((rep & ll0 & (seqs["ofv"] == v)).sum()) == cen[b], (name, v)
        assert len(blocks) == cen["block_raw"] + cen["block_rle"] + cen["block_compressed"], name
        for t, k in enumerate(("block_raw", "block_rle", "block_compressed")):
            assert int((blocks["type"] == t).sum()) == cen[k], (name, k)
        assert int(seqs["ll_code"].max(initial=0)) == cen["max_ll_code"] and int(seqs["ml_code"].max(initial=0)) == cen["max_ml_code"], name
        assert int(seqs["of_code"].max(initial=0)) == cen["max_of_code"], name


def test_replay_against_the_content_and_tiling():
    total = 0
    for name, content, frame, _ in C.frames():
        c = np.ascontiguousarray(content).view(np.uint8).reshape(-1)
        blocks, seqs = O.zstd_sequences(frame)
        pos = 0
        for k, (b, sq) in enumerate(per_block(blocks, seqs)):
            assert int(b["ordinal"]) == k and int(b["begin"]) == pos, (name, k)
            assert (sq["block"] == k).all(), (name, k)
            for s in sq:
                p, ll, ml, off = int(s["pos"]), int(s["ll"]), int(s["ml"]), int(s["offset"])
                assert p == pos, (name, k, p, pos)
                m = p + ll
                assert 1 <= off <= m and m + ml <= len(c), (name, k, p, ll, ml, off)
                assert np.array_equal(c[m : m + ml], c[m - off : m + ml - off]), (name, k, p, ll, ml, off)
                pos = m + ml
            tail = int(b["literals"]) - int(sq["ll"].sum())
            assert tail >= 0, (name, k)
            pos += tail
            assert int(b["end"]) == pos and pos - int(b["begin"]) <= O.BLOCK_MAX, (name, k, pos)
            total += len(sq)
        assert pos == len(c), name
    assert total > 100000   # (the corpus is not a handful of sequences)


def test_states_and_unread_bits_are_those_of_a_decoder():
    """The head-of-loop state of every sequence: states inside their tables (at most 9 bits), unread bits that fall strictly inside a block
    -- each sequence reads at least its state updates or extra bits unless all three tables are RLE -- and start again in the next."""
    for name, _, frame, _ in C.frames()[:40]:
        blocks, seqs = O.zstd_sequences(frame)
        for b, sq in per_block(blocks, seqs):
            if len(sq) == 0:
                continue
            assert (sq["unread"] >= 0).all() and (np.diff(sq["unread"]) <= 0).all(), name
            assert int(sq["ll_state"].max()) < 512 and int(sq["ml_state"].max()) < 512, name
            assert int(sq["unread"][0]) < 8 * O.BLOCK_MAX, name


def test_a_refused_buffer_returns_the_error():
    name, content, frame, _ = C.frames()[0]
    assert O.zstd_sequences(frame) is not None
    assert O.zstd_sequences(frame[: len(frame) - 1]) is None
    assert O.zstd_sequences(frame[: len(frame) // 2]) is None
    assert O.zstd_sequences(np.frombuffer(b"\x00\x01\x02\x03\x04\x05", np.uint8)) is None
    bad = frame.copy()
    bad[0] ^= 0xFF   # not a frame's magic
    assert O.zstd_sequences(bad) is None
    # what the decoder refuses, the listing refuses: the same verdict on damaged frames
    rng = np.random.default_rng(7)
    for _ in range(200):
        g = frame.copy()
        g[int(rng.integers(4, len(g)))] ^= 1 << int(rng.integers(0, 8))
        assert (O.zstd_sequences(g) is None) == (O.zstd_census(g) is None)


def test_skippable_frames_and_second_frames_are_listed_in_content_order():
    name, content, frame, _ = C.frames()[1]
    skip = np.frombuffer(b"\x5b\x2a\x4d\x18\x04\x00\x00\x00abcd", np.uint8)
    b1, s1 = O.zstd_sequences(frame)
    b2, s2 = O.zstd_sequences(np.concatenate([frame, skip, frame]))
    assert len(b2) == 2 * len(b1) and len(s2) == 2 * len(s1)
    assert np.array_equal(b2[: len(b1)], b1) and np.array_equal(s2[: len(s1)], s1)
    assert np.array_equal(b2["begin"][len(b1) :], b1["begin"] + len(content)) and np.array_equal(s2["pos"][len(s1) :], s1["pos"] + len(content))
    assert np.array_equal(b2["ordinal"][len(b1) :], b1["ordinal"])

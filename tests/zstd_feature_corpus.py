"""libzstd frames chosen by what they contain, shared by tests/test_zstd_feature_corpus_host.py (the census of every frame, the
classification of every counter) and tests/test_gpu_zstd_features.py (every frame on every device decode path).

DESIGN.md 2 T3 promises that the device decodes every frame libzstd writes.  A decoder rule that no test frame reaches is untested however
many frames there are, so this corpus is stated per RFC 8878 feature: oracle_lib.zstd_census (oracle/zstd_restate.c, the counters of
oracle/vbz_oracle.h's VBO_CENSUS) says what a frame holds, and every counter is in exactly one of three lists below:

  REQUIRED       at least two corpus frames reach it; at least one of them has at most four blocks (REF_MAXBLK: the chain walk takes no
                 more) unless the counter is in MANY_BLOCKS_ONLY, and that one is an int16 svb stream unless it is in PLAIN_ONLY (so that
                 the frame also goes through vbz_gpu_decompress_batch)
  UNREACHED      no setting tried made libzstd 1.4.8 write it; each entry says what was tried.  Asserted to be 0 over the corpus, so the
                 list cannot go stale
  INFORMATIONAL  maxima and sums that are not features

No frame is hand-built: every one is libzstd's own (oracle_lib.zstd_compress_params: ZSTD_CCtx_setParameter, flushes, streamed frames),
the work is to steer it.  frames() is deterministic (fixed seeds) and cached; contents are at most 256 KiB but for three frames of at most
2 MiB whose content lies behind windows of 1 MiB and more.  Build time of frames(): 2.1 s on the development machine (one core; 140 frames,
19.6 MB of content; the level 19 and 22 frames are most of it)."""
import functools

import numpy as np

import oracle_lib as O

LEVEL, WLOG, MINMATCH, STRATEGY = O.ZSTD_c_compressionLevel, O.ZSTD_c_windowLog, O.ZSTD_c_minMatch, O.ZSTD_c_strategy
LDM, FCS, CKSUM = O.ZSTD_c_enableLongDistanceMatching, O.ZSTD_c_contentSizeFlag, O.ZSTD_c_checksumFlag

MAX_CONTENT, MAX_FAR, MAX_FAR_FRAMES, MAX_FRAMES = 256 << 10, 2 << 20, 3, 160


def read(index, svb_bytes):
    """an int16 read whose svb stream (zig-zag, version 1) is about svb_bytes long, and that stream"""
    a = O.synth_signal(5, index, max(1, int(svb_bytes / 1.262)))
    return a, O.svb_compress(a, 2, True, 1)


def _pieces(rng, back, count, length, tail):
    """64 KiB of random bytes P, then `count` pieces P[r : r + length], each followed by one byte from tail()"""
    parts = [back]
    for _ in range(count):
        r = int(rng.integers(0, len(back) - length - 500))
        parts += [back[r : r + length], np.array([tail()], np.uint8)]
    return np.concatenate(parts)


def _zero_runs(rng, n, p_burst):
    a = np.zeros(n, np.uint8)
    for s0 in np.nonzero(rng.random(n) < p_burst)[0]:
        ln = min(int(rng.integers(1, 12)), n - int(s0))
        a[int(s0) : int(s0) + ln] = rng.integers(1, 86, ln, dtype=np.uint8)
    return a


@functools.lru_cache(maxsize=None)
def frames():
    """[(name, content (uint8), frame (uint8), params), ...]; a frame whose content is the svb stream of an int16 read has that read in
    reads()[name]"""
    return _build()[0]


def reads():
    """{name: int16 read} of the frames whose content is an svb stream (zig-zag, version 1, integer size 2)"""
    return _build()[1]


@functools.lru_cache(maxsize=None)
def _build():
    out, rd = [], {}

    def add(name, content, params, cuts=(), pledge=True, read_=None):
        c = np.ascontiguousarray(content).view(np.uint8).reshape(-1)
        assert name not in {f[0] for f in out}, name
        out.append((name, c, O.zstd_compress_params(c, params, cuts, pledge), dict(params, cuts=tuple(cuts), pledge=pledge)))
        if read_ is not None:
            rd[name] = read_

    rng = np.random.default_rng(8878)
    back = rng.integers(0, 256, 65536, dtype=np.uint8)
    # -- the recipes: matches of 20 bytes into a flushed block of random bytes with ONE literal value between them (RLE literals at levels
    #    9 and 19, RLE_Mode match lengths at 19, compressed literals at 1 and 3); 40 bytes and three skewed values (one stream)
    c = _pieces(rng, back, 3000, 20, lambda: 97)
    for lv in (1, 3, 9, 19):
        add("pieces20_L%d" % lv, c, {LEVEL: lv}, [65536])
    c = _pieces(rng, back, 200, 40, lambda: int(rng.choice([97, 98, 99], p=[.8, .15, .05])))
    for lv in (1, 3, 9, 19):
        add("pieces40_L%d" % lv, c, {LEVEL: lv}, [65536])
    c = _pieces(rng, back, 5000, 20, lambda: 97)                      # more than 4 095 literals: the three-byte header
    for lv in (9, 16, 19, 22):
        add("pieces20x5000_L%d" % lv, c, {LEVEL: lv}, [65536])
    # -- matches of three bytes with nothing between them: more than 0x7F00 sequences in a block (minMatch 3: the optimal parsers only)
    for A, p in ((256, {LEVEL: 19, MINMATCH: 3}), (1024, {LEVEL: 22, MINMATCH: 3, STRATEGY: 9})):
        alpha = rng.integers(0, 256, A, dtype=np.uint8)
        at = rng.integers(0, A - 3, 44000)
        add("pieces3_of_%d_L%d" % (A, p[LEVEL]), np.concatenate([alpha, alpha[at[:, None] + np.arange(3)].reshape(-1)]), p)
    # -- int16 svb streams: one, two and three blocks, every level class (fast negative levels; 1: fast; 3: dfast; 9: lazy2; 19, 22: optimal)
    for k, nbytes in enumerate((40 << 10, 150 << 10, 255 << 10)):
        a, s = read(2000 + k, nbytes)
        for lv in (-5, -1, 1, 3, 9, 19, 22):
            if lv == 22 and k != 1:
                continue
            add("svb%dk_L%d" % (nbytes >> 10, lv), s, {LEVEL: lv, CKSUM: int(lv in (3, 19))}, read_=a)
    # -- svb streams under small windows: many small blocks, treeless literals and repeated tables at small size; up to four blocks, and more
    for k, (w, nbytes) in enumerate(((10, 3800), (10, 30000), (11, 7800), (11, 40000), (12, 15000), (12, 60000))):
        a, s = read(2100 + k, nbytes)
        for lv in (1, 3, 19):
            add("svb_w%d_%dk_L%d" % (w, nbytes // 1000, lv), s, {LEVEL: lv, WLOG: w}, read_=a)
    # -- a window of 128 KiB below a larger content: a window descriptor beside the content size, blocks of the full size
    a, s = read(2140, 255 << 10)
    add("svb_w17_L1", s, {LEVEL: 1, WLOG: 17}, read_=a)
    add("svb_w17_L3", s, {LEVEL: 3, WLOG: 17, CKSUM: 1}, read_=a)
    # -- the smallest svb streams (a content size in one byte; fewer than 256 literals: one stream), a flat read (RLE blocks), a read that
    #    repeats a unit of 1 000 samples (a match longer than 64 KiB)
    for k, (samples, lv) in enumerate(((150, 1), (150, 19), (300, 3), (2400, -5), (2400, 3))):
        a = O.synth_signal(5, 2150 + k, samples)
        add("svb_%d_samples_L%d" % (samples, lv), O.svb_compress(a, 2, True, 1), {LEVEL: lv}, read_=a)
    for lv in (1, 19):
        a = np.full(60000, -1234, np.int16)
        add("svb_flat_L%d" % lv, O.svb_compress(a, 2, True, 1), {LEVEL: lv}, read_=a)
        a = np.zeros(120000, np.int16)                                   # (a stream of zeros: two RLE blocks)
        add("svb_zero_L%d" % lv, O.svb_compress(a, 2, True, 1), {LEVEL: lv}, read_=a)
        a = np.tile(O.synth_signal(5, 2160, 1000), 150)
        add("svb_periodic_L%d" % lv, O.svb_compress(a, 2, True, 1), {LEVEL: lv, CKSUM: 1}, read_=a)
    # -- a tree, a block without one, a treeless block: three blocks
    a, s = read(2170, 60 << 10)
    for lv in (1, 3, 9):
        add("svb_tiny_middle_L%d" % lv, s, {LEVEL: lv}, [len(s) - 3040, len(s) - 3000], read_=a)
    # -- reads that move in small steps: few literal values.  Fewer than 256 literals: one stream; a second block of 256 .. 1 023 under the
    #    first block's tree at the fast levels: treeless in four streams
    for k, (samples, lv) in enumerate(((200, 1), (200, 3), (1400, 1), (1400, 3), (1400, 19))):
        a = np.cumsum(np.random.default_rng(2180 + k).integers(-3, 4, samples)).astype(np.int16)
        s = O.svb_compress(a, 2, True, 1)
        add("svb_steps%d_L%d" % (samples, lv), s, {LEVEL: lv}, [len(s) - 700] if samples > 1000 else [], read_=a)
    # -- the recipes again as int16 reads, stated in the reads' DELTAS (one byte each in the stream's data section, behind control bytes
    #    that are all zero): 64 Ki random deltas, a flush, 3 000 pieces of 20 of them with the delta 1 between (RLE literals); 256 deltas,
    #    a flush behind the control bytes, 44 000 pieces of three (a sequence count in three bytes)
    def from_deltas(d):
        x = np.cumsum(d.astype(np.int64))
        assert np.abs(x).max() < 32768
        a = x.astype(np.int16)
        s = O.svb_compress(a, 2, True, 1)
        assert len(s) == (len(a) + 3) // 4 + len(a)   # (every delta in one byte)
        return a, s
    base = rng.integers(-40, 41, 65536)
    for count, levels in ((3000, (9, 19)), (5000, (16, 19))):        # (5 000: more than 4 095 literals again)
        at = rng.integers(0, 65000, count)
        d = np.concatenate([base, np.concatenate([base[at[:, None] + np.arange(20)], np.ones((count, 1), np.int64)], axis=1).reshape(-1)])
        a, s = from_deltas(d)
        for lv in levels:
            add("svb_pieces20x%d_L%d" % (count, lv), s, {LEVEL: lv}, [(len(a) + 3) // 4 + 65536], read_=a)
    base = rng.permutation(np.concatenate([np.arange(-16, 0), np.arange(1, 17)] * 8))   # (mean 0: the read does not drift away)
    at = rng.integers(0, 253, 44000)
    a, s = from_deltas(np.concatenate([base, base[at[:, None] + np.arange(3)].reshape(-1)]))
    for p in ({LEVEL: 19, MINMATCH: 3}, {LEVEL: 22, MINMATCH: 3, STRATEGY: 9}):
        add("svb_pieces3_L%d" % p[LEVEL], s, p, [(len(a) + 3) // 4], read_=a)
    # -- flush cuts: short blocks, a streamed frame (no content size), an empty last block
    a, s = read(2200, 200 << 10)
    add("svb_cuts_L1", s, {LEVEL: 1}, [1, 4097, 100000], read_=a)
    add("svb_cuts_L19", s, {LEVEL: 19, CKSUM: 1}, [50000, 50100, 180000], read_=a)
    add("svb_streamed_L3", s, {LEVEL: 3}, [90000], pledge=False, read_=a)
    add("svb_nosize_L1", s, {LEVEL: 1, FCS: 0}, read_=a)
    add("svb_empty_last_L1", s, {LEVEL: 1}, [len(s)], read_=a)
    a, s = read(2201, 30 << 10)
    add("svb_small_empty_last_L3", s, {LEVEL: 3, CKSUM: 1}, [len(s)], read_=a)
    add("svb_small_streamed_L1", s, {LEVEL: 1}, pledge=False, read_=a)
    # -- a read that repeats: the svb stream's data bytes come again 70 KiB and 150 KiB back (offsets above 64 KiB, above 128 KiB, matches
    #    from before the block)
    for k, (samples, lv) in enumerate(((62000, 3), (62000, 19), (110000, 9), (110000, 19))):
        a = O.synth_signal(5, 2300 + k, samples)
        a = np.concatenate([a, a])[: 125000 if samples > 100000 else None]
        add("svb_repeat%dk_L%d" % (samples // 1000, lv), O.svb_compress(a, 2, True, 1), {LEVEL: lv}, read_=a)
    # -- far offsets: a content that repeats more than 1 MiB back; long-distance matching, a large window at level 19
    far = np.concatenate([rng.integers(0, 256, 1100 << 10, dtype=np.uint8), np.zeros(4096, np.uint8)])
    far = np.concatenate([far, far[: 300 << 10], far[5000 : 200 << 10]])
    add("far_ldm_L3", far, {LEVEL: 3, LDM: 1, WLOG: 22})
    add("far_L19", far[: (1100 << 10) + 4096 + (120 << 10)], {LEVEL: 19, WLOG: 22})
    add("far_L3_w20", far, {LEVEL: 3, WLOG: 20, CKSUM: 1})   # (a window of 1 MiB below the content: a descriptor, and no match that far)
    # -- text
    text = np.frombuffer((b"the quick brown fox jumps over the lazy dog %d, " * 4000) % tuple((i * 7919) % 10007 for i in range(4000)), np.uint8)[:180000]
    for lv in (1, 3, 9, 19, 22):
        add("text_L%d" % lv, text, {LEVEL: lv})
    add("text_w12_L19", text[:60000], {LEVEL: 19, WLOG: 12})
    add("text_cuts_L22", text, {LEVEL: 22}, [777, 60000, 60003])
    words = rng.integers(0, 256, (300, 9), dtype=np.uint8)
    prose = words[np.minimum(rng.geometric(0.02, 30000), 299)].reshape(-1)[:200000]
    for lv in (3, 19, 22):
        add("prose_L%d" % lv, prose, {LEVEL: lv})
    # -- zero runs between short bursts (repeat offset 1 with literal length 0, overlapping matches), and runs longer than 64 KiB
    for k, (n, p) in enumerate(((30000, 0.01), (120000, 0.004), (250000, 0.02))):
        z = _zero_runs(rng, n, p)
        for lv in (1, 9, 19):
            add("zero_runs%d_L%d" % (k, lv), z, {LEVEL: lv})
    z = np.concatenate([rng.integers(0, 256, 900, dtype=np.uint8), np.zeros(100000, np.uint8), rng.integers(0, 256, 90, dtype=np.uint8), np.full(70000, 7, np.uint8)])
    for lv in (1, 19):
        add("long_runs_L%d" % lv, z, {LEVEL: lv})
    unit = rng.integers(0, 256, 3000, dtype=np.uint8)
    tiled = np.concatenate([rng.integers(0, 256, 500, dtype=np.uint8), np.tile(unit, 70)])
    for lv in (1, 19):
        add("tiled3000_L%d" % lv, tiled, {LEVEL: lv})
    # -- literals more than 64 KiB long ahead of a match (literal length code 35)
    lit = np.concatenate([rng.integers(0, 256, 100000, dtype=np.uint8), back[:3000], np.minimum(rng.geometric(0.2, 70000), 255).astype(np.uint8), back[100:900]])
    for lv in (1, 3, 19):
        add("long_literals_L%d" % lv, lit, {LEVEL: lv})
    # -- geometric bytes: literals alone, long Huffman codes; few values: direct weights, short codes
    for k, (p, n) in enumerate(((0.3, 150000), (0.05, 100000), (0.6, 9000))):
        g = np.minimum(rng.geometric(p, n), 255).astype(np.uint8)
        for lv in (1, 19):
            add("geometric%d_L%d" % (k, lv), g, {LEVEL: lv, CKSUM: k == 1})
    skew = rng.choice(256, 200000, p=(lambda w: w / w.sum())(1.0 / np.arange(1, 257) ** 1.6)).astype(np.uint8)
    add("zipf_L1", skew, {LEVEL: 1})
    add("zipf_w12_L3", skew[:50000], {LEVEL: 3, WLOG: 12})
    add("four_values_L1", rng.choice([3, 4, 5, 250], 20000, p=[.6, .2, .1, .1]).astype(np.uint8), {LEVEL: 1})
    # -- raw and RLE blocks, the smallest contents, every content-size field libzstd can be brought to write
    add("random70k_L1", rng.integers(0, 256, 70000, dtype=np.uint8), {LEVEL: 1})
    add("random300_L3", rng.integers(0, 256, 300, dtype=np.uint8), {LEVEL: 3, CKSUM: 1})
    add("zeros250k_L1", np.zeros(250000, np.uint8), {LEVEL: 1})
    add("zeros250k_L19", np.zeros(250000, np.uint8), {LEVEL: 19, CKSUM: 1})
    add("sevens1000_L3", np.full(1000, 7, np.uint8), {LEVEL: 3})
    for n in (0, 1):
        add("bytes%d_L1" % n, np.full(n, 65, np.uint8), {LEVEL: 1})
        add("bytes%d_streamed_L3" % n, np.full(n, 65, np.uint8), {LEVEL: 3, CKSUM: 1}, pledge=False)
    add("bytes0_nosize_L1", np.zeros(0, np.uint8), {LEVEL: 1, FCS: 0})
    add("text200_L3", text[:200], {LEVEL: 3})
    add("text200_L19", text[:200], {LEVEL: 19, CKSUM: 1})
    add("text3000_L1", text[:3000], {LEVEL: 1})
    assert len(out) <= MAX_FRAMES, len(out)
    return out, rd


# ---- the classification: every counter of the census in exactly one list ------------------------------------------------------------------
REQUIRED = [
    "frame_single_segment", "frame_window_descriptor", "frame_content_size_0_bytes", "frame_content_size_1_byte",
    "frame_content_size_2_bytes", "frame_content_size_4_bytes", "frame_checksum", "frame_window_log_up_to_16",
    "frame_window_log_17_to_19", "frame_window_log_from_20", "block_raw", "block_rle", "block_compressed", "block_last",
    "block_not_last", "block_raw_empty", "lit_raw_header_1_byte", "lit_raw_header_2_bytes", "lit_raw_header_3_bytes",
    "lit_rle_header_2_bytes", "lit_rle_header_3_bytes", "lit_compressed_format_0", "lit_compressed_format_1",
    "lit_compressed_format_2", "lit_compressed_format_3", "lit_treeless_format_0", "lit_treeless_format_1", "lit_treeless_format_2",
    "lit_treeless_format_3", "lit_streams_1", "lit_streams_4", "lit_treeless_tree_of_previous_block",
    "lit_treeless_tree_of_earlier_block", "huf_description_direct", "huf_description_fse", "huf_weights_log_5", "huf_trees_11_bits",
    "huf_trees_up_to_6_bits", "huf_symbols_up_to_16", "huf_symbols_above_128", "seq_none", "seq_count_1_byte", "seq_count_2_bytes",
    "seq_count_3_bytes", "seq_ll_predefined", "seq_ll_rle", "seq_ll_fse", "seq_ll_repeat", "seq_of_predefined", "seq_of_rle",
    "seq_of_fse", "seq_of_repeat", "seq_ml_predefined", "seq_ml_rle", "seq_ml_fse", "seq_ml_repeat", "seq_ll_log_5", "seq_of_log_5",
    "seq_ml_log_5", "seq_ll_log_9", "seq_of_log_8", "seq_ml_log_9", "seq_ll_less_than_1", "seq_of_less_than_1",
    "seq_ml_less_than_1", "off_new", "off_rep0", "off_rep1", "off_rep2", "off_ll0_rep1", "off_ll0_rep2", "off_ll0_rep0_minus_1",
    "seq_literal_length_0", "ll_code_35", "ml_code_52", "match_overlaps_itself", "match_offset_1", "match_from_before_the_block",
    "off_above_64k", "off_above_128k", "off_above_1m", "tail_literals_none", "tail_literals_some",
]

# counter: what was tried (libzstd 1.4.8)
UNREACHED = {
    "frame_content_size_8_bytes": "libzstd writes the eight-byte field for contents of 4 GiB and more only; a frame may not be hand-edited here",
    "lit_rle_header_1_byte": "RLE literals of at most 31 bytes: pieces of 20 bytes with one literal value between them, 25 of them in a block "
                             "behind a block with a Huffman tree, levels 9 and 19 -- libzstd leaves literals of up to 63 bytes raw unless a "
                             "DICTIONARY's tree is valid (ZSTD_compressLiterals: minLitSize), and dictionaries are outside this library",
    "huf_weights_log_6": "every tree of the corpus (2 .. 256 symbols, levels -5 .. 22) has weights of accuracy log 5: FSE_optimalTableLog caps "
                         "the log at highbit(weights - 1) - 2, which is 5 for the at most 255 weights of a tree description",
}

# maxima and sums that are not features
INFORMATIONAL = [
    "frames", "huf_max_bits", "huf_symbols_max", "seq_ll_log_max", "seq_of_log_max", "seq_ml_log_max", "max_ll_code", "max_of_code",
    "max_ml_code", "literal_bytes", "match_bytes",
]

# REQUIRED counters that no frame of at most four blocks can reach, with the reason
MANY_BLOCKS_ONLY = {
    "off_above_1m": "a match more than 1 MiB back lies behind at least eight blocks of 128 KiB",
}

# REQUIRED counters whose frames of at most four blocks are not int16 svb streams, with the reason (none now: the pieces recipes are
# restated in the deltas of a read)
PLAIN_ONLY = {}

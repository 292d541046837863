"""The feature corpus of libzstd frames (tests/zstd_feature_corpus.py) on the CPU: every frame decodes to its content, the census of the
restated decoder (oracle/zstd_restate.c: vbo_zstd_restate_census) adds up and agrees with an independent walk over the headers, and
every counter of the census is classified: REQUIRED ones are reached as the corpus module's docstring says, UNREACHED ones are 0.

The GPU half is tests/test_gpu_zstd_features.py."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import oracle_lib as O
import zstd_feature_corpus as Z

pytestmark = pytest.mark.skipif(O.lib().vbo_zstd_version() is None, reason="no libzstd on this box")


@functools.lru_cache(maxsize=None)
def _census():
    """{name: census} of every corpus frame, computed once"""
    return {name: O.zstd_census(f) for name, _, f, _ in Z.frames()}


def _nblocks(cen):
    return cen["block_raw"] + cen["block_rle"] + cen["block_compressed"]


def _header_walk(frame):
    """The header-level counters of one frame by a walk of its own over the frame, block, literals and sequences headers (RFC 8878
    3.1.1.1, 3.1.1.2, 3.1.1.3.1.1, 3.1.1.3.2.1): no code shared with the C census, nothing decoded."""
    f, c = bytes(frame), {}

    def hit(k):
        c[k] = c.get(k, 0) + 1

    assert f[:4] == b"\x28\xb5\x2f\xfd"
    fhd, pos = f[4], 5
    single = fhd >> 5 & 1
    hit("frame_single_segment" if single else "frame_window_descriptor")
    if not single:
        wlog = 10 + (f[pos] >> 3)
        hit("frame_window_log_up_to_16" if wlog <= 16 else "frame_window_log_17_to_19" if wlog < 20 else "frame_window_log_from_20")
        pos += 1
    pos += (0, 1, 2, 4)[fhd & 3]
    fcs = (1 if single else 0, 2, 4, 8)[fhd >> 6]
    hit("frame_content_size_%d_byte%s" % (fcs, "" if fcs == 1 else "s"))
    pos += fcs
    if fhd & 4:
        hit("frame_checksum")
    while True:
        bh = int.from_bytes(f[pos : pos + 3], "little")
        last, btype, bsize = bh & 1, bh >> 1 & 3, bh >> 3
        pos += 3
        hit(("block_raw", "block_rle", "block_compressed")[btype])
        hit("block_last" if last else "block_not_last")
        if btype == 0 and bsize == 0:
            hit("block_raw_empty")
        if btype == 2:
            b = f[pos : pos + bsize]
            ltype, fmt = b[0] & 3, b[0] >> 2 & 3
            if ltype < 2:
                hlen = (1, 2, 1, 3)[fmt]
                regen = int.from_bytes(b[:hlen], "little") >> (3 if hlen == 1 else 4)
                hit("lit_%s_header_%d_byte%s" % (("raw", "rle")[ltype], hlen, "" if hlen == 1 else "s"))
                at = hlen + (regen if ltype == 0 else 1)
            else:
                hlen, bits = ((3, 10), (3, 10), (4, 14), (5, 18))[fmt]
                csize = int.from_bytes(b[:hlen], "little") >> (4 + bits)
                hit("lit_%s_format_%d" % (("compressed", "treeless")[ltype - 2], fmt))
                hit("lit_streams_1" if fmt == 0 else "lit_streams_4")
                if ltype == 2:
                    hit("huf_description_direct" if b[hlen] >= 128 else "huf_description_fse")
                at = hlen + csize
            n0 = b[at]
            hit("seq_none" if n0 == 0 else "seq_count_1_byte" if n0 < 128 else "seq_count_2_bytes" if n0 < 255 else "seq_count_3_bytes")
            if n0:
                modes = b[at + (1 if n0 < 128 else 2 if n0 < 255 else 3)]
                for table, shift in (("ll", 6), ("of", 4), ("ml", 2)):
                    hit("seq_%s_%s" % (table, ("predefined", "rle", "fse", "repeat")[modes >> shift & 3]))
        pos += 1 if btype == 1 else bsize
        if last:
            break
    assert pos + (4 if fhd & 4 else 0) == len(f)
    return c


WALKED_PREFIXES = ("frame_", "block_", "lit_raw", "lit_rle", "lit_compressed", "lit_streams", "lit_treeless_format", "huf_description",
                   "seq_none", "seq_count", "seq_ll_p", "seq_ll_r", "seq_ll_f", "seq_of_p", "seq_of_r", "seq_of_f", "seq_ml_p", "seq_ml_r",
                   "seq_ml_f")


def test_corpus_stays_inside_its_sizes():
    F = Z.frames()
    assert len(F) <= Z.MAX_FRAMES and len({name for name, *_ in F}) == len(F)
    far = [name for name, c, _, _ in F if len(c) > Z.MAX_CONTENT]
    assert len(far) <= Z.MAX_FAR_FRAMES and all(len(c) <= Z.MAX_FAR for _, c, _, _ in F), far
    assert sum(len(c) for _, c, _, _ in F) < 20 << 20
    R = Z.reads()
    for name, c, _, _ in F:
        if name in R:
            assert R[name].dtype == np.int16 and O.svb_compress(R[name], 2, True, 1).tobytes() == c.tobytes(), name


def test_every_frame_decodes_to_its_content():
    for name, c, f, _ in Z.frames():
        want = c.tobytes()
        for what, dec in (("libzstd", O.zstd_decompress), ("restated", O.zstd_restate_decompress)):
            got = dec(f, len(c))
            assert got is not None and got.tobytes() == want, (name, what)
            if len(c):
                assert dec(f, len(c) - 1) is None, (name, what, "a destination one byte short")


def test_census_adds_up():
    """literal bytes + match bytes = the content size, the block counters = the blocks libzstd's bufferless decoder steps through (and
    the empty ones, which it has no step for), and every per-block counter family sums to its blocks"""
    for name, c, f, _ in Z.frames():
        cen = _census()[name]
        assert cen is not None, name
        assert cen["content_size"] == len(c) and cen["literal_bytes"] + cen["match_bytes"] == len(c), name
        ends = O.zstd_block_ends(f, len(c))
        # (a block of no bytes has nothing for the bufferless decoder to be handed: it steps from its header to the next)
        assert ends is not None and _nblocks(cen) == len(ends) + cen["block_raw_empty"] == cen["block_last"] + cen["block_not_last"], name
        assert (ends[-1] if ends else 0) == len(c), name
        assert cen["frames"] == 1 and cen["block_last"] == 1, name
        lits = sum(v for k, v in cen.items() if k.startswith(("lit_raw", "lit_rle", "lit_compressed", "lit_treeless_format")))
        seqs = cen["seq_none"] + cen["seq_count_1_byte"] + cen["seq_count_2_bytes"] + cen["seq_count_3_bytes"]
        assert lits == seqs == cen["block_compressed"], name
        with_seq = seqs - cen["seq_none"]
        for t in ("ll", "of", "ml"):
            assert sum(cen["seq_%s_%s" % (t, m)] for m in ("predefined", "rle", "fse", "repeat")) == with_seq, (name, t)
        assert cen["tail_literals_none"] + cen["tail_literals_some"] == with_seq, name
        nseq = cen["off_new"] + sum(cen[k] for k in ("off_rep0", "off_rep1", "off_rep2", "off_ll0_rep1", "off_ll0_rep2", "off_ll0_rep0_minus_1"))
        assert cen["seq_literal_length_0"] <= nseq and (nseq > 0) == (with_seq > 0), name
        assert cen["lit_streams_1"] + cen["lit_streams_4"] == lits - sum(cen[k] for k in cen if k.startswith(("lit_raw", "lit_rle"))), name
        assert cen["huf_description_direct"] + cen["huf_description_fse"] == sum(cen["lit_compressed_format_%d" % k] for k in range(4)), name


def test_census_headers_equal_an_independent_walk():
    for name, _, f, _ in Z.frames():
        cen = _census()[name]
        mine = {k: v for k, v in cen.items() if v and k.startswith(WALKED_PREFIXES)}
        assert mine == _header_walk(f), name


def test_census_refuses_what_the_decoder_refuses():
    name, c, f, _ = Z.frames()[0]
    assert O.zstd_census(f[:-1]) is None and O.zstd_restate_decompress(f[:-1], len(c)) is None
    both = np.concatenate([f, f])   # (concatenated frames: counted one after the other)
    cen = O.zstd_census(both)
    assert cen["frames"] == 2 and cen["content_size"] == 2 * len(c)


def test_every_counter_is_classified():
    names = O.census_names()
    assert len(set(names)) == len(names)
    lists = Z.REQUIRED + list(Z.UNREACHED) + Z.INFORMATIONAL
    assert sorted(lists) == sorted(names), (sorted(set(names) - set(lists)), sorted(set(lists) - set(names)), [k for k in lists if lists.count(k) > 1])
    assert set(Z.MANY_BLOCKS_ONLY) <= set(Z.REQUIRED) and set(Z.PLAIN_ONLY) <= set(Z.REQUIRED)
    assert all(isinstance(v, str) and len(v) > 20 for d in (Z.UNREACHED, Z.MANY_BLOCKS_ONLY, Z.PLAIN_ONLY) for v in d.values())
    assert O.census_maxima() <= set(Z.INFORMATIONAL)


def test_required_counters_are_reached():
    """Every REQUIRED counter: two frames at least; one of at most four blocks (REF_MAXBLK) unless MANY_BLOCKS_ONLY says why not, and
    that one an int16 svb stream unless PLAIN_ONLY says why not"""
    cen, R = _census(), Z.reads()
    short = {}
    for k in Z.REQUIRED:
        reach = [name for name, *_ in Z.frames() if cen[name][k]]
        small = [name for name in reach if _nblocks(cen[name]) <= 4]
        svb = [name for name in small if name in R]
        if len(reach) < 2 or (not small and k not in Z.MANY_BLOCKS_ONLY) or (small and not svb and k not in Z.PLAIN_ONLY):
            short[k] = (len(reach), len(small), len(svb))
        # (an exemption that is no longer needed is stale)
        assert not (k in Z.MANY_BLOCKS_ONLY and small) and not (k in Z.PLAIN_ONLY and svb), k
    assert not short, short


def test_unreached_counters_are_unreached():
    for k in Z.UNREACHED:
        assert [name for name, c in _census().items() if c[k]] == [], k


def _existing_corpora():
    """(label, frames) of the corpora the GPU suite had before this one: the int16 layouts and the plain contents of
    tests/test_gpu_block_layouts.py (that file's own functions, loaded from its path: it needs no GPU to import), and the contents of
    test_gpu_parity.test_zstd_decode_libzstd_frames at its levels (restated: they are built inside that test)"""
    spec = importlib.util.spec_from_file_location("_block_layouts", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_block_layouts.py"))
    bl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bl)
    yield "layouts", [O.zstd_compress_cuts(s, cuts, level=lv, window_log=w, checksum=ck) for _, cuts, _, s, lv, w, ck in bl.layouts()]
    yield "plain", [f for _, f in bl._plain()]
    rng = np.random.default_rng(21)
    contents = [O.svb_compress(O.synth_signal(5, i, n), 2, True, 0) for i, n in enumerate([0, 1, 5, 40, 200, 700, 1000, 3000, 9000, 30000, 100000, 110000, 400000])]
    contents += [O.svb_compress(np.arange(0, 1000, dtype=np.int16), 2, True, 0), O.svb_compress(O.synth_u32(5, 1, 200000), 4, False, 0)]
    contents += [rng.integers(0, 256, 70000, dtype=np.uint8), np.zeros(300000, np.uint8)]
    contents.append(np.frombuffer((b"the quick brown fox jumps over the lazy dog " * 4000), np.uint8).copy())
    contents.append(np.minimum(rng.geometric(0.3, 150000), 255).astype(np.uint8))
    for period in (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 79, 80, 81, 100, 255, 256, 257, 1000, 5000):
        unit = rng.integers(0, 256, period, dtype=np.uint8)
        rep = np.tile(unit, 40000 // period + 2)[: 40000 + period % 7]
        contents.append(np.concatenate([rng.integers(0, 256, 37 + period % 11, dtype=np.uint8), rep, unit[: period // 2], rep[: 300 + period]]))
    yield "libzstd_frames", [O.zstd_compress(c, lv) for c in contents for lv in (1, 3, 9)]


def test_census_of_the_existing_corpora_beside_this_one():
    """Prints (pytest -s) how many FRAMES of each corpus reach each counter (maxima: the maximum); asserts only that every frame decodes.
    DESIGN.md 2 T3 holds the table."""
    cols = {}
    for label, frames in list(_existing_corpora()) + [("feature corpus", [f for _, _, f, _ in Z.frames()])]:
        total, mx = {}, O.census_maxima()
        for f in frames:
            cen = O.zstd_census(f)
            assert cen is not None, label
            for k, v in cen.items():
                total[k] = max(total.get(k, 0), v) if k in mx else total.get(k, 0) + (v > 0)
        cols["%s (%d)" % (label, len(frames))] = total
    print("\n%-38s" % "frames that reach the counter" + "".join("%22s" % c for c in cols))
    for k in O.census_names():
        print("%-38s" % k + "".join("%22d" % t[k] for t in cols.values()))

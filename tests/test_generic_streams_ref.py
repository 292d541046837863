"""tests/generic_streams.py against the CPU oracle: encode(), decode() and build() are the oracle's generic workers and nibble codec on
the whole catalogue and on random small streams, and the catalogue holds what tests/test_gpu_generic_streams.py relies on -- counted
here, from the oracle and numpy alone, so the device tests cannot shrink unnoticed."""
import numpy as np
import pytest

import generic_streams as S
import oracle_lib as O

E_STREAM, E_DEST = 0xFFFFFFFB, 0xFFFFFFFC
KINDS = pytest.mark.parametrize("kind", S.KINDS, ids=S.kind_name)
# the words a kind's boundary rows must code, on both sides of every compare its encoder can reach
BOUNDARIES = {
    (4, False): {0, 0xFF, 0x100, 0xFFFF, 0x10000, 0xFFFFFF, 0x1000000, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF},
    (4, True): {254, 255, 256, 0xFFFF, 0x10000, 0xFFFFFF, 0x1000000, 2, 1},          # (2 and 1: the deltas that wrap through 2^32)
    (2, False): {0, 0xFF, 0x100, 0x7FFF, 0xFFFFFFFF, 0xFFFF8000},
    (1, False): {0, 1, 15, 16, 127, 0xFFFFFFFF, 0xFFFFFF80},
    (1, True): {0, 1, 15, 16, 254, 255, 256, 510, 509},
}
# the oracle's verdicts on the defects, as it gave them at every size (None: it decodes); the nibble codec reads a capacity of one
# value more as a value of code 0 (the last control byte's unused bits: no data) unless that value needs a control byte of its own; the
# byte codec misses the value's byte either way
ORACLE = {"intact": None, "last byte missing": E_STREAM, "one byte appended": E_STREAM, "src_size = K - 1": E_STREAM, "src_size = 0": E_STREAM,
          "dst_cap + E": E_STREAM, "dst_cap - E": E_STREAM, "dst_cap + 1": E_DEST, "dst_cap = 0": E_STREAM}


def oracle_table(half, n, defect):
    return None if half and defect == "dst_cap + E" and n % 4 else ORACLE[defect]


def oracle_decode(kind, buf, size, cap):
    return O.svb_decompress(buf[:size], cap, kind[0], kind[1], kind[2])


def same(got, want):
    if isinstance(want, int) or isinstance(got, int):
        return isinstance(got, int) and isinstance(want, int) and got == want
    return got.tobytes() == want.tobytes()


def test_the_kinds():
    assert len(S.KINDS) == 9 and len(set(S.KINDS)) == 9
    assert [k for k in S.KINDS if S.is_half(k)] == [(1, False, 1), (1, True, 1)]
    assert (4, True, 1) in S.KINDS and (2, False, 1) in S.KINDS   # version 1 with another size than 1: the byte codec
    assert S.geometry(4) == (4, 256, 1024, 8192) and S.geometry(2) == S.geometry(1) == (8, 512, 2048, 16384)


@KINDS
def test_encode_is_the_oracle_on_every_encoder_row(kind):
    size, zz, ver = kind
    for r in S.encoder_rows(kind):
        assert len(r.values) <= 3 * S.geometry(size)[3] + 5 <= 49157 and r.values.dtype == S.DT[size], r.name
        want = O.svb_compress(r.values, size, zz, ver)
        got = S.encode(r.values, size, zz, S.is_half(kind))
        assert same(got, want), (kind, r.name)
        assert len(got) == S.stream_len(S.code_of(S.to_u(r.values, size, zz), S.is_half(kind)), S.is_half(kind)) or len(r.values) == 0, r.name


@KINDS
def test_decode_is_the_oracle_on_every_decoder_row(kind):
    for r in S.decoder_rows(kind):
        want = oracle_decode(kind, r.buf, r.size, r.cap)
        got = S.verdict(r.buf[: r.size], r.cap, kind)
        assert same(got, want), (kind, r.name, hex(got) if isinstance(got, int) else "decoded", hex(want) if isinstance(want, int) else "decoded")
        if "own" in r.tags or "foreign" in r.tags:
            assert not isinstance(want, int), (kind, r.name, hex(want))


@KINDS
def test_build_and_decode_are_the_oracle_on_random_small_streams(kind):
    size, zz, ver = kind
    half = S.is_half(kind)
    rng = np.random.default_rng([3, S.KINDS.index(kind)])
    for j in range(200):
        n = int(rng.integers(1, 600))
        codes = rng.integers(0, 4, n)
        s = S.build(codes, rng.integers(0, 1 << 32, n).astype(np.uint64), half)
        assert len(s) == S.stream_len(codes, half)
        for stream, cap in ((s, n * size), (s[:-1], n * size), (s, n * size + size)):
            want = O.svb_decompress(stream, cap, size, zz, ver)
            assert same(S.verdict(stream, cap, kind), want), (kind, j, n, len(stream), cap)
        x = S.mix(kind, n, rng)
        assert same(S.encode(x, size, zz, half), O.svb_compress(x, size, zz, ver)), (kind, j, n)
        back = S.decode(S.encode(x, size, zz, half), n, size, zz, half)
        assert np.array_equal(back, x), (kind, j, n)


@KINDS
def test_boundaries_stand_at_every_slot_and_position_class(kind):
    size, zz, _ = kind
    V, W, T, G = S.geometry(size)
    its = S.items(kind)
    rows = [r for r in S.encoder_rows(kind) if "items" in r.marks]
    assert len(rows) == len(its)
    slots, lanes, classes, words = {}, {}, {}, {}
    for r in rows:
        u = S.to_u(r.values, size, zz)
        for k, p in r.marks["items"]:
            words.setdefault(k, set()).add(int(u[p]))
            slots.setdefault(k, set()).add(p % V)
            lanes.setdefault(k, set()).add(p // V % 256)
            cl = classes.setdefault(k, set())
            for name, hit in (("read", p == 0), ("wavefront share", p % W == 0 and p % T != 0), ("tile", p % T == 0 and p % G != 0), ("segment", p % G == 0 and p > 0)):
                if hit:
                    cl.add(name)
    for k, (name, prev, value) in enumerate(its):
        assert len(words[k]) == 1, (kind, name, words[k])   # every mark of an item codes the same word
        assert slots[k] == set(range(V)), (kind, name, slots[k])
        assert lanes[k] >= {0, 63, 64, 255}, (kind, name, lanes[k])
        want = {"wavefront share", "tile", "segment"} | ({"read"} if prev in (None, 0) else set())
        assert classes[k] == want, (kind, name, classes[k])
    assert {next(iter(w)) for w in words.values()} == BOUNDARIES[kind[:2]], (kind, sorted(hex(next(iter(w))) for w in words.values()))


@KINDS
def test_code_mixes(kind):
    size, zz, _ = kind
    half = S.is_half(kind)
    V, W, T, G = S.geometry(size)
    cs = S.codes_of(kind)
    rows = {r.name: r for r in S.encoder_rows(kind)}

    def codes(r):
        return S.code_of(S.to_u(r.values, size, zz), half)

    for r in S.encoder_rows(kind):   # every code the kind can write, at an eighth of every mixed row and more
        if r.marks.get("mixed") or r.marks.get("length", 0) >= T - 1:
            c = codes(r)
            assert set(np.unique(c)) == set(cs), (kind, r.name)
            share = min(np.mean(c == k) for k in cs)
            assert share >= 1 / 8, (kind, r.name, share)
    if half:
        assert (codes(rows["code 0 only"]) == 0).all() and len(rows["code 0 only"].values) > T
        for parity, name in ((1, "odd"), (0, "even")):
            r = rows["nibble total %s at every tile end" % name]
            c = codes(r)
            ends = np.cumsum(S.units(c, True))[T - 1 :: T]
            assert len(ends) == 3 and (ends % 2 == parity).all(), (kind, name, ends)
            assert len(set(np.unique(c))) >= 2, (kind, name)
        return
    r = rows["tiles of one length each"]
    c = codes(r).reshape(-1, T)
    assert (c == c[:, :1]).all() and c[:, 0].tolist() == r.marks["tiles"] and set(c[:, 0]) == set(cs), kind
    r = rows["length switches at lane, wavefront, tile and segment boundaries"]
    c, cuts = codes(r), r.marks["cuts"]
    kinds_of_cut = set()
    for a, p, b in zip([0] + cuts, cuts, cuts[1:] + [len(c)]):
        assert len(set(c[a:p])) == 1 and len(set(c[p:b])) == 1 and c[p - 1] != c[p], (kind, p)
        kinds_of_cut.add("segment" if p % G == 0 else "tile" if p % T == 0 else "wavefront" if p % W == 0 else "lane" if p % V == 0 else "none")
    assert kinds_of_cut == {"lane", "wavefront", "tile", "segment"}, kinds_of_cut


@KINDS
def test_length_rows_reach_every_flush_remainder(kind):
    """the encoder's stage flushes whole 16-byte lines at a tile's end and keeps the rest: every rest 0 ... 15 at some tile end"""
    size, zz, _ = kind
    half = S.is_half(kind)
    V, W, T, G = S.geometry(size)
    got = [r.marks["length"] for r in S.encoder_rows(kind) if "length" in r.marks]
    assert got == [0, 1, V - 1, V, V + 1, W - 1, W, W + 1, T - 1, T, T + 1, 2 * T - 1, 2 * T + 1, G - 1, G, G + 1, 2 * G + 3, 3 * G + 5]
    rests, parities = set(), set()
    for r in S.encoder_rows(kind):
        if "length" in r.marks and len(r.values):
            m = S.units(S.code_of(S.to_u(r.values, size, zz), half), half)
            ends = np.cumsum(m)[np.r_[T - 1 : len(m) : T, len(m) - 1]]
            if half:
                parities |= set((ends % 2).tolist())
                ends = ends // 2
            rests |= set((ends % 16).tolist())
    assert rests == set(range(16)), (kind, sorted(rests))
    assert not half or parities == {0, 1}


@KINDS
def test_foreign_rows(kind):
    size, zz, _ = kind
    half = S.is_half(kind)
    V, W, T, G = S.geometry(size)
    rows = [r for r in S.decoder_rows(kind) if "foreign" in r.tags]
    counts = lambda tag: sorted(r.cap // size for r in rows if tag in r.tags)
    assert counts("random") == [T + 5, 2 * T, G + 1, 3 * G + 5]
    assert counts("padded") == [T + 5, G + 1] and len(counts("wraps")) == (1 if zz and not half else 0)
    assert counts("high bits") == ([G + 1] if half else []) and counts("unused nibble") == ([T + 5, 3 * G + 5] if half else [])

    def layout(r):
        n = r.cap // size
        c = ((r.buf[: (n + 3) // 4, None] >> np.array([0, 2, 4, 6], np.uint8)) & 3).reshape(-1)[:n].astype(np.int64)
        return n, c

    for r in rows:
        n, c = layout(r)
        if "random" in r.tags:   # every code, and the announced width in use: values the kind's own encoder never writes
            assert min(np.mean(c == k) for k in range(4)) > 0.2, (kind, r.name)
            raw = S.decode(r.buf, n, 4, False, half) if not half else None
            if raw is not None and size < 4:
                assert np.mean(raw.view(np.uint32) >> (8 * size) != 0) > 0.3, (kind, r.name)   # wide codes in a narrow type
        if "padded" in r.tags:
            assert c.min() >= 1 and set(np.unique(c)) == {1, 2, 3}
            got = S.decode(r.buf, n, 4, False, False) if not half else None
            assert half or int(got.view(np.uint32).max()) < 256
        if "wraps" in r.tags:
            v = S.decode(r.buf, n, 4, False, False).view(np.uint32).astype(np.uint64)
            assert int(np.cumsum(v >> np.uint64(1))[-1]) >> 32 >= 100, kind   # (all deltas positive)
        if "high bits" in r.tags:
            assert np.mean(c == 3) > 0.8
        if "unused nibble" in r.tags:
            assert int(S.units(c, True).sum()) % 2 == 1 and r.buf[r.size - 1] >> 4 == 0xF
            clean = r.buf.copy()
            clean[r.size - 1] &= 0x0F
            assert same(oracle_decode(kind, clean, r.size, r.cap), oracle_decode(kind, r.buf, r.size, r.cap))


@KINDS
def test_every_defect_at_every_size_and_the_oracles_verdicts(kind):
    size, zz, _ = kind
    half = S.is_half(kind)
    V, W, T, G = S.geometry(size)
    rows = [r for r in S.decoder_rows(kind) if "defect" in r.tags]
    count = lambda r: int(next(t for t in r.tags if t.startswith("n = "))[4:])
    names = [d for d in S.DEFECTS if not (d == "dst_cap + 1" and size == 1)]
    assert len(names) == (8 if size == 1 else 9)
    for n in (9, W + 1, T + 1, 2 * T + 5):
        have = [d for r in rows if "n = %d" % n in r.tags for d in names if d in r.tags]
        assert have == names, (kind, n, have)
    big = [r for r in rows if "n = %d" % (2 * G + 1000) in r.tags]
    assert sorted(d for r in big for d in names if d in r.tags) == sorted(["intact"] * 3 + ["last byte missing", "one byte appended", "dst_cap + E"])
    for r in rows:
        d = next(d for d in names if d in r.tags)
        want = oracle_decode(kind, r.buf, r.size, r.cap)
        assert (want if isinstance(want, int) else None) == oracle_table(half, count(r), d), (kind, r.name, hex(want) if isinstance(want, int) else "decoded")
    if half:   # "one byte appended" where the nibble total is odd and where it is even
        assert {t for r in rows if "one byte appended" in r.tags for t in r.tags if t.startswith("nibbles")} == {"nibbles odd", "nibbles even"}
    errors = sum(isinstance(oracle_decode(kind, r.buf, r.size, r.cap), int) for r in rows)
    assert (len(rows), errors) == ((38, 27) if half else (38, 31) if size == 1 else (42, 35)), (kind, len(rows), errors)

"""CPU tests of vbz_compression_amd/csrc/zstd_tables.h, the table readers every zstd decoder of the library instantiates: on table
descriptions from the library's encoder, from libzstd, damaged copies of them and random bytes, each verdict, each count, each cell of an
FSE table and each Huffman code length must be what the oracle's restatement (oracle/zstd_restate.c) gives."""
import ctypes

import numpy as np

import entropy_host as E
import oracle_lib as O

# (max_symbol, max_log) of the descriptions the decoders read: literal lengths, offsets, match lengths, Huffman weights
PAIRS = ((35, 9), (31, 8), (52, 9), (11, 6))


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def oracle_ncount(desc, max_symbol, max_log):
    p = np.frombuffer(bytes(desc), np.uint8).copy()
    norm = np.zeros(256, np.int16)
    log, nsym = ctypes.c_int(0), ctypes.c_int(0)
    r = O.lib().vbo_debug_fse_read_ncount(_ptr(p), len(p), _ptr(norm), max_symbol, max_log, ctypes.byref(log), ctypes.byref(nsym))
    return (r, log.value, norm[: nsym.value].copy()) if r >= 0 else (r, None, None)


def oracle_fse_build(norm, log):
    norm = np.ascontiguousarray(norm, np.int16)
    sym, nb, base = np.zeros(1 << log, np.uint8), np.zeros(1 << log, np.uint8), np.zeros(1 << log, np.uint16)
    if O.lib().vbo_debug_fse_build(_ptr(norm), len(norm), log, _ptr(sym), _ptr(nb), _ptr(base)) != 0:
        return None
    return sym.astype(np.uint32) | (nb.astype(np.uint32) << 8) | (base.astype(np.uint32) << 16)


def oracle_huf(desc):
    p = np.frombuffer(bytes(desc), np.uint8).copy()
    nb = np.zeros(256, np.uint8)
    used = ctypes.c_int(0)
    log = O.lib().vbo_debug_huf_lengths(_ptr(p), len(p), _ptr(nb), ctypes.byref(used))
    return (used.value, log, nb) if log >= 0 else (-1, None, None)


def lengths(log, weights):
    nb = np.zeros(256, np.uint8)
    for s, w in enumerate(weights):
        nb[s] = log + 1 - int(w) if w else 0
    return nb


def _data(rng, it):
    n = int(rng.integers(2000, 40000))
    kind = it % 3
    if kind == 0:
        a = O.synth_signal(7, it, n)
        return O.svb_compress(a, 2, True, 0)
    if kind == 1:
        return np.clip(rng.normal(128, rng.uniform(2, 40), n), 0, 255).astype(np.uint8)
    return np.minimum(rng.geometric(rng.uniform(0.02, 0.5), n), 255).astype(np.uint8)


def _libzstd_descriptions(rng):
    """Tree descriptions and sequence-table descriptions (each with the rest of its block behind it) of the first block of libzstd frames."""
    trees, seqs = [], []
    for level in range(1, 20):
        for it in range(3):
            frame = bytes(O.zstd_compress(_data(rng, 3 * level + it), level))
            lit = E.parse_first_block_literals(frame)
            if lit is None or lit[0] < 2:
                continue
            if lit[3] is not None:
                trees.append(lit[3])
            # the sequences section: behind the literals section
            fhd = frame[4]
            single = (fhd >> 5) & 1
            pos = 5 + (0 if single else 1) + [1 if single else 0, 2, 4, 8][fhd >> 6]
            bsize = int.from_bytes(frame[pos : pos + 3], "little") >> 3
            end = pos + 3 + bsize
            fmt = (frame[pos + 3] >> 2) & 3
            q = pos + 3 + (3 if fmt < 2 else fmt + 2) + lit[2]
            ns = frame[q]
            q += 1 if ns < 128 else (3 if ns == 255 else 2)
            if ns == 0:
                continue
            modes = frame[q]
            q += 1
            for kind, shift in enumerate((6, 4, 2)):
                mode = (modes >> shift) & 3
                if mode == 1:
                    q += 1
                elif mode == 2:
                    ms, ml = ((35, 9), (31, 8), (52, 9))[kind]
                    used = oracle_ncount(frame[q:end], ms, ml)[0]
                    assert used > 0
                    seqs.append(frame[q : min(end, q + 200)])
                    q += used
    return trees, seqs


def _damaged(rng, descs, per):
    out = []
    for d in descs:
        for _ in range(per):
            b = bytearray(d)
            for _ in range(int(rng.integers(1, 4))):
                bit = int(rng.integers(0, 8 * len(b)))
                b[bit >> 3] ^= 1 << (bit & 7)
            out.append(bytes(b))
        out.append(bytes(d[: int(rng.integers(0, len(d)))]))
        out.append(bytes(d[: max(0, len(d) - 1)]))
    return out


def _inputs():
    rng = np.random.default_rng(11)
    trees = [E.tree_description(_data(rng, it))[2] for it in range(60)]
    trees = [t for t in trees if t]
    # a complete code of table log 12, direct weights 11, 10, ..., 2, 1, 1 (and the implied 12)
    w = list(range(11, 0, -1)) + [1]
    trees.append(bytes([127 + len(w)] + [(w[i] << 4) | w[i + 1] for i in range(0, len(w), 2)]))
    seqs = []
    if O.lib().vbo_zstd_version() is not None:
        zt, seqs = _libzstd_descriptions(rng)
        assert len(zt) > 20 and len(seqs) > 20
        trees += zt
    rand = [rng.integers(0, 256, int(rng.integers(0, 160)), dtype=np.uint8).tobytes() for _ in range(1500)]
    return trees + _damaged(rng, trees, 6), seqs + _damaged(rng, seqs, 6), rand


def test_fse_descriptions_and_tables_match_the_oracle():
    trees, seqs, rand = _inputs()
    # the FSE part of a tree description starts behind its header byte
    descs = [t[1:] for t in trees if t and t[0] < 128] + seqs + rand
    accepted = refused = tables = 0
    for d in descs:
        for ms, ml in PAIRS:
            got, want = E.fse_read_ncount(d, ms, ml), oracle_ncount(d, ms, ml)
            assert got[0] == want[0], (d.hex(), ms, ml)
            if want[0] < 0:
                refused += 1
                continue
            accepted += 1
            assert got[1] == want[1] and np.array_equal(got[2], want[2]), (d.hex(), ms, ml)
            cells, ref = E.fse_build(got[2], got[1]), oracle_fse_build(want[2], want[1])
            assert (cells is None) == (ref is None), (d.hex(), ms, ml)
            if ref is not None:
                assert np.array_equal(cells, ref), (d.hex(), ms, ml)
                tables += 1
    assert accepted > 2000 and refused > 2000 and tables > 2000, (accepted, refused, tables)


def test_tree_descriptions_match_the_oracle():
    trees, seqs, rand = _inputs()
    accepted = refused = deferred = 0
    for d in trees + rand:
        used, log, nb = oracle_huf(d)
        r12, log12, w12 = E.huf_read_weights(d, 12)
        r11, log11, w11 = E.huf_read_weights(d, 11)
        if used < 0:
            refused += 1
            assert r12 == -1 and r11 < 0, d.hex()
            continue
        accepted += 1
        assert r12 == used and log12 == log and np.array_equal(lengths(log12, w12), nb), d.hex()
        if log == 12:
            deferred += 1
            assert r11 == -2, d.hex()
        else:
            assert r11 == used and log11 == log and np.array_equal(lengths(log11, w11), nb), d.hex()
    assert accepted > 100 and refused > 1000 and deferred >= 1, (accepted, refused, deferred)

"""The generic svb workers and the v1 nibble codec on the MI355X over the catalogue of tests/generic_streams.py (svb_kernels.hip: the five
generic instantiations of svb_encode_range / svb_decode_range, svb_seg_encode_kernel / svb_seg_decode_kernel and their scans,
svb_half_encode_kernel / svb_half_decode_kernel).  Every comparison is exact: the oracle's bytes or its error code.
(a) the stage entry points, at destinations and sources aligned to 64 bytes and placed anywhere: every encoder row gives the oracle's
stream, every decoder row -- own streams, foreign streams, defects -- the oracle's bytes or verdict.  (b) level-0 codec calls, where the
svb stream is the frame: the only way into the segmented kernels (the stage entry points launch the one-workgroup kernels), on the
default context, both forced paths and the large-read path with scan launches.  The nibble kinds never take segments (vbz_api.hip:
half_codec): they run in all four shapes anyway, and it is the same kernel each time.  (c) level 1, the whole codec, both ways across
the oracle: the hand-over between the svb and the entropy stage for streams that look nothing like int16 signal -- control bytes all
zero or all 0xFF, no data section at all.  (d) a batch's rows do not depend on their order, and a failed row leaves its neighbours'
outputs and the bytes between the slots alone (what its own slot holds after an error is unspecified: include/vbz_gpu.h).
tests/test_generic_streams_ref.py holds the catalogue to the oracle and counts what it contains."""
import ctypes

import numpy as np
import pytest
import torch

import generic_streams as S
import oracle_lib as O
from typed_support import arena, codec, i32, u32
from vbz_compression_amd import _lib, batch

pytestmark = pytest.mark.gpu

KINDS = pytest.mark.parametrize("kind", S.KINDS, ids=S.kind_name)
SHAPES = [{}, {"VBZ_HIP_SEGMENTED": 0}, {"VBZ_HIP_SEGMENTED": 1}, {"VBZ_HIP_SEGMENTED": 1, "VBZ_HIP_SEG_SELF_MAX": 0}]
# (DST_ALIGN, SRC_ALIGN, SRC_SKEW) of gpu_util: data sections that start anywhere (A in svb_encode_range, mis in the decoders), and
# values that do not start on a 16-byte line (in_aligned == false)
PLACEMENTS = [(64, 64, 0), (1, 64, 0), (64, 1, 3), (1, 1, 3)]
FILL = 0xA5

_oracle = {}


def oracle_streams(kind):
    """the oracle's svb stream of every encoder row"""
    if ("enc", kind) not in _oracle:
        _oracle["enc", kind] = [O.svb_compress(r.values, *kind) for r in S.encoder_rows(kind)]
    return _oracle["enc", kind]


def oracle_decodes(kind):
    """the oracle's bytes or verdict of every decoder row"""
    if ("dec", kind) not in _oracle:
        _oracle["dec", kind] = [O.svb_decompress(r.buf[: r.size], r.cap, *kind) for r in S.decoder_rows(kind)]
    return _oracle["dec", kind]


def show(v):
    return hex(v) if isinstance(v, int) else "%d bytes" % len(v)


def expect(kind, what, names, got, want):
    assert len(got) == len(want) == len(names)
    bad = [(n, show(g), show(w)) for n, g, w in zip(names, got, want)
           if isinstance(g, int) != isinstance(w, int) or (g != w if isinstance(w, int) else g.tobytes() != w.tobytes())]
    assert not bad, (S.kind_name(kind), what, len(bad), "of", len(want), bad[:6])


def call(c, fn, bufs, sizes, caps, fill=0):
    """one batched call: bufs in source slots of their own, sizes / caps as the descriptors give them, the destination arena filled with
    `fill` first.  Returns (result[], the arena on the host, every slot's offset)"""
    dev = c.device
    src, off, _ = arena(c, bufs, 64)
    doff, total = batch.layout([int(x) + 32 for x in caps], 64)
    dst = torch.full((total + 64,), fill, dtype=torch.uint8, device=dev)
    res = torch.full((len(bufs),), -8, dtype=torch.int32, device=dev)
    fn(src, off, i32(sizes).to(dev), dst, doff.to(dev), i32(caps).to(dev), res)
    torch.cuda.synchronize()
    return [int(x) for x in u32(res)], dst.cpu().numpy(), doff.tolist()


def outputs(res, host, doff):
    return [r if _lib.is_error(r) else host[o : o + r].copy() for r, o in zip(res, doff)]


# ---- (a) the stage entry points -----------------------------------------------------------------------------------------------------------
@KINDS
def test_stage_entry_points(kind):
    import gpu_util as G

    size, zz, ver = kind
    enc, dec = S.encoder_rows(kind), S.decoder_rows(kind)
    old = G.DST_ALIGN, G.SRC_ALIGN, G.SRC_SKEW
    try:
        for place in PLACEMENTS:
            G.DST_ALIGN, G.SRC_ALIGN, G.SRC_SKEW = place
            got = G.svb_compress([r.values for r in enc], size, zz, ver)
            expect(kind, ("svb_compress", place), [r.name for r in enc], got, oracle_streams(kind))
            got = G.svb_decompress([r.buf[: r.size] for r in dec], [r.cap for r in dec], size, zz, ver)
            expect(kind, ("svb_decompress", place), [r.name for r in dec], got, oracle_decodes(kind))
    finally:
        G.DST_ALIGN, G.SRC_ALIGN, G.SRC_SKEW = old


# ---- (b) level-0 codec calls --------------------------------------------------------------------------------------------------------------
def codec_compress(c, values, opts, sized):
    caps = [c.L.vbz_max_compressed_size(int(x.nbytes), ctypes.byref(opts)) for x in values]
    return outputs(*call(c, lambda *a: c.compress(*a, opts, sized=sized), values, [x.nbytes for x in values], caps))


@KINDS
def test_level_0_codec_calls(kind):
    size, zz, ver = kind
    enc, dec = S.encoder_rows(kind), S.decoder_rows(kind)
    oo = O.options(zz, size, 0, ver)
    want_enc = {sized: [O.compress(r.values, oo, sized=sized) for r in enc] for sized in (False, True)}
    want_dec = [O.decompress(r.buf[: r.size], r.cap, oo) for r in dec]
    expect(kind, "the oracle's level-0 decode is its svb decode", [r.name for r in dec], want_dec, oracle_decodes(kind))
    for knobs in SHAPES:
        c = codec(**knobs)
        opts = c.options(zz, size, 0, ver)
        for sized in (False, True):
            expect(kind, ("compress", knobs, "sized" if sized else "unsized"), [r.name for r in enc], codec_compress(c, [r.values for r in enc], opts, sized),
                   want_enc[sized])
        got = outputs(*call(c, lambda *a: c.decompress(*a, opts), [r.buf for r in dec], [r.size for r in dec], [r.cap for r in dec]))
        expect(kind, ("decompress", knobs), [r.name for r in dec], got, want_dec)


# ---- (c) level 1, the whole codec ---------------------------------------------------------------------------------------------------------
@KINDS
def test_level_1_both_ways_across_the_oracle(kind):
    size, zz, ver = kind
    enc = S.encoder_rows(kind)
    values = [r.values for r in enc]
    names = [r.name for r in enc]
    raw = [np.frombuffer(x.tobytes(), np.uint8) for x in values]
    oo = O.options(zz, size, 1, ver)
    theirs = [O.compress(x, oo) for x in values]
    assert not any(isinstance(f, int) for f in theirs)
    for knobs in ({}, {"VBZ_HIP_SPLIT_MIN": 8}):
        c = codec(**knobs)
        opts = c.options(zz, size, 1, ver)
        ours = codec_compress(c, values, opts, False)
        assert not any(isinstance(f, int) for f in ours), (S.kind_name(kind), knobs, [(n, show(f)) for n, f in zip(names, ours) if isinstance(f, int)][:6])
        expect(kind, ("the oracle decodes the device's frames", knobs), names, [O.decompress(f, x.nbytes, oo) for f, x in zip(ours, values)], raw)
        got = outputs(*call(c, lambda *a: c.decompress(*a, opts), theirs, [len(f) for f in theirs], [x.nbytes for x in values]))
        expect(kind, ("the device decodes the oracle's frames", knobs), names, got, raw)


# ---- (d) independence inside a batch ------------------------------------------------------------------------------------------------------
def in_both_orders(kind, what, c, fn, names, bufs, sizes, caps, want):
    n = len(bufs)
    runs = []
    for order in (list(range(n)), list(range(n))[::-1]):
        res, host, doff = call(c, fn, [bufs[i] for i in order], [sizes[i] for i in order], [caps[i] for i in order], fill=FILL)
        out = outputs(res, host, doff)
        expect(kind, what, [names[i] for i in order], out, [want[i] for i in order])
        untouched = np.ones(len(host), bool)
        for r, o, cp in zip(res, doff, [caps[i] for i in order]):
            untouched[o : o + (cp if _lib.is_error(r) else r)] = False   # (a failed row's own slot: unspecified)
        assert (host[untouched] == FILL).all(), (S.kind_name(kind), what, "bytes outside the rows' outputs were written", int(np.argmax(untouched & (host != FILL))))
        runs.append({order[j]: out[j] for j in range(n)})
    expect(kind, (what, "reversed order"), names, [runs[1][i] for i in range(n)], [runs[0][i] for i in range(n)])
    return runs[0]


@KINDS
def test_rows_of_a_batch_are_independent(kind):
    size, zz, ver = kind
    c = codec()
    enc, dec = S.encoder_rows(kind), S.decoder_rows(kind)
    values = [r.values for r in enc]
    in_both_orders(kind, "svb_compress", c, lambda *a: c.svb_compress(*a, size=size, zigzag=zz, version=ver), [r.name for r in enc], values,
                   [x.nbytes for x in values], [(len(x) + 3) // 4 + 4 * len(x) for x in values], oracle_streams(kind))
    got = in_both_orders(kind, "svb_decompress", c, lambda *a: c.svb_decompress(*a, size=size, zigzag=zz, version=ver), [r.name for r in dec],
                         [r.buf for r in dec], [r.size for r in dec], [r.cap for r in dec], oracle_decodes(kind))
    failed = sum(isinstance(g, int) for g in got.values())
    assert failed >= 4 * 6 + 2 and failed < len(dec) // 2, (failed, len(dec))   # the defects' error rows, among neighbours that decode

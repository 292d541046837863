"""The feature corpus of libzstd frames (tests/zstd_feature_corpus.py) on every device decode path (-m gpu).

DESIGN.md 2 T3: the device decodes every frame libzstd writes, bit for bit, on every path.  The corpus states that promise per RFC 8878
feature (tests/test_zstd_feature_corpus_host.py holds its census); here every frame goes through vbz_gpu_zstd_decompress_batch -- all in
one call with roomy slots, all in one call with slots of exactly the content, every frame of at most four blocks alone --, the int16 ones
through vbz_gpu_decompress_batch and one calibrated float32 call, and damaged copies through the zstd stage, on the five paths of
tests/test_gpu_block_layouts.py.  Bytes are held to the content libzstd was given, verdicts to libzstd's, the walked counts to the walk's
admission rule restated below from zstd_decode_ref.hip."""
import hashlib
import os
import pickle
import subprocess
import sys
import tempfile
import time

import ctypes
import numpy as np
import pytest

import oracle_lib as O
import signal_ref as SR
import zstd_feature_corpus as Z

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
REF_MAXBLK, REF_HDR = 4, 160   # vbz_kernels.h, zstd_decode_ref.hip
CHILD_TIMEOUT = 120            # seconds a path: some ten times what the first run's children took (the test's docstring)

# include/vbz.h: "A frame whose header gives no Frame_Content_Size is VBZ_ZSTD_ERROR, as in the reference's vbz_decompress, which asks
# ZSTD_getFrameContentSize first and takes "unknown" for an error (vbz/vbz.cpp:236-240); ZSTD_decompress alone would decode it."
# These frames must be REFUSED on every path; every other frame of the corpus must decode.
NO_CONTENT_SIZE = ["svb_streamed_L3", "svb_nosize_L1", "svb_small_streamed_L1", "bytes0_streamed_L3", "bytes1_streamed_L3", "bytes0_nosize_L1"]


# REQUIRED counters that the chain walk never sees, by its admission rule (zstd_decode_ref.hip, ref_frame): the one-wavefront decoder alone
# decodes these, on every path
NOT_WALKED = {
    "frame_content_size_0_bytes": "BAIL(5), and the frame is refused by every path (NO_CONTENT_SIZE)",
    "seq_count_3_bytes": "BAIL(18): a sequences section whose count takes three bytes is left to the one-wavefront decoder",
}


def _slot(n):
    """a roomy slot: the pieces' stripes need room behind the content (tests/test_gpu_block_layouts.py)"""
    return 2 * n + (256 << 10)


def walk_admits(frame, cap):
    """zstd_decode_ref.hip, ref_frame, restated for a VALID frame: does the chain walk take it?  At least 32 bytes; no Dictionary_ID field;
    a content size, within the slot and below 2^30; at least one and at most REF_MAXBLK blocks with sequences; every sequences section
    with a count in one or two bytes (BAIL 18), a header -- count, modes, table descriptions -- that ends inside its first REF_HDR staged
    bytes (BAIL 20, 23 .. 26), not of the zero-run shape of this library's own encoder (BAIL 22: predefined lengths, RLE offsets of
    code 0); and at most one sequence per 16 bytes of content so far (BAIL 31)."""
    f = bytes(frame)
    if len(f) < 32 or f[4] & 0x08 or f[4] & 3 or ((f[4] >> 6) == 0 and not f[4] & 0x20):
        return False
    pos, fcs, _, _ = O.zstd_frame_geometry(f)
    if fcs > cap or fcs >= 1 << 30:
        return False
    L, hdr = O.lib(), (ctypes.c_uint32 * 4)()
    nblk = seqs = 0
    while True:
        bh = int.from_bytes(f[pos : pos + 3], "little")
        last, btype, bsize = bh & 1, bh >> 1 & 3, bh >> 3
        pos += 3
        if btype == 2:
            b = np.frombuffer(f[pos : pos + bsize], np.uint8)
            sq = b[L.vbo_debug_lit_header(b.ctypes.data, len(b), hdr) + hdr[2] :]
            if sq[0]:
                if nblk == REF_MAXBLK or sq[0] == 255:
                    return False
                hn = min(len(sq), REF_HDR)
                ns, used = (int(sq[0]), 1) if sq[0] < 128 else (((int(sq[0]) - 128) << 8) + int(sq[1]), 2)
                if used >= hn:
                    return False
                modes = int(sq[used])
                used += 1
                for shift, max_sym, max_log in ((6, 35, 9), (4, 31, 8), (2, 52, 9)):
                    mode = modes >> shift & 3
                    if shift == 4 and modes == 0x10 and used < hn and sq[used] == 0:
                        return False
                    if mode == 1:
                        used += 1
                    elif mode == 2:
                        t = np.ascontiguousarray(sq[used:hn])
                        norm, lg, nsym = np.zeros(256, np.int16), ctypes.c_int(), ctypes.c_int()
                        u = L.vbo_debug_fse_read_ncount(t.ctypes.data if len(t) else None, len(t), norm.ctypes.data, max_sym, max_log, ctypes.byref(lg), ctypes.byref(nsym))
                        if u < 0:
                            return False
                        used += u
                if used >= hn:
                    return False
                seqs += ns
                if 16 * seqs > fcs:
                    return False
                nblk += 1
        pos += 1 if btype == 1 else bsize
        if last:
            return nblk > 0


def _damaged(seed, frames, sources):
    """8 copies of each source frame with one or two bit flips inside block bodies: (buffer, source index)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in sources:
        f = frames[i]
        blocks, pos = [], O.zstd_frame_geometry(f)[0]
        while True:
            bh = int.from_bytes(bytes(f[pos : pos + 3]), "little")
            body = 1 if bh >> 1 & 3 == 1 else bh >> 3
            if body:
                blocks.append((pos + 3, body))
            pos += 3 + body
            if bh & 1:
                break
        if not blocks:
            continue
        for _ in range(8):
            g = f.copy()
            for _ in range(int(rng.integers(1, 3))):
                at, body = blocks[int(rng.integers(0, len(blocks)))]
                g[at + int(rng.integers(0, body))] ^= 1 << int(rng.integers(0, 8))
            out.append((g, i))
    return out[:600]


_CODE = r"""
import hashlib, os, sys, pickle, time
import numpy as np
import torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
import gpu_util as G
from vbz_compression_amd import _lib
t0 = time.time()
J = pickle.load(open(sys.argv[1], 'rb'))
out = {}
def dig(v):
    return [o if isinstance(o, int) else (len(o), hashlib.sha1(o.tobytes()).hexdigest()) for o in v]
def rec(key, v):
    out[key] = dig(v)
    out[key + '_paths'] = G.codec().decode_paths()
    out[key + '_ahead'] = G.codec().decode_literals_ahead()
F = J['frames']
# 1a. every frame in one call, shuffled, roomy slots
got = G.zstd_decompress([F[i] for i in J['order']], [J['roomy'][i] for i in J['order']])
back = [None] * len(F)
for i, g in zip(J['order'], got):
    back[i] = g
rec('roomy', back)
# 1b. every frame in one call, slots of exactly the content, one behind the other without a gap: a decoder that stages beyond its output
#     lands in its neighbour, or in the canary behind the last
c = G.codec(); dev = c.device
arena, off, sizes = G._pack(F)
caps = J['exact']
doff = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
dst = torch.full((int(doff[-1]) + 4096,), 0xA5, dtype=torch.uint8, device=dev)
res = torch.full((len(F),), -8, dtype=torch.int32, device=dev)
c.zstd_decompress(torch.from_numpy(arena).to(dev), off.to(dev), torch.tensor(sizes, dtype=torch.int32).to(dev), dst, torch.from_numpy(doff[:-1].copy()).to(dev),
                  torch.tensor(caps, dtype=torch.int32).to(dev), res)
torch.cuda.synchronize()
h = dst.cpu().numpy()
rr = [int(x) & 0xFFFFFFFF for x in res.cpu().tolist()]
rec('exact', [r if _lib.is_error(r) else h[o : o + r].copy() for r, o in zip(rr, doff.tolist())])
out['exact_canary'] = bool((h[int(doff[-1]):] == 0xA5).all())
# 2. every frame of at most four blocks alone in a call
for i in J['single']:
    rec('single%%d' %% i, G.zstd_decompress([F[i]], [J['roomy'][i]]))
# 3. the int16 frames to samples
o16 = _lib.CompressionOptions(True, 2, 1, 1)
f16 = [F[i] for i in J['svb']]
rec('i16', G.decompress(f16, J['n16'], o16))
# 4. ... and to calibrated float32
arena, off, sizes = G._pack(f16)
nsamp = [n // 2 for n in J['n16']]
toff, t = [], 0
for k in nsamp:
    toff.append(t); t += (4 * k + 63) // 64 * 64
dst = torch.zeros(t // 4 + 16, dtype=torch.float32, device=dev)
res = torch.full((len(nsamp),), -8, dtype=torch.int32, device=dev)
c.decompress_signal(torch.from_numpy(arena).to(dev), off.to(dev), torch.tensor(sizes, dtype=torch.int32).to(dev), dst,
                    torch.tensor(toff, dtype=torch.int64, device=dev), torch.tensor([4 * k for k in nsamp], dtype=torch.int32).to(dev), res, o16,
                    scale=torch.from_numpy(J['scale']).to(dev), offset=torch.from_numpy(J['offset']).to(dev))
torch.cuda.synchronize()
out['typed_paths'] = c.decode_paths()
out['typed_ahead'] = c.decode_literals_ahead()
h = dst.cpu().numpy().view(np.uint8)
out['typed'] = dig([int(r) & 0xFFFFFFFF if r < 0 else h[o : o + int(r)].copy() for r, o in zip(res.cpu().tolist(), toff)])
# 5. damaged frames
rec('bad', G.zstd_decompress(J['bad'], J['bad_cap']))
out['seconds'] = time.time() - t0
pickle.dump(out, open(sys.argv[2], 'wb'))
""" % (ROOT, TESTS)

# the decode paths: (name, environment); VBZ_HIP_REF_UNITS=4 everywhere (blocks a frame whose literals may be decoded beside the walk)
PATHS = [("default", {}),
         ("walk_lds", dict(VBZ_HIP_REF_CHAINS="2", VBZ_HIP_REF_TABLES="lds", VBZ_HIP_REF_LITERALS="1")),
         ("walk_mem", dict(VBZ_HIP_REF_CHAINS="2", VBZ_HIP_REF_TABLES="mem", VBZ_HIP_REF_LITERALS="1")),
         ("walk_nolits", dict(VBZ_HIP_REF_CHAINS="2", VBZ_HIP_REF_TABLES="lds", VBZ_HIP_REF_LITERALS="0")),
         ("nowalk", dict(VBZ_HIP_REF_CHAINS="0", VBZ_HIP_REF_TABLES="lds", VBZ_HIP_REF_LITERALS="1"))]


def _dig(a):
    a = np.ascontiguousarray(a)
    return (a.nbytes, hashlib.sha1(a.tobytes()).hexdigest())


def test_feature_corpus_on_every_decode_path():
    """Every corpus frame through vbz_gpu_zstd_decompress_batch (all in one call in a shuffled order with slots of 2 x content + 256 KiB; all in
    one call with slots of exactly the content -- 1 byte for the empty one -- laid one behind the other without a gap, a canary behind the
    last; every frame of at most four blocks, and whatever else the walk admits, alone in a call), the int16 ones through
    vbz_gpu_decompress_batch (version 1, zig-zag, size 2) and through one decompress_signal call to float32 with a scale and an offset per
    read (tests/signal_ref.py), and 8 damaged copies (one or two bit flips inside block bodies) of the first two frames that reach each
    REQUIRED counter, on five paths: the defaults; walked with the tables in LDS, in memory, without the literals beside the walk; not
    walked.  Every output equals the content libzstd was given (the samples, their typed bits) and has its length; no frame is refused
    but those of NO_CONTENT_SIZE, which every path refuses; a damaged frame is refused or gives exactly what libzstd gives, and at least
    a quarter are refused (libzstd alone refuses that share of the chosen buffers: checked before any child starts); all five paths agree
    on everything.

    What must have run: on the three walking paths every frame that walk_admits() admits is walked, alone and in the roomy call (the
    count is at least theirs), the int16 ones in the svb and the typed call too; nothing is walked on `nowalk`, no literals are decoded
    beside the walk on `walk_nolits` and `nowalk`.  The first run (140 frames, 132 of at most four blocks, 102 admitted, 61 of the 72
    int16 ones): the walking paths walked exactly the 102, alone and in both calls of all frames, and 61 in the svb and typed calls;
    literals beside the walk for 39 frames alone and in the roomy call, 23 in the svb call, none in the call with exact slots (the
    pieces' stripes need room behind the content).  Damaged: 384 buffers of 48 frames, libzstd refuses 129, the device 136.

    Per REQUIRED counter, frames that reach it and decode / of those walked / with literals beside the walk (walk_lds, one frame a call,
    first run): frame_single_segment 111/86/37, frame_window_descriptor 23/16/2, frame_content_size_0_bytes 0/0/0,
    frame_content_size_1_byte 8/6/0, frame_content_size_2_bytes 45/33/8, frame_content_size_4_bytes 81/63/31, frame_checksum 17/14/10,
    frame_window_log_up_to_16 20/13/0, frame_window_log_17_to_19 2/2/2, frame_window_log_from_20 1/1/0, block_raw 33/25/6, block_rle 6/2/0,
    block_compressed 130/102/39, block_last 134/102/39, block_not_last 100/77/34, block_raw_empty 3/2/2, lit_raw_header_1_byte 23/9/2,
    lit_raw_header_2_bytes 17/10/0, lit_raw_header_3_bytes 12/10/0, lit_rle_header_2_bytes 3/3/1, lit_rle_header_3_bytes 5/5/2,
    lit_compressed_format_0 10/8/0, lit_compressed_format_1 23/15/1, lit_compressed_format_2 44/34/6, lit_compressed_format_3 40/37/37,
    lit_treeless_format_0 5/3/1, lit_treeless_format_1 6/5/0, lit_treeless_format_2 9/8/6, lit_treeless_format_3 11/10/11,
    lit_streams_1 12/9/1, lit_streams_4 89/72/39, lit_treeless_tree_of_previous_block 27/22/14, lit_treeless_tree_of_earlier_block 6/4/3,
    huf_description_direct 15/11/4, huf_description_fse 85/71/37, huf_weights_log_5 85/71/37, huf_trees_11_bits 36/33/32,
    huf_trees_up_to_6_bits 18/13/2, huf_symbols_up_to_16 18/14/2, huf_symbols_above_128 48/42/30, seq_none 30/25/13,
    seq_count_1_byte 62/45/11, seq_count_2_bytes 81/68/37, seq_count_3_bytes 4/0/0, seq_ll_predefined 46/32/6, seq_ll_rle 20/18/6,
    seq_ll_fse 81/63/33, seq_ll_repeat 10/4/4, seq_of_predefined 39/27/5, seq_of_rle 20/19/7, seq_of_fse 82/64/32, seq_of_repeat 10/3/2,
    seq_ml_predefined 47/32/3, seq_ml_rle 7/5/3, seq_ml_fse 93/75/39, seq_ml_repeat 8/3/3, seq_ll_log_5 15/10/1, seq_of_log_5 22/16/7,
    seq_ml_log_5 9/5/3, seq_ll_log_9 37/26/16, seq_of_log_8 47/35/22, seq_ml_log_9 39/28/16, seq_ll_less_than_1 35/24/16,
    seq_of_less_than_1 36/25/15, seq_ml_less_than_1 37/26/15, off_new 99/79/32, off_rep0 109/85/37, off_rep1 16/10/5, off_rep2 26/17/7,
    off_ll0_rep1 62/44/24, off_ll0_rep2 27/16/8, off_ll0_rep0_minus_1 12/5/1, seq_literal_length_0 92/72/31, ll_code_35 3/2/1,
    ml_code_52 13/8/0, match_overlaps_itself 106/81/39, match_offset_1 96/76/37, match_from_before_the_block 70/52/23, off_above_64k 48/37/14,
    off_above_128k 20/15/7, off_above_1m 2/1/0, tail_literals_none 51/33/7, tail_literals_some 102/82/34.
    (literals beside the walk above the walked count: a frame of literals alone has no chain to walk, and its literals are decoded ahead
    all the same -- include/vbz_gpu.h, vbz_gpu_decode_literals_ahead.)

    REQUIRED counters that no walked frame reaches -- a statement of coverage: NOT_WALKED, held to the admission rule.

    Times of the first run: corpus, census and damaged frames 0.6 s; a child 3.1 .. 3.4 s as a process, 1.0 .. 1.1 s of it in its calls;
    the test 18 s."""
    if O.lib().vbo_zstd_version() is None:
        pytest.skip("no libzstd on this box")
    t_start = time.time()
    C = Z.frames()
    names = [name for name, *_ in C]
    contents = [c for _, c, _, _ in C]
    frames = [f for _, _, f, _ in C]
    census = [O.zstd_census(f) for f in frames]
    reads = Z.reads()
    nf = len(frames)
    assert set(NO_CONTENT_SIZE) == {names[i] for i in range(nf) if census[i]["frame_content_size_0_bytes"]}
    valid = [i for i in range(nf) if names[i] not in NO_CONTENT_SIZE]
    nblocks = [c["block_raw"] + c["block_rle"] + c["block_compressed"] for c in census]
    svb = [i for i in valid if names[i] in reads]
    roomy = [_slot(len(c)) for c in contents]
    exact = [max(len(c), 1) for c in contents]
    admit_roomy = [i for i in range(nf) if walk_admits(frames[i], roomy[i])]
    admit_exact = [i for i in range(nf) if walk_admits(frames[i], exact[i])]
    assert admit_roomy == admit_exact and len(admit_roomy) >= 60, len(admit_roomy)
    # alone in a call: every frame of at most four blocks, and whatever else the walk admits (blocks without sequences do not count there)
    single = [i for i in range(nf) if nblocks[i] <= REF_MAXBLK or i in admit_roomy]
    admit_svb = [i for i in admit_roomy if i in svb]
    assert {k for k in Z.REQUIRED if not any(census[i][k] for i in admit_roomy)} == set(NOT_WALKED)
    rng = np.random.default_rng(8879)
    # damaged copies of the first two frames that reach each REQUIRED counter; libzstd alone must refuse a quarter (else: another seed)
    sources = sorted({i for k in Z.REQUIRED for i in [j for j in valid if census[j][k]][:2]})
    for seed in range(90, 100):
        damaged = _damaged(seed, frames, sources)
        bad_cap = [_slot(len(contents[i])) for _, i in damaged]
        verdict = [O.zstd_decompress(g, cap) for (g, _), cap in zip(damaged, bad_cap)]
        if sum(v is None for v in verdict) >= len(damaged) // 4 + 8:
            break
    else:
        raise AssertionError("no seed whose damaged frames libzstd refuses often enough")
    assert 300 <= len(damaged) <= 600, len(damaged)
    J = dict(frames=frames, order=[int(x) for x in rng.permutation(nf)], roomy=roomy, exact=exact, single=single, svb=svb,
             n16=[reads[names[i]].nbytes for i in svb], bad=[g for g, _ in damaged], bad_cap=bad_cap,
             scale=rng.uniform(0.05, 2.0, len(svb)).astype(np.float32), offset=rng.uniform(-50, 50, len(svb)).astype(np.float32))
    outs, wall = {}, {}
    t_built = time.time() - t_start
    with tempfile.TemporaryDirectory() as td:
        pickle.dump(J, open(os.path.join(td, "in.pkl"), "wb"))
        for name, extra in PATHS:
            env = {k: v for k, v in os.environ.items() if not k.startswith("VBZ_HIP_REF_")}
            env.update(VBZ_HIP_REF_UNITS="4", VBZ_HIP_SEGMENTED="0", VBZ_HIP_ROUTING="0", **extra)
            t_child = time.time()
            subprocess.run([sys.executable, "-c", _CODE, os.path.join(td, "in.pkl"), os.path.join(td, "out.pkl")], check=True, env=env, timeout=CHILD_TIMEOUT)
            wall[name] = time.time() - t_child
            outs[name] = pickle.load(open(os.path.join(td, "out.pkl"), "rb"))
    print("corpus, census and damaged frames built in %.1f s; children (whole process, its calls alone): " % t_built
          + ", ".join("%s %.1f s, %.1f s" % (name, wall[name], o["seconds"]) for name, o in outs.items()))
    ref = outs["walk_lds"]
    # 1. the oracle's bytes and verdicts: the content libzstd was given, its length the content size; no valid frame refused
    want = [_dig(c) for c in contents]
    wrong = []
    for key, idx in [("roomy", range(nf)), ("exact", range(nf))] + [("single%d" % i, [i]) for i in single]:
        for g, i in zip(ref[key], idx):
            if names[i] in NO_CONTENT_SIZE:
                if g != 0xFFFFFFFF:   # VBZ_ZSTD_ERROR
                    wrong.append((key, names[i], "accepted or another verdict", g))
            elif g != want[i]:
                wrong.append((key, names[i], g, want[i]))
    for g, i in zip(ref["i16"], svb):
        if g != _dig(reads[names[i]]):
            wrong.append(("i16", names[i], g))
    for k, (g, i) in enumerate(zip(ref["typed"], svb)):
        bits = SR.typed_bits(reads[names[i]], J["offset"][k], J["scale"][k], "f32")
        if g != _dig(bits):
            wrong.append(("typed", names[i], g))
    assert not wrong, wrong[:20]
    assert ref["exact_canary"], "bytes behind the last slot were written"
    # 2. the same on every path (every difference in one message)
    keys = ["roomy", "exact", "i16", "typed", "bad"] + ["single%d" % i for i in single]
    diff = [(name, k, j) for name, o in outs.items() for k in keys for j, (a, b) in enumerate(zip(o[k], ref[k])) if a != b or len(o[k]) != len(ref[k])]
    assert not diff and all(o["exact_canary"] for o in outs.values()), diff[:40]
    # 3. damaged frames: refused, or exactly what libzstd returns
    refused = 0
    for k, (g, v) in enumerate(zip(ref["bad"], verdict)):
        if isinstance(g, int):
            refused += 1
        else:
            assert v is not None and g == _dig(v), ("accepted what libzstd refuses, or other bytes", names[damaged[k][1]], k)
    print("damaged: %d buffers of %d frames, libzstd refuses %d, the device %d" % (len(damaged), len(sources), sum(v is None for v in verdict), refused))
    assert refused >= len(damaged) // 4, (refused, len(damaged))
    # 4. what ran
    walked = {name: [i for i in single if o["single%d_paths" % i][2]] for name, o in outs.items()}
    ahead = {name: [i for i in single if o["single%d_ahead" % i]] for name, o in outs.items()}
    print("frames %d, of at most four blocks %d, admitted by the walk's rule %d (int16: %d of %d); " % (nf, len(single), len(admit_roomy), len(admit_svb), len(svb))
          + "; ".join("%s: roomy %s ahead %d, exact %s ahead %d, singles walked %d ahead %d, i16 %s ahead %d, typed %s" % (
              name, o["roomy_paths"], o["roomy_ahead"], o["exact_paths"], o["exact_ahead"], len(walked[name]), len(ahead[name]), o["i16_paths"], o["i16_ahead"],
              o["typed_paths"]) for name, o in outs.items()))
    not_walked = [names[i] for i in admit_roomy if i not in walked["walk_lds"]]
    print("admitted by the rule but not walked alone:", not_walked, "; walked beyond the rule:", [names[i] for i in walked["walk_lds"] if i not in admit_roomy])
    line = []
    for k in Z.REQUIRED:
        reach = [i for i in valid if census[i][k]]
        line.append("%s %d/%d/%d" % (k, len(reach), sum(i in walked["walk_lds"] for i in reach), sum(i in ahead["walk_lds"] for i in reach)))
    print("REQUIRED counter frames/walked/literals beside (walk_lds, one frame a call): " + ", ".join(line))
    for name in ("walk_lds", "walk_mem", "walk_nolits"):
        o = outs[name]
        assert set(admit_roomy) <= set(walked[name]), (name, [names[i] for i in admit_roomy if i not in walked[name]])
        assert o["roomy_paths"][0] == nf and o["roomy_paths"][2] >= len(admit_roomy), (name, o["roomy_paths"])
        assert o["exact_paths"][0] == nf, (name, o["exact_paths"])
        assert o["i16_paths"][2] >= len(admit_svb) and o["typed_paths"][2] >= len(admit_svb), (name, o["i16_paths"], o["typed_paths"])
    assert walked["walk_lds"] == walked["walk_mem"] == walked["walk_nolits"]
    assert not walked["nowalk"] and outs["nowalk"]["roomy_paths"][2] == 0 and outs["nowalk"]["exact_paths"][2] == 0 and outs["nowalk"]["i16_paths"][2] == 0
    for name in ("walk_nolits", "nowalk"):
        assert not ahead[name] and outs[name]["roomy_ahead"] == 0 and outs[name]["i16_ahead"] == 0, name
    assert ahead["walk_lds"] == ahead["walk_mem"]

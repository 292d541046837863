"""fast_runs_kernel at the edges of its LDS area.  The zero-run block of a frame (the control bytes of the svb stream: every run of
>= RMIN zero bytes is a sequence "first zero a literal, the rest copied from the byte in front") is placed 64 sequences a chunk
(zstd_runs.h, place_zero_runs): in LDS when 3 x lit_room + tt + 16 bytes fit the area (lit_room: the chunk's literals rounded up to 16,
tt: the bytes the chunk regenerates, the area: RUNS_LDS - 8 of zstd_decode_fast.hip), else straight to memory, with the chunk's
literals staged in LDS if they alone fit and from memory if not.  The sequences section is walked from the encoder's checkpoints
(one every 32 sequences, every 64 from 2 049 sequences on) when its bit stream fits RUNS_LDS - 16 bytes of LDS, serially otherwise and
when the frame has no checkpoint trailer.

The reads are built from their control bytes: in this codec (svb of int16, zig-zag deltas) FOUR samples make one control byte, two
bits each -- 0 for a delta of one data byte (|delta| < 128), 1 for two."""
import os
import re

import numpy as np
import pytest

import gpu_util as G
import oracle_lib as O
import typed_support as T
from vbz_compression_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constant(path, pattern):
    return int(re.search(pattern, open(os.path.join(ROOT, "vbz_compression_amd", "csrc", path)).read()).group(1))


RUNS_LDS = _constant("zstd_decode_fast.hip", r"#define VBZ_RUNS_LDS (\d+)")
RMIN = _constant("vbz_kernels.h", r"#define VBZ_RMIN (\d+)")
AREA = RUNS_LDS - 8        # place_zero_runs' lds_cap
STAGED = RUNS_LDS - 16     # zero_run_chain_segments' CAP: bytes of a sequences section's bit stream
PAD = 300   # literals behind a read's last sequence: from 256 literals on the block's literals are four streams, the batched decoder's shape
NONZERO = np.array([b for b in range(1, 256) if all(((b >> s) & 3) < 2 for s in (0, 2, 4, 6))], np.uint8)   # control bytes of codes 0 / 1

# What the batched own-frame decoder decoded of the 36 frames below on the parent of the change that introduced this test (its RUNS_LDS
# was 8 704 and a literal's shift a dword), with and without checkpoint trailers.  The nine it leaves to the one-wavefront decoder, then
# as now: the seven reads whose first block has fewer than 256 literals (one stream: literals1, literals1+tail, nseq1 / 63 / 64 / 65
# without padding) or raw literals (one_run), and the two reads at the staged capacity (more than 245 k samples: the treeless blocks
# of their data bytes have literals headers of five bytes, which its scan does not take).
PARENT_BATCHED = {"trailers": 27, "no_trailers": 27}


def control_bytes(rng, seqs, tail=0):
    """`seqs`: (nonzero literal bytes, zero bytes) per sequence -- literal length = the first + 1, match length = the second - 1"""
    parts = []
    for lits, run in seqs:
        parts.append(rng.choice(NONZERO, lits))
        parts.append(np.zeros(run, np.uint8))
    parts.append(rng.choice(NONZERO, tail))
    return np.concatenate(parts).astype(np.uint8)


def read_of(rng, ctl):
    """int16 samples whose svb stream begins with the control bytes `ctl`"""
    codes = ((ctl[:, None] >> np.array([0, 2, 4, 6])) & 3).reshape(-1)
    big = np.flatnonzero(codes)
    d = rng.integers(-3, 4, len(codes))
    d[big] = np.where(np.arange(len(big)) & 1, -300, 300)   # (alternating: the signal stays small)
    a = np.cumsum(d).astype(np.int16)
    assert O.svb_compress(a, 2, True)[: len(ctl)].tobytes() == ctl.tobytes()
    return a


def chunk_at_area(rng, delta, lits_first=1):
    """64 sequences whose 3 x lit_room + tt + 16 is AREA + delta, then five more and a tail of literals"""
    tl = 64 * 2 + (lits_first - 1)
    lit_room = (tl + 15) & ~15
    total_run = AREA + delta - 16 - 3 * lit_room - tl + 64     # tt = tl + sum(run - 1)
    base = total_run // 64
    seqs = [(lits_first if k == 0 else 1, base + (total_run - 64 * base if k == 63 else 0)) for k in range(64)]
    tt = sum(l + 1 + r - 1 for l, r in seqs)
    assert 3 * lit_room + tt + 16 == AREA + delta and sum(l + 1 for l, _ in seqs) == tl
    return control_bytes(rng, seqs + [(2, 20)] * 5, tail=PAD)


def sequences_section_bits(frame):
    """bytes of the first block's sequences bit stream (RFC 8878 3.1.1.3: behind the literals section, the sequence count, the modes byte
    and the offset table's one RLE byte)"""
    f = bytes(frame)
    pos = O.zstd_frame_geometry(f)[0]
    bsize = int.from_bytes(f[pos : pos + 3], "little") >> 3
    p = pos + 3
    assert f[p] & 3 == 2, "compressed literals"
    fmt = (f[p] >> 2) & 3
    lh, bits = ((3, 10), (3, 10), (4, 14), (5, 18))[fmt]
    csize = (int.from_bytes(f[p : p + lh], "little") >> (4 + bits)) & ((1 << bits) - 1)
    q = p + lh + csize
    nb = 1 if f[q] < 128 else (2 if f[q] < 255 else 3)
    assert f[q + nb] == 0x10, "LL / ML predefined, offsets RLE"
    return bsize - (q - p) - nb - 2


def make_reads():
    rng = np.random.default_rng(23)
    cases = []
    # the area's edge: the LDS path (16 below, exactly), the direct path with the chunk's literals staged (1 and 16 above); a literal
    # count that rounds up
    for delta in (-16, 0, 1, 16):
        cases.append(("area%+d" % delta, chunk_at_area(rng, delta)))
        cases.append(("area%+d/129" % delta, chunk_at_area(rng, delta, lits_first=2)))
    # the other direct path: a chunk's literals alone are more than the area; its runs cycle through the wave fill's edges
    runs = (RMIN, 63, 64, 65, 66, 130)
    cases.append(("literals>area", control_bytes(rng, [((AREA + 64) // 64 + 1, runs[k % len(runs)]) for k in range(70)], tail=3)))
    # the same runs in the LDS path, one below RMIN (no sequence), one whole control region
    cases.append(("runs", control_bytes(rng, [(1 + k % 3, r) for k, r in enumerate((RMIN - 1, RMIN, RMIN + 1, 63, 64, 65, 66) * 4)], tail=PAD)))
    cases.append(("one_run", np.zeros(5000, np.uint8)))
    # literals per chunk: none at all (no run: no sequence), 1, 15, 16, 17
    cases.append(("no_sequence", control_bytes(rng, [(9, RMIN - 1)] * 30)))
    for tl in (1, 15, 16, 17):
        cases.append(("literals%d" % tl, control_bytes(rng, [(tl - 1, 40)])))
        cases.append(("literals%d+tail" % tl, control_bytes(rng, [(tl - 1, 40)], tail=5)))
        cases.append(("literals%d+pad" % tl, control_bytes(rng, [(tl - 1, 40)], tail=PAD)))
    # sequences per read: around a chunk, and checkpoint spacing 32 and 64
    for nseq in (1, 63, 64, 65, 2048, 2049):
        cases.append(("nseq%d" % nseq, control_bytes(rng, [(1, RMIN + k % 3) for k in range(nseq)], tail=nseq % 4)))
        if nseq < 128:
            cases.append(("nseq%d+pad" % nseq, control_bytes(rng, [(1, RMIN + k % 3) for k in range(nseq)], tail=PAD)))
    return [(name, read_of(rng, ctl)) for name, ctl in cases]


def ladder_reads(bytes_per_seq):
    """two reads whose sequences sections stand on either side of the staged capacity: (1 literal, RMIN zeros) x nseq"""
    rng = np.random.default_rng(29)
    n0 = int(round(STAGED / bytes_per_seq))
    return [("staged%+d" % k, read_of(rng, control_bytes(rng, [(1, RMIN)] * (n0 + k)))) for k in (-40, 40)]


def roundtrip(c, named, what):
    """code and decode on the one-workgroup path; bytes and results; libzstd on every third frame; returns frames and decode_paths()"""
    saved = G.codec
    G.codec = lambda: c
    try:
        opts = _lib.CompressionOptions(True, 2, 1, 1)
        reads = [a for _, a in named]
        frames = G.compress(reads, opts)
        assert not any(isinstance(f, int) for f in frames), [(n, f) for (n, _), f in zip(named, frames) if isinstance(f, int)]
        back = G.decompress(frames, [a.nbytes for a in reads], opts)
        paths = c.decode_paths()
    finally:
        G.codec = saved
    print(what, "decode_paths", paths, "of", len(reads))
    for (name, a), b in zip(named, back):
        assert not isinstance(b, int), (name, b)
        assert len(b) == a.nbytes, (name, len(b), a.nbytes)
        assert b.tobytes() == a.tobytes(), name
    for (name, a), f in list(zip(named, frames))[::3]:
        svb = O.svb_compress(a, 2, True)
        assert O.zstd_decompress(f, len(svb)).tobytes() == svb.tobytes(), name
    return frames, paths


def test_zero_run_block_at_the_edges_of_its_lds_area():
    """Chunks of 64 sequences whose 3 x lit_room + tt + 16 is the area exactly, 16 below, 1 and 16 above (the LDS path and the direct
    path with staged literals), a chunk whose literals alone exceed the area (the other direct path); runs of RMIN - 1, RMIN, 63 .. 66
    bytes and of a whole control region; 0, 1, 15, 16, 17 literals in a chunk; reads of 1, 63, 64, 65, 2 048 and 2 049 sequences
    (checkpoint spacing 32 and 64), and all of it again without checkpoint trailers (VBZ_HIP_TRAILERS=0: fast_runs_kernel's serial
    zero_run_chain for every frame).  Two reads stand 50 bytes below and above the staged capacity (RUNS_LDS - 16 bytes of sequences
    bit stream).  A sequence of this encoder costs at least RMIN + 1 control bytes = 52 samples and 10 bits, so such a read has more
    than 255 k samples; at that length the batched decoder's scan leaves the frame to the one-wavefront decoder (see PARENT_BATCHED),
    whose staging area is its own: fast_runs_kernel never sees a section it cannot stage, and the two reads hold the bytes either way.
    VBZ_HIP_SEGMENTED=0 / VBZ_HIP_ROUTING=0 keep every read on the one-workgroup path whatever the batch's shape (a default context
    routes reads of 512 KB and more to the large-read path).  Decoded bytes and results are the input's, libzstd reads every third
    frame to the same svb stream, and the batched decoder decodes as many frames as it decoded on the parent."""
    named = make_reads()
    seen = {}
    for knob, trailers in (("trailers", 1), ("no_trailers", 0)):
        c = T.codec(VBZ_HIP_SEGMENTED=0, VBZ_HIP_ROUTING=0, VBZ_HIP_TRAILERS=trailers)
        # one probe for the ladder: bytes of bit stream per sequence of (1 literal, RMIN zeros)
        probe = ladder_reads(1.3)[:1]
        pf, _ = roundtrip(c, probe, knob + " probe")
        nprobe = int(round(STAGED / 1.3)) - 40
        ladder = ladder_reads(sequences_section_bits(pf[0]) / nprobe)
        frames, paths = roundtrip(c, named + ladder, knob)
        sizes = [sequences_section_bits(f) for f in frames[len(named):]]
        print(knob, "sequences sections of the ladder", sizes, "staged capacity", STAGED)
        assert min(sizes) <= STAGED < max(sizes), (sizes, STAGED)
        assert max(a.nbytes for _, a in ladder) < (1 << 20)
        assert paths[0] == len(named) + len(ladder)
        seen[knob] = paths[1]
    print("batched", seen)
    assert seen == PARENT_BATCHED, (seen, PARENT_BATCHED)

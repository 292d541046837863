"""Frames libzstd writes with blocks of other lengths than a one-shot ZSTD_compress gives (-m gpu).

A one-shot libzstd 1.4.8 frame has every block but the last exactly block_max = min(window, 128 KiB) long.  A writer that flushes
(ZSTD_compressStream2 with ZSTD_e_flush: streaming writers, libzstd >= 1.5 on its own) ends a block wherever it flushes, and a small
window (ZSTD_c_windowLog 10 .. 16) makes every block small.  The reference-frame path puts a block's literals ahead of the decoder at the
block's presumed end (zstd_decode_fast.hip: ref_lit_scan_kernel, ref_pieces_kernel) -- a guess that is wrong for a short non-last block,
whose literals then land inside a later block's range (oracle_lib.ref_literal_units; tests/test_oracle_zstd.py checks that the layouts
here really have such overlaps).  Every frame must decode bit for bit to its input on every decode path, and damaged frames must get
libzstd's verdict or a stricter one.  The frames come from oracle_lib.zstd_compress_cuts (libzstd itself)."""
import hashlib
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

B = O.BLOCK_MAX
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)


def _read(seed, svb_bytes):
    """an int16 read whose svb stream (zig-zag, version 1) is about svb_bytes long, and that stream"""
    a = O.synth_signal(5, seed, max(1, int(svb_bytes / 1.262)))
    return a, O.svb_compress(a, 2, True, 1)


def short_first_blocks():
    """(cuts, read, svb stream): the first block 2 .. 30 KiB short of 128 KiB, a last block of 15 .. 60 KiB"""
    rng = np.random.default_rng(71)
    out = []
    for i in range(6):
        short, last = int(rng.integers(2 << 10, 30 << 10)), int(rng.integers(15 << 10, 60 << 10))
        a, s = _read(1000 + i, B - short + last)
        out.append(([B - short], a, s))
    return out


def short_middle_blocks():
    """(cuts, read, svb stream): three or four blocks, a non-last one cut 2 .. 30 KiB short after a full one"""
    rng = np.random.default_rng(72)
    out = []
    for i in range(4):
        short, last = int(rng.integers(2 << 10, 30 << 10)), int(rng.integers(15 << 10, 60 << 10))
        if i % 2 == 0:   # B | B - short | last, or B | B - short | B | last
            a, s = _read(1100 + i, 2 * B - short + (i // 2) * B + last)
            out.append(([2 * B - short], a, s))
        else:            # B | B | B - short | last
            a, s = _read(1100 + i, 3 * B - short + last)
            out.append(([3 * B - short], a, s))
    return out


def layouts():
    """Every int16 frame of the module: (name, cuts, read, svb stream, level, window_log, checksum)"""
    rng = np.random.default_rng(73)
    L = []
    for k, (cuts, a, s) in enumerate(short_first_blocks()):
        L.append(("short_first", cuts, a, s, (1, 3, 9)[k % 3], 0, k % 3 == 1))
    for k, (cuts, a, s) in enumerate(short_middle_blocks()):
        L.append(("short_middle", cuts, a, s, (1, 3)[k % 2], 0, k == 2))
    for k, c in enumerate((1, 17, 4096)):   # a tiny first block, then full ones: every later non-last block's guess is wrong by c
        a, s = _read(1200 + k, c + 2 * B + int(rng.integers(20 << 10, 60 << 10)))
        L.append(("tiny_first", [c], a, s, (1, 3, 9)[k], 0, k == 0))
    for k, cuts in enumerate(([B], [B, 2 * B])):   # flushes where a one-shot frame ends its blocks anyway
        a, s = _read(1300 + k, 2 * B + int(rng.integers(20 << 10, 80 << 10)))
        L.append(("exact", cuts, a, s, 1, 0, False))
    for k, nb in enumerate((4, 5, 4, 5)):   # the walk's limit: REF_MAXBLK = REF_UNITS = 4 blocks
        shorts = sorted(int(x) for x in rng.integers(1 << 10, 40 << 10, nb - 1))   # (rising: no stretch between cuts exceeds 128 KiB)
        cuts = [(j + 1) * B - shorts[j] for j in range(nb - 1)]
        a, s = _read(1400 + k, cuts[-1] + int(rng.integers(15 << 10, 60 << 10)))
        L.append(("blocks%d" % nb, cuts, a, s, (1, 3)[k % 2], 0, k == 1))
    for k, w in enumerate((10, 12, 16, 17)):
        a, s = _read(1500 + k, 200000 + 30000 * k)
        L.append(("window%d" % w, [], a, s, (1, 3)[k % 2], w, k == 2))
    return L


def _wide():
    """int32 reads (svb 4-byte zig-zag, version 1) with a short first or middle block"""
    rng = np.random.default_rng(74)
    out = []
    for k in range(4):
        n = int(rng.integers(100000, 200000))
        a = (O.synth_signal(5, 1600 + k, n).astype(np.int32) * 3 - 7).astype(np.int32)
        s = O.svb_compress(a, 4, True, 1)
        cut = [B - int(rng.integers(2 << 10, 30 << 10))] if k % 2 == 0 else [2 * B - int(rng.integers(2 << 10, 30 << 10))]
        cut = [c for c in cut if c < len(s) - 4096]
        out.append((a, O.zstd_compress_cuts(s, cut, level=(1, 3)[k % 2], checksum=k == 3)))
    return out


def _plain():
    """plain contents through the zstd stage alone: text, svb streams, data with long matches"""
    rng = np.random.default_rng(75)
    srcs = [np.frombuffer((b"the quick brown fox jumps over the lazy dog %d " * 9000) % tuple(range(9000)), np.uint8)[:300000].copy()]
    for k in range(3):
        srcs.append(_read(1700 + k, 150000 + 70000 * k)[1])
    unit = rng.integers(0, 256, 3000, dtype=np.uint8)
    srcs.append(np.concatenate([rng.integers(0, 256, 1000, dtype=np.uint8), np.tile(unit, 80)]))
    out = []
    for k, c in enumerate(srcs):
        n = len(c)
        cuts = sorted(set(int(x) for x in rng.integers(1000, n - 1000, 1 + k % 3)))
        out.append((c, O.zstd_compress_cuts(c, cuts, level=(1, 3, 9)[k % 3], checksum=k % 2 == 1)))
        out.append((c, O.zstd_compress_cuts(c, [min(B, n // 2) - 5000], level=1)))
    return out


def _blocks(frame):
    """(header offset, type, size) of every block"""
    pos, _, _, _ = O.zstd_frame_geometry(frame)
    out = []
    while pos + 3 <= len(frame):
        bh = int.from_bytes(bytes(frame[pos : pos + 3]), "little")
        out.append((pos, (bh >> 1) & 3, bh >> 3))
        pos += 3 + (1 if (bh >> 1) & 3 == 1 else bh >> 3)
        if bh & 1:
            break
    return out


def _damaged(rng, frames):
    """(damaged frame, index of its source): bit flips in the frame and block headers and in the sequences sections (a block's last
    tenth) of flushed frames"""
    out = []
    for i, f in enumerate(frames):
        blocks = _blocks(f)
        hdr = O.zstd_frame_geometry(f)[0]
        for k in range(24):
            g = f.copy()
            if k % 4 == 0:
                g[int(rng.integers(4, hdr))] ^= 1 << int(rng.integers(0, 8))
            elif k % 4 == 1:
                p = blocks[int(rng.integers(0, len(blocks)))][0]
                g[p + int(rng.integers(0, 3))] ^= 1 << int(rng.integers(0, 8))
            else:
                p, t, sz = blocks[int(rng.integers(0, len(blocks)))]
                if t != 2:
                    continue
                for _ in range(int(rng.integers(1, 3))):
                    g[p + 3 + sz - 1 - int(rng.integers(0, max(1, sz // 10)))] ^= 1 << int(rng.integers(0, 8))
            out.append((g, i))
    return out


def _window_edits(frames):
    """(frame, must be refused): the window descriptor of frames that have one, shrunk below the block size (refused: a block larger
    than the window) or enlarged (decodes the same: the larger block_max makes every non-last block's guess wrong)"""
    out = []
    for f in frames:
        if f[4] & 0x20:
            continue
        for d in (-2, -1, 1, 3):
            g = f.copy()
            g[5] = (int(f[5]) + 8 * d) & 0xFF
            out.append((g, d < 0))
    return out


_CODE = r"""
import hashlib, os, sys, pickle
import numpy as np
import torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
import gpu_util as G
from vbz_compression_amd import _lib, batch
J = pickle.load(open(sys.argv[1], 'rb'))
out = {}
def b(v):
    return [o if isinstance(o, int) else o.tobytes() for o in v]
def rec(key, v):
    out[key] = b(v)
    out[key + '_paths'] = G.codec().decode_paths()
    out[key + '_ahead'] = G.codec().decode_literals_ahead()
o16 = _lib.CompressionOptions(True, 2, 1, 1)
# one frame a call: the units of one frame are the only workgroups of the pieces' kernel
for i in J['single']:
    rec('single%%d' %% i, G.decompress([J['f16'][i]], [J['n16'][i]], o16))
rec('i16', G.decompress(J['f16'], J['n16'], o16))
rec('i32', G.decompress(J['f32'], J['n32'], _lib.CompressionOptions(True, 4, 1, 1)))
rec('plain', G.zstd_decompress(J['plain'], J['plain_cap']))
rec('bad', G.zstd_decompress(J['bad'], J['bad_cap']))
rec('win', G.zstd_decompress(J['win'], J['win_cap']))
# a call large enough to walk by default: the reference's frames between this library's own of the same reads (digests: 1 GB of output)
own = G.compress(J['big_reads'], o16)
big, big_n = [], []
for k in range(J['big_count']):
    i = k %% len(own)
    big += [J['big_ref'][i], own[i]]
    big_n += [J['big_reads'][i].nbytes] * 2
rec('big', G.decompress(big, big_n, o16))
out['big'] = [o if isinstance(o, int) else hashlib.sha1(o).hexdigest() for o in out['big']]
# calibrated float32 straight from the walked frames
c = G.codec(); dev = c.device
arena, off, sizes = G._pack(J['f16'])
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
h = dst.cpu().numpy().view(np.uint8)
out['typed'] = [int(r) if r < 0 else h[o : o + int(r)].tobytes() for r, o in zip(res.cpu().tolist(), toff)]
pickle.dump(out, open(sys.argv[2], 'wb'))
""" % (ROOT, TESTS)

# the decode paths: (name, environment); VBZ_HIP_REF_UNITS=4 everywhere (blocks a frame whose literals may be decoded beside the walk)
PATHS = [("default", {}),
         ("walk_lds", dict(VBZ_HIP_REF_CHAINS="2", VBZ_HIP_REF_TABLES="lds", VBZ_HIP_REF_LITERALS="1")),
         ("walk_mem", dict(VBZ_HIP_REF_CHAINS="2", VBZ_HIP_REF_TABLES="mem", VBZ_HIP_REF_LITERALS="1")),
         ("walk_nolits", dict(VBZ_HIP_REF_CHAINS="2", VBZ_HIP_REF_TABLES="lds", VBZ_HIP_REF_LITERALS="0")),
         ("nowalk", dict(VBZ_HIP_REF_CHAINS="0", VBZ_HIP_REF_TABLES="lds", VBZ_HIP_REF_LITERALS="1"))]


def test_block_layouts_on_every_decode_path():
    """Every layout (short first, short middle and tiny first blocks; cuts at k x 128 KiB; four and five blocks; windows of 1, 4, 64 and
    128 KiB; levels 1, 3 and 9, some frames with checksums) as int16 svb frames -- one frame a call and all in one call --, int32 frames,
    plain contents through the zstd stage with slots of 2 x content + 256 KiB (the pieces' stripes need room behind the content), damaged
    frames, edited window descriptors, a call of 2 560 frames of both writers that walks by default (an average content above 96 KiB: 2 .. 4
    units a read) and one calibrated float32 call, on five paths: the defaults; walked with the tables in LDS, in memory, without the
    literals beside the walk; not walked.  Every path must give the same bytes and verdicts, the oracle's.

    What must have run (so that a change of routing cannot leave this test passing without exercising anything): on the walking paths
    at least every int16 layout frame with at most four blocks (REF_MAXBLK) is walked -- 19 of the 23; the first run walked 21 -- and
    at least those with a block of the unit's shape (oracle_lib.ref_literal_units: the same 19; the first run: 21) have literals decoded
    beside the walk, in the single-frame calls as in the batch; never on the paths without the walk or the literals.  The large call walks
    its 1 280 reference frames on the defaults too, with literals ahead for at least as many (first run: 2 085 of 2 560 frames, the own
    frames' included)."""
    if O.lib().vbo_zstd_version() is None:
        pytest.skip("no libzstd on this box")
    rng = np.random.default_rng(76)
    L = layouts()
    f16 = [O.zstd_compress_cuts(s, cuts, level=level, window_log=wlog, checksum=ck) for _, cuts, _, s, level, wlog, ck in L]
    reads = [a for _, _, a, *_ in L]
    n16 = [a.nbytes for a in reads]
    nblocks = [len(O.zstd_block_ends(f, len(s))) for f, (_, _, _, s, *_) in zip(f16, L)]
    # walked: at most four blocks (REF_MAXBLK); literals beside the walk: a block of the shape ref_literal_units restates
    walkable = [i for i in range(len(L)) if nblocks[i] <= 4]
    with_units = [i for i in walkable if O.ref_literal_units(f16[i])]
    overlapping = [i for i in walkable if O.overlapping_units(O.ref_literal_units(f16[i]))]
    assert len(walkable) >= 17 and len(with_units) >= 15 and len(overlapping) >= 10, (len(walkable), len(with_units), len(overlapping))
    wide = _wide()
    plain = _plain()
    bad_src = [O.zstd_compress_cuts(s, cuts, level=level) for (name, cuts, _, s, level, _, _) in L[:10]]
    damaged = _damaged(rng, bad_src)
    bad = [g for g, _ in damaged]
    bad_cap = [2 * O.zstd_content_size(bad_src[i]) + (256 << 10) for _, i in damaged]
    win_frames = [O.zstd_compress_cuts(s, [], level=1, window_log=w) for w, (_, _, _, s, *_) in zip((12, 16, 17, 16), L[-4:])]
    win = _window_edits(win_frames)
    assert len(win) == 16
    wcontent = [O.zstd_content_size(f) for f, _ in win]
    # the large call: 1 280 reference frames (the layouts of up to four blocks, over and over) between 1 280 of this library's own
    big_count = 1280
    big_want = [hashlib.sha1(reads[walkable[k % len(walkable)]].tobytes()).hexdigest() for k in range(big_count) for _ in (0, 1)]
    assert len(big_want) >= 2560 and sum(n16[i] for i in walkable) / len(walkable) > 96 << 10
    J = dict(f16=f16, n16=n16, single=list(range(len(f16))), f32=[f for _, f in wide], n32=[a.nbytes for a, _ in wide],
             plain=[f for _, f in plain], plain_cap=[2 * len(c) + (256 << 10) for c, _ in plain],
             bad=bad, bad_cap=bad_cap, win=[f for f, _ in win], win_cap=[2 * n + (256 << 10) for n in wcontent],
             big_ref=[f16[i] for i in walkable], big_reads=[reads[i] for i in walkable], big_count=big_count,
             scale=rng.uniform(0.05, 2.0, len(f16)).astype(np.float32), offset=rng.uniform(-50, 50, len(f16)).astype(np.float32))
    outs = {}
    with tempfile.TemporaryDirectory() as td:
        pickle.dump(J, open(os.path.join(td, "in.pkl"), "wb"))
        for name, extra in PATHS:
            env = {k: v for k, v in os.environ.items() if not k.startswith("VBZ_HIP_REF_")}
            env.update(VBZ_HIP_REF_UNITS="4", VBZ_HIP_SEGMENTED="0", VBZ_HIP_ROUTING="0", **extra)
            subprocess.run([sys.executable, "-c", _CODE, os.path.join(td, "in.pkl"), os.path.join(td, "out.pkl")], check=True, env=env, timeout=900)
            outs[name] = pickle.load(open(os.path.join(td, "out.pkl"), "rb"))
    ref = outs["walk_lds"]
    # 1. the same bytes and verdicts on every path
    keys = ["single%d" % i for i in range(len(f16))] + ["i16", "i32", "plain", "bad", "win", "big", "typed"]
    for name, o in outs.items():
        for k in keys:
            assert len(o[k]) == len(ref[k]), (name, k)
    # (every difference in one message: which layouts, which paths)
    diff = [(name, k, i) for name, o in outs.items() for k in keys for i, (a, b) in enumerate(zip(o[k], ref[k])) if a != b]
    assert not diff, diff[:40]
    # 2. ... and the oracle's
    wrong = [(i, L[i][0], L[i][1], k) for i, a in enumerate(reads) for k, g in (("i16", ref["i16"][i]), ("single", ref["single%d" % i][0]))
             if g != a.tobytes()]
    assert not wrong, wrong
    for (a, _), g in zip(wide, ref["i32"]):
        assert g == a.tobytes()
    for (c, _), g in zip(plain, ref["plain"]):
        assert g == c.tobytes()
    assert ref["big"] == big_want
    refused = 0
    for f, cap, g in zip(bad, J["bad_cap"], ref["bad"]):   # the device may refuse what libzstd lets through, never the other way round
        want = O.zstd_decompress(f, cap)
        if isinstance(g, int):
            refused += 1
        else:
            assert want is not None and g == want.tobytes()
    assert refused >= len(bad) // 4, (refused, len(bad))
    for (f, shrunk), cap, g in zip(win, J["win_cap"], ref["win"]):
        if shrunk:
            assert isinstance(g, int), "a block larger than the window was accepted"
        else:
            want = O.zstd_decompress(f, cap)
            assert want is not None and g == want.tobytes()
    for i, (a, g) in enumerate(zip(reads, ref["typed"])):
        want = (a.astype(np.float32) + J["offset"][i]) * J["scale"][i]
        assert g == want.tobytes(), (i, L[i][0])
    # 3. what ran
    nf, nw, nu = len(f16), len(walkable), len(with_units)
    print("layouts %d, walkable %d, with units %d, overlapping %d; " % (nf, nw, nu, len(overlapping)) + "; ".join(
        "%s: i16 %s ahead %d, singles walked %d ahead %d, typed %s, big %s ahead %d" % (
            name, o["i16_paths"], o["i16_ahead"], sum(o["single%d_paths" % i][2] for i in range(nf)), sum(o["single%d_ahead" % i] for i in range(nf)),
            o["typed_paths"], o["big_paths"], o["big_ahead"]) for name, o in outs.items()))
    for name in ("walk_lds", "walk_mem", "walk_nolits"):
        o = outs[name]
        assert o["i16_paths"][0] == nf and o["i16_paths"][2] >= nw, (name, o["i16_paths"])
        assert sum(o["single%d_paths" % i][2] for i in range(nf)) >= nw, name
        assert o["typed_paths"][2] >= nw, (name, o["typed_paths"])
    for name in ("walk_lds", "walk_mem"):
        o = outs[name]
        assert o["i16_ahead"] >= nu, (name, o["i16_ahead"])
        assert sum(o["single%d_ahead" % i] for i in range(nf)) >= nu, name
    for name in ("walk_nolits", "nowalk"):
        assert outs[name]["i16_ahead"] == 0 and outs[name]["big_ahead"] == 0, name
    assert outs["nowalk"]["i16_paths"][2] == 0 and outs["nowalk"]["big_paths"][2] == 0
    for name in ("default", "walk_lds", "walk_mem"):
        n, _, walked = outs[name]["big_paths"]
        assert n == 2 * big_count and walked >= big_count and outs[name]["big_ahead"] >= big_count * nu // nw, (name, outs[name]["big_paths"], outs[name]["big_ahead"])

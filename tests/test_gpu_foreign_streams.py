"""Every sink of the svb decoder on the MI355X over the streams of tests/foreign_streams.py (svb_store.h; svb_kernels.hip:
svb_decode_range, I16DecPairs::run): codes of 3 and 4 bytes in the reference's SIMD body and in its scalar tail, the pair loop handing a
read over to the tile loop at its first pair, in its steady state and at its last whole pair -- for a wide code, a stream shorter than
announced and a pair of more bytes than a stage buffer -- and reads of three segments with a wide code inside a carried delta total.
Level-0 frames make the svb stream the frame.  (a) the int16 decode gives the oracle's bytes or verdict for every row; (b) every typed
consumer runs through the runner its own test file uses, over reads that are foreign_streams.decode()'s int16 (held to the oracle by
tests/test_foreign_streams_ref.py), bit for bit and with those runners' canaries; error rows carry the int16 decode's verdict (their
output rows are the runners' `skip`: a stream found short while it was stored leaves them unspecified, every other row is checked).  (c) on
the default context, both forced paths, the large-read path with scan launches, a call cut in two, behind the entropy decoders, and
from source slots at alignment 1."""
import numpy as np
import pytest
import torch

import foreign_streams as F
import norm_ref as R
import oracle_lib as O
from events_support import EvRun
from segment_support import SegRun
from trim_support import TrimRun
from typed_support import NORMS, Frames, Run, arena, check_stats, codec, decode_both, u32
from windows_support import WinRun

pytestmark = pytest.mark.gpu

E_STREAM = 0xFFFFFFFB
L0, L1 = (True, 2, 0, 1), (True, 2, 1, 1)
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
PAD_CHUNKS = (1000, 776, "pad", 0)     # neither a multiple of a 16-byte line: lines put together from two lanes
END_CHUNKS = (2048, 1536, "end", 6)    # end_align no multiple of 8
WINDOW = 48

_cache = {}


class Case:
    """the catalogue once: rows, the oracle's answer and decode()'s reads (zeros for a row the oracle refuses), the error rows, and the
    tables the consumers are asked with"""

    def __init__(self, rows):
        self.rows, self.n = rows, len(rows)
        self.streams = [r.stream for r in rows]
        self.oracle = [O.decompress(r.stream, 2 * r.n, O.options(*L0)) for r in rows]
        got = [F.decode(r.stream, r.n) for r in rows]
        self.reads = [np.zeros(r.n, np.int16) if g is None else g[0] for r, g in zip(rows, got)]
        self.failed = {i for i, g in enumerate(got) if g is None}
        assert self.failed == {i for i, w in enumerate(self.oracle) if isinstance(w, int)} == {i for i, r in enumerate(rows) if "error" in r.tags}
        assert all(self.oracle[i] == E_STREAM for i in self.failed)
        self.expect = {i: E_STREAM for i in self.failed}
        rng = np.random.default_rng(71)
        self.offset = rng.uniform(-600.0, 600.0, self.n).astype(np.float32)
        self.scale = rng.uniform(0.01, 2.5, self.n).astype(np.float32)
        self.wide = [F.wide_values(r.stream, r.n) for r in rows]
        self.exit = [F.pair_exit(r.stream, r.n, 0) for r in rows]
        # where a row's output could go wrong: its wide values, the pair the loop stops in front of, the segment seams
        self.marks = [sorted({int(v) for v in self.wide[i]} | ({self.exit[i][0] * F.P} if self.exit[i] else set()) | set(range(F.SEG, r.n, F.SEG)))
                      for i, r in enumerate(rows)]
        # windows that straddle every mark, and a few across the read
        self.windows = [sorted({min(max(m - d, 0), r.n - 1) for m in self.marks[i] for d in (WINDOW - 1, WINDOW // 2, 1, 0)} | set(range(0, r.n, 2999)))
                        for i, r in enumerate(rows)]
        # events of dwell 2 ... 30 over the whole read
        self.events = []
        for r in rows:
            s = np.concatenate([[0], np.cumsum(rng.integers(2, 31, r.n // 2 + 1))])
            self.events.append(s[s < r.n].tolist())
        # ranged chunks: a begin behind the row's first wide code (else behind the first value of its exit pair, else of pair 1), a
        # multiple of 8 and an odd one
        behind = [int(w[0]) if len(w) else (e[0] * F.P if e else F.P) for w, e in zip(self.wide, self.exit)]
        self.begin_aligned = [min((b & ~7) + 8, r.n) for b, r in zip(behind, rows)]
        self.begin_odd = [min((b + 1) | 1, r.n) for b, r in zip(behind, rows)]

    def subset(self, keep):
        sub = Case.__new__(Case)
        sub.rows, sub.n = [self.rows[i] for i in keep], len(keep)
        for name in ("streams", "oracle", "reads", "wide", "exit", "marks", "windows", "events", "begin_aligned", "begin_odd"):
            setattr(sub, name, [getattr(self, name)[i] for i in keep])
        sub.offset, sub.scale = self.offset[keep], self.scale[keep]
        sub.failed = {j for j, i in enumerate(keep) if i in self.failed}
        sub.expect = {j: E_STREAM for j in sub.failed}
        return sub


def case():
    if "case" not in _cache:
        _cache["case"] = Case(F.catalogue(np.random.default_rng(61)))
    return _cache["case"]


def frames(c, k, wrap=None, lead=0, opts=L0):
    """the rows as a batch: every stream (wrap: what becomes of it) in a 64-byte aligned slot, `lead` bytes into it"""
    bufs = [np.concatenate([np.zeros(lead, np.uint8), s if wrap is None else wrap(s)]) for s in k.streams]
    src, off, size = arena(c, bufs, 64)
    return Frames(c, k.reads, c.options(*opts), comp=(src, off + lead, size - lead))


def good_frames(c, k, fr):
    """the rows the oracle decodes, in the same arena"""
    keep = [i for i in range(k.n) if i not in k.failed]
    idx = torch.tensor(keep, dtype=torch.int64, device=c.device)
    return Frames(c, [k.reads[i] for i in keep], fr.opts, comp=(fr.src, fr.off[idx].contiguous(), fr.size[idx].contiguous()))


def addr16(fr, i):
    return (fr.src.data_ptr() + int(fr.off[i])) % 16


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------------
def int16_decode(k, fr):
    c = fr.c
    dst = torch.zeros(fr.dst_bytes + 64, dtype=torch.uint8, device=c.device)
    res = torch.full((k.n,), -8, dtype=torch.int32, device=c.device)
    c.decompress(fr.src, fr.off, fr.size, dst, fr.doff, fr.dcap, res, fr.opts)
    torch.cuda.synchronize()
    res, host, doff = u32(res), dst.cpu().numpy(), fr.doff.tolist()
    for i, r in enumerate(k.rows):
        want = k.oracle[i]
        if isinstance(want, int):
            assert int(res[i]) == want, ("int16 decode", r.name, hex(int(res[i])), hex(want))
            continue
        assert int(res[i]) == 2 * r.n, ("int16 decode", r.name, hex(int(res[i])))
        got = host[doff[i] : doff[i] + 2 * r.n]
        assert got.tobytes() == want.tobytes(), ("int16 decode", r.name, "first wrong sample", int(np.argmax(got != want)) // 2, "wide", k.wide[i][:4].tolist(),
                                                 "exit", k.exit[i])


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------------
def signal(k, fr, signed=True):
    caps16 = [2 * r.n for r in k.rows]
    for name, dtype in DTYPES.items():
        for skew in (0, 1):   # skew 1: no typed slot starts on a 16-byte line, the tile loop alone runs the catalogue
            decode_both(fr.c, fr.src, fr.off, fr.size, caps16, fr.opts, False, dtype, offset=k.offset, scale=k.scale, signed=signed, skew=skew)


def chunks(k, fr, signed=True):
    Run(fr, PAD_CHUNKS, "f16", ranges=False, offset=k.offset, scale=k.scale, signed=signed).check(k.expect, skip=k.failed)
    Run(fr, END_CHUNKS, "bf16", ranges=False, offset=k.offset, scale=k.scale, signed=signed).check(k.expect, skip=k.failed)
    Run(fr, END_CHUNKS, "f32", ranges=False, signed=signed).check(k.expect, skip=k.failed)


def ranged_chunks(k, fr, signed=True):
    Run(fr, PAD_CHUNKS, "f32", begin=k.begin_aligned, offset=k.offset, scale=k.scale, signed=signed).check(k.expect, skip=k.failed)
    Run(fr, END_CHUNKS, "f16", begin=k.begin_odd, offset=k.offset, scale=k.scale, signed=signed).check(k.expect, skip=k.failed)


def normalised(k, fr, signed=True):
    good = good_frames(fr.c, k, fr)
    for method, p in (("med_mad", R.BONITO), ("quantile", R.DORADO)):
        Run(fr, PAD_CHUNKS, "f16", norm=NORMS[method], ranges=False, signed=signed).check(k.expect, skip=k.failed)
        check_stats(good, p, signed=signed)


def trim(k, fr, signed=True):
    TrimRun(fr, norm="med_mad", signed=signed).check(k.expect)


def windows(k, fr, signed=True):
    WinRun(fr, k.windows, WINDOW, "f16", offset=k.offset, scale=k.scale, signed=signed).check(k.expect, skip=k.failed)
    WinRun(fr, k.windows, WINDOW, "f32", signed=signed).check(k.expect, skip=k.failed)


def events(k, fr, signed=True):
    EvRun(fr, k.events, offset=k.offset, scale=k.scale, signed=signed, moments=True).check(k.expect, skip=k.failed)


def segment(k, fr, signed=True):
    SegRun(fr, signed=signed, failed=k.failed).check(k.expect)


CONSUMERS = [signal, chunks, ranged_chunks, normalised, trim, windows, events, segment]


def every_consumer(k, fr, signed=True):
    int16_decode(k, fr)
    for consumer in CONSUMERS:
        consumer(k, fr, signed)


def limit_rows(k, fr):
    """the row built to fit a stage buffer does, the row built one byte over does not, at the address its slot really has"""
    for i, r in enumerate(k.rows):
        if "limit" in r.tags:
            got = F.pair_exit(r.stream, r.n, addr16(fr, i))
            assert got == (None if "fits" in r.tags else (1, F.OVER)), (r.name, addr16(fr, i), got)


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------------
def test_default_context():
    k, c = case(), codec()
    fr = frames(c, k)
    limit_rows(k, fr)
    every_consumer(k, fr)


def test_one_wavefront_path():
    k, c = case(), codec(VBZ_HIP_SEGMENTED=0)
    fr = frames(c, k)
    limit_rows(k, fr)
    assert sum("limit" in r.tags for r in k.rows) == 2
    every_consumer(k, fr)


def test_large_read_path():
    k, c = case(), codec(VBZ_HIP_SEGMENTED=1)
    every_consumer(k, frames(c, k))


def test_large_read_path_with_scan_launches():
    k, c = case(), codec(VBZ_HIP_SEGMENTED=1, VBZ_HIP_SEG_SELF_MAX=0)
    every_consumer(k, frames(c, k))


def test_call_cut_in_two():
    """VBZ_HIP_SPLIT_MIN=8: the batch runs as two halves, and the wide-code and error rows lie in the upper one"""
    k, c = case(), codec(VBZ_HIP_SPLIT_MIN=8)
    assert any("wide" in r.tags for r in k.rows[k.n // 2 :]) and any(i >= k.n // 2 for i in k.failed)
    every_consumer(k, frames(c, k))


def test_behind_the_entropy_decoders():
    """the same streams as libzstd wraps them: the typed calls take them from where the entropy stage left them"""
    k, c = case(), codec()
    fr = frames(c, k, wrap=lambda s: O.zstd_compress(s, 1), opts=L1)
    k = k.subset(list(range(k.n)))
    k.oracle = [O.decompress(O.zstd_compress(s, 1), 2 * r.n, O.options(*L1)) for s, r in zip(k.streams, k.rows)]
    assert {i for i, w in enumerate(k.oracle) if isinstance(w, int)} == k.failed and all(k.oracle[i] == E_STREAM for i in k.failed)
    every_consumer(k, fr)


def test_source_slots_at_alignment_1():
    k, c = case(), codec()
    fr = frames(c, k, lead=1)
    assert all(addr16(fr, i) == 1 for i in range(k.n))
    every_consumer(k, fr)


def test_unsigned_samples():
    """a subset of the rows again as uint16 samples: every row with a wide code in the scalar tail, the defects, one row of every other kind"""
    k = case()
    keep = [i for i, r in enumerate(k.rows) if "last groups" in r.tags or "error" in r.tags or "random" in r.tags or "segments" in r.tags
            or "n - " in r.name or r.name in ("quiet 12T + 77", "border 6T + 3", "noise fills pair 1", "code 3 at value 2P + 3 of 12T + 77")]
    assert len(keep) >= 24, len(keep)
    sub = k.subset(keep)
    c = codec()
    fr = frames(c, sub)
    for consumer in CONSUMERS:
        consumer(sub, fr, signed=False)

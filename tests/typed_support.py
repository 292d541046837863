"""Batches, frames and C structs for the typed-decode tests on the MI355X (test_gpu_signal, _chunks, _norm, _pod5, _pod5_reads, _ranges,
_trim, _chunk_store, _typed_refusals; test_gpu_pack takes the codec): one definition of the codec cache, the table and arena helpers, the
two signal generators, the compress step, compressed reads with their int16 layout, the C-struct builders, and the raw chunk calls with
their checks against signal_ref / pod5_reads_ref / ranges_ref, the typed decode beside the int16 decode (decode_both) and the statistics
call's check (check_stats), which test_gpu_foreign_streams runs too.  A plain module (no assertion rewriting): every assert here carries its
operands.  Output types are signal_ref's strings; key() takes a torch dtype to them."""
import ctypes
import os

import numpy as np
import torch

import norm_ref as R
import pod5_ref as P
import pod5_reads_ref as PR
import ranges_ref as G
import signal_ref as SR
from signal_ref import is_nan_bits, typed_bits
from vbz_compression_amd import _lib, batch

CANARY = 0x5A
PAD = -7.0
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
ELEM = {"f32": 4, "f16": 2, "bf16": 2}
SIG = {"f32": _lib.VBZ_GPU_SIGNAL_F32, "f16": _lib.VBZ_GPU_SIGNAL_F16, "bf16": _lib.VBZ_GPU_SIGNAL_BF16}
NORMS = {"med_mad": (R.BONITO, batch.MED_MAD), "quantile": (R.DORADO, batch.DORADO_QUANTILE)}


def key(dtype):
    """the output type's string, of a torch dtype or of the string itself"""
    return dtype if isinstance(dtype, str) else {v: k for k, v in TORCH.items()}[dtype]


_codecs = {}


def codec(**env):
    """a codec whose context was created under the given VBZ_HIP_* knobs (read when the context is created); none: the default context"""
    k = tuple(sorted(env.items()))
    if k not in _codecs:
        old = {name: os.environ.get(name) for name in env}
        os.environ.update({name: str(v) for name, v in env.items()})
        try:
            _codecs[k] = batch.GpuCodec(0)
        finally:
            for name, v in old.items():
                if v is None:
                    os.environ.pop(name, None)
                else:
                    os.environ[name] = v
    return _codecs[k]


def i32(vals):
    return torch.tensor(np.asarray(vals, np.uint64).astype(np.uint32).view(np.int32), dtype=torch.int32)


def u32(t):
    return t.cpu().numpy().view(np.uint32).astype(np.uint64)


def arena(c, bufs, align):
    """host buffers -> (src, src_off, src_size) on the device"""
    sizes = [int(b.nbytes) for b in bufs]
    off, total = batch.layout(sizes, align)
    a = np.zeros(total + 64, np.uint8)
    for b, o in zip(bufs, off.tolist()):
        a[o : o + b.nbytes] = np.frombuffer(np.ascontiguousarray(b).tobytes(), np.uint8)
    return torch.from_numpy(a).to(c.device), off.to(c.device), i32(sizes).to(c.device)


class Stage:
    """what run_stage leaves: out (per read the result's bytes, or the error verdict), the destination arena on the host, the slots'
    offsets, and the extents the call declared (src_bytes, dst_bytes: what the library's shape rule sees)"""

    def __init__(self, out, host, off, src_bytes, dst_bytes):
        self.out, self.host, self.off, self.src_bytes, self.dst_bytes = out, host, off, src_bytes, dst_bytes


def run_stage(c, fn, bufs, caps, align=64, pad=32, fill=0):
    """gpu_util.run_stage on the codec c: fn(c, src, src_off, src_size, dst, dst_off, dst_cap, result) over host buffers, into slots of
    caps[i] + pad bytes at multiples of `align` in an arena filled with `fill` (align = 1, pad = 0: slots without gaps) -> Stage"""
    dev = c.device
    src, src_off, src_size = arena(c, bufs, 64)
    doff, dtotal = batch.layout([int(x) + pad for x in caps], align)
    dst = torch.full((dtotal + 64,), fill, dtype=torch.uint8, device=dev)
    result = torch.full((len(bufs),), -8, dtype=torch.int32, device=dev)
    fn(c, src, src_off, src_size, dst, doff.to(dev), i32(caps).to(dev), result)
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    out = []
    for r, o, cap in zip(u32(result).tolist(), doff.tolist(), caps):
        if _lib.is_error(int(r)):
            out.append(int(r))
        else:
            assert r <= cap, (r, cap)
            out.append(host[o : o + int(r)].copy())
    return Stage(out, host, doff.tolist(), int(src.numel()), int(dst.numel()))


# ---- signal -------------------------------------------------------------------------------------------------------------------------
def walk_signal(rng, T):
    """a slow random walk under noise, inside [80, 580]"""
    return np.clip(330 + np.cumsum(rng.normal(0, 3, T)) * 0.05 + rng.normal(0, 40, T), 80, 580).astype(np.int16)


def sine_signal(rng, T):
    """a sine of period 100 pi samples under noise, inside [-500, 900]"""
    return np.clip(330 + rng.normal(0, 40, T) + 60 * np.sin(np.arange(T) / 50.0), -500, 900).astype(np.int16)


# ---- frames -------------------------------------------------------------------------------------------------------------------------
def compress(c, reads, opts, sized=False, align=64, caps=None):
    """the library's frames of host reads -> (src, src_off, src_size) on the device; caps: other slot capacities than the size query's"""
    dev = c.device
    raw, off, size = arena(c, reads, align)
    if caps is None:
        caps = [c.L.vbz_max_compressed_size(int(a.nbytes), ctypes.byref(opts)) for a in reads]
    coff, ctotal = batch.layout(caps, align)
    comp = torch.zeros(ctotal + 64, dtype=torch.uint8, device=dev)
    res = torch.zeros(len(reads), dtype=torch.int32, device=dev)
    c.compress(raw, off, size, comp, coff.to(dev), i32(caps).to(dev), res, opts, sized=sized)
    torch.cuda.synchronize()
    bad = [(i, hex(int(r))) for i, r in enumerate(u32(res)) if _lib.is_error(int(r))]
    assert not bad, ("compress", bad[:4])
    return comp, coff.to(dev), res


def pod5_compress(c, rows, level=1):
    """the library's POD5 frames of host rows -> list of numpy frames"""
    comp, coff, res = compress(c, rows, batch.pod5_options(level), align=16, caps=[batch.pod5_max_compressed_size(len(x)) for x in rows])
    host = comp.cpu().numpy()
    return [host[o : o + int(r)].copy() for o, r in zip(coff.tolist(), u32(res))]


def device_frames(c, lens, seed, opts, sized=False):
    """the library's frames of device-synthesised signal (reads of `lens` samples) -> (src, src_off, src_size) on the device"""
    dev = c.device
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
    sizes = [2 * n for n in lens]
    off, total = batch.layout(sizes, 64)
    raw = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
    c.synth_signal(seed, 0, raw, off.to(dev), lens_t)
    caps = [c.L.vbz_max_compressed_size(s, ctypes.byref(opts)) for s in sizes]
    coff, ctotal = batch.layout(caps, 64)
    comp = torch.empty(ctotal + 64, dtype=torch.uint8, device=dev)
    res = torch.zeros(len(lens), dtype=torch.int32, device=dev)
    c.compress(raw, off.to(dev), i32(sizes).to(dev), comp, coff.to(dev), i32(caps).to(dev), res, opts, sized=sized)
    torch.cuda.synchronize()
    assert not any(_lib.is_error(r) for r in u32(res)), ("compress", [hex(int(r)) for r in u32(res) if _lib.is_error(r)][:4])
    return comp, coff.to(dev), res


class Frames:
    """reads (int16 bits) compressed once, and the int16 layout that describes them.  comp: (src, src_off, src_size) of frames made
    elsewhere; slack: bytes a sized read's capacity exceeds its header's size by; align / caps: compress()'s"""

    def __init__(self, c, reads, opts, sized=False, comp=None, slack=0, align=64, caps=None):
        self.c, self.reads, self.opts, self.sized, self.n = c, [np.asarray(x).view(np.int16) for x in reads], opts, sized, len(reads)
        self.src, self.off, self.size = compress(c, self.reads, opts, sized, align, caps) if comp is None else comp
        self.T = [len(x) for x in self.reads]
        caps16 = [2 * t + (slack if sized else 0) for t in self.T]
        doff, self.dst_bytes = batch.layout(caps16, 16)
        self.doff, self.dcap = doff.to(c.device), i32(caps16).to(c.device)


# the grouping shapes of POD5 reads: rows per read (sample counts)
SHAPES = [
    [1500],                                # one row: the row-wise call's chunks
    [2048, 100],
    [13, 7, 1, 2047, 2049],                # rows that begin inside a 16-byte line
    [800, 0, 800],                         # an empty row in the middle
    [1200, 0],                             # the last row is empty
    [],                                    # no rows
    [0, 0],                                # only empty rows
    [300] * 40,                            # a chunk spans more than 3 rows
    [4096, 4096, 5],
    [24, 8, 2056, 16],                     # every row begins at a multiple of 8: whole lines across rows
]


def make_rows(seed, shapes):
    """(rows, first_row) of reads with the given row lengths: signal-like int16, every third read full-range noise"""
    rng = np.random.default_rng(seed)
    rows, first = [], []
    for k, lens in enumerate(shapes):
        first.append(len(rows))
        for n in lens:
            rows.append(rng.integers(-32768, 32768, n).astype(np.int16) if k % 3 == 2 else sine_signal(rng, n))
    return rows, first


_frames = {}


def frames_of(seed, shapes):
    """the rows of make_rows as libzstd wrote them (pod5's frames), computed once"""
    k = (seed, repr(shapes))
    if k not in _frames:
        rows, first = make_rows(seed, shapes)
        _frames[k] = (rows, first, [P.compress_row(x) for x in rows])
    return _frames[k]


# ---- C structs ----------------------------------------------------------------------------------------------------------------------
def fmt(dtype, signed, offset=None, scale=None):
    """vbz_gpu_signal_format; offset / scale: float32 tables on the device (the caller keeps them alive)"""
    f = _lib.GpuSignalFormat()
    f.out_type, f.is_signed = SIG[key(dtype)], int(signed)
    if offset is not None:
        f.offset = offset.data_ptr()
    if scale is not None:
        f.scale = scale.data_ptr()
    return f


def ranges_struct(c, begin, end, stats=0, reserved=0):
    """(the C struct, its tables): begin / end per-read sequences, or None for a NULL table"""
    g = _lib.GpuSampleRanges()
    keep = []
    for name, t in (("begin", begin), ("end", end)):
        if t is not None:
            d = i32([int(v) & 0xFFFFFFFF for v in t]).to(c.device)
            keep.append(d)
            setattr(g, name, d.data_ptr())
    g.stats, g.reserved = stats, reserved
    return g, keep


def trim_struct(p, reserved=0):
    """the C struct of trim_ref's parameter tuple"""
    t = _lib.GpuTrim()
    t.window, t.min_elements, t.min_trim, t.max_samples, t.threshold_factor, t.max_fraction, t.flags = p
    t.reserved = reserved
    return t


def norm_of(p):
    """batch.Normalization of norm_ref's parameter tuple"""
    method = {R.MED_MAD: "med_mad", R.QUANTILE: "quantile"}[p[0]]
    return batch.Normalization(method, p[1], p[2], p[3], p[4], p[5], p[6])


def device_tables(c, f, offset, scale):
    """host offset / scale tables (or None) -> the device tensors behind f's pointers"""
    keep = []
    for name, t in (("offset", offset), ("scale", scale)):
        if t is not None:
            d = torch.from_numpy(np.asarray(t, np.float32)).to(c.device)
            keep.append(d)
            setattr(f, name, d.data_ptr())
    return keep


def full(vals, n):
    return [None] * n if vals is None else list(vals)


# ---- POD5 reads of several rows -------------------------------------------------------------------------------------------------------
class Call:
    """One raw vbz_gpu_pod5_* call over reads: the batch, the tables and canary-filled outputs, all kept alive on the object.  guard:
    canary chunk rows behind the arena's last row"""

    def __init__(self, c, frames, row_samples, table, dtype="f16", chunking=None, norm=None, offset=None, scale=None, chunk_first=None, signed=True,
                 guard=4):
        dev = c.device
        self.c, self.n, self.R, self.dtype, self.guard = c, len(frames), len(table) - 1, dtype, guard
        self.src, self.off, self.size = arena(c, frames, 16)
        caps = [2 * int(s) for s in row_samples]
        doff, self.total = batch.layout(caps, 16)
        self.doff, self.dcap = doff.to(dev), i32(caps).to(dev)
        self.result = torch.full((max(self.n, 1),), -8, dtype=torch.int32, device=dev)
        self.read_result = torch.full((max(self.R, 1),), -8, dtype=torch.int32, device=dev)
        self.table = i32(table).to(dev)
        self.reads = _lib.GpuPod5Reads()
        self.reads.n_reads, self.reads.first_row, self.reads.read_result = self.R, self.table.data_ptr(), self.read_result.data_ptr()
        self.b = c._batch(self.src, self.off, self.size, torch.empty(0, dtype=torch.uint8, device=dev), self.doff, self.dcap, self.result)
        self.b.dst, self.b.dst_bytes = None, self.total
        self.f = fmt(dtype, signed)
        self.keep = device_tables(c, self.f, offset, scale)
        self.m = norm.c_struct() if norm is not None else None
        self.ss = torch.full((max(self.R, 1), 2), -777.0, dtype=torch.float32, device=dev)
        self.opts = batch.pod5_options()
        self.ch = None
        if chunking is not None:
            L, S, mode, ea = chunking
            self.ch = c._chunking(L, S, mode, ea, PAD)
            T = [sum(int(s) for s in row_samples[table[k] : table[k + 1]]) if table[k] <= table[k + 1] <= self.n else 0 for k in range(self.R)]
            first = SR.table_of(T, L, S, mode, ea) if chunk_first is None else np.asarray(chunk_first, np.int64)
            self.first_host = first
            self.chunk_first = torch.from_numpy(first).to(dev)
            self.rows = int(max(first))
            self.chunks = torch.full(((self.rows + guard) * L * ELEM[dtype],), CANARY, dtype=torch.uint8, device=dev)

    def chunk_call(self):
        m = ctypes.byref(self.m) if self.m is not None else None
        rc = self.c.L.vbz_gpu_pod5_decompress_chunks_batch(self.c.ctx, ctypes.byref(self.b), ctypes.byref(self.opts), ctypes.byref(self.f), ctypes.byref(self.ch),
                                                           ctypes.byref(self.reads), self.chunk_first.data_ptr(), self.chunks.data_ptr(), self.rows, m,
                                                           self.ss.data_ptr() if self.m is not None else None)
        self.c.synchronize()
        return rc

    def stats_call(self, signed=True):
        rc = self.c.L.vbz_gpu_pod5_signal_norm_batch(self.c.ctx, ctypes.byref(self.b), ctypes.byref(self.opts), int(signed), ctypes.byref(self.reads),
                                                     ctypes.byref(self.m), self.ss.data_ptr())
        self.c.synchronize()
        return rc

    def chunk_bits(self):
        L = self.ch.chunk_len
        host = self.chunks.cpu().numpy()
        return host.view(np.uint32 if self.dtype == "f32" else np.uint16).reshape(self.rows + self.guard, L)


def check_chunks(call, rows, first, chunking, consts, skip=()):
    """every read's chunk rows against the reference, the canary behind the arena; consts[k] = (offset, scale) of read k"""
    L, S, mode, ea = chunking
    got = call.chunk_bits()
    sig = PR.read_signals(rows, first)
    cf = call.first_host
    for k, x in enumerate(sig):
        if k in skip:
            continue
        starts, want = SR.chunk_rows(x, L, S, mode, ea, consts[k][0], consts[k][1], PAD, call.dtype)
        assert cf[k + 1] - cf[k] == len(starts), ("rows of read", k, int(cf[k + 1] - cf[k]), len(starts))
        bad = np.argwhere(got[cf[k] : cf[k + 1]] != want)
        assert bad.size == 0, (chunking, call.dtype, "read", k, "chunk, position", bad[:4].tolist())
    assert (call.chunks.cpu().numpy()[call.rows * L * ELEM[call.dtype] :] == CANARY).all(), "rows behind chunk_first[n] were written"


def expect_results(call, rows, first, E):
    b = PR.bounds(first, len(rows))
    got, want = u32(call.result)[: call.n].tolist(), [E * len(x) for x in rows]
    assert got == want, ("result", [(i, hex(g), hex(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w][:4])
    got, want = u32(call.read_result)[: call.R].tolist(), [E * sum(len(x) for x in rows[b[k] : b[k + 1]]) for k in range(call.R)]
    assert got == want, ("read_result", [(k, hex(g), hex(w)) for k, (g, w) in enumerate(zip(got, want)) if g != w][:4])


def unranged_results(c, frames, rows, first, chunking=None, norm=None):
    """(result, read_result) of the call without ranges over the same rows"""
    call = Call(c, frames, [len(x) for x in rows], PR.bounds(first, len(rows)), "f16", chunking, norm=norm)
    rc = call.chunk_call() if chunking is not None else call.stats_call()
    assert rc == 0, (rc, c.L.vbz_gpu_last_error(c.ctx))
    return u32(call.result)[: call.n].tolist(), u32(call.read_result)[: call.R].tolist()


# ---- reads with ranges ------------------------------------------------------------------------------------------------------------------
class Run:
    """one raw vbz_gpu_decompress_chunks_range_batch call into a canary arena, and its check against ranges_ref.  guard: canary rows
    behind the arena's last row"""

    def __init__(self, fr, chunking, dtype="f16", begin=None, end=None, norm=None, stats=0, signed=True, offset=None, scale=None, chunk_first=None,
                 ranges=True, src=None, guard=3):
        c = fr.c
        self.fr, self.chunking, self.dtype, self.begin, self.end, self.norm, self.stats, self.signed = fr, chunking, dtype, begin, end, norm, stats, signed
        self.guard = guard
        L, S, mode, ea = chunking
        n, dev = fr.n, c.device
        self.bg, self.en = full(begin, n), full(end, n)
        self.Tp = [G.clamp(fr.T[i], self.bg[i], self.en[i]) for i in range(n)]
        self.table = SR.table_of([e - b for b, e in self.Tp], L, S, mode, ea) if chunk_first is None else np.asarray(chunk_first, np.int64)
        self.rows = int(self.table[-1]) if chunk_first is None else int(max(self.table))
        self.chunks = torch.full(((self.rows + guard) * L * ELEM[dtype],), CANARY, dtype=torch.uint8, device=dev)
        self.first_d = torch.from_numpy(self.table).to(dev)
        self.result = torch.full((max(n, 1),), -8, dtype=torch.int32, device=dev)
        self.ss = torch.full((max(n, 1), 2), -777.0, dtype=torch.float32, device=dev)
        self.o = np.zeros(n, np.float32) if offset is None else np.asarray(offset, np.float32)
        self.s = np.ones(n, np.float32) if scale is None else np.asarray(scale, np.float32)
        f = fmt(dtype, signed)
        self.keep = device_tables(c, f, offset, scale)
        b = c._batch(fr.src if src is None else src, fr.off, fr.size, torch.empty(0, dtype=torch.uint8, device=dev), fr.doff, fr.dcap, self.result)
        b.dst, b.dst_bytes = None, fr.dst_bytes
        ch = c._chunking(L, S, mode, ea, PAD)
        m = norm[1].c_struct() if norm is not None else None
        g, keep = ranges_struct(c, begin, end, stats)
        self.keep += keep
        torch.cuda.synchronize()
        self.rc = c.L.vbz_gpu_decompress_chunks_range_batch(c.ctx, ctypes.byref(b), ctypes.byref(fr.opts), int(fr.sized), ctypes.byref(f), ctypes.byref(ch),
                                                            self.first_d.data_ptr(), self.chunks.data_ptr(), self.rows,
                                                            ctypes.byref(m) if m is not None else None, self.ss.data_ptr() if m is not None else None,
                                                            ctypes.byref(g) if ranges else None)
        c.synchronize()
        self.err = c.L.vbz_gpu_last_error(c.ctx)

    def bits(self):
        L = self.chunking[0]
        return self.chunks.cpu().numpy().view(np.uint32 if self.dtype == "f32" else np.uint16).reshape(self.rows + self.guard, L)

    def values(self, i):
        x = self.fr.reads[i]
        return x if self.signed else x.view(np.uint16)

    def check(self, expect=None, skip=()):
        """verdicts (expect[i]: another verdict than T x E), every read's rows and constants, the canary everywhere else"""
        assert self.rc == 0, self.err
        fr = self.fr
        L, S, mode, ea = self.chunking
        E = ELEM[self.dtype]
        res = u32(self.result)
        got = self.bits()
        ss = self.ss.cpu().numpy()
        owned = np.zeros(self.rows + self.guard, bool)
        for i in range(fr.n):
            want_res = fr.T[i] * E if not (expect and i in expect) else expect[i]
            assert int(res[i]) == want_res, (i, hex(int(res[i])), hex(want_res))
            if _lib.is_error(want_res) or i in skip:
                if i in skip:   # (rows left unspecified: a stream that failed while it was stored)
                    owned[self.table[i] : self.table[i + 1]] = True
                continue
            x = self.values(i)
            if self.norm is not None:
                starts, want, shift, scale = G.norm_chunk_rows(x, self.bg[i], self.en[i], L, S, mode, ea, self.norm[0], self.stats, PAD, self.dtype)
                assert (ss[i][0].view(np.uint32), ss[i][1].view(np.uint32)) == (shift.view(np.uint32), scale.view(np.uint32)), (
                    "shift_scale", i, fr.T[i], self.bg[i], self.en[i], ss[i], shift, scale)
            else:
                starts, want = G.chunk_rows(x, self.bg[i], self.en[i], L, S, mode, ea, self.o[i], self.s[i], PAD, self.dtype)
            lo, hi = int(self.table[i]), int(self.table[i + 1])
            assert hi - lo == len(starts), (i, lo, hi, len(starts))
            bad = np.argwhere(got[lo:hi] != want)
            assert bad.size == 0, (self.chunking, self.dtype, "read", i, "T", fr.T[i], "range", self.bg[i], self.en[i], "chunk, position", bad[:4].tolist())
            owned[lo:hi] = True
        assert (got[~owned].view(np.uint8) == CANARY).all(), "a chunk row outside the reads' rows was written"
        return self


# ---- the typed decode beside the int16 decode ---------------------------------------------------------------------------------------
def decode_both(c, src, src_off, src_size, caps16, opts, sized, dtype, offset=None, scale=None, signed=True, skew=0, typed_cap=None,
                typed_off=None, expect=None, after_typed=None):
    """The batch decoded twice: typed (dtype), then int16 with the capacities caps16.  typed_cap / typed_off (bytes; default: caps16 / 2 * E
    in a layout E / 2 times the int16 one, `skew` elements further on) may break the E-alignment rule; expect[i] overrides the expected
    typed verdict.  Checks every verdict, every sample, and the canary around and between the typed slots.  Returns the typed results."""
    dev = c.device
    n = len(caps16)
    dt = key(dtype)
    E = ELEM[dt]
    off16, tot16 = batch.layout([int(x) + 32 for x in caps16], 64)
    off16 = off16.tolist()
    tcap = [int(x) // 2 * E for x in caps16] if typed_cap is None else [int(x) for x in typed_cap]
    toff = [o * E // 2 + skew * E for o in off16] if typed_off is None else [int(x) for x in typed_off]
    tbytes = (max([o + cp for o, cp in zip(toff, tcap)] + [0]) + 64 + 15) // 16 * 16
    tarena = torch.full((tbytes,), CANARY, dtype=torch.uint8, device=dev)
    tres = torch.full((n,), -8, dtype=torch.int32, device=dev)
    kw = {}
    if offset is not None:
        kw["offset"] = torch.from_numpy(np.asarray(offset, np.float32)).to(dev)
    if scale is not None:
        kw["scale"] = torch.from_numpy(np.asarray(scale, np.float32)).to(dev)
    c.decompress_signal(src, src_off, src_size, tarena.view(dtype), torch.tensor(toff, dtype=torch.int64, device=dev), i32(tcap).to(dev), tres, opts,
                        signed=signed, sized=sized, **kw)
    if after_typed:
        after_typed()
    raw = torch.zeros(tot16 + 64, dtype=torch.uint8, device=dev)
    res16 = torch.full((n,), -8, dtype=torch.int32, device=dev)
    c.decompress(src, src_off, src_size, raw, torch.tensor(off16, dtype=torch.int64, device=dev), i32(caps16).to(dev), res16, opts, sized=sized)
    torch.cuda.synchronize()
    r16, rt = u32(res16), u32(tres)
    raw_h = raw.cpu().numpy()
    t_h = tarena.cpu().numpy()
    o_all = np.zeros(n, np.float32) if offset is None else np.asarray(offset, np.float32)
    s_all = np.ones(n, np.float32) if scale is None else np.asarray(scale, np.float32)
    written = np.zeros(tbytes, bool)
    for i in range(n):
        want = int(r16[i]) if _lib.is_error(int(r16[i])) else int(r16[i]) // 2 * E
        if expect and i in expect:
            want = expect[i]
        assert int(rt[i]) == want, (i, hex(int(rt[i])), hex(want), hex(int(r16[i])))
        written[toff[i] : toff[i] + tcap[i]] = True
        if _lib.is_error(want):
            if expect and i in expect:   # (a slot refused by the alignment rule is never written)
                assert (t_h[toff[i] : toff[i] + tcap[i]] == CANARY).all(), i
            continue
        k = want // E
        x16 = raw_h[off16[i] : off16[i] + 2 * k].view(np.int16 if signed else np.uint16)
        ref = typed_bits(x16, o_all[i], s_all[i], dt)
        got = t_h[toff[i] : toff[i] + k * E].view(ref.dtype)
        nan = is_nan_bits(ref, dt)
        assert np.array_equal(got[~nan], ref[~nan]), (i, int(np.argmax(got != ref)))
        assert is_nan_bits(got[nan], dt).all(), i
    assert (t_h[~written] == CANARY).all(), "a byte outside every slot was written"
    return rt


# ---- the statistics call ------------------------------------------------------------------------------------------------------------
def int16(case):
    c = case.c
    dst = torch.zeros(case.dst_bytes + 64, dtype=torch.uint8, device=c.device)
    res = torch.zeros(case.n, dtype=torch.int32, device=c.device)
    c.decompress(case.src, case.off, case.size, dst, case.doff, case.dcap, res, case.opts, sized=case.sized)
    torch.cuda.synchronize()
    return u32(res)


def stats(case, p, signed=True):
    c = case.c
    res = torch.full((case.n,), -1, dtype=torch.int32, device=c.device)
    ss = c.signal_norm(case.src, case.off, case.size, case.doff, case.dcap, res, case.opts, norm_of(p), signed=signed, sized=case.sized)
    torch.cuda.synchronize()
    return ss.cpu().numpy(), u32(res)


def check_stats(case, p, signed=True):
    ss, res = stats(case, p, signed)
    assert (res == int16(case)).all()
    for i, x in enumerate(case.reads):
        x = x if signed else x.view(np.uint16)
        assert res[i] == 2 * len(x), (i, res[i])
        shift, scale = R.shift_scale(x, p)
        got = ss[i]
        assert got[0].view(np.uint32) == shift.view(np.uint32) and got[1].view(np.uint32) == scale.view(np.uint32), (
            i, len(x), p, got, shift, scale)
    return ss, res

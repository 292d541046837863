"""Batched, device-resident codec: torch tensors in HBM -> vbz_gpu_*_batch (include/vbz_gpu.h).

PyTorch is plumbing here (device memory, streams, torch.distributed); the codec itself is the HIP
library.  All tensors must live on the codec's device.  Offsets are int64, sizes/results int32
tensors whose bits are read as uint64 / uint32 by the C ABI.
"""
import collections
import ctypes
import dataclasses

import torch

from . import _lib

FLT_MIN = 1.1754943508222875e-38   # the smallest normal float32


def ptr(t):
    """a tensor's address, NULL for None"""
    return t.data_ptr() if t is not None else None


def ref(s):
    """a C struct by reference, NULL for None"""
    return ctypes.byref(s) if s is not None else None


def table(name, t, dtype, device=None, shape=None, numel=None, at_least=None, none=False):
    """What a device table must be, stated once -> t: of `dtype`, contiguous, on `device` (None: wherever it is) and, where a rule is given,
    of `shape` (a None entry: any extent), of exactly `numel` entries or of `at_least` entries.  none: None passes, as the C entry's NULL."""
    if t is None:
        assert none, "%s is required" % name
        return None
    ok = t.dtype == dtype and t.is_contiguous() and (device is None or t.device == device)
    if ok and shape is not None:
        ok = t.dim() == len(shape) and all(w is None or int(s) == w for s, w in zip(t.shape, shape))
    if ok and numel is not None:
        ok = int(t.numel()) == numel
    if ok and at_least is not None:
        ok = int(t.numel()) >= at_least
    assert ok, (name, t.dtype, tuple(t.shape), str(t.device))
    return t


def output(name, t, dtype, device, shape, three_state=False, at_least=False):
    """An output the caller may give -> the tensor: None allocates torch.empty(shape, dtype, device); a given tensor must be a table of that
    dtype and shape (shape an int: of that many entries, or with at_least of no fewer) and comes back as it is.  three_state: True
    allocates, False or None means not wanted (-> None), a tensor is checked."""
    if three_state:
        if t is None or t is False:
            return None
        t = None if t is True else t
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if isinstance(shape, int):
        return table(name, t, dtype, device, at_least=shape) if at_least else table(name, t, dtype, device, numel=shape)
    return table(name, t, dtype, device, shape=shape)


def wrap_u32(t):
    """values 0 ... 0xFFFFFFFF (a tensor or a sequence) as an int32 tensor of the same 32 bits; an int32 tensor as it is"""
    if isinstance(t, torch.Tensor) and t.dtype == torch.int32:
        return t
    w = torch.as_tensor(t, dtype=torch.int64).reshape(-1)
    return torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32)


@dataclasses.dataclass(frozen=True)
class Normalization:
    """Per-read normalisation from the read's own statistics (include/vbz_gpu.h: vbz_gpu_normalization): method "med_mad" (c = median,
    w = MAD) or "quantile" (c = Q(a) + Q(b), w = Q(b) - Q(a)); shift = max(shift_min, shift_mul c), scale = max(scale_min, scale_mul w),
    and a sample becomes (x - shift) * float32(1 / scale)."""

    method: str
    quantile_a: float = 0.0
    quantile_b: float = 0.0
    shift_mul: float = 1.0
    scale_mul: float = 1.0
    shift_min: float = float("-inf")
    scale_min: float = FLT_MIN

    _METHODS = {"med_mad": _lib.VBZ_GPU_NORM_MED_MAD, "quantile": _lib.VBZ_GPU_NORM_QUANTILE}

    def c_struct(self):
        m = _lib.GpuNormalization()
        m.method = self._METHODS.get(self.method, 0xFFFFFFFF)
        m.quantile_a, m.quantile_b = self.quantile_a, self.quantile_b
        m.shift_mul, m.scale_mul, m.shift_min, m.scale_min = self.shift_mul, self.scale_mul, self.shift_min, self.scale_min
        return m


MED_MAD = Normalization("med_mad", scale_mul=1.4826)                                  # Bonito / Remora: (x - med) / (1.4826 MAD)
DORADO_QUANTILE = Normalization("quantile", 0.2, 0.9, 0.51, 0.53, 10.0, 1.0)          # Dorado: q20 / q90


@dataclasses.dataclass(frozen=True)
class Trim:
    """Where a read's signal proper begins (include/vbz_gpu.h: vbz_gpu_trim): a sample is high above shift + threshold_factor * scale;
    the first window of `window` samples behind min_trim with more than min_elements high samples opens the peak, the first window at
    or behind it whose last sample is not high ends it, and that window's end is the trim -- min_trim when there is none in the first
    max_samples samples, when it lies beyond max_fraction of the read, or (reject_at_end) when its window is the last one looked at.
    The defaults are the shape of the trim Bonito and Dorado apply."""

    window: int = 40
    min_elements: int = 3
    min_trim: int = 10
    max_samples: int = 8000
    threshold_factor: float = 2.4
    max_fraction: float = 1.0
    reject_at_end: bool = False

    def c_struct(self):
        t = _lib.GpuTrim()
        t.window, t.min_elements, t.min_trim, t.max_samples = self.window, self.min_elements, self.min_trim, self.max_samples
        t.threshold_factor, t.max_fraction = self.threshold_factor, self.max_fraction
        t.flags = _lib.VBZ_GPU_TRIM_REJECT_AT_END if self.reject_at_end else 0
        return t


@dataclasses.dataclass(frozen=True)
class Segmentation:
    """How a read's signal is cut into events (include/vbz_gpu.h: vbz_gpu_segmentation): two two-window t-statistic detectors -- windows
    short_window and long_window (0: no second detector), thresholds on the t-statistic itself -- and a local non-maximum suppression of
    radius `radius`: a position is a boundary when its score (the larger squared t over its threshold's square) is at least 1, larger
    than every score up to `radius` positions in front of it and no smaller than every score up to `radius` behind it."""

    short_window: int = 3
    long_window: int = 6
    short_threshold: float = 4.0
    long_threshold: float = 9.0
    radius: int = 2

    def c_struct(self, start_cap=0):
        g = _lib.GpuSegmentation()
        g.short_window, g.long_window, g.radius = self.short_window, self.long_window, self.radius
        g.short_threshold, g.long_threshold = self.short_threshold, self.long_threshold
        g.start_cap = int(start_cap)
        return g

    def max_rows(self, samples):
        """the bound on a read's rows: 2 + T' / (radius + 1)"""
        return 2 + int(samples) // (self.radius + 1)


@dataclasses.dataclass(frozen=True)
class Spans:
    """Where a read's signal lies above or below a level (include/vbz_gpu.h: vbz_gpu_spans): a sample is in when it is above
    (direction "above") or below ("below") thr = a + threshold_factor * w -- {a, w} the read's {shift, scale} of a normalisation, or
    given per read -- and lies at or behind ignore_prefix; in-positions at most merge_gap apart form one span, and spans shorter than
    min_length are dropped."""

    direction: str = "above"
    merge_gap: int = 0
    min_length: int = 1
    ignore_prefix: int = 0
    threshold_factor: float = 0.0

    _DIRECTIONS = {"above": _lib.VBZ_GPU_SPAN_ABOVE, "below": _lib.VBZ_GPU_SPAN_BELOW}

    def c_struct(self, edge_cap=0, level=None):
        g = _lib.GpuSpans()
        g.direction = self._DIRECTIONS.get(self.direction, 0xFFFFFFFF)
        g.merge_gap, g.min_length, g.ignore_prefix = self.merge_gap, self.min_length, self.ignore_prefix
        g.threshold_factor = self.threshold_factor
        g.level = level
        g.edge_cap = int(edge_cap)
        return g

    def max_edges(self, samples):
        """the bound on a read's entries of edge: two per span, spans <= (T' + D + 1) / (m + D + 1)"""
        return 2 * ((int(samples) + self.merge_gap + 1) // (self.min_length + self.merge_gap + 1))


@dataclasses.dataclass(frozen=True)
class Match:
    """How reads are matched against reference squiggles (include/vbz_gpu.h: vbz_gpu_match): the query is the first query_len samples of
    a read's converted signal, quantised to int8 levels as clamp(rint(z * quant), -127, 127) (quantize_levels); every reference row is
    aligned whole to a stretch of it by subsequence DTW under |r - k|, and a hit is (cost, end)."""

    query_len: int = 2048
    quant: float = 32.0

    def c_struct(self, ref, ref_len):
        """ref: int8 [R, ref_stride] on the device; ref_len: int32 [R] on the device (uint32 bits)"""
        table("ref", ref, torch.int8, shape=(None, None))
        table("ref_len", ref_len, torch.int32, ref.device, numel=int(ref.shape[0]))
        g = _lib.GpuMatch()
        g.query_len, g.n_refs, g.ref_stride = int(self.query_len), int(ref.shape[0]), int(ref.shape[1])
        g.quant = self.quant
        g.ref, g.ref_len = ref.data_ptr(), ref_len.data_ptr()
        return g


@dataclasses.dataclass(frozen=True)
class Locate:
    """How reads are located in long target squiggles (include/vbz_gpu.h: vbz_gpu_locate): the query is the first query_len (<= 2048)
    samples of a read's converted signal, quantised as Match quantises them; the WHOLE query is aligned to a stretch of every target row
    by subsequence DTW under |k - g|, and a hit is (cost, end), end in target coordinates."""

    query_len: int = 2048
    quant: float = 32.0

    def c_struct(self, target, target_len):
        """target: int8 [G, target_stride] on the device; target_len: int32 [G] on the device (uint32 bits)"""
        table("target", target, torch.int8, shape=(None, None))
        table("target_len", target_len, torch.int32, target.device, numel=int(target.shape[0]))
        g = _lib.GpuLocate()
        g.query_len, g.n_targets, g.target_stride = int(self.query_len), int(target.shape[0]), int(target.shape[1])
        g.quant = self.quant
        g.target, g.target_len = target.data_ptr(), target_len.data_ptr()
        return g


def quantize_levels(values, quant):
    """The match calls' quantisation in numpy (include/vbz_gpu.h: vbz_gpu_match): float32 v = float32(values) * float32(quant), one
    multiply; 0 for NaN, else clamp(rint(v), -127, 127) with rint to nearest even -> int8.  A caller builds `ref` with it."""
    import numpy as np

    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(values, dtype=np.float32) * np.float32(quant)
        k = np.clip(np.rint(v), np.float32(-127), np.float32(127))
    return np.where(np.isnan(v), np.float32(0), k).astype(np.int8)


def _u32(t):
    """view an int32 result tensor as python ints in [0, 2**32)"""
    return [int(x) & 0xFFFFFFFF for x in t.tolist()]


class GpuCodec:
    """One context on one GPU.  The codec owns a torch stream (`self.stream`) and the C library
    launches every kernel on it; each call first makes that stream wait for torch's current stream
    and afterwards makes the current stream wait for the codec, so tensors produced or consumed by
    ordinary torch code need no extra synchronisation.  Under `with torch.cuda.stream(codec.stream)`
    both waits are no-ops."""

    def __init__(self, device=None):
        self.L = _lib.load()
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        with torch.cuda.device(self.device):
            self.stream = torch.cuda.Stream(self.device)
            self.ctx = self.L.vbz_gpu_create(self.device.index, ctypes.c_void_p(self.stream.cuda_stream))
        if not self.ctx:
            raise RuntimeError("vbz_gpu_create failed: no usable gfx950 device (the codec has no CPU path)")

    def _enter(self):
        cur = torch.cuda.current_stream(self.device)
        if cur != self.stream:
            self.stream.wait_stream(cur)
        return cur

    def _exit(self, cur):
        if cur != self.stream:
            cur.wait_stream(self.stream)

    def set_trailers(self, enable):
        """Decoder hints (checkpoints, span index) in skippable frames behind the zstd frame: on by default (include/vbz_gpu.h)."""
        self.L.vbz_gpu_set_trailers(self.ctx, int(bool(enable)))

    def set_canonical(self, enable):
        """A read's compressed bytes depend on the read, the options and the library version only -- not on the batch it arrives in
        (include/vbz_gpu.h: vbz_gpu_set_canonical)."""
        self.L.vbz_gpu_set_canonical(self.ctx, int(bool(enable)))

    def set_checksum(self, enable):
        """Write every zstd frame with its content checksum (XXH64 of the svb stream), which every zstd decoder verifies: off by default
        (include/vbz_gpu.h: vbz_gpu_set_checksum).  Decoding always verifies checksums that frames carry."""
        self.L.vbz_gpu_set_checksum(self.ctx, int(bool(enable)))

    def close(self):
        if getattr(self, "ctx", None):
            self.L.vbz_gpu_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers ---------------------------------------------------------------------------------
    def _batch(self, src, src_off, src_size, dst, dst_off, dst_cap, result):
        table("src_off", src_off, torch.int64, self.device)
        table("dst_off", dst_off, torch.int64, self.device)
        table("src_size", src_size, torch.int32, self.device)
        table("dst_cap", dst_cap, torch.int32, self.device)
        table("result", result, torch.int32, self.device)
        assert src.dtype == torch.uint8 and dst.dtype == torch.uint8
        b = self._src_batch(src, src_off, src_size)
        b.dst, b.dst_off, b.dst_cap, b.dst_bytes, b.result = dst.data_ptr(), dst_off.data_ptr(), dst_cap.data_ptr(), dst.numel(), result.data_ptr()
        return b

    @staticmethod
    def _src_batch(src, src_off, src_size):
        """the source half of a GpuBatch (the tables checked by the caller)"""
        b = _lib.GpuBatch()
        b.n_reads, b.src, b.src_off, b.src_size, b.src_bytes = int(src_off.numel()), src.data_ptr(), src_off.data_ptr(), src_size.data_ptr(), src.numel()
        return b

    def _rc(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, self.L.vbz_gpu_last_error(self.ctx).decode()))

    def _call(self, name, *args):
        """One entry of the library, vbz_gpu_<name>(ctx, *args), on the codec's stream between the two waits (see the class) -> its return
        code, after _rc has turned a failure into the RuntimeError that names the entry."""
        cur = self._enter()
        try:
            rc = getattr(self.L, "vbz_gpu_" + name)(self.ctx, *args)
            self._rc(rc, name)
            return rc
        finally:
            self._exit(cur)

    def _typed(self, src, src_off, src_size, dst, dst_off, dst_cap, result, opts, sized=False, dst_bytes=0, f=None, signed=True, ch=None,
               chunk_first=None, chunks=None, m=None, ss=None, g=None, r=None, t=None, out=None, w=None, ev=None, moments=None, sg=None,
               event_first=None, start=None, sp=None, mt=None, span=False, lc=None):
        """One typed decode (include/vbz_gpu.h): the batch, the device entered and left once, and the most general C entry of the call's
        family, NULL for every part that is None.  dst None: nothing is stored in the batch's dst (a chunk decode, the statistics) --
        dst_off / dst_cap are the int16 layout that describes the reads, dst_bytes its extent.  f (a GpuSignalFormat): what is stored,
        with ch (a GpuChunking) into `chunks` at chunk_first; f None: the statistics alone of `signed` samples, with t (a GpuTrim) the
        trim points behind them, into `out`.  m / ss: the GpuNormalization and the shift_scale pointer; g: a GpuSampleRanges; r: a
        GpuPod5Reads (the pod5_ entries: unsized).  w (a GpuWindows, in place of ch): the samples go to the caller-listed windows, the
        rows of `chunks`.  ev (a GpuEvents, with f): no sample is stored -- one record per caller-listed event into `out` (int32 [rows, 4]), the
        exact sums into `moments` (int64 [rows, 2], or None).  sg (a GpuSegmentation, f None): every read's event starts, found on the
        device, into event_first (int64 [reads + 1]) and start (int32, sg.start_cap entries; None: the count-only call).  sp (a GpuSpans,
        f None; m / ss optional): every read's spans into event_first (edge_first) and start (edge, sp.edge_cap entries or None).  mt (a GpuMatch
        or a GpuLocate, in place of ch, with f): the reads' prefixes into `chunks` (float32 [reads, query_len]) and every pair's hit into
        `out` by the *_match or the *_locate entries; with span the hits are vbz_gpu_match_span (the *_match_span and *_locate_span entries).
        lc: mt under the name the locate callers know."""
        b = self._batch(src, src_off, src_size, dst if dst is not None else torch.empty(0, dtype=torch.uint8, device=self.device), dst_off, dst_cap,
                        result)
        if dst is None:
            b.dst, b.dst_bytes = None, int(dst_bytes)
        mt = mt if mt is not None else lc
        reads = [ref(r)] if r is not None else []
        if ev is not None:
            assert ch is None and w is None, "a call has a chunking, windows or events, never two of them"
            name, args = "signal_events", [ref(f)] + reads + [ref(ev), out.data_ptr(), ptr(moments), ref(m), ss, ref(g)]
        elif mt is not None:
            assert ch is None and w is None, "a call has a chunking, windows, events, a match or a locate, never two of them"
            name = ("signal_match" if isinstance(mt, _lib.GpuMatch) else "signal_locate") + ("_span" if span else "")
            args = [ref(f)] + reads + [ref(m), ss, ref(g), ref(mt), chunks.data_ptr(), out.data_ptr()]
        elif w is not None:
            assert ch is None, "a call has a chunking or windows, never both"
            name, args = "decompress_windows", [ref(f)] + reads + [ref(w), chunks.data_ptr(), ref(m), ss, ref(g)]
        elif ch is not None:
            name, args = "decompress_chunks_range", [ref(f), ref(ch)] + reads + [chunk_first.data_ptr(), chunks.data_ptr(), int(chunks.shape[0]), ref(m),
                                                                                 ss, ref(g)]
        elif f is None and sp is not None:
            name, args = "signal_spans", [int(bool(signed))] + reads + [ref(m), ss, ref(g), ref(sp), event_first.data_ptr(), ptr(start)]
        elif f is None and sg is not None:
            name, args = "signal_segment", [int(bool(signed))] + reads + [ref(g), ref(sg), event_first.data_ptr(), ptr(start)]
        elif f is None and t is not None:
            name, args = "signal_trim", [int(bool(signed))] + reads + [ref(m), ref(g), ref(t), ss, out.data_ptr()]
        elif f is None:
            name, args = "signal_norm_range", [int(bool(signed))] + reads + [ref(m), ss, ref(g)]
        elif m is None:   # (the one choice between two entries: no signal entry takes a NULL norm)
            name, args = "decompress_signal", [ref(f)]
        else:
            name, args = "decompress_signal_norm", [ref(f)] + reads + [ref(m), ss]
        self._call(("pod5_" if r is not None else "") + name + "_batch", ref(b), ref(opts), *([int(sized)] if r is None else []), *args)

    @staticmethod
    def options(zigzag=True, size=2, level=1, version=1):
        return _lib.CompressionOptions(bool(zigzag), int(size), int(level), int(version))

    # -- full path -------------------------------------------------------------------------------
    def compress(self, src, src_off, src_size, dst, dst_off, dst_cap, result, opts, sized=False):
        b = self._batch(src, src_off, src_size, dst, dst_off, dst_cap, result)
        self._call("compress_batch", ctypes.byref(b), ctypes.byref(opts), int(sized))

    def decompress(self, src, src_off, src_size, dst, dst_off, dst_cap, result, opts, sized=False):
        b = self._batch(src, src_off, src_size, dst, dst_off, dst_cap, result)
        self._call("decompress_batch", ctypes.byref(b), ctypes.byref(opts), int(sized))

    _SIGNAL_TYPES = {torch.float32: _lib.VBZ_GPU_SIGNAL_F32, torch.float16: _lib.VBZ_GPU_SIGNAL_F16, torch.bfloat16: _lib.VBZ_GPU_SIGNAL_BF16}

    def _signal_format(self, dtype, n, scale, offset, signed):
        """The GpuSignalFormat of n reads decoded to dtype (see decompress_signal)."""
        f = _lib.GpuSignalFormat()
        f.out_type = self._SIGNAL_TYPES[dtype]
        f.is_signed = int(bool(signed))
        f.offset = ptr(table("offset", offset, torch.float32, self.device, at_least=n, none=True))
        f.scale = ptr(table("scale", scale, torch.float32, self.device, at_least=n, none=True))
        return f

    def _norm_args(self, n, norm, norm_out, scale, offset):
        """(the C struct, shift_scale pointer) of a normalising call; norm_out: a float32 [n, 2] tensor on the codec's device, or None"""
        assert scale is None and offset is None, "norm= replaces scale and offset"
        assert isinstance(norm, Normalization), norm
        return norm.c_struct(), ptr(table("norm_out", norm_out, torch.float32, self.device, shape=(n, 2), none=True))

    # -- per-read sample ranges (include/vbz_gpu.h: vbz_gpu_sample_ranges) ---------------------------
    _RANGE_STATS = {"range": _lib.VBZ_GPU_RANGE_STATS_RANGE, "read": _lib.VBZ_GPU_RANGE_STATS_READ}

    def _range_table(self, n, t):
        """a begin / end table (a tensor or a sequence of n values 0 ... 0xFFFFFFFF, or None) as int32 on the device (uint32 bits)"""
        if t is None:
            return None
        t = wrap_u32(t).to(self.device).contiguous()
        assert int(t.numel()) == n, (int(t.numel()), n)
        return t

    def _ranges(self, n, begin, end, stats):
        """(the C struct or None, the tables it points to) of begin= / end= / stats=; both tables None: the un-ranged call"""
        if begin is None and end is None:
            assert stats is None, "stats= goes with begin= / end="
            return None, ()
        assert stats is None or stats in self._RANGE_STATS, stats
        tb, te = self._range_table(n, begin), self._range_table(n, end)
        g = _lib.GpuSampleRanges()
        g.begin, g.end = ptr(tb), ptr(te)
        g.stats = self._RANGE_STATS[stats or "range"]
        return g, (tb, te)

    def range_samples(self, samples, begin=None, end=None):
        """The sample counts of the reads' clamped ranges (include/vbz_gpu.h: vbz_gpu_range_samples_batch): min(end, T) - min(begin, end, T)
        for T = samples[i] (int32 on the device; 2^31 or more as uint32 passes through) -> int32 [n] on the device; it feeds chunk_layout."""
        n = int(table("samples", samples, torch.int32, self.device).numel())
        g, keep = self._ranges(n, begin, end, None)
        out = torch.empty(n, dtype=torch.int32, device=self.device)
        self._call("range_samples_batch", n, samples.data_ptr(), ref(g), out.data_ptr())
        return out

    @staticmethod
    def _extent(n, dst_off, dst_cap):
        """the extent of the arena that the n slots dst_off / dst_cap describe (two host copies)"""
        return int(dst_off.max().item() + dst_cap.to(torch.int64).max().item()) if n else 0

    def signal_norm(self, src, src_off, src_size, dst_off, dst_cap, result, opts, norm, shift_scale=None, signed=True, sized=False, begin=None,
                    end=None, stats=None):
        """Every read's normalisation constants alone (include/vbz_gpu.h: vbz_gpu_signal_norm_batch) -> shift_scale, float32 [n, 2] of
        (shift, scale) per read (allocated when None).  dst_off / dst_cap: the int16 layout of the reads (nothing is stored); result[i] is
        what decompress gives.  begin / end (per-read sample positions, clamped; either may be None): the statistics of that range of
        every read (vbz_gpu_signal_norm_range_batch)."""
        n = int(src_off.numel())
        g, keep = self._ranges(n, begin, end, stats)
        shift_scale = output("shift_scale", shift_scale, torch.float32, self.device, (n, 2))
        m, ss = self._norm_args(n, norm, shift_scale, None, None)
        self._typed(src, src_off, src_size, None, dst_off, dst_cap, result, opts, sized, self._extent(n, dst_off, dst_cap), signed=signed, m=m, ss=ss, g=g)
        return shift_scale

    def _trim_args(self, n, trim, out, shift_scale):
        """(the C struct, the begin table, shift_scale or None) of a trim call over n reads.  out: an int32 tensor of n entries on the
        device (allocated when None); shift_scale: None (not wanted), True (allocated) or a float32 [n, 2] tensor"""
        trim = Trim() if trim is None else trim
        assert isinstance(trim, Trim), trim
        out = output("out", out, torch.int32, self.device, n)
        return trim.c_struct(), out, output("shift_scale", shift_scale, torch.float32, self.device, (n, 2), three_state=True)

    def signal_trim(self, src, src_off, src_size, dst_off, dst_cap, result, opts, norm, trim=None, out=None, shift_scale=None, signed=True,
                    sized=False, begin=None, end=None, stats=None):
        """Every read's trim point (include/vbz_gpu.h: vbz_gpu_signal_trim_batch) -> int32 [n] on the device (uint32 bits; `out` when
        given), which is the begin= of decompress_chunks and range_samples as it stands.  trim: a Trim (None: the defaults).  The
        threshold comes from the statistics signal_norm gives for the same norm / begin / end / stats -- those three say which samples
        the STATISTICS are taken over, nothing else.  shift_scale: True or a float32 [n, 2] tensor to get the constants as well; the
        return is then (begin, shift_scale).  dst_off / dst_cap: the int16 layout of the reads (nothing is stored)."""
        n = int(src_off.numel())
        g, keep = self._ranges(n, begin, end, stats)
        t, out, shift_scale = self._trim_args(n, trim, out, shift_scale)
        m, ss = self._norm_args(n, norm, shift_scale, None, None)
        self._typed(src, src_off, src_size, None, dst_off, dst_cap, result, opts, sized, self._extent(n, dst_off, dst_cap), signed=signed, m=m, ss=ss, g=g,
                    t=t, out=out)
        return out if shift_scale is None else (out, shift_scale)

    def _capped(self, name, t, cap, bound):
        """(cap, the table or None) of an int32 output of at least `cap` entries: the caller's `t`, checked, or a new one.  cap None: t's
        entries when t is given, else bound() (it may cost a host copy); cap 0: the count-only call, no table"""
        if cap is None:
            cap = int(t.numel()) if t is not None else bound()
        if t is not None or cap:
            t = output(name, t, torch.int32, self.device, cap, at_least=True)
        return cap, (t if cap else None)

    # -- signal segmentation (include/vbz_gpu.h: vbz_gpu_segmentation) -------------------------------
    def _segment_args(self, n, segmentation, samples, start_cap, event_first, start):
        """(the C struct, event_first, start) of a segmentation call over n reads of `samples` (an int tensor: the reads' sample counts).
        start_cap None: the bound, sum of 2 + T / (radius + 1) (one host copy); 0: the count-only call, start is None"""
        sg = Segmentation() if segmentation is None else segmentation
        assert isinstance(sg, Segmentation), sg
        start_cap, start = self._capped("start", start, start_cap, lambda: int((samples.to(torch.int64) // (sg.radius + 1) + 2).sum().item()) if n else 0)
        event_first = output("event_first", event_first, torch.int64, self.device, n + 1)
        return sg.c_struct(start_cap), event_first, start

    def signal_segment(self, src, src_off, src_size, dst_off, dst_cap, result, opts, segmentation=None, start_cap=None, signed=True, sized=False,
                       begin=None, end=None, event_first=None, start=None):
        """Every read's event starts, found on the device with no sample stored (include/vbz_gpu.h: vbz_gpu_signal_segment_batch) ->
        (event_first int64 [n + 1], start int32 [start_cap] or None), both on the device and in the layout signal_events reads as it
        stands: read i owns rows event_first[i] ... event_first[i + 1] - 1, row 0 of a read starts at 0 and one row follows per boundary.
        segmentation: a Segmentation (None: its defaults).  start_cap: entries of start (None: the bound 2 + T / (radius + 1) per read;
        0: the count-only call) -- a read whose rows end beyond it gets VBZ_DESTINATION_SIZE_ERROR and no starts.  begin / end: the
        signal is that range of every read, positions count from its first sample.  dst_off / dst_cap: the int16 layout of the reads
        (nothing is stored); result[i] is what decompress gives.  No synchronisation."""
        n = int(src_off.numel())
        g, keep = self._ranges(n, begin, end, None)
        sg, event_first, start = self._segment_args(n, segmentation, dst_cap.to(torch.int64) // 2, start_cap, event_first, start)
        self._typed(src, src_off, src_size, None, dst_off, dst_cap, result, opts, sized, self._extent(n, dst_off, dst_cap), signed=signed, g=g, sg=sg,
                    event_first=event_first, start=start)
        return event_first, start

    # -- signal spans (include/vbz_gpu.h: vbz_gpu_spans) --------------------------------------------
    def _span_args(self, n, spans, samples, edge_cap, edge_first, edge, norm, level, shift_scale):
        """(the C struct, edge_first, edge, the GpuNormalization or None, the shift_scale pointer, shift_scale, what to keep alive) of a span
        call over n reads of `samples` (an int tensor).  edge_cap None: the bound, sum of max_edges (one host copy); 0: the count-only call.
        Exactly one of norm (a Normalization) and level (float32 [n, 2] of {a, w} on the device) is given"""
        sp = Spans() if spans is None else spans
        assert isinstance(sp, Spans), sp
        assert (norm is None) != (level is None), "one of norm= and level="
        k = sp.min_length + sp.merge_gap + 1
        edge_cap, edge = self._capped("edge", edge, edge_cap, lambda: int((2 * ((samples.to(torch.int64) + sp.merge_gap + 1) // k)).sum().item()) if n else 0)
        edge_first = output("edge_first", edge_first, torch.int64, self.device, n + 1)
        m = ss = None
        if norm is not None:
            shift_scale = output("shift_scale", shift_scale, torch.float32, self.device, (n, 2), three_state=True)
            m, ss = self._norm_args(n, norm, shift_scale, None, None)
        else:
            assert shift_scale is None, "shift_scale= goes with norm="
            table("level", level, torch.float32, self.device, shape=(n, 2))
        return sp.c_struct(edge_cap, ptr(level)), edge_first, edge, m, ss, shift_scale

    def signal_spans(self, src, src_off, src_size, dst_off, dst_cap, result, opts, spans=None, edge_cap=None, signed=True, sized=False, begin=None,
                     end=None, edge_first=None, edge=None, norm=None, level=None, shift_scale=None, stats=None):
        """Every read's spans above or below its level, found on the device with no sample stored (include/vbz_gpu.h:
        vbz_gpu_signal_spans_batch) -> (edge_first int64 [n + 1], edge int32 [edge_cap] or None), both on the device: span k of read i is
        edge[edge_first[i] + 2 k] = begin, edge[edge_first[i] + 2 k + 1] = end, and the two tables go into signal_events as event_first and
        start as they stand.  spans: a Spans (None: its defaults).  The level: norm (a Normalization: the read's shift + f scale; the
        statistics are signal_norm's for the same begin / end / stats) or level (float32 [n, 2] of {a, w}: a + f w).  shift_scale (with
        norm): True or a float32 [n, 2] tensor to get the constants as well; the return is then (edge_first, edge, shift_scale).  edge_cap:
        entries of edge (None: the bound; 0: the count-only call) -- a read whose pairs end beyond it gets VBZ_DESTINATION_SIZE_ERROR and
        no pair.  begin / end: the signal is that range of every read.  dst_off / dst_cap: the int16 layout of the reads."""
        n = int(src_off.numel())
        g, keep = self._ranges(n, begin, end, stats)
        sp, edge_first, edge, m, ss, shift_scale = self._span_args(n, spans, dst_cap.to(torch.int64) // 2, edge_cap, edge_first, edge, norm, level,
                                                                   shift_scale)
        self._typed(src, src_off, src_size, None, dst_off, dst_cap, result, opts, sized, self._extent(n, dst_off, dst_cap), signed=signed, m=m, ss=ss, g=g,
                    sp=sp, event_first=edge_first, start=edge)
        return (edge_first, edge) if shift_scale is None else (edge_first, edge, shift_scale)

    def decompress_signal(self, src, src_off, src_size, dst, dst_off, dst_cap, result, opts, scale=None, offset=None, signed=True, sized=False,
                          norm=None, norm_out=None):
        """Decode int16 signal straight to calibrated samples, y = (x + offset[i]) * scale[i] in float32 arithmetic (include/vbz_gpu.h:
        vbz_gpu_decompress_signal_batch).  dst: a 1-D float32, float16 or bfloat16 tensor (its dtype is the output type); dst_off / dst_cap
        in bytes of dst, as everywhere in this class (unsized: dst_cap[i] = samples * element size); result[i] = samples * element size or
        an error code.  scale / offset: float32 tensors of n entries on the codec's device, or None (1 / 0 for every read).  signed: the
        16-bit samples are int16 (True) or uint16.  norm (a Normalization; not with scale / offset): every read normalised by its own
        statistics instead (vbz_gpu_decompress_signal_norm_batch), its (shift, scale) left in norm_out (float32 [n, 2], or None)."""
        assert dst.dtype in self._SIGNAL_TYPES, dst.dtype
        table("dst", dst, dst.dtype, shape=(None,))
        n = int(src_off.numel())
        m, ss = self._norm_args(n, norm, norm_out, scale, offset) if norm is not None else (None, None)
        f = self._signal_format(dst.dtype, n, scale, offset, signed)
        self._typed(src, src_off, src_size, dst.view(torch.uint8), dst_off, dst_cap, result, opts, sized, f=f, m=m, ss=ss)

    # -- stages ----------------------------------------------------------------------------------
    # (version: 0, 1, or _lib.VBZ_GPU_VERSION_POD5 -- the svb16 stream of POD5 rows, size 2 with zig-zag)
    def svb_compress(self, src, src_off, src_size, dst, dst_off, dst_cap, result, size=2, zigzag=True, version=0):
        b = self._batch(src, src_off, src_size, dst, dst_off, dst_cap, result)
        self._call("svb_compress_batch", ctypes.byref(b), size, int(zigzag), version)

    def svb_decompress(self, src, src_off, src_size, dst, dst_off, dst_cap, result, size=2, zigzag=True, version=0):
        b = self._batch(src, src_off, src_size, dst, dst_off, dst_cap, result)
        self._call("svb_decompress_batch", ctypes.byref(b), size, int(zigzag), version)

    def zstd_compress(self, src, src_off, src_size, dst, dst_off, dst_cap, result, key_bytes=None):
        b = self._batch(src, src_off, src_size, dst, dst_off, dst_cap, result)
        self._call("zstd_compress_batch", ctypes.byref(b), ptr(key_bytes))

    def zstd_decompress(self, src, src_off, src_size, dst, dst_off, dst_cap, result):
        b = self._batch(src, src_off, src_size, dst, dst_off, dst_cap, result)
        self._call("zstd_decompress_batch", ctypes.byref(b))

    def xxh64(self, src, src_off, src_size, out):
        """out[i] = XXH64 (seed 0) of src[src_off[i] : src_off[i] + src_size[i]]; out: an int64 tensor of n entries whose bits are
        the uint64 hashes (include/vbz_gpu.h: vbz_gpu_xxh64_batch)."""
        n = int(src_off.numel())
        table("src_off", src_off, torch.int64, self.device)
        table("src_size", src_size, torch.int32, self.device)
        table("out", out, torch.int64, self.device, at_least=n)
        assert src.dtype == torch.uint8
        self._call("xxh64_batch", ctypes.byref(self._src_batch(src, src_off, src_size)), out.data_ptr())

    # -- dense arenas ------------------------------------------------------------------------------
    def _sync_total(self, off):
        """off[-1] (an int64 table the codec's stream has written) on the host: one synchronisation, between the two waits"""
        self._call("synchronize")
        return int(off[-1].item())

    def pack(self, dst, dst_off, dst_cap, result, align=16, out=None):
        """Dense arena of a finished compress (or decompress) call (include/vbz_gpu.h: vbz_gpu_pack_batch) -> (packed, packed_off,
        packed_size): read i's result[i] bytes at packed[packed_off[i]:], packed_off int64 [n + 1] (packed_off[n] = the total), packed_size
        int32 [n] whose bits are the byte count or the error code.  Without `out` the tables are computed first, one synchronisation reads
        the total and the arena is allocated (total + 64 bytes: the decoders' slack); with `out` (uint8) nothing synchronises, and an `out`
        smaller than the total is left untouched."""
        n = int(dst_off.numel())
        table("dst_off", dst_off, torch.int64, self.device)
        table("dst_cap", dst_cap, torch.int32, self.device, numel=n)
        table("result", result, torch.int32, self.device, numel=n)
        assert dst.dtype == torch.uint8
        b = _lib.GpuBatch()
        b.n_reads, b.dst, b.dst_off, b.dst_cap, b.dst_bytes, b.result = n, dst.data_ptr(), dst_off.data_ptr(), dst_cap.data_ptr(), dst.numel(), result.data_ptr()
        packed_off = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        packed_size = torch.empty(n, dtype=torch.int32, device=self.device)
        if out is None:
            self._call("pack_batch", ctypes.byref(b), align, None, 0, packed_off.data_ptr(), packed_size.data_ptr())
            out = torch.empty(self._sync_total(packed_off) + 64, dtype=torch.uint8, device=self.device)
        table("out", out, torch.uint8, self.device)
        self._call("pack_batch", ctypes.byref(b), align, out.data_ptr(), out.numel(), packed_off.data_ptr(), packed_size.data_ptr())
        return out, packed_off, packed_size

    def decompressed_sizes(self, src, src_off, src_size, opts, align=16):
        """n x vbz_decompressed_size of sized buffers and their output layout (include/vbz_gpu.h: vbz_gpu_decompressed_size_batch) ->
        (raw_size int32 [n], bits = the size or an error code; raw_off int64 [n + 1], raw_off[n] = the total)."""
        n = int(src_off.numel())
        table("src_off", src_off, torch.int64, self.device)
        table("src_size", src_size, torch.int32, self.device, numel=n)
        assert src.dtype == torch.uint8
        b = self._src_batch(src, src_off, src_size)
        raw_size = torch.empty(n, dtype=torch.int32, device=self.device)
        raw_off = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        self._call("decompressed_size_batch", ctypes.byref(b), ctypes.byref(opts), align, raw_size.data_ptr(), raw_off.data_ptr())
        return raw_size, raw_off

    def decompress_packed(self, packed, packed_off, packed_size, opts, align=16):
        """Decode a dense arena of sized buffers (pack() of a sized compress call): the sizes come from the headers, the output is
        allocated (one synchronisation) and the batch decoded -> (raw, raw_off, raw_size, result).  An entry whose size is an error code
        gets dst_cap = 0, so the decoder gives the verdict vbz_decompress_sized gives for that buffer (VBZ_INPUT_SIZE_ERROR under 4 bytes)."""
        n = int(packed_size.numel())
        src_off = packed_off[:n]
        raw_size, raw_off = self.decompressed_sizes(packed, src_off, packed_size, opts, align)
        raw = torch.empty(self._sync_total(raw_off) + 64, dtype=torch.uint8, device=self.device)
        err = (raw_size < 0) & (raw_size >= _lib.VBZ_DEVICE_ERROR - (1 << 32))
        dst_cap = torch.where(err, torch.zeros_like(raw_size), raw_size)
        result = torch.empty(n, dtype=torch.int32, device=self.device)
        self.decompress(packed, src_off, packed_size, raw, raw_off[:n], dst_cap, result, opts, sized=True)
        return raw, raw_off, raw_size, result

    def decompress_packed_signal(self, packed, packed_off, packed_size, opts, dtype=torch.float32, scale=None, offset=None, signed=True, norm=None,
                                 norm_out=None):
        """decompress_packed into calibrated samples (decompress_signal): the sample counts come from the headers, the output (`dtype`)
        is laid out with 16-byte aligned slots and allocated (one synchronisation), and the batch decoded -> (out, out_off, samples,
        result): read i is out[out_off[i] : out_off[i] + samples[i]] (out_off int64 and samples int32, in elements) when result[i] is no
        error code."""
        assert dtype in self._SIGNAL_TYPES, dtype
        n = int(packed_size.numel())
        src_off = packed_off[:n]
        raw_size, raw_off = self.decompressed_sizes(packed, src_off, packed_size, opts, 16)   # (int16 bytes, 16-byte aligned)
        total16 = self._sync_total(raw_off)
        elem = torch.empty(0, dtype=dtype).element_size()
        # an int16 slot of b bytes holds b / 2 samples: its typed slot, b / 2 * elem bytes, keeps the 16-byte alignment
        out = torch.empty(total16 // 2, dtype=dtype, device=self.device)
        err = (raw_size < 0) & (raw_size >= _lib.VBZ_DEVICE_ERROR - (1 << 32))
        raw = torch.where(err, torch.zeros_like(raw_size), raw_size)
        # (capacity: the header's samples, rounded up -- an odd header gets the verdict the int16 decode gives it)
        dst_cap = ((raw + 1) // 2 * elem).to(torch.int32)
        out_off = raw_off[:n] // 2
        result = torch.empty(n, dtype=torch.int32, device=self.device)
        self.decompress_signal(packed, src_off, packed_size, out, out_off * elem, dst_cap, result, opts, scale=scale, offset=offset, signed=signed,
                               sized=True, norm=norm, norm_out=norm_out)
        return out, out_off, (raw // 2).to(torch.int32), result

    # -- model-input chunks ------------------------------------------------------------------------
    _CHUNK_MODES = {"pad": _lib.VBZ_GPU_CHUNK_PAD, "end": _lib.VBZ_GPU_CHUNK_END}

    def _chunking(self, chunk_len, step, mode, end_align, pad=0.0):
        assert mode in self._CHUNK_MODES, mode
        ch = _lib.GpuChunking()
        ch.chunk_len, ch.step, ch.mode = int(chunk_len), int(step), self._CHUNK_MODES[mode]
        ch.end_align = int(end_align) if mode == "end" else 0
        ch.pad = float(pad)
        return ch

    def _chunk_layout_call(self, samples, ch, chunk_first, info=None, info_cap=0):
        self._call("chunk_layout_batch", int(samples.numel()), samples.data_ptr(), ctypes.byref(ch), chunk_first.data_ptr(), ptr(info), int(info_cap))

    def _chunk_tables(self, samples, ch, info, also=None):
        """chunk_first (and chunk_info) of `samples` (int32 on the device, uint32 bits) under ch, with ONE synchronisation for the total;
        also: an int64 device scalar wanted on the host in the same synchronisation -> (chunk_first, chunk_info or None, also's value)"""
        n = int(table("samples", samples, torch.int32, self.device).numel())
        chunk_first = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        self._chunk_layout_call(samples, ch, chunk_first)
        self.synchronize()
        host = torch.stack([chunk_first[-1], also if also is not None else chunk_first[-1]]).cpu().tolist()
        chunk_info = None
        if info:
            chunk_info = torch.empty((host[0], 2), dtype=torch.int32, device=self.device)
            self._chunk_layout_call(samples, ch, chunk_first, chunk_info, host[0])
        return chunk_first, chunk_info, host

    def chunk_layout(self, samples, chunk_len, step, mode="pad", end_align=1, info=True):
        """The chunk layout of reads of `samples` samples (int32 on the device; 2^31 or more as uint32 -- an error code of
        decompressed_sizes -- counts 0 chunks) (include/vbz_gpu.h: vbz_gpu_chunk_layout_batch) -> (chunk_first int64 [n + 1],
        chunk_info int32 [total, 2] = (read, start sample) per row, or None).  One synchronisation for the total."""
        chunk_first, chunk_info, _ = self._chunk_tables(samples, self._chunking(chunk_len, step, mode, end_align), info)
        return chunk_first, chunk_info

    def _chunk_arena(self, rows, chunk_len, dtype):
        """an uninitialised [rows, chunk_len] arena (a valid pointer when it has no rows)"""
        return torch.empty((max(rows, 1), int(chunk_len)), dtype=dtype, device=self.device)[:rows]

    def _decode_chunks(self, src, src_off, src_size, dst_off, dst_cap, dst_bytes, result, opts, sized, ch, chunk_first, chunks, dtype, scale, offset,
                       signed, norm=None, norm_out=None, ranges=None):
        assert dtype in self._SIGNAL_TYPES, dtype
        table("chunks", chunks, dtype)
        n = int(src_off.numel())
        m, ss = self._norm_args(n, norm, norm_out, scale, offset) if norm is not None else (None, None)
        f = self._signal_format(dtype, n, scale, offset, signed)
        self._typed(src, src_off, src_size, None, dst_off, dst_cap, result, opts, sized, dst_bytes, f=f, ch=ch, chunk_first=chunk_first, chunks=chunks,
                    m=m, ss=ss, g=ranges)

    def decompress_chunks(self, src, src_off, src_size, samples, result, opts, chunk_len, step, mode="pad", end_align=1, pad=0.0, dtype=torch.float16,
                          scale=None, offset=None, signed=True, norm=None, norm_out=None, begin=None, end=None, stats=None):
        """Decode unsized int16 reads of `samples` samples (int32 on the device) straight into model-input chunks (include/vbz_gpu.h:
        vbz_gpu_decompress_chunks_batch), calibrated as decompress_signal does -> (chunks [total, chunk_len] of dtype, chunk_first int64
        [n + 1], chunk_info int32 [total, 2]): chunk k of read i is chunks[chunk_first[i] + k] when result[i] is no error code (result[i] =
        samples * element size).  The int16 layout the call describes the reads with is built here; one synchronisation.  norm / norm_out:
        as for decompress_signal (vbz_gpu_decompress_chunks_norm_batch).  begin / end (per-read sample positions, clamped; either
        may be None): the chunks are those of that range of every read, chunk_info's start samples relative to its begin, and with norm=
        the statistics are the range's (stats="range", the default) or the whole read's (stats="read")
        (vbz_gpu_decompress_chunks_range_batch)."""
        n = int(src_off.numel())
        assert int(samples.numel()) == n
        ch = self._chunking(chunk_len, step, mode, end_align, pad)
        g, keep = self._ranges(n, begin, end, stats)
        dst_off, dst_cap = self._row_layout(samples)
        laid = samples if g is None else self.range_samples(samples, begin=keep[0], end=keep[1])
        chunk_first, chunk_info, host = self._chunk_tables(laid, ch, True, also=dst_off[-1])
        chunks = self._chunk_arena(host[0], chunk_len, dtype)
        self._decode_chunks(src, src_off, src_size, dst_off[:n], dst_cap, host[1], result, opts, False, ch, chunk_first, chunks, dtype, scale, offset,
                            signed, norm, norm_out, g)
        return chunks, chunk_first, chunk_info

    def decompress_packed_chunks(self, packed, packed_off, packed_size, opts, chunk_len, step, mode="pad", end_align=1, pad=0.0, dtype=torch.float16,
                                 scale=None, offset=None, signed=True, norm=None, norm_out=None, begin=None, end=None, stats=None):
        """decompress_packed into model-input chunks (decompress_chunks): the sample counts come from the headers (decompressed_sizes),
        then the layout and the decode -> (chunks, chunk_first, chunk_info, result).  One synchronisation.  begin / end / stats: as for
        decompress_chunks."""
        n = int(packed_size.numel())
        g, keep = self._ranges(n, begin, end, stats)
        src_off = packed_off[:n]
        ch = self._chunking(chunk_len, step, mode, end_align, pad)
        raw_size, raw_off = self.decompressed_sizes(packed, src_off, packed_size, opts, 16)   # (int16 bytes, 16-byte aligned)
        err = (raw_size < 0) & (raw_size >= _lib.VBZ_DEVICE_ERROR - (1 << 32))
        raw = torch.where(err, torch.zeros_like(raw_size), raw_size)
        samples = torch.where(err, raw_size, raw // 2)   # (an error code: no chunks)
        laid = samples if g is None else self.range_samples(samples.contiguous(), begin=keep[0], end=keep[1])
        chunk_first, chunk_info, host = self._chunk_tables(laid, ch, True, also=raw_off[-1])
        chunks = self._chunk_arena(host[0], chunk_len, dtype)
        result = torch.empty(n, dtype=torch.int32, device=self.device)
        self._decode_chunks(packed, src_off, packed_size, raw_off[:n], raw, host[1], result, opts, True, ch, chunk_first, chunks, dtype, scale, offset,
                            signed, norm, norm_out, g)
        return chunks, chunk_first, chunk_info, result

    # -- signal windows (include/vbz_gpu.h: vbz_gpu_windows) -------------------------------------------
    def _windows(self, n, window_first, start, window_len, pad):
        """(the C struct, the tables it points to) of n reads' windows: window_first int64 [n + 1] and start int32 [rows] on the device"""
        table("window_first", window_first, torch.int64, self.device, numel=n + 1)
        table("start", start, torch.int32, self.device)
        w = _lib.GpuWindows()
        w.window_len, w.pad, w.window_rows, w.window_first, w.start = int(window_len), float(pad), int(start.numel()), window_first.data_ptr(), start.data_ptr()
        return w, (window_first, start)

    def _decode_windows(self, n, src, src_off, src_size, dst_off, dst_cap, dst_bytes, result, opts, sized, window_first, start, window_len, pad, dtype,
                        scale, offset, signed, norm, norm_out, begin, end, stats, r=None):
        assert dtype in self._SIGNAL_TYPES, dtype
        w, keep_w = self._windows(n, window_first, start, window_len, pad)
        g, keep_g = self._ranges(n, begin, end, stats)
        if norm is not None:
            norm_out = output("norm_out", norm_out, torch.float32, self.device, (n, 2))
        m, ss = self._norm_args(n, norm, norm_out, scale, offset) if norm is not None else (None, None)
        f = self._signal_format(dtype, n, scale, offset, signed)
        out = self._chunk_arena(int(start.numel()), window_len, dtype)
        self._typed(src, src_off, src_size, None, dst_off, dst_cap, result, opts, sized, dst_bytes, f=f, chunks=out, m=m, ss=ss, g=g, r=r, w=w)
        return out if norm is None else (out, norm_out)

    def decompress_windows(self, src, src_off, src_size, samples, result, opts, window_first, start, window_len, pad=0.0, dtype=torch.float16,
                           scale=None, offset=None, signed=True, norm=None, norm_out=None, begin=None, end=None, stats=None):
        """Decode unsized int16 reads of `samples` samples (int32 on the device) straight into caller-listed windows of their signal
        (include/vbz_gpu.h: vbz_gpu_decompress_windows_batch), calibrated as decompress_signal does -> windows [rows, window_len] of dtype,
        and with norm= (windows, shift_scale float32 [n, 2]).  Read i owns rows window_first[i] ... window_first[i + 1] - 1 (int64 [n + 1] on
        the device); row c holds samples start[c] ... start[c] + window_len - 1 (int32 [rows] on the device, sorted within a read; may
        hang over either end) of the read's signal -- of its range with begin / end (as for decompress_chunks) -- and `pad` outside it.
        result[i] = samples * element size when every position of the read's rows has been written.  No synchronisation."""
        n = int(src_off.numel())
        assert int(samples.numel()) == n
        dst_off, dst_cap = self._row_layout(samples)
        return self._decode_windows(n, src, src_off, src_size, dst_off[:n], dst_cap, int(dst_off[-1].item()), result, opts, False, window_first, start,
                                    window_len, pad, dtype, scale, offset, signed, norm, norm_out, begin, end, stats)

    # -- signal match (include/vbz_gpu.h: vbz_gpu_match) ------------------------------------------------
    def _align_arenas(self, n, al, query, out, words=2):
        """(query float32 [n, N], hits int32 [n, R, words]) of a match or locate call (al: its GpuMatch or GpuLocate; R: its references or
        targets): the caller's, checked, or new ones.  words: 2 (cost, end), or 4 of the span calls (cost, end, start, 0)"""
        N, R = int(al.query_len), int(al.n_refs if isinstance(al, _lib.GpuMatch) else al.n_targets)
        return output("query", query, torch.float32, self.device, (n, N)), output("out", out, torch.int32, self.device, (n, R, words))

    _match_arenas = _locate_arenas = _align_arenas   # (the names the two families' callers know)

    def _align_stage(self, rule, query, valid, levels, levels_len, out, span):
        """match() and locate(): rule a Match or a Locate, levels / levels_len its references or targets"""
        n = int(query.shape[0])
        al = rule.c_struct(levels, levels_len)
        table("valid", valid, torch.int32, self.device, numel=n)
        query, out = self._align_arenas(n, al, query, out, 4 if span else 2)
        self._call(("match" if isinstance(rule, Match) else "locate") + ("_span_batch" if span else "_batch"), n, query.data_ptr(), valid.data_ptr(),
                   ctypes.byref(al), out.data_ptr())
        return out

    def match(self, query, valid, ref, ref_len, match=None, out=None, span=False):
        """The stage entry (include/vbz_gpu.h: vbz_gpu_match_batch): subsequence DTW of every reference row (ref int8 [R, ref_stride],
        ref_len int32 [R], on the device) against the first min(valid[i], query_len) samples of query row i (float32 [n, query_len];
        valid int32 [n], uint32 bits) -> hits int32 [n, R, 2] = (cost, end) on the device (`out` when given).  match: a Match whose
        query_len is the rows' length (None: quant 32 and that length).  No synchronisation.  (span: match_span's route.)"""
        return self._align_stage(match or Match(query_len=int(query.shape[1])), query, valid, ref, ref_len, out, span)

    def _signal_align(self, n, src, src_off, src_size, dst_off, dst_cap, dst_bytes, result, opts, sized, rule, levels, levels_len, scale, offset, signed,
                      norm, norm_out, begin, end, stats, query, out, r=None, span=False):
        """signal_match(), signal_locate() and their pod5_ forms: rule a Match or a Locate, levels / levels_len its references or targets"""
        al = rule.c_struct(levels, levels_len)
        query, out = self._align_arenas(n, al, query, out, 4 if span else 2)
        g, keep_g = self._ranges(n, begin, end, stats)
        if norm is not None:
            norm_out = output("norm_out", norm_out, torch.float32, self.device, (n, 2))
        m, ss = self._norm_args(n, norm, norm_out, scale, offset) if norm is not None else (None, None)
        f = self._signal_format(torch.float32, n, scale, offset, signed)
        self._typed(src, src_off, src_size, None, dst_off, dst_cap, result, opts, sized, dst_bytes, f=f, chunks=query, m=m, ss=ss, g=g, r=r, mt=al, out=out,
                    span=span)
        return (out, query) if norm is None else (out, query, norm_out)

    def signal_match(self, src, src_off, src_size, dst_off, dst_cap, result, opts, ref, ref_len, match=None, scale=None, offset=None, signed=True,
                     sized=False, norm=None, norm_out=None, begin=None, end=None, stats=None, query=None, out=None, span=False):
        """Decode every read's prefix and match it against every reference row on the device (include/vbz_gpu.h:
        vbz_gpu_signal_match_batch) -> (hits int32 [n, R, 2] = (cost, end), query float32 [n, query_len]), and with norm= also
        shift_scale float32 [n, 2].  The query is the first query_len samples of the read's signal -- of its range with begin / end --
        converted as decompress_windows converts them, +0 behind the signal's end.  ref / ref_len / match: as for match().  dst_off /
        dst_cap: the int16 layout of the reads (nothing is stored there); result[i] = samples * 4.  No synchronisation."""
        n = int(src_off.numel())
        return self._signal_align(n, src, src_off, src_size, dst_off, dst_cap, self._extent(n, dst_off, dst_cap), result, opts, sized, match or Match(), ref, ref_len,
                                  scale, offset, signed, norm, norm_out, begin, end, stats, query, out, span=span)

    def pod5_signal_match(self, src, src_off, src_size, row_samples, read_first_row, result, ref, ref_len, match=None, scale=None, offset=None,
                          signed=True, norm=None, norm_out=None, begin=None, end=None, stats=None, query=None, out=None, read_result=None,
                          span=False):
        """signal_match over POD5 signal rows grouped into reads by read_first_row (include/vbz_gpu.h: vbz_gpu_pod5_signal_match_batch):
        hits, query, scale / offset / norm_out and begin / end are per READ, the positions those of the read's concatenated signal;
        result is per ROW, read_result (int32 [n_reads] on the device, optional) per read."""
        n = int(src_off.numel())
        assert int(row_samples.numel()) == n
        r, first_row, read_result = self._pod5_reads(n, read_first_row, read_result)
        dst_off, dst_cap = self._row_layout(row_samples)
        return self._signal_align(r.n_reads, src, src_off, src_size, dst_off[:n], dst_cap, int(dst_off[-1].item()), result, pod5_options(), False,
                                  match or Match(), ref, ref_len, scale, offset, signed, norm, norm_out, begin, end, stats, query, out, r=r, span=span)

    # -- signal locate (include/vbz_gpu.h: vbz_gpu_locate) ----------------------------------------------
    def locate(self, query, valid, target, target_len, locate=None, out=None, span=False):
        """The stage entry (include/vbz_gpu.h: vbz_gpu_locate_batch): the first min(valid[i], query_len) samples of query row i (float32
        [n, query_len <= 2048]; valid int32 [n], uint32 bits), quantised and aligned WHOLE by subsequence DTW to a stretch of every target row
        (target int8 [G, target_stride], target_len int32 [G], on the device) -> hits int32 [n, G, 2] = (cost, end) on the device (`out`
        when given), end in target coordinates.  locate: a Locate whose query_len is the rows' length (None: quant 32 and that length).  No
        synchronisation.  (span: locate_span's route.)"""
        return self._align_stage(locate or Locate(query_len=int(query.shape[1])), query, valid, target, target_len, out, span)

    def signal_locate(self, src, src_off, src_size, dst_off, dst_cap, result, opts, target, target_len, locate=None, scale=None, offset=None,
                      signed=True, sized=False, norm=None, norm_out=None, begin=None, end=None, stats=None, query=None, out=None, span=False):
        """Decode every read's prefix and locate it in every target row on the device (include/vbz_gpu.h: vbz_gpu_signal_locate_batch) ->
        (hits int32 [n, G, 2] = (cost, end), query float32 [n, query_len]), and with norm= also shift_scale float32 [n, 2].  The query is
        signal_match's; target / target_len / locate: as for locate().  No synchronisation."""
        n = int(src_off.numel())
        return self._signal_align(n, src, src_off, src_size, dst_off, dst_cap, self._extent(n, dst_off, dst_cap), result, opts, sized, locate or Locate(),
                                  target, target_len, scale, offset, signed, norm, norm_out, begin, end, stats, query, out, span=span)

    def pod5_signal_locate(self, src, src_off, src_size, row_samples, read_first_row, result, target, target_len, locate=None, scale=None, offset=None,
                           signed=True, norm=None, norm_out=None, begin=None, end=None, stats=None, query=None, out=None, read_result=None,
                           span=False):
        """signal_locate over POD5 signal rows grouped into reads by read_first_row (include/vbz_gpu.h: vbz_gpu_pod5_signal_locate_batch):
        hits, query, scale / offset / norm_out and begin / end are per READ; result is per ROW, read_result (optional) per read."""
        n = int(src_off.numel())
        assert int(row_samples.numel()) == n
        r, first_row, read_result = self._pod5_reads(n, read_first_row, read_result)
        dst_off, dst_cap = self._row_layout(row_samples)
        return self._signal_align(r.n_reads, src, src_off, src_size, dst_off[:n], dst_cap, int(dst_off[-1].item()), result, pod5_options(), False,
                                  locate or Locate(), target, target_len, scale, offset, signed, norm, norm_out, begin, end, stats, query, out, r=r, span=span)

    # -- signal locate with the start of the stretch (include/vbz_gpu.h: vbz_gpu_locate_span_batch) ----------
    def locate_span(self, query, valid, target, target_len, locate=None, out=None):
        """locate() with the start of the aligned stretch (include/vbz_gpu.h: vbz_gpu_locate_span_batch): the same arguments -> hits int32
        [n, G, 4] = (cost, end, start, 0); the whole query is aligned to the target's levels [start, end), start the smallest of a path of
        that cost to that end.  A match_best() over these hits gives each read's best target and its stretch.  No synchronisation."""
        return self.locate(query, valid, target, target_len, locate, out, span=True)

    def signal_locate_span(self, *args, **kw):
        """signal_locate() with the start of the aligned stretch (include/vbz_gpu.h: vbz_gpu_signal_locate_span_batch): the same arguments,
        hits int32 [n, G, 4] = (cost, end, start, 0)."""
        return self.signal_locate(*args, span=True, **kw)

    def pod5_signal_locate_span(self, *args, **kw):
        """pod5_signal_locate() with the start of the aligned stretch (include/vbz_gpu.h: vbz_gpu_pod5_signal_locate_span_batch): the same
        arguments, hits int32 [n, G, 4] = (cost, end, start, 0)."""
        return self.pod5_signal_locate(*args, span=True, **kw)

    # -- signal match with the start of the stretch (include/vbz_gpu.h: vbz_gpu_match_span) ------------------
    def match_span(self, query, valid, ref, ref_len, match=None, out=None):
        """match() with the start of the aligned stretch (include/vbz_gpu.h: vbz_gpu_match_span_batch): the same arguments -> hits int32
        [n, R, 4] = (cost, end, start, 0); the reference is aligned to the query's samples [start, end), start the smallest of a path of
        that cost to that end.  No synchronisation."""
        return self.match(query, valid, ref, ref_len, match, out, span=True)

    def signal_match_span(self, *args, **kw):
        """signal_match() with the start of the aligned stretch (include/vbz_gpu.h: vbz_gpu_signal_match_span_batch): the same arguments,
        hits int32 [n, R, 4] = (cost, end, start, 0)."""
        return self.signal_match(*args, span=True, **kw)

    def pod5_signal_match_span(self, *args, **kw):
        """pod5_signal_match() with the start of the aligned stretch (include/vbz_gpu.h: vbz_gpu_pod5_signal_match_span_batch): the same
        arguments, hits int32 [n, R, 4] = (cost, end, start, 0)."""
        return self.pod5_signal_match(*args, span=True, **kw)

    # -- signal match: the warping path of chosen pairs (include/vbz_gpu.h: vbz_gpu_match_path) ------------
    def match_best(self, spans, max_cost=None, out=None):
        """The winners' table of a span call (include/vbz_gpu.h: vbz_gpu_match_best_batch): spans int32 [n, R, 4] on the device -> pairs
        int32 [n, 4] = (read, ref, begin, end) on the device (`out` when given): per read the reference of least cost, ties to the
        smallest index, empty verdicts and costs above max_cost (None: no bound) skipped; ref 0xFFFFFFFF and begin = end = 0 when none
        qualifies.  No synchronisation."""
        table("spans", spans, torch.int32, self.device, shape=(None, None, 4))
        n, R = int(spans.shape[0]), int(spans.shape[1])
        out = output("out", out, torch.int32, self.device, (n, 4))
        self._call("match_best_batch", n, spans.data_ptr(), R, 0xFFFFFFFF if max_cost is None else int(max_cost), out.data_ptr())
        return out

    def match_path(self, query, valid, ref, ref_len, pairs, max_width, match=None, hit=None, rows=None):
        """The warping path of every listed pair (include/vbz_gpu.h: vbz_gpu_match_path_batch): pairs int32 [p, 4] = (read, ref, begin,
        end) on the device (match_best's table, or any other: it is untrusted), query / ref / ref_len / match as for match(), valid int32
        [n] or None (every row has query_len samples: the query arena of a fused span call) -> (hit int32 [p, 4] = (cost, end, start,
        rows), rows int32 [p, ref_stride, 2] = (begin, end) per reference row, {0, 0} behind the reference's end) on the device.  A
        pair's window is its samples [begin, end), at most max_width of them (a multiple of 8, 8 ... 65536; it sizes the scratch).  A
        pair outside the rules gets the empty verdict.  No synchronisation."""
        return self._align_path(match or Match(query_len=int(query.shape[1])), query, valid, ref, ref_len, pairs, max_width, hit, rows)

    # -- signal locate: the warping path of chosen pairs, in target coordinates (include/vbz_gpu.h: vbz_gpu_locate_path_batch) ------
    def locate_path(self, query, valid, target, target_len, pairs, max_width, locate=None, hit=None, rows=None):
        """The warping path of every listed pair of a located read (include/vbz_gpu.h: vbz_gpu_locate_path_batch): pairs int32 [p, 4] =
        (read, target, begin, end) on the device with [begin, end) in TARGET coordinates (match_best's table over a locate span arena, or
        any other: it is untrusted), query / valid / target / target_len / locate as for locate() (valid is required: query_valid() makes
        the fused calls') -> (hit int32 [p, 4] = (cost, end, start, rows), rows int32 [p, query_len, 2] = the target levels [begin, end)
        of every sample of the read's prefix, {0, 0} behind it) on the device.  A pair's window is at most max_width levels (a multiple of
        8, 8 ... 65536; it sizes the scratch).  A pair outside the rules gets the empty verdict.  No synchronisation."""
        return self._align_path(locate or Locate(query_len=int(query.shape[1])), query, valid, target, target_len, pairs, max_width, hit, rows)

    def _align_path(self, rule, query, valid, levels, levels_len, pairs, max_width, hit, rows):
        """match_path() and locate_path(): rule a Match or a Locate, levels / levels_len its references or targets.  The two differ in the
        entry, in valid (a Match may leave it None, a Locate needs it) and in what rows has one row for: a Match every reference row
        (ref_stride), a Locate every sample of the query (query_len)"""
        n, p, matching = int(query.shape[0]), int(pairs.shape[0]), isinstance(rule, Match)
        al = rule.c_struct(levels, levels_len)
        N = int(al.query_len)
        table("query", query, torch.float32, self.device, shape=(n, N))
        table("valid", valid, torch.int32, self.device, numel=n, none=matching)
        table("pairs", pairs, torch.int32, self.device, shape=(p, 4))
        hit = output("hit", hit, torch.int32, self.device, (p, 4))
        rows = output("rows", rows, torch.int32, self.device, (p, int(al.ref_stride) if matching else N, 2))
        path = _lib.GpuMatchPath(int(max_width), 0, 0)
        self._call("match_path_batch" if matching else "locate_path_batch", p, n, query.data_ptr(), ptr(valid), ctypes.byref(al), pairs.data_ptr(),
                   ctypes.byref(path), hit.data_ptr(), rows.data_ptr())
        return hit, rows

    def query_valid(self, result, query_len, begin=None, end=None, out=None):
        """The valid[] that the fused match and locate calls derive for themselves (include/vbz_gpu.h: vbz_gpu_query_valid_batch): result
        int32 [n] on the device, what such a call left (T x 4 bytes or an error; over POD5 reads its read_result), begin / end the call's
        range tables -> int32 [n] = min(T', query_len), 0 for an error, on the device (`out` when given).  No synchronisation."""
        n = int(table("result", result, torch.int32, self.device).numel())
        g, keep = self._ranges(n, begin, end, None)
        out = output("out", out, torch.int32, self.device, n)
        self._call("query_valid_batch", n, result.data_ptr(), ref(g), int(query_len), out.data_ptr())
        return out

    # -- event-space alignment (include/vbz_gpu.h: vbz_gpu_events_query_batch, vbz_gpu_locate_levels_batch) ------
    def events_query(self, event_first, records, query_len, min_n=0, result=None, index=True, query=None, valid=None):
        """The event records as the query arena of the alignment calls (include/vbz_gpu.h: vbz_gpu_events_query_batch): event_first int64
        [n + 1] and records int32 [rows, 4] on the device (the event call's arena: mean, sd, n, 0) -> (query float32 [n, query_len] = the
        means of each read's first query_len events with n >= min_n, +0 behind them, valid int32 [n] = their count, index int32 [n,
        query_len] = their row numbers within the read; None with index=False) on the device.  result int32 [n] (optional): a read with
        an error verdict gets valid 0.  query, valid and index may be given.  No synchronisation."""
        n, N = int(event_first.numel()) - 1, int(query_len)
        table("event_first", event_first, torch.int64, self.device, at_least=1)
        table("records", records, torch.int32, self.device, shape=(None, 4))
        table("result", result, torch.int32, self.device, numel=n, none=True)
        query = output("query", query, torch.float32, self.device, (n, N))
        valid = output("valid", valid, torch.int32, self.device, n)
        index = output("index", index, torch.int32, self.device, (n, N), three_state=True)
        ev = _lib.GpuEvents()
        ev.event_rows, ev.event_first = int(records.shape[0]), event_first.data_ptr()
        q = _lib.GpuEventsQuery(N, int(min_n), 0, 0)
        self._call("events_query_batch", n, ptr(result), ctypes.byref(ev), records.data_ptr() if int(records.shape[0]) else None, ctypes.byref(q),
                   query.data_ptr(), valid.data_ptr(), ptr(index))
        return query, valid, index

    def locate_levels(self, pairs, hit, rows, event_first, start, records, moments, max_width, index=None, n_levels=None, levels=None):
        """The path of every listed pair as a table per target level (include/vbz_gpu.h: vbz_gpu_locate_levels_batch): pairs int32 [p, 4],
        hit int32 [p, 4] and rows int32 [p, query_len, 2] as locate_path() took and left them; event_first int64 [n + 1], start int32
        [rows], records int32 [rows, 4] and moments int64 [rows, 2] the event call's tables; index int32 [n, query_len] the table of
        events_query() (None: entry k is the read's row k) -> (n_levels int32 [p], levels int32 [p, max_width, 8]: per target level of the
        pair's stretch (first_sample, end_sample, n_samples, n_entries, sum as two words, sumsq as two words), zeros behind n_levels[p]
        rows; levels.view(torch.int64)[..., 2:] are the exact sums) on the device.  max_width: a multiple of 8, 8 ... 65536, at least the
        widest stretch.  A pair outside the rules gets n_levels 0.  No synchronisation."""
        p, N, W = int(pairs.shape[0]), int(rows.shape[1]), int(max_width)
        n = int(event_first.numel()) - 1
        ev, keep = self._events(n, event_first, start)
        R = int(ev.event_rows)
        for name, t, shape in (("pairs", pairs, (p, 4)), ("hit", hit, (p, 4)), ("rows", rows, (p, N, 2)), ("records", records, (R, 4))):
            table(name, t, torch.int32, self.device, shape=shape)
        table("moments", moments, torch.int64, self.device, shape=(R, 2))
        table("index", index, torch.int32, self.device, shape=(n, N), none=True)
        n_levels = output("n_levels", n_levels, torch.int32, self.device, p)
        levels = output("levels", levels, torch.int32, self.device, (p, W, 8))
        self._call("locate_levels_batch", p, n, N, W, pairs.data_ptr(), hit.data_ptr(), rows.data_ptr(), ptr(index), ctypes.byref(ev),
                   records.data_ptr() if R else None, moments.data_ptr() if R else None, n_levels.data_ptr(), levels.data_ptr())
        return n_levels, levels

    # -- pore model: target levels from bases, new constants along the path (include/vbz_gpu.h: vbz_gpu_squiggle_batch, vbz_gpu_levels_fit_batch)
    def squiggle(self, seq, seq_len, model, k, target_stride, quant=32.0, both=False, reversed=False, level=False, target=None, target_len=None,
                 masked=None):
        """Target levels from bases (include/vbz_gpu.h: vbz_gpu_squiggle_batch): seq uint8 [S, seq_stride] ASCII, seq_len int32 [S] and model
        float32 [4 ** k] on the device -> (target int8 [rows, target_stride], target_len int32 [rows], masked int32 [rows], level float32
        [rows, target_stride] or None) on the device, rows = S, or 2 S with both (row 2s the sequence, row 2s + 1 its reverse complement);
        reversed: levels in 3'->5' order.  target and target_len are what the locate calls take.  level: True, False or a tensor; target,
        target_len and masked may be given.  No synchronisation."""
        S, k, T = int(seq.shape[0]), int(k), int(target_stride)
        rows = 2 * S if both else S
        table("seq", seq, torch.uint8, self.device, shape=(None, None))
        table("seq_len", seq_len, torch.int32, self.device, numel=S)
        assert 1 <= k <= 9, k
        table("model", model, torch.float32, self.device, numel=4 ** k)
        target = output("target", target, torch.int8, self.device, (rows, T))
        target_len = output("target_len", target_len, torch.int32, self.device, rows)
        masked = output("masked", masked, torch.int32, self.device, rows)
        level = output("level", level, torch.float32, self.device, (rows, T), three_state=True)
        sq = _lib.GpuSquiggle(k, S, int(seq.shape[1]), T, (_lib.SQUIGGLE_BOTH if both else 0) | (_lib.SQUIGGLE_REVERSED if reversed else 0), float(quant),
                              seq.data_ptr(), seq_len.data_ptr(), model.data_ptr())
        self._call("squiggle_batch", ctypes.byref(sq), target.data_ptr(), target_len.data_ptr(), masked.data_ptr(), ptr(level))
        return target, target_len, masked, level

    def levels_fit(self, pairs, hit, n_levels, levels, target, target_len, n_reads, locate=None, min_samples=0, max_entries=0, prior=None, sums=False,
                   out=None, offset=None, scale=None):
        """New constants per pair from the table per level (include/vbz_gpu.h: vbz_gpu_levels_fit_batch): pairs int32 [p, 4], hit int32
        [p, 4], n_levels int32 [p] and levels int32 [p, max_width, 8] as locate_levels() took and left them; target int8 [G, target_stride]
        and target_len int32 [G] the chain's targets; prior float32 [n_reads, 2] = (shift, scale) as the normalising calls write it, or
        None -> (out int32 [p, 4] = (offset and scale as float32 bits, used, ok), offset float32 [p], scale float32 [p], sums int64 [p, 4] =
        (Sg, Sgg, Sq, Sgq) or None) on the device.  offset and scale are what signal_events() and the other typed decodes take as
        per-read tables when pairs came from match_best().  sums: True, False or a tensor; out, offset and scale may be given.  No
        synchronisation."""
        p, W, n = int(pairs.shape[0]), int(levels.shape[1]), int(n_reads)
        loc = (locate or Locate()).c_struct(target, target_len)
        assert target.device == self.device
        for name, t, shape in (("pairs", pairs, (p, 4)), ("hit", hit, (p, 4)), ("n_levels", n_levels, (p,)), ("levels", levels, (p, W, 8))):
            table(name, t, torch.int32, self.device, shape=shape)
        table("prior", prior, torch.float32, self.device, shape=(n, 2), none=True)
        out = output("out", out, torch.int32, self.device, (p, 4))
        offset = output("offset", offset, torch.float32, self.device, p)
        scale = output("scale", scale, torch.float32, self.device, p)
        sums = output("sums", sums, torch.int64, self.device, (p, 4), three_state=True)
        fit = _lib.GpuLevelsFit(W, int(min_samples), int(max_entries), 0)
        self._call("levels_fit_batch", p, n, ctypes.byref(loc), pairs.data_ptr(), hit.data_ptr(), n_levels.data_ptr(), levels.data_ptr(), ctypes.byref(fit),
                   ptr(prior), out.data_ptr(), offset.data_ptr(), scale.data_ptr(), ptr(sums))
        return out, offset, scale, sums

    # -- the pile-up across reads: per-position and per-k-mer sums, a model update (include/vbz_gpu_pile.h) ------
    def squiggle_kmers(self, seq, seq_len, k, target_stride, both=False, reversed=False, kmer=None, target_len=None):
        """The k-mer index under every target position (include/vbz_gpu_pile.h: vbz_gpu_squiggle_kmers_batch): seq, seq_len, k,
        target_stride, both and reversed as for squiggle() -> (kmer int32 [rows, target_stride] = the index squiggle() would look up at
        each position, _lib.KMER_MARK (-1 as int32) where it would count a masked k-mer and at and behind target_len, target_len int32
        [rows]) on the device.  kmer and target_len may be given.  No synchronisation."""
        S, k, T = int(seq.shape[0]), int(k), int(target_stride)
        rows = 2 * S if both else S
        table("seq", seq, torch.uint8, self.device, shape=(None, None))
        table("seq_len", seq_len, torch.int32, self.device, numel=S)
        kmer = output("kmer", kmer, torch.int32, self.device, (rows, T))
        target_len = output("target_len", target_len, torch.int32, self.device, rows)
        sq = _lib.GpuSquiggle(k, S, int(seq.shape[1]), T, (_lib.SQUIGGLE_BOTH if both else 0) | (_lib.SQUIGGLE_REVERSED if reversed else 0), 1.0,
                              seq.data_ptr(), seq_len.data_ptr(), None)
        self._call("squiggle_kmers_batch", ctypes.byref(sq), kmer.data_ptr(), target_len.data_ptr())
        return kmer, target_len

    def levels_pile(self, pairs, hit, n_levels, levels, target, target_len, n_reads, fix=256.0, fit=None, require_ok=False, clear=False, locate=None,
                    min_samples=0, max_entries=0, pile=None):
        """Every pair's levels added into their target positions (include/vbz_gpu_pile.h: vbz_gpu_levels_pile_batch): pairs, hit, n_levels,
        levels, target, target_len, n_reads, locate, min_samples and max_entries as for levels_fit(); fit int32 [p, 4] its `out` table (None:
        offset 0, scale 1), require_ok: pairs without a good fit contribute nothing -> pile int64 [4, G, target_stride] on the device: the
        planes (count word = kept + 2^32 skipped, n_samples, sum, sumsq) of u = rint(((mean + offset) * scale) * fix) per kept level.
        pile=None makes a zeroed arena; a given one is added to, after clearing it with clear=True.  No synchronisation."""
        p, W = int(pairs.shape[0]), int(levels.shape[1])
        loc = (locate or Locate()).c_struct(target, target_len)
        assert target.device == self.device
        for name, t, shape in (("pairs", pairs, (p, 4)), ("hit", hit, (p, 4)), ("n_levels", n_levels, (p,)), ("levels", levels, (p, W, 8))):
            table(name, t, torch.int32, self.device, shape=shape)
        table("fit", fit, torch.int32, self.device, shape=(p, 4), none=True)
        clear = bool(clear) or pile is None
        pile = output("pile", pile, torch.int64, self.device, (4, int(target.shape[0]), int(target.shape[1])))
        par = _lib.GpuLevelsPile(W, int(min_samples), int(max_entries), (_lib.PILE_CLEAR if clear else 0) | (_lib.PILE_REQUIRE_OK if require_ok else 0),
                                 float(fix), 0, 0, 0)
        self._call("levels_pile_batch", p, int(n_reads), ctypes.byref(loc), pairs.data_ptr(), hit.data_ptr(), n_levels.data_ptr(), levels.data_ptr(),
                   ctypes.byref(par), ptr(fit), pile.data_ptr())
        return pile

    def pile_kmers(self, pile, kmer, target_len, k, clear=False, direct=False, kmer_pile=None):
        """The position cells added into the cells of their k-mers (include/vbz_gpu_pile.h: vbz_gpu_pile_kmers_batch): pile int64 [4, G,
        target_stride] of levels_pile(), kmer int32 [G, target_stride] and target_len int32 [G] of squiggle_kmers() -> kmer_pile int64 [4,
        4 ** k] on the device.  kmer_pile=None makes a zeroed arena; a given one is added to, after clearing it with clear=True.  direct:
        global adds whatever k is.  No synchronisation."""
        G, T, k = int(kmer.shape[0]), int(kmer.shape[1]), int(k)
        assert 1 <= k <= 9, k
        table("pile", pile, torch.int64, self.device, shape=(4, G, T))
        table("kmer", kmer, torch.int32, self.device, shape=(G, T))
        table("target_len", target_len, torch.int32, self.device, numel=G)
        clear = bool(clear) or kmer_pile is None
        kmer_pile = output("kmer_pile", kmer_pile, torch.int64, self.device, (4, 4 ** k))
        par = _lib.GpuPileKmers(k, G, T, (_lib.PILE_CLEAR if clear else 0) | (_lib.PILE_DIRECT if direct else 0))
        self._call("pile_kmers_batch", ctypes.byref(par), target_len.data_ptr(), kmer.data_ptr(), pile.data_ptr(), kmer_pile.data_ptr())
        return kmer_pile

    def model_update(self, kmer_pile, prior, k, fix=256.0, min_obs=0, sd=False, model=None):
        """A new k-mer table from the k-mer pile (include/vbz_gpu_pile.h: vbz_gpu_model_update_batch): kmer_pile int64 [4, 4 ** k] of
        pile_kmers(), prior float32 [4 ** k] -> (model float32 [4 ** k] = mean / fix where the k-mer has max(min_obs, 1) kept observations,
        the prior's bits elsewhere; sd float32 [4 ** k] or None) on the device.  model may be given, and may be prior; sd: True, False or a
        tensor.  What squiggle() takes as its model.  No synchronisation."""
        k = int(k)
        assert 1 <= k <= 9, k
        table("kmer_pile", kmer_pile, torch.int64, self.device, shape=(4, 4 ** k))
        table("prior", prior, torch.float32, self.device, numel=4 ** k)
        model = output("model", model, torch.float32, self.device, 4 ** k)
        sd = output("sd", sd, torch.float32, self.device, 4 ** k, three_state=True)
        par = _lib.GpuModelUpdate(k, int(min_obs), 0, float(fix))
        self._call("model_update_batch", ctypes.byref(par), kmer_pile.data_ptr(), prior.data_ptr(), model.data_ptr(), ptr(sd))
        return model, sd

    # -- signal events (include/vbz_gpu.h: vbz_gpu_events) ---------------------------------------------
    def _events(self, n, event_first, start):
        """(the C struct, the tables it points to) of n reads' events: event_first int64 [n + 1] on the device; start int32 [rows] on the
        device (uint32 bits), or any sequence of values 0 ... 0xFFFFFFFF"""
        table("event_first", event_first, torch.int64, self.device, numel=n + 1)
        start = wrap_u32(start).to(self.device).contiguous()
        ev = _lib.GpuEvents()
        ev.event_rows, ev.event_first = int(start.numel()), event_first.data_ptr()
        ev.start = start.data_ptr() if int(start.numel()) else None
        return ev, (event_first, start)

    def _signal_events(self, n, src, src_off, src_size, dst_off, dst_cap, dst_bytes, result, opts, sized, event_first, start, scale, offset, signed,
                       norm, norm_out, begin, end, stats, moments, arena, r=None):
        ev, keep_e = self._events(n, event_first, start)
        rows = int(ev.event_rows)
        g, keep_g = self._ranges(n, begin, end, stats)
        m, ss = self._norm_args(n, norm, norm_out, scale, offset) if norm is not None else (None, None)
        f = self._signal_format(torch.float32, n, scale, offset, signed)
        arena = output("arena", arena, torch.int32, self.device, (rows, 4))
        moments = output("moments", moments, torch.int64, self.device, (rows, 2), three_state=True)
        self._typed(src, src_off, src_size, None, dst_off, dst_cap, result, opts, sized, dst_bytes, f=f, m=m, ss=ss, g=g, r=r, ev=ev, out=arena, moments=moments)
        records = (arena[:, 0].view(torch.float32), arena[:, 1].view(torch.float32), arena[:, 2])
        return records if moments is None else records + (moments,)

    def signal_events(self, src, src_off, src_size, dst_off, dst_cap, result, opts, event_first, start, scale=None, offset=None, signed=True,
                      sized=False, norm=None, norm_out=None, begin=None, end=None, stats=None, moments=False, arena=None):
        """One record per caller-listed event of every read, with no sample stored (include/vbz_gpu.h: vbz_gpu_signal_events_batch) ->
        (mean float32 [rows], sd float32 [rows], n int32 [rows]), views of one int32 [rows, 4] arena (`arena` when given); with
        moments=True (or an int64 [rows, 2] tensor) also the exact (sum x, sum x^2) per row.  Read i owns rows event_first[i] ...
        event_first[i + 1] - 1 (int64 [n + 1] on the device); event c begins at sample start[c] of the read's signal -- of its range with
        begin / end -- and ends where the next one begins, the read's last at the signal's end (starts sorted within a read; uint32).
        mean = (m + offset) * scale and sd = r * |scale| in float64, rounded once; with norm= the read's own {-shift, 1 / scale}
        (norm_out: float32 [n, 2], filled with (shift, scale)).  dst_off / dst_cap: the int16 layout of the reads (nothing is stored);
        result[i] is what decompress gives.  No synchronisation."""
        n = int(src_off.numel())
        return self._signal_events(n, src, src_off, src_size, dst_off, dst_cap, self._extent(n, dst_off, dst_cap), result, opts, sized, event_first, start,
                                   scale, offset, signed, norm, norm_out, begin, end, stats, moments, arena)

    # -- POD5 reads of several rows (include/vbz_gpu.h: vbz_gpu_pod5_reads) ---------------------------
    def _pod5_reads(self, n_rows, read_first_row, read_result):
        """(the C struct, first_row int32 [n_reads + 1] on the device, read_result) of rows grouped by read_first_row: the first row of
        every read, ascending from 0 (a tensor or a sequence of n_reads entries; the last read owns the rows up to the end)."""
        first = torch.as_tensor(read_first_row, dtype=torch.int64).reshape(-1).to(self.device)
        n_reads = int(first.numel())
        first_row = torch.cat([first, torch.tensor([n_rows], dtype=torch.int64, device=self.device)]).to(torch.int32).contiguous()
        read_result = output("read_result", read_result, torch.int32, self.device, n_reads, at_least=True)
        r = _lib.GpuPod5Reads()
        r.n_reads, r.first_row, r.read_result = n_reads, first_row.data_ptr(), read_result.data_ptr()
        return r, first_row, read_result

    def _row_layout(self, row_samples):
        """the int16 layout that describes reads (or rows) of row_samples samples: (dst_off int64 [n + 1], dst_off[n] = the total; dst_cap int32 [n])"""
        n = int(row_samples.numel())
        table("row_samples", row_samples, torch.int32, self.device)
        dst_off = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
        if n:
            dst_off[1:] = torch.cumsum(row_samples.to(torch.int64) * 2, 0)
        return dst_off, (row_samples.to(torch.int64) * 2).to(torch.int32)

    def pod5_decompress_chunks(self, src, src_off, src_size, row_samples, read_first_row, result, chunk_len, step, mode="pad", end_align=1, pad=0.0,
                               dtype=torch.float16, scale=None, offset=None, signed=True, norm=None, norm_out=None, begin=None, end=None, stats=None):
        """Decode POD5 signal rows, grouped into reads by read_first_row, straight into model-input chunks of the READS (include/vbz_gpu.h:
        vbz_gpu_pod5_decompress_chunks_batch) -> (chunks [total, chunk_len], chunk_first int64 [n_reads + 1], chunk_info int32 [total, 2] =
        (read, start sample), read_result int32 [n_reads]).  row_samples: int32 on the device, one per row; result: int32 per ROW.  scale /
        offset / norm_out are per read.  One synchronisation.  begin / end / stats: as for decompress_chunks, per READ, in positions
        of the read's concatenated signal (vbz_gpu_pod5_decompress_chunks_range_batch)."""
        n = int(src_off.numel())
        assert int(row_samples.numel()) == n
        opts = pod5_options()
        ch = self._chunking(chunk_len, step, mode, end_align, pad)
        r, first_row, read_result = self._pod5_reads(n, read_first_row, None)
        g, keep = self._ranges(r.n_reads, begin, end, stats)
        read_samples = torch.empty(r.n_reads, dtype=torch.int32, device=self.device)
        dst_off, dst_cap = self._row_layout(row_samples)
        self._call("pod5_read_samples_batch", n, row_samples.data_ptr(), ctypes.byref(r), read_samples.data_ptr())
        laid = read_samples if g is None else self.range_samples(read_samples, begin=keep[0], end=keep[1])
        chunk_first, chunk_info, host = self._chunk_tables(laid, ch, True, also=dst_off[-1])
        chunks = self._chunk_arena(host[0], chunk_len, dtype)
        assert dtype in self._SIGNAL_TYPES
        m, ss = self._norm_args(r.n_reads, norm, norm_out, scale, offset) if norm is not None else (None, None)
        f = self._signal_format(dtype, r.n_reads, scale, offset, signed)
        self._typed(src, src_off, src_size, None, dst_off[:n], dst_cap, result, opts, dst_bytes=host[1], f=f, ch=ch, chunk_first=chunk_first, chunks=chunks,
                    m=m, ss=ss, g=g, r=r)
        return chunks, chunk_first, chunk_info, read_result

    def pod5_decompress_windows(self, src, src_off, src_size, row_samples, read_first_row, result, window_first, start, window_len, pad=0.0,
                                dtype=torch.float16, scale=None, offset=None, signed=True, norm=None, norm_out=None, begin=None, end=None, stats=None,
                                read_result=None):
        """decompress_windows over POD5 signal rows grouped into reads by read_first_row (include/vbz_gpu.h:
        vbz_gpu_pod5_decompress_windows_batch): window_first, scale / offset / norm_out and begin / end are per READ, the positions those of
        the read's concatenated signal; result is per ROW, read_result (int32 [n_reads] on the device, optional) per read."""
        n = int(src_off.numel())
        assert int(row_samples.numel()) == n
        r, first_row, read_result = self._pod5_reads(n, read_first_row, read_result)
        dst_off, dst_cap = self._row_layout(row_samples)
        return self._decode_windows(r.n_reads, src, src_off, src_size, dst_off[:n], dst_cap, int(dst_off[-1].item()), result, pod5_options(), False,
                                    window_first, start, window_len, pad, dtype, scale, offset, signed, norm, norm_out, begin, end, stats, r=r)

    def pod5_signal_events(self, src, src_off, src_size, row_samples, read_first_row, result, event_first, start, scale=None, offset=None, signed=True,
                           norm=None, norm_out=None, begin=None, end=None, stats=None, moments=False, arena=None, read_result=None):
        """signal_events over POD5 signal rows grouped into reads by read_first_row (include/vbz_gpu.h: vbz_gpu_pod5_signal_events_batch):
        event_first, scale / offset / norm_out and begin / end are per READ, the positions those of the read's concatenated signal; result
        is per ROW, read_result (int32 [n_reads] on the device, optional) per read."""
        n = int(src_off.numel())
        assert int(row_samples.numel()) == n
        r, first_row, read_result = self._pod5_reads(n, read_first_row, read_result)
        dst_off, dst_cap = self._row_layout(row_samples)
        return self._signal_events(r.n_reads, src, src_off, src_size, dst_off[:n], dst_cap, int(dst_off[-1].item()), result, pod5_options(), False,
                                   event_first, start, scale, offset, signed, norm, norm_out, begin, end, stats, moments, arena, r=r)

    def pod5_signal_norm(self, src, src_off, src_size, row_samples, read_first_row, result, norm, shift_scale=None, signed=True, begin=None,
                         end=None, stats=None):
        """Every READ's normalisation constants alone (vbz_gpu_pod5_signal_norm_batch) -> (shift_scale float32 [n_reads, 2], read_result).
        begin / end: the statistics of that range of every read's concatenated signal (vbz_gpu_pod5_signal_norm_range_batch)."""
        n = int(src_off.numel())
        opts = pod5_options()
        r, first_row, read_result = self._pod5_reads(n, read_first_row, None)
        g, keep = self._ranges(r.n_reads, begin, end, stats)
        shift_scale = output("shift_scale", shift_scale, torch.float32, self.device, (r.n_reads, 2))
        m, ss = self._norm_args(r.n_reads, norm, shift_scale, None, None)
        dst_off, dst_cap = self._row_layout(row_samples)
        self._typed(src, src_off, src_size, None, dst_off[:n], dst_cap, result, opts, dst_bytes=dst_off[-1].item(), signed=signed, m=m, ss=ss, g=g, r=r)
        return shift_scale, read_result

    def pod5_signal_trim(self, src, src_off, src_size, row_samples, read_first_row, result, norm, trim=None, out=None, shift_scale=None,
                         signed=True, begin=None, end=None, stats=None):
        """Every READ's trim point over its concatenated signal (vbz_gpu_pod5_signal_trim_batch) -> (begin int32 [n_reads], read_result),
        or (begin, shift_scale, read_result) with shift_scale (True, or a float32 [n_reads, 2] tensor).  The arguments are signal_trim's,
        per read; result is per ROW."""
        n = int(src_off.numel())
        opts = pod5_options()
        r, first_row, read_result = self._pod5_reads(n, read_first_row, None)
        g, keep = self._ranges(r.n_reads, begin, end, stats)
        t, out, shift_scale = self._trim_args(r.n_reads, trim, out, shift_scale)
        m, ss = self._norm_args(r.n_reads, norm, shift_scale, None, None)
        dst_off, dst_cap = self._row_layout(row_samples)
        self._typed(src, src_off, src_size, None, dst_off[:n], dst_cap, result, opts, dst_bytes=dst_off[-1].item(), signed=signed, m=m, ss=ss, g=g, r=r,
                    t=t, out=out)
        return (out, read_result) if shift_scale is None else (out, shift_scale, read_result)

    def pod5_signal_segment(self, src, src_off, src_size, row_samples, read_first_row, result, segmentation=None, start_cap=None, signed=True,
                            begin=None, end=None, event_first=None, start=None, read_result=None):
        """signal_segment over POD5 signal rows grouped into reads by read_first_row (vbz_gpu_pod5_signal_segment_batch) ->
        (event_first int64 [n_reads + 1], start, read_result): the tables and begin / end are per READ, the positions those of the read's
        concatenated signal; result is per ROW."""
        n = int(src_off.numel())
        assert int(row_samples.numel()) == n
        r, first_row, read_result = self._pod5_reads(n, read_first_row, read_result)
        g, keep = self._ranges(r.n_reads, begin, end, None)
        dst_off, dst_cap = self._row_layout(row_samples)
        if start_cap is None and start is None:   # (the bound: 2 + T / (radius + 1) per read, at most 2 n_reads + all samples / (radius + 1))
            radius = (segmentation or Segmentation()).radius
            start_cap = 2 * r.n_reads + int(torch.as_tensor(row_samples).to(torch.int64).sum().item()) // (radius + 1)
        sg, event_first, start = self._segment_args(r.n_reads, segmentation, None, start_cap, event_first, start)
        self._typed(src, src_off, src_size, None, dst_off[:n], dst_cap, result, pod5_options(), dst_bytes=dst_off[-1].item(), signed=signed, g=g, r=r,
                    sg=sg, event_first=event_first, start=start)
        return event_first, start, read_result

    def pod5_signal_spans(self, src, src_off, src_size, row_samples, read_first_row, result, spans=None, edge_cap=None, signed=True, begin=None,
                          end=None, edge_first=None, edge=None, norm=None, level=None, shift_scale=None, stats=None, read_result=None):
        """signal_spans over POD5 signal rows grouped into reads by read_first_row (vbz_gpu_pod5_signal_spans_batch) ->
        (edge_first int64 [n_reads + 1], edge, read_result), with shift_scale behind them when asked for: the tables, level and begin / end
        are per READ, the positions those of the read's concatenated signal; result is per ROW."""
        n = int(src_off.numel())
        assert int(row_samples.numel()) == n
        r, first_row, read_result = self._pod5_reads(n, read_first_row, read_result)
        g, keep = self._ranges(r.n_reads, begin, end, stats)
        dst_off, dst_cap = self._row_layout(row_samples)
        if edge_cap is None and edge is None:   # (the bound per read is at most the bound of all samples plus one span a read)
            sp0 = spans or Spans()
            edge_cap = 2 * (r.n_reads + int(torch.as_tensor(row_samples).to(torch.int64).sum().item()) // (sp0.min_length + sp0.merge_gap + 1))
        sp, edge_first, edge, m, ss, shift_scale = self._span_args(r.n_reads, spans, None, edge_cap, edge_first, edge, norm, level, shift_scale)
        self._typed(src, src_off, src_size, None, dst_off[:n], dst_cap, result, pod5_options(), dst_bytes=dst_off[-1].item(), signed=signed, m=m, ss=ss, g=g,
                    r=r, sp=sp, event_first=edge_first, start=edge)
        return (edge_first, edge, read_result) if shift_scale is None else (edge_first, edge, read_result, shift_scale)

    def pod5_decompress_signal_norm(self, src, src_off, src_size, row_samples, read_first_row, result, norm, dtype=torch.float32, signed=True,
                                    norm_out=None, align=16):
        """Decode POD5 rows into the contiguous signal of their reads (pod5_read_layout), every row normalised by its READ's statistics
        (vbz_gpu_pod5_decompress_signal_norm_batch) -> (out: 1-D `dtype`, Pod5Layout in bytes of out, read_result).  row_samples and
        read_first_row: host sequences or tensors (the layout is computed on the host)."""
        assert dtype in self._SIGNAL_TYPES, dtype
        n = int(src_off.numel())
        opts = pod5_options()
        elem = torch.empty(0, dtype=dtype).element_size()
        lay = pod5_read_layout(torch.as_tensor(row_samples).cpu(), torch.as_tensor(read_first_row).cpu(), elem=elem, align=align, device=self.device)
        r, first_row, read_result = self._pod5_reads(n, read_first_row, None)
        m, ss = self._norm_args(r.n_reads, norm, norm_out, None, None)
        f = self._signal_format(dtype, r.n_reads, None, None, signed)
        out = torch.empty(lay.total // elem + 32, dtype=dtype, device=self.device)
        self._typed(src, src_off, src_size, out.view(torch.uint8), lay.dst_off, lay.dst_cap, result, opts, f=f, m=m, ss=ss, r=r)
        return out, lay, read_result

    # -- synthetic workload ----------------------------------------------------------
    def synth_lengths(self, seed, first_read, n_reads):
        out = torch.empty(n_reads, dtype=torch.int32, device=self.device)
        self._call("synth_lengths", seed, first_read, n_reads, out.data_ptr())
        return out

    def synth_signal(self, seed, first_read, dst, off, length):
        self._call("synth_signal", seed, first_read, int(off.numel()), dst.data_ptr(), off.data_ptr(), length.data_ptr())

    def synth_u32(self, seed, first_read, dst, off, length):
        self._call("synth_u32", seed, first_read, int(off.numel()), dst.data_ptr(), off.data_ptr(), length.data_ptr())

    # -- profiling -------------------------------------------------------------------------------
    def profile(self, enable=True):
        self.L.vbz_gpu_profile_enable(self.ctx, int(enable))

    def profile_reset(self):
        self.L.vbz_gpu_profile_reset(self.ctx)

    def profile_read(self):
        cap = 32
        names = (ctypes.c_char_p * cap)()
        launches = (ctypes.c_uint32 * cap)()
        ms = (ctypes.c_double * cap)()
        k = self.L.vbz_gpu_profile_read(self.ctx, names, launches, ms, cap)
        return {names[i].decode(): (int(launches[i]), float(ms[i])) for i in range(min(k, cap))}

    def decode_paths(self):
        """(frames, batched, walked) of the last decompress launch group: include/vbz_gpu.h, vbz_gpu_decode_paths."""
        b, w = ctypes.c_uint32(0), ctypes.c_uint32(0)
        n = self.L.vbz_gpu_decode_paths(self.ctx, ctypes.byref(b), ctypes.byref(w))
        if n < 0:
            raise RuntimeError("vbz_gpu_decode_paths failed")
        return n, int(b.value), int(w.value)

    def decode_literals_ahead(self):
        """walked frames of the last decompress launch group whose first block's literals were decoded beside the walk: vbz_gpu_decode_literals_ahead."""
        n = self.L.vbz_gpu_decode_literals_ahead(self.ctx)
        if n < 0:
            raise RuntimeError("vbz_gpu_decode_literals_ahead failed")
        return n

    def decode_span_paths(self):
        """(frames, by_spans) of the last decompress launch group on the large-read path: include/vbz_gpu.h, vbz_gpu_decode_span_paths."""
        b = ctypes.c_uint32(0)
        n = self.L.vbz_gpu_decode_span_paths(self.ctx, ctypes.byref(b))
        if n < 0:
            raise RuntimeError("vbz_gpu_decode_span_paths failed")
        return n, int(b.value)

    def synchronize(self):
        self._rc(self.L.vbz_gpu_synchronize(self.ctx), "synchronize")


def layout(sizes, align=64, device="cpu"):
    """Offsets (int64) for slots of the given byte sizes, each aligned to `align`; returns (off, total)."""
    sizes = torch.as_tensor(sizes, dtype=torch.int64)
    padded = (sizes + (align - 1)) // align * align
    off = torch.zeros_like(padded)
    if padded.numel() > 1:
        off[1:] = torch.cumsum(padded, 0)[:-1]
    total = int(padded.sum().item()) + 64
    return off.to(device), total


# -- POD5 signal rows (include/vbz_gpu.h: VBZ_GPU_VERSION_POD5) ----------------------------------------------------------------
def pod5_options(level=1):
    """CompressionOptions of POD5 signal rows: int16 samples, delta + zig-zag, svb16 + one zstd frame (levels above 1 write level-1
    frames).  Unsized calls only: a row's sample count is the file's `samples` column."""
    return _lib.CompressionOptions(True, 2, int(level), _lib.VBZ_GPU_VERSION_POD5)


def pod5_max_compressed_size(samples):
    """ZSTD_COMPRESSBOUND(ceil(samples / 8) + 2 samples): the capacity a compress slot of a row needs (pod5's compressed_signal_max_size)."""
    return int(_lib.load().vbz_gpu_pod5_max_compressed_size(int(samples)))


Pod5Layout = collections.namedtuple("Pod5Layout", "dst_off dst_cap read_off read_len total")


def pod5_read_layout(row_samples, read_first_row, elem=2, align=16, device="cpu"):
    """The decode layout of POD5 reads stored as several signal rows: the rows of a read are laid out adjacently, so that its decoded
    rows form one contiguous signal, and every read starts `align`-aligned.  row_samples: the rows' sample counts, in file order;
    read_first_row: the first row of every read (ascending from 0; read k owns rows read_first_row[k] ... read_first_row[k + 1] - 1,
    the last read the rows up to the end).  elem: bytes per decoded sample (2: int16; 4 / 2: float32 / float16 or bfloat16 of
    decompress_signal, whose offset and scale are then passed once per ROW).
    -> Pod5Layout(dst_off int64 [rows] bytes, dst_cap int32 [rows] bytes, read_off int64 [reads] bytes, read_len int64 [reads] samples,
    total bytes): read k is bytes read_off[k] ... read_off[k] + elem * read_len[k] of the destination."""
    assert align >= 1 and align & (align - 1) == 0 and elem in (2, 4), (align, elem)
    rows = torch.as_tensor(row_samples, dtype=torch.int64).reshape(-1)
    first = torch.as_tensor(read_first_row, dtype=torch.int64).reshape(-1)
    n_rows, n_reads = int(rows.numel()), int(first.numel())
    bounds = torch.cat([first, torch.tensor([n_rows], dtype=torch.int64)])
    assert (n_reads == 0 or int(first[0]) == 0) and bool((bounds[1:] >= bounds[:-1]).all()) and int(bounds[-2 if n_reads else -1]) <= n_rows, \
        "read_first_row must ascend from 0 within the rows"
    read = torch.repeat_interleave(torch.arange(n_reads, dtype=torch.int64), bounds[1:] - bounds[:-1])   # the read of every row
    row_bytes = rows * elem
    read_len = torch.zeros(n_reads, dtype=torch.int64).index_add_(0, read, rows)
    padded = (read_len * elem + (align - 1)) // align * align
    read_off = torch.zeros(n_reads, dtype=torch.int64)
    if n_reads > 1:
        read_off[1:] = torch.cumsum(padded, 0)[:-1]
    excl = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(row_bytes, 0)])   # (bytes of the rows in front of each row)
    dst_off = read_off[read] + excl[:-1] - excl[first][read]   # (... and in front of the row within its read)
    return Pod5Layout(dst_off.to(device), row_bytes.to(torch.int32).to(device), read_off.to(device), read_len.to(device), int(padded.sum().item()))

"""What the fourteen typed decode entries of include/vbz_gpu.h accept and refuse, through ctypes, on the smallest inputs that give every
argument a meaning: three int16 reads of 40, 1000 and 2500 samples (POD5: four rows of 40, 1000, 1000 and 300 samples in two reads),
chunk_len 1000, step 504, float16.  Per entry: (a) the good call, sized and unsized; (b) every single fault that applies to it, with
the return code and the vbz_gpu_last_error text written out below, and every output table still its canary afterwards -- a refused call
ends on the host, nothing is launched; (c) the NULLs an entry allows, whose outputs are those of the call with the argument present
(ranges: the whole reads; norm: a normalisation whose constants are 0 and 1); (d) a call of no reads.  The codes and messages were
recorded from the library when every entry family still had checks of its own, before typed_decode (vbz_api.hip)
became the one way in: a call with one fault keeps them byte for byte."""
import ctypes
import types

import numpy as np
import pytest
import torch

from signal_ref import table_of
from typed_support import Frames, codec, i32, sine_signal
from vbz_compression_amd import _lib, batch

pytestmark = pytest.mark.gpu

WORD, BYTE, FLOAT = 0x5A5A5A5A, 0x5A, -777.0   # the canaries: 32-bit tables, arenas, shift_scale
CHUNK_LEN, STEP = 1000, 504
READS = [40, 1000, 2500]
ROWS, FIRST_ROW = [40, 1000, 1000, 300], [0, 1, 4]
GUARD_ROWS = 2

# entry (vbz_gpu_<name>_batch): its parameters behind ctx, in the C order, and what its error text calls it
ENTRIES = {
    "decompress_signal": ("b o sized f", "signal"),
    "decompress_chunks": ("b o sized f ch chunk_first chunks chunk_rows", "chunk"),
    "decompress_chunks_norm": ("b o sized f ch chunk_first chunks chunk_rows norm ss", "chunk"),
    "decompress_chunks_range": ("b o sized f ch chunk_first chunks chunk_rows norm ss ranges", "chunk"),
    "decompress_signal_norm": ("b o sized f norm ss", "signal"),
    "signal_norm": ("b o sized is_signed norm ss", "statistics"),
    "signal_norm_range": ("b o sized is_signed norm ss ranges", "statistics"),
    "signal_trim": ("b o sized is_signed norm ranges trim ss begin", "statistics"),
    "pod5_decompress_chunks": ("b o f ch reads chunk_first chunks chunk_rows norm ss", "chunk"),
    "pod5_decompress_chunks_range": ("b o f ch reads chunk_first chunks chunk_rows norm ss ranges", "chunk"),
    "pod5_signal_norm": ("b o is_signed reads norm ss", "statistics"),
    "pod5_signal_norm_range": ("b o is_signed reads norm ss ranges", "statistics"),
    "pod5_signal_trim": ("b o is_signed reads norm ranges trim ss begin", "statistics"),
    "pod5_decompress_signal_norm": ("b o f reads norm ss", "signal"),
}
STRUCTS = ("b", "o", "f", "ch", "norm", "ranges", "reads", "trim")
NORM_OPTIONAL = ("decompress_chunks_range", "pod5_decompress_chunks", "pod5_decompress_chunks_range")
SS_REQUIRED = ("signal_norm", "signal_norm_range", "pod5_signal_norm", "pod5_signal_norm_range")   # the statistics alone
SS_REQUIRED_WITHOUT_READS = ("signal_norm", "signal_norm_range")                                   # ... refused in a call of no reads too
IDENTITY = batch.Normalization("med_mad", shift_mul=0.0, scale_mul=0.0, scale_min=1.0)             # shift 0, scale 1: the samples themselves

M_FORMAT = "signal format: NULL, unknown out_type or is_signed not 0 / 1"
M_NORM = "normalization outside its rules (method %u, reserved %u, quantiles 0 / 0, shift_mul 1, scale_mul 1.4826, shift_min -inf, scale_min 1.17549e-38)"
M_RANGES = "sample ranges outside their rules (stats %u, reserved %u)"
M_READS = "reads: NULL, reserved not 0 or a NULL first_row"
M_CHUNKING = "chunking outside the rules (chunk_len %u, step %u, mode %u, end_align %u, reserved %u)"
M_TABLES = "chunk_first or the chunk arena is NULL"
M_TRIM = ("trim outside its rules (window %u, min_elements 3, min_trim 10, max_samples %u, threshold_factor 2.4, max_fraction 1, flags %u, "
          "reserved %u; at most 4096 windows)")


_frames = {}


def frames(c, kind):
    """signal-like int16 reads compressed once by GpuCodec.compress (typed_support.Frames: the source arena and the int16 layout that
    describes the reads), with the chunk_first of the reads (POD5: of FIRST_ROW's groups of rows)"""
    if kind not in _frames:
        rng = np.random.default_rng(7)
        if kind == "pod5":
            lens, opts, sized, caps, bounds = ROWS, batch.pod5_options(), False, [batch.pod5_max_compressed_size(t) for t in ROWS], FIRST_ROW + [len(ROWS)]
        else:
            lens, opts, sized, bounds = READS, c.options(True, 2, 1, 1), kind == "sized", list(range(len(READS) + 1))
            caps = [int(c.L.vbz_max_compressed_size(2 * t, ctypes.byref(opts))) + 16 for t in READS]
        fr = Frames(c, [sine_signal(rng, t) for t in lens], opts, sized, align=16, caps=caps)
        T = [sum(lens[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]
        table = table_of(T, CHUNK_LEN, STEP, "pad", 0)
        fr.n_out, fr.rows = len(T), int(table[-1])
        fr.chunk_first = torch.from_numpy(table).to(c.device)
        fr.first_row = i32(bounds).to(c.device)
        _frames[kind] = fr
    return _frames[kind]


def make(c, name, sized=False):
    """the arguments of the entry's good call: every optional part present, every output table filled with its canary"""
    params = ENTRIES[name][0].split()
    pod5 = "reads" in params
    fr = frames(c, "pod5" if pod5 else "sized" if sized else "plain")
    dev, R = c.device, fr.n_out
    a = types.SimpleNamespace(ctx=c.ctx, fr=fr, sized=int(sized), is_signed=1, chunk_rows=fr.rows)
    a.out = {
        "result": (torch.full((fr.n,), WORD, dtype=torch.int32, device=dev), WORD),
        "read_result": (torch.full((R,), WORD, dtype=torch.int32, device=dev), WORD),
        "ss": (torch.full((R, 2), FLOAT, dtype=torch.float32, device=dev), FLOAT),
        "begin": (torch.full((R,), WORD, dtype=torch.int32, device=dev), WORD),
        "chunks": (torch.full(((fr.rows + GUARD_ROWS) * CHUNK_LEN * 2,), BYTE, dtype=torch.uint8, device=dev), BYTE),
        "dst": (torch.full((fr.dst_bytes,), BYTE, dtype=torch.uint8, device=dev), BYTE),   # float16: the int16 layout is the typed arena's
    }
    a.b = c._batch(fr.src, fr.off, fr.size, a.out["dst"][0], fr.doff, fr.dcap, a.out["result"][0])
    a.o = batch.pod5_options() if pod5 else c.options(True, 2, 1, 1)
    a.f = _lib.GpuSignalFormat()
    a.f.out_type, a.f.is_signed = _lib.VBZ_GPU_SIGNAL_F16, 1
    a.ch = c._chunking(CHUNK_LEN, STEP, "pad", 0, -7.0)
    a.chunk_first, a.chunks = fr.chunk_first.data_ptr(), a.out["chunks"][0].data_ptr()
    a.norm = batch.MED_MAD.c_struct()
    a.ss, a.begin = a.out["ss"][0].data_ptr(), a.out["begin"][0].data_ptr()
    a.keep = (torch.zeros(R, dtype=torch.int32, device=dev), torch.full((R,), -1, dtype=torch.int32, device=dev))   # the whole reads
    a.ranges = _lib.GpuSampleRanges()
    a.ranges.begin, a.ranges.end = a.keep[0].data_ptr(), a.keep[1].data_ptr()
    a.reads = _lib.GpuPod5Reads()
    a.reads.n_reads, a.reads.first_row, a.reads.read_result = R, fr.first_row.data_ptr(), a.out["read_result"][0].data_ptr()
    a.trim = batch.Trim().c_struct()
    return a


def call(c, name, a):
    """-> (return code, vbz_gpu_last_error's text behind the call)"""
    args = [ctypes.byref(getattr(a, p)) if p in STRUCTS and getattr(a, p) is not None else getattr(a, p) for p in ENTRIES[name][0].split()]
    rc = getattr(c.L, "vbz_gpu_%s_batch" % name)(a.ctx, *args)
    return rc, c.L.vbz_gpu_last_error(c.ctx).decode()


def outputs(c, a):
    c.synchronize()
    return {k: t.clone() for k, (t, _) in a.out.items()}


def written(c, a):
    """the output tables that are no longer their canary"""
    c.synchronize()
    return [k for k, (t, fill) in a.out.items() if not bool((t == fill).all())]


def arg(name, value):
    return lambda a: setattr(a, name, value)


def field(name, member, value):
    return lambda a: setattr(getattr(a, name), member, value)


def faults(name):
    """(label, the change to the good call's arguments, return code, message) of every single fault that applies to the entry"""
    params, what = ENTRIES[name][0].split(), ENTRIES[name][1]
    m_options = "unsupported options for a %s decode (integer_size must be 2, version 0, 1 or POD5)" % what
    F = [
        ("ctx NULL", arg("ctx", None), -1, None),
        ("batch NULL", arg("b", None), -1, None),
        ("options NULL", arg("o", None), -2, m_options),
        ("integer_size 4", field("o", "integer_size", 4), -2, m_options),
        ("dst_bytes 2^47", field("b", "dst_bytes", 1 << 47), -2, "declared arena extents are not plausible (src_bytes {src_bytes}, dst_bytes 140737488355328)"),
        ("src_off NULL", field("b", "src_off", None), -2, "a table or arena pointer of the batch is NULL"),
    ]
    if "reads" in params:
        F += [
            ("options not POD5's", arg("o", batch.GpuCodec.options(True, 2, 1, 1)), -2, "the calls over POD5 reads take POD5 options only"),
            ("reads NULL", arg("reads", None), -2, M_READS),
            ("reads.reserved 1", field("reads", "reserved", 1), -2, M_READS),
            ("first_row NULL", field("reads", "first_row", None), -2, M_READS),
        ]
    if "f" in params:
        F += [
            ("format NULL", arg("f", None), -2, M_FORMAT),
            ("out_type 0", field("f", "out_type", 0), -2, M_FORMAT),
            ("out_type 4", field("f", "out_type", 4), -2, M_FORMAT),
            ("is_signed 2", field("f", "is_signed", 2), -2, M_FORMAT),
        ]
        if "norm" in params:
            F.append(("scale table with norm", lambda a: setattr(a.f, "scale", a.ss), -2,
                      "a normalising decode takes no offset or scale table (the statistics give them)"))
    else:
        F.append(("is_signed 2", arg("is_signed", 2), -2, M_FORMAT))
    if "norm" in params:
        if name not in NORM_OPTIONAL:
            F.append(("norm NULL", arg("norm", None), -2, "normalization is NULL"))
        F += [
            ("method 0", field("norm", "method", 0), -2, M_NORM % (0, 0)),
            ("norm.reserved 1", field("norm", "reserved", 1), -2, M_NORM % (1, 1)),
        ]
    if "ranges" in params:
        F += [
            ("ranges.stats 2", field("ranges", "stats", 2), -2, M_RANGES % (2, 0)),
            ("ranges.reserved 1", field("ranges", "reserved", 1), -2, M_RANGES % (0, 1)),
        ]
    if "ch" in params:
        F += [
            ("chunking NULL", arg("ch", None), -2, "chunking is NULL"),
            ("chunk_len 1004", field("ch", "chunk_len", 1004), -2, M_CHUNKING % (1004, 504, 0, 0, 0)),
            ("step > chunk_len", field("ch", "step", 1008), -2, M_CHUNKING % (1000, 1008, 0, 0, 0)),
            ("mode 2", field("ch", "mode", 2), -2, M_CHUNKING % (1000, 504, 2, 0, 0)),
            ("end_align 1, pad mode", field("ch", "end_align", 1), -2, M_CHUNKING % (1000, 504, 0, 1, 0)),
            ("chunking.reserved 1", field("ch", "reserved", 1), -2, M_CHUNKING % (1000, 504, 0, 0, 1)),
            ("chunk_first NULL", arg("chunk_first", None), -2, M_TABLES),
            ("chunk arena NULL", arg("chunks", None), -2, M_TABLES),
            ("chunk arena + 8 bytes", lambda a: setattr(a, "chunks", a.chunks + 8), -2, "the chunk arena is not 16-byte aligned"),
            ("chunk_rows 2^63", arg("chunk_rows", 1 << 63), -2, "declared chunk arena is not plausible (9223372036854775808 rows of 2000 bytes)"),
        ]
    if "trim" in params:
        F += [
            ("trim NULL", arg("trim", None), -2, "trim or begin is NULL"),
            ("begin NULL", arg("begin", None), -2, "trim or begin is NULL"),
            ("window 0", field("trim", "window", 0), -2, M_TRIM % (0, 8000, 0, 0)),
            ("flags 2", field("trim", "flags", 2), -2, M_TRIM % (40, 8000, 2, 0)),
            ("trim.reserved 1", field("trim", "reserved", 1), -2, M_TRIM % (40, 8000, 0, 1)),
            ("too many windows", lambda a: (setattr(a.trim, "window", 1), setattr(a.trim, "max_samples", 1 << 31)), -2, M_TRIM % (1, 1 << 31, 0, 0)),
        ]
    if name in SS_REQUIRED:
        F.append(("shift_scale NULL", arg("ss", None), -2, "shift_scale is NULL"))
    return F


def allowed_nulls(name):
    """(label, the change, what the outputs are compared with: None -- the good call's; else the change that gives the reference;
    the outputs left out of the comparison)"""
    params = ENTRIES[name][0].split()
    A = []
    if name in NORM_OPTIONAL:
        A.append(("norm NULL", lambda a: (setattr(a, "norm", None), setattr(a, "ss", None)), lambda a: (setattr(a, "norm", IDENTITY.c_struct()), setattr(a, "ss", None)), ()))
    if "ranges" in params:
        A.append(("ranges NULL", arg("ranges", None), None, ()))
    if "ss" in params and name not in SS_REQUIRED:
        A.append(("shift_scale NULL", arg("ss", None), None, ("ss",)))
    if "ch" in params or ENTRIES[name][1] == "statistics":
        A.append(("batch->dst NULL", field("b", "dst", None), None, ()))
    return A


def same(x, y, skip=()):
    """the names of the outputs that differ (the chunk arena as float16 values: a zero's sign is not an output)"""
    views = {"chunks": torch.float16}
    return [k for k in x if k not in skip and not torch.equal(x[k].view(views.get(k, x[k].dtype)), y[k].view(views.get(k, y[k].dtype)))]


@pytest.mark.parametrize("name", list(ENTRIES))
def test_entry_accepts_and_refuses(name):
    c = codec()
    params = ENTRIES[name][0].split()
    bad = []
    # (a) the good call
    good = None
    for sized in (False, True) if "sized" in params else (False,):
        a = make(c, name, sized)
        rc, msg = call(c, name, a)
        out = outputs(c, a)
        want = [2 * t for t in a.fr.T]
        if rc != 0 or batch._u32(out["result"]) != want:
            bad.append("good call (sized %d): rc %d %r, result %r, want %r" % (sized, rc, msg, batch._u32(out["result"]), want))
        if "reads" in params and any(_lib.is_error(v) or v == WORD for v in batch._u32(out["read_result"])):
            bad.append("good call: read_result %r" % batch._u32(out["read_result"]))
        good = good or out
    # (b) single faults: refused on the host, nothing written
    for label, change, want_rc, want_msg in faults(name):
        a = make(c, name)
        before = c.L.vbz_gpu_last_error(c.ctx).decode()
        change(a)
        rc, msg = call(c, name, a)
        want_msg = before if want_msg is None else want_msg.format(src_bytes=a.fr.src.numel())   # (-1: no message is left)
        touched = written(c, a)
        if (rc, msg) != (want_rc, want_msg) or touched:
            bad.append("%s: rc %d, %r; want %d, %r; written: %r" % (label, rc, msg, want_rc, want_msg, touched))
    # (c) the NULLs the entry allows
    for label, change, reference, skip in allowed_nulls(name):
        ref = good
        if reference is not None:
            a = make(c, name)
            reference(a)
            rc, msg = call(c, name, a)
            ref = outputs(c, a)
            if rc != 0:
                bad.append("%s, the reference call: rc %d, %r" % (label, rc, msg))
        a = make(c, name)
        change(a)
        rc, msg = call(c, name, a)
        differ = same(outputs(c, a), ref, skip)
        if rc != 0 or differ:
            bad.append("%s: rc %d, %r; outputs that differ: %r" % (label, rc, msg, differ))
    # (d) no reads (POD5: no rows and no reads): nothing to do, but shift_scale is looked at first by the statistics calls without reads
    for no_ss in (False, True) if "ss" in params else (False,):
        a = make(c, name)
        a.b.n_reads = a.reads.n_reads = 0
        if no_ss:
            a.ss = None
        rc, msg = call(c, name, a)
        want_rc = -2 if no_ss and name in SS_REQUIRED_WITHOUT_READS else 0
        touched = written(c, a)
        if rc != want_rc or (rc != 0 and msg != "shift_scale is NULL") or touched:
            bad.append("no reads (shift_scale NULL: %d): rc %d, %r; want %d; written: %r" % (no_ss, rc, msg, want_rc, touched))
    assert not bad, "\n".join([name] + bad)

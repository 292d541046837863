"""What the two signal-segmentation calls refuse on the host (include/vbz_gpu.h: -2, nothing launched), each single fault with its message;
the good call; the NULLs they allow; a call of no reads; a bad first_row."""
import ctypes
import math

import numpy as np
import pytest
import torch

import pod5_reads_ref as PR
import segment_ref as S
from segment_support import CANARY32, CANARY64, SegCall, seg_struct
from typed_support import Call, Frames, codec, frames_of, ranges_struct, sine_signal, u32
from vbz_compression_amd import _lib, batch

pytestmark = pytest.mark.gpu

E_INPUT = 0xFFFFFFFE
GOOD = (3, 6, 4.0, 9.0, 2)
CAP = 4096


class Setup:
    def __init__(self):
        c = self.c = codec()
        rng = np.random.default_rng(93)
        fr = self.fr = Frames(c, [sine_signal(rng, 500) for _ in range(4)], c.options(True, 2, 1, 1))
        dev = c.device
        self.res = torch.full((fr.n,), 12345, dtype=torch.int32, device=dev)
        self.first = torch.full((8,), CANARY64, dtype=torch.int64, device=dev)
        self.start = torch.full((CAP + 8,), CANARY32, dtype=torch.int32, device=dev)
        self.b = c._batch(fr.src, fr.off, fr.size, torch.empty(0, dtype=torch.uint8, device=dev), fr.doff, fr.dcap, self.res)
        self.b.dst, self.b.dst_bytes = None, fr.dst_bytes
        rows, rfirst, frames = frames_of(22, [[600, 700], [900, 1000, 1100], [500, 20]])
        self.rows, self.rfirst = rows, rfirst
        self.pc = Call(c, frames, [len(x) for x in rows], PR.bounds(rfirst, len(rows)), "f32", None)

    def calls(self, sg, first="ok", start="ok", o=None, signed=1, g=None, which=(0, 1)):
        c, L = self.c, self.c.L
        fp = self.first.data_ptr() if first == "ok" else first
        sp = self.start.data_ptr() if start == "ok" else start
        gp = ctypes.byref(g) if g is not None else None
        sgp = ctypes.byref(sg) if sg is not None else None
        fns = [lambda: L.vbz_gpu_signal_segment_batch(c.ctx, ctypes.byref(self.b), ctypes.byref(self.fr.opts if o is None else o), 0, signed, gp, sgp, fp, sp),
               lambda: L.vbz_gpu_pod5_signal_segment_batch(c.ctx, ctypes.byref(self.pc.b), ctypes.byref(self.pc.opts), signed, ctypes.byref(self.pc.reads), gp, sgp,
                                                           fp, sp)]
        return [(fns[k](), L.vbz_gpu_last_error(c.ctx).decode()) for k in which]

    def untouched(self):
        torch.cuda.synchronize()
        assert (self.res.cpu() == 12345).all()
        assert (self.first.cpu().numpy() == CANARY64).all() and (u32(self.start) == CANARY32).all()
        assert (self.pc.result.cpu() == -8).all() and (self.pc.read_result.cpu() == -8).all()


def refused(got, text):
    for rc, msg in got:
        assert rc == -2 and text in msg, (rc, msg, text)


def test_host_refusals_launch_nothing():
    s = Setup()
    good = seg_struct(GOOD, CAP)
    refused(s.calls(None), "segmentation or event_first is NULL")
    refused(s.calls(good, first=None), "segmentation or event_first is NULL")
    refused(s.calls(good, start=None), "start is NULL with start_cap")
    faults = [(0, 6, 4.0, 9.0, 2), (33, 6, 4.0, 9.0, 2), (3, 33, 4.0, 9.0, 2), (3, 6, 4.0, 9.0, 0), (3, 6, 4.0, 9.0, 33), (3, 6, 0.0, 9.0, 2),
              (3, 6, -1.0, 9.0, 2), (3, 6, math.nan, 9.0, 2), (3, 6, math.inf, 9.0, 2), (3, 6, 4.0, 0.0, 2), (3, 6, 4.0, math.nan, 2),
              (3, 6, 4.0, -math.inf, 2)]
    for P in faults:
        refused(s.calls(seg_struct(P, CAP)), "segmentation outside its rules")
    refused(s.calls(seg_struct(GOOD, CAP, flags=1)), "segmentation outside its rules")
    refused(s.calls(seg_struct(GOOD, (1 << 46) // 4 + 1)), "declared start table is not plausible")
    # what the ranged statistics calls refuse about the options, is_signed and the ranges
    refused(s.calls(good, o=_lib.CompressionOptions(True, 4, 1, 1), which=(0,)), "unsupported options")
    refused(s.calls(good, signed=2), "is_signed not 0 / 1")
    for kw in ({"reserved": 1}, {"stats": 2}):
        g, gk = ranges_struct(s.c, [0] * 4, None, **kw)
        refused(s.calls(good, g=g), "sample ranges outside their rules")
    s.untouched()


def test_pod5_entry_refuses_other_options_and_null_reads():
    s = Setup()
    L, good = s.c.L, seg_struct(GOOD, CAP)
    rc = L.vbz_gpu_pod5_signal_segment_batch(s.c.ctx, ctypes.byref(s.pc.b), ctypes.byref(s.fr.opts), 1, ctypes.byref(s.pc.reads), None, ctypes.byref(good),
                                             s.first.data_ptr(), s.start.data_ptr())
    assert rc == -2 and "POD5 options only" in L.vbz_gpu_last_error(s.c.ctx).decode()
    rc = L.vbz_gpu_pod5_signal_segment_batch(s.c.ctx, ctypes.byref(s.pc.b), ctypes.byref(s.pc.opts), 1, None, None, ctypes.byref(good), s.first.data_ptr(),
                                             s.start.data_ptr())
    assert rc == -2 and "reads: NULL" in L.vbz_gpu_last_error(s.c.ctx).decode()
    s.untouched()


def test_the_good_call_and_the_allowed_nulls():
    s = Setup()
    c = s.c
    # the good call; a long window of 0 ignores its threshold, whatever it holds; ranges NULL or with both tables NULL
    g0, gk = ranges_struct(c, None, None)
    want, st = S.tables(s.fr.reads, None, None, GOOD)
    want1, st1 = S.tables(s.fr.reads, None, None, (3, 0, 4.0, 0.0, 2))
    sig = PR.read_signals(s.rows, s.rfirst)
    pwant, pst = S.tables(sig, None, None, GOOD)
    for sg, g, w, pw in ((seg_struct(GOOD, CAP), None, want, pwant), (seg_struct(GOOD, CAP), g0, want, pwant),
                         (seg_struct((3, 0, 4.0, math.nan, 2), CAP), None, want1, None)):
        s.first.fill_(CANARY64)
        assert [rc for rc, _ in s.calls(sg, g=g, which=(0,))] == [0], c.L.vbz_gpu_last_error(c.ctx)
        c.synchronize()
        assert s.first.cpu().numpy()[:5].tolist() == w.tolist() and (s.res.cpu() == 1000).all()
        if pw is not None:
            assert [rc for rc, _ in s.calls(sg, g=g, which=(1,))] == [0], c.L.vbz_gpu_last_error(c.ctx)
            c.synchronize()
            assert s.first.cpu().numpy()[:4].tolist() == pw.tolist() and pw[-1] > 3
    # the count-only call: start NULL with start_cap 0 -- event_first alone
    s.start.fill_(CANARY32)
    assert [rc for rc, _ in s.calls(seg_struct(GOOD, 0), start=None)] == [0, 0]
    c.synchronize()
    assert (u32(s.start) == CANARY32).all() and s.first.cpu().numpy()[:4].tolist() == pwant.tolist()
    # a call of no reads: event_first[0] = 0, nothing else; start may be anything
    b0 = _lib.GpuBatch()
    for sp in (None, s.start.data_ptr()):
        s.first.fill_(CANARY64)
        sg = seg_struct(GOOD, 0 if sp is None else CAP)
        assert c.L.vbz_gpu_signal_segment_batch(c.ctx, ctypes.byref(b0), ctypes.byref(s.fr.opts), 0, 1, None, ctypes.byref(sg), s.first.data_ptr(), sp) == 0
        c.synchronize()
        assert s.first.cpu().numpy().tolist() == [0] + [CANARY64] * 7
        r0 = _lib.GpuPod5Reads()
        table = torch.zeros(1, dtype=torch.int32, device=c.device)
        r0.first_row = table.data_ptr()
        s.first.fill_(CANARY64)
        assert c.L.vbz_gpu_pod5_signal_segment_batch(c.ctx, ctypes.byref(b0), ctypes.byref(s.pc.opts), 1, ctypes.byref(r0), None, ctypes.byref(sg),
                                                     s.first.data_ptr(), sp) == 0
        c.synchronize()
        assert s.first.cpu().numpy().tolist() == [0] + [CANARY64] * 7
    assert (u32(s.start) == CANARY32).all()


def test_a_bad_first_row_fails_the_whole_call_with_nothing_written():
    c = codec()
    rows, first, frames = frames_of(21, [[600, 700], [900, 1000, 1100], [500]])
    table = list(PR.bounds(first, len(rows)))
    table[0] = 1
    call = SegCall(c, frames, rows, first, table=table)
    assert call.call() == 0
    assert u32(call.result)[: call.n].tolist() == [E_INPUT] * call.n and u32(call.read_result)[: call.R].tolist() == [E_INPUT] * call.R
    assert (call.t.first.cpu().numpy() == CANARY64).all() and (u32(call.t.start) == CANARY32).all()

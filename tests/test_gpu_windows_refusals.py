"""What the two signal-window calls refuse on the host (include/vbz_gpu.h: -2, nothing launched), each with its message; the NULLs they
allow; a call of no reads."""
import ctypes

import numpy as np
import pytest
import torch

import pod5_reads_ref as PR
from typed_support import CANARY, Call, Frames, codec, fmt, frames_of, ranges_struct, sine_signal
from vbz_compression_amd import _lib, batch
from windows_support import windows_struct

pytestmark = pytest.mark.gpu


class Setup:
    def __init__(self):
        c = self.c = codec()
        rng = np.random.default_rng(93)
        fr = self.fr = Frames(c, [sine_signal(rng, 500) for _ in range(4)], c.options(True, 2, 1, 1))
        dev = c.device
        self.res = torch.full((fr.n,), 12345, dtype=torch.int32, device=dev)
        self.ss = torch.full((fr.n, 2), 7.0, dtype=torch.float32, device=dev)
        self.out = torch.full((8 * 16 * 2 + 16,), CANARY, dtype=torch.uint8, device=dev)
        self.b = c._batch(fr.src, fr.off, fr.size, torch.empty(0, dtype=torch.uint8, device=dev), fr.doff, fr.dcap, self.res)
        self.b.dst, self.b.dst_bytes = None, fr.dst_bytes
        self.f = fmt("f16", True)
        self.first, self.flat = [0, 2, 4, 6, 8], [0, 8, 1, 9, 2, 10, 3, 11]
        rows, rfirst, frames = frames_of(22, [[600, 700], [900, 1000, 1100], [500, 20]])
        self.pc = Call(c, frames, [len(x) for x in rows], PR.bounds(rfirst, len(rows)), "f16", None)
        self.pfirst, self.pflat = [0, 2, 4, 6], [0, 8, 1, 9, 2, 10]

    def calls(self, w, pw, out="ok", o=None, f=None, m=None, ss=None, g=None, which=(0, 1)):
        c, L = self.c, self.c.L
        outp = self.out.data_ptr() if out == "ok" else out
        f = self.f if f is None else f
        mp, gp = (ctypes.byref(m) if m is not None else None), (ctypes.byref(g) if g is not None else None)
        ssp = ss.data_ptr() if ss is not None else None
        wp, pwp = (ctypes.byref(w) if w is not None else None), (ctypes.byref(pw) if pw is not None else None)
        fns = [lambda: L.vbz_gpu_decompress_windows_batch(c.ctx, ctypes.byref(self.b), ctypes.byref(self.fr.opts if o is None else o), 0, ctypes.byref(f), wp,
                                                          outp, mp, ssp, gp),
               lambda: L.vbz_gpu_pod5_decompress_windows_batch(c.ctx, ctypes.byref(self.pc.b), ctypes.byref(self.pc.opts), ctypes.byref(f),
                                                               ctypes.byref(self.pc.reads), pwp, outp, mp, ssp, gp)]
        got = []
        for k in which:
            got.append((fns[k](), L.vbz_gpu_last_error(c.ctx).decode()))
        return got

    def structs(self, L=16, **kw):
        w, k1 = windows_struct(self.c, self.first, self.flat, L, **kw)
        pw, k2 = windows_struct(self.c, self.pfirst, self.pflat, L, **kw)
        return w, pw, k1 + k2

    def untouched(self):
        torch.cuda.synchronize()
        assert (self.res.cpu() == 12345).all() and (self.ss.cpu() == 7.0).all() and (self.out.cpu().numpy() == CANARY).all()
        assert (self.pc.result.cpu() == -8).all() and (self.pc.read_result.cpu() == -8).all()


def refused(got, text):
    for rc, msg in got:
        assert rc == -2 and text in msg, (rc, msg, text)


def test_host_refusals_launch_nothing():
    s = Setup()
    refused(s.calls(None, None), "windows is NULL")
    for L in (0, 4, 12, (1 << 20) + 8):
        w, pw, keep = s.structs(L)
        refused(s.calls(w, pw), "windows outside the rules (window_len %u" % L)
    for kw in ({"flags": 1}, {"reserved": 1}):
        w, pw, keep = s.structs(**kw)
        refused(s.calls(w, pw), "windows outside the rules")
    w, pw, keep = s.structs()
    refused(s.calls(w, pw, out=None), "window arena is NULL")
    refused(s.calls(w, pw, out=s.out.data_ptr() + 8), "not 16-byte aligned")
    for name in ("window_first", "start"):
        w, pw, keep = s.structs()
        setattr(w, name, None)
        setattr(pw, name, None)
        refused(s.calls(w, pw), "window_first, start or the window arena is NULL")
    w, pw, keep = s.structs(rows=(1 << 46) // 32 + 1)
    refused(s.calls(w, pw), "declared window arena is not plausible")
    # what the ranged chunk calls refuse
    w, pw, keep = s.structs()
    refused(s.calls(w, pw, o=_lib.CompressionOptions(True, 4, 1, 1), which=(0,)), "unsupported options")
    bad_f = fmt("f16", True)
    bad_f.out_type = 9
    refused(s.calls(w, pw, f=bad_f), "signal format")
    bad_m = batch.MED_MAD.c_struct()
    bad_m.method = 9
    refused(s.calls(w, pw, m=bad_m, ss=s.ss), "normalization outside its rules")
    scale = torch.ones(4, dtype=torch.float32, device=s.c.device)
    refused(s.calls(w, pw, f=fmt("f16", True, scale=scale), m=batch.MED_MAD.c_struct(), ss=s.ss), "takes no offset or scale table")
    for kw in ({"reserved": 1}, {"stats": 2}):
        g, gk = ranges_struct(s.c, [0] * 4, None, **kw)
        refused(s.calls(w, pw, g=g), "sample ranges outside their rules")
    s.untouched()


def test_pod5_entry_refuses_other_options():
    s = Setup()
    w, pw, keep = s.structs()
    rc = s.c.L.vbz_gpu_pod5_decompress_windows_batch(s.c.ctx, ctypes.byref(s.pc.b), ctypes.byref(s.fr.opts), ctypes.byref(s.f), ctypes.byref(s.pc.reads),
                                                     ctypes.byref(pw), s.out.data_ptr(), None, None, None)
    assert rc == -2 and "POD5 options only" in s.c.L.vbz_gpu_last_error(s.c.ctx).decode()
    rc = s.c.L.vbz_gpu_pod5_decompress_windows_batch(s.c.ctx, ctypes.byref(s.pc.b), ctypes.byref(s.pc.opts), ctypes.byref(s.f), None, ctypes.byref(pw),
                                                     s.out.data_ptr(), None, None, None)
    assert rc == -2 and "reads: NULL" in s.c.L.vbz_gpu_last_error(s.c.ctx).decode()
    s.untouched()


def test_allowed_nulls_and_a_call_of_no_reads():
    s = Setup()
    c, L = s.c, s.c.L
    # no window at all: start may be NULL with window_rows == 0; norm, shift_scale and ranges may be NULL
    w, keep = windows_struct(c, [0] * 5, [], 16)
    pw, pkeep = windows_struct(c, [0] * 4, [], 16)
    assert w.start is None and w.window_rows == 0
    assert [rc for rc, _ in s.calls(w, pw)] == [0, 0]
    c.synchronize()
    assert (s.res.cpu() == 1000).all() and (s.out.cpu().numpy() == CANARY).all()
    assert [rc for rc, _ in s.calls(w, pw, m=batch.MED_MAD.c_struct())] == [0, 0]   # (norm without shift_scale)
    c.synchronize()
    # a call of no reads: every table and the arena may be NULL
    b0 = _lib.GpuBatch()
    w0 = _lib.GpuWindows()
    w0.window_len = 16
    assert L.vbz_gpu_decompress_windows_batch(c.ctx, ctypes.byref(b0), ctypes.byref(s.fr.opts), 0, ctypes.byref(s.f), ctypes.byref(w0), None, None, None, None) == 0
    r0 = _lib.GpuPod5Reads()
    table = torch.zeros(1, dtype=torch.int32, device=c.device)
    r0.first_row = table.data_ptr()
    assert L.vbz_gpu_pod5_decompress_windows_batch(c.ctx, ctypes.byref(b0), ctypes.byref(s.pc.opts), ctypes.byref(s.f), ctypes.byref(r0), ctypes.byref(w0),
                                                   None, None, None, None) == 0
    c.synchronize()
    assert (s.out.cpu().numpy() == CANARY).all()

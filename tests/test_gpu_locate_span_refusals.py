"""What the three locate span calls refuse on the host (include/vbz_gpu.h: the locate calls' refusals with the 16-byte arena: -2, nothing
launched, nothing written), each with its message and with canary-filled query, 16-byte hits and shift_scale untouched; the reachable
size rule; a call of no reads."""
import ctypes

import numpy as np
import pytest
import torch

import pod5_reads_ref as PR
from locate_span_support import SpanArenas
from locate_support import locate_struct
from typed_support import Call, Frames, codec, fmt, frames_of, i32, ranges_struct, sine_signal
from vbz_compression_amd import _lib, batch

pytestmark = pytest.mark.gpu

N, G, STRIDE = 64, 3, 32


class Setup:
    def __init__(self):
        c = self.c = codec()
        rng = np.random.default_rng(93)
        fr = self.fr = Frames(c, [sine_signal(rng, 500) for _ in range(4)], c.options(True, 2, 1, 1))
        dev = c.device
        self.res = torch.full((fr.n,), 12345, dtype=torch.int32, device=dev)
        self.a = SpanArenas(c, fr.n, N, G)
        self.valid = i32([N] * fr.n).to(dev)
        self.b = c._batch(fr.src, fr.off, fr.size, torch.empty(0, dtype=torch.uint8, device=dev), fr.doff, fr.dcap, self.res)
        self.b.dst, self.b.dst_bytes = None, fr.dst_bytes
        self.f = fmt("f32", True)
        self.target = rng.integers(-100, 101, (G, STRIDE)).astype(np.int8)
        rows, rfirst, frames = frames_of(22, [[600, 700], [900, 1000, 1100], [500, 20], [64]])
        self.pc = Call(c, frames, [len(x) for x in rows], PR.bounds(rfirst, len(rows)), "f32", None)

    def struct(self, **kw):
        args = {"N": N, "quant": 32.0, "target": self.target, "target_len": [20, 32, 7]}
        flags = {k: kw.pop(k) for k in ("flags", "reserved") if k in kw}
        args.update(kw)
        return locate_struct(self.c, args["N"], args["quant"], args["target"], args["target_len"], **flags)

    def calls(self, m, query="ok", out="ok", o=None, f=None, nm=None, ss=None, g=None, which=(0, 1, 2)):
        c, L = self.c, self.c.L
        qp = self.a.query.data_ptr() if query == "ok" else query
        outp = self.a.out.data_ptr() if out == "ok" else out
        f = self.f if f is None else f
        nmp, gp = (ctypes.byref(nm) if nm is not None else None), (ctypes.byref(g) if g is not None else None)
        ssp = ss.data_ptr() if ss is not None else None
        mp = ctypes.byref(m) if m is not None else None
        fns = [lambda: L.vbz_gpu_signal_locate_span_batch(c.ctx, ctypes.byref(self.b), ctypes.byref(self.fr.opts if o is None else o), 0, ctypes.byref(f), nmp, ssp,
                                                     gp, mp, qp, outp),
               lambda: L.vbz_gpu_pod5_signal_locate_span_batch(c.ctx, ctypes.byref(self.pc.b), ctypes.byref(self.pc.opts), ctypes.byref(f),
                                                          ctypes.byref(self.pc.reads), nmp, ssp, gp, mp, qp, outp),
               lambda: L.vbz_gpu_locate_span_batch(c.ctx, self.fr.n, qp, self.valid.data_ptr(), mp, outp)]
        return [(fns[k](), L.vbz_gpu_last_error(c.ctx).decode()) for k in which]

    def untouched(self):
        torch.cuda.synchronize()
        assert (self.res.cpu() == 12345).all() and self.a.untouched()
        assert (self.pc.result.cpu() == -8).all() and (self.pc.read_result.cpu() == -8).all()


def refused(got, text):
    for rc, msg in got:
        assert rc == -2 and text in msg, (rc, msg, text)


def test_host_refusals_launch_nothing():
    s = Setup()
    refused(s.calls(None), "locate is NULL")
    for n in (0, 4, 12, 2056):
        m, keep = s.struct(N=n)
        refused(s.calls(m), "locate outside the rules (query_len %u" % n)
    for quant in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        m, keep = s.struct(quant=quant)
        refused(s.calls(m), "locate outside the rules")
    for kw in ({"flags": 1}, {"reserved": 1}):
        m, keep = s.struct(**kw)
        refused(s.calls(m), "locate outside the rules")
    m, keep = s.struct()
    for field, bad in (("n_targets", (0, 4097)), ("target_stride", (0, 8, 24, (1 << 30) + 16))):
        for v in bad:
            m2, keep2 = s.struct()
            setattr(m2, field, v)
            refused(s.calls(m2), "locate outside the rules")
    refused(s.calls(m, query=None), "is NULL")
    refused(s.calls(m, out=None), "is NULL")
    for field in ("target", "target_len"):
        m2, keep2 = s.struct()
        setattr(m2, field, None)
        refused(s.calls(m2), "is NULL")
    refused(s.calls(m, query=s.a.query.data_ptr() + 8), "not 16-byte aligned")
    refused(s.calls(m, out=s.a.out.data_ptr() + 8), "not 16-byte aligned")
    m2, keep2 = s.struct()
    m2.target = m2.target + 8
    refused(s.calls(m2), "not 16-byte aligned")
    rc = s.c.L.vbz_gpu_locate_span_batch(s.c.ctx, s.fr.n, s.a.query.data_ptr(), None, ctypes.byref(m), s.a.out.data_ptr())
    assert rc == -2 and "valid is NULL" in s.c.L.vbz_gpu_last_error(s.c.ctx).decode()
    # the size rule: n_reads x G x 16 beyond 2^46 bytes (G x target_stride <= 2^42 and n_reads x N x 4 < 2^45 under the struct's own rules).
    # 2^31 reads x 4 096 targets is 2^46 bytes of 8-byte hits, which is not beyond the rule, and 2^47 of 16-byte ones, which is
    big, keepb = s.struct(N=8)
    big.n_targets = 4096
    rc = s.c.L.vbz_gpu_locate_span_batch(s.c.ctx, 0xFFFFFFFF, s.a.query.data_ptr(), s.valid.data_ptr(), ctypes.byref(big), s.a.out.data_ptr())
    assert rc == -2 and "not plausible" in s.c.L.vbz_gpu_last_error(s.c.ctx).decode()
    rc = s.c.L.vbz_gpu_locate_span_batch(s.c.ctx, 1 << 31, s.a.query.data_ptr(), s.valid.data_ptr(), ctypes.byref(big), s.a.out.data_ptr())
    assert rc == -2 and "not plausible" in s.c.L.vbz_gpu_last_error(s.c.ctx).decode()
    # an output type other than float32, and what the windows calls refuse
    for t in ("f16", "bf16"):
        refused(s.calls(m, f=fmt(t, True), which=(0, 1)), "float32")
    refused(s.calls(m, o=_lib.CompressionOptions(True, 4, 1, 1), which=(0,)), "unsupported options")
    bad_f = fmt("f32", True)
    bad_f.out_type = 9
    refused(s.calls(m, f=bad_f, which=(0, 1)), "signal format")
    bad_m = batch.MED_MAD.c_struct()
    bad_m.method = 9
    refused(s.calls(m, nm=bad_m, ss=s.a.ss, which=(0, 1)), "normalization outside its rules")
    for kw in ({"reserved": 1}, {"stats": 2}):
        g, gk = ranges_struct(s.c, [0] * 4, None, **kw)
        refused(s.calls(m, g=g, which=(0, 1)), "sample ranges outside their rules")
    rc = s.c.L.vbz_gpu_pod5_signal_locate_span_batch(s.c.ctx, ctypes.byref(s.pc.b), ctypes.byref(s.pc.opts), ctypes.byref(s.f), None, None, None, None,
                                                ctypes.byref(m), s.a.query.data_ptr(), s.a.out.data_ptr())
    assert rc == -2 and "reads: NULL" in s.c.L.vbz_gpu_last_error(s.c.ctx).decode()
    s.untouched()


def test_a_call_of_no_reads():
    s = Setup()
    c, L = s.c, s.c.L
    m0 = _lib.GpuLocate()
    m0.query_len, m0.n_targets, m0.target_stride, m0.quant = 64, 1, 16, 1.0
    b0 = _lib.GpuBatch()
    assert L.vbz_gpu_locate_span_batch(c.ctx, 0, None, None, ctypes.byref(m0), None) == 0
    assert L.vbz_gpu_signal_locate_span_batch(c.ctx, ctypes.byref(b0), ctypes.byref(s.fr.opts), 0, ctypes.byref(s.f), None, None, None, ctypes.byref(m0), None, None) == 0
    r0 = _lib.GpuPod5Reads()
    table = torch.zeros(1, dtype=torch.int32, device=c.device)
    r0.first_row = table.data_ptr()
    assert L.vbz_gpu_pod5_signal_locate_span_batch(c.ctx, ctypes.byref(b0), ctypes.byref(s.pc.opts), ctypes.byref(s.f), ctypes.byref(r0), None, None, None,
                                              ctypes.byref(m0), None, None) == 0
    c.synchronize()
    s.untouched()

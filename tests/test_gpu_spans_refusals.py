"""What the two signal-span calls refuse on the host (include/vbz_gpu.h: -2, nothing launched), each single fault with its message and
every output still holding its canary; the good call; the NULLs they allow; a call of no reads; a bad first_row."""
import ctypes
import math

import numpy as np
import pytest
import torch

import pod5_reads_ref as PR
import spans_ref as S
from segment_support import CANARY32, CANARY64
from spans_support import SS_CANARY, SpanCall, span_struct
from typed_support import NORMS, Call, Frames, codec, frames_of, ranges_struct, sine_signal, u32
from vbz_compression_amd import _lib, batch

pytestmark = pytest.mark.gpu

E_INPUT = 0xFFFFFFFE
GOOD = (S.ABOVE, 5, 2, 0, 0.0)
LEVEL = (420.0, 0.0)   # (the sine signal: 330 +- 60 under noise of sd 40)
CAP = 4096


class Setup:
    def __init__(self):
        c = self.c = codec()
        rng = np.random.default_rng(93)
        fr = self.fr = Frames(c, [sine_signal(rng, 500) for _ in range(4)], c.options(True, 2, 1, 1))
        dev = c.device
        self.res = torch.full((fr.n,), 12345, dtype=torch.int32, device=dev)
        self.first = torch.full((8,), CANARY64, dtype=torch.int64, device=dev)
        self.edge = torch.full((CAP + 8,), CANARY32, dtype=torch.int32, device=dev)
        self.ss = torch.full((8, 2), SS_CANARY, dtype=torch.float32, device=dev)
        self.level = torch.tensor([LEVEL] * 4, dtype=torch.float32, device=dev)
        self.b = c._batch(fr.src, fr.off, fr.size, torch.empty(0, dtype=torch.uint8, device=dev), fr.doff, fr.dcap, self.res)
        self.b.dst, self.b.dst_bytes = None, fr.dst_bytes
        rows, rfirst, frames = frames_of(22, [[600, 700], [900, 1000, 1100], [500, 20]])
        self.rows, self.rfirst = rows, rfirst
        self.pc = Call(c, frames, [len(x) for x in rows], PR.bounds(rfirst, len(rows)), "f32", None)

    def good(self, P=GOOD, cap=CAP, level=True, **kw):
        return span_struct(P, cap, self.level if level else None, **kw)

    def calls(self, sp, first="ok", edge="ok", o=None, signed=1, g=None, m=None, which=(0, 1)):
        c, L = self.c, self.c.L
        fp = self.first.data_ptr() if first == "ok" else first
        ep = self.edge.data_ptr() if edge == "ok" else edge
        gp = ctypes.byref(g) if g is not None else None
        spp = ctypes.byref(sp) if sp is not None else None
        mp = ctypes.byref(m) if m is not None else None
        ssp = self.ss.data_ptr() if m is not None else None
        fns = [lambda: L.vbz_gpu_signal_spans_batch(c.ctx, ctypes.byref(self.b), ctypes.byref(self.fr.opts if o is None else o), 0, signed, mp, ssp, gp, spp, fp, ep),
               lambda: L.vbz_gpu_pod5_signal_spans_batch(c.ctx, ctypes.byref(self.pc.b), ctypes.byref(self.pc.opts), signed, ctypes.byref(self.pc.reads), mp, ssp,
                                                         gp, spp, fp, ep)]
        return [(fns[k](), L.vbz_gpu_last_error(c.ctx).decode()) for k in which]

    def untouched(self):
        torch.cuda.synchronize()
        assert (self.res.cpu() == 12345).all()
        assert (self.first.cpu().numpy() == CANARY64).all() and (u32(self.edge) == CANARY32).all() and (self.ss.cpu().numpy() == SS_CANARY).all()
        assert (self.pc.result.cpu() == -8).all() and (self.pc.read_result.cpu() == -8).all()


def refused(got, text):
    for rc, msg in got:
        assert rc == -2 and text in msg, (rc, msg, text)


def test_host_refusals_launch_nothing():
    s = Setup()
    good = s.good()
    refused(s.calls(None), "spans or edge_first is NULL")
    refused(s.calls(good, first=None), "spans or edge_first is NULL")
    refused(s.calls(good, edge=None), "edge is NULL with edge_cap")
    faults = [(2, 5, 2, 0, 0.0), (0xFFFFFFFF, 5, 2, 0, 0.0), (S.ABOVE, 65536, 2, 0, 0.0), (S.BELOW, 5, 0, 0, 0.0), (S.ABOVE, 5, 1 << 31, 0, 0.0),
              (S.ABOVE, 5, 0xFFFFFFFF, 0, 0.0), (S.ABOVE, 5, 2, 0, math.nan), (S.BELOW, 5, 2, 0, math.inf), (S.ABOVE, 5, 2, 0, -math.inf)]
    for P in faults:
        refused(s.calls(s.good(P)), "spans outside their rules")
    refused(s.calls(s.good(flags=1)), "spans outside their rules")
    refused(s.calls(s.good(level=False)), "level is NULL and there is no normalisation")
    refused(s.calls(good, m=NORMS["med_mad"][1].c_struct()), "level must be NULL with a normalisation")
    refused(s.calls(s.good(cap=(1 << 46) // 4 + 1)), "declared edge table is not plausible")
    # a normalisation that is given must pass its rules
    bad = NORMS["med_mad"][1].c_struct()
    bad.method = 7
    refused(s.calls(s.good(level=False), m=bad), "normalization outside its rules")
    # what the ranged statistics calls refuse about the options, is_signed and the ranges
    refused(s.calls(good, o=_lib.CompressionOptions(True, 4, 1, 1), which=(0,)), "unsupported options")
    refused(s.calls(good, signed=2), "is_signed not 0 / 1")
    for kw in ({"reserved": 1}, {"stats": 2}):
        g, gk = ranges_struct(s.c, [0] * 4, None, **kw)
        refused(s.calls(good, g=g), "sample ranges outside their rules")
    s.untouched()


def test_pod5_entry_refuses_other_options_and_null_reads():
    s = Setup()
    L, good = s.c.L, s.good()
    rc = L.vbz_gpu_pod5_signal_spans_batch(s.c.ctx, ctypes.byref(s.pc.b), ctypes.byref(s.fr.opts), 1, ctypes.byref(s.pc.reads), None, None, None,
                                           ctypes.byref(good), s.first.data_ptr(), s.edge.data_ptr())
    assert rc == -2 and "POD5 options only" in L.vbz_gpu_last_error(s.c.ctx).decode()
    rc = L.vbz_gpu_pod5_signal_spans_batch(s.c.ctx, ctypes.byref(s.pc.b), ctypes.byref(s.pc.opts), 1, None, None, None, None, ctypes.byref(good),
                                           s.first.data_ptr(), s.edge.data_ptr())
    assert rc == -2 and "reads: NULL" in L.vbz_gpu_last_error(s.c.ctx).decode()
    s.untouched()


def test_the_good_call_and_the_allowed_nulls():
    s = Setup()
    c = s.c
    g0, gk = ranges_struct(c, None, None)
    want, ed = S.tables(s.fr.reads, GOOD, [LEVEL] * 4)
    sig = PR.read_signals(s.rows, s.rfirst)
    pwant, ped = S.tables(sig, GOOD, [LEVEL] * 3)
    assert want[-1] >= 8 and pwant[-1] >= 8
    for g in (None, g0):   # ranges NULL or with both tables NULL; a given level takes no shift_scale
        s.first.fill_(CANARY64)
        assert [rc for rc, _ in s.calls(s.good(), g=g, which=(0,))] == [0], c.L.vbz_gpu_last_error(c.ctx)
        c.synchronize()
        assert s.first.cpu().numpy()[:5].tolist() == want.tolist() and (s.res.cpu() == 1000).all()
        assert u32(s.edge)[: int(want[-1])].tolist() == np.concatenate(ed).tolist()
        assert [rc for rc, _ in s.calls(s.good(), g=g, which=(1,))] == [0], c.L.vbz_gpu_last_error(c.ctx)
        c.synchronize()
        assert s.first.cpu().numpy()[:4].tolist() == pwant.tolist()
    assert (s.ss.cpu().numpy() == SS_CANARY).all()
    # the count-only call: edge NULL with edge_cap 0 -- edge_first alone
    s.edge.fill_(CANARY32)
    assert [rc for rc, _ in s.calls(s.good(cap=0), edge=None)] == [0, 0]
    c.synchronize()
    assert (u32(s.edge) == CANARY32).all() and s.first.cpu().numpy()[:4].tolist() == pwant.tolist()
    # a call of no reads: edge_first[0] = 0, nothing else; edge may be anything
    b0 = _lib.GpuBatch()
    for ep in (None, s.edge.data_ptr()):
        s.first.fill_(CANARY64)
        sp = s.good(cap=0 if ep is None else CAP)
        assert c.L.vbz_gpu_signal_spans_batch(c.ctx, ctypes.byref(b0), ctypes.byref(s.fr.opts), 0, 1, None, None, None, ctypes.byref(sp), s.first.data_ptr(), ep) == 0
        c.synchronize()
        assert s.first.cpu().numpy().tolist() == [0] + [CANARY64] * 7
        r0 = _lib.GpuPod5Reads()
        table = torch.zeros(1, dtype=torch.int32, device=c.device)
        r0.first_row = table.data_ptr()
        s.first.fill_(CANARY64)
        assert c.L.vbz_gpu_pod5_signal_spans_batch(c.ctx, ctypes.byref(b0), ctypes.byref(s.pc.opts), 1, ctypes.byref(r0), None, None, None, ctypes.byref(sp),
                                                   s.first.data_ptr(), ep) == 0
        c.synchronize()
        assert s.first.cpu().numpy().tolist() == [0] + [CANARY64] * 7
    assert (u32(s.edge) == CANARY32).all()


@pytest.mark.parametrize("with_norm", [False, True], ids=["level", "norm"])
def test_a_bad_first_row_fails_the_whole_call_with_nothing_written(with_norm):
    c = codec()
    rows, first, frames = frames_of(21, [[600, 700], [900, 1000, 1100], [500]])
    table = list(PR.bounds(first, len(rows)))
    table[0] = 1
    kw = dict(norm=NORMS["med_mad"]) if with_norm else dict(levels=[LEVEL] * 3)
    call = SpanCall(c, frames, rows, first, GOOD, table=table, **kw)
    assert call.call() == 0
    assert u32(call.result)[: call.n].tolist() == [E_INPUT] * call.n and u32(call.read_result)[: call.R].tolist() == [E_INPUT] * call.R
    assert (call.t.first.cpu().numpy() == CANARY64).all() and (u32(call.t.start) == CANARY32).all()
    assert (call.ss2.cpu().numpy() == SS_CANARY).all()

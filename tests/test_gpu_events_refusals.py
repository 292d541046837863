"""What the two signal-event calls refuse on the host (include/vbz_gpu.h: -2, nothing launched), each with its message; the NULLs they
allow; a call of no reads; and what the event check refuses on the device, read by read."""
import ctypes

import numpy as np
import pytest
import torch

import pod5_reads_ref as PR
from events_support import EvCall, EvRun, events_struct
from typed_support import CANARY, NORMS, Call, Frames, codec, fmt, frames_of, ranges_struct, sine_signal, u32
from vbz_compression_amd import _lib, batch

pytestmark = pytest.mark.gpu

E_ZSTD, E_INPUT, E_DEST = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFC
TO_END = 0xFFFFFFFF


class Setup:
    def __init__(self):
        c = self.c = codec()
        rng = np.random.default_rng(93)
        fr = self.fr = Frames(c, [sine_signal(rng, 500) for _ in range(4)], c.options(True, 2, 1, 1))
        dev = c.device
        self.res = torch.full((fr.n,), 12345, dtype=torch.int32, device=dev)
        self.ss = torch.full((fr.n, 2), 7.0, dtype=torch.float32, device=dev)
        self.out = torch.full((8 * 16 + 16,), CANARY, dtype=torch.uint8, device=dev)
        self.mom = torch.full((8 * 16 + 16,), CANARY, dtype=torch.uint8, device=dev)
        self.b = c._batch(fr.src, fr.off, fr.size, torch.empty(0, dtype=torch.uint8, device=dev), fr.doff, fr.dcap, self.res)
        self.b.dst, self.b.dst_bytes = None, fr.dst_bytes
        self.f = fmt("f32", True)
        self.first, self.flat = [0, 2, 4, 6, 8], [0, 8, 1, 9, 2, 10, 3, 11]
        rows, rfirst, frames = frames_of(22, [[600, 700], [900, 1000, 1100], [500, 20]])
        self.pc = Call(c, frames, [len(x) for x in rows], PR.bounds(rfirst, len(rows)), "f32", None)
        self.pfirst, self.pflat = [0, 2, 4, 6], [0, 8, 1, 9, 2, 10]

    def calls(self, ev, pev, out="ok", mom="ok", o=None, f=None, m=None, ss=None, g=None, which=(0, 1)):
        c, L = self.c, self.c.L
        outp = self.out.data_ptr() if out == "ok" else out
        momp = self.mom.data_ptr() if mom == "ok" else mom
        f = self.f if f is None else f
        mp, gp = (ctypes.byref(m) if m is not None else None), (ctypes.byref(g) if g is not None else None)
        ssp = ss.data_ptr() if ss is not None else None
        ep, pep = (ctypes.byref(ev) if ev is not None else None), (ctypes.byref(pev) if pev is not None else None)
        fns = [lambda: L.vbz_gpu_signal_events_batch(c.ctx, ctypes.byref(self.b), ctypes.byref(self.fr.opts if o is None else o), 0, ctypes.byref(f), ep,
                                                     outp, momp, mp, ssp, gp),
               lambda: L.vbz_gpu_pod5_signal_events_batch(c.ctx, ctypes.byref(self.pc.b), ctypes.byref(self.pc.opts), ctypes.byref(f),
                                                          ctypes.byref(self.pc.reads), pep, outp, momp, mp, ssp, gp)]
        got = []
        for k in which:
            got.append((fns[k](), L.vbz_gpu_last_error(c.ctx).decode()))
        return got

    def structs(self, **kw):
        ev, k1 = events_struct(self.c, self.first, self.flat, **kw)
        pev, k2 = events_struct(self.c, self.pfirst, self.pflat, **kw)
        return ev, pev, k1 + k2

    def untouched(self):
        torch.cuda.synchronize()
        assert (self.res.cpu() == 12345).all() and (self.ss.cpu() == 7.0).all()
        assert (self.out.cpu().numpy() == CANARY).all() and (self.mom.cpu().numpy() == CANARY).all()
        assert (self.pc.result.cpu() == -8).all() and (self.pc.read_result.cpu() == -8).all()


def refused(got, text):
    for rc, msg in got:
        assert rc == -2 and text in msg, (rc, msg, text)


def test_host_refusals_launch_nothing():
    s = Setup()
    refused(s.calls(None, None), "events is NULL")
    for kw in ({"flags": 1}, {"reserved": 1}):
        ev, pev, keep = s.structs(**kw)
        refused(s.calls(ev, pev), "events outside the rules")
    ev, pev, keep = s.structs()
    for t in ("f16", "bf16"):
        refused(s.calls(ev, pev, f=fmt(t, True)), "event records are float32")
    refused(s.calls(ev, pev, out=None), "event arena is NULL")
    refused(s.calls(ev, pev, out=s.out.data_ptr() + 8), "not 16-byte aligned")
    refused(s.calls(ev, pev, mom=s.mom.data_ptr() + 8), "not 16-byte aligned")
    for name in ("event_first", "start"):
        ev, pev, keep = s.structs()
        setattr(ev, name, None)
        setattr(pev, name, None)
        refused(s.calls(ev, pev), "event_first, start or the event arena is NULL")
    ev, pev, keep = s.structs(rows=(1 << 46) // 16 + 1)
    refused(s.calls(ev, pev), "declared event arena is not plausible")
    # what the ranged statistics calls refuse
    ev, pev, keep = s.structs()
    refused(s.calls(ev, pev, o=_lib.CompressionOptions(True, 4, 1, 1), which=(0,)), "unsupported options")
    bad_f = fmt("f32", True)
    bad_f.out_type = 9
    refused(s.calls(ev, pev, f=bad_f), "signal format")
    bad_f = fmt("f32", True)
    bad_f.is_signed = 2
    refused(s.calls(ev, pev, f=bad_f), "signal format")
    bad_m = batch.MED_MAD.c_struct()
    bad_m.method = 9
    refused(s.calls(ev, pev, m=bad_m, ss=s.ss), "normalization outside its rules")
    scale = torch.ones(4, dtype=torch.float32, device=s.c.device)
    refused(s.calls(ev, pev, f=fmt("f32", True, scale=scale), m=batch.MED_MAD.c_struct(), ss=s.ss), "takes no offset or scale table")
    for kw in ({"reserved": 1}, {"stats": 2}):
        g, gk = ranges_struct(s.c, [0] * 4, None, **kw)
        refused(s.calls(ev, pev, g=g), "sample ranges outside their rules")
    s.untouched()


def test_pod5_entry_refuses_other_options():
    s = Setup()
    ev, pev, keep = s.structs()
    L = s.c.L
    rc = L.vbz_gpu_pod5_signal_events_batch(s.c.ctx, ctypes.byref(s.pc.b), ctypes.byref(s.fr.opts), ctypes.byref(s.f), ctypes.byref(s.pc.reads),
                                            ctypes.byref(pev), s.out.data_ptr(), None, None, None, None)
    assert rc == -2 and "POD5 options only" in L.vbz_gpu_last_error(s.c.ctx).decode()
    rc = L.vbz_gpu_pod5_signal_events_batch(s.c.ctx, ctypes.byref(s.pc.b), ctypes.byref(s.pc.opts), ctypes.byref(s.f), None, ctypes.byref(pev),
                                            s.out.data_ptr(), None, None, None, None)
    assert rc == -2 and "reads: NULL" in L.vbz_gpu_last_error(s.c.ctx).decode()
    s.untouched()


def test_allowed_nulls_and_a_call_of_no_reads():
    s = Setup()
    c, L = s.c, s.c.L
    # no event at all: start may be NULL with event_rows == 0; moments, norm, shift_scale and ranges may be NULL
    ev, keep = events_struct(c, [0] * 5, [])
    pev, pkeep = events_struct(c, [0] * 4, [])
    assert ev.start is None and ev.event_rows == 0
    assert [rc for rc, _ in s.calls(ev, pev, mom=None)] == [0, 0]
    c.synchronize()
    assert (s.res.cpu() == 1000).all() and (s.out.cpu().numpy() == CANARY).all() and (s.mom.cpu().numpy() == CANARY).all()
    assert [rc for rc, _ in s.calls(ev, pev, mom=None, m=batch.MED_MAD.c_struct())] == [0, 0]   # (norm without shift_scale)
    c.synchronize()
    ev, pev, keep2 = s.structs()
    assert [rc for rc, _ in s.calls(ev, pev, mom=None, m=batch.MED_MAD.c_struct())] == [0, 0]   # (... and with events: neither table is the caller's)
    c.synchronize()
    assert (s.mom.cpu().numpy() == CANARY).all() and not (s.out.cpu().numpy()[: 8 * 16] == CANARY).all()
    # a call of no reads: every table and both arenas may be NULL
    b0 = _lib.GpuBatch()
    e0 = _lib.GpuEvents()
    assert L.vbz_gpu_signal_events_batch(c.ctx, ctypes.byref(b0), ctypes.byref(s.fr.opts), 0, ctypes.byref(s.f), ctypes.byref(e0), None, None, None, None, None) == 0
    r0 = _lib.GpuPod5Reads()
    table = torch.zeros(1, dtype=torch.int32, device=c.device)
    r0.first_row = table.data_ptr()
    assert L.vbz_gpu_pod5_signal_events_batch(c.ctx, ctypes.byref(b0), ctypes.byref(s.pc.opts), ctypes.byref(s.f), ctypes.byref(r0), ctypes.byref(e0),
                                              None, None, None, None, None) == 0
    c.synchronize()
    assert (s.out.cpu().numpy()[8 * 16 :] == CANARY).all()


# ---- the event check, read by read -----------------------------------------------------------------------------------------------------------
def dwell(rng, T, k):
    return sorted(int(v) for v in rng.integers(0, T + 5, k))


def verdict_frames(c):
    rng = np.random.default_rng(91)
    return Frames(c, [sine_signal(rng, T) for T in (5000, 3000, 2500, 900)], c.options(True, 2, 1, 1))


def test_event_check_failures_fail_that_read_alone():
    c = codec()
    fr = verdict_frames(c)
    rng = np.random.default_rng(5)
    starts = [dwell(rng, T, k) for T, k in zip(fr.T, (20, 30, 40, 30))]
    flat = [v for s in starts for v in s]
    n0, n1, n3 = len(starts[0]), len(starts[1]), len(starts[3])
    for norm in (None, NORMS["med_mad"]):
        # event_first[2] > event_first[3]: the reads own rows n3 .. n3 + n0 - 1, the n1 behind them, (first > next), 0 .. n3 - 1
        per = [starts[0], starts[1], [], starts[3]]
        order = starts[3] + starts[0] + starts[1]
        EvRun(fr, per, first=[n3, n3 + n0, n3 + n0 + n1, 0, n3], flat=order, norm=norm).check(expect={2: E_DEST})
        # event_first[4] > event_rows: read 3's rows lie behind the rows the struct declares
        EvRun(fr, starts, rows=len(flat) - 1, norm=norm).check(expect={3: E_DEST})
        # a decreasing pair inside read 2's rows (and one between two reads' rows, which is none of the check's business)
        bad = [list(s) for s in starts]
        bad[2][2], bad[2][3] = 900, 899
        bad[1][0] = 2990
        bad[1].sort()
        EvRun(fr, bad, norm=norm).check(expect={2: E_DEST})
        # the starts are unsigned: 0x80000000 behind 5 is in order, 5 behind 0xFFFFFFFF is not
        EvRun(fr, [[5, 0x80000000], [0, TO_END, 5], starts[2], starts[3]], norm=norm).check(expect={1: E_DEST})
    # a long list whose only decreasing pair is its last
    long = [dwell(rng, 5000, 3000), [0], [], [5]]
    long[0][-1] = long[0][-2] - 1
    EvRun(fr, long).check(expect={0: E_DEST})


def test_a_damaged_frame_keeps_its_verdict():
    c = codec()
    fr = verdict_frames(c)
    src = fr.src.clone()
    size = fr.size.clone()
    size[1] = int(u32(fr.size)[1]) // 2   # the frame of read 1 cut off in its middle
    fr.size = size
    dst = torch.zeros(fr.dst_bytes + 64, dtype=torch.uint8, device=c.device)
    res16 = torch.full((fr.n,), -8, dtype=torch.int32, device=c.device)
    c.decompress(src, fr.off, fr.size, dst, fr.doff, fr.dcap, res16, fr.opts)
    torch.cuda.synchronize()
    un = u32(res16).tolist()
    assert _lib.is_error(un[1]) and not any(_lib.is_error(v) for i, v in enumerate(un) if i != 1), [hex(v) for v in un]
    rng = np.random.default_rng(6)
    starts = [dwell(rng, T, 25) for T in fr.T]
    EvRun(fr, starts, src=src).check(expect={1: un[1]}, skip={1})


def test_pod5_verdicts():
    c = codec()
    shapes = [[600, 700], [900, 1000, 1100], [500], [900, 1000, 1100], [640]]
    rows, first, frames = frames_of(21, shapes)
    rng = np.random.default_rng(8)
    starts = [dwell(rng, sum(lens), 30) for lens in shapes]
    b = PR.bounds(first, len(rows))
    sig = PR.read_signals(rows, first)
    # a decreasing pair inside read 1's rows, and read 3's event_first pair the wrong way round
    bad = [list(s) for s in starts]
    bad[1][4], bad[1][5] = bad[1][5] + 1, bad[1][4]
    n4 = len(starts[4])
    flat = bad[0] + bad[1] + starts[4]
    # the same, and: read 2's rows end behind the arena's, read 3's pair is the wrong way round; read 4 owns the last rows
    efirst = [0, len(bad[0]), len(flat) - n4, len(flat) + 2, len(flat) - n4, len(flat)]
    for which, call, refused_reads in (("sorted", EvCall(c, frames, rows, first, bad), {1}),
                                       ("pairs", EvCall(c, frames, rows, first, [bad[0], bad[1], [], [], starts[4]], efirst=efirst, flat=flat), {1, 2, 3})):
        assert call.call() == 0, c.L.vbz_gpu_last_error(c.ctx)
        assert u32(call.result)[: call.n].tolist() == [E_DEST if k in refused_reads else 2 * len(rows[j]) for k in range(len(first)) for j in range(b[k], b[k + 1])], which
        assert u32(call.read_result)[: call.R].tolist() == [E_DEST if k in refused_reads else 2 * len(sig[k]) for k in range(len(first))], which
        call.check(consts=[(0.0, 1.0)] * 5, refused=refused_reads)
    # a bad first_row fails whole
    table = list(b)
    table[0] = 1
    call = EvCall(c, frames, rows, first, starts, table=table)
    assert call.call() == 0
    assert u32(call.result)[: call.n].tolist() == [E_INPUT] * call.n and u32(call.read_result)[: call.R].tolist() == [E_INPUT] * call.R
    assert (call.out.cpu().numpy() == CANARY).all() and (call.mom.cpu().numpy() == CANARY).all()
    # a damaged row inside a read: its verdict, the other reads exact
    damaged = list(frames)
    damaged[3] = frames[3][: len(frames[3]) // 2]
    call = EvCall(c, damaged, rows, first, starts)
    assert call.call() == 0
    res = u32(call.result)[: call.n].tolist()
    assert res[3] == E_ZSTD and [r for j, r in enumerate(res) if j != 3] == [2 * len(x) for j, x in enumerate(rows) if j != 3]
    assert u32(call.read_result)[: call.R].tolist() == [E_ZSTD if k == 1 else 2 * len(sig[k]) for k in range(5)]
    call.check(consts=[(0.0, 1.0)] * 5, skip={1})

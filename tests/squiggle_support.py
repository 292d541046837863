"""The raw pore-model calls for the tests on the MI355X (test_gpu_squiggle, test_gpu_levels_fit, test_gpu_squiggle_refusals): one call of
squiggle_ref's catalogues into arenas with canary words in front of and behind each, and its check against the numpy statement bit for
bit.  A plain module: every assert carries its operands."""
import ctypes

import numpy as np
import torch

from eventalign_support import Guarded, dev_u32
from vbz_compression_amd import _lib


def dev_bytes(c, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(c.device)


class SquiggleTables:
    """the device tables and guarded arenas of one squiggle_ref.SquiggleCall"""

    def __init__(self, c, call):
        self.call, self.rows, self.T = call, call.rows, call.target_stride
        self.seq, self.seq_len, self.model = dev_bytes(c, call.seq), dev_u32(c, call.seq_len), dev_u32(c, call.model)
        self.target, self.target_len, self.masked = Guarded(c, self.rows * self.T // 4), Guarded(c, self.rows), Guarded(c, self.rows)
        self.level = Guarded(c, self.rows * self.T) if call.use_level else None

    def struct(self, **kw):
        call = self.call
        v = {"k": call.k, "n_seqs": len(call.seq_len), "seq_stride": call.seq_stride, "target_stride": self.T, "flags": call.flags, "quant": call.quant,
             "seq": self.seq.data_ptr(), "seq_len": self.seq_len.data_ptr(), "model": self.model.data_ptr()}
        v.update(kw)
        return _lib.GpuSquiggle(v["k"], v["n_seqs"], v["seq_stride"], v["target_stride"], v["flags"], v["quant"], v["seq"], v["seq_len"], v["model"])

    def run(self, c, sq="ok", **ptr):
        p = {"target": self.target.ptr(), "target_len": self.target_len.ptr(), "masked": self.masked.ptr(), "level": self.level.ptr() if self.level else None}
        p.update(ptr)
        s = self.struct() if isinstance(sq, str) else sq
        rc = c.L.vbz_gpu_squiggle_batch(c.ctx, ctypes.byref(s) if s is not None else None, p["target"], p["target_len"], p["masked"], p["level"])
        return rc, c.L.vbz_gpu_last_error(c.ctx).decode()

    def read(self):
        level = self.level.read("level").reshape(self.rows, self.T) if self.level else None
        return (self.target.read("target").view(np.int8).reshape(self.rows, self.T), self.target_len.read("target_len"), self.masked.read("masked"), level)

    def untouched(self):
        return all(a.untouched() for a in (self.target, self.target_len, self.masked, self.level) if a is not None)


def stage_squiggle(c, call):
    t = SquiggleTables(c, call)
    torch.cuda.synchronize()
    rc, msg = t.run(c)
    c.synchronize()
    assert rc == 0, msg
    return t.read()


def assert_squiggle(got, want, call):
    for name, g, w in zip(("target", "target_len", "masked", "level"), got, want):
        if g is None:
            continue
        bad = np.argwhere(g != w)
        assert bad.size == 0, (call.name, name, len(bad), bad[:6].tolist(), [int(g[tuple(b)]) for b in bad[:6]], [int(w[tuple(b)]) for b in bad[:6]],
                               call.seq_len.tolist()[:8])


class FitTables:
    """the device tables and guarded arenas of one squiggle_ref.FitCall"""

    def __init__(self, c, call):
        pairs, hit, n_levels, levels, self.n_reads, prior = call.arrays()
        self.call, self.P = call, len(pairs)
        self.pairs, self.hit, self.n_levels, self.levels = dev_u32(c, pairs), dev_u32(c, hit), dev_u32(c, n_levels), dev_u32(c, levels)
        self.prior = dev_u32(c, prior) if prior is not None else None
        self.target, self.target_len = dev_bytes(c, call.target), dev_u32(c, call.target_len)
        self.out, self.offset, self.scale = Guarded(c, 4 * self.P), Guarded(c, self.P), Guarded(c, self.P)
        self.sums = Guarded(c, 8 * self.P) if call.use_sums else None

    def locate(self, **kw):
        call = self.call
        v = {"query_len": 8, "n_targets": len(call.target_len), "target_stride": call.target.shape[1], "flags": 0, "quant": call.quant, "reserved": 0,
             "target": self.target.data_ptr(), "target_len": self.target_len.data_ptr()}
        v.update(kw)
        g = _lib.GpuLocate()
        for k, x in v.items():
            setattr(g, k, x)
        return g

    def run(self, c, n_pairs=None, n_reads=None, locate="ok", fit="ok", **ptr):
        p = {"pairs": self.pairs.data_ptr(), "hit": self.hit.data_ptr(), "n_levels": self.n_levels.data_ptr(), "levels": self.levels.data_ptr(),
             "prior": self.prior.data_ptr() if self.prior is not None else None, "out": self.out.ptr(), "offset": self.offset.ptr(), "scale": self.scale.ptr(),
             "sums": self.sums.ptr() if self.sums else None}
        p.update(ptr)
        loc = self.locate() if isinstance(locate, str) else locate
        f = _lib.GpuLevelsFit(self.call.W, self.call.min_samples, self.call.max_entries, 0) if isinstance(fit, str) else fit
        rc = c.L.vbz_gpu_levels_fit_batch(c.ctx, self.P if n_pairs is None else n_pairs, self.n_reads if n_reads is None else n_reads,
                                          ctypes.byref(loc) if loc is not None else None, p["pairs"], p["hit"], p["n_levels"], p["levels"],
                                          ctypes.byref(f) if f is not None else None, p["prior"], p["out"], p["offset"], p["scale"], p["sums"])
        return rc, c.L.vbz_gpu_last_error(c.ctx).decode()

    def read(self):
        sums = self.sums.read("sums").view(np.int64).reshape(self.P, 4) if self.sums else None
        return self.out.read("out").reshape(self.P, 4), self.offset.read("offset"), self.scale.read("scale"), sums

    def untouched(self):
        return all(a.untouched() for a in (self.out, self.offset, self.scale, self.sums) if a is not None)


def stage_fit(c, call):
    t = FitTables(c, call)
    torch.cuda.synchronize()
    rc, msg = t.run(c)
    c.synchronize()
    assert rc == 0, msg
    return t.read()


def assert_fit(got, want, call):
    out, offset, scale, sums = got
    want_out, want_sums = want
    bad = np.flatnonzero((out != want_out).any(axis=1))
    assert bad.size == 0, (call.name, "out of pairs", bad[:6].tolist(), "got", out[bad[:4]].tolist(), "want", want_out[bad[:4]].tolist())
    assert (offset == want_out[:, 0]).all() and (scale == want_out[:, 1]).all(), (call.name, "offset / scale repeat the record's floats")
    if sums is not None:
        bad = np.flatnonzero((sums != want_sums).any(axis=1))
        assert bad.size == 0, (call.name, "sums of pairs", bad[:6].tolist(), "got", sums[bad[:4]].tolist(), "want", want_sums[bad[:4]].tolist())

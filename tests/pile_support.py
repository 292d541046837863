"""The raw pile-up calls for the tests on the MI355X (test_gpu_levels_pile, test_gpu_squiggle_kmers, test_gpu_pile_kmers,
test_gpu_model_update, test_gpu_pile_refusals): one call of pile_ref's catalogues into arenas with canary words in front of and behind
each, and its check against the numpy statement bit for bit.  A plain module: every assert carries its operands."""
import ctypes

import numpy as np
import torch

from eventalign_support import GUARD, Guarded, dev_u32, dev_u64
from squiggle_support import dev_bytes
from vbz_compression_amd import _lib


class GuardedPile(Guarded):
    """a pile of n_cells cells between two guards; `before`: what it holds in front of the call (None: zeros)"""

    def __init__(self, c, n_cells, before=None):
        super().__init__(c, 8 * n_cells)
        self.n_cells = n_cells
        held = np.zeros((4, n_cells), np.uint64) if before is None else np.asarray(before, np.uint64).reshape(4, n_cells)
        self.before = held.copy()
        self.t[GUARD:GUARD + self.words] = torch.from_numpy(held.reshape(-1).view(np.int32).copy()).to(c.device)

    def read(self, what):
        return super().read(what).copy().view(np.uint64).reshape(4, self.n_cells)

    def untouched(self):
        got = self.t.cpu().numpy().view(np.uint32)
        return bool((got[GUARD:GUARD + self.words].view(np.uint64).reshape(4, self.n_cells) == self.before).all()) and self.read("the pile") is not None


def assert_pile(got, want, name):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (name, "plane, cell", len(bad), bad[:6].tolist(), [hex(int(got[tuple(b)])) for b in bad[:6]], [hex(int(want[tuple(b)])) for b in bad[:6]])


# ---- vbz_gpu_levels_pile_batch ----------------------------------------------------------------------------------------------------------
class PileTables:
    """the device tables and the guarded arena of one pile_ref.PileCall"""

    def __init__(self, c, call, pile=None):
        pairs, hit, n_levels, levels, self.n_reads, fit = call.arrays()
        self.call, self.P = call, len(pairs)
        self.pairs, self.hit, self.n_levels, self.levels = dev_u32(c, pairs), dev_u32(c, hit), dev_u32(c, n_levels), dev_u32(c, levels)
        self.fit = dev_u32(c, fit) if fit is not None else None
        self.target = dev_bytes(c, np.zeros((len(call.target_len), call.T), np.int8))
        self.target_len = dev_u32(c, call.target_len)
        self.pile = pile if pile is not None else GuardedPile(c, call.n_cells, call.before)

    def locate(self, **kw):
        call = self.call
        v = {"query_len": 8, "n_targets": len(call.target_len), "target_stride": call.T, "flags": 0, "quant": 32.0, "reserved": 0,
             "target": self.target.data_ptr(), "target_len": self.target_len.data_ptr()}
        v.update(kw)
        g = _lib.GpuLocate()
        for k, x in v.items():
            setattr(g, k, x)
        return g

    def params(self, **kw):
        call = self.call
        v = {"max_width": call.W, "min_samples": call.min_samples, "max_entries": call.max_entries, "flags": call.flags, "fix": call.fix, "reserved0": 0,
             "reserved1": 0, "reserved2": 0}
        v.update(kw)
        return _lib.GpuLevelsPile(*[v[f] for f, _ in _lib.GpuLevelsPile._fields_])

    def run(self, c, n_pairs=None, n_reads=None, locate="ok", params="ok", **ptr):
        p = {"pairs": self.pairs.data_ptr(), "hit": self.hit.data_ptr(), "n_levels": self.n_levels.data_ptr(), "levels": self.levels.data_ptr(),
             "fit": self.fit.data_ptr() if self.fit is not None else None, "pile": self.pile.ptr()}
        p.update(ptr)
        loc = self.locate() if isinstance(locate, str) else locate
        par = self.params() if isinstance(params, str) else params
        rc = c.L.vbz_gpu_levels_pile_batch(c.ctx, self.P if n_pairs is None else n_pairs, self.n_reads if n_reads is None else n_reads,
                                           ctypes.byref(loc) if loc is not None else None, p["pairs"], p["hit"], p["n_levels"], p["levels"],
                                           ctypes.byref(par) if par is not None else None, p["fit"], p["pile"])
        return rc, c.L.vbz_gpu_last_error(c.ctx).decode()


def stage_pile(c, call, pile=None):
    """one call -> the arena uint64 [4, n_cells] (the words around it checked)"""
    t = PileTables(c, call, pile)
    torch.cuda.synchronize()
    rc, msg = t.run(c)
    c.synchronize()
    assert rc == 0, msg
    return t.pile.read("the pile")


# ---- vbz_gpu_squiggle_kmers_batch -------------------------------------------------------------------------------------------------------
class KmersTables:
    """the device tables and guarded arenas of one squiggle_ref.SquiggleCall, for the kmers call"""

    def __init__(self, c, call):
        self.call, self.rows, self.T = call, call.rows, call.target_stride
        self.seq, self.seq_len = dev_bytes(c, call.seq), dev_u32(c, call.seq_len)
        self.kmer, self.target_len = Guarded(c, self.rows * self.T), Guarded(c, self.rows)

    def struct(self, **kw):
        call = self.call
        v = {"k": call.k, "n_seqs": len(call.seq_len), "seq_stride": call.seq_stride, "target_stride": self.T, "flags": call.flags, "quant": call.quant,
             "seq": self.seq.data_ptr(), "seq_len": self.seq_len.data_ptr(), "model": None}
        v.update(kw)
        return _lib.GpuSquiggle(*[v[f] for f, _ in _lib.GpuSquiggle._fields_])

    def run(self, c, sq="ok", **ptr):
        p = {"kmer": self.kmer.ptr(), "target_len": self.target_len.ptr()}
        p.update(ptr)
        s = self.struct() if isinstance(sq, str) else sq
        rc = c.L.vbz_gpu_squiggle_kmers_batch(c.ctx, ctypes.byref(s) if s is not None else None, p["kmer"], p["target_len"])
        return rc, c.L.vbz_gpu_last_error(c.ctx).decode()

    def read(self):
        return self.kmer.read("kmer").reshape(self.rows, self.T), self.target_len.read("target_len")

    def untouched(self):
        return self.kmer.untouched() and self.target_len.untouched()


def stage_kmers(c, call):
    t = KmersTables(c, call)
    torch.cuda.synchronize()
    rc, msg = t.run(c)
    c.synchronize()
    assert rc == 0, msg
    return t.read()


# ---- vbz_gpu_pile_kmers_batch -----------------------------------------------------------------------------------------------------------
class KmersPileTables:
    """the device tables and the guarded k-mer arena of one pile_ref.KmersPileCall"""

    def __init__(self, c, call):
        self.call, (self.rows, self.T) = call, call.kmer.shape
        self.kmer, self.target_len, self.pile = dev_u32(c, call.kmer), dev_u32(c, call.target_len), dev_u64(c, call.pile)
        self.kmer_pile = GuardedPile(c, 4 ** call.k, call.before)

    def params(self, **kw):
        v = {"k": self.call.k, "rows": self.rows, "target_stride": self.T, "flags": self.call.flags}
        v.update(kw)
        return _lib.GpuPileKmers(v["k"], v["rows"], v["target_stride"], v["flags"])

    def run(self, c, params="ok", **ptr):
        p = {"target_len": self.target_len.data_ptr(), "kmer": self.kmer.data_ptr(), "pile": self.pile.data_ptr(), "kmer_pile": self.kmer_pile.ptr()}
        p.update(ptr)
        par = self.params() if isinstance(params, str) else params
        rc = c.L.vbz_gpu_pile_kmers_batch(c.ctx, ctypes.byref(par) if par is not None else None, p["target_len"], p["kmer"], p["pile"], p["kmer_pile"])
        return rc, c.L.vbz_gpu_last_error(c.ctx).decode()


def stage_pile_kmers(c, call):
    t = KmersPileTables(c, call)
    torch.cuda.synchronize()
    rc, msg = t.run(c)
    c.synchronize()
    assert rc == 0, msg
    return t.kmer_pile.read("the k-mer pile")


# ---- vbz_gpu_model_update_batch ---------------------------------------------------------------------------------------------------------
class UpdateTables:
    """the device tables and guarded arenas of one pile_ref.UpdateCall; in place: the model arena holds the prior"""

    def __init__(self, c, call):
        self.call, self.cells = call, 4 ** call.k
        self.kmer_pile = dev_u64(c, call.kmer_pile)
        self.model, self.sd = Guarded(c, self.cells), Guarded(c, self.cells) if call.use_sd else None
        self.prior = dev_u32(c, call.prior)
        if call.in_place:
            self.model.t[GUARD:GUARD + self.cells] = self.prior

    def params(self, **kw):
        v = {"k": self.call.k, "min_obs": self.call.min_obs, "flags": 0, "fix": self.call.fix}
        v.update(kw)
        return _lib.GpuModelUpdate(v["k"], v["min_obs"], v["flags"], v["fix"])

    def run(self, c, params="ok", **ptr):
        p = {"kmer_pile": self.kmer_pile.data_ptr(), "prior": self.model.ptr() if self.call.in_place else self.prior.data_ptr(), "model": self.model.ptr(),
             "sd": self.sd.ptr() if self.sd else None}
        p.update(ptr)
        par = self.params() if isinstance(params, str) else params
        rc = c.L.vbz_gpu_model_update_batch(c.ctx, ctypes.byref(par) if par is not None else None, p["kmer_pile"], p["prior"], p["model"], p["sd"])
        return rc, c.L.vbz_gpu_last_error(c.ctx).decode()

    def read(self):
        return self.model.read("model"), self.sd.read("sd") if self.sd else None

    def untouched(self):
        return self.model.untouched() and (self.sd is None or self.sd.untouched())


def stage_update(c, call):
    t = UpdateTables(c, call)
    torch.cuda.synchronize()
    rc, msg = t.run(c)
    c.synchronize()
    assert rc == 0, msg
    return t.read()
